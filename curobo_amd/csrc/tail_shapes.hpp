// tail_shapes.hpp -- compile-time shapes of the one-launch L-BFGS iteration tail (optimization.hip), after fused_shapes.hpp.
//
// The run-time kernels read opt_dim, the history length, the candidate count and action_dim from their arguments: every
// unrolled history slot then carries a compare and a branch, the history arrays are sized for the largest history (32 slots,
// 16 in the row form) and `v % action_dim` is a division.  A TailShape fixes the four as template values on the same source:
// the slot loops become straight-line code over exactly m slots.  The host takes a shape only when EVERY dimension equals
// the shape's (curobo_hip_lbfgs_tail_shape_id); anything else runs the run-time kernels, so a stale table costs speed,
// never correctness.  tests/test_tail_shape_table.py holds the table to the packaged Franka and the solver configurations.
//
//           V = opt_dim, M = history length, NLS = line-search candidates, AD = action_dim
#pragma once

namespace curobo_hip {

struct TailShapeDyn {
  static constexpr bool kStatic = false;
  static constexpr int kV = 0, kM = 0, kNLS = 0, kAD = 0;
};

template <int V_, int M_, int NLS_, int AD_>
struct TailShape {
  static constexpr bool kStatic = true;
  static constexpr int kV = V_, kM = M_, kNLS = NLS_, kAD = AD_;
};

}  // namespace curobo_hip

//                                     V   M NLS AD
// 1: trajectory optimisation of a 7-dof arm, 12 knots (BASELINE C2: Franka, history 27, four candidates); held by the
//    wavefront form (between the seed shards) and the workgroup form (single stream)
#define CUROBO_TAIL_SHAPE_1 TailShape<84, 27, 4, 7>
// 2: inverse kinematics of a 7-dof arm (solver/ik.py: history 7, four candidates); held by the 16-lane row form
#define CUROBO_TAIL_SHAPE_2 TailShape<7, 7, 4, 7>
#define CUROBO_TAIL_NUM_SHAPES 2
