// rollout_fused.hip -- host side of the fused trajectory rollout launch (kernel and device machinery: fused_device.hpp):
// process-wide state (profile hooks, run-time shape table), LDS layout / workgroup size resolution, the dispatch cascade
// (run-time shapes, the compile-time shapes of rollout_fused_shape.hip, then the generic instantiations, which this unit
// holds), the C ABI of the trajectory launches, the longest-first dispatch workspace and the lane-list builder.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <vector>

#include "fused_device.hpp"

using namespace curobo_hip;

static long long *g_fused_prof = nullptr;
static bool g_fused_shapes_enabled = true;
// shapes compiled at run time (curobo_fused_jit_launch of their objects), tried before the built-in table
typedef int (*fused_jit_launcher_t)(const void *, int, int, int, int, int, int, size_t, void *, int *);
// A fixed table with an atomic count: ctypes releases the GIL around the entry points, so one thread may register a shape
// while another launches -- a launch reads the count once (acquire) and only the slots below it, a registration writes its slot
// before it publishes the count (release) under a lock that serialises writers (the std::vector here could be
// reallocated under a reader).
constexpr int kMaxJitShapes = 64;
static fused_jit_launcher_t g_jit_shapes[kMaxJitShapes];
static std::atomic<int> g_jit_shape_count{0};
static std::mutex g_jit_shape_lock;
struct JitShapeView {
  int n;
  const fused_jit_launcher_t *begin() const { return g_jit_shapes; }
  const fused_jit_launcher_t *end() const { return g_jit_shapes + n; }
  size_t size() const { return (size_t)n; }
  fused_jit_launcher_t operator[](size_t i) const { return g_jit_shapes[i]; }
};
static JitShapeView fused_jit_shapes() { return JitShapeView{g_jit_shape_count.load(std::memory_order_acquire)}; }
constexpr int kJitShapeIdBase = 100;
CUROBO_EXPORT int curobo_hip_rollout_fused_register_shape(void *launcher, int args_bytes) {
  CUROBO_REQUIRE(launcher != nullptr, "rollout_fused_register_shape: NULL launcher%s", "");
  CUROBO_REQUIRE(args_bytes == (int)sizeof(FusedTrajArgs),
                 "rollout_fused_register_shape: the shape object was built for an argument block of %d bytes, this library's is %d "
                 "(compile it from this library's sources)", args_bytes, (int)sizeof(FusedTrajArgs));
  std::lock_guard<std::mutex> guard(g_jit_shape_lock);
  const int n = g_jit_shape_count.load(std::memory_order_relaxed);
  for (int i = 0; i < n; i++)
    if ((void *)g_jit_shapes[i] == launcher) return CUROBO_HIP_OK;
  CUROBO_REQUIRE(n < kMaxJitShapes, "rollout_fused_register_shape: more than %d run-time shapes", kMaxJitShapes);
  g_jit_shapes[n] = reinterpret_cast<fused_jit_launcher_t>(launcher);
  g_jit_shape_count.store(n + 1, std::memory_order_release);
  return CUROBO_HIP_OK;
}
CUROBO_EXPORT int curobo_hip_rollout_fused_set_shapes_enabled(int enabled) {
  g_fused_shapes_enabled = enabled != 0;
  return CUROBO_HIP_OK;
}

// development hook (not part of the drop-in surface): device buffer [batch][8] of int64 that
// receives 100 MHz wall-clock stamps at the phase boundaries of every fused launch; NULL = off
CUROBO_EXPORT int curobo_hip_rollout_fused_set_profile_buffer(int64_t *device_buffer) {
  g_fused_prof = (long long *)device_buffer;
  return CUROBO_HIP_OK;
}

// Same hook for a SEQUENCE of launches (e.g. the launches recorded into a hipGraph): launch k after
// this call stamps into block k = device_buffer + k * block_rows * 16 (launches beyond n_blocks, or
// with more than block_rows trajectories, are not stamped).  NULL / 0 ends the sequence.
static long long *g_fused_prof_seq = nullptr;
static int g_fused_prof_blocks = 0, g_fused_prof_rows = 0, g_fused_prof_next = 0;
CUROBO_EXPORT int curobo_hip_rollout_fused_set_profile_sequence(int64_t *device_buffer, int n_blocks, int block_rows) {
  g_fused_prof_seq = (long long *)device_buffer;
  g_fused_prof_blocks = device_buffer ? n_blocks : 0;
  g_fused_prof_rows = block_rows;
  g_fused_prof_next = 0;
  return CUROBO_HIP_OK;
}

// workgroup size and LDS layout of the trajectory kernels (the layout depends on the number of waves
// through the per-wave scene lists): 8 waves when two workgroups then fit in a CU's LDS, see the
// kernel's header; else one row per point up to 16 waves
static FusedLayout trajectory_launch_shape(int H, int D, int L, int S, int C, int P, int n_rec, int n_dyn, int *threads_out,
                                           int rings = 1, int n_lane = 0) {
  int threads = ((H * kFkLanes + 63) / 64) * 64;
  if (threads > 1024) threads = 1024;
  if (threads > 512 && (size_t)fused_layout(H, D, L, S, C, P, n_rec, n_dyn, 8, rings, n_lane).total * sizeof(float) <= 80 * 1024) threads = 512;
  static const int force_threads = [] { const char *e = getenv("CUROBO_HIP_FUSED_THREADS"); return e ? atoi(e) : 0; }();
  if (force_threads >= 64 && force_threads <= 1024) threads = force_threads & ~63;  // tuning knob
  *threads_out = threads;
  return fused_layout(H, D, L, S, C, P, n_rec, n_dyn, threads >> 6, rings, n_lane);
}

CUROBO_EXPORT int curobo_hip_rollout_trajectory_fused_lds_bytes(int padded_horizon, int dof, int num_links,
                                                                   int num_spheres, int num_collision_pairs,
                                                                   int link_chain_len, int num_obstacles) {
  int threads;
  const FusedLayout lay = trajectory_launch_shape(padded_horizon, dof, num_links, num_spheres, link_chain_len,
                                                  num_collision_pairs, num_obstacles, 0, &threads, 2);
  return lay.total * (int)sizeof(float);
}

// layout and workgroup size of a launch; drops the lane form of the pair pass (a.lane_lists) where it would cost a workgroup slot
static FusedLayout fused_resolve_layout(FusedTrajArgs &a, int n_rec, bool with_terms, int *threads_out) {
  const int H = a.bs.padded_horizon, D = a.bs.dof, L = a.nlinks, S = a.nspheres, C = a.chain_len, P = a.npairs;
  const int n_dyn = a.use_cspace ? 4 * H * D : 0, rings = with_terms ? 1 : 2;
  int threads;
  FusedLayout lay = trajectory_launch_shape(H, D, L, S, C, P, n_rec, n_dyn, &threads, rings, a.lane_lists ? (a.lane_len0 + a.lane_len1) * 64 : 0);
  if (a.lane_lists) {
    // the lane form must not cost a workgroup slot: where its lists (64 words per entry, whatever the sphere count) push
    // the trajectory over 160 KB, or over the 80 KB that let two workgroups share a CU, the pass walks pair_locations
    int threads0;
    const FusedLayout lay0 = trajectory_launch_shape(H, D, L, S, C, P, n_rec, n_dyn, &threads0, rings, 0);
    const size_t l1 = (size_t)lay.total * sizeof(float), l0 = (size_t)lay0.total * sizeof(float);
    if (l1 > 160 * 1024 || (l1 > 80 * 1024 && l0 <= 80 * 1024) || (a.use_torque && !fused_torque_fits(lay, H, D, L, S))) {
      a.lane_lists = nullptr; a.lane_len0 = 0; a.lane_len1 = 0;
      lay = lay0;
      threads = threads0;
    }
  }
  *threads_out = threads;
  return lay;
}

// workgroup size a launch with these dimensions uses (a compile-time shape holds it as a constant).  Returns the thread count.
CUROBO_EXPORT int curobo_hip_rollout_fused_threads(int padded_horizon, int dof, int num_links, int num_spheres, int num_collision_pairs,
                                                   int link_chain_len, int self_lane_len, int num_obstacles, int with_trajopt_terms) {
  FusedTrajArgs a{};
  a.bs.padded_horizon = padded_horizon; a.bs.dof = dof; a.nlinks = num_links; a.nspheres = num_spheres; a.npairs = num_collision_pairs;
  a.chain_len = link_chain_len; a.lane_len0 = self_lane_len & 0xffff; a.lane_len1 = (self_lane_len >> 16) & 0xffff;
  static const uint32_t some_list = 0u;
  a.lane_lists = self_lane_len ? &some_list : nullptr;
  a.use_cspace = with_trajopt_terms ? 1 : 0;
  int threads = 0;
  (void)fused_resolve_layout(a, num_obstacles, with_trajopt_terms != 0, &threads);
  return threads;
}

CUROBO_EXPORT int curobo_hip_rollout_fused_shape_id(int padded_horizon, int n_knots, int dof, int num_links, int num_spheres,
                                                    int num_collision_pairs, int link_chain_len, int self_lane_len, int max_cuboids,
                                                    int max_voxel_grids, int bspline_degree, int sweep_steps, int kinds,
                                                    int with_trajopt_terms, int plain_launch) {
  FusedTrajArgs a{};
  a.bs.padded_horizon = padded_horizon; a.bs.n_knots = n_knots; a.bs.dof = dof; a.nlinks = num_links; a.nspheres = num_spheres;
  a.npairs = num_collision_pairs; a.chain_len = link_chain_len; a.sc.max_cuboids = max_cuboids; a.sc.max_voxel_grids = max_voxel_grids;
  a.lane_len0 = self_lane_len & 0xffff; a.lane_len1 = (self_lane_len >> 16) & 0xffff;
  static const uint32_t some_list = 0u;
  static const float some_float = 0.0f;
  static int32_t some_ws = 0;
  a.lane_lists = self_lane_len ? &some_list : nullptr;
  if (plain_launch) {  // self + scene collision with the speed metric, one environment, longest-first dispatch, nothing materialised
    a.use_self = 1; a.use_scene = 1; a.enable_speed_metric = 1; a.num_envs = 1; a.dispatch_ws = &some_ws; a.sphere_padding = &some_float;
  }
  a.use_cspace = with_trajopt_terms ? 1 : 0;
  a.use_pose = (with_trajopt_terms && plain_launch) ? 1 : 0;  // (plain + terms = a trajectory-optimisation iteration: pose + c-space STATE)
  int threads;
  (void)fused_resolve_layout(a, max_cuboids + max_voxel_grids, with_trajopt_terms != 0, &threads);
  {
    const JitShapeView v = fused_jit_shapes();
    for (size_t i = 0; i < v.size(); i++) {
      int e2 = 0;
      if (v[i](&a, bspline_degree, sweep_steps, kinds, with_trajopt_terms != 0 ? 1 : 0, 0, threads, 0, nullptr, &e2)) return kJitShapeIdBase + (int)i;
    }
  }
  hipError_t e = hipSuccess;
#define CUROBO_FUSED_QUERY_SHAPE(ID) \
  if (fused_shape_launch_##ID(a, bspline_degree, sweep_steps, kinds, with_trajopt_terms != 0, 0, threads, 0, nullptr, &e)) return ID;
  CUROBO_FUSED_FOR_EACH_SHAPE(CUROBO_FUSED_QUERY_SHAPE)
#undef CUROBO_FUSED_QUERY_SHAPE
  return 0;
}

// the optional reuse arguments of the *_reuse entry points (FusedTrajArgs::memo_*); all NULL = every trajectory is evaluated
struct FusedReuse {
  const float *x, *cost, *grad;
  int stride, slot;
};

static int rollout_trajectory_fused_impl(
    const char *what, const curobo_hip_trajopt_terms *terms,
    float *out_cost, float *out_grad_knots, float *out_position, float *out_robot_spheres, const float *u_position,
    const float *start_position, const float *start_velocity, const float *start_acceleration, const float *start_jerk,
    const float *goal_position, const float *goal_velocity, const float *goal_acceleration, const float *goal_jerk,
    const int32_t *start_idx, const int32_t *goal_idx, const float *traj_dt, const uint8_t *use_implicit_goal_state,
    const float *fixed_transform, const float *robot_spheres, const int8_t *joint_map_type, const int16_t *joint_map,
    const int16_t *link_map, const int16_t *link_sphere_map, const int16_t *link_chain_data,
    const int16_t *link_chain_offsets, const float *joint_offset_map, const float *sphere_padding,
    const float *self_collision_weight, const int16_t *pair_locations, const curobo_hip_scene *scene,
    const float *scene_collision_weight, const float *activation_distance, const float *speed_dt,
    const int32_t *env_query_idx, int num_envs, int use_multi_env, int batch_size, int padded_horizon, int dof,
    int n_knots, int bspline_degree, int num_links, int num_spheres, int num_collision_pairs, int link_chain_len,
    int sweep_steps, int enable_speed_metric, int32_t *dispatch_ws, int dispatch_phase, const uint32_t *self_lane_lists,
    int self_lane_len, const FusedReuse &reuse, curobo_hip_stream_t stream) {
  CUROBO_REQUIRE(bspline_degree >= 3 && bspline_degree <= 5, "%s: bspline_degree must be 3, 4 or 5", what);
  CUROBO_REQUIRE(sweep_steps == 0 || sweep_steps == 3, "%s: sweep_steps must be 0 or 3", what);
  if (const int bad = fused_check_dimensions(what, num_links, num_spheres, link_chain_len, pair_locations)) return bad;
  CUROBO_REQUIRE(dof >= 1 && padded_horizon >= 2 && n_knots >= 1, "%s: bad dimensions", what);
  const bool any_memo = reuse.x || reuse.cost || reuse.grad;
  if (any_memo) {
    CUROBO_REQUIRE(reuse.x && reuse.cost && reuse.grad, "%s: memo_x, memo_cost and memo_grad must be given together (all three or none)", what);
    CUROBO_REQUIRE(reuse.stride >= 1, "%s: memo_stride must be >= 1", what);
    CUROBO_REQUIRE(reuse.slot >= 0 && reuse.slot < reuse.stride, "%s: memo_slot must be in [0, memo_stride)", what);
    CUROBO_REQUIRE(batch_size % reuse.stride == 0, "%s: batch_size must be a multiple of memo_stride", what);
    // a copied row has no positions, spheres or per-term values to write
    const bool term_outputs = terms && (terms->out_pose_distance || terms->out_position_distance || terms->out_rotation_distance ||
                                        terms->out_goalset_idx || terms->out_cspace_cost);
    CUROBO_REQUIRE(!out_position && !out_robot_spheres && !term_outputs,
                   "%s: reuse (memo_x) with materialised outputs (out_position, out_robot_spheres, per-term outputs)", what);
  }
  if (batch_size == 0) return CUROBO_HIP_OK;
  FusedTrajArgs a{};
  a.out_cost = out_cost; a.out_grad_knots = out_grad_knots; a.out_position = out_position;
  a.out_spheres = out_robot_spheres;
  a.bs.u = u_position;
  a.bs.start[0] = start_position; a.bs.start[1] = start_velocity; a.bs.start[2] = start_acceleration; a.bs.start[3] = start_jerk;
  a.bs.goal[0] = goal_position; a.bs.goal[1] = goal_velocity; a.bs.goal[2] = goal_acceleration; a.bs.goal[3] = goal_jerk;
  a.bs.start_idx = start_idx; a.bs.goal_idx = goal_idx; a.bs.traj_dt = traj_dt; a.bs.use_implicit_goal = use_implicit_goal_state;
  a.bs.batch = batch_size; a.bs.padded_horizon = padded_horizon; a.bs.dof = dof; a.bs.n_knots = n_knots;
  fused_fill_robot_args(a, true, fixed_transform, robot_spheres, joint_map_type, joint_map, link_map, link_sphere_map, link_chain_data,
                        link_chain_offsets, joint_offset_map, sphere_padding, self_collision_weight, pair_locations, scene,
                        scene_collision_weight, activation_distance, env_query_idx, num_envs, use_multi_env, batch_size, dof, num_links,
                        num_spheres, num_collision_pairs, link_chain_len);
  a.speed_dt = speed_dt; a.dpad = dof | 1;
  a.enable_speed_metric = (a.use_scene && enable_speed_metric) ? 1 : 0;
  a.prof = g_fused_prof;
  if (g_fused_prof_seq && g_fused_prof_next < g_fused_prof_blocks && batch_size <= g_fused_prof_rows)
    a.prof = g_fused_prof_seq + (size_t)g_fused_prof_next++ * g_fused_prof_rows * 16;
  a.dispatch_ws = dispatch_ws; a.dispatch_phase = dispatch_phase;
  if (any_memo) { a.memo_x = reuse.x; a.memo_cost = reuse.cost; a.memo_grad = reuse.grad; a.memo_stride = reuse.stride; a.memo_slot = reuse.slot; }
  static const bool no_lanes = getenv("CUROBO_HIP_SELF_ROWS") != nullptr;  // development knob: the row form of the pair pass
  if (self_lane_lists && a.use_self && !no_lanes) {
    a.lane_lists = self_lane_lists; a.lane_len0 = self_lane_len & 0xffff; a.lane_len1 = (self_lane_len >> 16) & 0xffff;
    CUROBO_REQUIRE(a.lane_len0 + a.lane_len1 > 0 && num_spheres <= 128 && num_collision_pairs < 65535,
                   "%s: self_lane_lists does not describe this robot (curobo_hip_self_lane_lists_host)", what);
  }
  static const int scene_rows = [] { const char *e = getenv("CUROBO_HIP_SCENE_ROWS"); return e ? atoi(e) : 0; }();
  a.scene_rows = scene_rows;
  CUROBO_REQUIRE(!dispatch_ws || dispatch_phase == 0 || dispatch_phase == 1, "%s: dispatch_phase must be 0 or 1", what);
  CUROBO_REQUIRE(!a.enable_speed_metric || speed_dt, "%s: speed metric needs speed_dt", what);
  const int n_rec = a.sc.max_cuboids + a.sc.max_voxel_grids;
  if (terms) {
    const curobo_hip_trajopt_terms &t = *terms;
    a.use_pose = (t.n_tool_frames > 0 && t.goal_position) ? 1 : 0;
    a.use_cspace = t.cspace_weight ? 1 : 0;
    // development knob (timing by elimination): CUROBO_HIP_TERMS_MASK bit 0 = tool pose, bit 1 = c-space STATE
    static const int terms_mask = [] { const char *e = getenv("CUROBO_HIP_TERMS_MASK"); return e ? atoi(e) : 3; }();
    if (!(terms_mask & 1)) a.use_pose = 0;
    if (!(terms_mask & 2)) a.use_cspace = 0;
    if (a.use_pose) {
      CUROBO_REQUIRE(t.tool_frame_map && t.goal_quat && t.idxs_goal && t.position_orientation_weight &&
                         t.terminal_pose_axes_weight_factor && t.non_terminal_pose_axes_weight_factor &&
                         t.terminal_pose_convergence_tolerance && t.non_terminal_pose_convergence_tolerance &&
                         t.project_distance_to_goal && t.num_goalset >= 1,
                     "%s: incomplete tool-pose terms", what);
      CUROBO_REQUIRE(t.rotation_method >= 0 && t.rotation_method <= 2, "%s: rotation_method must be 0, 1 or 2", what);
      ToolPoseArgs &tp = a.tp;
      tp.out_distance = t.out_pose_distance; tp.out_position_distance = t.out_position_distance;
      tp.out_rotation_distance = t.out_rotation_distance; tp.out_goalset_idx = t.out_goalset_idx;
      tp.goal_position = t.goal_position; tp.goal_quat = t.goal_quat; tp.idxs_goal = t.idxs_goal;
      tp.position_orientation_weight = t.position_orientation_weight;
      tp.terminal_axes_weight = t.terminal_pose_axes_weight_factor;
      tp.non_terminal_axes_weight = t.non_terminal_pose_axes_weight_factor;
      tp.terminal_tolerance = t.terminal_pose_convergence_tolerance;
      tp.non_terminal_tolerance = t.non_terminal_pose_convergence_tolerance;
      tp.project_distance_to_goal = t.project_distance_to_goal;
      tp.batch = batch_size; tp.horizon = padded_horizon; tp.num_links = t.n_tool_frames; tp.num_goalset = t.num_goalset;
      tp.rotation_method = t.rotation_method;
      a.tool_frame_map = t.tool_frame_map; a.n_tool_frames = t.n_tool_frames;
    }
    if (a.use_cspace) {
      CUROBO_REQUIRE(t.state_dt && t.p_b && t.v_b && t.a_b && t.j_b && t.effort_b && t.cspace_activation_distance &&
                         t.squared_l2_regularization_weights && t.cspace_target_weight &&
                         t.cspace_non_terminal_weight_factor && t.cspace_target_dof_weight && t.target_joint_position &&
                         t.idxs_target_joint_position,
                     "%s: incomplete c-space terms", what);
      CUROBO_REQUIRE(dof <= 64, "%s: c-space term supports dof <= 64", what);
      CspaceStateArgs &cs = a.cs;
      cs.out_cost = t.out_cspace_cost; cs.state_dt = t.state_dt; cs.target = t.target_joint_position;
      cs.idxs_target = t.idxs_target_joint_position; cs.p_b = t.p_b; cs.v_b = t.v_b; cs.a_b = t.a_b; cs.j_b = t.j_b;
      cs.effort_b = t.effort_b; cs.weight = t.cspace_weight; cs.activation_distance = t.cspace_activation_distance;
      cs.sql2_weights = t.squared_l2_regularization_weights; cs.target_weight = t.cspace_target_weight;
      cs.non_terminal_factor = t.cspace_non_terminal_weight_factor; cs.target_dof_weight = t.cspace_target_dof_weight;
      cs.write_grad = 1; cs.batch = batch_size; cs.horizon = padded_horizon; cs.dof = dof;
      cs.retime_weights = t.retime_weights; cs.retime_reg_weights = t.retime_regularization_weights;
      if (t.use_torque_limits) {
        CUROBO_REQUIRE(t.link_masses_com && t.link_inertias && t.gravity && t.level_links,
                       "%s: torque limits need link_masses_com, link_inertias, gravity, level_links", what);
        a.link_masses_com = t.link_masses_com; a.link_inertias = t.link_inertias; a.gravity = t.gravity;
        a.level_links = t.level_links; a.use_torque = 1;
      }
    }
  }
  int threads;
  static const bool force_terms = getenv("CUROBO_HIP_FORCE_TERMS") != nullptr;
  const bool with_terms = a.use_pose || a.use_cspace || force_terms;  // the TERMS instantiation: one scene ring per wave
  const FusedLayout lay = fused_resolve_layout(a, n_rec, with_terms, &threads);
  const size_t lds = (size_t)lay.total * sizeof(float);
  CUROBO_REQUIRE(lds <= 160 * 1024, "%s: trajectory does not fit in LDS (%zu bytes); use the unfused kernels", what, lds);
  CUROBO_REQUIRE(!a.use_torque || fused_torque_fits(lay, padded_horizon, dof, num_links, num_spheres),
                 "%s: the inverse-dynamics state of this robot does not fit the LDS regions it borrows; run the torque "
                 "limits on the kernel sequence (curobo_hip_rollout_trajopt_fused_torque_fits)", what);
  const int kinds = fused_scene_kinds(a.sc);
  hipStream_t st = (hipStream_t)stream;
  {  // a compile-time shape that matches every dimension of this launch (fused_shapes.hpp), most specific first
    static const bool env_off = getenv("CUROBO_HIP_FUSED_NO_SHAPES") != nullptr;  // development knob: always the generic kernel
    const bool no_shapes = env_off || !g_fused_shapes_enabled;
    hipError_t se = hipSuccess;
    if (!no_shapes) {  // shapes compiled at run time for this robot / horizon
      for (fused_jit_launcher_t fn : fused_jit_shapes()) {
        int e = 0;
        if (fn(&a, bspline_degree, sweep_steps, kinds, with_terms ? 1 : 0, batch_size, threads, lds, (void *)st, &e))
          return fused_launch_status(what, (hipError_t)e, st);
      }
    }
#define CUROBO_FUSED_TRY_SHAPE(ID)                                                                                            \
    if (!no_shapes && fused_shape_launch_##ID(a, bspline_degree, sweep_steps, kinds, with_terms, batch_size, threads, lds, st, &se)) \
      return fused_launch_status(what, se, st);
    CUROBO_FUSED_FOR_EACH_SHAPE(CUROBO_FUSED_TRY_SHAPE)
#undef CUROBO_FUSED_TRY_SHAPE
  }
  // the generic instantiations: one per B-spline degree, sweep and obstacle kinds, with and without the optional terms
  void (*kfn)(const FusedTrajArgs) = nullptr;
#define CUROBO_FUSED_KERNEL_OF(DG, SW, KD) \
  if (bspline_degree == DG && sweep_steps == SW && (kinds ? kinds : 1) == KD) /* (no scene: the cuboid instantiation) */ \
    kfn = with_terms ? rollout_trajectory_fused_kernel<DG, SW, KD, true> : rollout_trajectory_fused_kernel<DG, SW, KD, false>;
#define CUROBO_FUSED_KINDS_OF(DG, SW) \
  CUROBO_FUSED_KERNEL_OF(DG, SW, 1) CUROBO_FUSED_KERNEL_OF(DG, SW, 2) CUROBO_FUSED_KERNEL_OF(DG, SW, 3) CUROBO_FUSED_KERNEL_OF(DG, SW, 7)
  CUROBO_FUSED_KINDS_OF(3, 0) CUROBO_FUSED_KINDS_OF(3, 3) CUROBO_FUSED_KINDS_OF(4, 0) CUROBO_FUSED_KINDS_OF(4, 3)
  CUROBO_FUSED_KINDS_OF(5, 0) CUROBO_FUSED_KINDS_OF(5, 3)
#undef CUROBO_FUSED_KINDS_OF
#undef CUROBO_FUSED_KERNEL_OF
  const hipError_t e = fused_launch(kfn, dim3((unsigned)batch_size), dim3(threads), lds, kFusedLdsUnasked, st, a);
  static const bool dbg = getenv("CUROBO_HIP_FUSED_DEBUG") != nullptr;
  if (dbg && e == hipSuccess) {
    int nb = -1;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)kfn, threads, lds);
    fprintf(stderr, "[curobo_hip] fused: threads %d lds %zu -> %d workgroups/CU\n", threads, lds, nb);
  }
  return fused_launch_status(what, e, st);
}

__global__ void dispatch_ws_init_kernel(int32_t *ws, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) { ws[i] = i; ws[B + i] = i; ws[2 * B + i] = 0; ws[3 * B + i] = 0; }
}

CUROBO_EXPORT int curobo_hip_rollout_dispatch_ws_size(int batch_size) { return batch_size > 0 ? 4 * batch_size : 0; }

CUROBO_EXPORT int curobo_hip_rollout_dispatch_ws_init(int32_t *dispatch_ws, int batch_size, curobo_hip_stream_t stream) {
  CUROBO_REQUIRE(dispatch_ws && batch_size > 0, "rollout_dispatch_ws_init: NULL workspace or empty batch%s", "");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dispatch_ws_init_kernel, dim3((batch_size + 255) / 256), dim3(256), 0, st, dispatch_ws, batch_size);
  return check_launch("rollout_dispatch_ws_init", st);
}

#define CUROBO_TRAJ_PARAMS                                                                                          \
  float *out_cost, float *out_grad_knots, float *out_position, float *out_robot_spheres, const float *u_position,     \
      const float *start_position, const float *start_velocity, const float *start_acceleration,                      \
      const float *start_jerk, const float *goal_position, const float *goal_velocity, const float *goal_acceleration, \
      const float *goal_jerk, const int32_t *start_idx, const int32_t *goal_idx, const float *traj_dt,                \
      const uint8_t *use_implicit_goal_state, const float *fixed_transform, const float *robot_spheres,               \
      const int8_t *joint_map_type, const int16_t *joint_map, const int16_t *link_map, const int16_t *link_sphere_map, \
      const int16_t *link_chain_data, const int16_t *link_chain_offsets, const float *joint_offset_map,               \
      const float *sphere_padding, const float *self_collision_weight, const int16_t *pair_locations,                 \
      const curobo_hip_scene *scene, const float *scene_collision_weight, const float *activation_distance,           \
      const float *speed_dt, const int32_t *env_query_idx, int num_envs, int use_multi_env, int batch_size,           \
      int padded_horizon, int dof, int n_knots, int bspline_degree, int num_links, int num_spheres,                   \
      int num_collision_pairs, int link_chain_len, int sweep_steps, int enable_speed_metric, int32_t *dispatch_ws,    \
      int dispatch_phase, const uint32_t *self_lane_lists, int self_lane_len
#define CUROBO_TRAJ_ARGS                                                                                              \
  out_cost, out_grad_knots, out_position, out_robot_spheres, u_position, start_position, start_velocity,             \
      start_acceleration, start_jerk, goal_position, goal_velocity, goal_acceleration, goal_jerk, start_idx, goal_idx, \
      traj_dt, use_implicit_goal_state, fixed_transform, robot_spheres, joint_map_type, joint_map, link_map,          \
      link_sphere_map, link_chain_data, link_chain_offsets, joint_offset_map, sphere_padding, self_collision_weight,  \
      pair_locations, scene, scene_collision_weight, activation_distance, speed_dt, env_query_idx, num_envs,          \
      use_multi_env, batch_size, padded_horizon, dof, n_knots, bspline_degree, num_links, num_spheres,                \
      num_collision_pairs, link_chain_len, sweep_steps, enable_speed_metric, dispatch_ws, dispatch_phase, self_lane_lists,   \
      self_lane_len

// The pair list dealt to lanes (lane = sphere form of the self-collision pass of the fused kernels): every pair (i, j)
// is given to ONE of its two spheres so that the longest list is as short as possible (a b-matching, found with
// augmenting paths); sphere s is owned by lane s % 64 of pass s / 64.  out_lists_host [(len0 + len1) * 64] words,
// word (e, lane) = partner byte offset (16 j) | pair index << 16, lists in ascending pair index, padded with the NaN
// sphere behind the last one (16 S) | 0xffff << 16.  Returns len0 | len1 << 16 (pass the value on as self_lane_len),
// 0 when this robot is outside the form (more than 128 spheres, 65535 pairs or `capacity_words`), < 0 on bad arguments.
// HOST pointers: call once per robot, copy out_lists_host to the device.
CUROBO_EXPORT int curobo_hip_self_lane_lists_host(uint32_t *out_lists_host, int capacity_words, const int16_t *pair_locations_host,
                                                  int num_collision_pairs, int num_spheres) {
  const char *what = "self_lane_lists_host";
  if (!out_lists_host || !pair_locations_host || num_collision_pairs <= 0 || num_spheres <= 0) {
    set_error(CUROBO_HIP_ERR_INVALID, "%s: bad arguments", what);
    return -1;
  }
  const int P = num_collision_pairs, S = num_spheres;
  if (S > 128 || P >= 65535 || P > 16384) return 0;
  for (int k = 0; k < P; k++) {
    const int i = pair_locations_host[2 * k], j = pair_locations_host[2 * k + 1];
    if (i < 0 || j < 0 || i >= S || j >= S) { set_error(CUROBO_HIP_ERR_INVALID, "%s: pair %d out of range", what, k); return -1; }
  }
  std::vector<int> owner(P), load(S), cap(S), seen(S);
  std::vector<std::vector<int>> owned(S);
  auto other = [&](int k, int x) { const int i = pair_locations_host[2 * k], j = pair_locations_host[2 * k + 1]; return x == i ? j : i; };
  // free one slot of sphere x by moving one of its pairs to that pair's other sphere (recursively)
  std::function<bool(int)> make_room = [&](int x) -> bool {
    for (size_t n = 0; n < owned[x].size(); n++) {
      const int k2 = owned[x][n], y = other(k2, x);
      if (y == x || seen[y]) continue;
      seen[y] = 1;
      if (load[y] < cap[y] || make_room(y)) {
        owned[x].erase(owned[x].begin() + (long)n);
        load[x]--;
        owned[y].push_back(k2);
        load[y]++;
        owner[k2] = y;
        return true;
      }
    }
    return false;
  };
  auto feasible = [&](int c0, int c1) -> bool {
    for (int x = 0; x < S; x++) { cap[x] = x < 64 ? c0 : c1; load[x] = 0; owned[x].clear(); }
    for (int k = 0; k < P; k++) {
      const int e[2] = {pair_locations_host[2 * k], pair_locations_host[2 * k + 1]};
      int x = -1;
      // the emptier of the two spheres when it has room, else make room at either
      const int a0 = load[e[0]] <= load[e[1]] ? e[0] : e[1], a1 = a0 == e[0] ? e[1] : e[0];
      if (load[a0] < cap[a0]) x = a0;
      else if (load[a1] < cap[a1]) x = a1;
      else {
        for (int t = 0; t < 2 && x < 0; t++) {
          std::fill(seen.begin(), seen.end(), 0);
          seen[e[0]] = seen[e[1]] = 1;
          if (cap[e[t]] > 0 && make_room(e[t])) x = e[t];
        }
      }
      if (x < 0) return false;
      owned[x].push_back(k);
      load[x]++;
      owner[k] = x;
    }
    return true;
  };
  int len0 = -1, len1 = -1;
  const int lower = (P + 63) / 64;
  for (int total = lower; total <= P && len0 < 0; total++)
    for (int c1 = 0; c1 <= (S > 64 ? total : 0) && len0 < 0; c1++)
      if (feasible(total - c1, c1)) { len0 = total - c1; len1 = c1; }
  if (len0 < 0 || len0 > 0xffff || len1 > 0xffff || (len0 + len1) * 64 > capacity_words) return 0;
  const uint32_t pad = (uint32_t)(S * 16) | (0xffffu << 16);
  for (int w = 0; w < (len0 + len1) * 64; w++) out_lists_host[w] = pad;
  for (int x = 0; x < S; x++) {
    std::sort(owned[x].begin(), owned[x].end());
    const int base = x < 64 ? 0 : len0, lane = x & 63;
    for (size_t n = 0; n < owned[x].size(); n++)
      out_lists_host[(size_t)(base + (int)n) * 64 + lane] = (uint32_t)(other(owned[x][n], x) * 16) | ((uint32_t)owned[x][n] << 16);
  }
  return len0 | (len1 << 16);
}

CUROBO_EXPORT int curobo_hip_rollout_trajectory_fused(CUROBO_TRAJ_PARAMS, curobo_hip_stream_t stream) {
  return rollout_trajectory_fused_impl("rollout_trajectory_fused", nullptr, CUROBO_TRAJ_ARGS, FusedReuse{}, stream);
}

CUROBO_EXPORT int curobo_hip_rollout_trajopt_fused(CUROBO_TRAJ_PARAMS, const curobo_hip_trajopt_terms *terms,
                                                   curobo_hip_stream_t stream) {
  return rollout_trajectory_fused_impl("rollout_trajopt_fused", terms, CUROBO_TRAJ_ARGS, FusedReuse{}, stream);
}

// The same two launches with reuse of evaluations the caller holds (fused_reuse_known_row): trajectories b with
// b % memo_stride == memo_slot whose knots have the bits of memo_x[b / memo_stride] get memo_cost / memo_grad of that row.
#define CUROBO_REUSE_PARAMS const float *memo_x, const float *memo_cost, const float *memo_grad, int memo_stride, int memo_slot
#define CUROBO_REUSE_ARGS FusedReuse{memo_x, memo_cost, memo_grad, memo_stride, memo_slot}
CUROBO_EXPORT int curobo_hip_rollout_trajectory_fused_reuse(CUROBO_TRAJ_PARAMS, CUROBO_REUSE_PARAMS, curobo_hip_stream_t stream) {
  return rollout_trajectory_fused_impl("rollout_trajectory_fused_reuse", nullptr, CUROBO_TRAJ_ARGS, CUROBO_REUSE_ARGS, stream);
}

CUROBO_EXPORT int curobo_hip_rollout_trajopt_fused_reuse(CUROBO_TRAJ_PARAMS, const curobo_hip_trajopt_terms *terms, CUROBO_REUSE_PARAMS,
                                                         curobo_hip_stream_t stream) {
  return rollout_trajectory_fused_impl("rollout_trajopt_fused_reuse", terms, CUROBO_TRAJ_ARGS, CUROBO_REUSE_ARGS, stream);
}
#undef CUROBO_REUSE_PARAMS
#undef CUROBO_REUSE_ARGS
#undef CUROBO_TRAJ_PARAMS
#undef CUROBO_TRAJ_ARGS

CUROBO_EXPORT int curobo_hip_rollout_trajopt_fused_lds_bytes(int padded_horizon, int dof, int num_links, int num_spheres,
                                                             int num_collision_pairs, int link_chain_len,
                                                             int num_obstacles, int with_cspace_terms) {
  int threads;
  const FusedLayout lay = trajectory_launch_shape(padded_horizon, dof, num_links, num_spheres, link_chain_len, num_collision_pairs,
                                                  num_obstacles, with_cspace_terms ? 4 * padded_horizon * dof : 0, &threads);
  return lay.total * (int)sizeof(float);
}

CUROBO_EXPORT int curobo_hip_rollout_trajopt_fused_torque_fits(int padded_horizon, int dof, int num_links, int num_spheres,
                                                               int num_collision_pairs, int link_chain_len, int num_obstacles) {
  int threads;
  const FusedLayout lay = trajectory_launch_shape(padded_horizon, dof, num_links, num_spheres, link_chain_len, num_collision_pairs,
                                                  num_obstacles, 4 * padded_horizon * dof, &threads, 1);
  return (size_t)lay.total * sizeof(float) <= 160 * 1024 && fused_torque_fits(lay, padded_horizon, dof, num_links, num_spheres) ? 1 : 0;
}
