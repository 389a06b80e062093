// rollout_ik_fused.hip -- horizon-1 ("teleport") rollout of the IK solver in one launch: q -> FK -> tool-pose goal-set
// cost + c-space bound cost + self + scene collision -> cost[b] and d cost / d q[b].  Replaces
// the seven launches of curobo_amd/rollout/ik_rollout.py (reference RobotRollout with
// StateFromPositionTeleport and the cost set of content/configs/task/ik/lbfgs_ik.yml); same
// device functions, intermediates in LDS.  16 configurations per 256-thread workgroup (one
// 16-lane row each) share the staged robot / scene tables.  The tool-pose gradient enters the
// link-wrench VJP as a force at the tool link's origin plus the free torque omega = 1/2 E(q)^T g
// (reference kinematics_backward_helper.cuh:102-183, quaternion_util.cuh:86-102).
#include <type_traits>

#include "fused_device.hpp"

namespace curobo_hip {

struct FusedIkArgs {
  FusedTrajArgs r;  // robot / self / scene members, out_cost, out_position (= nothing), out_spheres
  const float *x;   // [n_points, dof]
  float *out_grad_q;
  ToolPoseArgs tp;  // current_position / current_quat unused (computed here); out_* optional
  const float *p_b, *cs_weight, *cs_eta;  // c-space bound term: limits [2, dof], weight[>=1], activation[>=1]
  float *out_cspace_cost;                 // optional [n_points, dof]
  const int16_t *tool_frame_map;
  float *out_link_pos, *out_link_quat;  // optional [n_points, T, 3|4]
  int n_tool_frames, n_points;
};

// the current state of the STATE variant: limits tightened to one time step from it + implied velocity / acceleration
// regularisation (wp_cspace_position.py:299-356).  Read from global memory by the lane that owns the joint: no LDS.
struct FusedIkStateArgs : FusedIkArgs {
  const float *reg_weight;          // squared_l2_reg_weight [2]
  const float *current_position;    // [n_states, dof]
  const float *current_velocity;    // [n_states, dof] or NULL (no acceleration term then)
  const int32_t *idxs_current_state;  // [n_points]: any state per row, rows of one workgroup may differ
  const float *v_b, *state_dt;      // [2, dof], [n_states]
};

template <int KINDS, bool STATE = false>
__global__ void __launch_bounds__(256, 4) rollout_ik_fused_kernel(const std::conditional_t<STATE, FusedIkStateArgs, FusedIkArgs> ia) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const FusedTrajArgs &a = ia.r;
  const int H = kIkPoints, D = a.bs.dof, L = a.nlinks, S = a.nspheres, P = a.npairs, T = ia.n_tool_frames;
  const int n_rec = a.sc.max_cuboids + a.sc.max_voxel_grids;
  const FusedLayout lay = fused_layout(H, D, L, S, a.chain_len, P, n_rec, 0, 0, 1, 0, false);
  const int tid = threadIdx.x, nt = blockDim.x;
  const int pt0 = blockIdx.x * kIkPoints;
  const int npts = min(kIkPoints, ia.n_points - pt0);
  FusedCtx c;
  fused_ctx_carve(c, smem, lay, H, D, L, S, P);
  // the 16 configurations of a workgroup share ONE environment (scene and sphere set): that of its first configuration.
  // The caller checks that env_query_idx is constant over aligned runs of 16 (seeds of one problem: IkRollout).
  const int wg_env = (a.use_multi_env || a.num_envs > 1) ? a.env_query_idx[pt0] : 0;
  c.env = a.use_multi_env ? wg_env : 0;
  c.w_self = a.use_self ? a.w_self[0] : 0.0f;
  c.w_scene = a.use_scene ? a.w_scene[0] : 0.0f;
  c.eta = a.use_scene ? a.eta[0] : 0.0f;
  c.speed_metric = false;
  c.speed_dt = 0.0f;
  fused_stage_tables(c, a, lay, reinterpret_cast<const float4 *>(a.robot_spheres) + (size_t)(a.num_envs > 1 ? wg_env : 0) * S, n_rec);
  for (int e = rotated_tid((nt >> 6) / 2); e < npts * D; e += nt) c.q[e] = ia.x[(size_t)pt0 * D + e];
  __syncthreads();
  fused_derive_tables(c);

  const int h = tid / kFkLanes, lane = tid % kFkLanes, lane64 = tid & 63;
  const bool live = h < npts;
  const int n = pt0 + h;
  // ---- FK
  if (live) point_fk_row(c, a, blockIdx.x, h, lane);
  __syncthreads();  // derived tables (other waves) + this row's spheres
  if (!live) return;

  // ---- costs + wrenches
  const float4 *sph = c.spheres(h);
  float *wr = c.wrench + (size_t)h * c.wl;
  float cost_pt = 0.0f;
  bool any_grad = false;
  if (a.use_self) {
    int kmin;
    const float m = row_pair_argmax(c, sph, lane, kmin);
    if (kmin != 0x7fffffff && m > 0.0f) {
      any_grad = true;
      if (lane == 0) cost_pt += self_pair_apply(c, h, m, kmin);
    }
  }
  if (a.use_scene) {
    point_link_masks<0, KINDS>(c, a.sc, h, lane);
    for (int s0 = 0; s0 < S; s0 += kFkLanes) {  // (a copy of the sphere-per-lane scene loop of the trajectory kernel's row fallback, fused_device.hpp)
      const int s = s0 + lane;
      float d = 0.0f;
      f3 g = make_f3(0.f, 0.f, 0.f);
      float4 c4 = make_float4(0.f, 0.f, 0.f, -1.f);
      const uint32_t mask = s < S ? __float_as_uint(wr[c.sph_link[s] * kWrench + 6]) : 0u;
      if (s < S && (mask != 0u || n_rec > 32)) c4 = scene_sphere<0, KINDS>(c, a.sc, h, s, d, g, mask);
      cost_pt += d;
      any_grad = wrench_add_serialised(c, h, s, make_f3(c4.x, c4.y, c4.z), g, lane64) || any_grad;
    }
  }
  // tool-pose goal-set cost (wp_tool_pose.py:456-692), one tool frame per lane
  point_tool_pose(c, ia.tp, ia.tool_frame_map, T, n, 0, h, (size_t)n * T, ia.out_link_pos, ia.out_link_quat, lane, lane64,
                  cost_pt, any_grad);
  // c-space bound cost (wp_cspace_position.py:232-362): its gradient is already in joint space
  float gp_joint[kDofIters];
  int cur = 0;
  float state_dt = 0.0f;
  if constexpr (STATE) {
    cur = ia.idxs_current_state[n];
    state_dt = ia.state_dt[cur];
  }
#pragma unroll
  for (int it = 0; it < kDofIters; it++) {
    const int d = it * kFkLanes + lane;
    float g = 0.0f;
    if (d < D) {
      float pl = ia.p_b[d], pu = ia.p_b[D + d];
      { const float r = pu - pl, eta_p = ia.cs_eta[0]; pl = pl + eta_p * r; pu = pu - eta_p * r; }
      const float cp = c.q[h * D + d];
      float cur_p = 0.0f;
      if constexpr (STATE) {
        if (state_dt > 0.0f) {
          cur_p = ia.current_position[(size_t)cur * D + d];
          cspace_velocity_bounds(pl, pu, cur_p, ia.v_b[d], ia.v_b[D + d], state_dt);
        }
      }
      float cc = cspace_bound_term(cp, pl, pu, ia.cs_weight[0], g);
      if constexpr (STATE) {
        if (ia.current_velocity) {
          cspace_state_regularisation(cp, cur_p, ia.current_velocity + (size_t)cur * D + d, state_dt, ia.reg_weight, cc, g);
        } else {  // (no current velocity: the entry point was told the acceleration weight is zero)
          const float reg_v[2] = {ia.reg_weight[0], 0.0f};
          cspace_state_regularisation(cp, cur_p, nullptr, state_dt, reg_v, cc, g);
        }
      }
      cost_pt += cc;
      if (ia.out_cspace_cost) ia.out_cspace_cost[(size_t)n * D + d] = cc;
    }
    gp_joint[it] = g;
  }
  cost_pt = row16_sum(cost_pt);
  if (lane == 0) a.out_cost[n] = cost_pt;
  point_vjp_gather(c, h, any_grad, lane);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int it = 0; it < kDofIters; it++) {
    const int d = it * kFkLanes + lane;
    if (d < D) ia.out_grad_q[(size_t)n * D + d] = c.q[h * D + d] + gp_joint[it];
  }
}

}  // namespace curobo_hip

using namespace curobo_hip;

CUROBO_EXPORT int curobo_hip_rollout_ik_fused_lds_bytes(int dof, int num_links, int num_spheres, int num_collision_pairs,
                                                        int link_chain_len, int num_obstacles) {
  const FusedLayout lay = fused_layout(kIkPoints, dof, num_links, num_spheres, link_chain_len, num_collision_pairs, num_obstacles, 0, 0, 1, 0, false);
  return lay.total * (int)sizeof(float);
}

#define CUROBO_IK_FUSED_PARAMS                                                                                                      \
    float *out_cost, float *out_grad_q, float *out_pose_distance, float *out_position_distance,                                      \
    float *out_rotation_distance, int32_t *out_goalset_idx, float *out_link_pos, float *out_link_quat,                               \
    float *out_robot_spheres, float *out_cspace_cost, const float *q, const float *goal_position, const float *goal_quat,            \
    const int32_t *idxs_goal, const float *position_orientation_weight, const float *terminal_pose_axes_weight_factor,               \
    const float *terminal_pose_convergence_tolerance, const uint8_t *project_distance_to_goal, int num_goalset,                      \
    int rotation_method, const float *p_b, const float *cspace_weight, const float *cspace_activation_distance,                      \
    const float *fixed_transform, const float *robot_spheres, const int8_t *joint_map_type, const int16_t *joint_map,                \
    const int16_t *link_map, const int16_t *tool_frame_map, const int16_t *link_sphere_map,                                          \
    const int16_t *link_chain_data, const int16_t *link_chain_offsets, const float *joint_offset_map,                                \
    const float *sphere_padding, const float *self_collision_weight, const int16_t *pair_locations,                                  \
    const curobo_hip_scene *scene, const float *scene_collision_weight, const float *activation_distance,                            \
    int batch_size, int dof, int num_links, int n_tool_frames, int num_spheres, int num_collision_pairs,                             \
    int link_chain_len, const int32_t *env_query_idx, int num_envs, int use_multi_env
#define CUROBO_IK_FUSED_ARGS                                                                                                        \
    out_cost, out_grad_q, out_pose_distance, out_position_distance, out_rotation_distance, out_goalset_idx, out_link_pos,            \
    out_link_quat, out_robot_spheres, out_cspace_cost, q, goal_position, goal_quat, idxs_goal, position_orientation_weight,          \
    terminal_pose_axes_weight_factor, terminal_pose_convergence_tolerance, project_distance_to_goal, num_goalset,                    \
    rotation_method, p_b, cspace_weight, cspace_activation_distance, fixed_transform, robot_spheres, joint_map_type, joint_map,      \
    link_map, tool_frame_map, link_sphere_map, link_chain_data, link_chain_offsets, joint_offset_map, sphere_padding,                \
    self_collision_weight, pair_locations, scene, scene_collision_weight, activation_distance, batch_size, dof, num_links,           \
    n_tool_frames, num_spheres, num_collision_pairs, link_chain_len, env_query_idx, num_envs, use_multi_env

// both entry points: state == nullptr is curobo_hip_rollout_ik_fused, else the pointers of the STATE variant (the base part unset)
static int rollout_ik_fused_launch(
    const char *what, const FusedIkStateArgs *state, CUROBO_IK_FUSED_PARAMS, curobo_hip_stream_t stream) {
  CUROBO_REQUIRE((!use_multi_env && num_envs <= 1) || env_query_idx, "%s: per-environment scenes / sphere sets need env_query_idx", what);
  if (const int bad = fused_check_dimensions(what, num_links, num_spheres, link_chain_len, pair_locations)) return bad;
  CUROBO_REQUIRE(dof >= 1 && dof <= 64, "%s: bad dimensions", what);
  CUROBO_REQUIRE(n_tool_frames >= 1 && num_goalset >= 1, "%s: need at least one tool frame / goal", what);
  if (batch_size == 0) return CUROBO_HIP_OK;
  FusedIkStateArgs ia{};
  if (state) ia = *state;
  FusedTrajArgs &a = ia.r;
  a.out_cost = out_cost; a.out_spheres = out_robot_spheres;
  fused_fill_robot_args(a, true, fixed_transform, robot_spheres, joint_map_type, joint_map, link_map, link_sphere_map, link_chain_data,
                        link_chain_offsets, joint_offset_map, sphere_padding, self_collision_weight, pair_locations, scene,
                        scene_collision_weight, activation_distance, env_query_idx, num_envs, use_multi_env, batch_size, dof, num_links,
                        num_spheres, num_collision_pairs, link_chain_len);
  ia.x = q; ia.out_grad_q = out_grad_q; ia.tool_frame_map = tool_frame_map; ia.n_tool_frames = n_tool_frames;
  ia.n_points = batch_size; ia.out_link_pos = out_link_pos; ia.out_link_quat = out_link_quat;
  ToolPoseArgs &tp = ia.tp;
  tp.out_distance = out_pose_distance; tp.out_position_distance = out_position_distance;
  tp.out_rotation_distance = out_rotation_distance; tp.out_goalset_idx = out_goalset_idx;
  tp.goal_position = goal_position; tp.goal_quat = goal_quat; tp.idxs_goal = idxs_goal;
  tp.position_orientation_weight = position_orientation_weight;
  tp.terminal_axes_weight = terminal_pose_axes_weight_factor; tp.non_terminal_axes_weight = terminal_pose_axes_weight_factor;
  tp.terminal_tolerance = terminal_pose_convergence_tolerance; tp.non_terminal_tolerance = terminal_pose_convergence_tolerance;
  tp.project_distance_to_goal = project_distance_to_goal;
  tp.batch = batch_size; tp.horizon = 1; tp.num_links = n_tool_frames; tp.num_goalset = num_goalset; tp.rotation_method = rotation_method;
  CUROBO_REQUIRE(rotation_method >= 0 && rotation_method <= 2, "%s: rotation_method must be 0, 1 or 2", what);
  // c-space bound term (no effort or target term in the IK cost set); velocity-limited bounds and regularisation with a state
  ia.p_b = p_b; ia.cs_weight = cspace_weight; ia.cs_eta = cspace_activation_distance; ia.out_cspace_cost = out_cspace_cost;
  hipStream_t st = (hipStream_t)stream;
  const int n_rec = a.sc.max_cuboids + a.sc.max_voxel_grids;
  const FusedLayout lay = fused_layout(kIkPoints, dof, num_links, num_spheres, link_chain_len, a.npairs, n_rec, 0, 0, 1, 0, false);
  const size_t lds = (size_t)lay.total * sizeof(float);
  CUROBO_REQUIRE(lds <= 160 * 1024, "%s: 16 configurations do not fit in LDS (%zu bytes); use the unfused kernels", what, lds);
  const int kinds = fused_scene_kinds(a.sc);
  const dim3 grid((unsigned)ceil_div(batch_size, kIkPoints)), block(kIkPoints * kFkLanes);
  if (state) {
    const auto kfn = kinds == 2 ? rollout_ik_fused_kernel<2, true> : kinds == 3 ? rollout_ik_fused_kernel<3, true> : kinds == 7 ? rollout_ik_fused_kernel<7, true> : rollout_ik_fused_kernel<1, true>;
    return fused_launch_status(what, fused_launch(kfn, grid, block, lds, kFusedLdsUnasked, st, ia), st);
  }
  const auto kfn = kinds == 2 ? rollout_ik_fused_kernel<2> : kinds == 3 ? rollout_ik_fused_kernel<3> : kinds == 7 ? rollout_ik_fused_kernel<7> : rollout_ik_fused_kernel<1>;
  return fused_launch_status(what, fused_launch(kfn, grid, block, lds, kFusedLdsUnasked, st, static_cast<const FusedIkArgs &>(ia)), st);
}

CUROBO_EXPORT int curobo_hip_rollout_ik_fused(CUROBO_IK_FUSED_PARAMS, curobo_hip_stream_t stream) {
  return rollout_ik_fused_launch("rollout_ik_fused", nullptr, CUROBO_IK_FUSED_ARGS, stream);
}

CUROBO_EXPORT int curobo_hip_rollout_ik_fused_state(
    CUROBO_IK_FUSED_PARAMS, const float *squared_l2_reg_weight, const float *current_position, const float *current_velocity,
    const int32_t *idxs_current_state, const float *velocity_limits, const float *state_dt, int acceleration_regularization,
    curobo_hip_stream_t stream) {
  const char *what = "rollout_ik_fused_state";
  CUROBO_REQUIRE((current_position && idxs_current_state && velocity_limits && state_dt) ||
                     (!current_position && !idxs_current_state && !velocity_limits && !state_dt),
                 "%s: current_position, idxs_current_state, velocity_limits and state_dt are given together or not at all", what);
  CUROBO_REQUIRE(current_position, "%s: needs a current state (curobo_hip_rollout_ik_fused is the launch without one)", what);
  CUROBO_REQUIRE(squared_l2_reg_weight, "%s: squared_l2_reg_weight [2] is required", what);
  CUROBO_REQUIRE(!acceleration_regularization || current_velocity,
                 "%s: acceleration regularisation is configured, current_velocity is required", what);
  FusedIkStateArgs state{};
  state.reg_weight = squared_l2_reg_weight; state.current_position = current_position; state.current_velocity = current_velocity;
  state.idxs_current_state = idxs_current_state; state.v_b = velocity_limits; state.state_dt = state_dt;
  return rollout_ik_fused_launch(what, &state, CUROBO_IK_FUSED_ARGS, stream);
}
