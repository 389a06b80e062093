// pose_detect.hip -- mesh-SDF pose refinement (curobo_amd/perception/pose_estimation), one Levenberg-Marquardt iteration in
// two launches:
//   curobo_hip_pose_sdf_evaluate   observed points against ONE mesh at a pose held on the device: unsigned distance, world
//                                  gradient, validity, the six Jacobian entries, and per workgroup one row of partial sums of
//                                  J^T J (upper triangle), J^T r, sum r^2 and the valid count
//   curobo_hip_pose_lm_step        one lane: the partials summed in workgroup order, the trust-region update, the 6 x 6
//                                  Cholesky step, the predicted reduction and the next candidate pose
//
// Reference: perception/pose_estimation/wp_mesh_sdf_alignment.py (mesh_surface_distance_query_kernel :84-146 and
// jacobian_reduce_kernel :154-377, two Warp launches that accumulate with float atomics), perception/optim_pose_lm.py
// (compute_predicted_reduction :28-48, trust_region_update :53-175, solve_lm_step :180-202) and
// sdf_pose_detector.py:_setup_refinement / _refine_iteration (:266-399), which sequences them with ~40 torch launches.
//
// The row of partial sums, its sum in workgroup order, the Cholesky solve and the rules that make all of it deterministic:
// pose_device.hpp.  Here a workgroup is four wavefronts: each forms its row, they meet in LDS and are added in wavefront order.
#include "mesh_device.hpp"
#include "pose_device.hpp"

namespace curobo_hip {

constexpr int kPoseThreads = 256, kPoseWaves = kPoseThreads / kWave;

struct PoseEvalArgs {
  const float *points, *position, *quaternion;
  curobo_hip_mesh mesh;
  float max_distance, distance_threshold, huber_delta;
  int use_huber, n;
  float *out_distance, *out_gradient;
  int32_t *out_valid;
  float *ws;
};

__global__ __launch_bounds__(kPoseThreads) void pose_sdf_evaluate_kernel(PoseEvalArgs a) {
  __shared__ float part[kPoseWaves][kPoseRow];
  const int tid = threadIdx.x, i = blockIdx.x * kPoseThreads + tid;
  const f3 t = make_f3(a.position[0], a.position[1], a.position[2]);
  const float qw = a.quaternion[0], qx = a.quaternion[1], qy = a.quaternion[2], qz = a.quaternion[3];
  // a pose that is not finite (the step kernel answers a failed factorisation with one) finds nothing: without this test
  // every lane would walk the whole tree (fmaxf drops the NaN of a box distance) to reject every triangle
  const bool pose_ok = isfinite(t.x) && isfinite(t.y) && isfinite(t.z) && isfinite(qw) && isfinite(qx) && isfinite(qy) && isfinite(qz);
  float j0 = 0.f, j1 = 0.f, j2 = 0.f, j3 = 0.f, j4 = 0.f, j5 = 0.f, r = 0.f, dist = 0.f;
  f3 gw = make_f3(0.f, 0.f, 0.f);
  bool valid = false;
  if (i < a.n && pose_ok) {
    const f3 p = make_f3(a.points[(size_t)i * 3], a.points[(size_t)i * 3 + 1], a.points[(size_t)i * 3 + 2]);
    const f3 pm = quat_rot(qw, -qx, -qy, -qz, p - t);  // transform_point_inverse: R^T (p - t)
    float d2 = a.max_distance * a.max_distance;
    f3 cp = pm;
    int side;
    if (mesh_closest_point(a.mesh, pm, d2, cp, side)) {  // (unsigned: the side is not used)
      const f3 delta = cp - pm;
      const float d = sqrtf(dot(delta, delta));
      if (d <= a.distance_threshold && d > 1e-8f) {
        gw = quat_rot(qw, qx, qy, qz, (1.0f / d) * delta);
        dist = d;
        valid = true;
        r = d;
        float hs = 1.0f;
        if (a.use_huber != 0) {
          if (r > a.huber_delta) hs = sqrtf(a.huber_delta / r);
          r = r * hs;
        }
        j0 = gw.x * hs; j1 = gw.y * hs; j2 = gw.z * hs;            // wp_mesh_sdf_alignment.py:213-220
        j3 = (gw.z * p.y - gw.y * p.z) * hs;
        j4 = (gw.x * p.z - gw.z * p.x) * hs;
        j5 = (gw.y * p.x - gw.x * p.y) * hs;
      }
    }
  }
  if (i < a.n) {
    if (a.out_distance) a.out_distance[i] = dist;
    if (a.out_gradient) { a.out_gradient[(size_t)i * 3] = gw.x; a.out_gradient[(size_t)i * 3 + 1] = gw.y; a.out_gradient[(size_t)i * 3 + 2] = gw.z; }
    if (a.out_valid) a.out_valid[i] = valid ? 1 : 0;
  }
  // ---- the workgroup's row: J^T J, J^T r, sum r^2, count
  const float j[6] = {j0, j1, j2, j3, j4, j5};
  const int wave = tid / kWave, lane = tid % kWave;
  const float word = pose_row_word(j, j, r, r * r, valid, lane);
  if (lane < kPoseRow) part[wave][lane] = word;
  __syncthreads();
  if (tid < kPoseRow) {
    float *row = a.ws + (size_t)blockIdx.x * kPoseRow;
    if (tid == kPoseCount) {
      int c = 0;
#pragma unroll
      for (int w = 0; w < kPoseWaves; w++) c += __float_as_int(part[w][tid]);
      row[tid] = __int_as_float(c);
    } else {  // (the words after the count are zeros, and stay zeros)
      float s = part[0][tid];
#pragma unroll
      for (int w = 1; w < kPoseWaves; w++) s += part[w][tid];
      row[tid] = s;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- the LM step
struct PoseStepArgs {
  curobo_hip_pose_lm_state *s;
  const float *ws;
  int n_rows, mode;
  float lambda_initial, lambda_factor, lambda_min, lambda_max, rho_min;
  int minimum_valid_count;
};

__global__ __launch_bounds__(kWave) void pose_lm_step_kernel(PoseStepArgs a) {
  __shared__ float red[kPoseRow];
  const int lane = threadIdx.x;
  pose_sum_rows(red, a.ws, a.n_rows, lane);
  if (lane != 0) return;
  curobo_hip_pose_lm_state &s = *a.s;
  float cJ[36], cr[6];
  pose_unpack_symmetric(red, cJ);
  for (int u = 0; u < 6; u++) cr[u] = red[21 + u];
  const float sum_sq = red[27];
  const int n_valid = __float_as_int(red[kPoseCount]);
  const float cand_rms = sqrt_rn(div_rn(sum_sq, (float)n_valid + 1e-8f));
  s.cand_sum_sq = sum_sq;
  s.cand_n_valid = n_valid;
  bool accept;
  float lambda;
  if (a.mode == CUROBO_HIP_POSE_LM_INIT) {  // _setup_refinement: the evaluated pose is the best state, whatever it holds
    accept = true;
    lambda = a.lambda_initial;
    s.best_error = cand_rms;
    s.trust_ratio = 0.0f;
  } else {  // trust_region_update
    const bool enough = n_valid > a.minimum_valid_count;
    const float ratio = div_rn(s.best_sum_sq - sum_sq, s.pred_reduction + 1e-8f);
    accept = ratio >= 0.0f && enough;  // (rho_min is carried and not consulted: optim_pose_lm.py:142)
    lambda = accept ? div_rn(s.lambda_damping, a.lambda_factor) : s.lambda_damping * a.lambda_factor;
    lambda = fminf(fmaxf(lambda, a.lambda_min), a.lambda_max);
    if (accept) s.best_error = enough ? cand_rms : __builtin_inff();
    s.trust_ratio = ratio;
  }
  s.accepted = accept ? 1 : 0;
  s.lambda_damping = lambda;
  if (accept) {
    for (int k = 0; k < 3; k++) s.best_position[k] = s.cand_position[k];
    for (int k = 0; k < 4; k++) s.best_quaternion[k] = s.cand_quaternion[k];
    s.best_sum_sq = sum_sq;
    s.best_n_valid = n_valid;
    for (int k = 0; k < 36; k++) s.best_JtJ[k] = cJ[k];
    for (int k = 0; k < 6; k++) s.best_Jtr[k] = cr[k];
  } else {
    for (int k = 0; k < 36; k++) cJ[k] = s.best_JtJ[k];
    for (int k = 0; k < 6; k++) cr[k] = s.best_Jtr[k];
  }
  // ---- the next candidate, from the best state (cJ / cr hold it now)
  float d[6];
  const float nan = __builtin_nanf("");
  if (!pose_solve6<kPoseSolveLM>(cJ, lambda, cr, d))  // (J^T J + lambda I) delta = -J^T r (solve_lm_step)
    for (int k = 0; k < 6; k++) d[k] = nan;  // the candidate finds no point, is rejected, and lambda grows
  float pred = 0.0f, quad = 0.0f;  // compute_predicted_reduction
  for (int u = 0; u < 6; u++) {
    float row = 0.0f;
    for (int v = 0; v < 6; v++) row += cJ[u * 6 + v] * d[v];
    quad += d[u] * row;
    pred += d[u] * cr[u];
  }
  s.pred_reduction = -pred + -0.5f * quad;
  for (int k = 0; k < 6; k++) s.delta[k] = d[k];
  // Pose.from_euler_xyz(delta[3:], delta[:3]).multiply(best): fixed axes X, Y, Z (q = qz qy qx); not renormalised
  const float hx = d[3] * 0.5f, hy = d[4] * 0.5f, hz = d[5] * 0.5f;
  const float cx = cosf(hx), sx = sinf(hx), cy = cosf(hy), sy = sinf(hy), cz = cosf(hz), sz = sinf(hz);
  const float aw = cx * cy * cz + sx * sy * sz, ax = sx * cy * cz - cx * sy * sz, ay = cx * sy * cz + sx * cy * sz,
              az = cx * cy * sz - sx * sy * cz;
  const f3 bp = make_f3(s.best_position[0], s.best_position[1], s.best_position[2]);
  const float bw = s.best_quaternion[0], bx = s.best_quaternion[1], by = s.best_quaternion[2], bz = s.best_quaternion[3];
  const f3 u3 = make_f3(ax, ay, az);
  const f3 tt = 2.0f * cross(u3, bp);
  const f3 rp = bp + aw * tt + cross(u3, tt);
  s.cand_position[0] = d[0] + rp.x; s.cand_position[1] = d[1] + rp.y; s.cand_position[2] = d[2] + rp.z;
  s.cand_quaternion[0] = aw * bw - ax * bx - ay * by - az * bz;
  s.cand_quaternion[1] = aw * bx + ax * bw + ay * bz - az * by;
  s.cand_quaternion[2] = aw * by - ax * bz + ay * bw + az * bx;
  s.cand_quaternion[3] = aw * bz + ax * by - ay * bx + az * bw;
}

}  // namespace curobo_hip

using namespace curobo_hip;

static int pose_rows(int n_points) { return ceil_div(n_points, kPoseThreads); }
static int check_sdf_workspace(const void *workspace, int64_t workspace_bytes, int n_points, const char *what) {
  char counted[32];
  snprintf(counted, sizeof counted, "%d points", n_points);
  return check_pose_workspace(workspace, workspace_bytes, pose_rows(n_points), what, counted, "curobo_hip_pose_sdf_ws_bytes");
}

CUROBO_EXPORT int curobo_hip_pose_sdf_ws_bytes(int n_points, int64_t *out_bytes) {
  const char *what = "pose_sdf_ws_bytes";
  CUROBO_REQUIRE(out_bytes, "%s: out_bytes must not be null", what);
  CUROBO_REQUIRE(n_points > 0, "%s: n_points must be positive, got %d", what, n_points);
  *out_bytes = pose_ws_bytes(pose_rows(n_points));
  return CUROBO_HIP_OK;
}

static int check_pose_mesh(const curobo_hip_mesh *m, const char *what) {
  CUROBO_REQUIRE(m, "%s: mesh must not be null", what);
  CUROBO_REQUIRE(m->tri && m->node_box && m->n_tri > 0 && m->n_leaves >= 1 && m->leaf_size >= 1,
                 "%s: the mesh has no tree (build it with curobo_hip_mesh_bvh_build)", what);
  CUROBO_REQUIRE((m->n_leaves & (m->n_leaves - 1)) == 0 && m->n_leaves <= (1 << 24), "%s: n_leaves must be a power of two <= 2^24, got %d",
                 what, m->n_leaves);
  CUROBO_REQUIRE((int64_t)m->n_leaves * m->leaf_size >= m->n_tri, "%s: %d leaves of %d triangles do not hold %d triangles", what,
                 m->n_leaves, m->leaf_size, m->n_tri);
  return CUROBO_HIP_OK;
}

CUROBO_EXPORT int curobo_hip_pose_sdf_evaluate(float *out_distance, float *out_gradient, int32_t *out_valid, void *workspace,
                                               int64_t workspace_bytes, const float *points, const float *position,
                                               const float *quaternion, const curobo_hip_mesh *mesh, float max_distance,
                                               float distance_threshold, int use_huber, float huber_delta, int n_points,
                                               curobo_hip_stream_t stream) {
  const char *what = "pose_sdf_evaluate";
  CUROBO_REQUIRE(points && position && quaternion && workspace, "%s: points, position, quaternion and workspace must not be null", what);
  CUROBO_REQUIRE(n_points > 0, "%s: n_points must be positive, got %d", what, n_points);
  if (int rc = check_pose_mesh(mesh, what)) return rc;
  CUROBO_REQUIRE(max_distance > 0.0f && distance_threshold > 0.0f, "%s: max_distance and distance_threshold must be positive", what);
  CUROBO_REQUIRE(use_huber == 0 || huber_delta > 0.0f, "%s: huber_delta must be positive, got %g", what, (double)huber_delta);
  if (int rc = check_sdf_workspace(workspace, workspace_bytes, n_points, what)) return rc;
  PoseEvalArgs a{};
  a.points = points, a.position = position, a.quaternion = quaternion, a.mesh = *mesh;
  a.max_distance = max_distance, a.distance_threshold = distance_threshold, a.huber_delta = huber_delta;
  a.use_huber = use_huber != 0, a.n = n_points;
  a.out_distance = out_distance, a.out_gradient = out_gradient, a.out_valid = out_valid, a.ws = (float *)workspace;
  hipLaunchKernelGGL(pose_sdf_evaluate_kernel, dim3((unsigned)pose_rows(n_points)), dim3(kPoseThreads), 0, (hipStream_t)stream, a);
  return check_launch(what, (hipStream_t)stream);
}

CUROBO_EXPORT int curobo_hip_pose_lm_step(curobo_hip_pose_lm_state *state, const void *workspace, int64_t workspace_bytes, int n_points,
                                          int mode, float lambda_initial, float lambda_factor, float lambda_min, float lambda_max,
                                          float rho_min, int minimum_valid_count, curobo_hip_stream_t stream) {
  const char *what = "pose_lm_step";
  CUROBO_REQUIRE(state && workspace, "%s: state and workspace must not be null", what);
  CUROBO_REQUIRE(((uintptr_t)state & 3) == 0 && ((uintptr_t)workspace & 3) == 0, "%s: state and workspace must be 4-byte aligned", what);
  CUROBO_REQUIRE(n_points > 0, "%s: n_points must be positive, got %d", what, n_points);
  CUROBO_REQUIRE(mode == CUROBO_HIP_POSE_LM_INIT || mode == CUROBO_HIP_POSE_LM_UPDATE, "%s: mode must be 0 (initial) or 1 (update), got %d", what,
                 mode);
  CUROBO_REQUIRE(lambda_factor > 0.0f && lambda_min > 0.0f && lambda_max >= lambda_min && lambda_initial > 0.0f,
                 "%s: lambda_initial, lambda_factor and lambda_min must be positive and lambda_max >= lambda_min", what);
  if (int rc = check_sdf_workspace(workspace, workspace_bytes, n_points, what)) return rc;
  PoseStepArgs a{};
  a.s = state, a.ws = (const float *)workspace, a.n_rows = pose_rows(n_points), a.mode = mode;
  a.lambda_initial = lambda_initial, a.lambda_factor = lambda_factor, a.lambda_min = lambda_min, a.lambda_max = lambda_max;
  a.rho_min = rho_min, a.minimum_valid_count = minimum_valid_count;
  hipLaunchKernelGGL(pose_lm_step_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, a);
  return check_launch(what, (hipStream_t)stream);
}
