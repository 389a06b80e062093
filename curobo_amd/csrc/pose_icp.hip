// pose_icp.hip -- point-to-plane ICP with Huber weights (curobo_amd/perception/pose_estimation/pose_detector.py), every
// hypothesis of a stage advancing together, one iteration in two launches:
//   curobo_hip_pose_icp_correspond  mesh samples of every hypothesis at its pose against the observed points: the nearest
//                                   observed point by brute force, validity against the threshold, the weighted Jacobian
//                                   row, and per workgroup one row of partial sums of J^T W J (upper triangle), J^T W b, the
//                                   sum of nearest distances and the valid count
//   curobo_hip_pose_icp_step        one wavefront per hypothesis: the rows summed in workgroup order, the 6 x 6 Cholesky
//                                   solve, T <- T_update T, the stops of the reference's loops; or, in finalize mode, the error
//   curobo_hip_pose_icp_select      the arg-min of the hypotheses' errors, lowest index first
//
// Reference: perception/pose_estimation/pose_detector.py (_icp_coarse :172-283, _icp_fine :285-375), which runs the
// hypotheses one after the other with about fifteen torch launches per iteration, and util.py (find_nearest_neighbors :88-113,
// compute_pose_point_to_plane_cholesky :245-330, omega_to_quaternion :49-66).
//
// The row of partial sums, its sum in workgroup order, the Cholesky solve and the rules that make all of it deterministic:
// pose_device.hpp.  The nearest point is the minimum of (squared distance, index) in that order, which does
// not depend on how the observed range is shared out: 64 samples per workgroup, each wavefront scanning a quarter of every
// staged tile, the four candidates met in LDS.
#include "pose_device.hpp"

namespace curobo_hip {

constexpr int kIcpThreads = 256, kIcpWaves = kIcpThreads / kWave;
constexpr int kIcpSamples = kWave;                   // mesh samples per workgroup: lane l of every wavefront owns sample l
constexpr int kIcpTile = 1024;                       // observed points staged per pass (16 KB of LDS)
constexpr int kIcpSlice = kIcpTile / kIcpWaves;      // of which one wavefront scans this many
constexpr int kIcpMinValid = 10;                     // pose_detector.py:237 / :331
constexpr float kIcpDamping = 1e-6f;                 // util.py:252
static_assert(sizeof(curobo_hip_pose_icp_state) == 4 * CUROBO_HIP_POSE_ICP_STATE_WORDS, "state layout");

struct IcpCorrespondArgs {
  const float *mesh_points, *mesh_normals, *observed;
  const curobo_hip_pose_icp_state *state;
  float distance_threshold, huber_delta;
  int use_huber, honour_stopped, n_mesh, n_observed, rows_per_hypothesis;
  int32_t *out_index;
  float *out_distance;
  float *ws;
};

__global__ __launch_bounds__(kIcpThreads) void pose_icp_correspond_kernel(IcpCorrespondArgs a) {
  __shared__ float4 tile[kIcpTile];
  __shared__ float cand_d2[kIcpWaves][kIcpSamples];
  __shared__ int cand_idx[kIcpWaves][kIcpSamples];
  const int h = blockIdx.y, tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
  const curobo_hip_pose_icp_state &st = a.state[h];
  if (a.honour_stopped && st.stopped != 0) return;  // (uniform over the workgroup)
  const int i = blockIdx.x * kIcpSamples + lane;
  const bool live = i < a.n_mesh;
  const float *T = st.T;
  f3 s = make_f3(0.f, 0.f, 0.f);
  if (live) {
    const f3 p = make_f3(a.mesh_points[(size_t)i * 3], a.mesh_points[(size_t)i * 3 + 1], a.mesh_points[(size_t)i * 3 + 2]);
    s = make_f3(T[0] * p.x + T[1] * p.y + T[2] * p.z + T[3], T[4] * p.x + T[5] * p.y + T[6] * p.z + T[7],
                T[8] * p.x + T[9] * p.y + T[10] * p.z + T[11]);
  }
  // ---- the nearest observed point: strictly smaller squared distance wins, so within a slice the lowest index is kept
  float best = __builtin_inff();
  int best_j = -1;
  for (int base = 0; base < a.n_observed; base += kIcpTile) {
    const int count = min(kIcpTile, a.n_observed - base);
    __syncthreads();
    for (int k = tid; k < count; k += kIcpThreads) {
      const float *o = a.observed + (size_t)(base + k) * 3;
      tile[k] = make_float4(o[0], o[1], o[2], 0.f);
    }
    __syncthreads();
    const int lo = wave * kIcpSlice, hi = min(lo + kIcpSlice, count);
#pragma unroll 4
    for (int k = lo; k < hi; k++) {
      const float4 o = tile[k];  // (one address per wavefront: a broadcast)
      const float dx = o.x - s.x, dy = o.y - s.y, dz = o.z - s.z;
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (d2 < best) { best = d2; best_j = base + k; }
    }
  }
  cand_d2[wave][lane] = best;
  cand_idx[wave][lane] = best_j;
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int w = 1; w < kIcpWaves; w++) {
    const float d2 = cand_d2[w][lane];
    const int j = cand_idx[w][lane];
    if (j >= 0 && (d2 < best || (d2 == best && j < best_j) || best_j < 0)) { best = d2; best_j = j; }
  }
  // ---- the sample's row of the normal equations (util.py:279-307)
  float j6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, b = 0.f, wgt = 0.f, dist = 0.f;
  const bool found = live && best_j >= 0;
  bool valid = false;
  if (found) {
    dist = sqrt_rn(best);
    valid = dist <= a.distance_threshold;
    if (valid) {
      const f3 n = make_f3(a.mesh_normals[(size_t)i * 3], a.mesh_normals[(size_t)i * 3 + 1], a.mesh_normals[(size_t)i * 3 + 2]);
      const f3 nr = make_f3(T[0] * n.x + T[1] * n.y + T[2] * n.z, T[4] * n.x + T[5] * n.y + T[6] * n.z, T[8] * n.x + T[9] * n.y + T[10] * n.z);
      const float *op = a.observed + (size_t)best_j * 3;
      const f3 o = make_f3(op[0], op[1], op[2]);
      b = dot(o - s, nr);
      wgt = 1.0f;
      if (a.use_huber != 0 && !(fabsf(b) < a.huber_delta)) wgt = a.huber_delta / (fabsf(b) + 1e-10f);
      const f3 c = cross(s, nr);
      j6[0] = c.x; j6[1] = c.y; j6[2] = c.z; j6[3] = nr.x; j6[4] = nr.y; j6[5] = nr.z;
    }
  }
  if (live) {
    const size_t at = (size_t)h * a.n_mesh + i;
    if (a.out_index) a.out_index[at] = valid ? best_j : -1;
    if (a.out_distance) a.out_distance[at] = dist;
  }
  // ---- the workgroup's row: J^T W J, J^T W b, the sum of nearest distances, count
  const float wj6[6] = {wgt * j6[0], wgt * j6[1], wgt * j6[2], wgt * j6[3], wgt * j6[4], wgt * j6[5]};
  const float mine = pose_row_word(wj6, j6, b, dist, valid, lane);
  if (lane < kPoseRow) a.ws[((size_t)h * a.rows_per_hypothesis + blockIdx.x) * kPoseRow + lane] = mine;
}

// ---------------------------------------------------------------------------------------------------- the step
struct IcpStepArgs {
  curobo_hip_pose_icp_state *state;
  const float *ws;
  int rows_per_hypothesis, n_mesh, mode;
};

__global__ __launch_bounds__(kWave) void pose_icp_step_kernel(IcpStepArgs a) {
  __shared__ float red[kPoseRow];
  const int h = blockIdx.x, lane = threadIdx.x;
  curobo_hip_pose_icp_state &s = a.state[h];
  if (a.mode != CUROBO_HIP_POSE_ICP_FINALIZE && s.stopped != 0) return;
  pose_sum_rows(red, a.ws + (size_t)h * a.rows_per_hypothesis * kPoseRow, a.rows_per_hypothesis, lane);
  if (lane != 0) return;
  const int n_valid = __float_as_int(red[kPoseCount]);
  if (a.mode == CUROBO_HIP_POSE_ICP_FINALIZE) {  // errors.mean() over every sample (pose_detector.py:265-274)
    s.error = n_valid > 0 ? div_rn(red[27], (float)a.n_mesh) : __builtin_inff();
    return;
  }
  s.iterations += 1;  // iter_idx + 1 of the iteration now running
  s.n_valid = n_valid;
  if (n_valid < kIcpMinValid) { s.stopped = 1; return; }
  float A[36], x[6];
  pose_unpack_symmetric(red, A);
  // (J^T W J + damping I) x = J^T W b
  if (!pose_solve6<kPoseSolveICP>(A, kIcpDamping, red + 21, x)) { s.stopped = 1; s.solver_failed = 1; return; }
  for (int k = 0; k < 6; k++) s.x[k] = x[k];
  if (a.mode == CUROBO_HIP_POSE_ICP_FINE && sqrt_rn(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]) < 1e-4f) { s.stopped = 1; return; }
  // omega_to_quaternion, then the quaternion's matrix
  const float theta = sqrt_rn(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  const float coeff = div_rn(sinf(0.5f * theta), fmaxf(theta, 1e-10f));
  const float qw = cosf(0.5f * theta), qx = x[0] * coeff, qy = x[1] * coeff, qz = x[2] * coeff;
  const float U[9] = {1.0f - 2.0f * (qy * qy + qz * qz), 2.0f * (qx * qy - qz * qw), 2.0f * (qx * qz + qy * qw),
                      2.0f * (qx * qy + qz * qw), 1.0f - 2.0f * (qx * qx + qz * qz), 2.0f * (qy * qz - qx * qw),
                      2.0f * (qx * qz - qy * qw), 2.0f * (qy * qz + qx * qw), 1.0f - 2.0f * (qx * qx + qy * qy)};
  float Tn[12];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 4; c++) Tn[r * 4 + c] = U[r * 3] * s.T[c] + U[r * 3 + 1] * s.T[4 + c] + U[r * 3 + 2] * s.T[8 + c];
    Tn[r * 4 + 3] += x[3 + r];
  }
  for (int k = 0; k < 12; k++) s.T[k] = Tn[k];
}

// ---------------------------------------------------------------------------------------------------- the winner
struct IcpSelectArgs {
  const curobo_hip_pose_icp_state *state;
  int n_hypotheses;
  int32_t *out_index;
  float *out_error, *out_T;
};

__global__ __launch_bounds__(kWave) void pose_icp_select_kernel(IcpSelectArgs a) {
  const int lane = threadIdx.x;
  float best = __builtin_inff();
  int best_h = a.n_hypotheses;  // "none": loses every tie
  for (int h = lane; h < a.n_hypotheses; h += kWave) {
    const float e = a.state[h].error;
    if (e < best) { best = e; best_h = h; }  // (false for a NaN)
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const float e = __shfl_xor(best, off, kWave);
    const int h = __shfl_xor(best_h, off, kWave);
    if (e < best || (e == best && h < best_h)) { best = e; best_h = h; }
  }
  if (best_h >= a.n_hypotheses) best_h = 0;  // nothing finite: the reference keeps hypothesis 0
  if (lane == 0) {
    *a.out_index = best_h;
    if (a.out_error) *a.out_error = best;
  }
  if (a.out_T && lane < 12) a.out_T[lane] = a.state[best_h].T[lane];
}

}  // namespace curobo_hip

using namespace curobo_hip;

static int icp_rows(int n_mesh) { return ceil_div(n_mesh, kIcpSamples); }
static int64_t icp_ws_rows(int n_hypotheses, int n_mesh) { return (int64_t)n_hypotheses * icp_rows(n_mesh); }

static int check_icp_counts(int n_hypotheses, int n_mesh, const char *what) {
  CUROBO_REQUIRE(n_hypotheses > 0 && n_hypotheses <= 65535, "%s: n_hypotheses must be in 1..65535, got %d", what, n_hypotheses);
  CUROBO_REQUIRE(n_mesh > 0, "%s: n_mesh must be positive, got %d", what, n_mesh);
  return CUROBO_HIP_OK;
}

CUROBO_EXPORT int curobo_hip_pose_icp_ws_bytes(int n_hypotheses, int n_mesh, int64_t *out_bytes) {
  const char *what = "pose_icp_ws_bytes";
  CUROBO_REQUIRE(out_bytes, "%s: out_bytes must not be null", what);
  if (int rc = check_icp_counts(n_hypotheses, n_mesh, what)) return rc;
  *out_bytes = pose_ws_bytes(icp_ws_rows(n_hypotheses, n_mesh));
  return CUROBO_HIP_OK;
}

static int check_icp_workspace(const void *workspace, int64_t workspace_bytes, int n_hypotheses, int n_mesh, const char *what) {
  char counted[64];
  snprintf(counted, sizeof counted, "%d hypotheses of %d samples", n_hypotheses, n_mesh);
  return check_pose_workspace(workspace, workspace_bytes, icp_ws_rows(n_hypotheses, n_mesh), what, counted, "curobo_hip_pose_icp_ws_bytes");
}

CUROBO_EXPORT int curobo_hip_pose_icp_correspond(int32_t *out_index, float *out_distance, void *workspace, int64_t workspace_bytes,
                                                 const float *mesh_points, const float *mesh_normals, const float *observed_points,
                                                 const curobo_hip_pose_icp_state *state, float distance_threshold, int use_huber,
                                                 float huber_delta, int honour_stopped, int n_hypotheses, int n_mesh, int n_observed,
                                                 curobo_hip_stream_t stream) {
  const char *what = "pose_icp_correspond";
  CUROBO_REQUIRE(mesh_points && mesh_normals && observed_points && state && workspace,
                 "%s: mesh_points, mesh_normals, observed_points, state and workspace must not be null", what);
  if (int rc = check_icp_counts(n_hypotheses, n_mesh, what)) return rc;
  CUROBO_REQUIRE(n_observed > 0, "%s: n_observed must be positive, got %d", what, n_observed);
  CUROBO_REQUIRE(distance_threshold > 0.0f, "%s: distance_threshold must be positive (infinity allowed), got %g", what,
                 (double)distance_threshold);
  CUROBO_REQUIRE(use_huber == 0 || huber_delta > 0.0f, "%s: huber_delta must be positive, got %g", what, (double)huber_delta);
  if (int rc = check_icp_workspace(workspace, workspace_bytes, n_hypotheses, n_mesh, what)) return rc;
  CUROBO_REQUIRE(((uintptr_t)state & 3) == 0, "%s: state must be 4-byte aligned", what);
  IcpCorrespondArgs a{};
  a.mesh_points = mesh_points, a.mesh_normals = mesh_normals, a.observed = observed_points, a.state = state;
  a.distance_threshold = distance_threshold, a.huber_delta = huber_delta, a.use_huber = use_huber != 0;
  a.honour_stopped = honour_stopped != 0, a.n_mesh = n_mesh, a.n_observed = n_observed, a.rows_per_hypothesis = icp_rows(n_mesh);
  a.out_index = out_index, a.out_distance = out_distance, a.ws = (float *)workspace;
  hipLaunchKernelGGL(pose_icp_correspond_kernel, dim3((unsigned)icp_rows(n_mesh), (unsigned)n_hypotheses), dim3(kIcpThreads), 0,
                     (hipStream_t)stream, a);
  return check_launch(what, (hipStream_t)stream);
}

CUROBO_EXPORT int curobo_hip_pose_icp_step(curobo_hip_pose_icp_state *state, const void *workspace, int64_t workspace_bytes,
                                           int n_hypotheses, int n_mesh, int mode, curobo_hip_stream_t stream) {
  const char *what = "pose_icp_step";
  CUROBO_REQUIRE(state && workspace, "%s: state and workspace must not be null", what);
  CUROBO_REQUIRE(((uintptr_t)state & 3) == 0, "%s: state must be 4-byte aligned", what);
  if (int rc = check_icp_counts(n_hypotheses, n_mesh, what)) return rc;
  CUROBO_REQUIRE(mode == CUROBO_HIP_POSE_ICP_COARSE || mode == CUROBO_HIP_POSE_ICP_FINE || mode == CUROBO_HIP_POSE_ICP_FINALIZE,
                 "%s: mode must be 0 (coarse), 1 (fine) or 2 (finalize), got %d", what, mode);
  if (int rc = check_icp_workspace(workspace, workspace_bytes, n_hypotheses, n_mesh, what)) return rc;
  IcpStepArgs a{};
  a.state = state, a.ws = (const float *)workspace, a.rows_per_hypothesis = icp_rows(n_mesh), a.n_mesh = n_mesh, a.mode = mode;
  hipLaunchKernelGGL(pose_icp_step_kernel, dim3((unsigned)n_hypotheses), dim3(kWave), 0, (hipStream_t)stream, a);
  return check_launch(what, (hipStream_t)stream);
}

CUROBO_EXPORT int curobo_hip_pose_icp_select(int32_t *out_index, float *out_error, float *out_transform,
                                             const curobo_hip_pose_icp_state *state, int n_hypotheses, curobo_hip_stream_t stream) {
  const char *what = "pose_icp_select";
  CUROBO_REQUIRE(out_index && state, "%s: out_index and state must not be null", what);
  CUROBO_REQUIRE(n_hypotheses > 0, "%s: n_hypotheses must be positive, got %d", what, n_hypotheses);
  IcpSelectArgs a{};
  a.state = state, a.n_hypotheses = n_hypotheses, a.out_index = out_index, a.out_error = out_error, a.out_T = out_transform;
  hipLaunchKernelGGL(pose_icp_select_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, a);
  return check_launch(what, (hipStream_t)stream);
}
