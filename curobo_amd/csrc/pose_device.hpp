// pose_device.hpp -- what the pose estimators share (pose_detect.hip: mesh-SDF Levenberg-Marquardt; pose_icp.hip:
// point-to-plane ICP).  Both accumulate one row of partial sums per workgroup, add the rows in workgroup order in a
// one-wavefront step kernel, and solve a damped 6 x 6 system there.  The row, its assembly, its sum, its unpacking and the solve
// are stated here once; everything that belongs to one estimator stays in its unit.
//
// Determinism.  Nothing adds with atomics: a wavefront sums by the DPP ladder (common.hpp::wave_sum), a workgroup stores its own
// row, the step adds the rows in workgroup order.  Every row of a running evaluation is written by every launch, so nothing is
// zeroed between iterations and a captured block of iterations is a plain chain of kernel nodes.
#pragma once
#include "common.hpp"

namespace curobo_hip {

// ---- the row (include/curobo_hip.h): words 0..20 the upper triangle of sum a b^T (row major), 21..26 sum a * residual, 27 one
// scalar sum (floats), 28 the valid count (int32), the rest 0
constexpr int kPoseRow = CUROBO_HIP_POSE_WS_ROW;
constexpr int kPoseSums = 28, kPoseCount = 28;
static_assert(kPoseRow >= kPoseCount + 1 && kPoseRow <= kWave, "a row holds 28 sums and the count, one word per lane");

inline int64_t pose_ws_bytes(int64_t n_rows) { return n_rows * kPoseRow * (int64_t)sizeof(float); }

// the workspace holds n_rows rows and is 4-byte aligned; `counted` says what the rows were counted from ("300 points"), `query`
// names the entry point that gives the size
inline int check_pose_workspace(const void *workspace, int64_t workspace_bytes, int64_t n_rows, const char *what, const char *counted,
                                const char *query) {
  CUROBO_REQUIRE(workspace_bytes >= pose_ws_bytes(n_rows), "%s: workspace of %lld bytes, %s need %lld (%s)", what, (long long)workspace_bytes,
                 counted, (long long)pose_ws_bytes(n_rows), query);
  CUROBO_REQUIRE(((uintptr_t)workspace & 3) == 0, "%s: workspace must be 4-byte aligned", what);
  return CUROBO_HIP_OK;
}

// quotient and root rounded once (the library is built with the 2.5 ulp hardware forms; the LM damping must follow the
// reference's lambda / factor bit for bit, and a double quotient of two floats rounds to the correctly rounded float)
__device__ __forceinline__ float div_rn(float x, float y) { return (float)((double)x / (double)y); }
__device__ __forceinline__ float sqrt_rn(float x) { return (float)sqrt((double)x); }

// One wavefront's row of the lanes' terms: lane k returns word k (0 from word 29 on).  Called by every lane of the wavefront;
// a lane without a term passes zeros and valid = false.  The products are a[u] * b[v] and a[u] * residual, as written.
__device__ __forceinline__ float pose_row_word(const float (&a)[6], const float (&b)[6], float residual, float scalar, bool valid, int lane) {
  float mine = 0.0f;
  int k = 0;
#pragma unroll
  for (int u = 0; u < 6; u++) {
#pragma unroll
    for (int v = u; v < 6; v++) {
      const float sum = wave_sum(a[u] * b[v]);
      if (lane == k) mine = sum;
      k++;
    }
  }
#pragma unroll
  for (int u = 0; u < 6; u++) {
    const float sum = wave_sum(a[u] * residual);
    if (lane == 21 + u) mine = sum;
  }
  const float sum = wave_sum(scalar);
  if (lane == 27) mine = sum;
  const int c = __popcll(__ballot(valid));
  if (lane == kPoseCount) mine = __int_as_float(c);
  return mine;
}

// The rows of one evaluation added in order into red[kPoseRow] (LDS), by one wavefront: lane k < 28 adds word k as floats, lane
// 28 the counts as integers; the barrier follows, so every lane may read red[0..28] on return.
__device__ __forceinline__ void pose_sum_rows(float *red, const float *rows, int n_rows, int lane) {
  if (lane < kPoseSums) {
    float s = 0.0f;
    for (int r = 0; r < n_rows; r++) s += rows[(size_t)r * kPoseRow + lane];
    red[lane] = s;
  } else if (lane == kPoseCount) {
    int c = 0;
    for (int r = 0; r < n_rows; r++) c += __float_as_int(rows[(size_t)r * kPoseRow + lane]);
    red[lane] = __int_as_float(c);
  }
  __syncthreads();
}

// words 0..20 -> the symmetric 6 x 6, row major
__device__ __forceinline__ void pose_unpack_symmetric(const float *row, float *A) {
  int k = 0;
  for (int u = 0; u < 6; u++)
    for (int v = u; v < 6; v++) { A[u * 6 + v] = row[k]; A[v * 6 + u] = row[k]; k++; }
}

// (A + diag I) x = +-rhs by Cholesky in fp32, quotients and roots rounded once.  The two estimators differ, each as its reference
// does, and the caller picks:
//   kPoseSolveLM   x solves against -rhs (solve_lm_step); false only on a pivot that is not positive -- an infinite pivot and a
//                  solution that is not finite pass (the trust region rejects the candidate they give)
//   kPoseSolveICP  x solves against rhs; false also on a pivot or a solution that is not finite (the hypothesis stops)
enum PoseSolveRule { kPoseSolveLM, kPoseSolveICP };

template <PoseSolveRule RULE>
__device__ __forceinline__ bool pose_solve6(const float *A, float diag, const float *rhs, float *x) {
  float L[6][6];
  for (int i = 0; i < 6; i++) {
    for (int c = 0; c <= i; c++) {
      float acc = A[i * 6 + c] + (i == c ? diag : 0.0f);
      for (int k = 0; k < c; k++) acc -= L[i][k] * L[c][k];
      if (i == c) {
        if (!(acc > 0.0f) || (RULE == kPoseSolveICP && !isfinite(acc))) return false;
        L[i][i] = sqrt_rn(acc);
      } else {
        L[i][c] = div_rn(acc, L[c][c]);
      }
    }
  }
  float y[6];
  for (int i = 0; i < 6; i++) {
    float acc = RULE == kPoseSolveLM ? -rhs[i] : rhs[i];
    for (int k = 0; k < i; k++) acc -= L[i][k] * y[k];
    y[i] = div_rn(acc, L[i][i]);
  }
  for (int i = 5; i >= 0; i--) {
    float acc = y[i];
    for (int k = i + 1; k < 6; k++) acc -= L[k][i] * x[k];
    x[i] = div_rn(acc, L[i][i]);
  }
  if (RULE == kPoseSolveICP)
    for (int i = 0; i < 6; i++)
      if (!isfinite(x[i])) return false;
  return true;
}

}  // namespace curobo_hip
