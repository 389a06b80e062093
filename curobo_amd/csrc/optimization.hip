// optimization.hip -- fused L-BFGS direction update and Wolfe line search bookkeeping, plus the
// per-trajectory cost reduction used by the rollout.
// Reference: kernels/optimization/lbfgs/lbfgs_step_kernel.cuh:18-199 (+ lbfgs_step_helpers.cuh),
// kernels/optimization/line_search/line_search_kernel.cuh:27-155 (+ line_search_helpers.cuh),
// rollout/metrics.py:233-265 / util/tensor_util.py:104 (cat_sum).
//
// gfx950 design: the reference gives one problem to one CUDA block of V threads and pays
// 2m+2 block-wide reductions (shared memory + __syncthreads each).  On CDNA4 a problem is owned
// by ONE wavefront: each lane keeps ceil(V/64) components of the running vector in registers,
// every dot product is a wave64 butterfly (no LDS, no barrier), and 4 problems share a
// 256-thread workgroup so that 256 problems still fill 64 CUs.  History rows are streamed from
// L2 in [m][B][V] order (coalesced 256 B per wave-instruction); the shift-by-one of the
// history is done in the same pass that reads it, as in the reference.
#include <cstdlib>

#include "common.hpp"
#include "tail_shapes.hpp"

namespace curobo_hip {

// Every multiply-add of the reductions and updates below is an explicit fma: left to -ffp-contract the same
// source line becomes v_fma in one kernel and v_pk_mul + v_add in another (the vectoriser decides per context),
// and the one-launch and three-launch forms of an iteration would then differ in the last bit.
constexpr int kMaxVPL = 16;  // components per lane -> v_dim <= 1024 (reference: V < 1024)

struct LbfgsArgs {
  float *step_vec, *rho_buffer, *y_buffer, *s_buffer;
  const float *q, *grad_q;
  float *x_0, *grad_0;
  float epsilon;
  int batch, m, v_dim, stable_mode;
};

template <int VPL>
__global__ void __launch_bounds__(256) lbfgs_step_kernel(const LbfgsArgs a) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int b = blockIdx.x * (blockDim.x / kWave) + wave;
  if (b >= a.batch) return;  // whole wave exits together
  const int V = a.v_dim, m = a.m, B = a.batch;
  const size_t bv = (size_t)b * V;
  const size_t hist_stride = (size_t)B * V;
  float gq[VPL], y[VPL], s[VPL];
  float part = 0.0f;
  // ---- load state, form (y, s), update (x_0, grad_0): lbfgs_step_helpers.cuh:37-70
#pragma unroll
  for (int e = 0; e < VPL; e++) {
    const int v = lane + e * kWave;
    gq[e] = y[e] = s[e] = 0.0f;
    if (v < V) {
      const float g = a.grad_q[bv + v], x = a.q[bv + v];
      y[e] = g - a.grad_0[bv + v];
      s[e] = x - a.x_0[bv + v];
      a.grad_0[bv + v] = g;
      a.x_0[bv + v] = x;
      gq[e] = g;
      part = __builtin_fmaf(y[e], s[e], part);
    }
  }
  const float numerator = wave_sum(part);
  // ---- shift history by one and append (y, s): :89-150; rho likewise: :213-240
  for (int i = 0; i < m - 1; i++) {
#pragma unroll
    for (int e = 0; e < VPL; e++) {
      const int v = lane + e * kWave;
      if (v < V) {
        a.y_buffer[i * hist_stride + bv + v] = a.y_buffer[(i + 1) * hist_stride + bv + v];
        a.s_buffer[i * hist_stride + bv + v] = a.s_buffer[(i + 1) * hist_stride + bv + v];
      }
    }
  }
  if (m > 0) {
#pragma unroll
    for (int e = 0; e < VPL; e++) {
      const int v = lane + e * kWave;
      if (v < V) {
        a.y_buffer[(size_t)(m - 1) * hist_stride + bv + v] = y[e];
        a.s_buffer[(size_t)(m - 1) * hist_stride + bv + v] = s[e];
      }
    }
  }
  // rho: lanes 0..m-1 each own one history slot (m <= 31 < 64)
  float rho_mine = 0.0f;
  if (lane < m) {
    if (lane < m - 1) rho_mine = a.rho_buffer[(size_t)(lane + 1) * B + b];
    else {
      rho_mine = 1.0f / numerator;
      if (a.stable_mode && numerator <= 0.0f) rho_mine = 0.0f;
    }
    a.rho_buffer[(size_t)lane * B + b] = rho_mine;
  }
  // ---- two-loop recursion.  alpha_i lives in lane i.
  float alpha_mine = 0.0f;
  for (int i = m - 1; i >= 0; i--) {  // backward pass, :262-330
    float d = 0.0f;
    float yi[VPL];
#pragma unroll
    for (int e = 0; e < VPL; e++) {
      const int v = lane + e * kWave;
      yi[e] = 0.0f;
      if (v < V) {
        d = __builtin_fmaf(gq[e], a.s_buffer[i * hist_stride + bv + v], d);
        yi[e] = a.y_buffer[i * hist_stride + bv + v];
      }
    }
    d = wave_sum(d);
    const float alpha = d * __shfl(rho_mine, i, kWave);
    if (lane == i) alpha_mine = alpha;
#pragma unroll
    for (int e = 0; e < VPL; e++) gq[e] = __builtin_fmaf(-alpha, yi[e], gq[e]);
  }
  if (m > 0) {  // scaling gamma = relu(s.y / y.y), :346-373
    float d = 0.0f;
#pragma unroll
    for (int e = 0; e < VPL; e++) d = __builtin_fmaf(y[e], y[e], d);
    d = wave_sum(d);
    float var1 = numerator / d;
    if (a.stable_mode && (isinf(var1) || isnan(var1))) var1 = a.epsilon;
    const float gamma = var1 < 0.0f ? 0.0f : var1;
#pragma unroll
    for (int e = 0; e < VPL; e++) gq[e] = gamma * gq[e];
  }
  for (int i = 0; i < m; i++) {  // forward pass, :396-470
    float d = 0.0f;
    float si[VPL];
#pragma unroll
    for (int e = 0; e < VPL; e++) {
      const int v = lane + e * kWave;
      si[e] = 0.0f;
      if (v < V) {
        d = __builtin_fmaf(gq[e], a.y_buffer[i * hist_stride + bv + v], d);
        si[e] = a.s_buffer[i * hist_stride + bv + v];
      }
    }
    d = wave_sum(d);
    const float beta = __builtin_fmaf(-d, __shfl(rho_mine, i, kWave), __shfl(alpha_mine, i, kWave));
#pragma unroll
    for (int e = 0; e < VPL; e++) gq[e] = __builtin_fmaf(beta, si[e], gq[e]);
  }
#pragma unroll
  for (int e = 0; e < VPL; e++) {
    const int v = lane + e * kWave;
    if (v < V) a.step_vec[bv + v] = -gq[e];
  }
}

// Register-resident variant for the common sizes (V <= 128, m <= 32: trajopt V=84/m=27, IK
// V=7/m=7).  The whole (y, s) history of a problem is pulled into VGPRs with independent,
// fully pipelined loads (VPL * 2 * 32 <= 128 registers), written back shifted by one, and both
// loops of the recursion then run out of registers: the 2m dependent L2 round trips of the
// streaming variant above disappear.  m is a run-time value; slots >= m are predicated off.
__device__ __forceinline__ float lane_bcast(float v, int src_lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src_lane));
}

// A problem is owned by a lane GROUP: the whole wavefront (G = 64), or one 16-lane DPP row (G = 16,
// four problems per wavefront) for small problems such as IK (opt_dim 7): the reductions of a row
// are the first four steps of the wavefront ladder, so both group sizes produce the same bits.
template <int G>
__device__ __forceinline__ float gsum(float v) { return G == kWave ? wave_sum(v) : row16_sum(v); }
template <int G>
__device__ __forceinline__ float gbcast(float v, int i) { return G == kWave ? lane_bcast(v, i) : __shfl(v, i, G); }
template <int G>
__device__ __forceinline__ unsigned long long gballot(bool p) {
  const unsigned long long m = __ballot(p);
  return G == kWave ? m : (m >> (__lane_id() & 48)) & 0xffffull;
}

// The (y, s, rho) history of one problem plus its previous iterate, as one lane group holds it in VGPRs
// (separate arrays, not a struct: a struct this size stays an alloca and lands in scratch).
// S = a TailShape (tail_shapes.hpp) sizes the arrays for exactly its m slots, TailShapeDyn for the largest history.
template <int G, class S = TailShapeDyn>
struct LbfgsLimits {
  static constexpr int MMAX = S::kStatic ? (S::kM > 0 ? S::kM : 1) : (G == kWave ? 32 : 16);
};
#define LBFGS_HISTORY_DECL(VPL, G, S) \
  float h_ys[LbfgsLimits<G, S>::MMAX][VPL], h_ss[LbfgsLimits<G, S>::MMAX][VPL], h_g0[VPL], h_x0[VPL], h_rho
#define LBFGS_HISTORY_PARAMS(VPL, G, S)                                                                          \
  float (&h_ys)[LbfgsLimits<G, S>::MMAX][VPL], float (&h_ss)[LbfgsLimits<G, S>::MMAX][VPL], float (&h_g0)[VPL], \
      float (&h_x0)[VPL], float &h_rho
#define LBFGS_HISTORY_ARGS h_ys, h_ss, h_g0, h_x0, h_rho

// Row addressing.  A row of a [.][B][V] array is named by a wave-uniform 64-bit base (array + slot * B V, + b V where the
// problem index is wave-uniform: the 64-lane forms) and a per-lane byte offset that is computed once per element of the
// lane, not once per row: OFF = uint32_t makes every access `global_load_dword v, v_off, s[base:base+1]` (one scalar add
// per row instead of a 64-bit multiply-add and shifts per lane and row).  In the 16-lane row form the problem differs per
// row of lanes and goes into the lane offset: the host takes uint32_t there only when the largest offset fits 31 bits
// (tail_offsets_fit).  OFF = size_t is the 64-bit per-lane address of the three-launch kernels.
template <typename T, typename OFF>
__device__ __forceinline__ T &row_at(T *row, OFF off_bytes) {
  return *(T *)((const char *)row + off_bytes);
}
// The scalar-base form is matched per basic block: base + zext(offset) has to be formed in the block of the access, and
// the zext of an offset computed in a dominating block is hoisted there (the access then pays a 64-bit VALU add).  A
// block of several accesses therefore takes an opaque copy of its lane offset first: one v_mov for the block.
template <typename OFF>
__device__ __forceinline__ OFF block_offset(OFF off) {
  if constexpr (sizeof(OFF) == 4) asm volatile("" : "+v"(off));
  return off;
}
// A wave-uniform zero the optimiser cannot see through: row bases formed from `array + fresh_zero()` are computed where
// they are used.  Without it the write-back of the history reuses the ~4 m row bases of the loads, which then stay live
// across the whole recursion: more SGPRs than a wavefront has, spilled to VGPR lanes (a v_writelane and a v_readlane
// each, against two scalar adds).  (An integer, not the pointer: a pointer through asm comes back as a flat address.)
__device__ __forceinline__ size_t fresh_zero() {
  int z = 0;
  asm volatile("" : "+s"(z));
  return (size_t)(unsigned)z;
}
template <int G>
__device__ __forceinline__ int uniform_part(int b) { return G == kWave ? b : 0; }
template <int G, typename OFF>
__device__ __forceinline__ OFF lane_part(int b) { return G == kWave ? (OFF)0 : (OFF)b; }
// byte offset of element min(lane + e G, V - 1) of the [row_len]-float row of problem b
template <int G, typename OFF>
__device__ __forceinline__ OFF lane_offset(int b, int lane, int e, int V, int row_len) {
  const int v = lane + e * G, vc = v < V ? v : V - 1;
  return (lane_part<G, OFF>(b) * (OFF)row_len + (OFF)vc) * (OFF)sizeof(float);
}

// v & mask with a mask the optimiser cannot see through.  Out-of-range lanes load from a clamped address and
// are zeroed with this: written as `in_range ? load : 0` the compiler moves each load under its own branch
// (an exec-mask region per load, or worse a wait per load), and ~4 m loads that should leave as one burst
// trickle out between branches.
__device__ __forceinline__ int opaque_lane_mask(bool in_range) {
  int mk = in_range ? -1 : 0;
  asm volatile("" : "+v"(mk));
  return mk;
}
__device__ __forceinline__ float and_mask(float v, int mk) {
  return __builtin_bit_cast(float, __builtin_bit_cast(int, v) & mk);
}

// slot i <- old slot i+1 (the shift of the reference), every load independent of every other
template <int VPL, int G, class S, typename OFF>
__device__ __forceinline__ void lbfgs_history_load(const LbfgsArgs &a, int b, int lane, LBFGS_HISTORY_PARAMS(VPL, G, S)) {
  constexpr int MMAX = LbfgsLimits<G, S>::MMAX;
  const int V = S::kStatic ? S::kV : a.v_dim, m = S::kStatic ? S::kM : a.m, B = a.batch;
  const size_t bv = (size_t)uniform_part<G>(b) * V;
  const size_t hist_stride = (size_t)B * V;
  // Unconditional loads at clamped addresses: lanes past V are zeroed with the opaque mask; slots >= m-1 receive
  // a copy of the newest old slot, which nothing reads (slot m-1 is overwritten by the append, the recursion
  // stops at m).
  int mk[VPL];
  OFF off[VPL];
#pragma unroll
  for (int e = 0; e < VPL; e++) {
    mk[e] = opaque_lane_mask(lane + e * G < V);
    off[e] = lane_offset<G, OFF>(b, lane, e, V, V);
    h_g0[e] = and_mask(row_at(a.grad_0 + bv, off[e]), mk[e]);
    h_x0[e] = and_mask(row_at(a.x_0 + bv, off[e]), mk[e]);
  }
  if (m > 0) {
    if (!S::kStatic) {  // (a block of its own only where m is a run-time value)
#pragma unroll
      for (int e = 0; e < VPL; e++) off[e] = block_offset(off[e]);
    }
#pragma unroll
    for (int i = MMAX - 1; i >= 0; i--) {  // newest first: the order the recursion consumes them in
      if (S::kStatic && i >= m - 1) {  // (a shape knows which slots nothing reads)
#pragma unroll
        for (int e = 0; e < VPL; e++) h_ys[i][e] = h_ss[i][e] = 0.0f;
        continue;
      }
      const int slot = i + 1 < m ? i + 1 : m - 1;
      const float *yrow = a.y_buffer + (size_t)slot * hist_stride + bv, *srow = a.s_buffer + (size_t)slot * hist_stride + bv;
#pragma unroll
      for (int e = 0; e < VPL; e++) {
        h_ys[i][e] = and_mask(row_at(yrow, off[e]), mk[e]);
        h_ss[i][e] = and_mask(row_at(srow, off[e]), mk[e]);
      }
    }
    const int rl = lane + 1 < m ? lane + 1 : m - 1;
    h_rho = and_mask(a.rho_buffer[(size_t)rl * B + b], opaque_lane_mask(lane < m - 1));
  } else {
#pragma unroll
    for (int i = 0; i < MMAX; i++) {
#pragma unroll
      for (int e = 0; e < VPL; e++) h_ys[i][e] = h_ss[i][e] = 0.0f;
    }
    h_rho = 0.0f;
  }
}

// body for one problem b on one lane group; g_in / x_in = current gradient / iterate of the lane's
// elements (v = lane + e * G), dir_out = the new step direction (also stored to a.step_vec)
template <int VPL, int G, bool STORE_SHIFTED, class S, typename OFF>
__device__ __forceinline__ void lbfgs_step_from_history(const LbfgsArgs &a, int b, int lane, const float (&g_in)[VPL],
                                                        const float (&x_in)[VPL], LBFGS_HISTORY_PARAMS(VPL, G, S),
                                                        float (&dir_out)[VPL]) {
  constexpr int MMAX = LbfgsLimits<G, S>::MMAX;
  const int V = S::kStatic ? S::kV : a.v_dim, m = S::kStatic ? S::kM : a.m, B = a.batch;
  const size_t bv = (size_t)uniform_part<G>(b) * V;
  const size_t hist_stride = (size_t)B * V;
  OFF off[VPL];  // (lanes past V hold a clamped offset and store nothing)
#pragma unroll
  for (int e = 0; e < VPL; e++) off[e] = lane_offset<G, OFF>(b, lane, e, V, V);
  float (&ys)[MMAX][VPL] = h_ys;
  float (&ss)[MMAX][VPL] = h_ss;
  float rho_mine = h_rho;
  float gq[VPL], y[VPL], s[VPL];
  float part = 0.0f;
#pragma unroll
  for (int e = 0; e < VPL; e++) {
    const int v = lane + e * G;
    gq[e] = y[e] = s[e] = 0.0f;
    if (v < V) {
      const float g = g_in[e], x = x_in[e];
      y[e] = g - h_g0[e];
      s[e] = x - h_x0[e];
      const OFF o = block_offset(off[e]);
      row_at(a.grad_0 + bv, o) = g;
      row_at(a.x_0 + bv, o) = x;
      gq[e] = g;
      part = __builtin_fmaf(y[e], s[e], part);
    }
  }
  const float numerator = gsum<G>(part);
  if (lane == m - 1) {
    rho_mine = 1.0f / numerator;
    if (a.stable_mode && numerator <= 0.0f) rho_mine = 0.0f;
  }
  if (lane < m) a.rho_buffer[(size_t)lane * B + b] = rho_mine;
  float alpha_of[MMAX];  // alpha_i, the same value in every lane of the group (static indices: registers)
#pragma unroll
  for (int i = MMAX - 1; i >= 0; i--) {
    alpha_of[i] = 0.0f;
    if (i < m) {
      if (i == m - 1) {  // append the new pair at slot m-1 (kept inside this loop: as a loop of its own it
                         // becomes one dynamically indexed store and the history falls out of registers)
#pragma unroll
        for (int e = 0; e < VPL; e++) { ys[i][e] = y[e]; ss[i][e] = s[e]; }
      }
      float d = 0.0f;
#pragma unroll
      for (int e = 0; e < VPL; e++) d = __builtin_fmaf(gq[e], ss[i][e], d);
      d = gsum<G>(d);
      const float alpha = d * gbcast<G>(rho_mine, i);  // i is a constant after unrolling: v_readlane (G = 64)
      alpha_of[i] = alpha;
#pragma unroll
      for (int e = 0; e < VPL; e++) gq[e] = __builtin_fmaf(-alpha, ys[i][e], gq[e]);
    }
  }
  if (m > 0) {
    float d = 0.0f;
#pragma unroll
    for (int e = 0; e < VPL; e++) d = __builtin_fmaf(y[e], y[e], d);
    d = gsum<G>(d);
    float var1 = numerator / d;
    if (a.stable_mode && (isinf(var1) || isnan(var1))) var1 = a.epsilon;
    const float gamma = var1 < 0.0f ? 0.0f : var1;
#pragma unroll
    for (int e = 0; e < VPL; e++) gq[e] = gamma * gq[e];
  }
#pragma unroll
  for (int i = 0; i < MMAX; i++) {
    if (i < m) {
      float d = 0.0f;
#pragma unroll
      for (int e = 0; e < VPL; e++) d = __builtin_fmaf(gq[e], ys[i][e], d);
      d = gsum<G>(d);
      const float beta = __builtin_fmaf(-d, gbcast<G>(rho_mine, i), alpha_of[i]);
#pragma unroll
      for (int e = 0; e < VPL; e++) gq[e] = __builtin_fmaf(beta, ss[i][e], gq[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < VPL; e++) {
    const int v = lane + e * G;
    dir_out[e] = -gq[e];
    if (v < V) row_at(a.step_vec + bv, off[e]) = -gq[e];
  }
  // the shifted history goes back to memory last: 4 m stores per lane that nothing in this launch waits for
  // (!STORE_SHIFTED: only the appended pair, somebody else moves the rest)
  const size_t bv_late = sizeof(OFF) == 4 ? bv + fresh_zero() : bv;
  float *const y0 = a.y_buffer + bv_late, *const s0 = a.s_buffer + bv_late;
#pragma unroll
  for (int e = 0; e < VPL; e++) {
    if (lane + e * G < V) {
      const OFF o = block_offset(off[e]);
      if (!STORE_SHIFTED) {  // (the pair itself, not ys[m - 1]: a dynamic index would take the history out of registers)
        if (m > 0) {
          row_at(y0 + (size_t)(m - 1) * hist_stride, o) = y[e];
          row_at(s0 + (size_t)(m - 1) * hist_stride, o) = s[e];
        }
        continue;
      }
#pragma unroll
      for (int i = 0; i < MMAX; i++) {
        if (i < m) {
          row_at(y0 + (size_t)i * hist_stride, o) = ys[i][e];
          row_at(s0 + (size_t)i * hist_stride, o) = ss[i][e];
        }
      }
    }
  }
}

template <int VPL, int G = kWave>
__device__ __forceinline__ void lbfgs_step_reg_body(const LbfgsArgs &a, int b, int lane, const float (&g_in)[VPL],
                                                    const float (&x_in)[VPL], float (&dir_out)[VPL]) {
  LBFGS_HISTORY_DECL(VPL, G, TailShapeDyn);
  lbfgs_history_load<VPL, G, TailShapeDyn, size_t>(a, b, lane, LBFGS_HISTORY_ARGS);
  lbfgs_step_from_history<VPL, G, true, TailShapeDyn, size_t>(a, b, lane, g_in, x_in, LBFGS_HISTORY_ARGS, dir_out);
}

template <int VPL>
__global__ void __launch_bounds__(256) lbfgs_step_reg_kernel(const LbfgsArgs a) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int b = blockIdx.x * (blockDim.x / kWave) + wave;
  if (b >= a.batch) return;
  float g[VPL], x[VPL], dir[VPL];
#pragma unroll
  for (int e = 0; e < VPL; e++) {
    const int v = lane + e * kWave;
    g[e] = v < a.v_dim ? a.grad_q[(size_t)b * a.v_dim + v] : 0.0f;
    x[e] = v < a.v_dim ? a.q[(size_t)b * a.v_dim + v] : 0.0f;
  }
  lbfgs_step_reg_body<VPL>(a, b, lane, g, x, dir);
}

// ------------------------------------------------------------------------------------------
struct LineSearchArgs {
  float *best_cost, *best_action;
  int16_t *best_iteration, *current_iteration;
  uint8_t *converged;
  int convergence_iteration;
  float cost_delta_threshold, cost_relative_threshold;
  float *exploration_cost, *exploration_action, *exploration_gradient;
  int32_t *exploration_idx;
  float *selected_cost, *selected_action, *selected_gradient;
  int32_t *selected_idx;
  const float *search_cost, *search_action, *search_gradient, *step_direction, *search_magnitudes;
  float c_1, c_2;
  int strong_wolfe, approx_wolfe, n_linesearch, opt_dim, batch;
};

// body for one problem b on one wavefront; returns the exploration candidate index
template <int G = kWave>
__device__ __forceinline__ int line_search_body(const LineSearchArgs &a, int b, int lane) {
  const int V = a.opt_dim, NLS = a.n_linesearch;
  const float *dir = a.step_direction + (size_t)b * V;
  // g_k . d for every candidate; lane k keeps the k-th value (NLS <= 64)
  float gd_mine = 0.0f, gd0 = 0.0f;
  for (int k = 0; k < NLS; k++) {
    const float *g = a.search_gradient + ((size_t)b * NLS + k) * V;
    float d = 0.0f;
    for (int v = lane; v < V; v += G) d = __builtin_fmaf(g[v], dir[v], d);
    d = gsum<G>(d);
    if (k == 0) gd0 = d;
    if (lane == k) gd_mine = d;
  }
  // evaluate_wolfe_conditions (line_search_helpers.cuh:262-312), one candidate per lane
  bool w1 = false, wboth = false;
  const float c0 = a.search_cost[(size_t)b * NLS];
  if (lane < NLS) {
    const float alpha = a.search_magnitudes[lane];
    const float cv = a.search_cost[(size_t)b * NLS + lane];
    w1 = cv <= (c0 + a.c_1 * alpha * gd0);
    const bool w2 = a.strong_wolfe ? (fabsf(gd_mine) <= a.c_2 * fabsf(gd0)) : (gd_mine >= a.c_2 * gd0);
    wboth = w1 && w2;
  }
  // compute_wolfe_indices (:62-95): LARGEST candidate index that passes, 0 if none.
  // wave64 ballot + count-leading-zeros replaces the reference's 32-bit ballot/brev/ffs.
  const unsigned long long m1 = gballot<G>(w1), mb = gballot<G>(wboth);
  const int id1 = m1 ? 63 - __clzll((long long)m1) : 0;
  const int id = mb ? 63 - __clzll((long long)mb) : 0;
  const int sel = a.strong_wolfe ? id : (id == 0 ? id1 : id);  // get_linesearch_idx (:46-60)
  const int expl = (a.approx_wolfe && !a.strong_wolfe && sel == 0) ? 1 : sel;
  // update_costs_and_convergence (:97-150), computed redundantly by every lane (uniform)
  const float sc = a.search_cost[(size_t)b * NLS + sel];
  const float bc = a.best_cost[b];
  const int cur = (int)a.current_iteration[b] + 1;
  int bi = a.best_iteration[b];
  const float delta = bc - sc;
  const float rel = delta / (bc + 1e-6f);
  const bool update_best = delta > a.cost_delta_threshold && rel > a.cost_relative_threshold;
  if (update_best) bi = cur;
  __builtin_amdgcn_wave_barrier();  // all lanes have read the old state before lane 0 rewrites it
  if (lane == 0) {
    a.exploration_cost[b] = a.search_cost[(size_t)b * NLS + expl];
    a.selected_cost[b] = sc;
    a.converged[b] = (bi + a.convergence_iteration < cur) ? 1 : 0;
    a.best_iteration[b] = (int16_t)bi;
    a.current_iteration[b] = (int16_t)cur;
    if (update_best) a.best_cost[b] = sc;
  }
  // copy_action_gradient_results (:152-198)
  const size_t es = ((size_t)b * NLS + expl) * V, ss = ((size_t)b * NLS + sel) * V, o = (size_t)b * V;
  for (int v = lane; v < V; v += G) {
    a.exploration_action[o + v] = a.search_action[es + v];
    a.exploration_gradient[o + v] = a.search_gradient[es + v];
    const float av = a.search_action[ss + v];
    a.selected_action[o + v] = av;
    a.selected_gradient[o + v] = a.search_gradient[ss + v];
    if (update_best) a.best_action[o + v] = av;
  }
  if (lane < NLS) {
    a.exploration_idx[(size_t)b * NLS + lane] = expl;
    a.selected_idx[(size_t)b * NLS + lane] = sel;
  }
  return expl;
}

__global__ void __launch_bounds__(256) line_search_kernel(const LineSearchArgs a) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int b = blockIdx.x * (blockDim.x / kWave) + wave;
  if (b >= a.batch) return;
  line_search_body(a, b, lane);
}

// ------------------------------------------------------------------------------------------
// per-trajectory cost sum: one 256-lane workgroup per trajectory; every lane owns a strided
// slice (independent loads, all in flight at once), then wave64 DPP reduction and a fixed-order
// 4-entry LDS combine (deterministic).
__global__ void __launch_bounds__(256) trajectory_cost_sum_kernel(float *out, const float *self_cost,
                                                                  const float *scene_cost, int batch,
                                                                  int horizon, int nspheres) {
  __shared__ float s_part[4];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, wave = tid / kWave;
  float acc0 = 0.0f, acc1 = 0.0f;
  if (scene_cost) {
    const int n = horizon * nspheres;
    const float *src = scene_cost + (size_t)b * n;
    int i = tid;
    for (; i + 256 < n; i += 512) { acc0 += src[i]; acc1 += src[i + 256]; }
    if (i < n) acc0 += src[i];
  }
  if (self_cost)
    for (int h = tid; h < horizon; h += 256) acc1 += self_cost[(size_t)b * horizon + h];
  const float w = wave_sum(acc0 + acc1);
  if ((tid & (kWave - 1)) == 0) s_part[wave] = w;
  __syncthreads();
  if (tid == 0) out[b] = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}

// a / b as the library's fp32 division is built (-fno-hip-fp32-correctly-rounded-divide-sqrt: frexp both operands, v_rcp_f32
// of the divisor's mantissa, one multiply, ldexp), spelled out.  The `/` operator gets that sequence only while the
// optimiser carries its 2.5 ulp marking along: in the one-element instantiations of the one-launch tail the quotient
// |d_v| / step_max lost it and ran the IEEE sequence (v_div_scale / v_div_fmas / v_div_fixup), so their step scale differed
// in the last bit from the two-element instantiations and from prepare_search_points_kernel (and d / scale likewise in the
// one-element plain kernel).  Same bits as `/` wherever the marking survives.  Used for the step scale in all three places.
__device__ __forceinline__ float div_frexp_rcp(float a, float b) {
  const float q = __builtin_amdgcn_frexp_mantf(a) * __builtin_amdgcn_rcpf(__builtin_amdgcn_frexp_mantf(b));
  return __builtin_amdgcn_ldexpf(q, __builtin_amdgcn_frexp_expf(a) - __builtin_amdgcn_frexp_expf(b));
}

// ------------------------------------------------------------------------------------------
// Line-search candidate generation, fused (reference optim/gradient/line_search_strategy.py:
// 134-204 `_prepare_search_points` = scale_action (:301-325) + jit_get_x_set (:281-299), three to
// four torch elementwise/reduction kernels).  One wavefront per problem:
//   scale = max(1, max_v |d_v| / step_max[v % action_dim])   (only if step_scale not in {0,1})
//   d_out = d / scale ;  x_set[b,k,:] = x[b,:] + alpha_k * d_out
__global__ void __launch_bounds__(256) prepare_search_points_kernel(
    float *x_set, float *d_out, const float *x, const float *d, const float *step_max,
    const float *alphas, int batch, int nls, int opt_dim, int action_dim, int apply_scale) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int b = blockIdx.x * (blockDim.x / kWave) + wave;
  if (b >= batch) return;
  const size_t o = (size_t)b * opt_dim;
  float scale = 1.0f;
  if (apply_scale) {
    float mx = 0.0f;
    for (int v = lane; v < opt_dim; v += kWave) mx = fmaxf(mx, div_frexp_rcp(fabsf(d[o + v]), step_max[v % action_dim]));
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, kWave));
    scale = fmaxf(mx, 1.0f);
  }
  for (int v = lane; v < opt_dim; v += kWave) {
    const float dv = div_frexp_rcp(d[o + v], scale);
    const float xv = x[o + v];
    d_out[o + v] = dv;
    for (int k = 0; k < nls; k++) x_set[((size_t)b * nls + k) * opt_dim + v] = __builtin_fmaf(alphas[k], dv, xv);
  }
}

// ------------------------------------------------------------------------------------------
// The optimiser side of one L-BFGS iteration in ONE launch: line search over the evaluated
// candidates -> L-BFGS two-loop from the chosen exploration point -> the next iteration's
// candidates.  Same arithmetic as line_search_kernel + lbfgs_step_reg_kernel +
// prepare_search_points_kernel run back to back (those are the device functions above); the
// exploration point and the new direction are handed over in registers, so the three dependent
// launches (each a chain of global round trips on one wavefront per problem) become one.
struct PrepareArgs {
  float *x_set, *d_out;
  const float *step_max, *alphas;
  int action_dim, apply_scale;
};

template <int VPL, int G = kWave>
__global__ void __launch_bounds__(256) lbfgs_iteration_tail_kernel(const LineSearchArgs ls, const LbfgsArgs lb,
                                                                   const PrepareArgs pr) {
  const int grp = threadIdx.x / G, lane = threadIdx.x % G;
  const int b = blockIdx.x * (blockDim.x / G) + grp;
  if (b >= ls.batch) return;  // (groups of a wavefront exit together or run the same control flow)
  const int V = ls.opt_dim, NLS = ls.n_linesearch;
  const int expl = line_search_body<G>(ls, b, lane);
  float g[VPL], x[VPL], dir[VPL];
#pragma unroll
  for (int e = 0; e < VPL; e++) {  // the values line_search_body just copied to the exploration buffers
    const int v = lane + e * G;
    const size_t src = ((size_t)b * NLS + expl) * V + v;
    g[e] = v < V ? ls.search_gradient[src] : 0.0f;
    x[e] = v < V ? ls.search_action[src] : 0.0f;
  }
  lbfgs_step_reg_body<VPL, G>(lb, b, lane, g, x, dir);
  float scale = 1.0f;
  if (pr.apply_scale) {
    float mx = 0.0f;
#pragma unroll
    for (int e = 0; e < VPL; e++) {
      const int v = lane + e * G;
      if (v < V) mx = fmaxf(mx, div_frexp_rcp(fabsf(dir[e]), pr.step_max[v % pr.action_dim]));
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, G));
    scale = fmaxf(mx, 1.0f);
  }
#pragma unroll
  for (int e = 0; e < VPL; e++) {
    const int v = lane + e * G;
    if (v < V) {
      const float dv = div_frexp_rcp(dir[e], scale);
      pr.d_out[(size_t)b * V + v] = dv;
      for (int k = 0; k < NLS; k++) pr.x_set[((size_t)b * NLS + k) * V + v] = __builtin_fmaf(pr.alphas[k], dv, x[e]);
    }
  }
}

// ---- the same launch, restructured around memory latency -------------------------------------------------
// The kernel above is a string of ~a dozen DEPENDENT global round trips on one wavefront per problem (dot
// products candidate by candidate, then the chosen costs, then the chosen rows, then the history ...).  The two
// kernels below issue every load that does not depend on the line-search decision up front (all candidates'
// actions and gradients, the step direction, the previous iterate, the whole history, the scalars), take the
// decision in registers and pick the chosen rows with selects.  Same arithmetic in the same order => same bits.
// NLS <= NLSMAX (the reference uses 4 candidates).

// The ~350 B of arguments span six 64 B lines of the kernarg segment and the compiler fetches a field where it is
// first needed: up to six dependent scalar-cache misses strung along the kernel.  One dword of every line is
// requested here, back to back, so that all later s_loads hit the scalar cache.
__device__ __forceinline__ void touch_kernarg_lines() {
  const uint32_t *ka = (const uint32_t *)__builtin_amdgcn_kernarg_segment_ptr();
  // (+ 1: the line the hidden launch-size arguments begin in)
  constexpr int kLines = (int)((sizeof(LineSearchArgs) + sizeof(LbfgsArgs) + sizeof(PrepareArgs)) / 64) + 1;
  uint32_t touch = 0;
#pragma unroll
  for (int i = 0; i < kLines; i++) touch |= ka[i * 16];
  asm volatile("" ::"s"(touch));
}

// the inputs of the line search of problem b as one lane group holds them
#define TAIL_INPUTS_DECL(VPL, NLSMAX) \
  float t_sg[NLSMAX][VPL], t_sa[NLSMAX][VPL], t_dir[VPL], t_smax[VPL], t_cost, t_mag, t_bc; \
  int t_cur, t_bi
#define TAIL_INPUTS_PARAMS(VPL, NLSMAX)                                                                         \
  float (&t_sg)[NLSMAX][VPL], float (&t_sa)[NLSMAX][VPL], float (&t_dir)[VPL], float (&t_smax)[VPL], float &t_cost, \
      float &t_mag, float &t_bc, int &t_cur, int &t_bi
#define TAIL_INPUTS_ARGS t_sg, t_sa, t_dir, t_smax, t_cost, t_mag, t_bc, t_cur, t_bi

template <int VPL, int G, int NLSMAX, class S, typename OFF>
__device__ __forceinline__ void tail_inputs_load(const LineSearchArgs &ls, const PrepareArgs &pr, int b, int lane,
                                                 TAIL_INPUTS_PARAMS(VPL, NLSMAX)) {
  const int V = S::kStatic ? S::kV : ls.opt_dim, NLS = S::kStatic ? S::kNLS : ls.n_linesearch;
  const int action_dim = S::kStatic ? S::kAD : pr.action_dim;
  const size_t o = (size_t)uniform_part<G>(b) * V, oc = (size_t)uniform_part<G>(b) * NLS;
  const int ln = lane < NLS ? lane : NLS - 1;
  const int lane_is_cand = opaque_lane_mask(lane < NLS);
  t_cost = and_mask(row_at(ls.search_cost + oc, (lane_part<G, OFF>(b) * (OFF)NLS + (OFF)ln) * (OFF)sizeof(float)), lane_is_cand);
  t_mag = and_mask(ls.search_magnitudes[ln], lane_is_cand);
  t_bc = ls.best_cost[b];
  t_cur = (int)ls.current_iteration[b] + 1;
  t_bi = ls.best_iteration[b];
  // clamped unconditional loads (see lbfgs_history_load); candidates k >= NLS are copies of candidate NLS-1,
  // which go through the arithmetic but can never be chosen
#pragma unroll
  for (int e = 0; e < VPL; e++) {
    const int v = lane + e * G, vc = v < V ? v : V - 1;
    const int mk = opaque_lane_mask(v < V);
    t_dir[e] = and_mask(row_at(ls.step_direction + o, lane_offset<G, OFF>(b, lane, e, V, V)), mk);
    const OFF off = lane_offset<G, OFF>(b, lane, e, V, NLS * V);  // candidate rows: [B][NLS][V]
#pragma unroll
    for (int k = 0; k < NLSMAX; k++) {
      const int kc = k < NLS ? k : NLS - 1;
      t_sg[k][e] = and_mask(row_at(ls.search_gradient + (oc + kc) * V, off), mk);
      t_sa[k][e] = and_mask(row_at(ls.search_action + (oc + kc) * V, off), mk);
    }
    t_smax[e] = pr.step_max[vc % action_dim];
  }
}

// line_search_body from registers; g / x = gradient / iterate of the exploration candidate
template <int VPL, int G, int NLSMAX, class S, typename OFF>
__device__ __forceinline__ void tail_line_search(const LineSearchArgs &ls, int b, int lane, TAIL_INPUTS_PARAMS(VPL, NLSMAX),
                                                 float (&g)[VPL], float (&x)[VPL]) {
  const int V = S::kStatic ? S::kV : ls.opt_dim, NLS = S::kStatic ? S::kNLS : ls.n_linesearch;
  const size_t o = (size_t)uniform_part<G>(b) * V;
  float gd_mine = 0.0f, gd0 = 0.0f;
#pragma unroll
  for (int k = 0; k < NLSMAX; k++) {
    float d = 0.0f;
#pragma unroll
    for (int e = 0; e < VPL; e++) d = __builtin_fmaf(t_sg[k][e], t_dir[e], d);
    d = gsum<G>(d);
    if (k == 0) gd0 = d;
    if (lane == k) gd_mine = d;
  }
  bool w1 = false, wboth = false;
  const float c0 = gbcast<G>(t_cost, 0);
  if (lane < NLS) {
    w1 = t_cost <= (c0 + ls.c_1 * t_mag * gd0);
    const bool w2 = ls.strong_wolfe ? (fabsf(gd_mine) <= ls.c_2 * fabsf(gd0)) : (gd_mine >= ls.c_2 * gd0);
    wboth = w1 && w2;
  }
  const unsigned long long m1 = gballot<G>(w1), mb = gballot<G>(wboth);
  const int id1 = m1 ? 63 - __clzll((long long)m1) : 0;
  const int id = mb ? 63 - __clzll((long long)mb) : 0;
  const int sel = ls.strong_wolfe ? id : (id == 0 ? id1 : id);
  const int expl = (ls.approx_wolfe && !ls.strong_wolfe && sel == 0) ? 1 : sel;
  float sc = 0.0f, ec = 0.0f;
#pragma unroll
  for (int k = 0; k < NLSMAX; k++) {
    const float ck = gbcast<G>(t_cost, k);
    if (k == sel) sc = ck;
    if (k == expl) ec = ck;
  }
  const float delta = t_bc - sc;
  const float rel = delta / (t_bc + 1e-6f);
  const bool update_best = delta > ls.cost_delta_threshold && rel > ls.cost_relative_threshold;
  const int bi = update_best ? t_cur : t_bi;
  if (lane == 0) {
    ls.exploration_cost[b] = ec;
    ls.selected_cost[b] = sc;
    ls.converged[b] = (bi + ls.convergence_iteration < t_cur) ? 1 : 0;
    ls.best_iteration[b] = (int16_t)bi;
    ls.current_iteration[b] = (int16_t)t_cur;
    if (update_best) ls.best_cost[b] = sc;
  }
#pragma unroll
  for (int e = 0; e < VPL; e++) {
    const int v = lane + e * G;
    float gs = 0.0f, xs = 0.0f;
    g[e] = x[e] = 0.0f;
#pragma unroll
    for (int k = 0; k < NLSMAX; k++) {
      if (k == expl) { g[e] = t_sg[k][e]; x[e] = t_sa[k][e]; }
      if (k == sel) { gs = t_sg[k][e]; xs = t_sa[k][e]; }
    }
    if (v < V) {
      const OFF off = block_offset(lane_offset<G, OFF>(b, lane, e, V, V));
      row_at(ls.exploration_action + o, off) = x[e];
      row_at(ls.exploration_gradient + o, off) = g[e];
      row_at(ls.selected_action + o, off) = xs;
      row_at(ls.selected_gradient + o, off) = gs;
      if (update_best) row_at(ls.best_action + o, off) = xs;
    }
  }
  if (lane < NLS) {
    const size_t oc = (size_t)uniform_part<G>(b) * NLS;
    const OFF off = (lane_part<G, OFF>(b) * (OFF)NLS + (OFF)lane) * (OFF)sizeof(int32_t);
    row_at(ls.exploration_idx + oc, off) = expl;
    row_at(ls.selected_idx + oc, off) = sel;
  }
}

// prepare_search_points_kernel from registers
template <int VPL, int G, int NLSMAX, typename OFF>
__device__ __forceinline__ void tail_next_candidates(const PrepareArgs &pr, int b, int lane, int V, int NLS,
                                                     const float (&x)[VPL], const float (&dir)[VPL],
                                                     const float (&smax)[VPL], float mag_mine) {
  const size_t o = (size_t)uniform_part<G>(b) * V, oc = (size_t)uniform_part<G>(b) * NLS;
  float scale = 1.0f;
  if (pr.apply_scale) {
    float mx = 0.0f;
#pragma unroll
    for (int e = 0; e < VPL; e++) {
      const int v = lane + e * G;
      if (v < V) mx = fmaxf(mx, div_frexp_rcp(fabsf(dir[e]), smax[e]));
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, G));
    scale = fmaxf(mx, 1.0f);
  }
#pragma unroll
  for (int e = 0; e < VPL; e++) {
    const int v = lane + e * G;
    const float dv = div_frexp_rcp(dir[e], scale);
    float xk[NLSMAX];
#pragma unroll
    for (int k = 0; k < NLSMAX; k++) xk[k] = __builtin_fmaf(gbcast<G>(mag_mine, k), dv, x[e]);
    if (v < V) {
      row_at(pr.d_out + o, lane_offset<G, OFF>(b, lane, e, V, V)) = dv;
      const OFF off = block_offset(lane_offset<G, OFF>(b, lane, e, V, NLS * V));
#pragma unroll
      for (int k = 0; k < NLSMAX; k++)
        if (k < NLS) row_at(pr.x_set + (oc + k) * V, off) = xk[k];
    }
  }
}

// The tail is one dependent chain per problem (54 reductions) that shares its SIMD with the rollout wavefronts of the
// other seed shards (optim/pipelined.py): at equal priority it gets one issue slot in five.  Highest wave priority for
// the whole kernel; it issues an instruction every ~8 cycles, so the rollouts hardly notice.
__device__ __forceinline__ void tail_raise_priority() {
  __builtin_amdgcn_s_setprio(3);
}

// (a) one lane group per problem: everything in one burst of loads.  Used for the 16-lane-row problems (IK) and, one
// wavefront per problem, between the rollouts of other seed shards.  S: a compile-time shape (tail_shapes.hpp) or the
// run-time dimensions of the arguments; row offsets are 32-bit (the host checks tail_offsets_fit for the row form).
template <int VPL, int G, int NLSMAX, class S = TailShapeDyn>
__global__ void __launch_bounds__(256) lbfgs_iteration_tail_prefetch_kernel(const LineSearchArgs ls, const LbfgsArgs lb,
                                                                            const PrepareArgs pr) {
  typedef uint32_t OFF;
  tail_raise_priority();
  touch_kernarg_lines();
  const int grp = threadIdx.x / G, lane = threadIdx.x % G;
  int b = blockIdx.x * (blockDim.x / G) + grp;
  if (G == kWave) b = __builtin_amdgcn_readfirstlane(b);  // one problem per wavefront: its row bases live in SGPRs
  if (b >= ls.batch) return;
  const int V = S::kStatic ? S::kV : ls.opt_dim, NLS = S::kStatic ? S::kNLS : ls.n_linesearch;
  TAIL_INPUTS_DECL(VPL, NLSMAX);
  tail_inputs_load<VPL, G, NLSMAX, S, OFF>(ls, pr, b, lane, TAIL_INPUTS_ARGS);
  LBFGS_HISTORY_DECL(VPL, G, S);
  lbfgs_history_load<VPL, G, S, OFF>(lb, b, lane, LBFGS_HISTORY_ARGS);
  float g[VPL], x[VPL], dir[VPL];
  tail_line_search<VPL, G, NLSMAX, S, OFF>(ls, b, lane, TAIL_INPUTS_ARGS, g, x);
  lbfgs_step_from_history<VPL, G, true, S, OFF>(lb, b, lane, g, x, LBFGS_HISTORY_ARGS, dir);
  tail_next_candidates<VPL, G, NLSMAX, OFF>(pr, b, lane, V, NLS, x, dir, t_smax, t_mag);
}

// (b) one 256-lane workgroup per problem, for wavefront-sized problems (trajectory optimisation: V = 84, m = 27).
// A lone wavefront needs ~4 m + 25 loads per lane for such a problem: the address arithmetic alone is ~3 us of
// issue time on a wavefront that has its SIMD to itself, and the 64-entry vmcnt queue turns the burst into three
// round trips.  Here wavefronts 1..3 move the history: 192 lanes stage old slots 1..m-1 into LDS (coalesced, ~2 m V /
// 192 loads per lane, one round trip) while wavefront 0 loads the line-search inputs and decides; after ONE
// barrier wavefront 0 pulls the history from LDS into registers (transposed there: 8 float4 reads per array and
// element instead of 4 m dword loads) and runs the two-loop recursion, and wavefronts
// 1..3 write the shifted history back from the registers they staged it through -- off the critical path.
constexpr int kStageLanes = 192;
constexpr int kHistRow = 36;
template <int VPL, int NLSMAX, int RMAX, class S = TailShapeDyn>
__global__ void __launch_bounds__(256) lbfgs_iteration_tail_wg_kernel(const LineSearchArgs ls, const LbfgsArgs lb,
                                                                      const PrepareArgs pr) {
  // y then s, each [V + 1][kHistRow]: row v = the slots 0..m-2 (new numbering) of element v, so that the lane that
  // owns v fetches them with float4 reads; row V is zero (lanes past V).  36 floats per row: 16 B aligned and the
  // float4 reads of 16 consecutive lanes fall into distinct banks.
  extern __shared__ float s_hist[];
  constexpr int G = kWave;
  constexpr int MMAX = LbfgsLimits<G, S>::MMAX;
  typedef uint32_t OFF;  // (the host checks tail_offsets_fit: a staging lane's offset spans the slots it moves)
  tail_raise_priority();
  touch_kernarg_lines();
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid % kWave;
  const int V = S::kStatic ? S::kV : lb.v_dim, m = S::kStatic ? S::kM : lb.m;
  const int s_off = (V + 1) * kHistRow;
  const int n = m > 0 ? (m - 1) * V : 0;  // floats per array that move
  const size_t hist_stride = (size_t)lb.batch * V;
  const OFF hist_stride32 = (OFF)lb.batch * (OFF)V;
  float g[VPL], x[VPL];
  TAIL_INPUTS_DECL(VPL, NLSMAX);
  LBFGS_HISTORY_DECL(VPL, G, S);
  float stage_y[RMAX], stage_s[RMAX];
  if (tid < kWave) {
    tail_inputs_load<VPL, G, NLSMAX, S, OFF>(ls, pr, b, lane, TAIL_INPUTS_ARGS);
    int mk[VPL];
#pragma unroll
    for (int e = 0; e < VPL; e++) {
      const OFF off = lane_offset<G, OFF>(b, lane, e, V, V);
      mk[e] = opaque_lane_mask(lane + e * G < V);
      h_g0[e] = and_mask(row_at(lb.grad_0 + (size_t)b * V, off), mk[e]);
      h_x0[e] = and_mask(row_at(lb.x_0 + (size_t)b * V, off), mk[e]);
    }
    const int rl = lane + 1 < m ? lane + 1 : (m > 0 ? m - 1 : 0);
    h_rho = m > 0 ? and_mask(lb.rho_buffer[(size_t)rl * lb.batch + b], opaque_lane_mask(lane < m - 1)) : 0.0f;
    tail_line_search<VPL, G, NLSMAX, S, OFF>(ls, b, lane, TAIL_INPUTS_ARGS, g, x);
  } else if (n > 0) {
    // element idx = i * V + v of the new numbering comes from old slot i + 1; idx advances by 192 per round:
    // (i, v) are stepped, not divided
    const int t = tid - kWave;
    const int step_i = kStageLanes / V, step_v = kStageLanes % V;
    int i = t / V, v = t % V;
    const float *ysrc = lb.y_buffer + (size_t)b * V + hist_stride;  // old slot 1
    const float *ssrc = lb.s_buffer + (size_t)b * V + hist_stride;
#pragma unroll
    for (int r = 0; r < RMAX; r++) {
      const int idx = t + r * kStageLanes;
      // past the end: re-read the last element (and re-write it below), no predication
      const int ic = idx < n ? i : m - 2, vc = idx < n ? v : V - 1;
      const OFF off = ((OFF)ic * hist_stride32 + (OFF)vc) * (OFF)sizeof(float);
      stage_y[r] = row_at(ysrc, off);
      stage_s[r] = row_at(ssrc, off);
      v += step_v; i += step_i;
      if (v >= V) { v -= V; i++; }
    }
    {
      int i2 = t / V, v2 = t % V;
#pragma unroll
      for (int r = 0; r < RMAX; r++) {
        const int idx = t + r * kStageLanes;
        const int at = idx < n ? v2 * kHistRow + i2 : (V - 1) * kHistRow + m - 2;
        s_hist[at] = stage_y[r];
        s_hist[s_off + at] = stage_s[r];
        v2 += step_v; i2 += step_i;
        if (v2 >= V) { v2 -= V; i2++; }
      }
    }
    if (t < 32) s_hist[V * kHistRow + t] = s_hist[s_off + V * kHistRow + t] = 0.0f;  // the row lanes past V read
  }
  __syncthreads();  // every old slot has been read: the shifted write-back cannot overtake a read
  if (tid < kWave) {
    if (n > 0) {
#pragma unroll
      for (int e = 0; e < VPL; e++) {
        const int v = lane + e * G;
        const float4 *ry = reinterpret_cast<const float4 *>(s_hist + (v < V ? v : V) * kHistRow);
        const float4 *rs = reinterpret_cast<const float4 *>(s_hist + s_off + (v < V ? v : V) * kHistRow);
#pragma unroll
        for (int j = 0; j < (MMAX + 3) / 4; j++) {  // (slots >= m-1 of a row: never written, never used)
          const float4 qy = ry[j], qs = rs[j];
          const float cy[4] = {qy.x, qy.y, qy.z, qy.w}, cs[4] = {qs.x, qs.y, qs.z, qs.w};
#pragma unroll
          for (int c = 0; c < 4; c++)
            if (4 * j + c < MMAX) { h_ys[4 * j + c][e] = cy[c]; h_ss[4 * j + c][e] = cs[c]; }
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < MMAX; i++) {
#pragma unroll
        for (int e = 0; e < VPL; e++) h_ys[i][e] = h_ss[i][e] = 0.0f;
      }
    }
    float dir[VPL];
    lbfgs_step_from_history<VPL, G, false, S, OFF>(lb, b, lane, g, x, LBFGS_HISTORY_ARGS, dir);
    tail_next_candidates<VPL, G, NLSMAX, OFF>(pr, b, lane, V, S::kStatic ? S::kNLS : ls.n_linesearch, x, dir, t_smax, t_mag);
  } else if (n > 0) {
    const int t = tid - kWave;
    const int step_i = kStageLanes / V, step_v = kStageLanes % V;
    int i = t / V, v = t % V;
    float *ydst = lb.y_buffer + (size_t)b * V;  // new slot 0
    float *sdst = lb.s_buffer + (size_t)b * V;
#pragma unroll
    for (int r = 0; r < RMAX; r++) {
      const int idx = t + r * kStageLanes;
      if (idx < n) {
        const OFF off = ((OFF)i * hist_stride32 + (OFF)v) * (OFF)sizeof(float);
        row_at(ydst, off) = stage_y[r];
        row_at(sdst, off) = stage_s[r];
      }
      v += step_v; i += step_i;
      if (v >= V) { v -= V; i++; }
    }
  }
}

}  // namespace curobo_hip

using namespace curobo_hip;

CUROBO_EXPORT int curobo_hip_launch_lbfgs_step(
    float *step_vec, float *rho_buffer, float *y_buffer, float *s_buffer, const float *q,
    const float *grad_q, float *x_0, float *grad_0, float epsilon, int batch_size, int history_m,
    int v_dim, int stable_mode, int use_shared_buffers, curobo_hip_stream_t stream) {
  (void)use_shared_buffers;
  const char *what = "launch_lbfgs_step";
  // reference cuda_core_backend/optimization.py:185-188 and optim/gradient/lbfgs.py:177
  CUROBO_REQUIRE(history_m <= 31, "%s: History_m greater than 31 is not supported", what);
  CUROBO_REQUIRE(history_m >= 0, "%s: History_m less than 0 is not supported", what);
  CUROBO_REQUIRE(v_dim >= 1 && v_dim <= kWave * kMaxVPL, "%s: v_dim=%d out of range [1,%d]", what, v_dim, kWave * kMaxVPL);
  if (batch_size == 0) return CUROBO_HIP_OK;
  LbfgsArgs a{step_vec, rho_buffer, y_buffer, s_buffer, q, grad_q, x_0, grad_0,
              epsilon, batch_size, history_m, v_dim, stable_mode};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)ceil_div(batch_size, 4)), block(256);
  const int vpl = ceil_div(v_dim, kWave);
  if (vpl <= 1) hipLaunchKernelGGL((lbfgs_step_reg_kernel<1>), grid, block, 0, st, a);
  else if (vpl <= 2) hipLaunchKernelGGL((lbfgs_step_reg_kernel<2>), grid, block, 0, st, a);
  else if (vpl <= 4) hipLaunchKernelGGL((lbfgs_step_kernel<4>), grid, block, 0, st, a);
  else if (vpl <= 8) hipLaunchKernelGGL((lbfgs_step_kernel<8>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((lbfgs_step_kernel<16>), grid, block, 0, st, a);
  return check_launch(what, st);
}

CUROBO_EXPORT int curobo_hip_launch_line_search(
    float *best_cost, float *best_action, int16_t *best_iteration, int16_t *current_iteration,
    uint8_t *converged_global, int convergence_iteration, float cost_delta_threshold,
    float cost_relative_threshold, float *exploration_cost, float *exploration_action,
    float *exploration_gradient, int32_t *exploration_idx, float *selected_cost,
    float *selected_action, float *selected_gradient, int32_t *selected_idx,
    const float *search_cost, const float *search_action, const float *search_gradient,
    const float *step_direction, const float *search_magnitudes, float armijo_threshold_c_1,
    float curvature_threshold_c_2, int strong_wolfe, int approx_wolfe, int n_linesearch,
    int opt_dim, int batchsize, curobo_hip_stream_t stream) {
  const char *what = "launch_line_search";
  CUROBO_REQUIRE(n_linesearch >= 1 && n_linesearch <= kWave, "%s: n_linesearch=%d out of range [1,64]", what, n_linesearch);
  CUROBO_REQUIRE(opt_dim >= 1, "%s: opt_dim must be >= 1", what);
  if (batchsize == 0) return CUROBO_HIP_OK;
  LineSearchArgs a{best_cost, best_action, best_iteration, current_iteration, converged_global,
                   convergence_iteration, cost_delta_threshold, cost_relative_threshold,
                   exploration_cost, exploration_action, exploration_gradient, exploration_idx,
                   selected_cost, selected_action, selected_gradient, selected_idx,
                   search_cost, search_action, search_gradient, step_direction, search_magnitudes,
                   armijo_threshold_c_1, curvature_threshold_c_2, strong_wolfe, approx_wolfe,
                   n_linesearch, opt_dim, batchsize};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(line_search_kernel, dim3((unsigned)ceil_div(batchsize, 4)), dim3(256), 0, st, a);
  return check_launch(what, st);
}

CUROBO_EXPORT int curobo_hip_trajectory_cost_sum(float *out_cost, const float *self_cost,
                                                 const float *scene_cost, int batch_size, int horizon,
                                                 int num_spheres, curobo_hip_stream_t stream) {
  const char *what = "trajectory_cost_sum";
  CUROBO_REQUIRE(horizon >= 1 && num_spheres >= 0, "%s: bad horizon/num_spheres", what);
  if (batch_size == 0) return CUROBO_HIP_OK;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(trajectory_cost_sum_kernel, dim3((unsigned)batch_size), dim3(256), 0, st,
                     out_cost, self_cost, scene_cost, batch_size, horizon, num_spheres);
  return check_launch(what, st);
}

CUROBO_EXPORT int curobo_hip_prepare_search_points(float *x_set, float *step_direction_out, const float *x,
                                                   const float *step_direction, const float *action_step_max,
                                                   const float *search_magnitudes, int batchsize,
                                                   int n_linesearch, int opt_dim, int action_dim,
                                                   int apply_step_scale, curobo_hip_stream_t stream) {
  const char *what = "prepare_search_points";
  CUROBO_REQUIRE(n_linesearch >= 1 && opt_dim >= 1 && action_dim >= 1, "%s: bad dimensions", what);
  CUROBO_REQUIRE(opt_dim % action_dim == 0, "%s: opt_dim must be a multiple of action_dim", what);
  if (batchsize == 0) return CUROBO_HIP_OK;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(prepare_search_points_kernel, dim3((unsigned)ceil_div(batchsize, 4)), dim3(256), 0, st,
                     x_set, step_direction_out, x, step_direction, action_step_max, search_magnitudes,
                     batchsize, n_linesearch, opt_dim, action_dim, apply_step_scale);
  return check_launch(what, st);
}

// ---- which kernel a one-launch tail runs: decided in ONE place, for the launch and for the host-side queries --------
static bool g_tail_shapes_enabled = true;

template <class S>
static bool tail_shape_matches(int opt_dim, int history_m, int n_linesearch, int action_dim) {
  return opt_dim == S::kV && history_m == S::kM && n_linesearch == S::kNLS && action_dim == S::kAD;
}
static int tail_shape_of(int opt_dim, int history_m, int n_linesearch, int action_dim) {
  if (tail_shape_matches<CUROBO_TAIL_SHAPE_1>(opt_dim, history_m, n_linesearch, action_dim)) return 1;
  if (tail_shape_matches<CUROBO_TAIL_SHAPE_2>(opt_dim, history_m, n_linesearch, action_dim)) return 2;
  return 0;
}
// 32-bit lane offsets (row_at with OFF = uint32_t): the largest byte offset a lane forms must stay below 2^31.
//   row form: the problem index is part of the offset, the largest row is a candidate row: batch * n_linesearch * opt_dim
//   workgroup form: a staging lane's offset spans the history slots it moves: history_m * batch * opt_dim
// Both imply batch * opt_dim * 4 < 2^31.  The 64-lane wavefront form keeps the problem in the scalar base: always fits.
static bool tail_offsets_fit(long long rows, int batchsize, int opt_dim) {
  return rows * (long long)batchsize * opt_dim * 4 < (1ll << 31);
}
enum TailForm { kTailPlain = 0, kTailRow = 1, kTailWave = 2, kTailWorkgroup = 3 };
struct TailChoice { int form, shape; };
static TailChoice tail_choose(int opt_dim, int history_m, int n_linesearch, int action_dim, int batchsize, int overlapped) {
  static const bool no_row16 = getenv("CUROBO_HIP_NO_ROW16") != nullptr;
  static const bool no_prefetch = getenv("CUROBO_HIP_TAIL_NO_PREFETCH") != nullptr;
  static const bool no_wg_env = getenv("CUROBO_HIP_TAIL_NO_WG") != nullptr;
  static const bool wg_env = getenv("CUROBO_HIP_TAIL_WG") != nullptr;  // (tuning knobs: force either form)
  static const bool no_shapes_env = getenv("CUROBO_HIP_TAIL_NO_SHAPES") != nullptr;
  const bool row16 = !no_row16 && opt_dim <= 16 && history_m <= 16 && n_linesearch <= 16;
  TailChoice c{kTailPlain, 0};
  if (n_linesearch <= 4 && !no_prefetch) {
    // a workgroup per problem pays while the problems do not fill the chip (64 / 256: 9.0 / 10.1 us against 12.3 /
    // 12.9 us for a wavefront per problem); at 1024 problems the extra wavefronts cost more than they hide (19 vs 15).
    // Between the rollout workgroups of other seed shards (`overlapped`) it is the other way round: the workgroup form
    // needs 24 KB of LDS and four 179-VGPR wavefronts per problem on CUs that the rollouts fill to 151 of 160 KB and
    // 384 of 512 VGPRs per SIMD (C2, 100-iteration blocks: 65.1 us per iteration with it, 60.4 us without)
    const bool no_wg = !wg_env && (no_wg_env || overlapped != 0 || batchsize > 512);
    if (row16) c.form = tail_offsets_fit(n_linesearch, batchsize, opt_dim) ? kTailRow : kTailPlain;
    else if (no_wg || !tail_offsets_fit(history_m, batchsize, opt_dim)) c.form = kTailWave;
    else c.form = kTailWorkgroup;
  }
  if (c.form != kTailPlain && g_tail_shapes_enabled && !no_shapes_env) {
    const int id = tail_shape_of(opt_dim, history_m, n_linesearch, action_dim);
    // (a shape is held by the forms its problems run in: 1 = wavefront and workgroup, 2 = row)
    if ((id == 1 && (c.form == kTailWave || c.form == kTailWorkgroup)) || (id == 2 && c.form == kTailRow)) c.shape = id;
  }
  return c;
}

CUROBO_EXPORT int curobo_hip_lbfgs_tail_shape_id(int opt_dim, int history, int n_linesearch, int action_dim) {
  return tail_shape_of(opt_dim, history, n_linesearch, action_dim);
}
CUROBO_EXPORT int curobo_hip_lbfgs_set_tail_shapes_enabled(int enabled) {
  g_tail_shapes_enabled = enabled != 0;
  return CUROBO_HIP_OK;
}
CUROBO_EXPORT int curobo_hip_lbfgs_tail_form(int opt_dim, int history, int n_linesearch, int action_dim, int batchsize,
                                             int overlapped) {
  const TailChoice c = tail_choose(opt_dim, history, n_linesearch, action_dim, batchsize, overlapped);
  return c.form | (c.shape << 4);
}

CUROBO_EXPORT int curobo_hip_launch_lbfgs_iteration_tail(
    float *best_cost, float *best_action, int16_t *best_iteration, int16_t *current_iteration,
    uint8_t *converged_global, int convergence_iteration, float cost_delta_threshold,
    float cost_relative_threshold, float *exploration_cost, float *exploration_action,
    float *exploration_gradient, int32_t *exploration_idx, float *selected_cost,
    float *selected_action, float *selected_gradient, int32_t *selected_idx,
    const float *search_cost, float *search_action, const float *search_gradient,
    float *step_direction_scaled, const float *search_magnitudes, float armijo_threshold_c_1,
    float curvature_threshold_c_2, int strong_wolfe, int approx_wolfe, int n_linesearch,
    int opt_dim, int batchsize, float *step_vec, float *rho_buffer, float *y_buffer, float *s_buffer,
    float *x_0, float *grad_0, float epsilon, int history_m, int stable_mode,
    const float *action_step_max, int action_dim, int apply_step_scale, int overlapped, curobo_hip_stream_t stream) {
  const char *what = "launch_lbfgs_iteration_tail";
  CUROBO_REQUIRE(n_linesearch >= 1 && n_linesearch <= kWave, "%s: n_linesearch=%d out of range [1,64]", what, n_linesearch);
  CUROBO_REQUIRE(history_m <= 31, "%s: History_m greater than 31 is not supported", what);
  CUROBO_REQUIRE(history_m >= 0, "%s: History_m less than 0 is not supported", what);
  CUROBO_REQUIRE(opt_dim >= 1 && opt_dim <= 2 * kWave, "%s: opt_dim=%d out of range [1,%d] (use the three separate launches)",
                 what, opt_dim, 2 * kWave);
  CUROBO_REQUIRE(action_dim >= 1 && opt_dim % action_dim == 0, "%s: opt_dim must be a multiple of action_dim", what);
  if (batchsize == 0) return CUROBO_HIP_OK;
  LineSearchArgs ls{best_cost, best_action, best_iteration, current_iteration, converged_global,
                    convergence_iteration, cost_delta_threshold, cost_relative_threshold,
                    exploration_cost, exploration_action, exploration_gradient, exploration_idx,
                    selected_cost, selected_action, selected_gradient, selected_idx,
                    search_cost, search_action, search_gradient, step_direction_scaled, search_magnitudes,
                    armijo_threshold_c_1, curvature_threshold_c_2, strong_wolfe, approx_wolfe,
                    n_linesearch, opt_dim, batchsize};
  LbfgsArgs lb{step_vec, rho_buffer, y_buffer, s_buffer, exploration_action, exploration_gradient, x_0, grad_0,
               epsilon, batchsize, history_m, opt_dim, stable_mode};
  PrepareArgs pr{search_action, step_direction_scaled, action_step_max, search_magnitudes, action_dim, apply_step_scale};
  hipStream_t st = (hipStream_t)stream;
  static const bool wg64 = getenv("CUROBO_HIP_TAIL_WG64") != nullptr;
  const dim3 grid((unsigned)ceil_div(batchsize, wg64 ? 1 : 4)), block(wg64 ? 64 : 256);
  const dim3 grid16((unsigned)ceil_div(batchsize, 16));
  const TailChoice c = tail_choose(opt_dim, history_m, n_linesearch, action_dim, batchsize, overlapped);
  if (c.form == kTailRow) {
    if (c.shape == 2) hipLaunchKernelGGL((lbfgs_iteration_tail_prefetch_kernel<1, 16, 4, CUROBO_TAIL_SHAPE_2>), grid16, block, 0, st, ls, lb, pr);
    else hipLaunchKernelGGL((lbfgs_iteration_tail_prefetch_kernel<1, 16, 4>), grid16, block, 0, st, ls, lb, pr);
  } else if (c.form == kTailWave) {
    if (c.shape == 1) hipLaunchKernelGGL((lbfgs_iteration_tail_prefetch_kernel<2, kWave, 4, CUROBO_TAIL_SHAPE_1>), grid, block, 0, st, ls, lb, pr);
    else if (opt_dim <= kWave) hipLaunchKernelGGL((lbfgs_iteration_tail_prefetch_kernel<1, kWave, 4>), grid, block, 0, st, ls, lb, pr);
    else hipLaunchKernelGGL((lbfgs_iteration_tail_prefetch_kernel<2, kWave, 4>), grid, block, 0, st, ls, lb, pr);
  } else if (c.form == kTailWorkgroup) {
    const int n_move = history_m > 0 ? (history_m - 1) * opt_dim : 0;
    const int rounds = ceil_div(n_move, kStageLanes);
    const size_t lds = (size_t)2 * (opt_dim + 1) * kHistRow * sizeof(float);
    const dim3 grid_wg((unsigned)batchsize);
    if (c.shape == 1) hipLaunchKernelGGL((lbfgs_iteration_tail_wg_kernel<2, 4, 12, CUROBO_TAIL_SHAPE_1>), grid_wg, block, lds, st, ls, lb, pr);
    else if (opt_dim <= kWave && rounds <= 12) hipLaunchKernelGGL((lbfgs_iteration_tail_wg_kernel<1, 4, 12>), grid_wg, block, lds, st, ls, lb, pr);
    else if (opt_dim <= kWave) hipLaunchKernelGGL((lbfgs_iteration_tail_wg_kernel<1, 4, 20>), grid_wg, block, lds, st, ls, lb, pr);
    else if (rounds <= 12) hipLaunchKernelGGL((lbfgs_iteration_tail_wg_kernel<2, 4, 12>), grid_wg, block, lds, st, ls, lb, pr);
    else hipLaunchKernelGGL((lbfgs_iteration_tail_wg_kernel<2, 4, 20>), grid_wg, block, lds, st, ls, lb, pr);
  } else if (opt_dim <= 16 && history_m <= 16 && n_linesearch <= 16 && getenv("CUROBO_HIP_NO_ROW16") == nullptr)
    hipLaunchKernelGGL((lbfgs_iteration_tail_kernel<1, 16>), grid16, block, 0, st, ls, lb, pr);  // IK-sized problems: one 16-lane row each
  else if (opt_dim <= kWave) hipLaunchKernelGGL((lbfgs_iteration_tail_kernel<1>), grid, block, 0, st, ls, lb, pr);
  else hipLaunchKernelGGL((lbfgs_iteration_tail_kernel<2>), grid, block, 0, st, ls, lb, pr);
  return check_launch(what, st);
}
