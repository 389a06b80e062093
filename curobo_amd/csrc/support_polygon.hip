// support_polygon.hip -- the support-polygon balance cost: 2-D convex hulls of the foot spheres and the smooth signed
// distance of the centre of mass to its hull, with the analytic gradient the FK VJP consumes.
// Reference (torch, no backend hook): geom/convex_polygon_helper.py:63-336 (ConvexPolygon2DHelper: a Python loop over
// the batch for the hulls, ~25 elementwise launches + autograd for the distance), cost/cost_support_polygon.py:35-109.
//
// Both kernels are tiny and latency / issue bound.  The hull build runs when the stance changes, never per iteration.
#include "common.hpp"

namespace curobo_hip {

constexpr int kHullMaxPoints = 64;   // one wave per hull, one input point per lane
constexpr int kHullStack = 2 * kHullMaxPoints;  // the chain's stack: n + 1 in exact arithmetic, 2 n - 1 whatever the rounding
constexpr int kHullsPerBlock = 4;
constexpr int kCostMaxVertices = 32;

struct ConvexHullArgs {
  float *hulls;
  int32_t *counts;
  const float *points;
  float padding;
  int n_hulls, n_pts;
};

// the turn of c against a -> b; products of two floats are exact in double, so the decision is that of the float64 statement
// of the reference up to the rounding of one sum
__device__ __forceinline__ double turn(float2 a, float2 b, float2 c) {
  return ((double)b.x - (double)a.x) * ((double)c.y - (double)a.y) - ((double)b.y - (double)a.y) * ((double)c.x - (double)a.x);
}

// Monotone chain over the points sorted by (x, y): the strictly convex vertices counter-clockwise (a vertex whose turn is
// <= 1e-10 is dropped, the reference's Graham-scan rule: convex_polygon_helper.py:158-173), rotated to start at the lowest
// vertex (leftmost among those within 1e-8 of the lowest y, :123-135), then moved by `padding` along the unit vector from the
// vertex mean (:186-216).  Rows past counts[i] repeat the last vertex (:94-104).
__global__ void __launch_bounds__(kWave *kHullsPerBlock) convex_hull_2d_kernel(const ConvexHullArgs a) {
  __shared__ float2 sorted[kHullsPerBlock][kHullMaxPoints];
  __shared__ float2 stack[kHullsPerBlock][kHullStack];
  __shared__ int meta[kHullsPerBlock][2];
  const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int hull = blockIdx.x * kHullsPerBlock + w;
  const bool valid = hull < a.n_hulls;
  const int n = a.n_pts;
  const float2 *pts = reinterpret_cast<const float2 *>(a.points) + (size_t)(valid ? hull : 0) * n;
  // ---- rank sort: lane i places point i (ties by index, so every rank is taken once)
  const bool has = valid && lane < n;
  float2 p = make_float2(0.f, 0.f);
  if (has) {
    p = pts[lane];
    stack[w][lane] = p;  // (the raw points, read by every lane below; the scan overwrites them afterwards)
  }
  __syncthreads();
  if (has) {
    int rank = 0;
    for (int j = 0; j < n; j++) {
      const float2 o = stack[w][j];
      rank += (o.x < p.x || (o.x == p.x && (o.y < p.y || (o.y == p.y && j < lane)))) ? 1 : 0;
    }
    sorted[w][min(rank, n - 1)] = p;
  }
  __syncthreads();
  // ---- the serial scan
  if (valid && lane == 0) {
    float2 *H = stack[w];
    const float2 *P = sorted[w];
    int k = 0;
    for (int i = 0; i < n; i++) {
      while (k >= 2 && turn(H[k - 2], H[k - 1], P[i]) <= 1e-10) k--;
      H[k++] = P[i];
    }
    const int t = k + 1;
    for (int i = n - 2; i >= 0; i--) {
      while (k >= t && turn(H[k - 2], H[k - 1], P[i]) <= 1e-10) k--;
      H[k++] = P[i];
    }
    const int count = max(1, min(k - 1, n));  // (the last vertex is the first again)
    float min_y = H[0].y;
    for (int i = 1; i < count; i++) min_y = fminf(min_y, H[i].y);
    int start = 0;
    float min_x = INFINITY;
    for (int i = 0; i < count; i++)
      if (fabsf(H[i].y - min_y) < 1e-8f && H[i].x < min_x) { min_x = H[i].x; start = i; }
    meta[w][0] = count;
    meta[w][1] = start;
  }
  __syncthreads();
  if (!valid) return;
  const int count = meta[w][0], start = meta[w][1];
  // ---- padding (in double: one rounding per coordinate) and the write, one row per lane
  double mx = 0.0, my = 0.0;
  for (int i = 0; i < count; i++) { mx += (double)stack[w][i].x; my += (double)stack[w][i].y; }
  mx /= (double)count; my /= (double)count;
  if (lane < n) {
    int src = start + min(lane, count - 1);
    src = src >= count ? src - count : src;
    const float2 v = stack[w][src];
    float2 o = v;
    if (a.padding > 0.0f && count > 1) {
      const double dx = (double)v.x - mx, dy = (double)v.y - my;
      const double nrm = sqrt(dx * dx + dy * dy);
      if (nrm > 1e-8) {
        o.x = (float)((double)v.x + dx / nrm * (double)a.padding);
        o.y = (float)((double)v.y + dy / nrm * (double)a.padding);
      }
    }
    reinterpret_cast<float2 *>(a.hulls)[(size_t)hull * n + lane] = o;
  }
  if (lane == 0) a.counts[hull] = count;
}

struct SupportPolygonArgs {
  float *cost, *grad_com, *signed_distance;
  const float *com, *hulls, *weight;
  const int32_t *counts, *idxs_hull;
  float inside_cost_weight, margin_target, smoothing;
  int batch, horizon, n_hulls, max_vertices, cost_mode;
};

// distance of p to the segment a -> b (reference _point_to_line_distance_optimized, :295-336, same order of operations);
// dx, dy = p - closest point
__device__ __forceinline__ float segment_distance(float2 p, float2 a, float2 b, float &dx, float &dy, float &cr) {
  const float ex = b.x - a.x, ey = b.y - a.y, px = p.x - a.x, py = p.y - a.y;
  const float t = fminf(fmaxf((px * ex + py * ey) / fmaxf(ex * ex + ey * ey, 1e-8f), 0.0f), 1.0f);
  dx = p.x - (a.x + t * ex);
  dy = p.y - (a.y + t * ey);
  cr = ex * py - ey * px;
  return sqrtf(dx * dx + dy * dy);
}

// One thread per (b, h).  Two passes over the hull's edges, four edges per trip with their five vertex loads issued together
// (the addresses do not depend on loaded data; a plain loop over a run-time count is one round trip per edge): pass 1 finds
// the smallest edge distance and the inside test, pass 2 recomputes the distances for the soft-min weights and the gradient
//   s = sum_k w_k d_k / Z,  ds/dp = sum_k w_k (1 - (d_k - s) / smoothing) u_k / Z,  w_k = exp(-(d_k - d_min) / smoothing),
// u_k = (p - c_k) / d_k (0 where d_k = 0, as torch.norm's backward has it).  Nothing is indexed by a run-time k: no scratch.
__global__ void __launch_bounds__(256) support_polygon_cost_kernel(const SupportPolygonArgs a) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)a.batch * a.horizon;
  if (tid >= total) return;
  const int b = (int)(tid / a.horizon);
  const float4 c = reinterpret_cast<const float4 *>(a.com)[tid];
  const float2 p = make_float2(c.x, c.y);
  const int hull = min(max(a.idxs_hull[b], 0), a.n_hulls - 1);
  const int M = a.max_vertices;
  const int cnt = a.counts ? min(max(a.counts[hull], 1), M) : M;
  const float2 *V = reinterpret_cast<const float2 *>(a.hulls) + (size_t)hull * M;
  constexpr int U = 4;
  float dmin = INFINITY;
  bool all_pos = true, all_neg = true;
  for (int k0 = 0; k0 < cnt; k0 += U) {
    float2 v[U + 1];
#pragma unroll
    for (int u = 0; u <= U; u++) {
      int i = min(k0 + u, cnt);  // (cnt wraps to vertex 0: the closing edge)
      v[u] = V[i == cnt ? 0 : i];
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      float dx, dy, cr;
      const float d = segment_distance(p, v[u], v[u + 1], dx, dy, cr);
      if (k0 + u < cnt) {
        dmin = fminf(dmin, d);
        all_pos = all_pos && cr >= -1e-8f;
        all_neg = all_neg && cr <= 1e-8f;
      }
    }
  }
  float Z = 0.f, S = 0.f, ax = 0.f, ay = 0.f, bx = 0.f, by = 0.f;
  for (int k0 = 0; k0 < cnt; k0 += U) {
    float2 v[U + 1];
#pragma unroll
    for (int u = 0; u <= U; u++) {
      int i = min(k0 + u, cnt);
      v[u] = V[i == cnt ? 0 : i];
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      float dx, dy, cr;
      const float d = segment_distance(p, v[u], v[u + 1], dx, dy, cr);
      if (k0 + u < cnt) {
        const float wk = expf((dmin - d) / a.smoothing);
        const float inv = d > 0.0f ? wk / d : 0.0f;
        Z += wk;
        S += wk * d;
        ax += inv * dx; ay += inv * dy;          // sum w u
        bx += wk * dx; by += wk * dy;            // sum w d u
      }
    }
  }
  const float s = S / Z;
  const float k1 = 1.0f + s / a.smoothing;
  float gx = (k1 * ax - bx / a.smoothing) / Z, gy = (k1 * ay - by / a.smoothing) / Z;
  const bool inside = all_pos || all_neg;
  const float sd = inside ? -s : s;
  if (inside) { gx = -gx; gy = -gy; }
  float cost, factor;
  if (a.cost_mode == 1) {  // the signed distance itself (ConvexPolygon2DHelper.compute_point_hull_distance)
    cost = sd;
    factor = 1.0f;
  } else if (a.inside_cost_weight > 0.0f) {
    // (the reference takes the inside branch on sd < 0, cost_support_polygon.py:99: a point of distance exactly 0 costs 0)
    const bool in_branch = sd < 0.0f;
    const float m = a.margin_target + sd;
    cost = in_branch ? a.inside_cost_weight * fmaxf(m, 0.0f) : sd;
    factor = in_branch ? (m > 0.0f ? a.inside_cost_weight : 0.0f) : 1.0f;
  } else {
    cost = fmaxf(sd, 0.0f);
    factor = sd > 0.0f ? 1.0f : 0.0f;
  }
  const float wgt = a.weight[0];
  a.cost[tid] = wgt * cost;
  reinterpret_cast<float4 *>(a.grad_com)[tid] = make_float4(wgt * factor * gx, wgt * factor * gy, 0.0f, 0.0f);
  if (a.signed_distance) a.signed_distance[tid] = sd;
}

}  // namespace curobo_hip

using namespace curobo_hip;

CUROBO_EXPORT int curobo_hip_convex_hull_2d(float *hulls, int32_t *counts, const float *points, float padding, int n_hulls,
                                            int n_pts, curobo_hip_stream_t stream) {
  const char *what = "convex_hull_2d";
  CUROBO_REQUIRE(n_pts >= 3 && n_pts <= kHullMaxPoints, "%s: n_pts must be in 3..%d, got %d", what, kHullMaxPoints, n_pts);
  CUROBO_REQUIRE(n_hulls >= 0, "%s: n_hulls must not be negative, got %d", what, n_hulls);
  CUROBO_REQUIRE(hulls && counts && points, "%s: hulls, counts and points must not be null", what);
  CUROBO_REQUIRE(((uintptr_t)hulls & 7) == 0 && ((uintptr_t)points & 7) == 0, "%s: hulls and points must be 8-byte aligned", what);
  CUROBO_REQUIRE(padding == padding, "%s: padding is NaN", what);
  if (n_hulls == 0) return CUROBO_HIP_OK;
  ConvexHullArgs a{hulls, counts, points, padding, n_hulls, n_pts};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(convex_hull_2d_kernel, dim3((unsigned)ceil_div(n_hulls, kHullsPerBlock)), dim3(kWave * kHullsPerBlock), 0,
                     st, a);
  return check_launch(what, st);
}

CUROBO_EXPORT int curobo_hip_support_polygon_cost(float *cost, float *grad_com, float *signed_distance, const float *com,
                                                  const float *hulls, const int32_t *counts, const int32_t *idxs_hull,
                                                  const float *weight, float inside_cost_weight, float margin_target,
                                                  float smoothing, int batch_size, int horizon, int n_hulls,
                                                  int max_vertices, int cost_mode, curobo_hip_stream_t stream) {
  const char *what = "support_polygon_cost";
  CUROBO_REQUIRE(max_vertices >= 1 && max_vertices <= kCostMaxVertices, "%s: max_vertices must be in 1..%d, got %d", what,
                 kCostMaxVertices, max_vertices);
  CUROBO_REQUIRE(batch_size >= 0 && horizon >= 1 && n_hulls >= 1, "%s: bad dimensions (batch %d, horizon %d, hulls %d)", what,
                 batch_size, horizon, n_hulls);
  CUROBO_REQUIRE(cost_mode == 0 || cost_mode == 1, "%s: cost_mode must be 0 (cost) or 1 (signed distance), got %d", what, cost_mode);
  CUROBO_REQUIRE(cost && grad_com, "%s: cost and grad_com must not be null", what);
  CUROBO_REQUIRE(com && hulls && idxs_hull && weight, "%s: com, hulls, idxs_hull and weight must not be null", what);
  CUROBO_REQUIRE(((uintptr_t)com & 15) == 0 && ((uintptr_t)grad_com & 15) == 0, "%s: com and grad_com must be 16-byte aligned", what);
  CUROBO_REQUIRE(((uintptr_t)hulls & 7) == 0, "%s: hulls must be 8-byte aligned", what);
  CUROBO_REQUIRE(smoothing > 0.0f, "%s: smoothing must be positive, got %g", what, (double)smoothing);
  CUROBO_REQUIRE(inside_cost_weight == inside_cost_weight && margin_target == margin_target, "%s: NaN parameter", what);
  const long total = (long)batch_size * horizon;
  if (total == 0) return CUROBO_HIP_OK;
  SupportPolygonArgs a{cost, grad_com, signed_distance, com, hulls, weight, counts, idxs_hull, inside_cost_weight,
                       margin_target, smoothing, batch_size, horizon, n_hulls, max_vertices, cost_mode};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(support_polygon_cost_kernel, dim3((unsigned)ceil_div_l(total, 256)), dim3(256), 0, st, a);
  return check_launch(what, st);
}
