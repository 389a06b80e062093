// Weighted k-nearest neighbours of the PRM graph planner (reference DistanceNeighborCalculator
// .jit_find_nearest_neighbors, graph_planner/graph/node_distance.py:128-155: cdist over
// weighted configurations, then a stable top-k, smallest first).
//
// One wave per query.  Lane i < k holds slot i of the query's sorted top-k list (key = squared
// weighted distance in fp64, then node index), so the list lives in registers and needs no
// dynamic indexing.  The wave scans the nodes 64 at a time (one per lane, in index order); a node
// whose key is below the current k-th key is inserted by a one-step shift of the list
// (lanes at or past its rank take their left neighbour's slot).  Nodes are scanned in increasing
// index order and a node only displaces strictly larger keys, so equal distances keep the lower
// node index first, as a stable top-k does.  fp64 keeps the order that of exact arithmetic for
// fp32 inputs up to ties that are ties in fp32 too (duplicated nodes).
#include "common.hpp"

#include <hip/hip_runtime.h>

#include <climits>

namespace curobo_hip {
namespace {

__device__ __forceinline__ bool key_less(double ad, int ai, double bd, int bi) { return ad < bd || (ad == bd && ai < bi); }

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

__global__ void __launch_bounds__(256) graph_knn_kernel(const float *__restrict__ queries, int ld_q, const float *__restrict__ nodes,
                                                        int ld_n, const float *__restrict__ weight, int n_queries, int n_nodes, int dof,
                                                        int k, int32_t *__restrict__ out_idx) {
  const int lane = threadIdx.x & 63;
  const int qi = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (qi >= n_queries) return;  // whole wave
  const float *q = queries + (size_t)qi * ld_q;
  double slot_d = __builtin_huge_val();
  int slot_i = INT_MAX;
  for (int base = 0; base < n_nodes; base += 64) {
    const int n = base + lane;
    double dist = __builtin_huge_val();
    if (n < n_nodes) {
      const float *x = nodes + (size_t)n * ld_n;
      dist = 0.0;
      for (int d = 0; d < dof; d++) {
        const double v = ((double)x[d] - (double)q[d]) * (double)weight[d];
        dist = fma(v, v, dist);
      }
    }
    const double thr_d = readlane_f64(slot_d, k - 1);
    const int thr_i = __builtin_amdgcn_readlane(slot_i, k - 1);
    unsigned long long cand = __ballot(n < n_nodes && key_less(dist, n, thr_d, thr_i));
    while (cand) {
      const int src = __builtin_ctzll(cand);
      cand &= cand - 1;
      const double cd = readlane_f64(dist, src);
      const int ci = base + src;
      if (!key_less(cd, ci, readlane_f64(slot_d, k - 1), __builtin_amdgcn_readlane(slot_i, k - 1))) continue;
      const double left_d = __shfl_up(slot_d, 1, 64);
      const int left_i = __shfl_up(slot_i, 1, 64);
      if (lane < k && !key_less(slot_d, slot_i, cd, ci)) {  // this slot moves right by one, the first such takes the node
        const bool first = lane == 0 || key_less(left_d, left_i, cd, ci);
        slot_d = first ? cd : left_d;
        slot_i = first ? ci : left_i;
      }
    }
  }
  if (lane < k) out_idx[(size_t)qi * k + lane] = slot_i;
}

}  // namespace

CUROBO_EXPORT int curobo_hip_graph_knn(int32_t *out_idx, const float *queries, int ld_q, const float *nodes, int ld_n,
                                       const float *cspace_distance_weight, int n_queries, int n_nodes, int dof, int k,
                                       curobo_hip_stream_t stream) {
  const char *what = "graph_knn";
  CUROBO_REQUIRE(dof >= 1 && ld_q >= dof && ld_n >= dof, "%s: bad dimensions", what);
  CUROBO_REQUIRE(k >= 1 && k <= 64, "%s: k must be in [1, 64], got %d", what, k);
  CUROBO_REQUIRE(k <= n_nodes, "%s: k = %d exceeds the %d nodes searched", what, k, n_nodes);
  if (n_queries == 0) return CUROBO_HIP_OK;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(graph_knn_kernel, dim3((unsigned)ceil_div(n_queries, 4)), dim3(256), 0, st, queries, ld_q, nodes, ld_n,
                     cspace_distance_weight, n_queries, n_nodes, dof, k, out_idx);
  return check_launch(what, st);
}

}  // namespace curobo_hip
