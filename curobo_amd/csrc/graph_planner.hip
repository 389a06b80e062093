// graph_planner.hip -- kernels of the PRM graph planner: weighted k-nearest neighbours, then edge steering (further down).
//
// Weighted k-nearest neighbours (reference DistanceNeighborCalculator
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
#include "fused_device.hpp"

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

// ------------------------------------------------------------------------------------------
// Graph-planner edge steering (reference LinearConnector.steer_until_infeasible,
// graph_planner/graph/connector_linear.py:75-192) without materialising the interpolated points:
// a workgroup walks one edge's points k = 0 .. max_steps (coefficient k / max_steps, max_steps the
// batch-wide count of graph_steer_max_steps_kernel) in chunks of 16 -- one 16-lane row per point,
// the same FK / self / scene device functions and LDS tables as the IK launch (fused_device.hpp, rollout_ik_fused.hip) -- and stops
// at the first chunk holding an infeasible point.  Feasible = scene cost, self-collision cost and
// joint-bound cost all exactly 0 with activation distance 0 (RobotCollisionChecker.validate).
// point_mode: 16 configurations per workgroup (start rows only), out_feasible[n] per configuration.
struct FusedSteerArgs {
  FusedTrajArgs r;             // robot / self / scene members (no outputs)
  const float *start, *target;  // [n, ld] rows, the first dof columns used
  const float *p_b;             // joint limits [2, dof]
  const int32_t *max_steps;     // [1] batch-wide step count (edge mode)
  float *out_node;              // [n, dof + 1] last feasible point, index column 0 (edge mode)
  int32_t *out_index;           // [n] its step index (edge mode)
  uint8_t *out_feasible;        // [n] (point mode)
  int n, ld, point_mode;
};

// num_steps = ceil(max_k |w_k (t_k - s_k)| / threshold) + 1, reduced over the batch in one workgroup (no host sync)
__global__ void __launch_bounds__(1024) graph_steer_max_steps_kernel(const float *start, const float *target, const float *w,
                                                                      float threshold, int n, int ld, int dof, int32_t *out) {
  __shared__ int red[16];
  int m = 0;
  for (int e = threadIdx.x; e < n; e += blockDim.x) {
    float mx = 0.0f;
    for (int d = 0; d < dof; d++) mx = fmaxf(mx, fabsf(__fmul_rn(target[(size_t)e * ld + d] - start[(size_t)e * ld + d], w[d])));
    m = max(m, (int)ceilf(__fdiv_rn(mx, threshold)) + 1);
  }
  m = -wave64_min(-m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < (int)(blockDim.x >> 6); i++) m = max(m, red[i]);
    out[0] = max(m, red[0]);
  }
}

// point of step k of edge e: start + (k / max_steps) * (target - start), each operation rounded on its own as in torch
__device__ __forceinline__ float steer_point(const float *s, const float *t, int d, int k, int max_steps) {
  const float cf = __fdiv_rn((float)k, (float)max_steps);
  return __fadd_rn(s[d], __fmul_rn(cf, t[d] - s[d]));
}

template <int KINDS>
__global__ void __launch_bounds__(256, 4) graph_steer_kernel(const FusedSteerArgs ga) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ int first_bad;
  const FusedTrajArgs &a = ga.r;
  const int H = kIkPoints, D = a.bs.dof, L = a.nlinks, S = a.nspheres, P = a.npairs;
  const int n_rec = a.sc.max_cuboids + a.sc.max_voxel_grids;
  const FusedLayout lay = fused_layout(H, D, L, S, a.chain_len, P, n_rec, 0, 0, 1, 0, false);
  const int tid = threadIdx.x;
  FusedCtx c;
  fused_ctx_carve(c, smem, lay, H, D, L, S, P);
  c.env = 0;
  c.w_self = 1.0f; c.w_scene = 1.0f; c.eta = 0.0f;
  c.speed_metric = false; c.speed_dt = 0.0f;
  fused_stage_tables(c, a, lay, reinterpret_cast<const float4 *>(a.robot_spheres), n_rec);
  __syncthreads();
  fused_derive_tables(c);
  const int h = tid / kFkLanes, lane = tid % kFkLanes;
  const int max_steps = ga.point_mode ? 1 : ga.max_steps[0];
  const int n_pts = max_steps + 1;  // points per edge
  const int n_items = ga.point_mode ? (ga.n + H - 1) / H : ga.n;
  for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
    const int e = ga.point_mode ? -1 : item;
    const float *s = ga.start + (size_t)(ga.point_mode ? 0 : e) * ga.ld, *t = ga.target + (size_t)(ga.point_mode ? 0 : e) * ga.ld;
    int result = n_pts;  // first infeasible step (n_pts = none)
    for (int k0 = 0; k0 < (ga.point_mode ? 1 : n_pts); k0 += H) {
      const int k = k0 + h;
      const int row = ga.point_mode ? item * H + h : e;
      const bool live = ga.point_mode ? row < ga.n : k < n_pts;
      __syncthreads();  // the previous chunk's readers of q / spheres / first_bad are done
      if (tid == 0) first_bad = 0x7fffffff;
      if (live && lane < D)
        for (int d = lane; d < D; d += kFkLanes)
          c.q[h * D + d] = ga.point_mode ? ga.start[(size_t)row * ga.ld + d] : steer_point(s, t, d, k, max_steps);
      __syncthreads();
      bool bad = false;
      if (live) {
        point_fk_row(c, a, 0, h, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (no workgroup barrier between the row's spheres and their readers here)
        __builtin_amdgcn_wave_barrier();
        // joint bounds (cspace_bound_term with unit weight and no activation margin, as RobotCollisionChecker.get_bound)
        float viol = 0.0f;
        for (int d = lane; d < D; d += kFkLanes) {
          float g;
          viol += cspace_bound_term(c.q[h * D + d], ga.p_b[d], ga.p_b[D + d], 1.0f, g);
        }
        // self collision: the largest pair penetration of the row (the IK launch's first pass)
        float pen = 0.0f;
        if (a.use_self) {
          const float4 *sph = c.spheres(h);
          const int P_pad = (P + 63) & ~63;
          for (int k1 = lane; k1 < P_pad; k1 += kFkLanes) pen = fmaxf(pen, staged_pair_penetration(sph, c.pairs[k1]));
        }
        // scene cost of every sphere (activation distance 0)
        float dsc = 0.0f;
        if (a.use_scene) {
          point_link_masks<0, KINDS>(c, a.sc, h, lane);
          const float *wr = c.wrench + (size_t)h * c.wl;
          for (int s0 = 0; s0 < S; s0 += kFkLanes) {  // (a copy of the sphere-per-lane scene loop of the trajectory kernel's row fallback, without the wrenches)
            const int sp = s0 + lane;
            float d = 0.0f;
            f3 g = make_f3(0.f, 0.f, 0.f);
            const uint32_t mask = sp < S ? __float_as_uint(wr[c.sph_link[sp] * kWrench + 6]) : 0u;
            if (sp < S && (mask != 0u || n_rec > 32)) scene_sphere<0, KINDS>(c, a.sc, h, sp, d, g, mask);
            dsc += d;
          }
        }
        const float tot = row16_max(fmaxf(fmaxf(viol, pen), dsc));
        bad = tot > 0.0f;
      }
      if (ga.point_mode) {
        if (live && lane == 0) ga.out_feasible[row] = bad ? 0 : 1;
        continue;
      }
      if (bad && lane == 0) atomicMin(&first_bad, k);
      __syncthreads();
      if (first_bad != 0x7fffffff) { result = first_bad; break; }
    }
    if (ga.point_mode) continue;
    // the point before the first infeasible one (clamped to 0); the end point when there is none
    const int idx = result < n_pts ? max(result - 1, 0) : n_pts - 1;
    for (int d = tid; d <= D; d += blockDim.x)
      ga.out_node[(size_t)e * (D + 1) + d] = d < D ? steer_point(s, t, d, idx, max_steps) : 0.0f;
    if (tid == 0) ga.out_index[e] = idx;
  }
}

CUROBO_EXPORT int curobo_hip_graph_steer(
    float *out_node, int32_t *out_index, uint8_t *out_feasible, int32_t *max_steps_ws, const float *start, const float *target,
    int ld, const float *cspace_distance_weight, float cspace_similarity_threshold, int n, int point_mode, const float *p_b,
    const float *fixed_transform, const float *robot_spheres, const int8_t *joint_map_type, const int16_t *joint_map,
    const int16_t *link_map, const int16_t *link_sphere_map, const int16_t *link_chain_data, const int16_t *link_chain_offsets,
    const float *joint_offset_map, const float *sphere_padding, const int16_t *pair_locations, const curobo_hip_scene *scene,
    int dof, int num_links, int num_spheres, int num_collision_pairs, int link_chain_len, curobo_hip_stream_t stream) {
  const char *what = "graph_steer";
  if (const int bad = fused_check_dimensions(what, num_links, num_spheres, link_chain_len, pair_locations)) return bad;
  CUROBO_REQUIRE(dof >= 1 && dof <= 64 && ld >= dof, "%s: bad dimensions", what);
  CUROBO_REQUIRE(point_mode ? out_feasible != nullptr : (out_node && out_index && max_steps_ws && cspace_distance_weight
                 && target && cspace_similarity_threshold > 0.0f), "%s: missing outputs / inputs for this mode", what);
  if (n == 0) return CUROBO_HIP_OK;
  FusedSteerArgs ga{};
  FusedTrajArgs &a = ga.r;
  fused_fill_robot_args(a, false, fixed_transform, robot_spheres, joint_map_type, joint_map, link_map, link_sphere_map, link_chain_data,
                        link_chain_offsets, joint_offset_map, sphere_padding, nullptr, pair_locations, scene, nullptr, nullptr, nullptr,
                        1, 0, n, dof, num_links, num_spheres, num_collision_pairs, link_chain_len);
  ga.start = start; ga.target = point_mode ? start : target; ga.p_b = p_b; ga.max_steps = max_steps_ws;
  ga.out_node = out_node; ga.out_index = out_index; ga.out_feasible = out_feasible;
  ga.n = n; ga.ld = ld; ga.point_mode = point_mode ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  const int n_rec = a.sc.max_cuboids + a.sc.max_voxel_grids;
  const FusedLayout lay = fused_layout(kIkPoints, dof, num_links, num_spheres, link_chain_len, a.npairs, n_rec, 0, 0, 1, 0, false);
  const size_t lds = (size_t)lay.total * sizeof(float);
  CUROBO_REQUIRE(lds <= 160 * 1024 - 64, "%s: 16 configurations do not fit in LDS (%zu bytes)", what, lds);
  if (!point_mode) {
    hipLaunchKernelGGL(graph_steer_max_steps_kernel, dim3(1), dim3(1024), 0, st, start, target, cspace_distance_weight,
                       cspace_similarity_threshold, n, ld, dof, max_steps_ws);
    const int err = check_launch("graph_steer_max_steps", st);
    if (err != CUROBO_HIP_OK) return err;
  }
  const int kinds = fused_scene_kinds(a.sc), items = point_mode ? ceil_div(n, kIkPoints) : n;
  const dim3 grid((unsigned)(items < 2048 ? items : 2048)), block(kIkPoints * kFkLanes);
  const auto kfn = kinds == 2 ? graph_steer_kernel<2> : kinds == 3 ? graph_steer_kernel<3> : kinds == 7 ? graph_steer_kernel<7> : graph_steer_kernel<1>;
  // (the kernel also has static LDS: the limit is raised 4 KB below what a kernel may take unasked)
  return fused_launch_status(what, fused_launch(kfn, grid, block, lds, 60 * 1024, st, ga), st);
}

}  // namespace curobo_hip
