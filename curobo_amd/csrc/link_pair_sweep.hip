// link_pair_sweep.hip -- per-LINK-PAIR statistics of a batch of configurations, for the self-collision matrix builder
// (reference: RobotBuilder._prune_collision_pairs / _check_default_joint_configuration_collisions,
// robot/builder/builder_robot.py:993-1172, which store the distance of every sphere pair, [N, P] floats, and walk the link
// pairs on the host).  Here the sphere pairs of a configuration are reduced where they are evaluated: per group g (= one
// link pair, a contiguous run of the group-sorted pair list)
//   max_penetration[g] = max over the N points and the group's valid pairs of (r_i + pad_i) + (r_j + pad_j) - |c_i - c_j|
//   collision_count[g] = number of points at which some valid pair of the group penetrates (> 0)
// and [N, P] never exists.
//
// gfx950 design: one 256-thread workgroup walks a chunk of points.  LDS holds the point's spheres (staged once, padding
// added, disabled spheres marked) and three arrays of G words: the group maxima of this point, the running maxima and the
// running counts of the chunk.  A lane takes kRun consecutive pairs per trip (two 16-byte loads of pair dwords, two of group
// ids), folds them in registers and flushes on a group change with an LDS INTEGER max on the order-preserving integer image
// of the float -- the only atomics of the launch, no floating-point atomic anywhere.  After a point the arrays are merged by
// threads strided over g (thread g % 256 owns group g in every merge: no barrier between merge and the final write).  The
// chunks' partials [n_chunks, G] are reduced by a second, small launch.  max is exact and the counts are integers, so the
// result does not depend on the order of the atomics nor on how the points are split over workgroups: bit-identical from
// run to run and for every points_per_workgroup.
#include "common.hpp"

namespace curobo_hip {

constexpr int kSweepThreads = 256;
constexpr int kSweepRun = 8;                   // consecutive pairs a lane folds per trip
constexpr int kKeyNegInf = (int)0x807fffffu;   // float_key(-inf)

// order-preserving integer image of a float (signed compare; its own inverse): -inf < ... < -0 < +0 < ... < +inf
__device__ __forceinline__ int float_key(float v) {
  const int b = __float_as_int(v);
  return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float key_float(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }

struct SweepArgs {
  float *part_max;  // [n_chunks, G]
  int *part_cnt;    // [n_chunks, G]
  const float4 *spheres;
  const float *padding;
  const uint32_t *pairs;  // (i | j << 16) per pair
  const int *group;
  int n_points, S, P, G, ppw;
};

__global__ void __launch_bounds__(kSweepThreads) link_pair_sweep_kernel(const SweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int S = a.S, P = a.P, G = a.G, tid = threadIdx.x;
  float4 *sph = reinterpret_cast<float4 *>(smem);   // [S]
  int *cur = reinterpret_cast<int *>(sph + S);      // [G] this point's group maxima (keys)
  int *run_max = cur + G;                           // [G] the chunk's
  int *run_cnt = run_max + G;                       // [G] points of the chunk at which the group penetrates
  for (int g = tid; g < G; g += kSweepThreads) {
    cur[g] = kKeyNegInf;
    run_max[g] = kKeyNegInf;
    run_cnt[g] = 0;
  }
  const float ninf = -__builtin_inff();
  const int n0 = blockIdx.x * a.ppw, n1 = n0 + min(a.ppw, a.n_points - n0);  // (ppw <= n_points: the host clamps it)
  for (int n = n0; n < n1; n++) {
    // ---- the point's spheres, once: padded radius; a disabled sphere (padded radius < 0, the rule of pair_penetration in
    // self_device.hpp) carries NaN, so every pair of it compares false below
    const float4 *src = a.spheres + (size_t)n * S;
    for (int s = tid; s < S; s += kSweepThreads) {
      float4 v = src[s];
      v.w += a.padding[s];
      if (!(v.w >= 0.0f)) v.w = __builtin_nanf("");
      sph[s] = v;
    }
    __syncthreads();  // spheres staged, cur[] reset (by the previous merge)
    for (int base = tid * kSweepRun; base < P; base += kSweepThreads * kSweepRun) {
      uint32_t ij[kSweepRun];
      int gg[kSweepRun];
      if (base + kSweepRun <= P) {
        const uint4 p0 = *reinterpret_cast<const uint4 *>(a.pairs + base), p1 = *reinterpret_cast<const uint4 *>(a.pairs + base + 4);
        const int4 g0 = *reinterpret_cast<const int4 *>(a.group + base), g1 = *reinterpret_cast<const int4 *>(a.group + base + 4);
        ij[0] = p0.x; ij[1] = p0.y; ij[2] = p0.z; ij[3] = p0.w; ij[4] = p1.x; ij[5] = p1.y; ij[6] = p1.z; ij[7] = p1.w;
        gg[0] = g0.x; gg[1] = g0.y; gg[2] = g0.z; gg[3] = g0.w; gg[4] = g1.x; gg[5] = g1.y; gg[6] = g1.z; gg[7] = g1.w;
      } else {  // the list's last, incomplete run
#pragma unroll
        for (int u = 0; u < kSweepRun; u++) {
          const int k = base + u;
          ij[u] = k < P ? a.pairs[k] : 0u;
          gg[u] = k < P ? a.group[k] : -1;
        }
      }
      int open = -1;  // the group being folded (-1: none)
      float m = ninf;
      auto flush = [&]() {
        if (open >= 0 && m > ninf) atomicMax(&cur[open], float_key(m));
      };
#pragma unroll
      for (int u = 0; u < kSweepRun; u++) {
        const int i = (int)(ij[u] & 0xffffu), j = (int)(ij[u] >> 16);
        // (an index outside the tables is skipped, never followed: negative int16 values arrive here as >= 32768)
        const int g = ((unsigned)gg[u] < (unsigned)G && i < S && j < S) ? gg[u] : -1;
        if (g != open) {
          flush();
          open = g;
          m = ninf;
        }
        if (g >= 0) {
          const float4 s1 = sph[i], s2 = sph[j];
          const float dx = s1.x - s2.x, dy = s1.y - s2.y, dz = s1.z - s2.z;
          const float pen = (s1.w + s2.w) - sqrtf(dx * dx + dy * dy + dz * dz);
          if (pen > m) m = pen;  // (NaN: a disabled sphere)
        }
      }
      flush();
    }
    __syncthreads();  // every pair of the point is in cur[]; nobody reads sph[] any more
    for (int g = tid; g < G; g += kSweepThreads) {
      const int c = cur[g];
      if (c > run_max[g]) run_max[g] = c;
      run_cnt[g] += c > 0 ? 1 : 0;  // key > key(+0) = 0 <=> penetration > 0
      cur[g] = kKeyNegInf;
    }
  }
  for (int g = tid; g < G; g += kSweepThreads) {
    a.part_max[(size_t)blockIdx.x * G + g] = key_float(run_max[g]);
    a.part_cnt[(size_t)blockIdx.x * G + g] = run_cnt[g];
  }
}

// out[g] = (max, sum) over the chunks' partials; `accumulate`: folded into what out[] already holds (the next batch)
__global__ void __launch_bounds__(kSweepThreads) link_pair_reduce_kernel(float *out_max, int *out_cnt, const float *part_max,
                                                                         const int *part_cnt, int n_chunks, int G, int accumulate) {
  const int g = blockIdx.x * kSweepThreads + threadIdx.x;
  if (g >= G) return;
  float m = accumulate ? out_max[g] : -__builtin_inff();
  int c = accumulate ? out_cnt[g] : 0;
  for (int k = 0; k < n_chunks; k++) {
    const float v = part_max[(size_t)k * G + g];
    m = v > m ? v : m;
    c += part_cnt[(size_t)k * G + g];
  }
  out_max[g] = m;
  out_cnt[g] = c;
}

}  // namespace curobo_hip

using namespace curobo_hip;

CUROBO_EXPORT int curobo_hip_link_pair_sweep(
    float *max_penetration, int32_t *collision_count, float *partial_max, int32_t *partial_count, int partial_chunks,
    const float *robot_spheres, const float *sphere_padding, const int16_t *pair_locations, const int32_t *pair_group,
    int n_points, int nspheres, int num_pairs, int n_groups, int points_per_workgroup, int accumulate,
    curobo_hip_stream_t stream) {
  const char *what = "link_pair_sweep";
  CUROBO_REQUIRE(nspheres >= 1 && nspheres <= 1024, "%s: nspheres=%d out of range [1,1024]", what, nspheres);
  CUROBO_REQUIRE(n_groups >= 1 && n_groups <= 4096, "%s: n_groups=%d out of range [1,4096]", what, n_groups);
  CUROBO_REQUIRE(num_pairs >= 0 && n_points >= 0, "%s: negative num_pairs / n_points", what);
  CUROBO_REQUIRE(points_per_workgroup >= 1, "%s: points_per_workgroup=%d must be >= 1", what, points_per_workgroup);
  CUROBO_REQUIRE(max_penetration && collision_count, "%s: NULL output", what);
  if (n_points > 0 && points_per_workgroup > n_points) points_per_workgroup = n_points;
  const long n_chunks = ceil_div_l(n_points, points_per_workgroup);
  CUROBO_REQUIRE(n_chunks <= partial_chunks, "%s: the partial buffers hold %d chunks, %ld are needed", what, partial_chunks, n_chunks);
  hipStream_t st = (hipStream_t)stream;
  if (n_chunks > 0) {
    CUROBO_REQUIRE(partial_max && partial_count && robot_spheres && sphere_padding, "%s: NULL input", what);
    CUROBO_REQUIRE(num_pairs == 0 || (pair_locations && pair_group), "%s: NULL pair tables", what);
    CUROBO_REQUIRE(((uintptr_t)pair_locations & 15) == 0 && ((uintptr_t)pair_group & 15) == 0 && ((uintptr_t)robot_spheres & 15) == 0,
                   "%s: robot_spheres, pair_locations and pair_group must be 16-byte aligned", what);
    SweepArgs a{};
    a.part_max = partial_max; a.part_cnt = partial_count;
    a.spheres = reinterpret_cast<const float4 *>(robot_spheres); a.padding = sphere_padding;
    a.pairs = reinterpret_cast<const uint32_t *>(pair_locations); a.group = pair_group;
    a.n_points = n_points; a.S = nspheres; a.P = num_pairs; a.G = n_groups; a.ppw = points_per_workgroup;
    const size_t lds = (size_t)nspheres * 16 + (size_t)n_groups * 12;  // <= 16 KiB + 48 KiB
    static bool attr = false;
    if (!attr) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(link_pair_sweep_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
      attr = true;
    }
    hipLaunchKernelGGL(link_pair_sweep_kernel, dim3((unsigned)n_chunks), dim3(kSweepThreads), lds, st, a);
  }
  hipLaunchKernelGGL(link_pair_reduce_kernel, dim3((unsigned)ceil_div(n_groups, kSweepThreads)), dim3(kSweepThreads), 0, st,
                     max_penetration, collision_count, partial_max, partial_count, (int)n_chunks, n_groups, accumulate);
  return check_launch(what, st);
}
