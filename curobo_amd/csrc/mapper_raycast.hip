// mapper_raycast.hip -- the TSDF read back along camera rays (curobo_amd/perception/mapper/renderer.py, pose_refiner.py):
//   curobo_hip_mapper_raycast    one lane per pixel: march the ray, refine the first sign change, the normal at the hit
//   curobo_hip_mapper_ray_align  one lane per (sampled pixel, sample along its ray): the along-ray SDF residual and its
//                                Jacobian row, summed into one pose_device.hpp row per workgroup
//
// Reference: perception/mapper/kernel/builder/builder_raycast.py (refine_hit_bisection :381-422, ray_block_exit_t :424-461,
// raycast_block_sparse_kernel :467-573, raycast_block_sparse_accelerated_kernel :690-834) and
// kernel/wp_raycast_pose_refine.py (_ray_sdf_alignment_block_sparse_tiled_kernel :100-316).  The grid's addressing, the samplers
// (under the sample rule, tsdf_voxel), the camera and the pixel's ray are mapper_device.hpp's.  The reference asks its hash table
// whether a block is allocated; here that is the byte block_mask, and a block outside the grid is not allocated.
//
// Range of the casts: tsdf_trilinear turns floor(v - 0.5) of the continuous voxel coordinate v into an int.  Both launches
// compare v with the padded grid's extent in float first (ray_sample, ray_gradient): a position further out than one voxel
// (three for the gradient) has no valid corner, so the answer is known without the cast.  The accelerated march keeps the
// block coordinate floor(v / block_size) in float and converts it only once it lies inside the grid.
#include "mapper_device.hpp"
#include "pose_device.hpp"

namespace curobo_hip {

constexpr int kRayTile = 16, kRayThreads = kRayTile * kRayTile;  // a workgroup's rays stay in neighbouring voxels
constexpr int kHitRefineIterations = 10;                         // builder_raycast.py:57
constexpr int kRayMaxSteps = 10000;                              // :518, :754
constexpr int kAlignThreads = 256, kAlignWaves = kAlignThreads / kWave;

struct RayMap {
  const uint32_t *block_data;
  const uint8_t *block_mask;
  MapGrid g;
};

__device__ __forceinline__ bool ray_within(const MapGrid &g, f3 p, float margin) {
  const f3 v = grid_continuous(g, p);
  return v.x >= -margin && v.x < (float)(g.nbx * g.bs) + margin && v.y >= -margin && v.y < (float)(g.nby * g.bs) + margin &&
         v.z >= -margin && v.z < (float)(g.nbz * g.bs) + margin;  // (false for a coordinate that is not a number)
}
__device__ __forceinline__ float ray_sample(const RayMap &m, f3 p) {
  return ray_within(m.g, p, 1.0f) ? tsdf_trilinear(m.block_data, m.block_mask, m.g, p) : kSdfInvalid;
}
__device__ __forceinline__ f3 ray_gradient(const RayMap &m, f3 p) {
  return ray_within(m.g, p, 3.0f) ? tsdf_gradient<true>(m.block_data, m.block_mask, m.g, p) : make_f3(0.0f, 0.0f, 1.0f);
}

__device__ __forceinline__ bool pose_is_finite(const float *position, const float *quaternion) {
  return isfinite(position[0]) && isfinite(position[1]) && isfinite(position[2]) && isfinite(quaternion[0]) && isfinite(quaternion[1]) &&
         isfinite(quaternion[2]) && isfinite(quaternion[3]);
}

// refine_hit_bisection (:381-422): regula falsi between the last positive and the first negative sample
__device__ __forceinline__ float ray_refine_hit(const RayMap &m, f3 cam, f3 ray, float t_lo, float t_hi, float sdf_lo, float sdf_hi) {
  float denom = sdf_lo - sdf_hi;
  if (fabsf(denom) < 1e-6f) return (t_lo + t_hi) * 0.5f;
  float t_mid = t_lo + sdf_lo * (t_hi - t_lo) / denom;
  for (int it = 0; it < kHitRefineIterations; it++) {
    const float sdf_mid = ray_sample(m, cam + t_mid * ray);
    if (sdf_is_invalid(sdf_mid)) break;
    if (fabsf(sdf_mid) < 1e-6f) break;
    if (sdf_mid > 0.0f) t_lo = t_mid, sdf_lo = sdf_mid;
    else t_hi = t_mid, sdf_hi = sdf_mid;
    denom = sdf_lo - sdf_hi;
    t_mid = fabsf(denom) < 1e-6f ? (t_lo + t_hi) * 0.5f : t_lo + sdf_lo * (t_hi - t_lo) / denom;
  }
  return t_mid;
}

// ray_block_exit_t (:424-461) for the block whose coordinate is b (whole numbers held as floats); wp.sign(0) is +1
__device__ __forceinline__ float ray_block_exit(const MapGrid &g, f3 o, f3 d, f3 b) {
  const f3 lo = make_f3(grid_face<false>(g, b.x, g.grid_w, g.ox), grid_face<false>(g, b.y, g.grid_h, g.oy), grid_face<false>(g, b.z, g.grid_d, g.oz));
  const f3 hi = make_f3(grid_face<true>(g, b.x, g.grid_w, g.ox), grid_face<true>(g, b.y, g.grid_h, g.oy), grid_face<true>(g, b.z, g.grid_d, g.oz));
  const float ix = fabsf(d.x) > 1e-8f ? 1.0f / d.x : (d.x < 0.0f ? -1e10f : 1e10f);
  const float iy = fabsf(d.y) > 1e-8f ? 1.0f / d.y : (d.y < 0.0f ? -1e10f : 1e10f);
  const float iz = fabsf(d.z) > 1e-8f ? 1.0f / d.z : (d.z < 0.0f ? -1e10f : 1e10f);
  const float tx = fmaxf((lo.x - o.x) * ix, (hi.x - o.x) * ix), ty = fmaxf((lo.y - o.y) * iy, (hi.y - o.y) * iy);
  const float tz = fmaxf((lo.z - o.z) * iz, (hi.z - o.z) * iz);
  return fminf(fminf(tx, ty), tz);
}

struct RaycastArgs {
  float *hit_points, *hit_normals, *hit_depths;
  uint8_t *hit_mask;
  const float *intrinsics, *position, *quaternion;
  RayMap m;
  float t_min, t_max;
  int height, width, max_steps, z_depth;
};

// ACCEL = false: raycast_block_sparse_kernel; true: raycast_block_sparse_accelerated_kernel.  The two sample at different t.
template <bool ACCEL>
__global__ __launch_bounds__(kRayThreads) void mapper_raycast_kernel(RaycastArgs a) {
  const int px = blockIdx.x * kRayTile + threadIdx.x % kRayTile, py = blockIdx.y * kRayTile + threadIdx.x / kRayTile;
  if (px >= a.width || py >= a.height) return;
  const size_t pixel = (size_t)py * a.width + px;
  const MapGrid &g = a.m.g;
  const MapCamera camera = read_camera(a.intrinsics, a.position, a.quaternion, 0);
  const f3 cam = camera.t;
  const f3 r = pixel_ray<true>(camera, px, py);
  const float ray_len = sqrtf(r.x * r.x + r.y * r.y + 1.0f);
  const f3 ray_cam = make_f3(r.x / ray_len, r.y / ray_len, 1.0f / ray_len);
  const f3 ray = quat_rotate(camera.qw, camera.qv, ray_cam);
  const float step = g.vs * 0.5f;  // MIN_STEP_SCALE

  float t = a.t_min, prev_sdf = kSdfInvalid, prev_t = a.t_min, hit_t = 0.0f;
  bool hit = false;
  f3 cur = make_f3(-999999.0f, -999999.0f, -999999.0f);
  bool allocated = false;
  float exit_t = 0.0f;
  const int n_iterations = pose_is_finite(a.position, a.quaternion) ? (ACCEL ? kRayMaxSteps : a.max_steps) : 0;
  for (int it = 0; it < n_iterations; it++) {
    if (!(t <= a.t_max)) break;  // (also ends a march whose t is no number any more)
    const f3 pos = cam + t * ray;
    if (ACCEL) {
      const f3 v = grid_continuous(g, pos);
      const float bs = (float)g.bs;
      const f3 b = make_f3(floorf(v.x / bs), floorf(v.y / bs), floorf(v.z / bs));  // world_to_block_coords
      if (b.x != cur.x || b.y != cur.y || b.z != cur.z) {
        cur = b;
        allocated = false;
        if (b.x >= 0.0f && b.x < (float)g.nbx && b.y >= 0.0f && b.y < (float)g.nby && b.z >= 0.0f && b.z < (float)g.nbz)
          allocated = a.m.block_mask[((int)b.z * g.nby + (int)b.y) * g.nbx + (int)b.x] != 0;
        exit_t = ray_block_exit(g, cam, ray, b);
      }
      if (!allocated) {
        t = exit_t + step;
        prev_sdf = kSdfInvalid;
        continue;
      }
    }
    const float sdf = ray_sample(a.m, pos);
    if (sdf_is_invalid(sdf)) {
      t += step;
      continue;
    }
    if (prev_sdf < kSdfValidBelow && prev_sdf > 0.0f && sdf < 0.0f) {  // (false for a prev_sdf that is not a number)
      hit_t = ray_refine_hit(a.m, cam, ray, prev_t, t, prev_sdf, sdf);
      hit = true;
      break;
    }
    prev_sdf = sdf;
    prev_t = t;
    t += step;
  }
  f3 point = make_f3(0.0f, 0.0f, 0.0f), normal = point;
  float depth = 0.0f;
  if (hit) {
    point = cam + hit_t * ray;
    normal = ray_gradient(a.m, point);
    depth = a.z_depth ? hit_t * ray_cam.z : hit_t;  // the reference's "z_depth" is hit_t * 1.0: range along the ray (:564, :825)
  }
  a.hit_points[pixel * 3] = point.x, a.hit_points[pixel * 3 + 1] = point.y, a.hit_points[pixel * 3 + 2] = point.z;
  a.hit_normals[pixel * 3] = normal.x, a.hit_normals[pixel * 3 + 1] = normal.y, a.hit_normals[pixel * 3 + 2] = normal.z;
  a.hit_depths[pixel] = depth;
  a.hit_mask[pixel] = hit ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------- along-ray alignment
struct AlignArgs {
  const float *depth, *intrinsics, *position, *quaternion;
  RayMap m;
  float depth_min, depth_max, distance_threshold;
  int height, width, stride, out_w, n_total, n_samples;
  float *ws;
};

__global__ __launch_bounds__(kAlignThreads) void mapper_ray_align_kernel(AlignArgs a) {
  __shared__ float part[kAlignWaves][kPoseRow];
  const int tid = threadIdx.x, sample = blockIdx.x * kAlignThreads + tid;
  const MapGrid &g = a.m.g;
  // a pose that is not finite (the step kernel answers a failed factorisation with one) yields no valid sample
  const bool pose_ok = pose_is_finite(a.position, a.quaternion);
  float j[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, r = 0.0f;
  bool valid = false;
  if (sample < a.n_total && pose_ok) {
    const int pixel = sample / a.n_samples, k = sample - pixel * a.n_samples - a.n_samples / 2;
    const int pi = (pixel / a.out_w) * a.stride, pj = (pixel % a.out_w) * a.stride;
    if (pi < a.height && pj < a.width) {
      const float d = a.depth[(size_t)pi * a.width + pj];
      if (d >= a.depth_min && d <= a.depth_max && isfinite(d)) {
        const MapCamera camera = read_camera(a.intrinsics, a.position, a.quaternion, 0);
        const f3 d1 = pixel_ray<false>(camera, pj, pi);  // (no half pixel: :171-172)
        const float ray_len = sqrtf(d1.x * d1.x + d1.y * d1.y + 1.0f);
        const f3 ray = quat_rotate(camera.qw, camera.qv, make_f3(d1.x / ray_len, d1.y / ray_len, 1.0f / ray_len));
        const float obs_t = d * ray_len;
        const float sdf_k0 = ray_sample(a.m, camera.t + obs_t * ray);
        if (sdf_is_valid(sdf_k0) && fabsf(sdf_k0) <= a.distance_threshold) {
          const float sample_t = obs_t + (float)k * g.vs;
          if (sample_t >= 0.1f) {
            const f3 p = camera.t + sample_t * ray;
            const float sdf = ray_sample(a.m, p);
            const float expected = (float)(-k) * g.vs;
            if (sdf_is_valid(sdf) && fabsf(expected) <= g.trunc) {
              r = sdf - expected;
              const float abs_r = fabsf(r), huber_delta = 0.05f * (sample_t * sample_t);
              float hs = 1.0f;
              if (abs_r > huber_delta) hs = sqrtf(huber_delta / abs_r);
              r = r * hs;
              const f3 gr = ray_gradient(a.m, p);
              j[0] = gr.x * hs, j[1] = gr.y * hs, j[2] = gr.z * hs;  // :225-230
              j[3] = (gr.z * p.y - gr.y * p.z) * hs;
              j[4] = (gr.x * p.z - gr.z * p.x) * hs;
              j[5] = (gr.y * p.x - gr.x * p.y) * hs;
              valid = true;
            }
          }
        }
      }
    }
  }
  // ---- the workgroup's row, as pose_sdf_evaluate_kernel (pose_detect.hip) stores its own: the wavefronts' rows meet in LDS and
  // are added in wavefront order, the counts as integers
  const int wave = tid / kWave, lane = tid % kWave;
  const float word = pose_row_word(j, j, r, r * r, valid, lane);
  if (lane < kPoseRow) part[wave][lane] = word;
  __syncthreads();
  if (tid < kPoseRow) {
    float *row = a.ws + (size_t)blockIdx.x * kPoseRow;
    if (tid == kPoseCount) {
      int c = 0;
#pragma unroll
      for (int w = 0; w < kAlignWaves; w++) c += __float_as_int(part[w][tid]);
      row[tid] = __int_as_float(c);
    } else {  // (the words after the count are zeros, and stay zeros)
      float s = part[0][tid];
#pragma unroll
      for (int w = 1; w < kAlignWaves; w++) s += part[w][tid];
      row[tid] = s;
    }
  }
}

}  // namespace curobo_hip

using namespace curobo_hip;

// the map both launches read: the grid of `params` with minimum_tsdf_weight in place of the mapper's own
static int read_ray_map(RayMap *m, const void *block_data, const uint8_t *block_mask, const curobo_hip_mapper_params *params,
                        float minimum_tsdf_weight, const char *what) {
  if (int rc = read_params(params, &m->g, what)) return rc;
  if (int rc = check_map(block_data && block_mask, block_data, "block_data and block_mask", what)) return rc;
  CUROBO_REQUIRE(minimum_tsdf_weight >= 0.0f, "%s: minimum_tsdf_weight must not be negative, got %g", what, (double)minimum_tsdf_weight);
  m->block_data = (const uint32_t *)block_data, m->block_mask = block_mask;
  m->g.min_weight = minimum_tsdf_weight;
  return CUROBO_HIP_OK;
}

CUROBO_EXPORT int curobo_hip_mapper_raycast(float *hit_points, float *hit_normals, float *hit_depths, uint8_t *hit_mask, const float *intrinsics,
                                            const float *position, const float *quaternion, const void *block_data, const uint8_t *block_mask,
                                            const curobo_hip_mapper_params *params, float minimum_tsdf_weight, float depth_minimum_distance,
                                            float depth_maximum_distance, int height, int width, int accelerated, int z_depth,
                                            curobo_hip_stream_t stream) {
  const char *what = "mapper_raycast";
  RaycastArgs a{};
  if (int rc = read_ray_map(&a.m, block_data, block_mask, params, minimum_tsdf_weight, what)) return rc;
  CUROBO_REQUIRE(hit_points && hit_normals && hit_depths && hit_mask, "%s: hit_points, hit_normals, hit_depths and hit_mask must not be null",
                 what);
  CUROBO_REQUIRE(intrinsics && position && quaternion, "%s: intrinsics, position and quaternion must not be null", what);
  CUROBO_REQUIRE(height > 0 && width > 0 && (int64_t)height * width < ((int64_t)1 << 31) / 3,
                 "%s: the image must be H x W with 0 < 3 H W < 2^31, got %d x %d", what, height, width);
  CUROBO_REQUIRE(depth_minimum_distance >= 0.0f && depth_minimum_distance < depth_maximum_distance,
                 "%s: need 0 <= depth_minimum_distance < depth_maximum_distance, got %g and %g", what, (double)depth_minimum_distance,
                 (double)depth_maximum_distance);
  a.hit_points = hit_points, a.hit_normals = hit_normals, a.hit_depths = hit_depths, a.hit_mask = hit_mask;
  a.intrinsics = intrinsics, a.position = position, a.quaternion = quaternion;
  a.t_min = depth_minimum_distance, a.t_max = depth_maximum_distance, a.height = height, a.width = width, a.z_depth = z_depth != 0;
  // min(int((max - min) / step) + 1, 10000)  (:517-518), the comparison before the cast
  const float steps = (depth_maximum_distance - depth_minimum_distance) / (a.m.g.vs * 0.5f);
  a.max_steps = steps >= (float)(kRayMaxSteps - 1) ? kRayMaxSteps : (int)steps + 1;
  const dim3 grid((unsigned)ceil_div(width, kRayTile), (unsigned)ceil_div(height, kRayTile));
  if (accelerated != 0) hipLaunchKernelGGL(mapper_raycast_kernel<true>, grid, dim3(kRayThreads), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(mapper_raycast_kernel<false>, grid, dim3(kRayThreads), 0, (hipStream_t)stream, a);
  return check_launch(what, (hipStream_t)stream);
}

CUROBO_EXPORT int curobo_hip_mapper_ray_align(void *workspace, int64_t workspace_bytes, const float *depth, const float *intrinsics,
                                              const float *position, const float *quaternion, const void *block_data,
                                              const uint8_t *block_mask, const curobo_hip_mapper_params *params, float minimum_tsdf_weight,
                                              float depth_minimum_distance, float depth_maximum_distance, float distance_threshold, int height,
                                              int width, int stride, int n_samples_per_ray, curobo_hip_stream_t stream) {
  const char *what = "mapper_ray_align";
  AlignArgs a{};
  if (int rc = read_ray_map(&a.m, block_data, block_mask, params, minimum_tsdf_weight, what)) return rc;
  CUROBO_REQUIRE(workspace, "%s: workspace must not be null", what);
  CUROBO_REQUIRE(depth && intrinsics && position && quaternion, "%s: depth, intrinsics, position and quaternion must not be null", what);
  CUROBO_REQUIRE(height > 0 && width > 0, "%s: depth must be (H, W), got (%d, %d)", what, height, width);
  CUROBO_REQUIRE(stride >= 1, "%s: stride must be at least 1, got %d", what, stride);
  CUROBO_REQUIRE(n_samples_per_ray >= 1 && n_samples_per_ray <= 9 && (n_samples_per_ray & 1) == 1,
                 "%s: n_samples_per_ray must be odd and in 1..9, got %d", what, n_samples_per_ray);
  const int out_h = ceil_div(height, stride), out_w = ceil_div(width, stride);
  const int64_t n_total = (int64_t)out_h * out_w * n_samples_per_ray;
  CUROBO_REQUIRE((int64_t)height * width < ((int64_t)1 << 31) && n_total < ((int64_t)1 << 31) - kAlignThreads,
                 "%s: %lld samples are more than one launch holds", what, (long long)n_total);
  char counted[48];
  snprintf(counted, sizeof counted, "%lld samples", (long long)n_total);
  const int n_rows = ceil_div((int)n_total, kAlignThreads);
  if (int rc = check_pose_workspace(workspace, workspace_bytes, n_rows, what, counted, "curobo_hip_pose_sdf_ws_bytes")) return rc;
  a.depth = depth, a.intrinsics = intrinsics, a.position = position, a.quaternion = quaternion;
  a.depth_min = depth_minimum_distance, a.depth_max = depth_maximum_distance, a.distance_threshold = distance_threshold;
  a.height = height, a.width = width, a.stride = stride, a.out_w = out_w, a.n_total = (int)n_total, a.n_samples = n_samples_per_ray;
  a.ws = (float *)workspace;
  hipLaunchKernelGGL(mapper_ray_align_kernel, dim3((unsigned)n_rows), dim3(kAlignThreads), 0, (hipStream_t)stream, a);
  return check_launch(what, (hipStream_t)stream);
}
