// mapper_lidar.hip -- lidar range images into the mapper's dense TSDF (curobo_amd/perception/mapper/mapper.py), the two stages of
// mapper.hip with a spherical sensor model:
//   curobo_hip_mapper_lidar_mark_blocks   one lane per (sensor, pixel, sample along the ray): the blocks this frame's lidars see
//   curobo_hip_mapper_lidar_integrate     one workgroup per block, at once back where the lidars do not see it: the running sum
//                                         of the signed distance ALONG THE RAY (surface range - voxel range), weight 1
//
// Reference: perception/mapper/kernel/builder/builder_lidar_integrate.py (_lidar_pixel_ray :75-94, _range_valid :106-112,
// lidar_compute_block_keys_only_kernel :114-180, _nearest_lidar_range :244-279, _interpolate_lidar_range :281-367,
// lidar_integrate_voxels_kernel :369-467).  The support-pixel lists (:182-242) and the launches that read them gather colour and
// features, which this map does not store.  As in mapper.hip nothing is allocated, hashed or counted with atomics: every store
// of a launch goes to a word no other lane of that launch writes, except the mask bytes, which every writer sets to 1.
//
// Where the arithmetic is done.  Marking is fp32 throughout, as the camera's: a sample decides a block, and a sample near a block
// face may fall either way.  Integration stores sdf = surface range - voxel range, which cancels to nothing at the surface, where
// the fp16 word has steps of 6e-8 .. 5e-7 m; and here the surface range is interpolated at (u, v), which come from two atan2 of
// the voxel's position in the sensor frame, so an fp32 error in that position reaches the sdf twice: through the voxel range
// (a few 1e-7 m at 2 m) and through u, v times the range image's slope (up to the linear guard per pixel).  So the position in
// the sensor frame, its range, both angles, (u, v), the bilinear sum and the difference are double, from fp32 poses, bounds and
// pixel reads widened exactly; pi and 2 pi are the reference's fp32 constants widened (mapper_device.hpp).  What only DECIDES with a
// tolerance stays fp32: the nearest pixel's ray and the voxel's distance to it, against a guard of a fraction of a voxel.
// The result is rounded once to fp32; the comparison with -truncation, the clamp and the sums over the sensors are fp32.
#include "mapper_device.hpp"

namespace curobo_hip {

constexpr int kLidarThreads = 256;

struct MapLidars {
  const float *range, *position, *quaternion, *valid_range, *elevation_range;
  int n, height, width;
  float linear_max_diff, nearest_max_dist;  // metres
};

// ---------------------------------------------------------------------------------------------------- stage 1: visible blocks
__global__ __launch_bounds__(kLidarThreads) void mapper_lidar_mark_kernel(uint8_t *lidar_mask, uint8_t *frame_mask, uint8_t *block_mask,
                                                                          MapLidars c, MapGrid g) {
  const int64_t tid = (int64_t)blockIdx.x * kLidarThreads + threadIdx.x;
  const int n_pixels = c.height * c.width;
  const int64_t per_lidar = (int64_t)n_pixels * g.num_samples;
  if (tid >= per_lidar * c.n) return;
  const int lidar = (int)(tid / per_lidar);
  const int rem = (int)(tid - (int64_t)lidar * per_lidar);
  const int pixel = rem / g.num_samples, k = rem - pixel * g.num_samples;
  const int px = pixel % c.width, py = pixel / c.width;
  const MapLidar l = read_lidar(c.position, c.quaternion, c.valid_range, c.elevation_range, lidar);
  const float range = c.range[(size_t)lidar * n_pixels + pixel];
  if (!lidar_range_valid(range, l)) return;
  const float r = fmaxf(range - g.trunc, l.min_range) + (float)k * g.step;
  if (r > range + g.trunc + g.step) return;
  const f3 p = l.t + quat_rotate(l.qw, l.qv, r * lidar_pixel_ray(l, px, py, c.height, c.width));
  const int vx = (int)floorf(grid_axis(g, p.x, g.ox, g.grid_w)), vy = (int)floorf(grid_axis(g, p.y, g.oy, g.grid_h));
  const int vz = (int)floorf(grid_axis(g, p.z, g.oz, g.grid_d));
  if (vx < 0 || vx >= g.grid_w || vy < 0 || vy >= g.grid_h || vz < 0 || vz >= g.grid_d) return;
  const int b = grid_block(g, vx, vy, vz);  // < nbx nby nbz: the voxel is inside the grid
  lidar_mask[b] = 1;
  frame_mask[b] = 1;
  block_mask[b] = 1;
}

// ---------------------------------------------------------------------------------------------------- stage 2: voxels
// _nearest_lidar_range (:244-279): the pixel nearest (u, v), its range valid, the voxel (fp32, sensor frame) within the guard of its ray
__device__ __forceinline__ bool lidar_nearest_range(const MapLidars &c, const MapLidar &l, int lidar, double u, double v, f3 voxel,
                                                    double *surface) {
  int u_near = (int)floor(u + 0.5);
  if (u_near >= c.width) u_near -= c.width;
  if (u_near < 0) u_near += c.width;
  if (u_near < 0 || u_near >= c.width) return false;  // (u is not a number: a pose that is not finite)
  int v_near = 0;
  if (c.height > 1) {
    v_near = (int)floor(v + 0.5);
    if (v_near < 0 || v_near >= c.height) return false;
  }
  const float range = c.range[((size_t)lidar * c.height + v_near) * c.width + u_near];
  if (!lidar_range_valid(range, l)) return false;
  const f3 ray = lidar_pixel_ray(l, u_near, v_near, c.height, c.width);
  const f3 off = voxel - dot(voxel, ray) * ray;
  if (sqrtf(dot(off, off)) > c.nearest_max_dist) return false;
  *surface = (double)range;
  return true;
}

// _interpolate_lidar_range (:281-367): bilinear over the four pixels about (u, v), the columns wrapping at the seam, when all four
// are valid and none differs from the result by more than the guard; else the nearest pixel
__device__ __forceinline__ bool lidar_surface_range(const MapLidars &c, const MapLidar &l, int lidar, double u, double v, f3 voxel,
                                                    double *surface) {
  const int v0 = (int)floor(v);
  int u0 = (int)floor(u);
  if (u0 < 0) u0 += c.width;
  if (u0 >= c.width) u0 -= c.width;
  if (c.height > 1 && v0 >= 0 && v0 < c.height - 1 && u0 >= 0 && u0 < c.width) {  // (u0 outside: u is not a number)
    const int u1 = u0 + 1 >= c.width ? 0 : u0 + 1;
    const float *row0 = c.range + ((size_t)lidar * c.height + v0) * c.width, *row1 = row0 + c.width;
    const float d00 = row0[u0], d01 = row0[u1], d10 = row1[u0], d11 = row1[u1];
    if (lidar_range_valid(d00, l) && lidar_range_valid(d01, l) && lidar_range_valid(d10, l) && lidar_range_valid(d11, l)) {
      const double fu = u - floor(u), fv = v - floor(v);
      const double top = (double)d00 * (1.0 - fu) + (double)d01 * fu, bottom = (double)d10 * (1.0 - fu) + (double)d11 * fu;
      const double interp = top * (1.0 - fv) + bottom * fv;
      const double max_diff = fmax(fmax(fabs((double)d00 - interp), fabs((double)d01 - interp)),
                                   fmax(fabs((double)d10 - interp), fabs((double)d11 - interp)));
      if (max_diff <= (double)c.linear_max_diff) {
        *surface = interp;
        return true;
      }
    }
  }
  return lidar_nearest_range(c, l, lidar, u, v, voxel, surface);
}

__global__ __launch_bounds__(kLidarThreads) void mapper_lidar_integrate_kernel(uint32_t *block_data, const uint8_t *lidar_mask, MapLidars c,
                                                                               MapGrid g) {
  const int b = blockIdx.x;
  if (lidar_mask[b] == 0) return;  // (uniform over the workgroup)
  const int bs3 = grid_block_voxels(g);
  for (int local = threadIdx.x; local < bs3; local += blockDim.x) {
    const i3 voxel = grid_voxel(g, b, local);
    const double cx = grid_centre_axis<double>(g, voxel.x, g.grid_w, g.ox), cy = grid_centre_axis<double>(g, voxel.y, g.grid_h, g.oy);
    const double cz = grid_centre_axis<double>(g, voxel.z, g.grid_d, g.oz);
    float total_sw = 0.0f, total_w = 0.0f;
    for (int lidar = 0; lidar < c.n; lidar++) {
      const MapLidar l = read_lidar(c.position, c.quaternion, c.valid_range, c.elevation_range, lidar);
      // quat_rotate by the conjugate (quat_inverse), in double: x (2 w^2 - 1) + 2 w (v x x) + 2 v (v . x)
      const double qw = l.qw, qx = -(double)l.qv.x, qy = -(double)l.qv.y, qz = -(double)l.qv.z;
      const double ex = cx - (double)l.t.x, ey = cy - (double)l.t.y, ez = cz - (double)l.t.z;
      const double s = 2.0 * qw * qw - 1.0, d2 = 2.0 * (qx * ex + qy * ey + qz * ez), w2 = 2.0 * qw;
      const double x = ex * s + w2 * (qy * ez - qz * ey) + d2 * qx, y = ey * s + w2 * (qz * ex - qx * ez) + d2 * qy;
      const double z = ez * s + w2 * (qx * ey - qy * ex) + d2 * qz;
      const double voxel_range = sqrt(x * x + y * y + z * z);
      if (!lidar_range_valid(voxel_range, l)) continue;
      double u, v, surface;
      if (!lidar_voxel_uv<double>(l, x, y, z, c.height, c.width, &u, &v)) continue;
      if (!lidar_surface_range(c, l, lidar, u, v, make_f3((float)x, (float)y, (float)z), &surface)) continue;
      const float sdf = (float)(surface - voxel_range);
      if (!(sdf >= -g.trunc)) continue;
      total_sw += fminf(sdf, g.trunc);  // times the weight: compute_tsdf_weight is 1
      total_w += 1.0f;
    }
    if (total_w > 0.0f) {
      uint32_t *word = block_data + (size_t)b * bs3 + local;
      *word = tsdf_pair_add(*word, total_sw, total_w);
    }
  }
}

}  // namespace curobo_hip

using namespace curobo_hip;

// ---------------------------------------------------------------------------------------------------- host side
static int read_lidars(MapLidars *c, const float *range, const float *position, const float *quaternion, const float *valid_range,
                       const float *elevation_range, int n_lidars, int height, int width, const char *what) {
  CUROBO_REQUIRE(range && position && quaternion && valid_range && elevation_range,
                 "%s: range, lidar_position, lidar_quaternion, valid_range and elevation_range must not be null", what);
  CUROBO_REQUIRE(n_lidars > 0 && height > 0 && width > 0, "%s: range must be (n_lidars, H, W), got (%d, %d, %d)", what, n_lidars, height, width);
  CUROBO_REQUIRE((int64_t)n_lidars * height * width < ((int64_t)1 << 31), "%s: the range images hold 2^31 pixels or more", what);
  c->range = range, c->position = position, c->quaternion = quaternion, c->valid_range = valid_range, c->elevation_range = elevation_range;
  c->n = n_lidars, c->height = height, c->width = width, c->linear_max_diff = 0.0f, c->nearest_max_dist = 0.0f;
  return CUROBO_HIP_OK;
}

CUROBO_EXPORT int curobo_hip_mapper_lidar_mark_blocks(uint8_t *lidar_mask, uint8_t *frame_mask, uint8_t *block_mask, const float *range,
                                                      const float *lidar_position, const float *lidar_quaternion, const float *valid_range,
                                                      const float *elevation_range, const curobo_hip_mapper_params *params, int n_lidars,
                                                      int height, int width, curobo_hip_stream_t stream) {
  const char *what = "mapper_lidar_mark_blocks";
  MapGrid g;
  MapLidars c;
  if (int rc = read_params(params, &g, what)) return rc;
  if (int rc = read_lidars(&c, range, lidar_position, lidar_quaternion, valid_range, elevation_range, n_lidars, height, width, what)) return rc;
  CUROBO_REQUIRE(lidar_mask && frame_mask && block_mask, "%s: lidar_mask, frame_mask and block_mask must not be null", what);
  CUROBO_REQUIRE(g.num_samples > 0 && g.step > 0.0f, "%s: num_samples and step_size must be positive, got %d and %g", what, g.num_samples,
                 (double)g.step);
  const int64_t lanes = (int64_t)n_lidars * height * width * g.num_samples;
  CUROBO_REQUIRE(lanes < ((int64_t)1 << 31) * kLidarThreads, "%s: %lld samples are more than one launch holds", what, (long long)lanes);
  hipLaunchKernelGGL(mapper_lidar_mark_kernel, dim3((unsigned)ceil_div_l(lanes, kLidarThreads)), dim3(kLidarThreads), 0, (hipStream_t)stream,
                     lidar_mask, frame_mask, block_mask, c, g);
  return check_launch(what, (hipStream_t)stream);
}

CUROBO_EXPORT int curobo_hip_mapper_lidar_integrate(void *block_data, const uint8_t *lidar_mask, const float *range, const float *lidar_position,
                                                    const float *lidar_quaternion, const float *valid_range, const float *elevation_range,
                                                    const curobo_hip_mapper_params *params, int n_lidars, int height, int width,
                                                    float linear_max_diff_m, float nearest_max_dist_m, curobo_hip_stream_t stream) {
  const char *what = "mapper_lidar_integrate";
  MapGrid g;
  MapLidars c;
  if (int rc = read_params(params, &g, what)) return rc;
  if (int rc = read_lidars(&c, range, lidar_position, lidar_quaternion, valid_range, elevation_range, n_lidars, height, width, what)) return rc;
  if (int rc = check_map(block_data && lidar_mask, block_data, "block_data and lidar_mask", what)) return rc;
  CUROBO_REQUIRE(linear_max_diff_m > 0.0f && nearest_max_dist_m > 0.0f,
                 "%s: linear_max_diff_m and nearest_max_dist_m must be positive, got %g and %g", what, (double)linear_max_diff_m,
                 (double)nearest_max_dist_m);
  c.linear_max_diff = linear_max_diff_m, c.nearest_max_dist = nearest_max_dist_m;
  const int bs3 = g.bs * g.bs * g.bs;
  const int64_t n_blocks = (int64_t)g.nbx * g.nby * g.nbz;
  hipLaunchKernelGGL(mapper_lidar_integrate_kernel, dim3((unsigned)n_blocks), dim3(bs3 >= kLidarThreads ? kLidarThreads : kWave), 0,
                     (hipStream_t)stream, (uint32_t *)block_data, lidar_mask, c, g);
  return check_launch(what, (hipStream_t)stream);
}
