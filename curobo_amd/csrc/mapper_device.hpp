// mapper_device.hpp -- the one statement of the mapper's grid for mapper.hip, mapper_raycast.hip and mapper_lidar.hip: how a world
// position, a voxel, a block, the stored fp16 pair, an ESDF cell, a packed site, a camera's pixel and a lidar's are addressed and read.  The lookups take the two
// arrays they read, block_data and block_mask, and nothing else of a launch's arguments.
#pragma once
#include "common.hpp"

namespace curobo_hip {

constexpr float kSdfInvalid = 1e10f, kSdfValidBelow = kSdfInvalid / 10.0f;  // SDF_INFINITY as the lookups return it; = 1e9f, builder_esdf.py:299
constexpr int kSiteBits = 10, kSiteMask = 0x3ff, kEsdfMaxAxis = 1 << kSiteBits;  // a site packs three coordinates of 10 bits: an axis has <= 1024 cells
struct MapGrid {
  int grid_w, grid_h, grid_d, bs, nbx, nby, nbz, num_samples;
  float ox, oy, oz, vs, trunc, depth_min, depth_max, min_weight, step;
};
struct EsdfArgs {
  const uint32_t *block_data;
  const uint8_t *block_mask;
  const float *origin, *voxel_size;
  int d, h, w;
};
#if defined(__HIPCC__)
struct i3 { int x, y, z; };
// continuous voxel coordinate of a world position (builder_coord.py:45-54): one axis (origin o, n voxels), and all three
__device__ __forceinline__ float grid_axis(const MapGrid &g, float p, float o, int n) { return (p - o) / g.vs + (float)n * 0.5f; }
__device__ __forceinline__ f3 grid_continuous(const MapGrid &g, f3 p) {
  return make_f3(grid_axis(g, p.x, g.ox, g.grid_w), grid_axis(g, p.y, g.oy, g.grid_h), grid_axis(g, p.z, g.oz, g.grid_d));
}
// centre of voxel gv of an axis (n voxels, origin o), where the TSDF was sampled: o + (gv + 0.5 - n / 2) voxel_size
// (builder_coord.py:57-66); T = double for the integrate kernel's depth along the camera axis
template <typename T> __device__ __forceinline__ T grid_centre_axis(const MapGrid &g, int gv, int n, float o) {
  return ((T)gv + (T)0.5 - (T)n * (T)0.5) * (T)g.vs + (T)o;
}
__device__ __forceinline__ f3 grid_centre(const MapGrid &g, int gx, int gy, int gz) {
  return make_f3(grid_centre_axis<float>(g, gx, g.grid_w, g.ox), grid_centre_axis<float>(g, gy, g.grid_h, g.oy), grid_centre_axis<float>(g, gz, g.grid_d, g.oz));
}
// lower (UPPER: upper) face of block b of an axis, b a whole number held as a float (ray_block_exit_t).  Not grid_centre_axis: a
// face has no half voxel and b stays a float, (b bs - n / 2) vs + o, so the centre's sum would be reassociated
template <bool UPPER> __device__ __forceinline__ float grid_face(const MapGrid &g, float b, int n, float o) {
  return ((UPPER ? b * (float)g.bs + (float)g.bs : b * (float)g.bs) - (float)n * 0.5f) * g.vs + o;
}
// centre of block b of an axis (n voxels, origin o): ((b bs + bs / 2) - n / 2) voxel_size + o, b a whole number (builder_decay.py:154-165)
__device__ __forceinline__ float grid_block_centre_axis(const MapGrid &g, int b, int n, float o) {
  return (((float)(b * g.bs) + (float)g.bs * 0.5f) - (float)n * 0.5f) * g.vs + o;
}
__device__ __forceinline__ f3 grid_block_centre(const MapGrid &g, int b) {
  return make_f3(grid_block_centre_axis(g, b % g.nbx, g.grid_w, g.ox), grid_block_centre_axis(g, (b / g.nbx) % g.nby, g.grid_h, g.oy),
                 grid_block_centre_axis(g, b / (g.nbx * g.nby), g.grid_d, g.oz));
}
__device__ __forceinline__ int grid_block_voxels(const MapGrid &g) { return g.bs * g.bs * g.bs; }
// block (bx, by, bz) is row (bz nby + by) nbx + bx; voxel (lx, ly, lz) of a block is its word (lz bs + ly) bs + lx (builder_coord.py:163-176)
__device__ __forceinline__ int grid_block(const MapGrid &g, int gx, int gy, int gz) { return ((gz / g.bs) * g.nby + gy / g.bs) * g.nbx + gx / g.bs; }
__device__ __forceinline__ int grid_local(const MapGrid &g, int gx, int gy, int gz) { return ((gz % g.bs) * g.bs + gy % g.bs) * g.bs + gx % g.bs; }
__device__ __forceinline__ i3 grid_voxel(const MapGrid &g, int b, int local) {
  return i3{(b % g.nbx) * g.bs + local % g.bs, ((b / g.nbx) % g.nby) * g.bs + (local / g.bs) % g.bs, (b / (g.nbx * g.nby)) * g.bs + local / (g.bs * g.bs)};
}
__device__ __forceinline__ float half_lo(uint32_t v) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(v & 0xffffu)); }
__device__ __forceinline__ float half_hi(uint32_t v) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(v >> 16)); }
__device__ __forceinline__ uint32_t pack_half2(float a, float b) {  // (the casts round to nearest even)
  return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)a) | ((uint32_t)__builtin_bit_cast(uint16_t, (_Float16)b) << 16);
}
__device__ __forceinline__ uint32_t tsdf_pair_add(uint32_t v, float sw, float w) { return pack_half2(half_lo(v) + sw, half_hi(v) + w); }
// both words times f: each product formed in fp32, then rounded to fp16, as torch's mul_ on an fp16 tensor (wp_decay.py:127, :141)
// The two products are made fp32 values of their own (the empty statement emits nothing): left to itself the compiler folds product
// and conversion into v_fma_mixlo_f16, a fused multiply-add with a +0 addend, which turns a -0 product into +0 and is not the
// fp32-then-fp16 rounding sequence of the host arithmetic this is compared with bit for bit
__device__ __forceinline__ uint32_t tsdf_pair_scale(uint32_t v, float f) {
  float sw = half_lo(v) * f, w = half_hi(v) * f;
  asm volatile("" : "+v"(sw), "+v"(w));
  return pack_half2(sw, w);
}
// a lookup's answer is invalid above kSdfValidBelow; a value that is not a number counts as valid, as the kernels have left it
__device__ __forceinline__ bool sdf_is_invalid(float s) { return s > kSdfValidBelow; }
__device__ __forceinline__ bool sdf_is_valid(float s) { return !(s > kSdfValidBelow); }
// the pair's sdf, kSdfInvalid below the minimum weight (the reference compares both ways: the two lookups); then a voxel that exists, read so
template <bool AT_MINIMUM_TOO> __device__ __forceinline__ float tsdf_pair_sdf(uint32_t v, float min_weight) {
  const float w = half_hi(v);
  return (AT_MINIMUM_TOO ? w >= min_weight : w > min_weight) ? half_lo(v) / w : kSdfInvalid;
}
template <bool AT_MINIMUM_TOO>
__device__ __forceinline__ float tsdf_read(const uint32_t *block_data, const uint8_t *block_mask, const MapGrid &g, int gx, int gy, int gz) {
  const int b = grid_block(g, gx, gy, gz);
  if (block_mask[b] == 0) return kSdfInvalid;
  const int local = grid_local(g, gx, gy, gz);
  return tsdf_pair_sdf<AT_MINIMUM_TOO>(block_data[(size_t)b * grid_block_voxels(g) + local], g.min_weight);
}
// THE PROBE RULE, of the ESDF path (builder_esdf.py:279-291, wp_tsdf_sample.py:46-52): the voxel of a world position by a cast
// toward zero (a coordinate in (-1, 0) is voxel 0), which must lie in the grid proper, observed when its weight is ABOVE the minimum
__device__ __forceinline__ float tsdf_probe(const uint32_t *block_data, const uint8_t *block_mask, const MapGrid &g, f3 p) {
  const int gx = (int)grid_axis(g, p.x, g.ox, g.grid_w), gy = (int)grid_axis(g, p.y, g.oy, g.grid_h), gz = (int)grid_axis(g, p.z, g.oz, g.grid_d);
  if (gx < 0 || gx >= g.grid_w || gy < 0 || gy >= g.grid_h || gz < 0 || gz >= g.grid_d) return kSdfInvalid;
  return tsdf_read<false>(block_data, block_mask, g, gx, gy, gz);
}
// THE SAMPLE RULE, of the mesh, the renderer and the refiner (builder_raycast.py:63-90, the comparison :78): voxel (gx, gy, gz) of
// the PADDED grid (the samplers below reach it by floor), observed when its weight is AT LEAST the minimum
__device__ __forceinline__ float tsdf_voxel(const uint32_t *block_data, const uint8_t *block_mask, const MapGrid &g, int gx, int gy, int gz) {
  if (gx < 0 || gx >= g.nbx * g.bs || gy < 0 || gy >= g.nby * g.bs || gz < 0 || gz >= g.nbz * g.bs) return kSdfInvalid;
  return tsdf_read<true>(block_data, block_mask, g, gx, gy, gz);
}
__device__ __forceinline__ bool is_seed(float sdf, const MapGrid &g) {
  if (sdf_is_invalid(sdf)) return false;
  return fabsf(sdf) <= g.vs * 0.9f || sdf < -(g.trunc - g.vs * 1.1f);
}
// nearest-voxel sample: voxel floor(v)  (builder_raycast.py:92-109)
__device__ __forceinline__ float tsdf_nearest(const uint32_t *block_data, const uint8_t *block_mask, const MapGrid &g, f3 p) {
  const f3 v = grid_continuous(g, p);
  return tsdf_voxel(block_data, block_mask, g, (int)floorf(v.x), (int)floorf(v.y), (int)floorf(v.z));
}
// trilinear sample, lower corner floor(v - 0.5); an invalid corner contributes the truncation distance, no valid corner at
// all makes the sample invalid  (builder_raycast.py:168-258)
__device__ __forceinline__ float tsdf_trilinear(const uint32_t *block_data, const uint8_t *block_mask, const MapGrid &g, f3 p) {
  const f3 v = grid_continuous(g, p);
  const float fx = v.x - 0.5f, fy = v.y - 0.5f, fz = v.z - 0.5f;
  const float x0 = floorf(fx), y0 = floorf(fy), z0 = floorf(fz);
  const float tx = fx - x0, ty = fy - y0, tz = fz - z0;
  const int ix = (int)x0, iy = (int)y0, iz = (int)z0;
  float total = 0.0f;
  bool any_valid = false;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
    const float s = tsdf_voxel(block_data, block_mask, g, ix + dx, iy + dy, iz + dz);
    const bool ok = sdf_is_valid(s);
    any_valid |= ok;
    total += (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty) * (dz ? tz : 1.0f - tz) * (ok ? s : g.trunc);
  }
  return any_valid ? total : kSdfInvalid;
}
// normalised central difference of six samples at +-voxel_size; (0, 0, 1) where one of them is invalid or the magnitude is
// below 1e-6  (builder_raycast.py:277-325 with trilinear samples, :327-375 with nearest-voxel samples)
template <bool TRILINEAR>
__device__ __forceinline__ f3 tsdf_gradient(const uint32_t *block_data, const uint8_t *block_mask, const MapGrid &g, f3 p) {
  float s[6];
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const float e = (k & 1) ? -g.vs : g.vs;
    const f3 q = make_f3(p.x + (k / 2 == 0 ? e : 0.0f), p.y + (k / 2 == 1 ? e : 0.0f), p.z + (k / 2 == 2 ? e : 0.0f));
    s[k] = TRILINEAR ? tsdf_trilinear(block_data, block_mask, g, q) : tsdf_nearest(block_data, block_mask, g, q);
  }
  const f3 up = make_f3(0.0f, 0.0f, 1.0f);
  if (sdf_is_invalid(s[0]) || sdf_is_invalid(s[1]) || sdf_is_invalid(s[2]) || sdf_is_invalid(s[3]) || sdf_is_invalid(s[4]) || sdf_is_invalid(s[5])) return up;
  const f3 grad = make_f3((s[0] - s[1]) / (2.0f * g.vs), (s[2] - s[3]) / (2.0f * g.vs), (s[4] - s[5]) / (2.0f * g.vs));
  const float mag = sqrtf(grad.x * grad.x + grad.y * grad.y + grad.z * grad.z);
  if (mag < 1e-6f) return up;
  return make_f3(grad.x / mag, grad.y / mag, grad.z / mag);
}
// centre of cell (x, y, z) of the ESDF grid, x the slowest axis, of d cells (builder_esdf.py:334-336)
__device__ __forceinline__ f3 esdf_centre(const EsdfArgs &a, int x, int y, int z) {
  const float vs = a.voxel_size[0];
  return make_f3(a.origin[0] + ((float)x + 0.5f - (float)a.d * 0.5f) * vs, a.origin[1] + ((float)y + 0.5f - (float)a.h * 0.5f) * vs,
                 a.origin[2] + ((float)z + 0.5f - (float)a.w * 0.5f) * vs);
}
__device__ __forceinline__ int32_t site_pack(int x, int y, int z) { return x | (y << kSiteBits) | (z << (2 * kSiteBits)); }
// coordinate c of a cell minus that coordinate (axis 0, 1, 2) of the cell that site s names
__device__ __forceinline__ int site_offset(int32_t s, int axis, int c) { return c - ((s >> (axis * kSiteBits)) & kSiteMask); }
// wp.quat_rotate for q = (w, v): x (2 w^2 - 1) + 2 w (v x x) + 2 v (v . x)
__device__ __forceinline__ f3 quat_rotate(float w, f3 v, f3 x) {
  return (2.0f * w * w - 1.0f) * x + (2.0f * w) * cross(v, x) + (2.0f * dot(v, x)) * v;
}
// camera `cam` of the arrays intrinsics [n, 3, 3], position [n, 3], quaternion [n, 4] wxyz: its pose in the world is t, (qw, qv)
struct MapCamera { float fx, fy, cx, cy; f3 t; float qw; f3 qv; };
__device__ __forceinline__ MapCamera read_camera(const float *intrinsics, const float *position, const float *quaternion, int cam) {
  const float *K = intrinsics + cam * 9, *q = quaternion + cam * 4, *t = position + cam * 3;
  return MapCamera{K[0], K[4], K[2], K[5], make_f3(t[0], t[1], t[2]), q[0], make_f3(q[1], q[2], q[3])};
}
// the ray of pixel (px, py) in the camera frame, z = 1, NOT normalised (marking scales it by z, the ray launches normalise it).
// HALF_PIXEL: through the pixel's centre (builder_camera_integrate.py:125-127, the renders); not so wp_raycast_pose_refine.py:171-172
template <bool HALF_PIXEL> __device__ __forceinline__ f3 pixel_ray(const MapCamera &c, int px, int py) {
  return make_f3(((HALF_PIXEL ? (float)px + 0.5f : (float)px) - c.cx) / c.fx, ((HALF_PIXEL ? (float)py + 0.5f : (float)py) - c.cy) / c.fy, 1.0f);
}
// lidar `i` of the arrays position [n, 3], quaternion [n, 4] wxyz, valid_range [n, 2] metres, elevation_range [n, 2] radians: its pose
// in the world is t, (qw, qv); a range image of H x W pixels covers the full azimuth and the elevation band
struct MapLidar { f3 t; float qw; f3 qv; float min_range, max_range, min_elev, max_elev; };
__device__ __forceinline__ MapLidar read_lidar(const float *position, const float *quaternion, const float *valid_range,
                                               const float *elevation_range, int i) {
  const float *q = quaternion + i * 4, *t = position + i * 3, *r = valid_range + i * 2, *e = elevation_range + i * 2;
  return MapLidar{make_f3(t[0], t[1], t[2]), q[0], make_f3(q[1], q[2], q[3]), r[0], r[1], e[0], e[1]};
}
// pi and 2 pi as the reference's kernels hold them, fp32 constants (builder_lidar_integrate.py:52-53); the double forms of the rules
// below widen THESE, so that a float64 restatement with the same two numbers says what the launch computes
constexpr float kLidarPi = 3.141592653589793f, kLidarTwoPi = 6.283185307179586f;
// _range_valid (builder_lidar_integrate.py:106-112), of a pixel's range or a voxel's; false for a value that is not a number
template <typename T> __device__ __forceinline__ bool lidar_range_valid(T value, const MapLidar &l) {
  return value >= (T)l.min_range && value <= (T)l.max_range;
}
// the unit ray of pixel (px, py) in the sensor frame (:75-94): azimuth px 2 pi / W - pi, NO half pixel; elevation from max_elev in
// row 0 down to min_elev in row H - 1, min_elev where H == 1
__device__ __forceinline__ f3 lidar_pixel_ray(const MapLidar &l, int px, int py, int height, int width) {
  const float azimuth = (float)px * kLidarTwoPi / (float)width - kLidarPi;
  const float elevation = height > 1 ? l.max_elev - (float)py * (l.max_elev - l.min_elev) / (float)(height - 1) : l.min_elev;
  const float ce = cosf(elevation);
  return make_f3(cosf(azimuth) * ce, sinf(azimuth) * ce, sinf(elevation));
}
// voxel -> (u, v), the inverse of the above (:421-437), from the voxel's position (x, y, z) in the sensor frame.  false where the
// elevation is outside the band (H > 1 only; the planar sensor takes every elevation and v = 0); u is wrapped into [0, W)
template <typename T> __device__ __forceinline__ bool lidar_voxel_uv(const MapLidar &l, T x, T y, T z, int height, int width, T *u, T *v) {
  *v = (T)0;
  if (height > 1) {
    const T elevation = atan2(z, sqrt(x * x + y * y));
    if (elevation < (T)l.min_elev || elevation > (T)l.max_elev) return false;
    *v = ((T)l.max_elev - elevation) * ((T)(height - 1) / ((T)l.max_elev - (T)l.min_elev));
  }
  T uf = (atan2(y, x) + (T)kLidarPi) * ((T)width / (T)kLidarTwoPi);
  if (uf >= (T)width) uf -= (T)width;
  if (uf < (T)0) uf += (T)width;
  *u = uf;
  return true;
}
#endif  // __HIPCC__
static int read_params(const curobo_hip_mapper_params *p, MapGrid *g, const char *what) {
  CUROBO_REQUIRE(p, "%s: params must not be null", what);
  CUROBO_REQUIRE(p->grid_w > 0 && p->grid_h > 0 && p->grid_d > 0, "%s: the grid must have voxels along every axis, got %d x %d x %d", what,
                 p->grid_w, p->grid_h, p->grid_d);
  const int bs = p->block_size;
  CUROBO_REQUIRE(bs >= 1 && bs <= 32 && (bs & (bs - 1)) == 0, "%s: block_size must be 1 or a power of two in 2..32, got %d", what, bs);
  CUROBO_REQUIRE(p->nbx == ceil_div(p->grid_w, bs) && p->nby == ceil_div(p->grid_h, bs) && p->nbz == ceil_div(p->grid_d, bs),
                 "%s: nbx, nby, nbz must be ceil(grid / block_size) = %d, %d, %d, got %d, %d, %d", what, ceil_div(p->grid_w, bs),
                 ceil_div(p->grid_h, bs), ceil_div(p->grid_d, bs), p->nbx, p->nby, p->nbz);
  const int64_t voxels = (int64_t)p->nbx * p->nby * p->nbz * bs * bs * bs;
  CUROBO_REQUIRE(voxels < ((int64_t)1 << 31), "%s: the padded grid holds %lld voxels, the kernels index below 2^31", what, (long long)voxels);
  CUROBO_REQUIRE(p->voxel_size > 0.0f && p->truncation_distance > 0.0f, "%s: voxel_size and truncation_distance must be positive", what);
  CUROBO_REQUIRE(p->depth_min < p->depth_max, "%s: depth_min must be below depth_max", what);
  g->grid_w = p->grid_w, g->grid_h = p->grid_h, g->grid_d = p->grid_d, g->bs = bs, g->nbx = p->nbx, g->nby = p->nby, g->nbz = p->nbz;
  g->num_samples = p->num_samples, g->ox = p->origin[0], g->oy = p->origin[1], g->oz = p->origin[2], g->vs = p->voxel_size;
  g->trunc = p->truncation_distance, g->depth_min = p->depth_min, g->depth_max = p->depth_max, g->min_weight = p->minimum_tsdf_weight;
  g->step = p->step_size;
  return CUROBO_HIP_OK;
}
static int check_map(bool pointers_non_null, const void *block_data, const char *pointer_names, const char *what) {
  CUROBO_REQUIRE(pointers_non_null, "%s: %s must not be null", what, pointer_names);
  CUROBO_REQUIRE(((uintptr_t)block_data & 3) == 0, "%s: block_data must be 4-byte aligned", what);
  return CUROBO_HIP_OK;
}

}  // namespace curobo_hip
