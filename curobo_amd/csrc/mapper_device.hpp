// mapper_device.hpp -- what the mapper's units share (mapper.hip: integration, ESDF, mesh extraction; mapper_raycast.hip:
// rendering and the along-ray alignment): the grid as the launches see it, the fp16 pair's halves, wp.quat_rotate, and the
// reads of the TSDF -- one voxel, the nearest voxel, the trilinear sample and the gradients of builder_raycast.py
// (sample_voxel :63-90, sample_tsdf_trilinear :168-258, compute_gradient :277-375).  The samplers take the two arrays they
// read, block_data and block_mask, and nothing else of a launch's arguments.
#pragma once
#include "common.hpp"

namespace curobo_hip {

constexpr float kSdfInvalid = 1e10f;      // wp_tsdf_sample.py SDF_INFINITY as the lookups return it

struct MapGrid {
  int grid_w, grid_h, grid_d, bs, nbx, nby, nbz, num_samples;
  float ox, oy, oz, vs, trunc, depth_min, depth_max, min_weight, step;
};

#if defined(__HIPCC__)

// wp.quat_rotate for q = (w, v): x (2 w^2 - 1) + 2 w (v x x) + 2 v (v . x)
__device__ __forceinline__ f3 quat_rotate(float w, f3 v, f3 x) {
  return (2.0f * w * w - 1.0f) * x + (2.0f * w) * cross(v, x) + (2.0f * dot(v, x)) * v;
}

__device__ __forceinline__ float half_lo(uint32_t v) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(v & 0xffffu)); }
__device__ __forceinline__ float half_hi(uint32_t v) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(v >> 16)); }

// the stored sdf of voxel (gx, gy, gz) of the PADDED grid, kSdfInvalid where there is no such voxel, its block was never
// visible or its weight is below the minimum (>=: builder_raycast.py:78, the lookups of the mesh and the renderer)
__device__ __forceinline__ float mesh_voxel(const uint32_t *block_data, const uint8_t *block_mask, const MapGrid &g, int gx, int gy, int gz) {
  if (gx < 0 || gx >= g.nbx * g.bs || gy < 0 || gy >= g.nby * g.bs || gz < 0 || gz >= g.nbz * g.bs) return kSdfInvalid;
  const int b = ((gz / g.bs) * g.nby + gy / g.bs) * g.nbx + gx / g.bs;
  if (block_mask[b] == 0) return kSdfInvalid;
  const int local = ((gz % g.bs) * g.bs + gy % g.bs) * g.bs + gx % g.bs;
  const uint32_t v = block_data[(size_t)b * (g.bs * g.bs * g.bs) + local];
  const float w = half_hi(v);
  return w >= g.min_weight ? half_lo(v) / w : kSdfInvalid;
}

// continuous voxel coordinate of a world position (builder_coord.py:45-54)
__device__ __forceinline__ f3 mesh_continuous(const MapGrid &g, f3 p) {
  return make_f3((p.x - g.ox) / g.vs + (float)g.grid_w * 0.5f, (p.y - g.oy) / g.vs + (float)g.grid_h * 0.5f,
                 (p.z - g.oz) / g.vs + (float)g.grid_d * 0.5f);
}

// nearest-voxel sample: voxel floor(v)  (builder_raycast.py:92-109)
__device__ __forceinline__ float mesh_nearest(const uint32_t *block_data, const uint8_t *block_mask, const MapGrid &g, f3 p) {
  const f3 v = mesh_continuous(g, p);
  return mesh_voxel(block_data, block_mask, g, (int)floorf(v.x), (int)floorf(v.y), (int)floorf(v.z));
}

// trilinear sample, lower corner floor(v - 0.5); an invalid corner contributes the truncation distance, no valid corner at
// all makes the sample invalid  (builder_raycast.py:168-258)
__device__ __forceinline__ float mesh_trilinear(const uint32_t *block_data, const uint8_t *block_mask, const MapGrid &g, f3 p) {
  const f3 v = mesh_continuous(g, p);
  const float fx = v.x - 0.5f, fy = v.y - 0.5f, fz = v.z - 0.5f;
  const float x0 = floorf(fx), y0 = floorf(fy), z0 = floorf(fz);
  const float tx = fx - x0, ty = fy - y0, tz = fz - z0;
  const int ix = (int)x0, iy = (int)y0, iz = (int)z0;
  float total = 0.0f;
  bool any_valid = false;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
    const float s = mesh_voxel(block_data, block_mask, g, ix + dx, iy + dy, iz + dz);
    const bool ok = !(s > 1e9f);
    any_valid |= ok;
    total += (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty) * (dz ? tz : 1.0f - tz) * (ok ? s : g.trunc);
  }
  return any_valid ? total : kSdfInvalid;
}

// normalised central difference of six samples at +-voxel_size; (0, 0, 1) where one of them is invalid or the magnitude is
// below 1e-6  (builder_raycast.py:277-325 with trilinear samples, :327-375 with nearest-voxel samples)
template <bool TRILINEAR>
__device__ __forceinline__ f3 mesh_gradient(const uint32_t *block_data, const uint8_t *block_mask, const MapGrid &g, f3 p) {
  float s[6];
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const float e = (k & 1) ? -g.vs : g.vs;
    const f3 q = make_f3(p.x + (k / 2 == 0 ? e : 0.0f), p.y + (k / 2 == 1 ? e : 0.0f), p.z + (k / 2 == 2 ? e : 0.0f));
    s[k] = TRILINEAR ? mesh_trilinear(block_data, block_mask, g, q) : mesh_nearest(block_data, block_mask, g, q);
  }
  const f3 up = make_f3(0.0f, 0.0f, 1.0f);
  if (s[0] > 1e9f || s[1] > 1e9f || s[2] > 1e9f || s[3] > 1e9f || s[4] > 1e9f || s[5] > 1e9f) return up;
  const f3 grad = make_f3((s[0] - s[1]) / (2.0f * g.vs), (s[2] - s[3]) / (2.0f * g.vs), (s[4] - s[5]) / (2.0f * g.vs));
  const float mag = sqrtf(grad.x * grad.x + grad.y * grad.y + grad.z * grad.z);
  if (mag < 1e-6f) return up;
  return make_f3(grad.x / mag, grad.y / mag, grad.z / mag);
}

#endif  // __HIPCC__

// ---------------------------------------------------------------------------------------------------- host side
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

}  // namespace curobo_hip
