// mapper.hip -- depth frames -> dense TSDF -> exact fp16 ESDF (curobo_amd/perception/mapper/mapper.py):
//   curobo_hip_mapper_clear_mask      the frame's visible mask to 0 (a kernel, so that a captured chain holds kernel nodes only)
//   curobo_hip_mapper_mark_blocks     one lane per (camera, pixel, sample along the ray): the blocks this frame sees
//   curobo_hip_mapper_integrate       one workgroup per block, at once back where the frame does not see it: the weighted
//                                     running mean of the projective signed distance, two fp16 words per voxel
//   curobo_hip_mapper_esdf_seed       one lane per ESDF cell: 7 TSDF probes decide whether the cell is a site
//   curobo_hip_mapper_edt_pass        one pass of the separable exact nearest-site transform, the lines of a tile in LDS
//   curobo_hip_mapper_esdf_distance   site -> signed fp16 distance
//   curobo_hip_mapper_occupied_flags  the rule of extract_occupied_voxels per voxel
//   curobo_hip_mapper_decay           per ever-visible block: its words times the block's factor, the weights summed, the block
//                                     recycled (words and mask byte to 0) where the sum is below the threshold
//   curobo_hip_mapper_decay_sensors   the same launch with the frusta of lidars beside the cameras' (lidar integration: mapper_lidar.hip)
//   curobo_hip_mapper_mesh_classify  extract_mesh, per (visible block, tile): corner values in LDS, the cubes' cases and counts
//   curobo_hip_mapper_mesh_vertices   ... per voxel: the vertices of its own cut edges, refined, with normals
//   curobo_hip_mapper_mesh_triangles  ... per voxel: the table's triangles through the edges' owner cubes, and which of them stay
//   curobo_hip_mapper_mesh_compact    ... per triangle: those that stay, in order
//
// Reference: perception/mapper/kernel/builder/builder_camera_integrate.py (compute_block_keys_only_kernel :89-166,
// integrate_voxels_kernel :400-487), builder_coord.py (world_to_continuous_voxel :45-54, voxel_to_world :57-66),
// builder_esdf.py (_esdf_to_tsdf_voxel_coords :107-133, _check_seed_at_world_pos :267-306, seed_esdf_sites_gather_kernel
// :308-406, compute_esdf_from_min_tsdf_kernel :412-491), wp_tsdf_sample.py (sample_dynamic_sdf :26-52), builder_raycast.py
// (count_occupied_voxels_kernel :1015-1042; sample_voxel :63-90, sample_tsdf_trilinear :168-258, compute_gradient :277-375),
// builder_mesh.py (refine_vertex_mesh :52-80, is_surface_cube_combined :147-229, the vertex and triangle kernels :376-675),
// marching_cubes/kernel/wp_mc_common.py (interpolate_edge_vertex :464-489), wp_mc_filter.py.  The reference keeps the blocks in a hash table over a pool; here the grid is
// dense, "block is allocated" is the byte block_mask, and nothing is allocated, hashed or counted with atomics: every store
// of a launch goes to a word no other lane of that launch writes, except the mask bytes, which every writer sets to 1.
//
// The nearest-site transform: after the pass along z a cell knows the nearest seed of its z line, after y of its x plane,
// after x of the grid (the squared distance separates by axis).  Within a pass the site of the line's cell j keeps j as its
// coordinate along the line, so the pass is min_j (d2(j) + (i - j)^2) with d2(j) the squared distance of cell j to its own
// site: d2 of a tile of lines is staged in LDS once and every cell scans its line by brute force, in integers.
//
// How positions, voxels, blocks, the stored pair, ESDF cells, sites and a camera's pixels are addressed and read: mapper_device.hpp.
#include "mapper_device.hpp"

namespace curobo_hip {

constexpr int kMapThreads = 256;
constexpr int kEdtThreads = 256;
constexpr int kEdtLdsWords = 8192;        // 32 KB: columns per tile = min(64, kEdtLdsWords / line length)
constexpr int kEdtNoSite = 1 << 30;       // above 3 * 1023^2 + 1023^2; kEdtNoSite + 1023^2 does not overflow

struct MapCameras {
  const float *depth, *intrinsics, *position, *quaternion;
  int n, height, width;
};

// ---------------------------------------------------------------------------------------------------- frame mask
__global__ __launch_bounds__(kMapThreads) void mapper_clear_mask_kernel(uint32_t *mask, int64_t n_words) {
  const int64_t i = (int64_t)blockIdx.x * kMapThreads + threadIdx.x;
  if (i < n_words) mask[i] = 0u;
}

// ---------------------------------------------------------------------------------------------------- stage 1: visible blocks
__global__ __launch_bounds__(kMapThreads) void mapper_mark_kernel(uint8_t *frame_mask, uint8_t *block_mask, MapCameras c, MapGrid g) {
  const int64_t tid = (int64_t)blockIdx.x * kMapThreads + threadIdx.x;
  const int n_pixels = c.height * c.width;
  const int64_t per_cam = (int64_t)n_pixels * g.num_samples;
  if (tid >= per_cam * c.n) return;
  const int cam = (int)(tid / per_cam);
  const int rem = (int)(tid - (int64_t)cam * per_cam);
  const int pixel = rem / g.num_samples, k = rem - pixel * g.num_samples;
  const int px = pixel % c.width, py = pixel / c.width;
  const float depth = c.depth[(size_t)cam * n_pixels + pixel];
  if (depth < g.depth_min || depth > g.depth_max) return;
  const float z_start = fmaxf(depth - g.trunc, g.depth_min);
  const float z = z_start + (float)k * g.step;
  if (z > depth + g.trunc + g.step) return;
  const MapCamera camera = read_camera(c.intrinsics, c.position, c.quaternion, cam);
  const f3 p = camera.t + quat_rotate(camera.qw, camera.qv, z * pixel_ray<true>(camera, px, py));  // (the z = 1 ray scaled, not normalised)
  const int vx = (int)floorf(grid_axis(g, p.x, g.ox, g.grid_w)), vy = (int)floorf(grid_axis(g, p.y, g.oy, g.grid_h));
  const int vz = (int)floorf(grid_axis(g, p.z, g.oz, g.grid_d));
  if (vx < 0 || vx >= g.grid_w || vy < 0 || vy >= g.grid_h || vz < 0 || vz >= g.grid_d) return;
  const int b = grid_block(g, vx, vy, vz);  // < nbx nby nbz: the voxel is inside the grid
  frame_mask[b] = 1;
  block_mask[b] = 1;
}

// ---------------------------------------------------------------------------------------------------- stage 2: voxels
__global__ __launch_bounds__(kMapThreads) void mapper_integrate_kernel(uint32_t *block_data, const uint8_t *frame_mask, MapCameras c, MapGrid g) {
  const int b = blockIdx.x;
  if (frame_mask[b] == 0) return;  // (uniform over the workgroup)
  const int bs3 = grid_block_voxels(g);
  for (int local = threadIdx.x; local < bs3; local += blockDim.x) {
    const i3 voxel = grid_voxel(g, b, local);
    const f3 centre = grid_centre(g, voxel.x, voxel.y, voxel.z);
    float total_sw = 0.0f, total_w = 0.0f;
    for (int cam = 0; cam < c.n; cam++) {
      const MapCamera camera = read_camera(c.intrinsics, c.position, c.quaternion, cam);
      const f3 v = quat_rotate(camera.qw, make_f3(-camera.qv.x, -camera.qv.y, -camera.qv.z), centre - camera.t);  // quat_inverse = the conjugate
      // The depth along the camera's axis once more in double (the z row of the same rotation): sdf = depth - z cancels to
      // nothing at the surface, where an fp32 z leaves an absolute error of a few 1e-7 m -- more than one step of the fp16
      // word that stores sdf * weight there (steps of 6e-8 .. 5e-7 below 1e-3).  Pixel choice and weight stay fp32.
      const double qw = camera.qw, qx = -(double)camera.qv.x, qy = -(double)camera.qv.y, qz = -(double)camera.qv.z;
      const double ex = grid_centre_axis<double>(g, voxel.x, g.grid_w, g.ox) - (double)camera.t.x;
      const double ey = grid_centre_axis<double>(g, voxel.y, g.grid_h, g.oy) - (double)camera.t.y;
      const double ez = grid_centre_axis<double>(g, voxel.z, g.grid_d, g.oz) - (double)camera.t.z;
      const double zd = ez * (2.0 * qw * qw - 1.0) + 2.0 * qw * (qx * ey - qy * ex) + 2.0 * qz * (qx * ex + qy * ey + qz * ez);
      const float z = (float)zd;
      if (!(zd > (double)g.depth_min)) continue;
      const float u = camera.fx * v.x / z + camera.cx, w = camera.fy * v.y / z + camera.cy;
      const int px = (int)u, py = (int)w;  // toward zero: u in (-1, 0) is pixel 0, as in the reference
      if (px < 0 || px >= c.width || py < 0 || py >= c.height) continue;
      const float depth = c.depth[((size_t)cam * c.height + py) * c.width + px];
      if (!(depth >= g.depth_min && depth <= g.depth_max)) continue;
      const float sdf = (float)((double)depth - zd);
      if (!(sdf >= -g.trunc)) continue;
      const float weight = fmaxf((camera.fx * g.vs / z) * (camera.fy * g.vs / z), 1.0f);  // compute_tsdf_weight is 1
      total_sw += fminf(sdf, g.trunc) * weight;
      total_w += weight;
    }
    if (total_w > 0.0f) {
      uint32_t *word = block_data + (size_t)b * bs3 + local;
      *word = tsdf_pair_add(*word, total_sw, total_w);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- ESDF stage 1: seed
__global__ __launch_bounds__(kMapThreads) void mapper_esdf_seed_kernel(int32_t *sites, EsdfArgs a, MapGrid g) {
  const int tid = blockIdx.x * kMapThreads + threadIdx.x;
  if (tid >= a.d * a.h * a.w) return;
  const int z = tid % a.w, y = (tid / a.w) % a.h, x = tid / (a.w * a.h);
  const float half = a.voxel_size[0] * 0.5f;
  const f3 c = esdf_centre(a, x, y, z);
  const auto seed_at = [&](float wx, float wy, float wz) { return is_seed(tsdf_probe(a.block_data, a.block_mask, g, make_f3(wx, wy, wz)), g); };
  const bool seed = seed_at(c.x, c.y, c.z) || seed_at(c.x + half, c.y, c.z) || seed_at(c.x - half, c.y, c.z) || seed_at(c.x, c.y + half, c.z) ||
                    seed_at(c.x, c.y - half, c.z) || seed_at(c.x, c.y, c.z + half) || seed_at(c.x, c.y, c.z - half);
  sites[tid] = seed ? site_pack(x, y, z) : -1;
}

// ---------------------------------------------------------------------------------------------------- ESDF stage 2: one pass
// The grid seen from the pass: lines of `len` cells `stride_a` words apart; the lines are (p, q) with q the faster of the two
// other axes.  A workgroup owns the `cols` lines q0 .. q0 + cols - 1 of one p.
struct EdtArgs {
  const int32_t *in;
  int32_t *out;
  int len, n_q, cols, axis;
  int64_t stride_a, stride_p, stride_q;
};

__global__ __launch_bounds__(kEdtThreads) void mapper_edt_pass_kernel(EdtArgs a) {
  __shared__ int d2[kEdtLdsWords];  // [j][col]
  const int tid = threadIdx.x, p = blockIdx.y, q0 = blockIdx.x * a.cols;
  const int32_t *in = a.in + (int64_t)p * a.stride_p;
  const bool along_memory = a.stride_a == 1;
  const int n = a.len * a.cols;  // <= kEdtLdsWords (the launcher's choice of cols)
  for (int idx = tid; idx < n; idx += kEdtThreads) {
    // consecutive lanes read consecutive words: along the line where the line is contiguous, else across the columns
    const int col = along_memory ? idx / a.len : idx % a.cols;
    const int j = along_memory ? idx % a.len : idx / a.cols;
    const int q = q0 + col;
    int v = kEdtNoSite;
    if (q < a.n_q) {
      const int32_t s = in[(int64_t)q * a.stride_q + (int64_t)j * a.stride_a];
      if (s >= 0) {
        // the cell's own coordinates: axis 2 = (p, q, j), axis 1 = (p, j, q), axis 0 = (j, p, q)
        const int x = a.axis == 0 ? j : p, y = a.axis == 0 ? p : (a.axis == 1 ? j : q), z = a.axis == 2 ? j : q;
        const int dx = site_offset(s, 0, x), dy = site_offset(s, 1, y), dz = site_offset(s, 2, z);
        v = dx * dx + dy * dy + dz * dz;
      }
    }
    d2[j * a.cols + col] = v;
  }
  __syncthreads();
  // cells of a column kEdtThreads / cols apart per lane; where the line is contiguous consecutive lanes take consecutive cells
  const int rows = kEdtThreads / a.cols;
  const int col = along_memory ? tid / rows : tid % a.cols;
  const int i0 = along_memory ? tid % rows : tid / a.cols;
  const int q = q0 + col;
  if (q >= a.n_q) return;
  const int64_t line = (int64_t)q * a.stride_q;
  for (int i = i0; i < a.len; i += rows) {
    int best = kEdtNoSite, best_j = -1;
    for (int j = 0; j < a.len; j++) {
      const int v = d2[j * a.cols + col] + (i - j) * (i - j);
      if (v < best) best = v, best_j = j;
    }
    a.out[(int64_t)p * a.stride_p + line + (int64_t)i * a.stride_a] = best_j >= 0 ? in[line + (int64_t)best_j * a.stride_a] : -1;
  }
}

// ---------------------------------------------------------------------------------------------------- ESDF stage 3: distance
// (the reference's skip_steps branch reads the static channel only, which this mapper does not have: left out)
__global__ __launch_bounds__(kMapThreads) void mapper_esdf_distance_kernel(uint16_t *distance, const int32_t *sites, EsdfArgs a, MapGrid g) {
  const int tid = blockIdx.x * kMapThreads + threadIdx.x;
  if (tid >= a.d * a.h * a.w) return;
  const int32_t s = sites[tid];
  float out = 1e4f;
  if (s >= 0) {
    const int z = tid % a.w, y = (tid / a.w) % a.h, x = tid / (a.w * a.h);
    const float dx = (float)site_offset(s, 0, x), dy = (float)site_offset(s, 1, y), dz = (float)site_offset(s, 2, z);
    out = sqrtf(dx * dx + dy * dy + dz * dz) * a.voxel_size[0];
    const float sdf = tsdf_probe(a.block_data, a.block_mask, g, esdf_centre(a, x, y, z));
    if (sdf_is_valid(sdf) && sdf < 0.0f) out = -out;
  }
  distance[tid] = __builtin_bit_cast(uint16_t, (_Float16)out);
}

// ---------------------------------------------------------------------------------------------------- occupied voxels
__global__ __launch_bounds__(kMapThreads) void mapper_occupied_kernel(uint8_t *flags, const uint32_t *block_data, const uint8_t *block_mask,
                                                                      int64_t n_voxels, int bs3, float min_weight, int surface_only,
                                                                      float sdf_threshold) {
  const int64_t i = (int64_t)blockIdx.x * kMapThreads + threadIdx.x;
  if (i >= n_voxels) return;
  uint8_t flag = 0;
  if (block_mask[i / bs3] != 0) {
    const float sdf = tsdf_pair_sdf<false>(block_data[i], min_weight);  // (above the minimum, as the probe rule)
    if (sdf_is_valid(sdf)) flag = surface_only ? (fabsf(sdf) < sdf_threshold) : (sdf <= 0.0f);
  }
  flags[i] = flag;
}

// ---------------------------------------------------------------------------------------------------- decay and recycling
// Per ever-visible block: both words of every voxel times the block's factor (factor_inside where the block lies in the union of
// the cameras' and the lidars' frusta, else factor_outside), the stored weights summed, and the block recycled -- words and mask byte to 0 -- where
// the sum is below empty_threshold (wp_decay.py:111-149, builder_decay.py:322-363).  recycled[b] says what this launch did.
struct DecayArgs {
  uint32_t *block_data;
  uint8_t *block_mask, *recycled;
  const float *intrinsics, *position, *quaternion;
  int n_cameras, height, width;
  float factor_outside, factor_inside, empty_threshold;
  const float *lidar_position, *lidar_quaternion, *lidar_valid_range, *lidar_elevation_range;  // curobo_hip_mapper_decay_sensors
  int n_lidars, lidar_height;
};

// mark_blocks_in_frustum_kernel (builder_decay.py:111-215) for one block and every camera: the block's bounding sphere against the
// depth range, then its projected disc against the image; the depth image is not read
__device__ __forceinline__ bool block_in_frusta(const DecayArgs &a, const MapGrid &g, int b) {
  const f3 centre = grid_block_centre(g, b);
  const float r = 0.866f * ((float)g.bs * g.vs);
  for (int cam = 0; cam < a.n_cameras; cam++) {
    const MapCamera c = read_camera(a.intrinsics, a.position, a.quaternion, cam);
    const f3 v = quat_rotate(c.qw, make_f3(-c.qv.x, -c.qv.y, -c.qv.z), centre - c.t);  // quat_inverse = the conjugate
    const float z = v.z;
    if (z + r < g.depth_min || z - r > g.depth_max) continue;
    if (z < 0.01f) return true;
    const float u = c.fx * v.x / z + c.cx, w = c.fy * v.y / z + c.cy;
    const float ru = c.fx * r / z, rw = c.fy * r / z;
    if (u + ru < 0.0f || u - ru > (float)a.width || w + rw < 0.0f || w - rw > (float)a.height) continue;
    return true;
  }
  // mark_lidar_blocks_in_frustum_kernel (builder_decay.py:217-313) for every lidar: the same sphere against the range band, then its
  // angular radius about the centre's elevation against the elevation band (a planar sensor: against its one elevation); a lidar
  // sees every azimuth, and no range image is read
  for (int i = 0; i < a.n_lidars; i++) {
    const MapLidar l = read_lidar(a.lidar_position, a.lidar_quaternion, a.lidar_valid_range, a.lidar_elevation_range, i);
    const f3 v = quat_rotate(l.qw, make_f3(-l.qv.x, -l.qv.y, -l.qv.z), centre - l.t);
    const float range = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    if (range + r < l.min_range || range - r > l.max_range) continue;
    const float elevation = atan2f(v.z, sqrtf(v.x * v.x + v.y * v.y));
    const float angular = range > r ? asinf(fminf(fmaxf(r / range, 0.0f), 1.0f)) : kLidarPi;
    if (a.lidar_height == 1) {
      if (fabsf(elevation - (l.min_elev + l.max_elev) * 0.5f) <= angular) return true;
      continue;
    }
    if (elevation + angular < l.min_elev || elevation - angular > l.max_elev) continue;
    return true;
  }
  return false;
}

// Blocks of G = bs^3 <= 64 voxels: G consecutive lanes own a block, a word each, and 256 / G blocks share a workgroup (the blocks of
// a wavefront are consecutive in memory: one 256-byte run).  The weights meet in a butterfly over the G lanes, whose pairs add
// in a fixed order and commute, so every lane of the block holds the same sum and decides alike; each word is stored once.
template <int G> __global__ __launch_bounds__(kMapThreads) void mapper_decay_lanes_kernel(DecayArgs a, MapGrid g, int n_blocks) {
  const int64_t tid = (int64_t)blockIdx.x * kMapThreads + threadIdx.x;
  const int64_t block = tid / G;
  const int b = block < n_blocks ? (int)block : n_blocks - 1;  // (lanes past the end take part in the butterfly and store nothing)
  const bool live = block < n_blocks && a.block_mask[b] != 0;
  uint32_t word = 0u;
  if (live) word = tsdf_pair_scale(a.block_data[tid], block_in_frusta(a, g, b) ? a.factor_inside : a.factor_outside);
  const float sum = group_sum<G>(half_hi(word));
  const bool recycle = live && sum < a.empty_threshold;
  if (live) a.block_data[tid] = recycle ? 0u : word;
  if (block < n_blocks && tid % G == 0) {
    if (recycle) a.block_mask[b] = 0;
    a.recycled[b] = recycle ? 1 : 0;
  }
}

// Blocks of 512 voxels or more: a workgroup per block, at once back where the block was never visible; a lane owns 16-byte
// runs of four voxels.  Lane sums in the order of the lane's runs, the wavefront's by the DPP ladder, the wavefronts' through
// LDS in wavefront order.  The scaled words are stored before the sum is known; a recycled block's owners store zeros over them.
__global__ __launch_bounds__(kMapThreads) void mapper_decay_block_kernel(DecayArgs a, MapGrid g) {
  __shared__ float wave_total[kMapThreads / kWave];
  const int b = blockIdx.x;
  if (a.block_mask[b] == 0) {  // (uniform over the workgroup: the byte is written after the barrier below only)
    if (threadIdx.x == 0) a.recycled[b] = 0;
    return;
  }
  const float f = block_in_frusta(a, g, b) ? a.factor_inside : a.factor_outside;
  const int runs = grid_block_voxels(g) / 4;  // a multiple of blockDim.x (the launcher's choice)
  uint4 *data = reinterpret_cast<uint4 *>(a.block_data + (size_t)b * grid_block_voxels(g));
  float sum = 0.0f;
  for (int i = threadIdx.x; i < runs; i += blockDim.x) {
    uint4 v = data[i];
    v.x = tsdf_pair_scale(v.x, f), v.y = tsdf_pair_scale(v.y, f), v.z = tsdf_pair_scale(v.z, f), v.w = tsdf_pair_scale(v.w, f);
    sum += (half_hi(v.x) + half_hi(v.y)) + (half_hi(v.z) + half_hi(v.w));
    data[i] = v;
  }
  sum = wave_sum(sum);
  if (threadIdx.x % kWave == 0) wave_total[threadIdx.x / kWave] = sum;
  __syncthreads();
  float total = wave_total[0];
  for (int w = 1; w < (int)blockDim.x / kWave; w++) total += wave_total[w];
  const bool recycle = total < a.empty_threshold;
  if (recycle)
    for (int i = threadIdx.x; i < runs; i += blockDim.x) data[i] = make_uint4(0u, 0u, 0u, 0u);
  if (threadIdx.x == 0) {
    if (recycle) a.block_mask[b] = 0;
    a.recycled[b] = recycle ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------- mesh extraction
// Marching cubes over the ever-visible blocks.  Slot k of the compacted list is block block_list[k]; block_slot maps a block
// back to its slot (-1: never visible).  Per-voxel scratch is [n_slots][bs^3] in the order (slot, voxel local index), which is
// the order of the output; the offsets into the vertex and triangle lists are prefix sums the caller forms between launches.
constexpr int kMeshTile = 8;                                                         // cubes per edge of a classify workgroup's tile
constexpr int kMeshTileCorners = (kMeshTile + 1) * (kMeshTile + 1) * (kMeshTile + 1);  // 729 corner values in LDS

struct MeshArgs {
  const uint32_t *block_data;
  const uint8_t *block_mask;
  const int32_t *block_list, *block_slot;
  int n_slots;
  float level;
};

// Stage 1, one workgroup per (slot, tile of min(bs, 8)^3 cubes): the (tile + 1)^3 corner values sw / w - level once into LDS,
// then per cube: is it a surface cube (builder_mesh.py:147-229), its case (:610-626), how many of its own edges 0, 3, 8 are
// cut (exactly one end negative) and how many triangles its table row holds.  A cube that is no surface cube gets case 0.
__global__ __launch_bounds__(kMapThreads) void mapper_mesh_classify_kernel(uint8_t *cube_case, uint8_t *vert_count, uint8_t *tri_count, MeshArgs a,
                                                                           const int8_t *table, int surface_only, MapGrid g) {
  __shared__ float corner[kMeshTileCorners];
  const int tb = g.bs < kMeshTile ? g.bs : kMeshTile, tiles = g.bs / tb, tiles3 = tiles * tiles * tiles;
  const int slot = blockIdx.x / tiles3, tile = blockIdx.x - slot * tiles3;
  const int b = a.block_list[slot];
  if (b < 0 || b >= g.nbx * g.nby * g.nbz) return;  // (uniform over the workgroup; the caller's list holds block rows only)
  const int tx = tile % tiles, ty = (tile / tiles) % tiles, tz = tile / (tiles * tiles);
  const i3 first = grid_voxel(g, b, 0);
  const int x0 = first.x + tx * tb, y0 = first.y + ty * tb, z0 = first.z + tz * tb;
  const int tc = tb + 1;
  for (int idx = threadIdx.x; idx < tc * tc * tc; idx += blockDim.x) {
    const float s = tsdf_voxel(a.block_data, a.block_mask, g, x0 + idx % tc, y0 + (idx / tc) % tc, z0 + idx / (tc * tc));
    corner[idx] = sdf_is_valid(s) ? s - a.level : kSdfInvalid;
  }
  __syncthreads();
  const int bs3 = grid_block_voxels(g);
  for (int v = threadIdx.x; v < tb * tb * tb; v += blockDim.x) {
    const int lx = v % tb, ly = (v / tb) % tb, lz = v / (tb * tb);
    const int at = (lz * tc + ly) * tc + lx;
    // corners 0..7 at (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1)
    const float s[8] = {corner[at],           corner[at + 1],           corner[at + tc + 1],           corner[at + tc],
                        corner[at + tc * tc], corner[at + tc * tc + 1], corner[at + tc * tc + tc + 1], corner[at + tc * tc + tc]};
    bool valid = true, positive = false, negative = false, in_band = false;
    int config = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      valid &= sdf_is_valid(s[c]);
      positive |= s[c] > 0.0f;
      negative |= s[c] < 0.0f;
      in_band |= fabsf(s[c]) < g.trunc;
      config |= (s[c] < 0.0f) << c;
    }
    const bool surface = valid && positive && negative && (!surface_only || in_band);
    int n_vert = 0, n_tri = 0;
    if (surface) {
      n_vert = (int)((s[0] < 0.0f) != (s[1] < 0.0f)) + (int)((s[0] < 0.0f) != (s[3] < 0.0f)) + (int)((s[0] < 0.0f) != (s[4] < 0.0f));
      while (n_tri < 5 && table[config * 16 + n_tri * 3] >= 0) n_tri++;
    }
    const size_t out = (size_t)slot * bs3 + ((tz * tb + lz) * g.bs + ty * tb + ly) * g.bs + tx * tb + lx;
    cube_case[out] = surface ? (uint8_t)config : (uint8_t)0;
    vert_count[out] = (uint8_t)n_vert;
    tri_count[out] = (uint8_t)n_tri;
  }
}

// Stage 2, one lane per voxel of the visible blocks: the vertices of its own cut edges at vert_offset[i] .. in the order x, y,
// z, refined (builder_mesh.py:52-80) and with their normals, and the voxel's three vertex ids (-1 where it emits none)
__global__ __launch_bounds__(kMapThreads) void mapper_mesh_vertices_kernel(float *vertices, float *normals, int32_t *vert_ids, int n_vertices,
                                                                           const uint8_t *vert_count, const int32_t *vert_offset, MeshArgs a,
                                                                           int refine_iterations, MapGrid g) {
  const int bs3 = grid_block_voxels(g);
  const int64_t i = (int64_t)blockIdx.x * kMapThreads + threadIdx.x;
  if (i >= (int64_t)a.n_slots * bs3) return;
  int32_t *ids = vert_ids + (size_t)i * 3;
  ids[0] = ids[1] = ids[2] = -1;
  if (vert_count[i] == 0) return;
  const int slot = (int)(i / bs3), local = (int)(i - (int64_t)slot * bs3);
  const int b = a.block_list[slot];
  if (b < 0 || b >= g.nbx * g.nby * g.nbz) return;
  const i3 voxel = grid_voxel(g, b, local);
  const int gx = voxel.x, gy = voxel.y, gz = voxel.z;
  // (a surface cube: all four are valid)
  const float s0 = tsdf_voxel(a.block_data, a.block_mask, g, gx, gy, gz) - a.level;
  const float sb[3] = {tsdf_voxel(a.block_data, a.block_mask, g, gx + 1, gy, gz) - a.level,
                       tsdf_voxel(a.block_data, a.block_mask, g, gx, gy + 1, gz) - a.level,
                       tsdf_voxel(a.block_data, a.block_mask, g, gx, gy, gz + 1) - a.level};
  // the cube's edges run between voxel centres: this voxel's and, per axis, its upper neighbour's
  const f3 ca = grid_centre(g, gx, gy, gz), cb = grid_centre(g, gx + 1, gy + 1, gz + 1);
  const float pa[3] = {ca.x, ca.y, ca.z}, pb[3] = {cb.x, cb.y, cb.z};
  int vid = vert_offset[i];
#pragma unroll
  for (int axis = 0; axis < 3; axis++) {
    if ((s0 < 0.0f) == (sb[axis] < 0.0f)) continue;
    if (vid < 0 || vid >= n_vertices) return;  // (offsets that do not belong to these counts)
    const float t = fminf(fmaxf(-s0 / (sb[axis] - s0), 0.0f), 1.0f);  // wp_mc_common.py:487-488
    float p[3] = {pa[0], pa[1], pa[2]};
    p[axis] = pa[axis] + t * (pb[axis] - pa[axis]);
    f3 pos = make_f3(p[0], p[1], p[2]);
    for (int it = 0; it < refine_iterations; it++) {
      const float sdf = tsdf_trilinear(a.block_data, a.block_mask, g, pos);
      if (sdf_is_invalid(sdf)) break;
      const float value = sdf - a.level;
      if (fabsf(value) < 1e-6f || value > 100.0f) break;
      const f3 dir = tsdf_gradient<true>(a.block_data, a.block_mask, g, pos);
      const float step = fminf(fmaxf(value, -0.5f * g.vs), 0.5f * g.vs);
      pos = pos - step * dir;
    }
    const f3 n = tsdf_gradient<false>(a.block_data, a.block_mask, g, pos);
    float *vo = vertices + (size_t)vid * 3, *no = normals + (size_t)vid * 3;
    vo[0] = pos.x, vo[1] = pos.y, vo[2] = pos.z;
    no[0] = n.x, no[1] = n.y, no[2] = n.z;
    ids[axis] = vid++;
  }
}

// Stage 3, one lane per voxel of the visible blocks: the triangles of the cube's table row at tri_offset[i] .., every corner the
// vertex of the edge's owner cube (edge_owner[e] = dx, dy, dz, axis), -1 where that cube emits none or is not there; and per
// triangle whether it stays: three vertices, all different, |cross|^2 above (voxel_size 1e-6)^2  (wp_mc_filter.py:91-108, :156)
__global__ __launch_bounds__(kMapThreads) void mapper_mesh_triangles_kernel(int32_t *raw, uint8_t *keep, int n_raw, const uint8_t *cube_case,
                                                                            const uint8_t *tri_count, const int32_t *tri_offset,
                                                                            const int32_t *vert_ids, const float *vertices, int n_vertices, MeshArgs a,
                                                                            const int8_t *table, const int8_t *edge_owner, MapGrid g) {
  const int bs3 = grid_block_voxels(g);
  const int64_t i = (int64_t)blockIdx.x * kMapThreads + threadIdx.x;
  if (i >= (int64_t)a.n_slots * bs3) return;
  const int count = tri_count[i];
  if (count == 0) return;
  const int slot = (int)(i / bs3), local = (int)(i - (int64_t)slot * bs3);
  const int b = a.block_list[slot];
  if (b < 0 || b >= g.nbx * g.nby * g.nbz) return;
  const i3 voxel = grid_voxel(g, b, local);
  const int gx = voxel.x, gy = voxel.y, gz = voxel.z;
  const int8_t *row = table + (int)cube_case[i] * 16;
  const int base = tri_offset[i];
  const float min_cross2 = (g.vs * 1e-6f) * (g.vs * 1e-6f);
  for (int t = 0; t < count && t < 5; t++) {
    if (base < 0 || base + t >= n_raw) return;  // (offsets that do not belong to these counts)
    int id[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int e = row[t * 3 + k];
      id[k] = -1;
      if (e < 0 || e >= 12) continue;
      const int ox = gx + edge_owner[e * 4], oy = gy + edge_owner[e * 4 + 1], oz = gz + edge_owner[e * 4 + 2], axis = edge_owner[e * 4 + 3];
      if (ox >= g.nbx * g.bs || oy >= g.nby * g.bs || oz >= g.nbz * g.bs || axis < 0 || axis > 2) continue;
      const int os = a.block_slot[grid_block(g, ox, oy, oz)];
      if (os < 0 || os >= a.n_slots) continue;
      id[k] = vert_ids[((size_t)os * bs3 + grid_local(g, ox, oy, oz)) * 3 + axis];
      if (id[k] >= n_vertices) id[k] = -1;
    }
    bool stays = id[0] >= 0 && id[1] >= 0 && id[2] >= 0 && id[0] != id[1] && id[1] != id[2] && id[0] != id[2];
    if (stays) {
      const float *v0 = vertices + (size_t)id[0] * 3, *v1 = vertices + (size_t)id[1] * 3, *v2 = vertices + (size_t)id[2] * 3;
      const f3 p0 = make_f3(v0[0], v0[1], v0[2]);
      const f3 c = cross(make_f3(v1[0], v1[1], v1[2]) - p0, make_f3(v2[0], v2[1], v2[2]) - p0);
      stays = !(dot(c, c) <= min_cross2);
    }
    int32_t *out = raw + (size_t)(base + t) * 3;
    out[0] = id[0], out[1] = id[1], out[2] = id[2];
    keep[base + t] = stays ? 1 : 0;
  }
}

// Stage 4, one lane per triangle of stage 3: those that stay to keep_offset[j], in their order
__global__ __launch_bounds__(kMapThreads) void mapper_mesh_compact_kernel(int32_t *triangles, int n_triangles, const int32_t *raw, const uint8_t *keep,
                                                                          const int32_t *keep_offset, int n_raw) {
  const int64_t j = (int64_t)blockIdx.x * kMapThreads + threadIdx.x;
  if (j >= n_raw || keep[j] == 0) return;
  const int o = keep_offset[j];
  if (o < 0 || o >= n_triangles) return;
  triangles[(size_t)o * 3] = raw[(size_t)j * 3], triangles[(size_t)o * 3 + 1] = raw[(size_t)j * 3 + 1], triangles[(size_t)o * 3 + 2] = raw[(size_t)j * 3 + 2];
}

}  // namespace curobo_hip

using namespace curobo_hip;

// ---------------------------------------------------------------------------------------------------- host side
static int64_t map_blocks(const MapGrid &g) { return (int64_t)g.nbx * g.nby * g.nbz; }

static int read_cameras(MapCameras *c, const float *depth, const float *intrinsics, const float *cam_position, const float *cam_quaternion,
                        int n_cameras, int height, int width, const char *what) {
  CUROBO_REQUIRE(depth && intrinsics && cam_position && cam_quaternion,
                 "%s: depth, intrinsics, cam_position and cam_quaternion must not be null", what);
  CUROBO_REQUIRE(n_cameras > 0 && height > 0 && width > 0, "%s: depth must be (n_cameras, H, W), got (%d, %d, %d)", what, n_cameras, height,
                 width);
  CUROBO_REQUIRE((int64_t)n_cameras * height * width < ((int64_t)1 << 31), "%s: the depth images hold 2^31 pixels or more", what);
  c->depth = depth, c->intrinsics = intrinsics, c->position = cam_position, c->quaternion = cam_quaternion;
  c->n = n_cameras, c->height = height, c->width = width;
  return CUROBO_HIP_OK;
}

CUROBO_EXPORT int curobo_hip_mapper_clear_mask(uint8_t *mask, int64_t n_bytes, curobo_hip_stream_t stream) {
  const char *what = "mapper_clear_mask";
  CUROBO_REQUIRE(mask, "%s: mask must not be null", what);
  CUROBO_REQUIRE(n_bytes > 0 && n_bytes % 4 == 0 && ((uintptr_t)mask & 3) == 0,
                 "%s: the mask must be 4-byte aligned and a positive multiple of 4 bytes long, got %lld", what, (long long)n_bytes);
  const int64_t words = n_bytes / 4;
  hipLaunchKernelGGL(mapper_clear_mask_kernel, dim3((unsigned)ceil_div_l(words, kMapThreads)), dim3(kMapThreads), 0, (hipStream_t)stream,
                     (uint32_t *)mask, words);
  return check_launch(what, (hipStream_t)stream);
}

CUROBO_EXPORT int curobo_hip_mapper_mark_blocks(uint8_t *frame_mask, uint8_t *block_mask, const float *depth, const float *intrinsics,
                                                const float *cam_position, const float *cam_quaternion,
                                                const curobo_hip_mapper_params *params, int n_cameras, int height, int width,
                                                curobo_hip_stream_t stream) {
  const char *what = "mapper_mark_blocks";
  MapGrid g;
  MapCameras c;
  if (int rc = read_params(params, &g, what)) return rc;
  if (int rc = read_cameras(&c, depth, intrinsics, cam_position, cam_quaternion, n_cameras, height, width, what)) return rc;
  CUROBO_REQUIRE(frame_mask && block_mask, "%s: frame_mask and block_mask must not be null", what);
  CUROBO_REQUIRE(g.num_samples > 0 && g.step > 0.0f, "%s: num_samples and step_size must be positive, got %d and %g", what, g.num_samples,
                 (double)g.step);
  const int64_t lanes = (int64_t)n_cameras * height * width * g.num_samples;
  CUROBO_REQUIRE(lanes < ((int64_t)1 << 31) * kMapThreads, "%s: %lld samples are more than one launch holds", what, (long long)lanes);
  hipLaunchKernelGGL(mapper_mark_kernel, dim3((unsigned)ceil_div_l(lanes, kMapThreads)), dim3(kMapThreads), 0, (hipStream_t)stream, frame_mask,
                     block_mask, c, g);
  return check_launch(what, (hipStream_t)stream);
}

CUROBO_EXPORT int curobo_hip_mapper_integrate(void *block_data, const uint8_t *frame_mask, const float *depth, const float *intrinsics,
                                              const float *cam_position, const float *cam_quaternion,
                                              const curobo_hip_mapper_params *params, int n_cameras, int height, int width,
                                              curobo_hip_stream_t stream) {
  const char *what = "mapper_integrate";
  MapGrid g;
  MapCameras c;
  if (int rc = read_params(params, &g, what)) return rc;
  if (int rc = read_cameras(&c, depth, intrinsics, cam_position, cam_quaternion, n_cameras, height, width, what)) return rc;
  if (int rc = check_map(block_data && frame_mask, block_data, "block_data and frame_mask", what)) return rc;
  const int bs3 = g.bs * g.bs * g.bs;
  hipLaunchKernelGGL(mapper_integrate_kernel, dim3((unsigned)map_blocks(g)), dim3(bs3 >= kMapThreads ? kMapThreads : kWave), 0,
                     (hipStream_t)stream, (uint32_t *)block_data, frame_mask, c, g);
  return check_launch(what, (hipStream_t)stream);
}

static int check_esdf_shape(int esdf_d, int esdf_h, int esdf_w, const char *what) {
  CUROBO_REQUIRE(esdf_d > 0 && esdf_h > 0 && esdf_w > 0 && esdf_d <= kEsdfMaxAxis && esdf_h <= kEsdfMaxAxis && esdf_w <= kEsdfMaxAxis,
                 "%s: every axis of the ESDF grid must hold 1..%d cells (sites pack 10 bits per axis), got %d x %d x %d", what, kEsdfMaxAxis,
                 esdf_d, esdf_h, esdf_w);
  return CUROBO_HIP_OK;
}
static int read_esdf(EsdfArgs *a, const void *block_data, const uint8_t *block_mask, const float *esdf_origin, const float *esdf_voxel_size,
                     int esdf_d, int esdf_h, int esdf_w, const char *what) {
  if (int rc = check_map(block_data && block_mask && esdf_origin && esdf_voxel_size, block_data,
                         "block_data, block_mask, esdf_origin and esdf_voxel_size", what)) return rc;
  if (int rc = check_esdf_shape(esdf_d, esdf_h, esdf_w, what)) return rc;
  a->block_data = (const uint32_t *)block_data, a->block_mask = block_mask, a->origin = esdf_origin, a->voxel_size = esdf_voxel_size;
  a->d = esdf_d, a->h = esdf_h, a->w = esdf_w;
  return CUROBO_HIP_OK;
}

CUROBO_EXPORT int curobo_hip_mapper_esdf_seed(int32_t *sites, const void *block_data, const uint8_t *block_mask, const float *esdf_origin,
                                              const float *esdf_voxel_size, const curobo_hip_mapper_params *params, int esdf_d, int esdf_h,
                                              int esdf_w, curobo_hip_stream_t stream) {
  const char *what = "mapper_esdf_seed";
  MapGrid g;
  EsdfArgs a;
  if (int rc = read_params(params, &g, what)) return rc;
  if (int rc = read_esdf(&a, block_data, block_mask, esdf_origin, esdf_voxel_size, esdf_d, esdf_h, esdf_w, what)) return rc;
  CUROBO_REQUIRE(sites, "%s: sites must not be null", what);
  const int cells = esdf_d * esdf_h * esdf_w;  // <= 2^30
  hipLaunchKernelGGL(mapper_esdf_seed_kernel, dim3((unsigned)ceil_div(cells, kMapThreads)), dim3(kMapThreads), 0, (hipStream_t)stream, sites, a, g);
  return check_launch(what, (hipStream_t)stream);
}

CUROBO_EXPORT int curobo_hip_mapper_edt_pass(int32_t *sites_out, const int32_t *sites_in, int esdf_d, int esdf_h, int esdf_w, int axis,
                                             curobo_hip_stream_t stream) {
  const char *what = "mapper_edt_pass";
  CUROBO_REQUIRE(sites_out && sites_in, "%s: sites_out and sites_in must not be null", what);
  if (int rc = check_esdf_shape(esdf_d, esdf_h, esdf_w, what)) return rc;
  CUROBO_REQUIRE(axis >= 0 && axis <= 2, "%s: axis must be 0 (x), 1 (y) or 2 (z), got %d", what, axis);
  const int64_t cells = (int64_t)esdf_d * esdf_h * esdf_w;
  CUROBO_REQUIRE(sites_out + cells <= sites_in || sites_in + cells <= sites_out, "%s: sites_out and sites_in must not overlap", what);
  EdtArgs a{};
  a.in = sites_in, a.out = sites_out, a.axis = axis;
  int n_p;
  const int64_t hw = (int64_t)esdf_h * esdf_w;
  if (axis == 2) a.len = esdf_w, n_p = esdf_d, a.n_q = esdf_h, a.stride_a = 1, a.stride_p = hw, a.stride_q = esdf_w;
  else if (axis == 1) a.len = esdf_h, n_p = esdf_d, a.n_q = esdf_w, a.stride_a = esdf_w, a.stride_p = hw, a.stride_q = 1;
  else a.len = esdf_d, n_p = esdf_h, a.n_q = esdf_w, a.stride_a = hw, a.stride_p = esdf_w, a.stride_q = 1;
  // columns per workgroup: a power of two that divides the workgroup, fits the LDS tile (len <= 1024 leaves 8 or more) and does
  // not run far past the lines there are; a pass along memory takes 4, so that a wavefront's 64 lanes write one line's run
  int cols = a.stride_a == 1 ? 4 : 64;
  while (cols * a.len > kEdtLdsWords) cols /= 2;
  while (cols / 2 >= a.n_q) cols /= 2;
  a.cols = cols;
  hipLaunchKernelGGL(mapper_edt_pass_kernel, dim3((unsigned)ceil_div(a.n_q, cols), (unsigned)n_p), dim3(kEdtThreads), 0, (hipStream_t)stream, a);
  return check_launch(what, (hipStream_t)stream);
}

CUROBO_EXPORT int curobo_hip_mapper_esdf_distance(void *distance, const int32_t *sites, const void *block_data, const uint8_t *block_mask,
                                                  const float *esdf_origin, const float *esdf_voxel_size,
                                                  const curobo_hip_mapper_params *params, int esdf_d, int esdf_h, int esdf_w,
                                                  curobo_hip_stream_t stream) {
  const char *what = "mapper_esdf_distance";
  MapGrid g;
  EsdfArgs a;
  if (int rc = read_params(params, &g, what)) return rc;
  if (int rc = read_esdf(&a, block_data, block_mask, esdf_origin, esdf_voxel_size, esdf_d, esdf_h, esdf_w, what)) return rc;
  CUROBO_REQUIRE(distance && sites, "%s: distance and sites must not be null", what);
  CUROBO_REQUIRE(((uintptr_t)distance & 1) == 0, "%s: distance must be 2-byte aligned", what);
  const int cells = esdf_d * esdf_h * esdf_w;
  hipLaunchKernelGGL(mapper_esdf_distance_kernel, dim3((unsigned)ceil_div(cells, kMapThreads)), dim3(kMapThreads), 0, (hipStream_t)stream,
                     (uint16_t *)distance, sites, a, g);
  return check_launch(what, (hipStream_t)stream);
}

CUROBO_EXPORT int curobo_hip_mapper_occupied_flags(uint8_t *flags, const void *block_data, const uint8_t *block_mask,
                                                   const curobo_hip_mapper_params *params, int surface_only, float sdf_threshold,
                                                   curobo_hip_stream_t stream) {
  const char *what = "mapper_occupied_flags";
  MapGrid g;
  if (int rc = read_params(params, &g, what)) return rc;
  if (int rc = check_map(flags && block_data && block_mask, block_data, "flags, block_data and block_mask", what)) return rc;
  const int bs3 = g.bs * g.bs * g.bs;
  const int64_t voxels = map_blocks(g) * bs3;
  hipLaunchKernelGGL(mapper_occupied_kernel, dim3((unsigned)ceil_div_l(voxels, kMapThreads)), dim3(kMapThreads), 0, (hipStream_t)stream, flags,
                     (const uint32_t *)block_data, block_mask, voxels, bs3, g.min_weight, surface_only != 0, sdf_threshold);
  return check_launch(what, (hipStream_t)stream);
}

static int launch_decay(const char *what, void *block_data, uint8_t *block_mask, uint8_t *recycled, const float *intrinsics,
                        const float *cam_position, const float *cam_quaternion, int n_cameras, int height, int width,
                        const float *lidar_position, const float *lidar_quaternion, const float *lidar_valid_range,
                        const float *lidar_elevation_range, int n_lidars, int lidar_height, float factor_outside, float factor_inside,
                        float empty_threshold, const curobo_hip_mapper_params *params, curobo_hip_stream_t stream) {
  MapGrid g;
  if (int rc = read_params(params, &g, what)) return rc;
  if (int rc = check_map(block_data && block_mask && recycled, block_data, "block_data, block_mask and recycled", what)) return rc;
  CUROBO_REQUIRE(n_cameras >= 0, "%s: n_cameras must be >= 0 (0: no frustum test), got %d", what, n_cameras);
  CUROBO_REQUIRE(n_cameras == 0 || (intrinsics && cam_position && cam_quaternion && height > 0 && width > 0),
                 "%s: with n_cameras = %d, intrinsics, cam_position and cam_quaternion must not be null and the image %d x %d positive", what,
                 n_cameras, height, width);
  CUROBO_REQUIRE(n_lidars >= 0, "%s: n_lidars must be >= 0 (0: no lidar frustum), got %d", what, n_lidars);
  CUROBO_REQUIRE(n_lidars == 0 || (lidar_position && lidar_quaternion && lidar_valid_range && lidar_elevation_range && lidar_height > 0),
                 "%s: with n_lidars = %d, lidar_position, lidar_quaternion, lidar_valid_range and lidar_elevation_range must not be null "
                 "and lidar_height = %d positive", what, n_lidars, lidar_height);
  CUROBO_REQUIRE(factor_outside >= 0.0f && factor_outside <= 1.0f && factor_inside >= 0.0f && factor_inside <= 1.0f,
                 "%s: factor_outside and factor_inside must lie in [0, 1], got %g and %g", what, (double)factor_outside, (double)factor_inside);
  CUROBO_REQUIRE(empty_threshold >= 0.0f, "%s: empty_threshold must be >= 0, got %g", what, (double)empty_threshold);
  DecayArgs a{};
  a.block_data = (uint32_t *)block_data, a.block_mask = block_mask, a.recycled = recycled;
  a.intrinsics = intrinsics, a.position = cam_position, a.quaternion = cam_quaternion;
  a.n_cameras = n_cameras, a.height = height, a.width = width;
  a.factor_outside = factor_outside, a.factor_inside = factor_inside, a.empty_threshold = empty_threshold;
  a.lidar_position = lidar_position, a.lidar_quaternion = lidar_quaternion, a.lidar_valid_range = lidar_valid_range;
  a.lidar_elevation_range = lidar_elevation_range, a.n_lidars = n_lidars, a.lidar_height = lidar_height;
  const int bs3 = g.bs * g.bs * g.bs, n_blocks = (int)map_blocks(g);
  const hipStream_t s = (hipStream_t)stream;
  if (bs3 > kWave) {  // 512 voxels or more: 128 runs of four voxels, or a multiple of 256
    CUROBO_REQUIRE(((uintptr_t)block_data & 15) == 0, "%s: block_data must be 16-byte aligned for blocks of %d voxels", what, bs3);
    hipLaunchKernelGGL(mapper_decay_block_kernel, dim3((unsigned)n_blocks), dim3(bs3 / 4 < kMapThreads ? bs3 / 4 : kMapThreads), 0, s, a, g);
  } else {
    const dim3 grid((unsigned)ceil_div_l((int64_t)n_blocks * bs3, kMapThreads)), lanes(kMapThreads);
    if (bs3 == 1) hipLaunchKernelGGL(mapper_decay_lanes_kernel<1>, grid, lanes, 0, s, a, g, n_blocks);
    else if (bs3 == 8) hipLaunchKernelGGL(mapper_decay_lanes_kernel<8>, grid, lanes, 0, s, a, g, n_blocks);
    else hipLaunchKernelGGL(mapper_decay_lanes_kernel<64>, grid, lanes, 0, s, a, g, n_blocks);
  }
  return check_launch(what, s);
}

CUROBO_EXPORT int curobo_hip_mapper_decay(void *block_data, uint8_t *block_mask, uint8_t *recycled, const float *intrinsics,
                                          const float *cam_position, const float *cam_quaternion, int n_cameras, int height, int width,
                                          float factor_outside, float factor_inside, float empty_threshold,
                                          const curobo_hip_mapper_params *params, curobo_hip_stream_t stream) {
  return launch_decay("mapper_decay", block_data, block_mask, recycled, intrinsics, cam_position, cam_quaternion, n_cameras, height, width,
                      nullptr, nullptr, nullptr, nullptr, 0, 0, factor_outside, factor_inside, empty_threshold, params, stream);
}

CUROBO_EXPORT int curobo_hip_mapper_decay_sensors(void *block_data, uint8_t *block_mask, uint8_t *recycled, const float *intrinsics,
                                                  const float *cam_position, const float *cam_quaternion, int n_cameras, int height,
                                                  int width, const float *lidar_position, const float *lidar_quaternion,
                                                  const float *lidar_valid_range, const float *lidar_elevation_range, int n_lidars,
                                                  int lidar_height, float factor_outside, float factor_inside, float empty_threshold,
                                                  const curobo_hip_mapper_params *params, curobo_hip_stream_t stream) {
  return launch_decay("mapper_decay_sensors", block_data, block_mask, recycled, intrinsics, cam_position, cam_quaternion, n_cameras, height,
                      width, lidar_position, lidar_quaternion, lidar_valid_range, lidar_elevation_range, n_lidars, lidar_height,
                      factor_outside, factor_inside, empty_threshold, params, stream);
}

static int check_slots(int n_slots, const MapGrid &g, const char *what) {
  CUROBO_REQUIRE(n_slots > 0 && n_slots <= map_blocks(g), "%s: block_list must hold 1..%lld blocks, got %d", what, (long long)map_blocks(g), n_slots);
  return CUROBO_HIP_OK;
}
static int read_mesh(MeshArgs *a, const void *block_data, const uint8_t *block_mask, const int32_t *block_list, const int32_t *block_slot,
                     int n_slots, float level, const MapGrid &g, const char *what) {
  if (int rc = check_map(block_data && block_mask && block_list, block_data, "block_data, block_mask and block_list", what)) return rc;
  if (int rc = check_slots(n_slots, g, what)) return rc;
  a->block_data = (const uint32_t *)block_data, a->block_mask = block_mask, a->block_list = block_list, a->block_slot = block_slot;
  a->n_slots = n_slots, a->level = level;
  return CUROBO_HIP_OK;
}

CUROBO_EXPORT int curobo_hip_mapper_mesh_classify(uint8_t *cube_case, uint8_t *vert_count, uint8_t *tri_count, const void *block_data,
                                                  const uint8_t *block_mask, const int32_t *block_list, int n_slots, const int8_t *table,
                                                  const curobo_hip_mapper_params *params, float level, int surface_only,
                                                  curobo_hip_stream_t stream) {
  const char *what = "mapper_mesh_classify";
  MapGrid g;
  MeshArgs a;
  if (int rc = read_params(params, &g, what)) return rc;
  if (int rc = read_mesh(&a, block_data, block_mask, block_list, nullptr, n_slots, level, g, what)) return rc;
  CUROBO_REQUIRE(cube_case && vert_count && tri_count && table, "%s: cube_case, vert_count, tri_count and table must not be null", what);
  const int tb = g.bs < kMeshTile ? g.bs : kMeshTile, tiles = g.bs / tb;
  const int64_t groups = (int64_t)n_slots * tiles * tiles * tiles;  // <= the voxels of the padded grid < 2^31
  hipLaunchKernelGGL(mapper_mesh_classify_kernel, dim3((unsigned)groups), dim3(tb * tb * tb >= kMapThreads ? kMapThreads : kWave), 0,
                     (hipStream_t)stream, cube_case, vert_count, tri_count, a, table, surface_only != 0, g);
  return check_launch(what, (hipStream_t)stream);
}

CUROBO_EXPORT int curobo_hip_mapper_mesh_vertices(float *vertices, float *normals, int32_t *vert_ids, int n_vertices, const uint8_t *vert_count,
                                                  const int32_t *vert_offset, const void *block_data, const uint8_t *block_mask,
                                                  const int32_t *block_list, int n_slots, const curobo_hip_mapper_params *params, float level,
                                                  int refine_iterations, curobo_hip_stream_t stream) {
  const char *what = "mapper_mesh_vertices";
  MapGrid g;
  MeshArgs a;
  if (int rc = read_params(params, &g, what)) return rc;
  if (int rc = read_mesh(&a, block_data, block_mask, block_list, nullptr, n_slots, level, g, what)) return rc;
  CUROBO_REQUIRE(vertices && normals && vert_ids && vert_count && vert_offset,
                 "%s: vertices, normals, vert_ids, vert_count and vert_offset must not be null", what);
  CUROBO_REQUIRE(n_vertices > 0 && refine_iterations >= 0, "%s: n_vertices must be positive and refine_iterations >= 0, got %d and %d", what,
                 n_vertices, refine_iterations);
  const int64_t voxels = (int64_t)n_slots * g.bs * g.bs * g.bs;
  hipLaunchKernelGGL(mapper_mesh_vertices_kernel, dim3((unsigned)ceil_div_l(voxels, kMapThreads)), dim3(kMapThreads), 0, (hipStream_t)stream,
                     vertices, normals, vert_ids, n_vertices, vert_count, vert_offset, a, refine_iterations, g);
  return check_launch(what, (hipStream_t)stream);
}

CUROBO_EXPORT int curobo_hip_mapper_mesh_triangles(int32_t *raw_triangles, uint8_t *keep, int n_raw, const uint8_t *cube_case,
                                                   const uint8_t *tri_count, const int32_t *tri_offset, const int32_t *vert_ids,
                                                   const float *vertices, int n_vertices, const int32_t *block_list,
                                                   const int32_t *block_slot, int n_slots, const int8_t *table, const int8_t *edge_owner,
                                                   const curobo_hip_mapper_params *params, curobo_hip_stream_t stream) {
  const char *what = "mapper_mesh_triangles";
  MapGrid g;
  if (int rc = read_params(params, &g, what)) return rc;
  CUROBO_REQUIRE(raw_triangles && keep && cube_case && tri_count && tri_offset && vert_ids && vertices && block_list && block_slot && table &&
                     edge_owner,
                 "%s: no pointer may be null", what);
  if (int rc = check_slots(n_slots, g, what)) return rc;
  MeshArgs a{};  // (this launch reads no TSDF)
  a.block_list = block_list, a.block_slot = block_slot, a.n_slots = n_slots;
  CUROBO_REQUIRE(n_raw > 0 && n_vertices > 0, "%s: n_raw and n_vertices must be positive, got %d and %d", what, n_raw, n_vertices);
  const int64_t voxels = (int64_t)n_slots * g.bs * g.bs * g.bs;
  hipLaunchKernelGGL(mapper_mesh_triangles_kernel, dim3((unsigned)ceil_div_l(voxels, kMapThreads)), dim3(kMapThreads), 0, (hipStream_t)stream,
                     raw_triangles, keep, n_raw, cube_case, tri_count, tri_offset, vert_ids, vertices, n_vertices, a, table, edge_owner, g);
  return check_launch(what, (hipStream_t)stream);
}

CUROBO_EXPORT int curobo_hip_mapper_mesh_compact(int32_t *triangles, int n_triangles, const int32_t *raw_triangles, const uint8_t *keep,
                                                 const int32_t *keep_offset, int n_raw, curobo_hip_stream_t stream) {
  const char *what = "mapper_mesh_compact";
  CUROBO_REQUIRE(triangles && raw_triangles && keep && keep_offset, "%s: no pointer may be null", what);
  CUROBO_REQUIRE(n_raw > 0 && n_triangles > 0 && n_triangles <= n_raw, "%s: need 0 < n_triangles <= n_raw, got %d and %d", what, n_triangles,
                 n_raw);
  hipLaunchKernelGGL(mapper_mesh_compact_kernel, dim3((unsigned)ceil_div(n_raw, kMapThreads)), dim3(kMapThreads), 0, (hipStream_t)stream, triangles,
                     n_triangles, raw_triangles, keep, keep_offset, n_raw);
  return check_launch(what, (hipStream_t)stream);
}
