/*
 * curobo_hip.h -- C ABI of libcurobo_hip.so, the MI355X (gfx950) kernel backend for cuRobo's
 * batched motion-generation hot path.
 *
 * This is the drop-in boundary: every entry point replaces one module-level launch function of
 * the reference's kernel backend (curobo/_src/curobolib/backends/__init__.py:162-227; the two
 * existing backends are cuda_core_backend/ (Python) and pybind/ (C++ bindings)).  Argument order and
 * meaning follow the reference function that each entry point cites; torch.Tensor arguments
 * become raw device pointers, and one trailing `stream` (hipStream_t, may be NULL = default
 * stream) replaces the reference's implicit torch.cuda.current_stream() lookup
 * (cuda_core_backend/kinematics.py:50-51).
 *
 * Contract (same as the reference):
 *   - the caller owns all memory; every output is pre-allocated and mutated in place;
 *   - no allocation, no host synchronisation and no host read of device data happens inside a
 *     launch, so every entry point is hipGraph-capturable;
 *   - tensors are contiguous, fp32 unless stated; index tables int16 / int8 / int32 / uint8;
 *   - return value: 0 on success, non-zero on error; curobo_hip_last_error() returns a
 *     thread-local message (the reference raises via log_and_raise; the Python shim in
 *     curobo_amd/backends converts the status to the same exception types).
 */
#ifndef CUROBO_HIP_H
#define CUROBO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *curobo_hip_stream_t; /* hipStream_t */

#define CUROBO_HIP_OK 0
#define CUROBO_HIP_ERR_INVALID 1 /* bad argument (reference: ValueError / RuntimeError) */
#define CUROBO_HIP_ERR_LAUNCH 2  /* hipGetLastError() != hipSuccess after a launch */

const char *curobo_hip_last_error(void);
/* ABI version of this header; bumped on any signature change.  2 = round 2 (new arguments on the extension entry
 * points: fused rollouts, seed IK, dense self collision, the L-BFGS iteration tail; the reference-shaped entry points are
 * unchanged). */
int curobo_hip_abi_version(void);
/* when non-zero every launch is followed by hipStreamSynchronize + error check
 * (reference runtime.debug, cuda_core_backend/launch_helper.py:13-19). */
void curobo_hip_set_debug_sync(int enabled);

/* ---------------------------------------------------------------- kinematics
 * reference: cuda_core_backend/kinematics.py:21-379, pybind/kinematics_bindings.cpp:128-237
 * kernels:   kernels/kinematics/kinematics_forward_kernel.cuh:20-433,
 *            kernels/kinematics/kinematics_backward_kernel.cuh:27-157
 * batch_size is the number of points N = batch * horizon (cuda_ops/kinematics.py:113).
 */
/* replaces launch_kinematics_forward (cuda_core_backend/kinematics.py:21-88) */
int curobo_hip_launch_kinematics_forward(
    float *link_pos, float *link_quat, float *batch_center_of_mass, float *global_cumul_mat,
    const float *joint_vec, const float *fixed_transform, const float *link_masses_com,
    const int8_t *joint_map_type, const int16_t *joint_map, const int16_t *link_map,
    const int16_t *tool_frame_map, const float *joint_offset_map, int batch_size, int horizon,
    int n_joints, int num_links, int n_tool_frames, int compute_com, curobo_hip_stream_t stream);

/* replaces launch_kinematics_forward_spheres (cuda_core_backend/kinematics.py:91-190) */
int curobo_hip_launch_kinematics_forward_spheres(
    float *link_pos, float *link_quat, float *batch_robot_spheres, float *batch_center_of_mass,
    float *global_cumul_mat, const float *joint_vec, const float *fixed_transform,
    const float *robot_spheres, const float *link_masses_com, const int8_t *joint_map_type,
    const int16_t *joint_map, const int16_t *link_map, const int16_t *tool_frame_map,
    const int16_t *link_sphere_map, const float *joint_offset_map, const int32_t *env_query_idx,
    int num_envs, int batch_size, int horizon, int n_joints, int num_spheres, int num_links,
    int n_tool_frames, int write_global_cumul, int compute_com, curobo_hip_stream_t stream);

/* replaces launch_kinematics_forward_spheres_jacobian (cuda_core_backend/kinematics.py:193-300) */
int curobo_hip_launch_kinematics_forward_spheres_jacobian(
    float *link_pos, float *link_quat, float *batch_robot_spheres, float *batch_center_of_mass,
    float *batch_jacobian, float *global_cumul_mat, const float *joint_vec,
    const float *fixed_transform, const float *robot_spheres, const float *link_masses_com,
    const int8_t *joint_map_type, const int16_t *joint_map, const int16_t *link_map,
    const int16_t *tool_frame_map, const int16_t *link_sphere_map, const int16_t *link_chain_data,
    const int16_t *link_chain_offsets, const int16_t *joint_links_data,
    const int16_t *joint_links_offsets, const uint8_t *joint_affects_endeffector,
    const float *joint_offset_map, const int32_t *env_query_idx, int num_envs, int batch_size,
    int horizon, int n_joints, int num_spheres, int num_links, int n_tool_frames,
    int write_global_cumul, int compute_com, curobo_hip_stream_t stream);

/* replaces launch_kinematics_backward (cuda_core_backend/kinematics.py:303-379).
 * grad_spheres_b (extension, may be NULL): a second sphere-gradient buffer that is added to
 * grad_spheres on the fly, so the self-collision and scene-collision gradient buffers can be
 * consumed without a separate elementwise add.  link_chain_len = number of entries of
 * link_chain_data (link_chain_data.shape[0] in the reference).  compute_jacobian_grad != 0 is rejected
 * (CUROBO_HIP_ERR_INVALID): the dJ/dq term is a SURVEY section 8f-2 "next" row. */
int curobo_hip_launch_kinematics_backward(
    float *grad_out, const float *grad_nlinks_pos, const float *grad_nlinks_quat,
    const float *grad_spheres, const float *grad_spheres_b, const float *grad_center_of_mass,
    const float *batch_center_of_mass, const float *grad_jacobian, const float *global_cumul_mat,
    const float *robot_spheres, const float *link_masses_com, const int16_t *link_map,
    const int16_t *joint_map, const int8_t *joint_map_type, const int16_t *tool_frame_map,
    const int16_t *link_sphere_map, const int16_t *link_chain_data,
    const int16_t *link_chain_offsets, const int16_t *joint_links_data,
    const int16_t *joint_links_offsets, const uint8_t *joint_affects_endeffector,
    const float *joint_offset_map, const int32_t *env_query_idx, int num_envs, int batch_size,
    int horizon, int n_joints, int num_spheres, int num_links, int n_tool_frames, int link_chain_len,
    int compute_com, int compute_jacobian_grad, curobo_hip_stream_t stream);

/* ---------------------------------------------------------------- geometry: self collision
 * reference: cuda_core_backend/geometry.py:63-227, pybind/geometry_bindings.cpp:16-45
 * kernels:   kernels/geometry/self_collision/self_collision_kernel.cuh:19-297
 * num_blocks_per_batch / max_threads_per_block are accepted for signature parity; the HIP
 * backend picks its own wave64 tiling (block_batch_max_* scratch is used when it splits the
 * pair list across workgroups).
 */
int curobo_hip_self_collision_distance(
    float *out_distance, float *out_vec, float *pair_distance, uint8_t *sparse_index,
    const float *robot_spheres, const float *sphere_padding, const float *weight,
    const int16_t *pair_locations, float *block_batch_max_value, int16_t *block_batch_max_index,
    int num_blocks_per_batch, int max_threads_per_block, int batch_size, int horizon, int nspheres,
    int num_collision_pairs, int store_pair_distance, int compute_grad,
    curobo_hip_stream_t stream);

/* Dense pair sets (humanoids: most of the S (S - 1) / 2 sphere pairs are enabled): the same result as
 * curobo_hip_self_collision_distance without store_pair_distance, from a register-tiled all-pairs pass masked by a
 * bitmap of the pair set instead of a gather per listed pair.  pair_bitmap: uint32 [2 * nslots][nslots * 64], bit jj
 * of pair_bitmap[jb][i] <-> pair (i, 32 * jb + jj) of pair_locations (i < j; the list must be (i, j)-sorted so
 * that "lowest pair index" = lexicographically first pair); nslots = multiple of 4 with nslots * 64 >= nspheres.
 * reference: self_collision_max_block_kernel + _max_reduce_kernel, self_collision_kernel.cuh:113-297.
 * tile_list (optional, NULL = evaluate every tile): the 16 x 16 tiles of the pair matrix that hold an enabled pair, as
 * (i / 16) | (j / 16) << 8; with it a tile is only evaluated when the bounding boxes of its two 16-sphere blocks overlap
 * (result preserving: only positive penetrations count).
 * With a tile list the narrow phase runs on the matrix cores: one v_mfma_f32_16x16x4_f32 per surviving tile gives all 256
 * penetrations of the tile in the expanded form 2 c_i.c_j + 2 r_i r_j + (r_i^2 - |c_i|^2) + (r_j^2 - |c_j|^2); that value
 * only culls, the listed pairs it leaves are evaluated again exactly (same bits as the other kernels).
 * tile_lane_masks (ABI 6, optional, NULL = read the pair bitmap instead): uint8 [num_tiles][64], bit reg of byte (c, lane)
 * <-> pair (16 ib + 4 (lane / 16) + reg, 16 jb + lane % 16) of tile c is listed: the tile's pair set in the layout in which
 * a lane receives the matrix-core result, 64 bytes per tile instead of 1 KB of bitmap words. */
int curobo_hip_self_collision_distance_dense(
    float *out_distance, float *out_vec, uint8_t *sparse_index, const float *robot_spheres,
    const float *sphere_padding, const float *weight, const uint32_t *pair_bitmap, const int32_t *tile_list, int num_tiles,
    const uint8_t *tile_lane_masks, int batch_size, int horizon, int nspheres, int nslots, int compute_grad,
    curobo_hip_stream_t stream);

/* Link-pair sweep (the self-collision matrix builder; reference RobotBuilder._prune_collision_pairs,
 * robot/builder/builder_robot.py:1054-1172, without its [N, P] pair_distance buffer): robot_spheres [n_points, nspheres, 4]
 * in the world frame, pair_locations [num_pairs, 2] sorted so that every group -- pair_group [num_pairs] in [0, n_groups),
 * one link pair -- is one contiguous run.  Per group g:
 *   max_penetration[g] = max over the points and the group's valid pairs of (r_i + pad_i) + (r_j + pad_j) - |c_i - c_j|
 *                        (metres, signed; a pair is valid when both padded radii are >= 0; -inf without a valid pair)
 *   collision_count[g] = number of points at which some valid pair of the group has penetration > 0
 * accumulate != 0: folded into what the two outputs hold (max / sum) instead of replacing it.
 * partial_max / partial_count: scratch [partial_chunks, n_groups], partial_chunks >= ceil(n_points / points_per_workgroup).
 * No floating-point atomics; the result is bit-identical from run to run and for every points_per_workgroup.
 * nspheres <= 1024, n_groups <= 4096 (LDS: 16 nspheres + 12 n_groups bytes <= 64 KiB); robot_spheres, pair_locations and
 * pair_group 16-byte aligned. */
int curobo_hip_link_pair_sweep(
    float *max_penetration, int32_t *collision_count, float *partial_max, int32_t *partial_count, int partial_chunks,
    const float *robot_spheres, const float *sphere_padding, const int16_t *pair_locations, const int32_t *pair_group,
    int n_points, int nspheres, int num_pairs, int n_groups, int points_per_workgroup, int accumulate,
    curobo_hip_stream_t stream);

/* ---------------------------------------------------------------- collision: sphere vs scene
 * The reference has NO backend hook here: these are NVIDIA Warp kernels launched from
 * geom/collision/wp_autograd.py:37-249 (SphereObstacleCollision / SweptSphereObstacleCollision).
 * The struct mirrors CuboidDataWarp (geom/data/data_cuboid.py:43-62) and VoxelDataWarp
 * (geom/data/data_voxel.py:684-702).  One launch handles every obstacle type, sums the
 * obstacles of a sphere in index order (deterministic; the reference uses float atomics) and
 * fully rewrites distance/gradient (no separate zero_() pass).
 */
typedef struct curobo_hip_scene {
  const float *cuboid_dims;       /* [num_envs, max_cuboids, 4] full extents */
  const float *cuboid_inv_pose;   /* [num_envs, max_cuboids, 8] x y z qw qx qy qz pad */
  const uint8_t *cuboid_enable;   /* [num_envs, max_cuboids] */
  const int32_t *cuboid_count;    /* [num_envs] */
  int32_t max_cuboids;
  const float *voxel_params;      /* [num_envs, max_voxel_grids, 4] nx ny nz voxel_size */
  const float *voxel_inv_pose;    /* [num_envs, max_voxel_grids, 8] */
  const uint8_t *voxel_enable;    /* [num_envs, max_voxel_grids] */
  const int32_t *voxel_count;     /* [num_envs] */
  const uint16_t *voxel_features; /* fp16 ESDF [num_envs, max_voxel_grids, n_voxels] */
  int32_t max_voxel_grids;
  int32_t voxel_n_voxels;
  float voxel_max_distance;
  /* optional culling aid built at scene upload (NULL = none; results are identical with and without it):
   * fp16 [num_envs, max_voxel_grids, voxel_n_coarse], cell (cx, cy, cz) of a grid = the MINIMUM of its ESDF over
   * the block of voxel_coarse_block^3 voxels starting at (cx, cy, cz) * voxel_coarse_block, dilated by
   * voxel_coarse_dilate voxels on every side; row-major over (ceil(nx / block), ceil(ny / block), ceil(nz / block)).
   * A sphere whose whole sweep stays (voxel_coarse_dilate - 1) voxels around its centre's voxel and whose radius +
   * activation distance is below that minimum cannot touch the grid: its 8-corner lookups are skipped. */
  const uint16_t *voxel_coarse_min;
  int32_t voxel_coarse_block;
  int32_t voxel_coarse_dilate;
  int32_t voxel_n_coarse;
  /* Analytic primitives (beyond the reference, which turns Sphere / Capsule / Cylinder obstacles into meshes,
   * geom/types.py:1104-1124): a record of the cuboid store is a primitive when cuboid_dims[..., 3] (the reference's
   * zero padding) holds a tag: 1 sphere (dims = radius, -, -), 2 capsule (radius, half length of the segment on the
   * local z axis, -), 3 cylinder (radius, half height along local z, -); pose / enable / count as for cuboids.  Set
   * cuboid_has_primitives when any tag is non-zero (selects the kernel instantiations that test the tag). */
  int32_t cuboid_has_primitives;
} curobo_hip_scene;

/* sweep_steps: 0 = SphereObstacleCollision, 3 = SweptSphereObstacleCollision (SWEEP_STEPS,
 * wp_sweep_collision_kernel.py:66).  enable_speed_metric applies wp_speed_metric.py:10-93 in
 * the same launch; speed_dt is the reference's 1-element device tensor (may be NULL if off). */
int curobo_hip_sphere_obstacle_collision(
    float *distance, float *gradient, const float *spheres, const curobo_hip_scene *scene,
    const float *weight, const float *activation_distance, const int32_t *env_query_idx,
    int batch_size, int horizon, int num_spheres, int use_multi_env, int sweep_steps,
    int enable_speed_metric, const float *speed_dt, curobo_hip_stream_t stream);

/* The kernel form curobo_hip_sphere_obstacle_collision runs for these arguments (host-side, no GPU work; `scene` is the
 * host struct, only its capacities are read; -1 for arguments the launch would refuse).  All forms give the same
 * results bit for bit:
 *   INLANE        one lane per sphere walks the obstacles, records read from global memory (the staged records of the
 *                 batch rows a 256-sphere workgroup can touch would exceed 32 KiB of LDS: small horizon * spheres);
 *   INLANE_STAGED the same loop over records staged in LDS;
 *   PACKED        scenes with voxel grids and at most 32 records: early rejects first, the surviving (sphere, obstacle)
 *                 items evaluated densely from an LDS queue. */
#define CUROBO_HIP_SCENE_FORM_INLANE 0
#define CUROBO_HIP_SCENE_FORM_INLANE_STAGED 1
#define CUROBO_HIP_SCENE_FORM_PACKED 2
int curobo_hip_scene_collision_form(const curobo_hip_scene *scene, int batch_size, int horizon, int num_spheres,
                                    int sweep_steps);

/* Mesh obstacles -> one more ESDF grid of the voxel store (scene-upload time, not the hot path).  The reference
 * queries meshes through NVIDIA Warp's BVH (geom/data/data_mesh.py:555-700, wp.mesh_query_point); here a closed,
 * consistently oriented triangle mesh is baked into an fp16 grid [nx, ny, nz] (voxel centres
 * (i + 0.5 - n / 2) * voxel_size in the grid frame, the layout of geom/data/data_voxel.py:42-95): exact
 * point-triangle distance, sign from the generalised winding number, clamped to +-max_distance.
 * vertices [n_vertices, 3] (mesh frame) and faces int32 [n_faces, 3] are device pointers; grid_to_mesh_3x4_host is a
 * HOST pointer to the row-major 3x4 transform grid frame -> mesh frame. */
int curobo_hip_mesh_esdf_bake(uint16_t *out_esdf_fp16, const float *vertices, const int32_t *faces, int n_vertices,
                              int n_faces, int nx, int ny, int nz, float voxel_size, float max_distance,
                              const float *grid_to_mesh_3x4_host, curobo_hip_stream_t stream);

/* Triangle-mesh obstacles queried directly (the reference: geom/data/data_mesh.py:555-700, wp.mesh_query_point per query
 * sphere through NVIDIA Warp's BVH).  A mesh is a linear BVH in heap layout: triangles sorted by the Morton code of their
 * centroids, `leaf_size` consecutive triangles per leaf, `n_leaves` (a power of two) leaves, node k has the children 2k and
 * 2k + 1, the leaves are the nodes n_leaves .. 2 n_leaves - 1.  tri: [n_tri][12] floats = (a, b - a, c - a) as float4 each,
 * in sorted order; node_box: [2 * n_leaves][8] floats = (lo xyz, -, hi xyz, -), node 0 unused.  All device pointers. */
typedef struct curobo_hip_mesh {
  const float *tri;
  const float *node_box;
  /* optional (ABI 5): [n_tri][6][4] floats in the sorted triangle order = the angle-weighted pseudonormals of the triangle's
   * vertices a, b, c and the edge pseudonormals of ab, bc, ca (sum of the normals of the faces that share the feature;
   * Baerentzen & Aanaes 2005).  The sign of a query whose closest point lies on an edge or a vertex is the sign of
   * (point - closest) . pseudonormal; NULL = count ray crossings instead (three tree walks per such query). */
  const float *tri_pn;
  int32_t n_tri, n_leaves, leaf_size;
  /* ABI 7 (was padding = 0).  How inside / outside is decided:
   *   0 = by the closest feature (face normal / pseudonormal; crossings counted when that gives no verdict): the same function
   *       as the reference's rule on a closed, consistently oriented surface, without a ray;
   *   1 = the reference's rule as published -- Warp's mesh_query_point -> mesh_query_inside (warp/native/mesh.h; called from
   *       data_mesh.py:632,682): rays from the query point along +x, +y, +z, inside iff all three hit and every ray's NEAREST
   *       hit is a back face.  The rule for meshes that are open or not consistently oriented, where the two differ. */
  int32_t sign_rule;
  /* ABI 7, optional: distance-sorted closest-triangle cell lists over a uniform grid in the mesh frame (NULL = every query
   * walks the tree).  The grid covers the bounding box grown by grid_pad, cells of edge grid_h, cell (ix, iy, iz) has the
   * index (ix * grid_n[1] + iy) * grid_n[2] + iz.  cell_start [n_cells + 1][2]: word 0: bits 0..29 = first entry of the cell's list in
   * cell_list, bits 30..31 = 1 / 2 when every point of the cell is outside / inside the surface (sign_rule 0 only), else 0;
   * word 1: the distance of the cell's centre from the surface (float bits).
   * cell_list: 16-byte entries (int32 triangle index in sorted order, float distance of that triangle from the CELL CENTRE c,
   * two floats = the octahedral code of the unit vector n from the triangle's closest point towards c), ascending in distance,
   * closed by a sentinel (-1, cover, 0, 0): every triangle not listed is farther than `cover` from the centre.  A query point p
   * at distance delta from its cell's centre goes through the list in order: an entry needs its triangle tested only when its
   * bound distance + (p - c) . n (the triangle lies behind the plane through its closest point with normal n) does not exceed
   * the best distance found; the query stops at the first entry whose distance - delta exceeds it (every later triangle is
   * farther still: the result is the exact closest point); a list that ends before that (best > cover - delta) sends the query
   * to the tree walk. */
  const uint32_t *cell_start;
  const int32_t *cell_list;
  float grid_lo[3], grid_h;
  int32_t grid_n[3];
  float grid_pad;
} curobo_hip_mesh;

/* The mesh obstacles of a scene (layout of the reference's MeshData, data_mesh.py:60-120): meshes = DEVICE array of
 * curobo_hip_mesh (the cache of loaded meshes), mesh_id [num_envs, max_n] picks one per obstacle slot, dims [num_envs,
 * max_n, 4] = bounding-box extents (the query's max_distance is half their diagonal), inv_pose / enable / count as for
 * cuboids.  gradient_mode 0: the local gradient exactly as data_mesh.py:693-697 computes it, (p - closest) / |p - closest|
 * on either side of the surface; 1: that vector negated for centres outside the surface, i.e. minus the gradient of the
 * signed distance everywhere, which is what the cuboid (data_cuboid.py:596-626) and voxel kinds hand to the same kernel. */
/* some mesh of the set carries cell lists: the queued launch answers what it can through them before it walks trees */
#define CUROBO_HIP_MESH_SET_HAS_CELLS 1
typedef struct curobo_hip_mesh_set {
  const curobo_hip_mesh *meshes;
  const int32_t *mesh_id;
  const float *dims;
  const float *inv_pose;
  const uint8_t *enable;
  const int32_t *count;
  int32_t max_n, gradient_mode;
  int32_t num_envs;        /* leading dimension of mesh_id / dims / inv_pose / enable / count (ABI 5) */
  int32_t flags;           /* ABI 7 (was padding = 0): CUROBO_HIP_MESH_SET_HAS_CELLS */
} curobo_hip_mesh_set;

/* Build: (1) Morton keys of the triangle centroids inside bounds_lo_hi_host (HOST pointer, 6 floats: the mesh's bounding
 * box) -> out_codes [n_faces] int64 = code << 32 | triangle index; (2) the caller sorts the keys (any sort: they are
 * unique); (3) triangles in sorted order + leaf boxes + one launch per level of the tree for the inner boxes.  out_tri
 * [n_faces * 12], out_node_box [2 * n_leaves * 8] floats. */
int curobo_hip_mesh_morton_codes(int64_t *out_codes, const float *vertices, const int32_t *faces, int n_faces,
                                 const float *bounds_lo_hi_host, curobo_hip_stream_t stream);
int curobo_hip_mesh_bvh_build(float *out_tri, float *out_node_box, const float *vertices, const int32_t *faces,
                              const int64_t *sorted_codes, int n_faces, int n_leaves, int leaf_size,
                              curobo_hip_stream_t stream);

/* The cell lists of a mesh (curobo_hip_mesh.cell_start / cell_list), in two launches around the caller's prefix sum and sort
 * (plumbing, as for the Morton keys).  `mesh` (HOST pointer) carries the tree and the grid fields; its cell pointers are not
 * read.  (1) count: per cell the length of its list including the sentinel -> out_count [n_cells], its cover radius ->
 * out_cover [n_cells] (0 = the cell has no list: more than gather_cap triangles about equally far), the side of the whole
 * cell -> out_side [n_cells] (1 outside / 2 inside / 0 may straddle), the distance of its centre from the surface ->
 * out_centre_dist [n_cells].  (2) fill, given offsets [n_cells + 1] = the exclusive
 * prefix sum of out_count as int64: out_entries [offsets[n_cells]][4] = (triangle, distance bits, direction code x, y), unsorted within a cell,
 * out_keys [offsets[n_cells]] = cell << 32 | distance bits (sentinel: 0x7fffffff), out_cell_start [n_cells + 1][2] = the packed
 * words of curobo_hip_mesh.cell_start.  The caller sorts the keys and gathers the entries with the permutation. */
int curobo_hip_mesh_cells_count(int32_t *out_count, float *out_cover, uint8_t *out_side, float *out_centre_dist,
                                const curobo_hip_mesh *mesh, int gather_cap, curobo_hip_stream_t stream);
int curobo_hip_mesh_cells_fill(int64_t *out_keys, int32_t *out_entries, uint32_t *out_cell_start, const int64_t *offsets,
                               const float *cover, const uint8_t *side, const float *centre_dist,
                               const curobo_hip_mesh *mesh, curobo_hip_stream_t stream);

/* compute_local_sdf_with_grad of data_mesh.py:630-700 for points [n, 3] in the mesh frame: out_sdf [n] = signed distance
 * (negative inside; max_distance when no surface lies within max_distance), out_grad [n, 3] (may be NULL) = (point -
 * closest point) / distance.  Exact point-triangle distances; the sign is the parity of ray crossings (closed meshes). */
int curobo_hip_mesh_query(float *out_sdf, float *out_grad, const float *points, const curobo_hip_mesh *mesh,
                          float max_distance, int n_points, curobo_hip_stream_t stream);

/* curobo_hip_mesh_esdf_bake through the BVH: O(voxels x log triangles) instead of O(voxels x triangles). */
int curobo_hip_mesh_esdf_bake_bvh(uint16_t *out_esdf_fp16, const curobo_hip_mesh *mesh, int nx, int ny, int nz,
                                  float voxel_size, float max_distance, const float *grid_to_mesh_3x4_host,
                                  curobo_hip_stream_t stream);

/* Sphere-vs-mesh collision: the mesh share of SphereObstacleCollision / SweptSphereObstacleCollision.forward
 * (geom/collision/wp_autograd.py:37-249 launches its kernel once per obstacle kind into the same buffers; this is the
 * launch for the mesh kind).  accumulate != 0: add to distance / gradient as written by curobo_hip_sphere_obstacle_collision
 * for the other kinds (the speed metric is applied to this share: it is linear); 0: overwrite them. */
int curobo_hip_sphere_mesh_collision(
    float *distance, float *gradient, const float *spheres, const curobo_hip_mesh_set *meshes, const float *weight,
    const float *activation_distance, const int32_t *env_query_idx, int batch_size, int horizon, int num_spheres,
    int use_multi_env, int sweep_steps, int enable_speed_metric, const float *speed_dt, int accumulate,
    curobo_hip_stream_t stream);

/* The same launch with a caller-owned device workspace (>= curobo_hip_sphere_mesh_collision_ws_bytes(...) bytes, 16-byte
 * aligned, contents irrelevant; the size is written to the HOST pointer out_bytes_host): the spheres that survive the bounding-box reject of any mesh -- few, and clustered in the
 * batch -- are queued launch-wide and their tree walks run on a grid that covers the chip once, instead of inside the
 * workgroups that happen to hold them.  Same results (per sphere the slots are summed in ascending order in both forms);
 * kernels only on `stream` (since the end of round 6 the queue counters -- the first 16 bytes: spheres queued from the head,
 * handed to the tree walk, queued from the tail, handed to a workgroup of their own -- are cleared by a kernel: a captured
 * 16-byte memset node faulted at the second replay of its graph), graph-capturable: counter reset, select, and with cell lists
 * the cell-list kernel, the workgroup-per-sphere kernel and the tree walk of what is left. */
int curobo_hip_sphere_mesh_collision_ws_bytes(int batch_size, int horizon, int num_spheres, int64_t *out_bytes_host);
int curobo_hip_sphere_mesh_collision_ws(
    float *distance, float *gradient, const float *spheres, const curobo_hip_mesh_set *meshes, const float *weight,
    const float *activation_distance, const int32_t *env_query_idx, int batch_size, int horizon, int num_spheres,
    int use_multi_env, int sweep_steps, int enable_speed_metric, const float *speed_dt, int accumulate, void *workspace,
    size_t workspace_bytes, curobo_hip_stream_t stream);

/* ---------------------------------------------------------------- cost: tool pose + c-space
 * The reference runs these as NVIDIA Warp kernels without a backend hook:
 * ToolPoseDistance (cost/wp_tool_pose.py:698-914, kernel :456-692) and the POSITION c-space cost
 * (cost/wp_cspace_position.py:232-362).  Argument order follows the Warp kernels' inputs.
 * goal_position/goal_quat: [n_goals, num_links, num_goalset, 3|4] (quaternions wxyz);
 * out_distance [b,h,2*num_links] = (position cost, rotation cost) per link; out_rotation_gradient
 * is the quaternion rate q (x) (omega,0) (wxyz) that launch_kinematics_backward consumes.
 * rotation_method: 0 axis-angle, 1 lie group, 2 lie group advanced. */
int curobo_hip_tool_pose_distance(
    float *out_distance, float *out_position_distance, float *out_rotation_distance,
    float *out_position_gradient, float *out_rotation_gradient, int32_t *out_goalset_idx,
    const float *current_position, const float *current_quat, const float *goal_position,
    const float *goal_quat, const int32_t *idxs_goal, const float *position_orientation_weight,
    const float *terminal_pose_axes_weight_factor, const float *non_terminal_pose_axes_weight_factor,
    const float *terminal_pose_convergence_tolerance,
    const float *non_terminal_pose_convergence_tolerance, const uint8_t *project_distance_to_goal,
    int batch_size, int horizon, int num_links, int num_goalset, int rotation_method,
    curobo_hip_stream_t stream);

/* p_b/effort_b/v_b: [2, dof] lower then upper; weight/activation_distance: [2] (position,
 * effort); squared_l2_reg_weight: [2] (velocity, acceleration); effort / out_grad_tau may be NULL. */
int curobo_hip_cspace_position_cost(
    float *out_cost, float *out_grad_p, float *out_grad_tau, const float *pos, const float *effort,
    const float *cspace_target, const int32_t *cspace_target_idx, const float *p_b,
    const float *effort_b, const float *weight, const float *activation_distance,
    const float *cspace_target_weight, const float *cspace_target_dof_weight,
    const float *squared_l2_reg_weight, const float *current_position,
    const float *current_velocity, const int32_t *idxs_current_state, const float *v_b,
    const float *state_dt, int write_grad, int batch_size, int horizon, int dof,
    curobo_hip_stream_t stream);

/* c-space STATE cost (reference cost/wp_cspace_state.py:20-287, a Warp kernel): bound costs on
 * position / velocity / acceleration / jerk / effort, optional joint target, squared-L2 and
 * energy regularisation.  weight, activation_distance, squared_l2_regularization_weights: [5];
 * limits [2, dof] each; state_dt [batch]; effort / out_grad_tau may be NULL. */
int curobo_hip_cspace_state_cost(
    float *out_cost, float *out_grad_p, float *out_grad_v, float *out_grad_a, float *out_grad_j,
    float *out_grad_tau, const float *pos, const float *vel, const float *acc, const float *jerk,
    const float *effort, const float *state_dt, const float *target_joint_position,
    const int32_t *idxs_target_joint_position, const float *p_b, const float *v_b,
    const float *a_b, const float *j_b, const float *effort_b, const float *weight,
    const float *activation_distance, const float *squared_l2_regularization_weights,
    const float *cspace_target_weight, const float *cspace_non_terminal_weight_factor,
    const float *cspace_target_dof_weight, int write_grad, int batch_size, int horizon, int dof,
    int retime_weights, int retime_regularization_weights, curobo_hip_stream_t stream);

/* Per-row aggregation for horizon-1 (teleport / IK) rollouts (reference: torch cat+sum and autograd
 * accumulation, rollout/metrics.py:233-265): out_cost[r] = sum(pose_cost[r,:2*num_links]) +
 * sum(cspace_cost[r,:dof]) + self_cost[r] + sum(scene_cost[r,:num_spheres]);
 * grad_q[r,:] += cspace_grad[r,:].  Any input may be NULL. */
int curobo_hip_rollout_point_aggregate(
    float *out_cost, float *grad_q, const float *pose_cost, const float *cspace_cost,
    const float *cspace_grad, const float *self_cost, const float *scene_cost, int rows,
    int num_links, int dof, int num_spheres, curobo_hip_stream_t stream);

/* The same with one more per-row term: out_cost[r] += extra_cost[r] (NULL = none), e.g. the support-polygon cost below. */
int curobo_hip_rollout_point_aggregate_terms(
    float *out_cost, float *grad_q, const float *pose_cost, const float *cspace_cost,
    const float *cspace_grad, const float *self_cost, const float *scene_cost, const float *extra_cost,
    int rows, int num_links, int dof, int num_spheres, curobo_hip_stream_t stream);

/* ---------------------------------------------------------------- support polygon (balance) cost
 * reference (torch ops, no backend hook): geom/convex_polygon_helper.py:63-336, cost/cost_support_polygon.py:35-109.
 *
 * convex_hull_2d: points [n_hulls, n_pts, 2] -> hulls [n_hulls, n_pts, 2], counts [n_hulls].  The strictly convex vertices
 * counter-clockwise from the lowest one (leftmost on a tie); a vertex whose turn is <= 1e-10 is dropped; every vertex then
 * moves by `padding` (> 0) along the unit vector from the vertex mean; rows past counts[i] repeat the last vertex.
 * 3 <= n_pts <= 64.
 *
 * support_polygon_cost: com [batch, horizon, 4] (xyz + total mass: the FK launches' centre-of-mass buffer), hulls
 * [n_hulls, max_vertices, 2], idxs_hull [batch] (row b -> hull), weight [1] -> cost [batch, horizon], grad_com
 * [batch, horizon, 4] (d cost / d com: xy filled, z and w zero, weight applied: what launch_kinematics_backward takes as
 * grad_center_of_mass) and, unless NULL, signed_distance [batch, horizon] (negative inside).  The distance is the
 * soft-min (softmax(-d / smoothing)) of the distances to the hull's edges.  counts NULL: all max_vertices rows form edges,
 * repeated rows included (the reference's padded tensor); else hull i uses its first counts[i] rows.
 * inside_cost_weight > 0: inside costs inside_cost_weight * max(margin_target + sd, 0), outside sd; else max(sd, 0).
 * cost_mode 1: cost = weight * sd and grad_com its gradient (the distance query of the reference's helper); 0: the cost.
 * max_vertices <= 32. */
int curobo_hip_convex_hull_2d(float *hulls, int32_t *counts, const float *points, float padding, int n_hulls,
                              int n_pts, curobo_hip_stream_t stream);

int curobo_hip_support_polygon_cost(float *cost, float *grad_com, float *signed_distance, const float *com,
                                    const float *hulls, const int32_t *counts, const int32_t *idxs_hull,
                                    const float *weight, float inside_cost_weight, float margin_target,
                                    float smoothing, int batch_size, int horizon, int n_hulls,
                                    int max_vertices, int cost_mode, curobo_hip_stream_t stream);

/* ---------------------------------------------------------------- dynamics: RNEA
 * reference: cuda_core_backend/dynamics.py:24-131,134-260
 * kernels:   kernels/dynamics/rnea_forward_kernel.cuh:53-292, rnea_backward_kernel.cuh:65-468
 * tau[b, num_dof] = RNEA(q, qd, qdd, f_ext); spatial vectors are [angular; linear], gravity[6] is
 * the spatial base acceleration (0,0,0,0,0,+9.81 for z-up gravity).  forward_cache is the
 * reference's opaque [batch, num_links*20] scratch handed from forward to backward (internal
 * layout here: [link][20][batch]).  level_starts / n_levels / threads_per_batch are accepted for
 * signature parity; links are visited in level_links order.  f_ext / grad_f_ext [b, links, 6]
 * may be NULL.  The backward needs a caller-owned workspace of num_links*18*batch floats (the
 * Python shim keeps one per device). */
int curobo_hip_launch_rnea_forward(
    float *tau, const float *q, const float *qd, const float *qdd, const float *fixed_transforms,
    const float *link_masses_com, const float *link_inertias, const int8_t *joint_map_type,
    const int16_t *joint_map, const int16_t *link_map, const float *joint_offset_map,
    const float *gravity, const int16_t *level_starts, const int16_t *level_links,
    float *forward_cache, int batch_size, int num_links, int num_dof, int n_levels,
    int threads_per_batch, const float *f_ext, curobo_hip_stream_t stream);

int curobo_hip_launch_rnea_backward(
    float *grad_q, float *grad_qd, float *grad_qdd, const float *grad_tau, const float *q,
    const float *qd, const float *fixed_transforms, const float *link_masses_com,
    const float *link_inertias, const int8_t *joint_map_type, const int16_t *joint_map,
    const int16_t *link_map, const float *joint_offset_map, const float *gravity,
    const int16_t *level_starts, const int16_t *level_links, const float *forward_cache,
    int batch_size, int num_links, int num_dof, int n_levels, int threads_per_batch,
    float *grad_f_ext, float *workspace, curobo_hip_stream_t stream);

/* Extensions: the same two launches with a caller-provided scratch of 3 * num_dof * batch_size floats.  The launch first
 * transposes its joint-space inputs (q, qd, qdd | grad_tau) into it, [dof][batch], and the walks read them from there:
 * coalesced without staging them through LDS (38 KB per workgroup for a 49-dof humanoid).  Same values as the launches
 * above; meant for rollouts that run the walks NEXT TO a kernel that lives on LDS (C4: the self-collision kernel holds
 * eight points per CU in 160 KB, and three while the staged walks share the CU).  flags bit 0: the scratch still holds q and qd of a
 * forward launch on the same inputs (its first two thirds): only grad_tau is transposed; bit 1: the gradients are ADDED to
 * grad_q / grad_qd / grad_qdd (the caller's running joint-space gradients) instead of overwriting them. */
int curobo_hip_launch_rnea_forward_scratch(
    float *tau, const float *q, const float *qd, const float *qdd, const float *fixed_transforms,
    const float *link_masses_com, const float *link_inertias, const int8_t *joint_map_type,
    const int16_t *joint_map, const int16_t *link_map, const float *joint_offset_map,
    const float *gravity, const int16_t *level_starts, const int16_t *level_links,
    float *forward_cache, int batch_size, int num_links, int num_dof, int n_levels,
    int threads_per_batch, const float *f_ext, float *scratch, curobo_hip_stream_t stream);

int curobo_hip_launch_rnea_backward_scratch(
    float *grad_q, float *grad_qd, float *grad_qdd, const float *grad_tau, const float *q,
    const float *qd, const float *fixed_transforms, const float *link_masses_com,
    const float *link_inertias, const int8_t *joint_map_type, const int16_t *joint_map,
    const int16_t *link_map, const float *joint_offset_map, const float *gravity,
    const int16_t *level_starts, const int16_t *level_links, const float *forward_cache,
    int batch_size, int num_links, int num_dof, int n_levels, int threads_per_batch,
    float *grad_f_ext, float *workspace, float *scratch, int flags, curobo_hip_stream_t stream);

/* ---------------------------------------------------------------- linalg: Levenberg-Marquardt step
 * reference: optim/util/levenberg_marquardt_step.py:96-199 (Warp tile kernel, no backend hook).
 * Per problem: delta = -(J^T J + lambda I)^-1 jTerror; joint_position_out = joint_position_in +
 * delta; pred_reduction = 0.5 * delta . (lambda * delta - jTerror).
 * jacobian [batch, n_residuals, action_dim], action_dim <= 64.  J^T J runs on the matrix cores
 * (v_mfma_f32_16x16x4_f32, exact fp32), the Cholesky solve in LDS, one wavefront per problem. */
int curobo_hip_levenberg_marquardt_step(
    float *joint_position_out, float *pred_reduction, const float *jacobian, const float *jTerror,
    const float *lambda_damping, const float *joint_position_in, int batch_size, int n_residuals,
    int action_dim, curobo_hip_stream_t stream);

/* c-space L2 distance cost (reference forward_l2_warp / L2DistFunction,
 * cost/wp_torch_cspace_dist.py:12-158): out_cost[b, h, d] = weight[0] * r[d] * (pos - target[target_idx[b]])^2
 * with r = terminal_dof_weight at h == horizon - 1, else non_terminal_dof_weight [dof]; out_grad_p =
 * 2 w err.  Entries of zero weight are left untouched, as in the reference. */
int curobo_hip_cspace_l2_distance(float *out_cost, float *out_grad_p, const float *pos, const float *target,
                                  const int32_t *target_idx, const float *weight,
                                  const float *terminal_dof_weight, const float *non_terminal_dof_weight,
                                  int write_grad, int batch_size, int horizon, int dof,
                                  curobo_hip_stream_t stream);

/* ---------------------------------------------------------------- seed IK: iteration-state update
 * reference (torch elementwise ops, ~25 launches per iteration):
 *   solver/seed_ik/seed_ik_error_calculator.py:292-305,338-387,464-495 (pose-error reduction,
 *   joint-limit residual rows, combination) and solver/seed_ik/seed_iteration_state_manager.py:74-260
 *   (trust ratio rho = (old - new) / (pred + 1e-8), accept rho >= rho_min, lambda /= or *= factor
 *   clamped, candidate-or-current selection, convergence flags).
 * State [n, ...] is updated in place from the candidate evaluation: candidate_pose_jacobian
 * [n, 6T, dof] (FK Jacobian kernel), candidate_pose_jTerror [n, dof] (FK VJP of the pose cost),
 * candidate_pose_cost [n, T, 2], candidate_{position,rotation}_distance [n, T] (tool-pose kernel),
 * predicted_reduction [n] (LM step).  jacobian [n, 6T + dof, dof] gets the pose rows and the
 * diagonal joint-limit rows; error_norm always takes the candidate's value (as the reference does).
 * initial != 0: the candidate becomes the state unconditionally (lambda is left as set by the
 * caller).  current_position / dt / velocity_limits [2, dof] (optional, all or none) tighten the
 * limits for velocity-aware IK.  * velocity / acceleration regularisation rows (seed_ik_error_calculator.py:389-456): with current_position + dt given,
 * velocity_weight > 0 adds r_v = sqrt(w dt) (q - current_position) / dt and acceleration_weight > 0 (current_velocity
 * given) r_a = sqrt(w) ((q - current_position) / dt - current_velocity); velocity_limits may be NULL (no clamping).
 */
int curobo_hip_seed_ik_update_state(
    float *joint_position, float *jacobian, float *jTerror, float *error_norm, float *position_error,
    float *orientation_error, float *lambda_damping, uint8_t *success, uint8_t *improvement,
    const float *candidate_joint_position, const float *candidate_pose_jacobian,
    const float *candidate_pose_jTerror, const float *candidate_pose_cost,
    const float *candidate_position_distance, const float *candidate_rotation_distance,
    const float *predicted_reduction, const float *action_min, const float *action_max,
    const float *current_position, const float *dt, const float *velocity_limits,
    const float *current_velocity, float velocity_weight, float acceleration_weight,
    float joint_limit_weight, float rho_min, float lambda_factor, float lambda_min, float lambda_max,
    float convergence_position_tolerance, float convergence_orientation_tolerance,
    float convergence_joint_limit_weight, int num_problems, int dof, int num_tool_frames,
    int initial, curobo_hip_stream_t stream);

/* `iterations` whole Levenberg-Marquardt iterations of the seed-IK solver (LM step -> FK + tool-frame Jacobian ->
 * tool-pose error -> J^T e -> curobo_hip_seed_ik_update_state) in ONE launch, preceded by the initial evaluation of
 * seed_joint_position when `initial` != 0: a problem lives on one 16-lane row with its state in LDS, global memory sees
 * the state (the buffers of curobo_hip_seed_ik_update_state) on the way in and on the way out.  Replaces
 * 5 x iterations launches of curobo_hip_levenberg_marquardt_step, curobo_hip_launch_kinematics_forward_spheres_jacobian,
 * curobo_hip_tool_pose_distance, curobo_hip_launch_kinematics_backward, curobo_hip_seed_ik_update_state (reference:
 * solver/seed_ik/seed_ik_solver.py:48-824, one torch graph per inner loop).  dof <= 16.  Goal / weight pointers as in
 * curobo_hip_tool_pose_distance (horizon 1: terminal weights and tolerances). */
int curobo_hip_seed_ik_iterate(
    float *joint_position, float *jacobian, float *jTerror, float *error_norm, float *position_error,
    float *orientation_error, float *lambda_damping, uint8_t *success, uint8_t *improvement, const float *seed_joint_position,
    const float *goal_position, const float *goal_quat, const int32_t *idxs_goal, const float *position_orientation_weight,
    const float *pose_axes_weight_factor, const float *pose_convergence_tolerance, const uint8_t *project_distance_to_goal,
    int num_goalset, int rotation_method, const float *fixed_transform, const int8_t *joint_map_type, const int16_t *joint_map,
    const int16_t *link_map, const int16_t *tool_frame_map, const int16_t *link_chain_data, const int16_t *link_chain_offsets,
    const int16_t *joint_links_data, const int16_t *joint_links_offsets, const uint8_t *joint_affects_endeffector,
    const float *joint_offset_map, const float *action_min, const float *action_max, const float *current_position,
    const float *dt, const float *velocity_limits, const float *current_velocity, float velocity_weight,
    float acceleration_weight, float joint_limit_weight, float rho_min, float lambda_factor, float lambda_min,
    float lambda_max, float convergence_position_tolerance, float convergence_orientation_tolerance,
    float convergence_joint_limit_weight, int num_problems, int dof, int num_links, int num_tool_frames, int link_chain_len,
    int iterations, int initial, const int32_t *stop_flag, int32_t *blocks_run, curobo_hip_stream_t stream);

/* 1 when the per-problem state of curobo_hip_seed_ik_iterate (16 problems per workgroup: accepted / candidate Jacobian,
 * normal matrix, the candidate's link transforms, pose scratch) fits the launch's 64 KB of LDS and dof <= 16, else 0: the
 * caller then runs the five-launch iteration (curobo_hip_levenberg_marquardt_step ... curobo_hip_seed_ik_update_state).
 * Returns the answer itself, not a status (like curobo_hip_rollout_trajopt_fused_torque_fits). */
int curobo_hip_seed_ik_iterate_fits(int dof, int num_links, int num_tool_frames, int link_chain_len);

/* Device-side early exit of the seed-IK solver (reference _calculate_exit_condition, seed_ik_solver.py:452-468): sets
 * *stop_flag = 1 when at least `needed` of the num_problems problems have a converged seed in success [P, S].  Launches of
 * curobo_hip_seed_ik_iterate that are given the flag (optional, NULL = always run) return at once when it is set and count
 * themselves in *blocks_run otherwise, so the host can enqueue every block of iterations without a round trip. */
int curobo_hip_seed_ik_batch_status(const uint8_t *success, int num_problems, int num_seeds, int needed,
                                    int32_t *stop_flag, curobo_hip_stream_t stream);

/* Ranking of the seeds of every problem in one launch (ties -> lower seed index: the order of a stable sort).
 * curobo_hip_seed_ik_select: reference SeedIKSolver._select_top_solutions (seed_ik_solver.py:522-572): success =
 * position / orientation error under the tolerances (and strictly inside the limits), cost = position + orientation
 * error (+ start_cspace_dist_weight |q - current_position|) + 1e10 for failures; the return_seeds best, best first.
 * curobo_hip_ik_rank: reference IKSolver._get_result (solver_ik.py:440-580): feasible = no self collision, no
 * joint-limit cost, no scene collision (scene_distance [P, S, num_scene_columns], NULL = no scene), success = feasible
 * and EVERY tool frame within the thresholds (position_distance / rotation_distance / goalset_idx [P, S, T]), ranked by
 * cost + 1e16 for failures; out_position_error / out_rotation_error [P, k] = the largest error over the tool frames,
 * out_goalset_index [P, k, T] (ABI 6: one column per tool frame, as the reference returns it).  num_seeds <= 1024. */
int curobo_hip_seed_ik_select(
    uint8_t *out_success, float *out_solution, float *out_position_error, float *out_orientation_error,
    const float *joint_position, const float *position_error, const float *orientation_error, const float *limit_lower,
    const float *limit_upper, const float *current_position, float position_tolerance, float orientation_tolerance,
    float start_cspace_dist_weight, int check_limits, int num_problems, int num_seeds, int dof, int return_seeds,
    curobo_hip_stream_t stream);
int curobo_hip_ik_rank(
    uint8_t *out_success, float *out_solution, float *out_position_error, float *out_rotation_error, float *out_cost,
    int64_t *out_seed_index, int64_t *out_goalset_index, const float *joint_position, const float *cost,
    const float *position_distance, const float *rotation_distance, const float *self_collision_distance,
    const float *cspace_cost, const float *scene_distance, const int32_t *goalset_idx, float position_threshold,
    float rotation_threshold, int num_problems, int num_seeds, int dof, int num_tool_frames, int num_scene_columns,
    int return_seeds, int seed_offset, curobo_hip_stream_t stream);

/* Local stage of the seed-parallel arg-min exchange in one launch: out_rows[p] = (min over the seeds of cost[p, :], seed_offset
 * + the first index that attains it (as fp32), payload[p, index, :]), [num_problems, 2 + payload_width].  Reference
 * single-GPU equivalent: solver_ik.py:503-515, solver_trajopt.py:469-484. */
int curobo_hip_argmin_rows(float *out_rows, const float *cost, const float *payload, int num_problems, int num_seeds,
                           int payload_width, int seed_offset, curobo_hip_stream_t stream);

/* ---------------------------------------------------------------- optimization: MPPI update
 * reference: optim/particle/mppi.py:201-313 + jit helpers :615-757 (pure torch, DIAG_A
 * covariance).  costs [problems, particles, cost_horizon] (cost_horizon may be 1 for totals),
 * gamma_seq [cost_horizon], actions [problems, particles, action_horizon, action_dim],
 * mean [problems, action_horizon, action_dim], cov / new_cov / new_scale_tril
 * [problems, 1, action_dim].  w = softmax(-(sum_h gamma_h cost_h / gamma_0) / beta);
 * best_traj (optional) = the action sequence of arg-max w (first index); weights (optional)
 * [problems, particles]. */
int curobo_hip_mppi_update_distribution(
    float *new_mean, float *new_cov, float *new_scale_tril, float *best_traj, float *weights,
    const float *costs, const float *gamma_seq, const float *actions, const float *mean,
    const float *cov, int num_problems, int num_particles, int cost_horizon, int action_horizon,
    int action_dim, float beta, float step_size_mean, float step_size_cov, float kappa,
    curobo_hip_stream_t stream);

/* ---------------------------------------------------------------- fused rollout
 * One launch for the data path of RobotRollout.evaluate_action + cost.backward
 * (reference rollout/rollout_robot.py:252-263,537-587, optim/components/gradient_opt_core.py
 * :445-480): B-spline knots -> joint positions -> FK -> collision spheres -> self collision +
 * (swept) scene collision -> out_cost[b] (sum over the padded horizon) and
 * out_grad_knots[b, n_knots, dof] = d out_cost / d knots.  It replaces the launch sequence
 * bspline forward, kinematics forward, self collision, sphere-obstacle collision, cost sum,
 * kinematics backward, bspline backward of the entry points above with identical arithmetic; all
 * intermediates stay in LDS.  out_position [b, h, dof] and out_robot_spheres [b, h, s, 4] are
 * optional (NULL = not materialised).  pair_locations / self_collision_weight NULL = no self
 * collision term; scene / scene_collision_weight NULL = no scene term.  Returns
 * CUROBO_HIP_ERR_INVALID when one trajectory's working set does not fit in 160 KB of LDS (use the
 * unfused entry points then). */
int curobo_hip_rollout_trajectory_fused(
    float *out_cost, float *out_grad_knots, float *out_position, float *out_robot_spheres,
    const float *u_position, const float *start_position, const float *start_velocity,
    const float *start_acceleration, const float *start_jerk, const float *goal_position,
    const float *goal_velocity, const float *goal_acceleration, const float *goal_jerk,
    const int32_t *start_idx, const int32_t *goal_idx, const float *traj_dt,
    const uint8_t *use_implicit_goal_state, const float *fixed_transform,
    const float *robot_spheres, const int8_t *joint_map_type, const int16_t *joint_map,
    const int16_t *link_map, const int16_t *link_sphere_map, const int16_t *link_chain_data,
    const int16_t *link_chain_offsets, const float *joint_offset_map, const float *sphere_padding,
    const float *self_collision_weight, const int16_t *pair_locations,
    const curobo_hip_scene *scene, const float *scene_collision_weight,
    const float *activation_distance, const float *speed_dt, const int32_t *env_query_idx,
    int num_envs, int use_multi_env, int batch_size, int padded_horizon, int dof, int n_knots,
    int bspline_degree, int num_links, int num_spheres, int num_collision_pairs,
    int link_chain_len, int sweep_steps, int enable_speed_metric, int32_t *dispatch_ws,
    int dispatch_phase, const uint32_t *self_lane_lists, int self_lane_len, curobo_hip_stream_t stream);

/* The pair list of a robot dealt to lanes, for the self-collision pass of the fused trajectory kernels (optional:
 * self_lane_lists NULL = the pass walks pair_locations as the reference kernel does, self_collision_kernel.cuh:19-111).
 * Every pair is given to one of its two spheres so that the longest per-sphere list is as short as possible; a lane
 * then keeps its own sphere in registers and reads one partner per pair.  Same arg-max, same bits.  HOST pointers in,
 * HOST words out ((len0 + len1) * 64 of them; 64 * (num_collision_pairs / 64 + 2) words of capacity always suffice for
 * robots of up to 64 spheres); the return value (len0 | len1 << 16) is the self_lane_len argument; 0 = this robot is
 * outside the form (pass NULL); < 0 = bad arguments.  Copy the words to the device once per robot. */
int curobo_hip_self_lane_lists_host(uint32_t *out_lists_host, int capacity_words, const int16_t *pair_locations_host,
                                    int num_collision_pairs, int num_spheres);

/* Longest-first dispatch workspace of the fused trajectory kernels (optional; no reference
 * counterpart: the reference launches one thread per sphere, its work per thread block is
 * uniform).  dispatch_ws = device int32 [curobo_hip_rollout_dispatch_ws_size(batch)], set up once by
 * curobo_hip_rollout_dispatch_ws_init; the caller alternates dispatch_phase 0, 1, 0, ... between
 * consecutive launches on the same batch (each launch measures its workgroup durations and one
 * workgroup sorts the previous launch's into the order the next launch uses).  Outputs are
 * identical with and without it (NULL = blockIdx order); only the tail of the launch shortens. */
int curobo_hip_rollout_dispatch_ws_size(int batch_size);
int curobo_hip_rollout_dispatch_ws_init(int32_t *dispatch_ws, int batch_size, curobo_hip_stream_t stream);

/* Optional cost terms of the full trajopt task (reference content/configs/task/trajopt/
 * lbfgs_bspline_trajopt.yml: tool_pose_cfg + cspace_cfg with cost_type STATE) for
 * curobo_hip_rollout_trajopt_fused.  Pointer meaning = curobo_hip_tool_pose_distance and
 * curobo_hip_cspace_state_cost.  Set n_tool_frames = 0 / cspace_weight = NULL to switch a term off.
 * Optional metric outputs (NULL = skip): out_pose_distance [b, h, T, 2], out_position_distance,
 * out_rotation_distance, out_goalset_idx [b, h, T], out_cspace_cost [b, h, dof]. */
typedef struct curobo_hip_trajopt_terms {
  float *out_pose_distance, *out_position_distance, *out_rotation_distance;
  int32_t *out_goalset_idx;
  const float *goal_position, *goal_quat;
  const int32_t *idxs_goal;
  const float *position_orientation_weight;
  const float *terminal_pose_axes_weight_factor, *non_terminal_pose_axes_weight_factor;
  const float *terminal_pose_convergence_tolerance, *non_terminal_pose_convergence_tolerance;
  const uint8_t *project_distance_to_goal;
  const int16_t *tool_frame_map;
  int32_t n_tool_frames, num_goalset, rotation_method;
  float *out_cspace_cost;
  const float *state_dt, *target_joint_position;
  const int32_t *idxs_target_joint_position;
  const float *p_b, *v_b, *a_b, *j_b, *effort_b;
  const float *cspace_weight, *cspace_activation_distance, *squared_l2_regularization_weights;
  const float *cspace_target_weight, *cspace_non_terminal_weight_factor, *cspace_target_dof_weight;
  int32_t retime_weights, retime_regularization_weights;
  /* joint-torque limits: the effort terms of the c-space STATE cost on tau = RNEA(q, qd, qdd) (reference
   * cost/wp_cspace_state.py + kernels/dynamics/rnea_*_kernel.cuh), inverse dynamics and its VJP inside the launch.
   * Pointers as in curobo_hip_launch_rnea_forward; needs curobo_hip_rollout_trajopt_fused_torque_fits(...) != 0 */
  const float *link_masses_com, *link_inertias, *gravity;
  const int16_t *level_links;
  int32_t use_torque_limits;
} curobo_hip_trajopt_terms;

/* curobo_hip_rollout_trajectory_fused plus the optional terms above: the whole reference trajopt
 * rollout (B-spline -> FK -> tool pose + c-space STATE + self + swept scene collision -> cost and
 * gradient to the knots) in one launch; the velocity / acceleration / jerk samples and their
 * gradients live in LDS as well.  terms may be NULL (then identical to the function above). */
int curobo_hip_rollout_trajopt_fused(
    float *out_cost, float *out_grad_knots, float *out_position, float *out_robot_spheres,
    const float *u_position, const float *start_position, const float *start_velocity,
    const float *start_acceleration, const float *start_jerk, const float *goal_position,
    const float *goal_velocity, const float *goal_acceleration, const float *goal_jerk,
    const int32_t *start_idx, const int32_t *goal_idx, const float *traj_dt,
    const uint8_t *use_implicit_goal_state, const float *fixed_transform,
    const float *robot_spheres, const int8_t *joint_map_type, const int16_t *joint_map,
    const int16_t *link_map, const int16_t *link_sphere_map, const int16_t *link_chain_data,
    const int16_t *link_chain_offsets, const float *joint_offset_map, const float *sphere_padding,
    const float *self_collision_weight, const int16_t *pair_locations,
    const curobo_hip_scene *scene, const float *scene_collision_weight,
    const float *activation_distance, const float *speed_dt, const int32_t *env_query_idx,
    int num_envs, int use_multi_env, int batch_size, int padded_horizon, int dof, int n_knots,
    int bspline_degree, int num_links, int num_spheres, int num_collision_pairs,
    int link_chain_len, int sweep_steps, int enable_speed_metric, int32_t *dispatch_ws,
    int dispatch_phase, const uint32_t *self_lane_lists, int self_lane_len, const curobo_hip_trajopt_terms *terms,
    curobo_hip_stream_t stream);

/* The two launches above with reuse of evaluations the caller already holds.  The launch is a pure function of its inputs, so
 * a trajectory b with b % memo_stride == memo_slot whose knots u_position[b] equal memo_x[b / memo_stride] bit for bit (compared
 * as 32-bit integers: equal NaN payloads are equal, -0.0 is not +0.0) gets out_cost[b] = memo_cost[b / memo_stride] and
 * out_grad_knots[b] = memo_grad[b / memo_stride] instead of a rollout; every other trajectory, and every trajectory whose knots
 * differ in any bit, is evaluated in full.  memo_x / memo_grad [batch_size / memo_stride, n_knots * dof], memo_cost
 * [batch_size / memo_stride]; all three NULL = the functions above.  THE CALLER'S CONTRACT: the memo row holds what this launch
 * would compute, i.e. it was produced by an earlier launch with the same scene, weights and robot, and with the start / goal
 * state, dt and environment that trajectory b has now (an L-BFGS line search whose first step magnitude is 0: the point it kept
 * is candidate 0 of the next iteration).  Rejected (CUROBO_HIP_ERR_INVALID) before any launch: only some of the three pointers,
 * memo_stride < 1, memo_slot outside [0, memo_stride), batch_size not a multiple of memo_stride, and reuse together with any
 * materialised output (out_position, out_robot_spheres, the per-term outputs of curobo_hip_trajopt_terms): a copied row cannot
 * fill those.  Reference: none (its optimiser re-evaluates the kept point, optim/components/gradient_opt_core.py:445-480). */
int curobo_hip_rollout_trajectory_fused_reuse(
    float *out_cost, float *out_grad_knots, float *out_position, float *out_robot_spheres,
    const float *u_position, const float *start_position, const float *start_velocity,
    const float *start_acceleration, const float *start_jerk, const float *goal_position,
    const float *goal_velocity, const float *goal_acceleration, const float *goal_jerk,
    const int32_t *start_idx, const int32_t *goal_idx, const float *traj_dt,
    const uint8_t *use_implicit_goal_state, const float *fixed_transform,
    const float *robot_spheres, const int8_t *joint_map_type, const int16_t *joint_map,
    const int16_t *link_map, const int16_t *link_sphere_map, const int16_t *link_chain_data,
    const int16_t *link_chain_offsets, const float *joint_offset_map, const float *sphere_padding,
    const float *self_collision_weight, const int16_t *pair_locations,
    const curobo_hip_scene *scene, const float *scene_collision_weight,
    const float *activation_distance, const float *speed_dt, const int32_t *env_query_idx,
    int num_envs, int use_multi_env, int batch_size, int padded_horizon, int dof, int n_knots,
    int bspline_degree, int num_links, int num_spheres, int num_collision_pairs,
    int link_chain_len, int sweep_steps, int enable_speed_metric, int32_t *dispatch_ws,
    int dispatch_phase, const uint32_t *self_lane_lists, int self_lane_len,
    const float *memo_x, const float *memo_cost, const float *memo_grad, int memo_stride, int memo_slot,
    curobo_hip_stream_t stream);

int curobo_hip_rollout_trajopt_fused_reuse(
    float *out_cost, float *out_grad_knots, float *out_position, float *out_robot_spheres,
    const float *u_position, const float *start_position, const float *start_velocity,
    const float *start_acceleration, const float *start_jerk, const float *goal_position,
    const float *goal_velocity, const float *goal_acceleration, const float *goal_jerk,
    const int32_t *start_idx, const int32_t *goal_idx, const float *traj_dt,
    const uint8_t *use_implicit_goal_state, const float *fixed_transform,
    const float *robot_spheres, const int8_t *joint_map_type, const int16_t *joint_map,
    const int16_t *link_map, const int16_t *link_sphere_map, const int16_t *link_chain_data,
    const int16_t *link_chain_offsets, const float *joint_offset_map, const float *sphere_padding,
    const float *self_collision_weight, const int16_t *pair_locations,
    const curobo_hip_scene *scene, const float *scene_collision_weight,
    const float *activation_distance, const float *speed_dt, const int32_t *env_query_idx,
    int num_envs, int use_multi_env, int batch_size, int padded_horizon, int dof, int n_knots,
    int bspline_degree, int num_links, int num_spheres, int num_collision_pairs,
    int link_chain_len, int sweep_steps, int enable_speed_metric, int32_t *dispatch_ws,
    int dispatch_phase, const uint32_t *self_lane_lists, int self_lane_len, const curobo_hip_trajopt_terms *terms,
    const float *memo_x, const float *memo_cost, const float *memo_grad, int memo_stride, int memo_slot,
    curobo_hip_stream_t stream);

/* 1 if the torque-limit terms fit (they borrow LDS regions that are dead when the inverse dynamics runs) */
int curobo_hip_rollout_trajopt_fused_torque_fits(
    int padded_horizon, int dof, int num_links, int num_spheres, int num_collision_pairs,
    int link_chain_len, int num_obstacles);

int curobo_hip_rollout_trajopt_fused_lds_bytes(
    int padded_horizon, int dof, int num_links, int num_spheres, int num_collision_pairs,
    int link_chain_len, int num_obstacles, int with_cspace_terms);

/* LDS bytes one trajectory needs in curobo_hip_rollout_trajectory_fused (host-side query, no GPU
 * work); the fused entry point is usable when this is <= 163840.  num_obstacles = max_cuboids +
 * max_voxel_grids of the scene (0 without a scene term). */
int curobo_hip_rollout_trajectory_fused_lds_bytes(
    int padded_horizon, int dof, int num_links, int num_spheres, int num_collision_pairs,
    int link_chain_len, int num_obstacles);

/* Horizon-1 (IK / teleport) rollout in one launch: q[b, dof] -> FK -> tool-pose goal-set cost
 * (curobo_hip_tool_pose_distance semantics, terminal weights) + joint-limit term of the c-space
 * cost (weight[0], activation_distance[0], limits p_b[2, dof]) + self collision + scene collision
 * (no sweep) -> out_cost[b] and out_grad_q[b, dof].  Replaces the launch sequence kinematics
 * forward, tool_pose_distance, cspace_position_cost, self_collision_distance,
 * sphere_obstacle_collision, kinematics backward, rollout_point_aggregate (reference: RobotRollout
 * with StateFromPositionTeleport and content/configs/task/ik/lbfgs_ik.yml).  Optional outputs
 * (NULL = skip): out_pose_distance [b, T, 2], out_position_distance / out_rotation_distance /
 * out_goalset_idx [b, T], out_link_pos [b, T, 3], out_link_quat [b, T, 4] (wxyz),
 * out_robot_spheres [b, S, 4], out_cspace_cost [b, dof].  env_query_idx [b] (use_multi_env: scene environment; num_envs > 1:
 * sphere set) must be constant over aligned runs of 16 configurations -- the seeds of one problem -- which share a
 * workgroup and its staged tables; NULL / 1 / 0 = one environment. */
int curobo_hip_rollout_ik_fused(
    float *out_cost, float *out_grad_q, float *out_pose_distance, float *out_position_distance,
    float *out_rotation_distance, int32_t *out_goalset_idx, float *out_link_pos,
    float *out_link_quat, float *out_robot_spheres, float *out_cspace_cost, const float *q,
    const float *goal_position, const float *goal_quat, const int32_t *idxs_goal,
    const float *position_orientation_weight, const float *terminal_pose_axes_weight_factor,
    const float *terminal_pose_convergence_tolerance, const uint8_t *project_distance_to_goal,
    int num_goalset, int rotation_method, const float *p_b, const float *cspace_weight,
    const float *cspace_activation_distance, const float *fixed_transform,
    const float *robot_spheres, const int8_t *joint_map_type, const int16_t *joint_map,
    const int16_t *link_map, const int16_t *tool_frame_map, const int16_t *link_sphere_map,
    const int16_t *link_chain_data, const int16_t *link_chain_offsets,
    const float *joint_offset_map, const float *sphere_padding,
    const float *self_collision_weight, const int16_t *pair_locations,
    const curobo_hip_scene *scene, const float *scene_collision_weight,
    const float *activation_distance, int batch_size, int dof, int num_links, int n_tool_frames,
    int num_spheres, int num_collision_pairs, int link_chain_len, const int32_t *env_query_idx, int num_envs,
    int use_multi_env, curobo_hip_stream_t stream);

/* curobo_hip_rollout_ik_fused with a current state: the arguments of that entry point in its order, then the current state, the
 * stream last.  The c-space term becomes the reference's with a state (cost/wp_cspace_position.py:299-356,
 * curobo_hip_cspace_position_cost semantics): row b reads state cur = idxs_current_state[b] (rows of one workgroup may differ)
 * and dt = state_dt[cur]; with dt > 0 the activation-shrunk limits are tightened to [current_position + velocity_limits[0] * dt,
 * current_position + velocity_limits[1] * dt] and 0.5 * (squared_l2_reg_weight[0] * dt) * v^2 + 0.5 * (squared_l2_reg_weight[1] *
 * dt^2) * a^2 is added, v = (q - current_position) / dt, a = (v - current_velocity) / dt; dt == 0 is the term of
 * curobo_hip_rollout_ik_fused, bit for bit.  out_cspace_cost [b, dof] carries the whole term.  current_position /
 * current_velocity [n_states, dof], idxs_current_state [b], velocity_limits [2, dof], state_dt [n_states],
 * squared_l2_reg_weight [2] (device).  current_velocity may be NULL when the acceleration weight is 0 (the acceleration term is
 * then skipped whatever the device-side weight says); acceleration_regularization != 0 states that the weight may be positive:
 * current_velocity is then required.  Same LDS layout as curobo_hip_rollout_ik_fused (curobo_hip_rollout_ik_fused_lds_bytes). */
int curobo_hip_rollout_ik_fused_state(
    float *out_cost, float *out_grad_q, float *out_pose_distance, float *out_position_distance,
    float *out_rotation_distance, int32_t *out_goalset_idx, float *out_link_pos,
    float *out_link_quat, float *out_robot_spheres, float *out_cspace_cost, const float *q,
    const float *goal_position, const float *goal_quat, const int32_t *idxs_goal,
    const float *position_orientation_weight, const float *terminal_pose_axes_weight_factor,
    const float *terminal_pose_convergence_tolerance, const uint8_t *project_distance_to_goal,
    int num_goalset, int rotation_method, const float *p_b, const float *cspace_weight,
    const float *cspace_activation_distance, const float *fixed_transform,
    const float *robot_spheres, const int8_t *joint_map_type, const int16_t *joint_map,
    const int16_t *link_map, const int16_t *tool_frame_map, const int16_t *link_sphere_map,
    const int16_t *link_chain_data, const int16_t *link_chain_offsets,
    const float *joint_offset_map, const float *sphere_padding,
    const float *self_collision_weight, const int16_t *pair_locations,
    const curobo_hip_scene *scene, const float *scene_collision_weight,
    const float *activation_distance, int batch_size, int dof, int num_links, int n_tool_frames,
    int num_spheres, int num_collision_pairs, int link_chain_len, const int32_t *env_query_idx, int num_envs,
    int use_multi_env, const float *squared_l2_reg_weight, const float *current_position,
    const float *current_velocity, const int32_t *idxs_current_state, const float *velocity_limits,
    const float *state_dt, int acceleration_regularization, curobo_hip_stream_t stream);

/* LDS bytes of one 16-configuration workgroup of curobo_hip_rollout_ik_fused (usable when <= 163840) */
int curobo_hip_rollout_ik_fused_lds_bytes(int dof, int num_links, int num_spheres,
                                          int num_collision_pairs, int link_chain_len,
                                          int num_obstacles);

/* Development hook: device buffer [batch, 16] (int64) that receives 100 MHz wall-clock stamps at
 * the phase boundaries (start, tables+spline, FK, costs+VJP, end) of every fused launch; NULL
 * (default) turns it off.  Used by tools/profile_fused.py. */
int curobo_hip_rollout_fused_set_profile_buffer(int64_t *device_buffer);
/* Same hook for a sequence of launches (e.g. those recorded into a hipGraph): launch k after this
 * call stamps into block k = device_buffer + k * block_rows * 16; launches beyond n_blocks (or with
 * more than block_rows trajectories) are not stamped.  NULL ends the sequence.  bench.py uses it to
 * time the rollout launches inside the replayed graph (stamp 0 = workgroup start, 4 = end). */
int curobo_hip_rollout_fused_set_profile_sequence(int64_t *device_buffer, int n_blocks, int block_rows);

/* Compile-time shapes of the fused trajectory launches (csrc/fused_shapes.hpp): for the robots / horizons listed there the
 * library holds instantiations whose every dimension is a compile-time constant (the reference compiles its kernels per
 * robot with NVRTC templates: kinematics_forward_kernel.cuh:126 N_LINKS, cuda_core_backend/kernel_cache.py:161-235); a launch
 * takes one only when ALL its dimensions match, otherwise the generic kernel -- same results, bit for bit.
 * curobo_hip_rollout_fused_shape_id: host-side query (no GPU work), the id (>= 1) of the shape a launch with these arguments
 * runs, 0 = the generic kernel.  self_lane_len = the value curobo_hip_self_lane_lists_host returned (0 = no lane lists);
 * num_collision_pairs = 0 when the self-collision term is off; kinds = 1 cuboids | 2 voxel grids (7 = analytic primitives).
 * plain_launch = 1: the launch form of an optimiser iteration -- self + scene collision with the speed metric, one environment,
 * a dispatch workspace, no materialised outputs, no profile stamps -- which some shapes also hold as compile-time facts.
 * curobo_hip_rollout_fused_set_shapes_enabled(0) makes every launch take the generic kernel (tests, A/B timing). */
int curobo_hip_rollout_fused_shape_id(int padded_horizon, int n_knots, int dof, int num_links, int num_spheres,
                                      int num_collision_pairs, int link_chain_len, int self_lane_len, int max_cuboids,
                                      int max_voxel_grids, int bspline_degree, int sweep_steps, int kinds,
                                      int with_trajopt_terms, int plain_launch);
int curobo_hip_rollout_fused_set_shapes_enabled(int enabled);
/* Shapes compiled at run time (curobo_amd/backends/fused_jit.py: hipcc on csrc/rollout_fused_shape.hip with the shape on the command
 * line, as the reference compiles its kernels per robot with NVRTC): `launcher` = the object's curobo_fused_jit_launch,
 * args_bytes = its curobo_fused_jit_args_bytes() (an object built from other sources is refused).  Registered shapes are tried
 * before the built-in table and report ids >= 100 from curobo_hip_rollout_fused_shape_id.
 * curobo_hip_rollout_fused_threads returns the workgroup size a launch with these dimensions uses (a shape holds it as a
 * constant); num_obstacles = max_cuboids + max_voxel_grids.  Host-side, no GPU work. */
int curobo_hip_rollout_fused_register_shape(void *launcher, int args_bytes);
int curobo_hip_rollout_fused_threads(int padded_horizon, int dof, int num_links, int num_spheres, int num_collision_pairs,
                                     int link_chain_len, int self_lane_len, int num_obstacles, int with_trajopt_terms);

/* ---------------------------------------------------------------- trajectory: B-spline
 * reference: cuda_core_backend/trajectory.py:28-204, pybind/trajectory_bindings.cpp:133-142
 * kernels:   kernels/trajectory/bspline/bspline_kernel.cuh:81-151,332-380
 * `horizon` of the forward launch is the padded horizon (out_position.shape[1]).
 */
int curobo_hip_launch_bspline_interpolation_forward_kernel(
    float *out_position, float *out_velocity, float *out_acceleration, float *out_jerk,
    float *out_dt, const float *u_position, const float *start_position,
    const float *start_velocity, const float *start_acceleration, const float *start_jerk,
    const float *goal_position, const float *goal_velocity, const float *goal_acceleration,
    const float *goal_jerk, const int32_t *start_idx, const int32_t *goal_idx,
    const float *traj_dt, const uint8_t *use_implicit_goal_state, int batch_size, int horizon,
    int dof, int n_knots, int bspline_degree, curobo_hip_stream_t stream);

int curobo_hip_launch_bspline_interpolation_backward_kernel(
    float *out_grad_position, const float *grad_position, const float *grad_velocity,
    const float *grad_acceleration, const float *grad_jerk, const float *traj_dt,
    const int32_t *dt_idx, const uint8_t *use_implicit_goal_state, int batch_size,
    int padded_horizon, int dof, int n_knots, int bspline_degree, int use_direct_polynomial,
    curobo_hip_stream_t stream);

/* reference: cuda_core_backend/trajectory.py:207-306, kernel bspline_kernel.cuh:221-270.
 * One interpolation_dt[1] for all trajectories, interpolation_horizon[b] per trajectory; outputs
 * are [batch, max_out_tsteps, dof]; points past a trajectory's horizon repeat its last sample.
 * knot_dt is accepted and ignored, as in the reference kernel. */
int curobo_hip_launch_bspline_interpolation_single_dt_kernel(
    float *out_position, float *out_velocity, float *out_acceleration, float *out_jerk,
    float *out_dt, const float *knots, const float *knot_dt, const float *start_position,
    const float *start_velocity, const float *start_acceleration, const float *start_jerk,
    const float *goal_position, const float *goal_velocity, const float *goal_acceleration,
    const float *goal_jerk, const int32_t *start_idx, const int32_t *goal_idx,
    const float *interpolation_dt, const uint8_t *use_implicit_goal_state,
    const int32_t *interpolation_horizon, int batch_size, int max_out_tsteps, int dof,
    int n_knots, int bspline_degree, curobo_hip_stream_t stream);

/* Legacy control spaces (reference cuda_core_backend/trajectory.py:309-556; kernels
 * kernels/trajectory/legacy/differentiation_position_kernel.cuh:15-370 with use_stencil = true,
 * legacy/integration_acceleration_kernel.cuh:8-135).
 * POSITION: u_position [batch, horizon-4, dof] -> position/velocity/acceleration/jerk
 * [batch, horizon, dof] by five-point stencils over the start-extrapolated, goal-replicated
 * position sequence; horizon >= 9.  goal_velocity / goal_acceleration are accepted and unused.
 * ACCELERATION: u_acc [batch, horizon, dof], traj_dt [horizon] (indexed by step); use_rk2 selects
 * nothing (both reference kernels run the same recursion). */
int curobo_hip_launch_differentiation_position_forward_kernel(
    float *out_position, float *out_velocity, float *out_acceleration, float *out_jerk,
    float *out_dt, const float *u_position, const float *start_position,
    const float *start_velocity, const float *start_acceleration, const float *goal_position,
    const float *goal_velocity, const float *goal_acceleration, const int32_t *start_idx,
    const int32_t *goal_idx, const float *traj_dt, const uint8_t *use_implicit_goal_state,
    int batch_size, int horizon, int dof, curobo_hip_stream_t stream);

int curobo_hip_launch_differentiation_position_backward_kernel(
    float *out_grad_position, const float *grad_position, const float *grad_velocity,
    const float *grad_acceleration, const float *grad_jerk, const float *traj_dt,
    const int32_t *dt_idx, const uint8_t *use_implicit_goal_state, int batch_size, int horizon,
    int dof, curobo_hip_stream_t stream);

int curobo_hip_launch_integration_acceleration_kernel(
    float *out_position, float *out_velocity, float *out_acceleration, float *out_jerk,
    const float *u_acc, const float *start_position, const float *start_velocity,
    const float *start_acceleration, const int32_t *start_idx, const float *traj_dt,
    int batch_size, int horizon, int dof, int use_rk2, curobo_hip_stream_t stream);

/* ---------------------------------------------------------------- optimization
 * reference: cuda_core_backend/optimization.py:27-260, pybind/optimization_bindings.cpp:14-75
 * kernels:   kernels/optimization/lbfgs/lbfgs_step_kernel.cuh:18-199,
 *            kernels/optimization/line_search/line_search_kernel.cuh:27-155
 */
int curobo_hip_launch_lbfgs_step(
    float *step_vec, float *rho_buffer, float *y_buffer, float *s_buffer, const float *q,
    const float *grad_q, float *x_0, float *grad_0, float epsilon, int batch_size, int history_m,
    int v_dim, int stable_mode, int use_shared_buffers, curobo_hip_stream_t stream);

int curobo_hip_launch_line_search(
    float *best_cost, float *best_action, int16_t *best_iteration, int16_t *current_iteration,
    uint8_t *converged_global, int convergence_iteration, float cost_delta_threshold,
    float cost_relative_threshold, float *exploration_cost, float *exploration_action,
    float *exploration_gradient, int32_t *exploration_idx, float *selected_cost,
    float *selected_action, float *selected_gradient, int32_t *selected_idx,
    const float *search_cost, const float *search_action, const float *search_gradient,
    const float *step_direction, const float *search_magnitudes, float armijo_threshold_c_1,
    float curvature_threshold_c_2, int strong_wolfe, int approx_wolfe, int n_linesearch,
    int opt_dim, int batchsize, curobo_hip_stream_t stream);

/* Line-search candidates, fused (extension; reference: torch ops in
 * optim/gradient/line_search_strategy.py:134-204 `_prepare_search_points`, :281-325):
 *   scale = max(1, max_v |d_v| / action_step_max[v % action_dim])  (if apply_step_scale)
 *   step_direction_out = d / scale;  x_set[b,k,:] = x[b,:] + search_magnitudes[k] * d / scale */
int curobo_hip_prepare_search_points(
    float *x_set, float *step_direction_out, const float *x, const float *step_direction,
    const float *action_step_max, const float *search_magnitudes, int batchsize, int n_linesearch,
    int opt_dim, int action_dim, int apply_step_scale, curobo_hip_stream_t stream);

/* The optimiser side of one L-BFGS iteration in ONE launch (opt_dim <= 128): launch_line_search,
 * then launch_lbfgs_step from the chosen exploration point, then prepare_search_points for the
 * next iteration -- the same arithmetic as the three entry points above run back to back
 * (reference optim/gradient/lbfgs.py:156-265, gradient_opt_core.py:255-480), with the exploration
 * point and the new direction handed over in registers.  search_action (the candidate set x_set)
 * and step_direction_scaled are read by the line search and then overwritten with the next
 * iteration's candidates / scaled direction.  step_vec receives the unscaled direction.
 * overlapped != 0: the launch shares the GPU with other work (the seed shards of optim/pipelined.py run their rollouts
 * next to it): wavefront-sized problems then take ONE wavefront and no LDS each instead of a 256-lane workgroup with
 * the history staged through LDS -- 1 us more on an idle GPU, 5 us less per iteration between busy rollout
 * workgroups, whose LDS and registers the workgroup form has to wait for.  Same results bit for bit. */
int curobo_hip_launch_lbfgs_iteration_tail(
    float *best_cost, float *best_action, int16_t *best_iteration, int16_t *current_iteration,
    uint8_t *converged_global, int convergence_iteration, float cost_delta_threshold,
    float cost_relative_threshold, float *exploration_cost, float *exploration_action,
    float *exploration_gradient, int32_t *exploration_idx, float *selected_cost,
    float *selected_action, float *selected_gradient, int32_t *selected_idx,
    const float *search_cost, float *search_action, const float *search_gradient,
    float *step_direction_scaled, const float *search_magnitudes, float armijo_threshold_c_1,
    float curvature_threshold_c_2, int strong_wolfe, int approx_wolfe, int n_linesearch,
    int opt_dim, int batchsize, float *step_vec, float *rho_buffer, float *y_buffer,
    float *s_buffer, float *x_0, float *grad_0, float epsilon, int history_m, int stable_mode,
    const float *action_step_max, int action_dim, int apply_step_scale, int overlapped,
    curobo_hip_stream_t stream);

/* Compile-time shapes of the one-launch tail (csrc/tail_shapes.hpp), after the fused rollout's: for the problem sizes listed
 * there (trajectory optimisation of a 7-dof arm: opt_dim 84, history 27; its inverse kinematics: opt_dim 7, history 7; four
 * candidates each) the library holds instantiations whose opt_dim, history, n_linesearch and action_dim are constants.  A
 * launch takes one only when ALL four match, otherwise the kernels that read them from their arguments -- same results, bit
 * for bit.  Host-side, no GPU work:
 * curobo_hip_lbfgs_tail_shape_id: the id (>= 1) of the shape with these dimensions, 0 = none.
 * curobo_hip_lbfgs_set_tail_shapes_enabled(0) makes every launch take the run-time kernels (tests, A/B timing).
 * curobo_hip_lbfgs_tail_form: what curobo_hip_launch_lbfgs_iteration_tail runs for these arguments, as form | shape << 4:
 *   form 0 = the plain kernel (64-bit addresses), 1 = 16-lane row per problem, 2 = wavefront per problem, 3 = workgroup per
 *   problem; shape = the compile-time shape taken (0 = run-time dimensions).  Forms 1 and 3 keep part of the row address in a
 *   32-bit lane offset and are taken only when it fits (batchsize * opt_dim * 4 bytes times n_linesearch resp. history stays
 *   below 2^31); past that the launch runs form 0 resp. 2. */
int curobo_hip_lbfgs_tail_shape_id(int opt_dim, int history, int n_linesearch, int action_dim);
int curobo_hip_lbfgs_set_tail_shapes_enabled(int enabled);
int curobo_hip_lbfgs_tail_form(int opt_dim, int history, int n_linesearch, int action_dim, int batchsize, int overlapped);

/* ---------------------------------------------------------------- rollout glue
 * Per-trajectory cost sum (reference rollout/metrics.py:233-265 + util/tensor_util.py:104:
 * torch cat + sum): out[b] = sum_h( self_cost[b,h] + sum_s scene_cost[b,h,s] ), one wavefront
 * per trajectory with a wave64 shuffle reduction.  Either input may be NULL. */
int curobo_hip_trajectory_cost_sum(float *out_cost, const float *self_cost,
                                   const float *scene_cost, int batch_size, int horizon,
                                   int num_spheres, curobo_hip_stream_t stream);

/* ---- PRM graph planner (curobo_amd/graph_planner) ---------------------------------------------
 * Edge steering (reference LinearConnector.steer_until_infeasible): rows start[n, ld] -> target[n, ld]
 * (first dof columns) are walked at the batch-wide step count max_steps = max over edges of
 * ceil(max_k |w_k (t_k - s_k)| / cspace_similarity_threshold) + 1, reduced on the device into
 * max_steps_ws[1] ahead of the walk (no host sync).  Point k of an edge is s + (k / max_steps)(t - s);
 * a point is feasible when its scene cost, self-collision cost and joint-bound cost are all exactly 0
 * with activation distance 0.  Outputs: out_node[n, dof + 1] = the point before the first infeasible
 * one (clamped to index 0; the end point when none is infeasible), index column 0; out_index[n] =
 * its step index.  point_mode != 0: start rows only (target, weight, threshold, out_node, out_index
 * and max_steps_ws unused), out_feasible[n] = 1 where the configuration is feasible.  Scenes of
 * cuboids, primitives and voxel grids (meshes are not covered). */
int curobo_hip_graph_steer(float *out_node, int32_t *out_index, uint8_t *out_feasible, int32_t *max_steps_ws,
                           const float *start, const float *target, int ld, const float *cspace_distance_weight,
                           float cspace_similarity_threshold, int n, int point_mode, const float *p_b,
                           const float *fixed_transform, const float *robot_spheres, const int8_t *joint_map_type,
                           const int16_t *joint_map, const int16_t *link_map, const int16_t *link_sphere_map,
                           const int16_t *link_chain_data, const int16_t *link_chain_offsets,
                           const float *joint_offset_map, const float *sphere_padding,
                           const int16_t *pair_locations, const curobo_hip_scene *scene, int dof, int num_links,
                           int num_spheres, int num_collision_pairs, int link_chain_len, curobo_hip_stream_t stream);

/* Weighted k nearest neighbours (reference DistanceNeighborCalculator.jit_find_nearest_neighbors):
 * for each query row of queries[n_queries, ld_q], the indices of the k closest of the first n_nodes
 * rows of nodes[*, ld_n] under the distance || w * (x - q) || over the first dof columns, nearest
 * first, ties to the lower node index -> out_idx[n_queries, k].  1 <= k <= min(64, n_nodes). */
int curobo_hip_graph_knn(int32_t *out_idx, const float *queries, int ld_q, const float *nodes, int ld_n,
                         const float *cspace_distance_weight, int n_queries, int n_nodes, int dof, int k,
                         curobo_hip_stream_t stream);

/* ---- perception (curobo_amd/perception) ---------------------------------------------------------
 * Depth filter (reference FilterDepth: perception/filter_depth.py): (batch, height, width) fp32 depth ->
 * depth_out (rejected pixels 0) and valid_mask_out u8 (1 = kept).  Range check (finite, minimum / maximum
 * distance), flying-pixel rejection (enable_flying_pixel != 0: largest 4-neighbour difference against
 * flying_tolerance * depth, the tolerance computed by the caller as 0.08 (0.005 / 0.08)^threshold) and
 * bilateral smoothing (bilateral_kernel_size odd, 0 = off; sigma_*_sq2 = 2 sigma^2).  Kernel sizes below 7 are
 * one launch; from 7 on the reference's three passes (the fused pass without smoothing into temp_a, a
 * horizontal pass into temp_b, a vertical pass into depth_out): temp_a / temp_b are (batch, height, width)
 * fp32 scratch images then, unused (may be NULL) otherwise.  depth_out must not alias depth_in. */
int curobo_hip_filter_depth(float *depth_out, uint8_t *valid_mask_out, const float *depth_in, float *temp_a,
                            float *temp_b, int batch, int height, int width, float depth_minimum_distance,
                            float depth_maximum_distance, int enable_flying_pixel, float flying_tolerance,
                            int bilateral_kernel_size, float sigma_spatial_sq2, float sigma_depth_sq2,
                            curobo_hip_stream_t stream);

/* Robot mask (reference RobotSegmenter._mask_op): pixel point = depth * projection_rays[pixel] moved by the
 * camera pose (position + wxyz quaternion) into the robot frame; mask_out u8 = depth > 0 and some sphere
 * with radius >= 0 has radius - |point - centre| > -distance_threshold; depth_out = depth with the masked
 * pixels set to 0.  depth (batch, height, width); projection_rays (ray_batch, height * width, 3),
 * camera_position (pose_batch, 3), camera_quaternion (pose_batch, 4), robot_spheres (sphere_batch,
 * num_spheres, 4) = x y z radius, 16-byte aligned; each of the three batches is 1 or batch.  bf16_ops != 0
 * is the reference's default arithmetic (ops_dtype = bfloat16): depth, rays and spheres rounded to bf16
 * (nearest even), depth * ray rounded to bf16, everything after that fp32.  One launch; nothing of size
 * pixels x spheres is written. */
int curobo_hip_robot_mask(uint8_t *mask_out, float *depth_out, const float *depth, const float *projection_rays,
                          const float *camera_position, const float *camera_quaternion, const float *robot_spheres,
                          int batch, int height, int width, int num_spheres, int ray_batch, int pose_batch,
                          int sphere_batch, float distance_threshold, int bf16_ops, curobo_hip_stream_t stream);

/* ---- mesh-SDF pose refinement (curobo_amd/perception/pose_estimation; reference SDFPoseDetector:
 * perception/pose_estimation/sdf_pose_detector.py).  One Levenberg-Marquardt iteration is two launches: an evaluation
 * of the observed points at the candidate pose, then one step.  Nothing accumulates with atomics: results are
 * bit-identical from run to run.
 *
 * The evaluation's workspace: one row of CUROBO_HIP_POSE_WS_ROW 4-byte words per workgroup of 256 points -- words 0..20 the
 * upper triangle of J^T J (row major), 21..26 J^T r, 27 sum r^2 (floats), 28 the valid count (int32), the rest 0.  Every row is
 * written by every evaluation: nothing needs zeroing in between. */
#define CUROBO_HIP_POSE_WS_ROW 32
int curobo_hip_pose_sdf_ws_bytes(int n_points, int64_t *out_bytes);

/* mesh_surface_distance_query_kernel (wp_mesh_sdf_alignment.py:84-146) and the per-thread part of jacobian_reduce_kernel
 * (:176-222) for points [n_points, 3] in the world frame against ONE mesh at the pose position [3] / quaternion [4] wxyz
 * (DEVICE pointers: the step kernel writes them): p_mesh = R^T (p - t) (:121), the closest surface point within
 * max_distance (:124-128; unsigned, no inside test), valid iff one was found and 1e-8 < distance <= distance_threshold
 * (:135), gradient = R (closest - p_mesh) / distance (:137-140), the Huber scale sqrt(huber_delta / r) for r > huber_delta
 * (:207-211, use_huber != 0), the Jacobian row [g, (g_z p_y - g_y p_z, g_x p_z - g_z p_x, g_y p_x - g_x p_y)] times that
 * scale (:213-220).  out_distance [n_points], out_gradient [n_points, 3], out_valid [n_points] int32: optional (NULL skips
 * one), 0 at invalid points.  The sums the reference adds with tile_atomic_add (:238-377) leave as one row per workgroup
 * in `workspace` (see above), in a fixed order.  mesh: HOST pointer (the struct is copied into the launch).  A pose that is
 * not finite finds nothing. */
int curobo_hip_pose_sdf_evaluate(float *out_distance, float *out_gradient, int32_t *out_valid, void *workspace,
                                 int64_t workspace_bytes, const float *points, const float *position,
                                 const float *quaternion, const curobo_hip_mesh *mesh, float max_distance,
                                 float distance_threshold, int use_huber, float huber_delta, int n_points,
                                 curobo_hip_stream_t stream);

/* The refinement state (SDFRefinementState, sdf_pose_detector.py:56-75, plus the candidate the next evaluation reads), on
 * the DEVICE; 4-byte fields only. */
typedef struct curobo_hip_pose_lm_state {
  float best_position[3], best_quaternion[4]; /* wxyz */
  float best_error, best_sum_sq;
  int32_t best_n_valid;
  float lambda_damping;
  float best_JtJ[36], best_Jtr[6];
  float cand_position[3], cand_quaternion[4]; /* what curobo_hip_pose_sdf_evaluate is to be called with next */
  float pred_reduction;
  float delta[6];       /* translation_change = delta[0..2], rotation_change = delta[3..5] */
  float cand_sum_sq;    /* of the evaluation this step consumed */
  int32_t cand_n_valid;
  float trust_ratio;    /* of this step (0 in the initial mode) */
  int32_t accepted;     /* of this step (1 in the initial mode) */
} curobo_hip_pose_lm_state;

#define CUROBO_HIP_POSE_LM_INIT 0
#define CUROBO_HIP_POSE_LM_UPDATE 1
/* Everything _refine_iteration (sdf_pose_detector.py:305-399) does outside its two Warp launches, by one lane.  The rows
 * of `workspace` (the evaluation at state->cand_*) are added in workgroup order.  Then
 *   mode CUROBO_HIP_POSE_LM_INIT   (_setup_refinement :266-302): the sums become the best state, best_error =
 *        sqrt(sum r^2 / (n + 1e-8)), lambda_damping = lambda_initial;
 *   mode CUROBO_HIP_POSE_LM_UPDATE (trust_region_update, optim_pose_lm.py:53-175): has_enough_valid = n >
 *        minimum_valid_count (the reference's 10); trust ratio = (best_sum_sq - sum r^2) / (pred_reduction + 1e-8); the
 *        step is accepted iff ratio >= 0 and has_enough_valid -- rho_min is carried and, as in the reference (:142), not
 *        consulted; lambda is divided (accepted) or multiplied by lambda_factor and clamped to [lambda_min, lambda_max];
 *        the best position, quaternion, error, sum r^2, count, J^T J and J^T r are the candidate's or stay.
 * Both modes then produce the next candidate from the best state: delta from the fp32 Cholesky factorisation of
 * J^T J + lambda I (solve_lm_step :180-202), pred_reduction = -delta . J^T r - 0.5 delta . J^T J delta (:28-48), and the pose
 * Pose.from_euler_xyz(delta[3..5], delta[0..2]).multiply(best) (sdf_pose_detector.py:327-334), not renormalised.  A pivot
 * that is not positive makes delta, the prediction and the candidate NaN: that candidate finds no point, is rejected by the
 * next step, and lambda grows. */
int curobo_hip_pose_lm_step(curobo_hip_pose_lm_state *state, const void *workspace, int64_t workspace_bytes, int n_points,
                            int mode, float lambda_initial, float lambda_factor, float lambda_min, float lambda_max,
                            float rho_min, int minimum_valid_count, curobo_hip_stream_t stream);

/* ---- point-to-plane ICP (curobo_amd/perception/pose_estimation/pose_detector.py; reference PoseDetector:
 * perception/pose_estimation/pose_detector.py :172-375 and util.py :88-113, :245-330).  Every hypothesis of a stage advances
 * together, one iteration in two launches; nothing accumulates with atomics, results are bit-identical from run to run.
 *
 * One state per hypothesis, on the DEVICE, 4-byte fields only.  T: rows 0..2 of the homogeneous transform, row major
 * (R | t).  iterations: the reference's iter_idx + 1.  stopped: set by the step where the reference's loop breaks. */
typedef struct curobo_hip_pose_icp_state {
  float T[12];
  float error;            /* written by the finalize step: mean nearest distance, +inf when nothing was found */
  int32_t iterations, stopped, solver_failed;
  int32_t n_valid;        /* of the last step that ran */
  float x[6];             /* the last solve: rotation vector, translation */
  int32_t reserved;
} curobo_hip_pose_icp_state;
#define CUROBO_HIP_POSE_ICP_STATE_WORDS 24

/* The workspace: per hypothesis one row of CUROBO_HIP_POSE_WS_ROW words per workgroup of 64 mesh samples -- words 0..20 the
 * upper triangle of sum w J J^T (row major), 21..26 sum w J b, 27 the sum of nearest distances over every sample (thresholded
 * or not), 28 the valid count (int32), the rest 0. */
int curobo_hip_pose_icp_ws_bytes(int n_hypotheses, int n_mesh, int64_t *out_bytes);

/* For hypothesis h and mesh sample i: s = R_h p_i + t_h, n' = R_h n_i, the nearest of observed_points [n_observed, 3] by
 * brute force (squared distances in fp32, ties to the lowest index), valid iff distance <= distance_threshold (infinity
 * allowed: every sample valid); for a valid one b = (o - s) . n', w = 1 if |b| < huber_delta else huber_delta / (|b| + 1e-10)
 * (1 when use_huber == 0), Jacobian row [s x n', n'].  One workspace row per workgroup (above).  Optional per-sample outputs
 * [n_hypotheses, n_mesh]: out_index (-1 when invalid), out_distance.  honour_stopped != 0: the workgroups of a hypothesis
 * whose state is marked stopped return at once and leave its rows as they are. */
int curobo_hip_pose_icp_correspond(int32_t *out_index, float *out_distance, void *workspace, int64_t workspace_bytes,
                                   const float *mesh_points, const float *mesh_normals, const float *observed_points,
                                   const curobo_hip_pose_icp_state *state, float distance_threshold, int use_huber,
                                   float huber_delta, int honour_stopped, int n_hypotheses, int n_mesh, int n_observed,
                                   curobo_hip_stream_t stream);

#define CUROBO_HIP_POSE_ICP_COARSE 0
#define CUROBO_HIP_POSE_ICP_FINE 1
#define CUROBO_HIP_POSE_ICP_FINALIZE 2
/* One wavefront per hypothesis; its rows are added in workgroup order.  COARSE / FINE (a stopped hypothesis is left as it
 * is): iterations += 1; fewer than 10 valid samples stop it with T unchanged; else (J^T W J + 1e-6 I) x = J^T W b by a 6 x 6
 * Cholesky in fp32, q = (cos(theta/2), omega sin(theta/2) / max(theta, 1e-10)), T <- T_update T.  FINE stops BEFORE the
 * update when |x[3..5]| < 1e-4.  Deviation from the reference, which falls back to lstsq when the factorisation fails: a
 * pivot that is not positive or not finite stops the hypothesis with T unchanged and sets solver_failed.
 * FINALIZE (stopped or not): error = sum of distances / n_mesh, +inf when no sample is valid; nothing else changes. */
int curobo_hip_pose_icp_step(curobo_hip_pose_icp_state *state, const void *workspace, int64_t workspace_bytes,
                             int n_hypotheses, int n_mesh, int mode, curobo_hip_stream_t stream);

/* out_index[0] = arg-min of the states' errors: the lowest index wins a tie, a NaN never wins, nothing finite gives 0.
 * Optional: out_error [1] the winning error, out_transform [12] the winner's T. */
int curobo_hip_pose_icp_select(int32_t *out_index, float *out_error, float *out_transform,
                               const curobo_hip_pose_icp_state *state, int n_hypotheses, curobo_hip_stream_t stream);

/* ---- depth mapper (curobo_amd/perception/mapper; reference perception/mapper: kernel/builder/builder_camera_integrate.py
 * :89-166 and :400-487, builder_esdf.py :107-133, :267-491, builder_raycast.py :1015-1042).  The TSDF is stored DENSE:
 * the grid of grid_w x grid_h x grid_d voxels (x, y, z) padded to whole blocks of block_size^3, block (bx, by, bz) at index
 * (bz nby + by) nbx + bx, block_data fp16 [n_blocks][block_size^3][2] = (sum sdf w, sum w) at local index
 * lz BS^2 + ly BS + lx, and one byte per block: block_mask "ever visible" (the reference's "allocated"), frame_mask
 * "visible in this frame".  Voxel centre = origin + (g + 0.5 - N / 2) voxel_size.  No launch uses an atomic; every launch
 * has dimensions fixed by the shapes alone (the mesh launches further down: by the number of visible blocks as well).  The
 * struct is read on the HOST at launch. */
typedef struct curobo_hip_mapper_params {
  int32_t grid_w, grid_h, grid_d;   /* voxels along x, y, z */
  int32_t block_size;               /* 1 or a power of two in 2..32 */
  int32_t nbx, nby, nbz;            /* blocks along x, y, z = ceil(grid / block_size) */
  int32_t num_samples;              /* samples per pixel of the marking stage: ceil(2 truncation / step_size) + 1 */
  float origin[3];                  /* world position of the grid's centre */
  float voxel_size, truncation_distance, depth_min, depth_max, minimum_tsdf_weight;
  float step_size;                  /* block_size voxel_size / 1.42 */
} curobo_hip_mapper_params;

/* n_bytes (a multiple of 4) bytes of a mask to 0: a kernel node, where a memset node would do on other stacks */
int curobo_hip_mapper_clear_mask(uint8_t *mask, int64_t n_bytes, curobo_hip_stream_t stream);

/* One lane per (camera, pixel, sample): depth [n_cameras, height, width] metres, intrinsics [n_cameras, 3, 3],
 * cam_position [n_cameras, 3], cam_quaternion [n_cameras, 4] wxyz.  A pixel with depth in [depth_min, depth_max] is walked
 * along its ray ((px + 0.5 - cx) / fx, (py + 0.5 - cy) / fy, 1) z from z_start = max(depth - truncation, depth_min) in
 * steps of step_size while z <= depth + truncation + step_size; the block of every sample that falls into the grid gets 1
 * in frame_mask and block_mask (plain byte stores of the same value). */
int curobo_hip_mapper_mark_blocks(uint8_t *frame_mask, uint8_t *block_mask, const float *depth, const float *intrinsics,
                                  const float *cam_position, const float *cam_quaternion,
                                  const curobo_hip_mapper_params *params, int n_cameras, int height, int width,
                                  curobo_hip_stream_t stream);

/* One workgroup per block, returning at once where frame_mask is 0.  Per voxel and camera: the centre in the camera frame,
 * z > depth_min, u = fx x / z + cx, v = fy y / z + cy, pixel ((int)u, (int)v) inside the image, its depth d in [depth_min,
 * depth_max], sdf = d - z >= -truncation, clamped to truncation, weight = max((fx vs / z)(fy vs / z), 1).  z for the sdf is
 * evaluated in double (d - z cancels at the surface, where an fp32 z is off by more than a step of the fp16 word); the pixel
 * and the weight are fp32.  The sums over the cameras are fp32; where the summed weight is > 0 they are added to the stored
 * pair in fp32 and rounded once to fp16. */
int curobo_hip_mapper_integrate(void *block_data, const uint8_t *frame_mask, const float *depth, const float *intrinsics,
                                const float *cam_position, const float *cam_quaternion,
                                const curobo_hip_mapper_params *params, int n_cameras, int height, int width,
                                curobo_hip_stream_t stream);

/* The ESDF grid: esdf_d x esdf_h x esdf_w cells along x, y, z (x slowest, each <= 1024), cell centre = esdf_origin +
 * (i + 0.5 - n / 2) esdf_voxel_size, both read from the DEVICE ([3] and [1] floats).  A TSDF sample at a world position:
 * voxel (int)((p - origin) / voxel_size + N / 2) per axis, valid iff inside the grid, its block ever visible and its
 * weight > minimum_tsdf_weight; then sdf = sum / weight.
 * seed: one lane per cell; the cell is a seed iff at its centre or at +-half a cell along one axis a valid sample has
 * |sdf| <= 0.9 voxel_size or sdf < -(truncation - 1.1 voxel_size).  A seed stores x | y << 10 | z << 20, every other cell -1. */
int curobo_hip_mapper_esdf_seed(int32_t *sites, const void *block_data, const uint8_t *block_mask, const float *esdf_origin,
                                const float *esdf_voxel_size, const curobo_hip_mapper_params *params, int esdf_d, int esdf_h,
                                int esdf_w, curobo_hip_stream_t stream);

/* One of the three passes of the exact Euclidean nearest-site transform: along axis (2 = z, then 1 = y, then 0 = x) every
 * cell of a line receives the site of the line's cell j that minimises |cell - site(j)|^2 in integers (lowest j on a tie),
 * or -1 when the line holds no site.  sites_in and sites_out [esdf_d esdf_h esdf_w] must not overlap.  After the three
 * passes in that order every cell holds a nearest seed. */
int curobo_hip_mapper_edt_pass(int32_t *sites_out, const int32_t *sites_in, int esdf_d, int esdf_h, int esdf_w, int axis,
                               curobo_hip_stream_t stream);

/* distance fp16 [esdf_d esdf_h esdf_w]: 1e4 where the cell has no site, else |cell - site| esdf_voxel_size in fp32, negated
 * when the TSDF sample at the cell's own centre is valid and < 0. */
int curobo_hip_mapper_esdf_distance(void *distance, const int32_t *sites, const void *block_data, const uint8_t *block_mask,
                                    const float *esdf_origin, const float *esdf_voxel_size,
                                    const curobo_hip_mapper_params *params, int esdf_d, int esdf_h, int esdf_w,
                                    curobo_hip_stream_t stream);

/* flags uint8 [n_blocks][block_size^3]: 1 where the block was ever visible, the voxel's weight > minimum_tsdf_weight and
 * sdf <= 0 (surface_only == 0) or |sdf| < sdf_threshold (surface_only != 0), else 0. */
int curobo_hip_mapper_occupied_flags(uint8_t *flags, const void *block_data, const uint8_t *block_mask,
                                     const curobo_hip_mapper_params *params, int surface_only, float sdf_threshold,
                                     curobo_hip_stream_t stream);

/* Weight decay and block recycling (reference kernel/wp_decay.py :111-149, kernel/builder/builder_decay.py :111-215, :322-363).
 * Per block with block_mask != 0: both fp16 words of every voxel are multiplied in fp32 by the block's factor and rounded to
 * nearest even -- factor_inside where the block lies in the union of the n_cameras frusta, else factor_outside (n_cameras == 0:
 * no frustum test, factor_outside throughout; the camera pointers may be null).  The host passes the factors rounded as the
 * reference's two paths round them: float(time_decay) for the uniform path, (float)(half)time_decay and
 * (float)(half)(time_decay frustum_decay) for the frustum path.  In the frustum of camera c (wxyz pose, image height x width,
 * depth range from params): with (x, y, z) the block's centre ((b BS + BS / 2) - N / 2) voxel_size + origin in the camera frame
 * and r = 0.866 BS voxel_size: not when z + r < depth_min or z - r > depth_max; else at once when z < 0.01; else iff the disc
 * of radii fx r / z, fy r / z about (fx x / z + cx, fy y / z + cy) reaches [0, width] x [0, height].  No depth image is read.
 * Then the stored weights of the block are summed in fp32 in a fixed order; where the sum is < empty_threshold the block is
 * recycled: its words and block_mask[b] become 0.  recycled uint8 [n_blocks] is written for EVERY block: 1 where this launch
 * recycled it, else 0.  A block with block_mask == 0 is not read.  No atomics, no host read: fixed dimensions, safe in a graph.
 * Blocks of 512 voxels or more need block_data 16-byte aligned. */
int curobo_hip_mapper_decay(void *block_data, uint8_t *block_mask, uint8_t *recycled, const float *intrinsics,
                            const float *cam_position, const float *cam_quaternion, int n_cameras, int height, int width,
                            float factor_outside, float factor_inside, float empty_threshold,
                            const curobo_hip_mapper_params *params, curobo_hip_stream_t stream);

/* The same launch over the union of the frusta of n_cameras cameras AND n_lidars lidars (reference kernel/wp_decay.py :152-291,
 * builder_decay.py :217-313); either set may be empty (its pointers null) and with both empty factor_outside holds throughout.
 * lidar_position [n_lidars, 3], lidar_quaternion [n_lidars, 4] wxyz, lidar_valid_range [n_lidars, 2] = (min, max) metres,
 * lidar_elevation_range [n_lidars, 2] = (min, max) radians, lidar_height the rows of the range image (1: a planar scan).  In the
 * frustum of lidar l, with rho the range of the block's centre in the lidar frame, el = atan2(z, |xy|) its elevation and r as
 * above: not when rho + r < min or rho - r > max; else with the angular radius a = asin(r / rho) (pi when rho <= r): for
 * lidar_height == 1 iff |el - (min_el + max_el) / 2| <= a, otherwise iff el + a >= min_el and el - a <= max_el.  A lidar sees
 * every azimuth; no range image is read.  curobo_hip_mapper_decay is this entry with n_lidars = 0. */
int curobo_hip_mapper_decay_sensors(void *block_data, uint8_t *block_mask, uint8_t *recycled, const float *intrinsics,
                                    const float *cam_position, const float *cam_quaternion, int n_cameras, int height, int width,
                                    const float *lidar_position, const float *lidar_quaternion, const float *lidar_valid_range,
                                    const float *lidar_elevation_range, int n_lidars, int lidar_height, float factor_outside,
                                    float factor_inside, float empty_threshold, const curobo_hip_mapper_params *params,
                                    curobo_hip_stream_t stream);

/* ---- lidar range images into the same TSDF (csrc/mapper_lidar.hip; reference kernel/builder/builder_lidar_integrate.py :75-180,
 * :244-467).  range [n_lidars, height, width] metres is the EUCLIDEAN range from the sensor, lidar_position [n_lidars, 3],
 * lidar_quaternion [n_lidars, 4] wxyz the sensors in the world, valid_range [n_lidars, 2] = (min, max) metres, elevation_range
 * [n_lidars, 2] = (min, max) radians.  Pixel (px, py) looks along azimuth px 2 pi / width - pi (no half pixel) and elevation
 * max_el - py (max_el - min_el) / (height - 1) (min_el when height == 1): ray = (cos az cos el, sin az cos el, sin el).
 *
 * mark: one lane per (lidar, pixel, sample).  A pixel with range in [min, max] is walked along its ray from
 * max(range - truncation, min) in steps of step_size while r <= range + truncation + step_size; the block of every sample
 * lidar_position + R(q) (ray r) that falls into the grid gets 1 in lidar_mask (what the integration reads), frame_mask (the
 * frame's union with the cameras') and block_mask: plain byte stores of the same value, fp32 throughout. */
int curobo_hip_mapper_lidar_mark_blocks(uint8_t *lidar_mask, uint8_t *frame_mask, uint8_t *block_mask, const float *range,
                                        const float *lidar_position, const float *lidar_quaternion, const float *valid_range,
                                        const float *elevation_range, const curobo_hip_mapper_params *params, int n_lidars,
                                        int height, int width, curobo_hip_stream_t stream);

/* One workgroup per block, returning at once where lidar_mask is 0.  Per voxel and lidar: the centre (x, y, z) in the lidar
 * frame, its range rho in [min, max]; el = atan2(z, |xy|), for height > 1 in [min_el, max_el] and v = (max_el - el)(height - 1)
 * / (max_el - min_el), else v = 0; u = (atan2(y, x) + pi) width / (2 pi) wrapped into [0, width).  The surface range is
 * bilinear over rows floor(v), floor(v) + 1 and columns floor(u), (floor(u) + 1) mod width when height > 1, 0 <= floor(v) <
 * height - 1, all four ranges are valid and none differs from the result by more than linear_max_diff_m; else that of the
 * nearest pixel (floor(u + 0.5) wrapped, floor(v + 0.5) inside the image), valid, with the voxel within nearest_max_dist_m of
 * that pixel's ray; else the lidar contributes nothing.  sdf = surface - rho >= -truncation, clamped to truncation, weight 1.
 * (x, y, z), rho, el, u, v, the bilinear sum and the difference are evaluated in double from the fp32 inputs, with pi and 2 pi the
 * fp32 constants widened (the sdf cancels at the surface and depends on u, v through the image's slope); the ray distance is
 * fp32.  The sums over the lidars are fp32; where the summed weight is > 0 they are added to the stored pair in fp32 and
 * rounded once to fp16. */
int curobo_hip_mapper_lidar_integrate(void *block_data, const uint8_t *lidar_mask, const float *range, const float *lidar_position,
                                      const float *lidar_quaternion, const float *valid_range, const float *elevation_range,
                                      const curobo_hip_mapper_params *params, int n_lidars, int height, int width,
                                      float linear_max_diff_m, float nearest_max_dist_m, curobo_hip_stream_t stream);

/* ---- mesh extraction: marching cubes over the ever-visible blocks (reference kernel/builder/builder_mesh.py,
 * builder_raycast.py :63-375, marching_cubes/kernel/wp_mc_common.py :464-489, wp_mc_filter.py).  block_list int32 [n_slots]
 * holds the rows of the ever-visible blocks in ascending order, block_slot int32 [n_blocks] the slot of a block or -1.
 * Per-voxel arrays are [n_slots][block_size^3] in the order (slot, voxel local index): scratch grows with the visible
 * blocks, never with the grid.  A voxel is valid iff it lies in the PADDED grid, its block is ever visible and its weight
 * >= minimum_tsdf_weight; its value is s = sum / weight - level.  Cube g has corners 0..7 at the voxels g + (0,0,0) (1,0,0)
 * (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1) and edges 0..11 = 0-1 1-2 2-3 3-0 4-5 5-6 6-7 7-4 0-4 1-5 2-6 3-7.  The
 * four launches run in this order; between them the caller turns counts into exclusive prefix sums and reads the totals.
 * No launch uses an atomic: the output order is (block row, voxel local index, then axis x y z / table order).
 *
 * classify: one workgroup per (slot, tile of min(block_size, 8)^3 cubes), the tile's corner values once in LDS.  A cube is
 * a surface cube iff all eight corners are valid, some s > 0, some s < 0 and, with surface_only, some |s| < truncation.
 * cube_case = sum of (s_c < 0) << c for a surface cube, else 0; vert_count = how many of its own edges 0, 3, 8 are cut
 * (exactly one end negative); tri_count = the triangles of row cube_case of table int8 [256][16] (edge triples, then -1). */
int curobo_hip_mapper_mesh_classify(uint8_t *cube_case, uint8_t *vert_count, uint8_t *tri_count, const void *block_data,
                                    const uint8_t *block_mask, const int32_t *block_list, int n_slots, const int8_t *table,
                                    const curobo_hip_mapper_params *params, float level, int surface_only,
                                    curobo_hip_stream_t stream);

/* One lane per voxel.  vert_offset int32: the exclusive prefix sum of vert_count, n_vertices its total.  The vertex of a cut
 * edge a-b is p_a + clamp(-s_a / (s_b - s_a), 0, 1) (p_b - p_a), p the voxel CENTRES; then refine_iterations times: a
 * trilinear sample at the vertex (lower corner floor(v - 0.5) of the continuous coordinate v, an invalid corner counts as the
 * truncation distance, no valid corner = invalid); stop when it is invalid, |sdf - level| < 1e-6 or sdf - level > 100; else
 * step clamp(sdf - level, +-voxel_size / 2) against the normalised central difference of six trilinear samples at
 * +-voxel_size ((0, 0, 1) where one is invalid or the magnitude is below 1e-6).  normals: the same difference of six
 * nearest-voxel samples (voxel floor(v)) at the final position.  vertices, normals float [n_vertices][3]; vert_ids int32
 * [n_slots][block_size^3][3]: the voxel's vertices along x, y, z, -1 where it emits none. */
int curobo_hip_mapper_mesh_vertices(float *vertices, float *normals, int32_t *vert_ids, int n_vertices, const uint8_t *vert_count,
                                    const int32_t *vert_offset, const void *block_data, const uint8_t *block_mask,
                                    const int32_t *block_list, int n_slots, const curobo_hip_mapper_params *params, float level,
                                    int refine_iterations, curobo_hip_stream_t stream);

/* One lane per voxel.  tri_offset int32: the exclusive prefix sum of tri_count, n_raw its total.  Every triangle of the
 * cube's table row goes to raw_triangles int32 [n_raw][3]: a corner on edge e is vertex axis of the cube g + (dx, dy, dz),
 * (dx, dy, dz, axis) = edge_owner int8 [12][4], or -1 where that cube is outside the padded grid, in a block never visible,
 * or emits no such vertex.  keep uint8 [n_raw] = 1 iff the three are there, all different, and |(v1 - v0) x (v2 - v0)|^2 >
 * (voxel_size 1e-6)^2.  (v1 - v0) x (v2 - v0) points to the positive side when the table's rows do. */
int curobo_hip_mapper_mesh_triangles(int32_t *raw_triangles, uint8_t *keep, int n_raw, const uint8_t *cube_case,
                                     const uint8_t *tri_count, const int32_t *tri_offset, const int32_t *vert_ids,
                                     const float *vertices, int n_vertices, const int32_t *block_list, const int32_t *block_slot,
                                     int n_slots, const int8_t *table, const int8_t *edge_owner,
                                     const curobo_hip_mapper_params *params, curobo_hip_stream_t stream);

/* One lane per raw triangle: triangles int32 [n_triangles][3] = the raw triangles with keep != 0, in their order;
 * keep_offset int32 [n_raw]: the exclusive prefix sum of keep, n_triangles its total. */
int curobo_hip_mapper_mesh_compact(int32_t *triangles, int n_triangles, const int32_t *raw_triangles, const uint8_t *keep,
                                   const int32_t *keep_offset, int n_raw, curobo_hip_stream_t stream);

/* ---- the TSDF read back along camera rays (csrc/mapper_raycast.hip; reference kernel/builder/builder_raycast.py :381-834,
 * kernel/wp_raycast_pose_refine.py :100-316).  Both launches read block_data / block_mask as described above, sample
 * trilinearly (an invalid corner counts as the truncation distance, no valid corner = invalid) and take minimum_tsdf_weight
 * as an argument in place of params->minimum_tsdf_weight (a voxel is valid iff its weight >= it).  The camera -- intrinsics
 * [3][3], position [3], quaternion [4] wxyz -- is read from the DEVICE, so a replayed graph follows a moving camera.  A
 * position is compared with the grid's extent in float before any conversion to int.
 *
 * One lane per pixel, 16 x 16 pixels per workgroup.  The ray through the pixel centre ((px + 0.5 - cx) / fx, (py + 0.5 - cy)
 * / fy, 1), normalised and rotated, is marched from t = depth_minimum_distance in steps of voxel_size / 2 while t <=
 * depth_maximum_distance; a hit is the first pair of valid samples prev > 0, cur < 0, refined by ten regula-falsi iterations
 * (:381-422); the normal is the normalised central difference of six trilinear samples at the hit ((0, 0, 1) where one is
 * invalid).  accelerated == 0 is raycast_block_sparse_kernel (:467-573): an invalid sample advances t and keeps prev, at most
 * min((max - min) / step + 1, 10000) steps.  accelerated != 0 is raycast_block_sparse_accelerated_kernel (:690-834): on
 * entering a block that was never visible (a block outside the grid included) t jumps to the block's slab exit (:424-461)
 * + step and prev is forgotten, at most 10000 iterations.  The two forms sample at different t and give different depths.
 * hit_points, hit_normals float [H W][3], hit_depths float [H W], hit_mask uint8 [H W] are all written by every launch, 0
 * on a miss (:486-493).  hit_depths is the RANGE along the ray, as the reference's (its "z_depth" is hit_t * 1.0, :564,
 * :825); z_depth != 0 writes range * ray_cam.z, the depth along the camera's axis, instead.  A camera pose that is not
 * finite hits nothing. */
int curobo_hip_mapper_raycast(float *hit_points, float *hit_normals, float *hit_depths, uint8_t *hit_mask, const float *intrinsics,
                              const float *position, const float *quaternion, const void *block_data, const uint8_t *block_mask,
                              const curobo_hip_mapper_params *params, float minimum_tsdf_weight, float depth_minimum_distance,
                              float depth_maximum_distance, int height, int width, int accelerated, int z_depth,
                              curobo_hip_stream_t stream);

/* _ray_sdf_alignment_block_sparse_tiled_kernel (wp_raycast_pose_refine.py:100-316).  One lane per sample: out_H x out_W =
 * ceil(H / stride) x ceil(W / stride) pixels (out_i stride, out_j stride) of depth [H][W], n_samples_per_ray (odd, 1..9)
 * samples k = -n/2 .. n/2 each.  A pixel counts when its depth d is finite and in [depth_minimum_distance,
 * depth_maximum_distance]; its ray is ((pj - cx) / fx, (pi - cy) / fy, 1) -- no half pixel here (:171-172) -- normalised and
 * rotated, obs_t = d |ray|.  The sample at obs_t must be valid with |sdf| <= distance_threshold (:187); sample k lies at t =
 * obs_t + k voxel_size >= 0.1 (:191), expects sdf = -k voxel_size (within the truncation distance, :198), residual r = sdf -
 * expected times the Huber scale sqrt(0.05 t^2 / |r|) where |r| > 0.05 t^2 (:201-209), Jacobian row [g, g_z p_y - g_y p_z,
 * g_x p_z - g_z p_x, g_y p_x - g_x p_y] times that scale (:225-230), g the trilinear gradient at the sample p.  The 44 sums
 * the reference adds with atomics leave as rows of `workspace` (CUROBO_HIP_POSE_WS_ROW words, one per workgroup of 256
 * samples: words 0..20 J^T J, 21..26 J^T r, 27 sum r^2, 28 the count), which curobo_hip_pose_lm_step adds in order when called
 * with n_points = out_H out_W n_samples_per_ray; curobo_hip_pose_sdf_ws_bytes of that count is the size.  No atomics, nothing
 * to zero between evaluations, bit-identical from run to run.  position / quaternion: DEVICE pointers, e.g. cand_position /
 * cand_quaternion of a curobo_hip_pose_lm_state; a pose that is not finite yields no valid sample. */
int curobo_hip_mapper_ray_align(void *workspace, int64_t workspace_bytes, const float *depth, const float *intrinsics,
                                const float *position, const float *quaternion, const void *block_data, const uint8_t *block_mask,
                                const curobo_hip_mapper_params *params, float minimum_tsdf_weight, float depth_minimum_distance,
                                float depth_maximum_distance, float distance_threshold, int height, int width, int stride,
                                int n_samples_per_ray, curobo_hip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CUROBO_HIP_H */
