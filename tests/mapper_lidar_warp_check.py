"""The float64 restatement tests/mapper_lidar_ref.py against the reference's own ``lidar_compute_block_keys_only_kernel``,
``lidar_integrate_voxels_kernel`` (perception/mapper/kernel/builder/builder_lidar_integrate.py) and
``mark_lidar_blocks_in_frustum_kernel`` (builder_decay.py), all unmodified and wired to the reference's own coordinate and hash
functions (builder_coord.py, builder_hash.py), run thread by thread in fp32 through tests/golden/warp_emulator on the lidar tests'
scene (tests/mapper_lidar_cases.py): sensor A and the planar sensor P through marking and integration, the decay tests' lidars
through the frustum kernel at block sizes 2, 4 and 8.

On everything the restatement is sure of the kernels must give its answer: sure blocks are marked and nothing outside the possible
ones; on the voxels of those blocks that are not ambiguous the same voxels are updated, with weight exactly 1 and the stored
sdf within FP32_SDF = 2e-6 m of the restatement's -- the kernel's fp32 position in the sensor frame (a few ulp of 1 m), range, two
atan2 and bilinear sum, worked out generously -- plus the fp16 word's own rounding; every sure frustum flag is the kernel's.
CPU only; needs the reference tree and says so where it is absent.  Run by tests/test_mapper_lidar_host.py in a process of its own,
because the reference's package is called ``curobo`` like this repository's facade.
    python tests/mapper_lidar_warp_check.py"""
import os
import sys

import numpy as np

REFERENCE = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not os.path.isdir(os.path.join(REFERENCE, "curobo", "_src", "perception", "mapper")):
    print("no reference tree here: nothing to compare; 0 failed")
    sys.exit(0)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, REFERENCE)
import make_scene_warp_golden as _emu  # noqa: E402,F401  (the Warp stand-in + module stubs)
import warp as wp  # noqa: E402
from curobo._src.perception.mapper.kernel.builder.builder_coord import make_coord_kernels  # noqa: E402
from curobo._src.perception.mapper.kernel.builder.builder_decay import make_decay_kernels  # noqa: E402
from curobo._src.perception.mapper.kernel.builder.builder_hash import make_hash_kernels  # noqa: E402
from curobo._src.perception.mapper.kernel.builder.builder_lidar_integrate import make_lidar_integrate_kernels  # noqa: E402

import mapper_cases as C  # noqa: E402
import mapper_lidar_cases as LC  # noqa: E402
import mapper_lidar_ref as LR  # noqa: E402

FP32_SDF = 2e-6
bad = compared = 0


def f32(a, **kw):
    return wp.array(np.ascontiguousarray(np.asarray(a, np.float32)), dtype=wp.float32, **kw)


def key_coords(g):
    """the reference's centred block keys of every dense block row: key = index - blocks // 2 (builder_coord.py:86-102)"""
    nbx, nby, nbz = g.nb
    b = np.arange(g.n_blocks)
    return np.stack([b % nbx - nbx // 2, (b // nbx) % nby - nby // 2, b // (nbx * nby) - nbz // 2], -1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------- marking and integration
g = LC.grid()
keys = key_coords(g)
hash_k = make_hash_kernels(g.bs)
coord_k = make_coord_kernels(g.bs, grid_shape=(g.nz, g.ny, g.nx), origin_xyz=tuple(g.origin), voxel_size=g.vs)


def pack_key_only(bx, by, bz):
    """the reference's pack_key_only with its result wrapped to a signed 64-bit word, as Warp's int64 is: the emulator's int64 is
    an unbounded Python int, and a key with its top bit set does not fit the int64 array the kernel stores it in"""
    key = int(hash_k["pack_key_only"](bx, by, bz)) & 0xFFFFFFFFFFFFFFFF
    return wp.int64(key - (1 << 64) if key >> 63 else key)


packed = {int(pack_key_only(wp.int32(int(k[0])), wp.int32(int(k[1])), wp.int32(int(k[2])))): row for row, k in enumerate(keys)}
assert len(packed) == g.n_blocks
for name in ("A", "P"):
    rng, pos, quat, valid_range, elev_range = LC.frame(name)
    n, H, W = rng.shape
    # the builder's plain @wp.func closures (_range_valid, ...) are new functions at every build; the emulator files functions by
    # module and name and would take a second build's for overloads of the first's
    wp._functions.clear()
    kernels = make_lidar_integrate_kernels(
        g.bs, feature_dim=0, lidar_num_sensors=n, lidar_image_height=H, lidar_image_width=W, num_samples=g.num_samples,
        grid_shape=(g.nz, g.ny, g.nx), origin_xyz=tuple(g.origin), voxel_size=g.vs, truncation_distance=g.trunc, lidar_feature_grid_shape=None,
        feature_channels_per_thread=1, max_feature_tile_channels=1, max_support_pixels_per_block_lidar=8, pack_key_only=pack_key_only,
        unpack_block_key=hash_k["unpack_block_key"], hash_lookup=hash_k["hash_lookup"], world_to_continuous_voxel=coord_k["world_to_continuous_voxel"],
        block_local_to_world=coord_k["block_local_to_world"], block_grid_to_key_coords=coord_k["block_grid_to_key_coords"])
    sensors = [f32(pos, ndim=2), f32(quat, ndim=2), f32(rng, ndim=3), f32(valid_range, ndim=2), f32(elev_range, ndim=2)]
    n_threads = n * H * W * g.num_samples
    block_keys = np.full(n_threads, -2, np.int64)
    wp.launch(kernels["lidar_compute_block_keys_only_kernel"], dim=n_threads, inputs=[*sensors, wp.array(block_keys, dtype=wp.int64)])
    marked = np.zeros(g.n_blocks, bool)
    for k in np.unique(block_keys):
        if k != -1:
            marked[packed[int(k)]] = True
    sure, possible = LR.mark_blocks(g, rng, pos, quat, valid_range, elev_range)
    wrong = int((sure & ~marked).sum() + (marked & ~possible).sum())
    print(f"sensor {name}: {int(marked.sum())} blocks marked by the kernel, {int(sure.sum())} sure, {int(possible.sum())} possible, {wrong} disagree")
    bad += wrong
    compared += g.n_blocks
    assert sure.sum() >= 20 and (possible & ~sure).sum() <= 0.01 * possible.sum()

    rows = np.nonzero(sure)[0].astype(np.int32)
    data = np.zeros((g.n_blocks, g.bs ** 3, 2), np.float16)
    wp.launch(kernels["lidar_integrate_voxels_kernel"], dim=(len(rows), g.bs ** 3),
              inputs=[wp.array(rows, dtype=wp.int32), len(rows), *sensors, LC.LINEAR_MAX_DIFF, LC.NEAREST_MAX_DIST,
                      wp.array(keys.reshape(-1), dtype=wp.int32), wp.array(data, dtype=wp.float16, ndim=3)])
    zero = np.zeros(data.shape[:2], np.float16)
    sw, w, upd, amb = LR.integrate(g, zero, zero, sure, rng, pos, quat, valid_range, elev_range, LC.LINEAR_MAX_DIFF, LC.NEAREST_MAX_DIST)
    keep = sure[:, None] & ~amb
    got_upd = data[..., 1] != 0
    wrong_upd = int((got_upd != upd)[keep].sum())
    both = keep & upd & got_upd
    wrong_w = int((data[..., 1][both] != w[both]).sum())
    want, got = sw.astype(np.float64)[both], data[..., 0].astype(np.float64)[both]
    gap = np.abs(got - want) - np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)
    wrong_sdf = int((gap > FP32_SDF).sum())
    print(f"sensor {name}: {int(upd[keep].sum())} voxels updated on {int(keep.sum())} compared ({float((~keep)[sure].mean()):.4f} of the sure blocks' "
          f"voxels excluded), {wrong_upd} updated otherwise, {wrong_w} weights differ, largest sdf gap beyond an fp16 step "
          f"{float(gap.max()):.2e} m, {wrong_sdf} above {FP32_SDF} m")
    bad += wrong_upd + wrong_w + wrong_sdf
    compared += int(keep.sum())
    assert upd[keep].sum() >= 200 and (~keep)[sure].mean() <= 0.01

# ---------------------------------------------------------------------------------------------------- the decay's lidar frustum
for bs in (2, 4, 8):
    g = LC.grid(bs)
    keys = key_coords(g).reshape(-1)
    kernels = make_decay_kernels(bs, grid_shape=(g.nz, g.ny, g.nx), origin_xyz=tuple(g.origin), voxel_size=g.vs, num_cameras=1,
                                 image_height=C.H, image_width=C.W, free_list_push=lambda *a: None)
    for name in LC.DECAY_LIDARS:
        pos, quat, valid_range, elev_range, H = LC.decay_lidars(name)
        flags = np.zeros(g.n_blocks, np.int32)
        wp.launch(kernels["mark_lidar_blocks_in_frustum_kernel"], dim=(g.n_blocks, len(pos)),
                  inputs=[wp.array(keys, dtype=wp.int32), wp.array(np.zeros(g.n_blocks, np.int32), dtype=wp.int32),
                          wp.array(np.array([g.n_blocks], np.int32), dtype=wp.int32), f32(pos, ndim=2), f32(quat, ndim=2), f32(valid_range, ndim=2),
                          f32(elev_range, ndim=2), int(H), wp.array(flags, dtype=wp.int32), g.n_blocks])
        sure_in, sure_out = LR.frustum_flags(g, lidars=(pos, quat, valid_range, elev_range, H))
        wrong = int((sure_in & (flags == 0)).sum() + (sure_out & (flags != 0)).sum())
        either = int((~sure_in & ~sure_out).sum())
        print(f"block size {bs}, lidars '{name}': {int((flags != 0).sum())} of {g.n_blocks} blocks flagged by the kernel, {int(sure_in.sum())} sure in, "
              f"{int(sure_out.sum())} sure out, {either} either, {wrong} disagree")
        bad += wrong
        compared += int(sure_in.sum() + sure_out.sum())
        assert sure_in.sum() >= 20 and sure_out.sum() >= 20 and either <= 0.01 * g.n_blocks
print(f"{compared} answers compared, {bad} failed")
sys.exit(1 if bad else 0)
