"""Randomised parity of the depth mapper (csrc/mapper.hip) against the float64 oracle tests/mapper_ref.py:

    python tests/randomised/fuzz_mapper.py <cases> <seed>

Random grids (block sizes 2, 4 and 8, axes that are no multiple of the block), camera poses around the scene of
tests/mapper_cases.py, depth images with holes, one or two cameras, two frames per case.  The rules of tests/test_gpu_mapper.py:
the frame's blocks between the oracle's sure and possible sets; on blocks whose visibility was certain and voxels that are not
ambiguous, which voxels were updated exact and the fp16 pair within k fp16 steps after k frames; then the ESDF of the device's
own TSDF: outside the cells the oracle flags, the seed set and the sign exact, the squared distance to the returned site equal
to the exact transform's, the fp16 field within one step.  Exit status 0 when every case passes."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import mapper_ref as R  # noqa: E402

DEV = "cuda:0"


def one_case(rng) -> str:
    from curobo_amd.backends import mapper as B
    from curobo_amd.perception.mapper import Mapper, MapperCfg
    from curobo_amd.types import CameraObservation, Pose

    bs = int(rng.choice([2, 4, 8]))
    vs = float(rng.choice([0.02, 0.025, 0.04]))
    n_vox = rng.integers(9, 41, 3)
    evs = vs * float(rng.choice([1.0, 1.5, 2.0]))
    extent = tuple(float(n * vs - 0.25 * vs) for n in n_vox)
    H, W = int(rng.integers(20, 49)), int(rng.integers(24, 65))
    n_cam = int(rng.integers(1, 3))
    cfg = MapperCfg(extent_meters_xyz=extent, voxel_size=vs, esdf_voxel_size=evs, extent_esdf_meters_xyz=tuple(e * float(rng.uniform(0.7, 1.2)) for e in extent),
                    truncation_distance=float(rng.uniform(2.5, 5.0)) * vs, block_size=bs, image_height=H, image_width=W, num_cameras=n_cam,
                    depth_minimum_distance=float(rng.uniform(0.05, 0.3)), depth_maximum_distance=float(rng.uniform(2.0, 6.0)),
                    grid_center=[float(v) for v in rng.uniform(-0.05, 0.05, 3)])
    assert tuple(cfg.grid_shape[::-1]) == tuple(int(n) for n in n_vox)
    g = R.Grid.from_cfg(cfg)
    mapper = Mapper(cfg, use_graph=False)
    radius, ground = float(rng.uniform(0.1, 0.3)), float(rng.uniform(-0.3, -0.1))
    sw, w = np.zeros((g.n_blocks, bs ** 3), np.float16), np.zeros((g.n_blocks, bs ** 3), np.float16)
    clean, amb, ever_sure = np.ones(g.n_blocks, bool), np.zeros(sw.shape, bool), np.zeros(g.n_blocks, bool)
    for k in (1, 2):
        n = int(rng.integers(1, n_cam + 1))
        f = float(rng.uniform(25.0, 70.0))
        K = np.array([[f, 0, 0.5 * W + rng.uniform(-0.4, 0.4)], [0, f * rng.uniform(0.9, 1.1), 0.5 * H + rng.uniform(-0.4, 0.4)], [0, 0, 1]], np.float32)
        pos, quat, depth = [], [], []
        for _ in range(n):
            eye = rng.normal(size=3)
            eye = eye / np.linalg.norm(eye) * rng.uniform(0.6, 1.4)
            eye[2] = abs(eye[2]) + 0.05
            q = R.look_at(eye, rng.uniform(-0.08, 0.08, 3), float(rng.uniform(-0.6, 0.6))).astype(np.float32)
            holes = rng.random((H, W)) < rng.uniform(0.0, 0.3)
            pos.append(eye.astype(np.float32)), quat.append(q)
            depth.append(R.render_depth(K, pos[-1], q, H, W, radius, ground, holes))
        depth, Ks, pos, quat = np.stack(depth), np.stack([K] * n), np.stack(pos), np.stack(quat)
        t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
        mapper.integrate(CameraObservation(depth_image=t(depth), intrinsics=t(Ks), pose=Pose(t(pos), t(quat))))
        torch.cuda.synchronize()
        sure, possible = R.mark_blocks(g, depth, Ks, pos, quat)
        data = mapper.tsdf.block_data.cpu().numpy()
        frame = mapper.tsdf.frame_visible.cpu().numpy()[: g.n_blocks] != 0
        if not ((sure <= frame).all() and (frame <= possible).all()):
            return f"frame {k}: the device's {int(frame.sum())} blocks are not between the {int(sure.sum())} sure and {int(possible.sum())} possible"
        new_sw, new_w, upd, a = R.integrate(g, sw, w, sure, depth, Ks, pos, quat)
        clean &= sure | ~possible
        amb |= a
        ever_sure |= sure
        keep = clean[:, None] & ~amb
        changed = (data[..., 0] != dev_prev[0]) | (data[..., 1] != dev_prev[1]) if k > 1 else (data[..., 1] != 0)
        if not np.array_equal(changed[keep], upd[keep]):
            return f"frame {k}: {int((changed[keep] != upd[keep]).sum())} voxels updated on one side only"
        steps = max(int(R.half_steps(data[..., 0], new_sw)[keep].max()), int(R.half_steps(data[..., 1], new_w)[keep].max()))
        if steps > k:
            return f"frame {k}: {steps} fp16 steps from the oracle"
        sw, w, dev_prev = new_sw, new_w, (data[..., 0].copy(), data[..., 1].copy())
    # the ESDF of the device's own TSDF, the window a random fraction of a voxel off the grid's centre
    ever = mapper.tsdf.block_visible.cpu().numpy()[: g.n_blocks] != 0
    shape = tuple(int(v) for v in cfg.esdf_grid_shape)
    origin = (np.asarray(g.origin) + rng.uniform(-0.4, 0.4, 3) * vs).astype(np.float32)
    out = mapper.compute_esdf(esdf_origin=torch.as_tensor(origin)).feature_tensor.cpu().numpy()
    ref = R.esdf(g, data[..., 0], data[..., 1], ever, shape, origin.astype(np.float64), float(np.float32(evs)))
    sites = torch.empty(int(np.prod(shape)), dtype=torch.int32, device=DEV)
    tt = mapper.tsdf
    B.mapper_esdf_seed(sites, tt.block_data, tt.block_visible, mapper._esdf_origin, mapper._esdf_voxel_size, tt.params, shape)
    seeds = sites.cpu().numpy().reshape(shape) >= 0
    ok = ~ref["ambiguous"]
    if not np.array_equal(seeds[ok], ref["seed"][ok]):
        return f"ESDF: {int((seeds[ok] != ref['seed'][ok]).sum())} cells seeded on one side only"
    # the transform and the distance on the DEVICE's seed set (the sets may differ on flagged cells)
    d2, _ = R.edt(seeds)
    nearest = B.mapper_edt(sites, torch.empty_like(sites), shape).cpu().numpy().reshape(shape)
    cells = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1)
    got_d2 = np.where(nearest < 0, -1, ((cells - R.unpack_sites(nearest)) ** 2).sum(-1))
    if not np.array_equal(got_d2, d2):
        return f"ESDF: {int((got_d2 != d2).sum())} cells with a site that is not a nearest one"
    want, inside = R.distance(g, data[..., 0], data[..., 1], ever, d2, origin.astype(np.float64), float(np.float32(evs)))
    if not np.array_equal(np.signbit(out)[ok], inside[ok]):
        return "ESDF: sign differs on unflagged cells"
    if int(R.half_steps(np.abs(out), np.abs(want)).max()) > 1:
        return f"ESDF: {int(R.half_steps(np.abs(out), np.abs(want)).max())} fp16 steps from the oracle"
    return ""


def main(cases: int, seed: int) -> int:
    failed = 0
    for c in range(cases):
        rng = np.random.default_rng([seed, c])
        msg = one_case(rng)
        if msg:
            failed += 1
            print(f"case {c} (seed {seed}): {msg}")
    print(f"fuzz_mapper: {cases} cases, {failed} failed")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 16, int(sys.argv[2]) if len(sys.argv) > 2 else 0))
