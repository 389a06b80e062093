"""Randomised parity of the ray launches (csrc/mapper_raycast.hip) against the float64 restatement tests/mapper_raycast_ref.py:

    python tests/randomised/fuzz_mapper_raycast.py <cases> <seed>

Random grids (block sizes 1, 2, 4 and 8, axes that are no multiple of the block), random injected states (a sphere's clipped
distance plus noise, half the blocks never visible, voxels unobserved, below and exactly at the minimum weight), cameras outside
and inside the grid, images that are no multiple of a tile.  The rules of tests/test_gpu_mapper_raycast.py through
mapper_raycast_cases.compare_render / compare_rows: both forms of the raycast -- the mask equal at every unflagged pixel, range
and normals within four times the restatement's own float32 gap, a miss zero everywhere -- and the alignment rows of the depth
image the restatement renders from a pose nearby, summed in order, within the row bound.  A case whose restatement flags more
than 3 % is drawn again (at most five times).  Exit status 0 when every case passes."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import mapper_raycast_cases as RC  # noqa: E402
import mapper_raycast_ref as RR  # noqa: E402
import mapper_ref as R  # noqa: E402

DEV = "cuda:0"


def one_case(rng) -> str:
    from curobo_amd.backends import mapper as B
    from curobo_amd.backends import perception as P
    from curobo_amd.perception.mapper import Mapper, MapperCfg

    bs = int(rng.choice([1, 2, 4, 8]))
    vs = float(rng.choice([0.02, 0.025, 0.04]))
    n_vox = rng.integers(12, 33, 3)
    extent = tuple(float(n * vs - 0.25 * vs) for n in n_vox)
    H, W = int(rng.integers(9, 40)), int(rng.integers(9, 50))
    cfg = MapperCfg(extent_meters_xyz=extent, voxel_size=vs, esdf_voxel_size=2 * vs, extent_esdf_meters_xyz=extent,
                    truncation_distance=float(rng.uniform(2.5, 5.0)) * vs, block_size=bs, image_height=H, image_width=W,
                    grid_center=[float(v) for v in rng.uniform(-0.05, 0.05, 3)])
    g = R.Grid.from_cfg(cfg)
    mapper = Mapper(cfg, use_graph=False)
    t = mapper.tsdf
    dev = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    for _ in range(5):
        sw, w, visible = RC.injected_state(g, int(rng.integers(1 << 30)))
        t.block_data.copy_(dev(np.stack([sw, w], -1)))
        t.block_visible.zero_()
        t.block_visible[: g.n_blocks] = dev(visible.astype(np.uint8))
        f = float(rng.uniform(0.5, 1.2)) * W
        K = np.array([[f, 0, 0.5 * W + rng.uniform(-0.4, 0.4)], [0, f * rng.uniform(0.9, 1.1), 0.5 * H + rng.uniform(-0.4, 0.4)], [0, 0, 1]], np.float32)
        eye = rng.normal(size=3)
        eye = eye / np.linalg.norm(eye) * (rng.uniform(0.6, 1.2) if rng.random() < 0.7 else rng.uniform(0.05, 0.2))  # outside / inside
        pos = eye.astype(np.float32)
        quat = R.look_at(eye, rng.uniform(-0.05, 0.05, 3), float(rng.uniform(-0.6, 0.6))).astype(np.float32)
        t_min, t_max, mw = float(rng.uniform(0.05, 0.2)), float(rng.uniform(1.5, 2.5)), RC.INJECTED_MIN_WEIGHT
        refs = [RR.raycast(g, sw, w, visible, K, pos, quat, H, W, t_min, t_max, mw, acc) for acc in (0, 1)]
        # the alignment: the depth image of the plain form seen from here, the pose a little off, every pixel or every second
        n_samples, stride = int(rng.choice([1, 3, 5])), int(rng.choice([1, 2]))
        depth = (refs[0]["depth"] * refs[0]["ray_cam_z"]).reshape(H, W).astype(np.float32)
        pos2 = (pos + rng.uniform(-0.01, 0.01, 3)).astype(np.float32)
        align = RR.ray_align(g, sw, w, visible, depth, K, pos2, quat, stride, n_samples, t_min, t_max, 2.0 * g.vs, mw)
        if max(refs[0]["ambiguous"].mean(), refs[1]["ambiguous"].mean(), align["ambiguous"].mean()) <= RC.AMBIGUOUS_CAP:
            break
    else:
        return "five draws in a row with more than 3 % flagged"
    for acc, ref in enumerate(refs):
        n = H * W
        out = (torch.full((n, 3), 5.0, device=DEV), torch.full((n, 3), 5.0, device=DEV), torch.full((n,), 5.0, device=DEV),
               torch.full((n,), 5, dtype=torch.uint8, device=DEV))
        B.mapper_raycast(*out, dev(K), dev(pos), dev(quat), t.block_data, t.block_visible, t.params, mw, t_min, t_max, (H, W), acc)
        torch.cuda.synchronize()
        msg = RC.compare_render(*(o.cpu().numpy() for o in out), ref)
        if msg:
            return f"raycast, accelerated {acc}, block size {bs}, {H} x {W}: {msg}"
    ws = torch.full((P.pose_sdf_ws_bytes(B.ray_align_samples((H, W), stride, n_samples)) // 4,), 5.0, device=DEV)
    B.mapper_ray_align(ws, dev(depth), dev(K), dev(pos2), dev(quat), t.block_data, t.block_visible, t.params, mw, t_min, t_max, 2.0 * g.vs, stride,
                       n_samples)
    torch.cuda.synchronize()
    msg = RC.compare_rows(ws.cpu().numpy().reshape(-1, 32), align, g.trunc)
    return f"alignment, block size {bs}, {H} x {W}, stride {stride}, {n_samples} per ray: {msg}" if msg else ""


def main(cases: int, seed: int) -> int:
    failed = 0
    for c in range(cases):
        rng = np.random.default_rng([seed, c])
        msg = one_case(rng)
        if msg:
            failed += 1
            print(f"case {c} (seed {seed}): {msg}")
    print(f"fuzz_mapper_raycast: {cases} cases, {failed} failed")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]) if len(sys.argv) > 1 else 16, int(sys.argv[2]) if len(sys.argv) > 2 else 0))
