"""The scene-collision kernel against the oracle on random voxel stores: one to three grids per environment with 1 to 12
voxels per axis (thin grids included), rotated poses, fields truncated at a random max_distance, a random coarse aid, straight
trajectories through and around the grids; discrete (tight everywhere) and swept + speed metric -- the comparison of
fuzz_scene.py.   python tests/randomised/fuzz_voxel.py [cases] [seed]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxel_cases as VC  # noqa: E402

from curobo_amd.backends import collision as Cn  # noqa: E402
from curobo_amd.scene import SceneData  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

dev = torch.device("cuda:0")
oracle = Oracle()
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)


def random_grid(md):
    shape = tuple(int(v) for v in rng.integers(1, 13, 3))
    vs = float(rng.choice([0.03, 0.05, 0.0625]))
    q = rng.normal(size=4)
    pose = [*rng.uniform(-0.3, 0.3, 3), *(q / np.linalg.norm(q))]
    ext = np.asarray(shape) * vs
    balls = [VC.ball(rng.uniform(-0.5, 0.5, 3) * ext, float(rng.uniform(0.5, 2.5)) * vs) for _ in range(int(rng.integers(1, 4)))]
    g = VC.make_grid(shape, pose, VC.union(*balls), vs=vs, clip=md, enable=bool(rng.random() > 0.1))
    VC.assert_lipschitz(g)
    return g


bad = 0
for case in range(n_cases):
    sweep = bool(rng.random() < 0.5)
    speed = sweep and bool(rng.random() < 0.6)
    md = float(rng.choice([0.08, 0.125, 10.0]))
    eta = float(rng.choice([0.0, 0.0025, 0.02]))
    w = float(rng.choice([1.0, 3.0, 1e5]))
    coarse = bool(rng.random() < 0.5)
    n_env = int(rng.integers(1, 3))
    envs = [[random_grid(md) for _ in range(int(rng.integers(1, 4)))] for _ in range(n_env)]
    arrays = VC.stack_voxel_grids(envs, max_distance=md, n_slots=3)
    b, h, S = int(rng.integers(1, 24)), int(rng.integers(2, 12)), int(rng.integers(1, 9))
    env_idx = rng.integers(0, n_env, b).astype(np.int32)
    sph = np.zeros((b, h, S, 4), np.float32)
    for row in range(b):  # straight lines through (or past) a random grid of the row's environment
        g = [envs[env_idx[row]][k] for k in rng.integers(0, len(envs[env_idx[row]]), S)]
        ext = np.array([np.asarray(x["shape"]) * x["voxel_size"] for x in g])
        mid = np.array([VC.grid_to_world(x["pose"], rng.uniform(-0.8, 0.8, 3) * e) for x, e in zip(g, ext)])
        d = rng.normal(size=(S, 3))
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        step = rng.uniform(0.2, 6.0, S) * np.array([x["voxel_size"] for x in g])  # (>= 6 mm: no sphere rests up to rounding)
        sph[row, ..., :3] = mid[None] + (np.arange(h) - h // 2)[:, None, None] * step[None, :, None] * d[None]
        sph[row, ..., 3] = rng.choice([0.01, 0.03, 0.06, 0.11], S)[None]
    ref = oracle.scene_collision(sph, arrays, w, eta, sweep=sweep, enable_speed_metric=speed, speed_dt=0.05, env_query_idx=env_idx, use_multi_env=True)
    scene = SceneData.from_arrays(arrays, dev, coarse_culling=coarse)
    dist, grad = torch.full((b, h, S), 5.0, device=dev), torch.full((b, h, S, 4), 5.0, device=dev)
    Cn.sphere_obstacle_collision(dist, grad, torch.as_tensor(sph, device=dev), scene.struct, torch.tensor([w], device=dev), torch.tensor([eta], device=dev),
                                 torch.as_tensor(env_idx, device=dev), b, h, S, True, 3 if sweep else 0, speed, torch.tensor([0.05], device=dev))
    torch.cuda.synchronize()
    d, g = dist.cpu().numpy(), grad.cpu().numpy()
    dr, gr = ref["distance"], ref["gradient"]
    sc = (20.0 if speed else 1.0) * w
    graze = np.abs(d - dr) < 2e-5 * sc
    try:
        assert np.array_equal((d > 0)[~graze], (dr > 0)[~graze]), "hit set differs"
        e = np.abs(d - dr)
        tol = 3e-5 * sc + 2e-4 * np.abs(dr)
        n_off = int((e > tol).sum())
        allowed = (2 + int(1e-4 * (dr > 0).sum())) if sweep else 0  # fuzz_scene.py's: the sweep's `jump >= half_dist` within rounding
        assert n_off <= allowed, f"{n_off} spheres beyond the cost bound (allowed {allowed}), worst {float((e / tol).max()):.1f} x the bound; colliding {int((dr > 0).sum())}"
        eg = np.abs(g - gr).max(-1)
        tolg = 3e-4 * sc + 2e-3 * np.abs(gr).max(-1)
        n_goff = int((eg > tolg).sum())
        assert n_goff <= allowed + int(2e-3 * (dr > 0).sum()), f"{n_goff} spheres beyond the gradient bound, worst {float((eg / tolg).max()):.1f} x"
    except AssertionError as ex:
        bad += 1
        print(f"FAILED case {case}: sweep {sweep} speed {speed} md {md} eta {eta} w {w} coarse {coarse} envs {n_env} b {b} h {h} S {S}: {str(ex)[:300]}")
print(f"{n_cases} cases, {bad} failed")
