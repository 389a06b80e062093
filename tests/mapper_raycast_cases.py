"""What the raycast tests share (tests/test_oracle_mapper_raycast.py on the CPU, tests/test_gpu_mapper_raycast.py on the device):
the two TSDF states over the grid of tests/mapper_cases.py, the views, the references (computed once, cached) and the bounds.

The bounds.  GAP_RANGE and GAP_NORMAL are the float32-against-float64 gap of the restatement itself (tests/mapper_raycast_ref.py) over
exactly these states and views, ANALYTIC_RANGE_ERROR its error against the exact scene: the measured values, rounded up in the last
digit.  tests/test_oracle_mapper_raycast.py measures them again and asserts that each lies within 1 % below its constant.  The device is
held to 4 x the gaps (fused multiply-adds and the 2.5 ulp divide and root, the margin of the support-polygon tests), to
2 x ANALYTIC_RANGE_ERROR, and to twice the distance from the truth that the float64 restatement's own refiner (refiner_ref) leaves
(docs/NOTEBOOK.md has the measured values)."""

from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import mapper_cases as C
import mapper_raycast_ref as RR
import mapper_ref as R

GAP_RANGE = 5.91e-6        # metres (measured 5.908e-6)
GAP_NORMAL = 6.12e-5       # per component of the unit normal (measured 6.115e-5)
#: ``roundings`` of pose_rows.row_bound for the alignment rows.  A term is a product of two of g hs, (g x p) hs, r hs.  The position
#: under a sample is off by a few ulp of a coordinate of 1..2 m, 2e-7 m, which the trilinear form hands on one to one: a residual of
#: the typical 1e-2 m is then good to 2e-5 = 340 x 2^-24 of itself, a gradient component (a difference of two samples over two voxels)
#: to 1e-5 = 170 x 2^-24 of the unit gradient; two factors and the Huber root: 1024.  The float32 restatement is held to the same.
ALIGN_ROUNDINGS = 1024
ANALYTIC_RANGE_ERROR = 1.175e-2  # metres, both forms, away from the silhouette and the junction (measured 1.1743e-2)
AMBIGUOUS_CAP = 0.03

T_MIN, T_MAX = 0.1, 2.0    # the parity views march 0.1 .. 2 m: every view's rays have left the grid by then
VH, VW = 30, 40
#: a 40 x 30 camera; VIEW_K_CENTRED has its principal point on a pixel centre, so that pixel's ray is the camera's axis exactly
VIEW_K = np.array([[30.0, 0.0, 20.3], [0.0, 30.0, 14.6], [0.0, 0.0, 1.0]], np.float32)
VIEW_K_CENTRED = np.array([[30.0, 0.0, 20.5], [0.0, 30.0, 14.5], [0.0, 0.0, 1.0]], np.float32)


def _look(eye, roll):
    return np.asarray(eye, np.float32), R.look_at(eye, (0.03, -0.02, -0.05), roll).astype(np.float32)


#: name -> (K, position, quaternion wxyz).  "down" looks along -z from above: the quaternion (0, 1, 0, 0) is exact in float32 and
#: the rays of the pixel column / row through the principal point have components that are exactly 0
VIEWS = {
    "outside": (VIEW_K, *_look(C.EYES[2][0], C.EYES[2][1])),
    "inside": (VIEW_K, *_look((0.41, -0.37, 0.13), 0.4)),
    "down": (VIEW_K_CENTRED, np.array([0.013, -0.021, 0.9], np.float32), np.array([0.0, 1.0, 0.0, 0.0], np.float32)),
}
INJECTED_MIN_WEIGHT = 0.125  # exact in fp16: some injected weights EQUAL it


@lru_cache(maxsize=None)
def grid() -> "R.Grid":
    from curobo_amd.perception.mapper import MapperCfg

    return R.Grid.from_cfg(MapperCfg(**C.CFG))


@lru_cache(maxsize=None)
def integrated_state():
    """(sw, w, visible) of the oracle after the three frames of mapper_cases.FRAMES"""
    run = C.oracle_run(grid())
    visible = np.zeros(grid().n_blocks, bool)
    for f in run:
        visible |= f["sure"]
    return run[-1]["sw"], run[-1]["w"], visible


def injected_state(g: "R.Grid", seed: int):
    """a random state: a sphere's clipped distance plus noise of a fifth of a voxel, half the blocks never visible, a tenth of the
    voxels unobserved or below INJECTED_MIN_WEIGHT, three voxels exactly at it (every ray that reads one is flagged)"""
    rng = np.random.default_rng(seed)
    c = g.voxel_centres()
    centre, radius = rng.uniform(-0.1, 0.1, 3), rng.uniform(0.15, 0.3)
    sdf = np.clip(np.linalg.norm(c - centre, axis=-1) - radius + rng.uniform(-0.2, 0.2, c.shape[:2]) * g.vs, -g.trunc, g.trunc)
    kind = rng.random(c.shape[:2])
    w = np.select([kind < 0.05, kind < 0.10], [0.0, 0.0625], rng.integers(1, 40, c.shape[:2]) * 0.5).astype(np.float16)
    w.reshape(-1)[rng.integers(0, w.size, 3)] = INJECTED_MIN_WEIGHT
    sw = (sdf * w.astype(np.float64)).astype(np.float16)
    return sw, w, rng.random(g.n_blocks) < 0.5


def state(name: str):
    """(sw, w, visible, minimum weight) of "integrated" or "injected" over grid()"""
    if name == "integrated":
        return (*integrated_state(), grid().min_weight)
    return (*_injected(), INJECTED_MIN_WEIGHT)


@lru_cache(maxsize=None)
def _injected():
    return injected_state(grid(), 7)


@lru_cache(maxsize=None)
def render_ref(state_name: str, view: str, accelerated: int, double: bool = True):
    sw, w, visible, mw = state(state_name)
    K, pos, quat = VIEWS[view]
    return RR.raycast(grid(), sw, w, visible, K, pos, quat, VH, VW, T_MIN, T_MAX, mw, accelerated, np.float64 if double else np.float32)


# ---------------------------------------------------------------------------------------------------- analytic truth: camera 2
@lru_cache(maxsize=None)
def camera2_ref(accelerated: int):
    """the full 80 x 60 view of camera 2, which integrated nothing, over the integrated state with the mapper's own range"""
    sw, w, visible, mw = state("integrated")
    K, pos, quat, _ = C.camera(2)
    g = grid()
    return RR.raycast(g, sw, w, visible, K, pos, quat, C.H, C.W, g.depth_min, g.depth_max, mw, accelerated, np.float64)


@lru_cache(maxsize=None)
def camera2_truth():
    """(exact range [H W], pixels to compare): a pixel is compared when its 5 x 5 neighbourhood meets one surface only (two
    voxels at this camera are under two pixels: away from the silhouette and from the junction of sphere and ground) and every
    pixel of it hits in the float64 restatement of both forms"""
    K, pos, quat, _ = C.camera(2)
    ray = RR.camera_rays(K, quat, C.H, C.W, True, np.float64)[0]
    exact, which = RR.sphere_ground_range(pos.astype(np.float64), ray)
    label = np.where(np.isfinite(exact), which, -1).reshape(C.H, C.W)
    hit = (camera2_ref(0)["mask"] & camera2_ref(1)["mask"]).reshape(C.H, C.W)
    keep = hit.copy()
    for di in range(-2, 3):
        for dj in range(-2, 3):
            sl = np.roll(np.roll(label, di, 0), dj, 1)
            sh = np.roll(np.roll(hit, di, 0), dj, 1)
            keep &= (sl == label) & sh
    keep[:2], keep[-2:], keep[:, :2], keep[:, -2:] = False, False, False, False
    # the map holds a surface only where a camera that integrated saw it: the exact hit point is in the image of camera 0 or 1, two
    # pixels from its border, nothing in front of it, seen at more than 17 degrees off the surface (a projective TSDF has no
    # band to speak of where its camera grazes), and two voxels inside the grid
    point = pos.astype(np.float64) + ray * np.where(np.isfinite(exact), exact, 0.0)[:, None]
    g = grid()
    extent = 0.5 * np.array([g.nx, g.ny, g.nz]) * g.vs - 2 * g.vs
    seen = np.zeros(len(point), bool)
    normal = np.where((which == 1)[:, None], np.array([0.0, 0.0, 1.0]), point / R.SPHERE_RADIUS)
    for i in (0, 1):
        Ki, pi, qi, _ = C.camera(i)
        d = point - pi.astype(np.float64)
        rng_i = np.linalg.norm(d, axis=-1)
        first, _ = RR.sphere_ground_range(pi.astype(np.float64), d / rng_i[:, None])
        pc = R.quat_rotate(qi.astype(np.float64) * np.array([1.0, -1.0, -1.0, -1.0]), d)
        u, v = Ki[0, 0] * pc[:, 0] / pc[:, 2] + Ki[0, 2], Ki[1, 1] * pc[:, 1] / pc[:, 2] + Ki[1, 2]
        facing = -(normal * d).sum(-1) / rng_i > 0.3
        seen |= facing & (np.abs(first - rng_i) < 1e-6) & (pc[:, 2] > 0.1) & (u > 2) & (u < C.W - 2) & (v > 2) & (v < C.H - 2)
    inside = (np.abs(point - np.asarray(g.origin)) < extent).all(-1)
    return exact, keep.reshape(-1) & seen & inside & np.isfinite(exact)


# ---------------------------------------------------------------------------------------------------- alignment
ALIGN_CFG = dict(stride=2, depth_min=0.1, depth_max=10.0, distance_threshold=0.1)
ALIGN_MIN_WEIGHT = 0.1  # the mapper's: the integrated state's weights are mostly below the refiner's default 2.0


def perturbed_pose(i: int):
    """camera i moved by 0.03 m and turned by 2 degrees"""
    _, pos, quat, _ = C.camera(i)
    d = np.array([0.02, -0.02, 0.01])  # |d| = 0.03
    axis = np.array([0.3, -0.5, 0.81])
    axis /= np.linalg.norm(axis)
    h = np.deg2rad(2.0) / 2
    import pose_detector_ref as PR

    q = PR.quat_mul(np.concatenate([[np.cos(h)], np.sin(h) * axis]), quat.astype(np.float64))
    return (pos.astype(np.float64) + d).astype(np.float32), q.astype(np.float32)


@lru_cache(maxsize=None)
def align_depth(i: int = 0):
    """camera i's depth in the alignment kernel's own convention: pixel (pi, pj) holds the depth along the ray ((pj - cx) / fx,
    (pi - cy) / fy, 1), with NO half pixel (wp_raycast_pose_refine.py:171-172), so that the true pose is where the residuals vanish.
    mapper_ref.render_depth goes through pixel centres, so it is asked for the camera whose principal point lies half a pixel
    further: the same rays.  The alignment ROW tests use it; the refiner tests use the image of mapper_cases.camera, through the
    pixel centres, as a depth camera delivers it."""
    K, pos, quat, _ = C.camera(i)
    shifted = K.copy()
    shifted[0, 2] += 0.5
    shifted[1, 2] += 0.5
    return R.render_depth(shifted, pos, quat, C.H, C.W)


def align_pose(which: str):
    if which == "true":
        _, pos, quat, _ = C.camera(0)
        return pos, quat
    return perturbed_pose(0)


@lru_cache(maxsize=None)
def align_ref(which: str, n_samples: int, double: bool = True):
    sw, w, visible, _ = state("integrated")
    K, depth = C.camera(0)[0], align_depth(0)
    pos, quat = align_pose(which)
    return RR.ray_align(grid(), sw, w, visible, depth, K, pos, quat, ALIGN_CFG["stride"], n_samples, ALIGN_CFG["depth_min"], ALIGN_CFG["depth_max"],
                        ALIGN_CFG["distance_threshold"], ALIGN_MIN_WEIGHT, np.float64 if double else np.float32)


def refiner_cfg(**over):
    """the refiner's configuration of the tests: 1200 points (stride 2), five samples per ray (with one, the float64 restatement
    itself ends 81 mm from the truth on camera 0's image, further than the 30 mm it starts at, on this 2 cm grid), the mapper's minimum weight, 5 x 4 iterations"""
    base = dict(n_points=1200, minimum_valid_depth_pixels=100, max_iterations=20, inner_iterations=4, distance_threshold=0.1,
                n_samples_per_ray=5, depth_minimum_distance=0.1, depth_maximum_distance=10.0, minimum_tsdf_weight=ALIGN_MIN_WEIGHT,
                lambda_initial=1e-3, lambda_factor=10.0, lambda_min=1e-7, lambda_max=1e7, rho_min=0.25)
    base.update(over)
    return base


@lru_cache(maxsize=None)
def refiner_ref(i: int = 0):
    """the float64 restatement's refiner from perturbed_pose(i) on the depth image of mapper_cases.camera(i): (position, quaternion,
    final, initial error)"""
    sw, w, visible, _ = state("integrated")
    K, _, _, depth = C.camera(i)
    pos, quat = perturbed_pose(i)
    cfg = SimpleNamespace(**refiner_cfg())
    cfg.outer_iterations = cfg.max_iterations // cfg.inner_iterations
    return RR.refine(grid(), sw, w, visible, depth, K, pos, quat, cfg)


def pose_distance(pos, quat, pos_true, quat_true):
    """(translation, angle) between two poses"""
    a, b = np.asarray(quat, np.float64), np.asarray(quat_true, np.float64)
    c = abs(float(a @ b)) / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.linalg.norm(np.asarray(pos, np.float64) - np.asarray(pos_true, np.float64))), float(2 * np.arccos(min(1.0, c)))


# ---------------------------------------------------------------------------------------------------- the device against a reference
def compare_render(points, normals, depth, mask, ref, cam=None) -> str:
    """the device's four outputs (NumPy, [H W, ...]) against a float64 ``raycast``: "" or what differs.  The mask equal at every
    unflagged pixel, range and normals within 4 x the restatement's own float32 gap, every output exactly 0 on a miss."""
    mask = np.asarray(mask).reshape(-1) != 0
    points, normals, depth = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3), np.asarray(depth, np.float64).reshape(-1)
    flagged = ref["ambiguous"]
    if flagged.mean() > AMBIGUOUS_CAP:
        return f"{flagged.mean():.3f} of the pixels are flagged, more than {AMBIGUOUS_CAP}"
    clear = ~flagged
    if not np.array_equal(mask[clear], ref["mask"][clear]):
        return f"the hit mask differs at {int((mask != ref['mask'])[clear].sum())} unflagged pixels"
    if points[~mask].any() or normals[~mask].any() or depth[~mask].any():
        return "a miss is not zero in every output"
    both = clear & mask
    if both.any():
        gap_range, gap_normal = np.abs(depth - ref["depth"])[both].max(), np.abs(normals - ref["normals"])[both].max()
        if gap_range > 4 * GAP_RANGE or gap_normal > 4 * GAP_NORMAL:
            return f"range off by {gap_range:.2e} (bound {4 * GAP_RANGE:.1e}), normals by {gap_normal:.2e} (bound {4 * GAP_NORMAL:.1e})"
        if np.abs(points - ref["points"])[both].max() > 4 * GAP_RANGE + 1e-6:
            return f"hit points off by {np.abs(points - ref['points'])[both].max():.2e}"
    return ""


def compare_rows(rows, ref, trunc=None) -> str:
    """workspace rows [n, 32] (float32) of the device against a float64 ``ray_align``: the in-order sum within pose_rows.row_bound of
    the unflagged samples' sums plus the flagged samples' terms; the count equal up to the flagged samples"""
    import pose_rows

    got, count = pose_rows.reduce_rows(np.asarray(rows, np.float32))
    flagged = ref["ambiguous"]
    if flagged.mean() > AMBIGUOUS_CAP:
        return f"{flagged.mean():.3f} of the samples are flagged, more than {AMBIGUOUS_CAP}"
    sums, mags, n = RR.align_sums(ref, ~flagged)
    if not n <= count <= n + int(flagged.sum()):
        return f"count {count}, the reference has {n} unflagged and {int(flagged.sum())} flagged samples"
    # a flagged sample may count on one side only: its terms as the reference has them, or as large as a term can be where it
    # has none (|g| <= 1, |g x p| <= 2 in these scenes, |r| <= twice the truncation distance)
    _, flagged_mags, n_flagged_valid = RR.align_sums(ref, flagged)
    cap_j = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])
    cap_r = 2 * (grid().trunc if trunc is None else trunc)
    cap = np.concatenate([np.outer(cap_j, cap_j)[np.triu_indices(6)], cap_j * cap_r, [cap_r ** 2]]) * (int(flagged.sum()) - n_flagged_valid)
    bound = pose_rows.row_bound(max(count, 1), mags, ALIGN_ROUNDINGS) + flagged_mags + cap
    worst = np.abs(got.astype(np.float64) - sums) - bound
    if (worst > 0).any():
        k = int(np.argmax(worst))
        return f"row word {k}: {got[k]:.8e} against {sums[k]:.8e}, bound {bound[k]:.2e}"
    return ""
