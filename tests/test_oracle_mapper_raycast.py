"""The restatement of the ray launches (tests/mapper_raycast_ref.py) held against the analytic scene, and against itself in
float32: what the device tests' bounds are made of (tests/mapper_raycast_cases.py, docs/NOTEBOOK.md).  No GPU.

Measured here (printed with -s): the restatement's range error against the exact sphere and ground at camera 2, which integrated
nothing, is at most 11.7 mm (median 2.3 mm) over 783 pixels in both forms; its float32-against-float64 gap is at most 5.9e-6 m of
range and 6.1e-5 of a normal's component over the twelve parity renders and 2.8e-5 of a row sum relative to its terms; its float64
refiner, on the depth image of mapper_cases, brings camera 0 from 30 mm / 2 degrees to 12.0 mm / 0.55 degrees and camera 1 to 6.1 mm /
0.51 degrees.

One condition of the issue is not met as written and is stated here in the form that can be: "at the true pose of camera 0 ...
at least half of the samples are valid".  The grid is 1.0 x 0.96 x 0.4 m and camera 0 stands 1.2 m from it with a 67 x 53 degree
view: 28 % of its sampled pixels observe a point inside the grid at all, and 32 % of the samples are valid (385 of 1200).  The test
asserts that the valid samples are at least half of those whose observed point lies inside the grid, and prints both figures."""

import numpy as np
import pytest

import mapper_cases as C
import mapper_raycast_cases as RC
import mapper_raycast_ref as RR
import pose_rows

RENDERS = [(s, v, a) for s in ("integrated", "injected") for v in RC.VIEWS for a in (0, 1)]


def _within(measured, ceiling, what):
    print(f"{what}: measured {measured:.3e}, ceiling {ceiling:.3e}")
    assert 0.99 * ceiling <= measured <= ceiling, f"{what}: {measured:.4e} is not within 1 % below {ceiling:.4e}: the constant is the measured value"


def test_warp_definitions_the_restatement_relies_on():
    """wp.sign(0) is +1, so a ray component of exactly 0 gives the slab +1e10, not 0; wp.quat_rotate is the expanded form"""
    import sys

    sys.path.insert(0, str(__import__("pathlib").Path(__file__).parent / "golden" / "warp_emulator"))
    try:
        import warp as wp
    finally:
        sys.path.pop(0)
    assert float(wp.sign(wp.float32(0.0))) == 1.0 and float(wp.sign(wp.float32(-0.0))) == 1.0 and float(wp.sign(wp.float32(-1e-9))) == -1.0
    g = RC.grid()
    M = RR.DenseMap(g, *RC.integrated_state(), g.min_weight, np.float64)
    cam = np.array([0.013, -0.021, 0.9])
    t = RR._block_exit(M, cam, np.array([[0.0, 0.0, -1.0], [-0.0, 0.0, -1.0]]), np.array([[6.0, 5.0, 4.0], [6.0, 5.0, 4.0]]))
    assert np.allclose(t, 0.9 - (-0.2 + 4 * 4 * 0.02)) and t[0] == t[1]  # the block's lower z face: z = -0.2 + 16 voxels
    q = np.array([0.5, 0.5, -0.5, 0.5])
    v = np.array([0.3, -1.0, 2.0])
    w = wp.quat_rotate(wp.quat(q[1], q[2], q[3], q[0]), wp.vec3(*v))
    assert np.allclose(RR.R.quat_rotate(q, v), [float(w[0]), float(w[1]), float(w[2])], atol=1e-6)


@pytest.mark.parametrize("state,view,accelerated", RENDERS)
def test_render_restatement_against_itself_in_float32(state, view, accelerated):
    a, b = RC.render_ref(state, view, accelerated), RC.render_ref(state, view, accelerated, False)
    assert a["ambiguous"].mean() <= RC.AMBIGUOUS_CAP and b["ambiguous"].mean() <= RC.AMBIGUOUS_CAP
    clear = ~(a["ambiguous"] | b["ambiguous"])
    assert np.array_equal(a["mask"][clear], b["mask"][clear])
    assert a["mask"].sum() >= 25, "the view must see the map"
    both = clear & a["mask"]
    gap_range, gap_normal = np.abs(a["depth"] - b["depth"])[both].max(), np.abs(a["normals"] - b["normals"])[both].max()
    print(f"{state} {view} accelerated {accelerated}: {a['mask'].sum()} hits, {a['ambiguous'].sum()} flagged, gap {gap_range:.2e} m, {gap_normal:.2e}")
    assert gap_range <= RC.GAP_RANGE and gap_normal <= RC.GAP_NORMAL
    for key in ("points", "normals", "depth"):
        assert not a[key][~a["mask"]].any(), "a miss is zero in every output"


def test_the_gap_ceilings_are_what_was_measured():
    gr = gn = 0.0
    for s, v, acc in RENDERS:
        a, b = RC.render_ref(s, v, acc), RC.render_ref(s, v, acc, False)
        both = ~(a["ambiguous"] | b["ambiguous"]) & a["mask"] & b["mask"]
        gr, gn = max(gr, np.abs(a["depth"] - b["depth"])[both].max()), max(gn, np.abs(a["normals"] - b["normals"])[both].max())
    _within(gr, RC.GAP_RANGE, "float32-against-float64 gap of the range")
    _within(gn, RC.GAP_NORMAL, "float32-against-float64 gap of a normal's component")


def test_the_two_forms_are_two_contracts():
    a, b = RC.render_ref("integrated", "outside", 0), RC.render_ref("integrated", "outside", 1)
    both = a["mask"] & b["mask"]
    assert both.sum() > 300 and (a["depth"][both] != b["depth"][both]).any()
    diff = np.abs(a["depth"] - b["depth"])[both]
    # the same surface for most pixels; not where the plain march carries a positive sample across unseen space and the accelerated
    # one forgets it at the first block it skips
    assert np.median(diff) < 1e-6 and diff.max() > 0.05 and a["mask"].sum() != b["mask"].sum()


def test_render_against_the_analytic_scene():
    exact, keep = RC.camera2_truth()
    worst = 0.0
    for acc in (0, 1):
        r = RC.camera2_ref(acc)
        assert r["ambiguous"].mean() <= RC.AMBIGUOUS_CAP
        k = keep & ~r["ambiguous"]
        err = np.abs(r["depth"] - exact)[k]
        print(f"accelerated {acc}: {k.sum()} pixels, range error max {err.max():.5f} m, median {np.median(err):.5f} m")
        assert k.sum() > 600
        worst = max(worst, err.max())
    _within(worst, RC.ANALYTIC_RANGE_ERROR, "range error of the restatement against the exact scene")


@pytest.mark.parametrize("pose", ["true", "off"])
@pytest.mark.parametrize("n_samples", [1, 5])
def test_alignment_restatement_against_itself_in_float32(pose, n_samples):
    a, b = RC.align_ref(pose, n_samples), RC.align_ref(pose, n_samples, False)
    assert a["ambiguous"].mean() <= RC.AMBIGUOUS_CAP and b["ambiguous"].mean() <= RC.AMBIGUOUS_CAP
    clear = ~(a["ambiguous"] | b["ambiguous"])
    assert np.array_equal(a["valid"][clear], b["valid"][clear])
    sa, mags, n = RR.align_sums(a, clear)
    sb, _, nb = RR.align_sums(b, clear)
    assert n == nb and n > 300
    bound = pose_rows.row_bound(n, mags, RC.ALIGN_ROUNDINGS)
    print(f"{pose} pose, {n_samples} per ray: {n} of {len(a['valid'])} valid, worst sum at {np.max(np.abs(sa - sb) / bound):.2f} of its bound")
    assert (np.abs(sa - sb) <= bound).all()


def test_enough_of_the_alignment_samples_are_valid():
    """(see the module's docstring: the issue's "half of the samples" cannot hold for camera 0 over this grid)"""
    a = RC.align_ref("true", 1)
    K, pos, quat, _ = C.camera(0)
    ray, _, ray_len, pi, pj = RR.camera_rays(K, quat, C.H, C.W, False, np.float64, RC.ALIGN_CFG["stride"])
    d = RC.align_depth(0)[pi, pj].astype(np.float64)
    g = RC.grid()
    point = pos.astype(np.float64) + ray * (d * ray_len)[:, None]
    in_grid = (d > 0) & (np.abs(point - np.asarray(g.origin)) < 0.5 * np.array([g.nx, g.ny, g.nz]) * g.vs).all(-1)
    print(f"{a['valid'].sum()} of {len(d)} samples valid ({a['valid'].mean():.3f}); {in_grid.sum()} observe a point inside the grid ({in_grid.mean():.3f})")
    assert len(d) == 1200 and a["valid"].sum() >= 0.5 * in_grid.sum() and a["valid"].sum() >= 380


def test_a_pose_that_is_not_finite_has_no_valid_sample():
    sw, w, visible, _ = RC.state("integrated")
    K, pos, quat, _ = C.camera(0)
    bad = quat.copy()
    bad[2] = np.nan
    ev = RR.ray_align(RC.grid(), sw, w, visible, RC.align_depth(0), K, pos, bad, 2, 1, 0.1, 10.0, 0.1, 0.1)
    assert not ev["valid"].any() and not ev["J"].any()


@pytest.mark.parametrize("camera", [0, 1])
def test_float64_refiner_approaches_the_truth(camera):
    """on the depth images of mapper_cases, as the device test runs it"""
    p, q, final, initial = RC.refiner_ref(camera)
    _, pos, quat, _ = C.camera(camera)
    start, end = RC.pose_distance(*RC.perturbed_pose(camera), pos, quat), RC.pose_distance(p, q, pos, quat)
    print(f"float64 refiner, camera {camera}: {start[0]:.4f} m, {start[1]:.4f} rad -> {end[0]:.4f} m, {end[1]:.4f} rad; error {initial:.4f} -> {final:.4f}")
    assert start[0] == pytest.approx(0.03, abs=1e-6) and start[1] == pytest.approx(np.deg2rad(2.0), abs=1e-6)
    assert final <= initial and end[0] < 0.5 * start[0] and end[1] < 0.5 * start[1]
