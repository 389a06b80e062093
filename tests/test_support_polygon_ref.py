"""The support-polygon term on the host: the float64 restatement (tests/support_polygon_ref.py) against what the reference's own
code returned (tests/golden/support_polygon.npz, float64, 1e-12), the kernel's hull algorithm against the reference's on every
hull case of the GPU test, the launchers' argument checks, and the new C symbols.  No GPU is needed."""

import os

import numpy as np
import pytest
import torch

import support_polygon_ref as R
from curobo_amd import _lib
from curobo_amd.backends import cost as cost_hip

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "support_polygon.npz")
NAMES = ("curobo_hip_convex_hull_2d", "curobo_hip_support_polygon_cost", "curobo_hip_rollout_point_aggregate_terms")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_symbols_are_declared_and_the_abi_is_unchanged():
    lib = _lib.load()
    for n in NAMES:
        assert n in _lib.declared_symbols() and n in _lib._signatures() and hasattr(lib, n)
    assert lib.curobo_hip_abi_version() == 7
    for fn in ("convex_hull_2d", "support_polygon_cost", "rollout_point_aggregate_terms"):
        assert callable(getattr(cost_hip, fn))
    from curobo_amd.cost import ConvexPolygon2DHelper, CostSupportPolygon, CostSupportPolygonCfg  # noqa: F401
    from curobo_amd.hip_ops import SupportPolygonCostFunction  # noqa: F401


def test_restated_hull_equals_the_reference(golden):
    g = golden
    for algorithm in (R.hull, R.hull_monotone_chain):
        hulls, counts = R.hulls_padded(g["hull_vertices"], float(g["padding"]), algorithm)
        assert np.array_equal(counts, g["hull_counts"]) and 4 <= counts.min() and counts.max() <= 9
        assert hulls.shape == g["hull_out64"].shape and np.abs(hulls - g["hull_out64"]).max() < 1e-12
    for k in range(4):
        hulls, counts = R.hulls_padded(g[f"c{k}_vertices"], float(g["padding"]), R.hull_monotone_chain)
        assert np.array_equal(counts, g[f"c{k}_counts"]) and np.abs(hulls - g[f"c{k}_hulls64"]).max() < 1e-12


@pytest.mark.parametrize("name", sorted(R.hull_cases()))
def test_monotone_chain_gives_the_graham_scan_sequence(name):
    """what the kernel runs against what the reference runs, on the GPU test's hull cases (the degenerate ones included)"""
    points, padding = R.hull_cases()[name]
    a, ca = R.hulls_padded(points, padding, R.hull)
    b, cb = R.hulls_padded(points, padding, R.hull_monotone_chain)
    assert np.array_equal(ca, cb) and np.abs(a - b).max() < 1e-15
    expect = dict(three_points=3, one_interior=3, collinear_triple=4, repeated_point=3, two_lowest=4)
    if name in expect:
        assert ca.tolist() == [expect[name]]
    if name == "two_lowest":  # the leftmost of the two lowest points comes first
        assert np.allclose(R.hull(points[0])[0], [-0.25, -0.5])


@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("mode", ["padded", "counts"])
def test_restated_cost_equals_the_reference(golden, case, mode):
    g, k = golden, case
    counts = g[f"c{k}_counts"] if mode == "counts" else None
    for i, icw in ((1, 0.001), (0, 0.0)):
        r = R.support_polygon(g[f"c{k}_points"], g[f"c{k}_hulls"], g[f"c{k}_idxs"], counts, float(g["weight"]), icw)
        assert np.abs(r["sd"] - g[f"c{k}_{mode}_sd64"]).max() < 1e-12
        assert np.abs(r["cost"] - g[f"c{k}_{mode}_cost{i}_64"]).max() < 1e-12
        # (the reference's autograd runs through d / 0.01 twice: its own rounding is ~1e-13 on a gradient of size 1)
        assert np.abs(r["grad"] - g[f"c{k}_{mode}_grad{i}_64"]).max() < 1e-12
        assert np.isfinite(r["grad"]).all() and np.isfinite(r["cost"]).all()
    if k == 2:
        far = np.abs(g["c2_points"]).max(axis=-1) > 3.0
        assert far.sum() == 4 and (r["sd"][far] > 4.0).all()
        assert (r["boundary"] == 0).sum() == 2  # the two points on a vertex


def test_launchers_reject_bad_sizes_and_null_outputs_without_a_gpu():
    lib = _lib.load()
    t = torch.zeros(4 * 66 * 2)
    cnt, idx = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    p = lambda x: x.data_ptr()  # noqa: E731
    for n in (2, 65):
        assert lib.curobo_hip_convex_hull_2d(p(t), p(cnt), p(t), 0.05, 1, n, None) == 1
        assert f"n_pts must be in 3..64, got {n}".encode() in lib.curobo_hip_last_error()
        with pytest.raises(ValueError, match="n_pts must be in 3..64"):
            cost_hip.convex_hull_2d(torch.zeros(1, n, 2), torch.zeros(1, dtype=torch.int32), torch.zeros(1, n, 2), 0.05)
    assert lib.curobo_hip_convex_hull_2d(None, p(cnt), p(t), 0.05, 1, 8, None) == 1 and b"must not be null" in lib.curobo_hip_last_error()
    assert lib.curobo_hip_convex_hull_2d(p(t), None, p(t), 0.05, 1, 8, None) == 1 and b"must not be null" in lib.curobo_hip_last_error()
    assert lib.curobo_hip_convex_hull_2d(p(t), p(cnt), p(t), 0.05, -1, 8, None) == 1

    def cost(out=p(t), grad=p(t), com=p(t), hulls=p(t), idxs=p(idx), w=p(t), smoothing=0.01, B=4, H=1, N=2, M=8, mode=0):
        return lib.curobo_hip_support_polygon_cost(out, grad, None, com, hulls, None, idxs, w, 0.001, 0.1, smoothing, B, H, N, M, mode, None)

    assert cost(M=33) == 1 and b"max_vertices must be in 1..32, got 33" in lib.curobo_hip_last_error()
    assert cost(M=0) == 1
    assert cost(out=None) == 1 and b"cost and grad_com must not be null" in lib.curobo_hip_last_error()
    assert cost(grad=None) == 1 and b"cost and grad_com must not be null" in lib.curobo_hip_last_error()
    for kw in (dict(com=None), dict(hulls=None), dict(idxs=None), dict(w=None)):
        assert cost(**kw) == 1 and b"must not be null" in lib.curobo_hip_last_error()
    assert cost(smoothing=0.0) == 1 and b"smoothing must be positive" in lib.curobo_hip_last_error()
    assert cost(H=0) == 1 and cost(N=0) == 1 and cost(mode=2) == 1
    assert cost(com=p(t) + 4) == 1 and b"16-byte aligned" in lib.curobo_hip_last_error()
    with pytest.raises(ValueError, match="max_vertices must be in 1..32, got 33"):
        cost_hip.support_polygon_cost(torch.zeros(2, 1), torch.zeros(2, 1, 4), None, torch.zeros(2, 1, 4), torch.zeros(1, 33, 2),
                                      None, torch.zeros(2, dtype=torch.int32), torch.ones(1), 0.001)
    with pytest.raises(ValueError, match=r"out_grad_com must have shape \(2, 1, 4\)"):
        cost_hip.support_polygon_cost(torch.zeros(2, 1), torch.zeros(2, 1, 3), None, torch.zeros(2, 1, 4), torch.zeros(1, 8, 2),
                                      None, torch.zeros(2, dtype=torch.int32), torch.ones(1), 0.001)
    with pytest.raises(ValueError, match="idxs_hull must be a contiguous torch.int32"):
        cost_hip.support_polygon_cost(torch.zeros(2, 1), torch.zeros(2, 1, 4), None, torch.zeros(2, 1, 4), torch.zeros(1, 8, 2),
                                      None, torch.zeros(2, dtype=torch.int64), torch.ones(1), 0.001)
    assert lib.curobo_hip_rollout_point_aggregate_terms(None, None, None, None, None, None, None, None, 4, 1, 7, 10, None) == 1
    assert b"out_cost must not be null" in lib.curobo_hip_last_error()
