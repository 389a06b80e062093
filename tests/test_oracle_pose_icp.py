"""The reference's own fp32 ICP (tests/golden/pose_icp_golden.npz, recorded by tests/golden/make_pose_icp_golden.py) against the
float64 oracle tests/pose_icp_ref.py: its correspondences outside the excluded set (up to what its expanded cdist can tell apart), its 28 sums within the order-free bound,
its steps within the K bound -- which is how K is established -- and the oracle against the reference's float64 run.  No GPU."""

import os

import numpy as np
import pytest

import pose_icp_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_icp_golden.npz")


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    cfg = dict(zip(g["cfg_names"].tolist(), g["cfg_values"].tolist()))
    return g, cfg


def iterations(g, run, stage):
    ran = g[f"{run}/{stage}/ran"]
    return [(int(i), int(it)) for i, it in zip(*np.nonzero(ran))]


def oracle_of(g, cfg, run, stage, i, it, index=None):
    return R.correspond(g[f"{stage}_mesh_points"], g[f"{stage}_mesh_normals"], g[f"{stage}_observed"], g[f"{run}/{stage}/T_before"][i, it],
                        cfg[f"distance_threshold_{stage}"], True, cfg["huber_delta"], index=index)


@pytest.mark.parametrize("stage", ["coarse", "fine"])
def test_reference_correspondences_and_sums(golden, stage):
    g, cfg = golden
    worst_share, worst_row, n_checked, n_differs = 0.0, 0.0, 0, 0
    for i, it in iterations(g, "fp32", stage):
        c = oracle_of(g, cfg, "fp32", stage, i, it)
        ref_index = g[f"fp32/{stage}/index"][i, it]
        keep = ~c["excluded"]
        worst_share = max(worst_share, float(c["excluded"].mean()))
        assert c["excluded"].mean() <= 0.02
        # torch.cdist in fp32 expands |a - b|^2 into |a|^2 + |b|^2 - 2 a.b, each within a few 2^-24 of |a|^2 + |b|^2, so the
        # reference itself may pick a point whose squared distance is that much larger than the least; nothing more than that
        differs = np.nonzero(keep & (ref_index != c["index"]))[0]
        n_differs += len(differs)
        for k in differs:
            assert ref_index[k] >= 0 and c["index"][k] >= 0, (stage, i, it, k)
            T = R.as_T(g[f"fp32/{stage}/T_before"][i, it])
            sk = T[:, :3] @ g[f"{stage}_mesh_points"][k].astype(np.float64) + T[:, 3]
            ok = g[f"{stage}_observed"][ref_index[k]].astype(np.float64)
            d2_gap = ((sk - ok) ** 2).sum() - c["dist"][k] ** 2
            assert d2_gap <= 8 * R.EPS * ((sk ** 2).sum() + (ok ** 2).sum()), (stage, i, it, k, d2_gap)
        if not g[f"fp32/{stage}/solved"][i, it]:
            continue
        # the sums over the reference's own correspondences
        s = oracle_of(g, cfg, "fp32", stage, i, it, index=ref_index)
        assert s["count"] == g[f"fp32/{stage}/count"][i, it]
        n = len(ref_index)
        err = np.abs(g[f"fp32/{stage}/rows"][i, it].astype(np.float64) - s["row"])
        bound = R.row_bound(n, s["row_abs"], R.ROW_ROUNDINGS_REFERENCE)
        worst_row = max(worst_row, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (stage, i, it, err / bound)
        n_checked += 1
    print(f"{stage}: {n_checked} iterations, largest excluded share {worst_share:.4f}, largest row error / bound {worst_row:.3f}, "
          f"{n_differs} correspondences where the reference's cdist picked a near tie")
    assert n_checked > 0


def test_reference_steps_establish_k(golden):
    g, cfg = golden
    need = 0.0
    for stage, mode in (("coarse", R.COARSE), ("fine", R.FINE)):
        for i, it in iterations(g, "fp32", stage):
            if not g[f"fp32/{stage}/solved"][i, it]:
                continue
            A, rhs = R.unpack_row(g[f"fp32/{stage}/rows"][i, it])  # teacher-forced: the reference's own fp32 sums
            st = R.step(A, rhs, int(g[f"fp32/{stage}/count"][i, it]), g[f"fp32/{stage}/T_before"][i, it], mode)
            err = np.abs(g[f"fp32/{stage}/x"][i, it].astype(np.float64) - st["x"]).max()
            need = max(need, err / (st["cond"] * R.EPS * np.abs(st["x"]).max()))
            assert err <= R.step_bound(st["cond"], st["x"]), (stage, i, it)
            # T after, entry by entry: the update's rounding next to entries of size <= 1 + |t|
            T_err = np.abs(g[f"fp32/{stage}/T_after"][i, it].astype(np.float64) - st["T"].reshape(-1)).max()
            assert T_err <= 2.0 * R.step_bound(st["cond"], st["x"]) + 32 * R.EPS, (stage, i, it, T_err)
    print(f"K needed by the reference's fp32 steps: {need:.4f}; POSE_ICP_K = {R.POSE_ICP_K}")
    assert 2.0 * need <= R.POSE_ICP_K < 8.0 * max(need, 0.125)  # a power of two above the need, doubled; not a loose one


def test_oracle_follows_the_float64_run(golden):
    """the oracle's correspond + step on the float64 run's transforms reproduce its sums, steps and counts"""
    g, cfg = golden
    for stage, mode in (("coarse", R.COARSE), ("fine", R.FINE)):
        for i, it in iterations(g, "fp64", stage):
            c = oracle_of(g, cfg, "fp64", stage, i, it)
            assert np.array_equal(g[f"fp64/{stage}/index"][i, it], c["index"]) and c["count"] == g[f"fp64/{stage}/count"][i, it]
            if not g[f"fp64/{stage}/solved"][i, it]:
                continue
            rows = g[f"fp64/{stage}/rows"][i, it]
            assert np.allclose(rows, c["row"], rtol=1e-9, atol=1e-12 * np.abs(c["row_abs"]).max())
            st = R.step(c["JtJ"], c["Jtb"], c["count"], g[f"fp64/{stage}/T_before"][i, it], mode)
            assert np.allclose(st["x"], g[f"fp64/{stage}/x"][i, it], rtol=1e-6, atol=1e-9 * st["cond"] * 1e-6 + 1e-12)
            assert np.allclose(st["T"].reshape(-1), g[f"fp64/{stage}/T_after"][i, it], atol=1e-9)


def test_the_recorded_runs_meet_what_the_maker_asserted(golden):
    g, cfg = golden
    for run in ("fp32", "fp64"):
        t_err, r_err = g[f"{run}/final_error"]
        assert t_err < 1e-3 and r_err < np.radians(0.5)
        e = np.sort(g[f"{run}/coarse/error"])
        assert e[0] < 0.75 * e[1]
        assert int(np.argmin(g[f"{run}/coarse/error"])) == int(g[f"{run}/best_hypothesis"])
    assert float(g["excluded_share"]) <= 0.02
    assert (cfg["n_mesh_points_coarse"], cfg["n_observed_points_coarse"], cfg["n_rotation_samples"], cfg["n_iterations_coarse"],
            cfg["distance_threshold_coarse"]) == (200, 500, 8, 10, 0.1)
    assert (cfg["n_mesh_points_fine"], cfg["n_observed_points_fine"], cfg["n_iterations_fine"], cfg["distance_threshold_fine"],
            cfg["huber_delta"]) == (500, 1000, 20, 0.02, 0.02)
