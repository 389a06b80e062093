"""oracle/graph_ref.py (the float64 oracle of the graph-planner launches) on the CPU: its k-NN against a plain double loop, its
steering rules against the torch functions of curobo_amd/graph_planner/prm.py, and -- before any device result exists -- the
conditions the GPU tests rely on, for every batch of tests/graph_cases.py: the step count is unambiguous, at most 5 % of a batch is
undecided in the oracle's band, and every kind of edge a batch is meant to hold is there among the decided ones."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import graph_cases as gc
from oracle.graph_ref import (EPS, EPS_Q, FEASIBLE, INFEASIBLE, UNDECIDED, feasible_band, index_from_first_bad, knn_ref, last_feasible_index_ref,
                              steer_band, steer_num_steps_ref, steer_points_fp32, steer_points_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tolerances_are_the_derived_ones():
    assert EPS == 2 * 1e-5  # twice the FK position tolerance of tests/test_gpu_kernels.py::test_fk_forward
    assert EPS_Q == 1e-6 and EPS_Q < 4 * float(np.spacing(np.float32(4.0)))  # a few fp32 ulps at a few radians


@pytest.mark.parametrize("name", [n for n in gc.knn_ids() if n.startswith("grid") and int(n.split("-")[1][1:]) <= 65] + ["identical"])
def test_knn_ref_against_a_double_loop(name):
    c = gc.knn_set(name)
    q, x, w = gc.knn_queries(c), c["buffer"], c["weight"]
    order, _ = knn_ref(q, x, w, c["n_nodes"], c["k"])
    for qi in range(q.shape[0]):
        keys = []
        for n in range(c["n_nodes"]):
            d = 0.0
            for j in range(c["D"]):
                v = (float(x[n, j]) - float(q[qi, j])) * float(w[j])
                d += v * v
            keys.append((d, n))
        assert [n for _, n in sorted(keys)[:c["k"]]] == order[qi].tolist()
    if name == "identical":
        np.testing.assert_array_equal(order, np.tile(np.arange(64), (q.shape[0], 1)))
    else:  # the queries lie past the searched prefix, nearer to themselves than any searched node
        assert c["query_rows"][0] == c["n_nodes"] and (knn_ref(q, x, w, x.shape[0], 1)[0][:, 0] >= c["n_nodes"]).all()


def test_knn_grid_sets_are_exact_and_hold_ties():
    for name in gc.knn_ids():
        c = gc.knn_set(name)
        if not c["exact"]:
            continue
        x = c["buffer"][:, :c["D"]].astype(np.float64)
        assert (x * 512 == np.rint(x * 512)).all() and np.abs(x).max() <= 2.0 and (c["weight"] * 16 == np.rint(c["weight"] * 16)).all()
        _, dist = knn_ref(gc.knn_queries(c), c["buffer"], c["weight"], c["n_nodes"], c["k"])
        assert (dist * 2.0 ** 26 == np.rint(dist * 2.0 ** 26)).all(), "a distance that is not exact in float64"
        if c["n_nodes"] >= 1000 or name == "identical":
            assert (np.diff(np.sort(dist, 1)[:, :c["k"] + 1], axis=1) == 0).any(), f"{name}: no tie among the first k keys"


def test_steering_rules_match_prm():
    from curobo_amd.graph_planner.prm import last_feasible_index, steer_num_steps, steer_points

    rng = np.random.default_rng(0)
    mask = rng.random((400, 40)) < 0.93
    mask[:5] = True  # all feasible; none; only the start infeasible; only the last point; the first of the second chunk of 16
    mask[1], mask[2, 0], mask[3, -1], mask[4, 16] = False, False, False, False
    np.testing.assert_array_equal(last_feasible_index_ref(mask), last_feasible_index(torch.as_tensor(mask)).numpy())
    assert last_feasible_index_ref(mask)[:5].tolist() == [39, 0, 0, 38, 15]
    assert index_from_first_bad([0, 1, 16, 40], 40).tolist() == [0, 0, 15, 39]
    for n_pts in (16, 17, 40):
        c = gc.placed_crossings(n_pts)
        s, t, w = (torch.as_tensor(c[k]) for k in ("start", "target", "weight"))
        steps, margin = steer_num_steps_ref(c["start"], c["target"], c["weight"], c["threshold"])
        np.testing.assert_array_equal(steps, steer_num_steps(s, t, w, c["threshold"]).numpy().astype(np.int64))
        ms = int(steps.max())
        assert ms == n_pts - 1 and int(np.argmax(steps)) == 0 and margin[0] >= 0.25
        pts = steer_points(s, t, ms).numpy()
        np.testing.assert_array_equal(steer_points_fp32(c["start"], c["target"], ms), pts)
        np.testing.assert_allclose(steer_points_ref(c["start"], c["target"], ms), pts, atol=1e-6, rtol=0)
        idx = np.arange(len(steps)) % (ms + 1)
        np.testing.assert_array_equal(steer_points_fp32(c["start"], c["target"], ms, idx), pts[np.arange(len(steps)), idx])
        # the limits alone, on the points torch computes: the placed step is the first outside, the expected index the rule's
        lo, hi = (np.asarray(v, np.float32) for v in gc.robot("franka").joint_limits_position)
        inside = torch.as_tensor(((pts >= lo) & (pts <= hi)).all(-1))
        np.testing.assert_array_equal(last_feasible_index(inside).numpy(), c["expect"])
        first = np.where((~inside.numpy()).any(1), (~inside.numpy()).argmax(1), ms + 1)
        np.testing.assert_array_equal(first, c["kstar"])


def test_placed_crossings_have_literal_answers():
    """first violating step k* -> index max(k* - 1, 0); the long feasible edge -> max_steps"""
    expect = {16: [15] + 4 * [0] + 4 * [0] + 4 * [14],
              17: [16] + 4 * [0] + 4 * [0] + 4 * [14] + 4 * [15],
              40: [39] + 4 * [0] + 4 * [0] + 4 * [14] + 4 * [15] + 4 * [16] + 4 * [30] + 4 * [31] + 4 * [38]}
    for n_pts, want in expect.items():
        c = gc.placed_crossings(n_pts)
        assert c["expect"].tolist() == want
        band = gc.steering_reference(c)["band"]
        assert band["decided"].all() and band["index"].tolist() == want


def test_band_is_ordered_and_honours_disabled_slots(oracle):
    m = gc.robot("franka")
    c = gc.oracle_case("franka", "slots40")
    q = c["start"][:200]
    state = feasible_band(q, m, gc.scene_arrays("slots40"), oracle=oracle)
    wide = feasible_band(q, m, gc.scene_arrays("slots40"), eps=50 * EPS, oracle=oracle)
    assert ((wide == UNDECIDED) | (wide == state)).all(), "a wider band may only move points to undecided"
    on = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in gc.scene_arrays("slots40").items()}
    on["cuboid_enable"][:] = 1
    assert (feasible_band(q, m, on, oracle=oracle) == INFEASIBLE).all() and (state == FEASIBLE).any(), "the disabled box around the base"
    a = gc.scene_arrays("slots40")
    assert a["cuboid_dims"].shape[1] == 40 and np.flatnonzero(a["cuboid_enable"][0]).tolist() == [0, 7, 31, 32, 39]
    assert "cuboid_dims" not in gc.scene_arrays("voxels") and "voxel_params" in gc.scene_arrays("c3") and "cuboid_dims" in gc.scene_arrays("c3")


def test_cases_lie_on_both_sides_of_the_60_kib_launch_path():
    """``curobo_hip_graph_steer`` raises the kernel's LDS limit above 60 KiB.  Of the packaged robots only dual_ur10e comes near (57 KiB
    without a scene, 60 480 bytes with the 40-slot scene; unitree_g1 needs 900 KiB and never takes the fused launch), so the 40-slot
    world is also given in 64 slots (``slots64``): 62 400 bytes."""
    lds = {p: gc.fused_lds_bytes(*p) for p in gc.oracle_pairs()}
    print({f"{r}/{s}": b for (r, s), b in lds.items()})
    assert min(lds.values()) < 60 * 1024 < max(lds.values())
    assert not gc.fits_fused("unitree_g1", "none") and ("unitree_g1", "none") not in gc.oracle_pairs()


_INTENDS = {"placed": ("feasible", "start", "later"), "zero_length": ("feasible", "start"), "default": ("feasible", "start", "later")}


@pytest.mark.parametrize("name", list(gc.steering_batches()))
def test_steering_batch_is_inside_its_caps(name):
    c = gc.steering_batches()[name]
    ref = gc.steering_reference(c)
    band, ms = ref["band"], ref["max_steps"]
    assert ms == c["max_steps"] and c["start"].shape[0] * (ms + 1) <= 100_000
    top = int(np.argmax(ref["steps"]))
    # (a batch of zero-length edges only: the ratio is exactly 0 in fp32 and in float64, nothing to round)
    assert ref["margin"][top] >= 0.25 or (c["start"] == c["target"]).all(), f"ratio {ref['margin'][top]:.3f} from an integer"
    assert (ref["steps"] <= ms).all()
    dec, st = band["decided"], band["state"]
    share = 1.0 - float(dec.mean())
    kinds = {"feasible": dec & (st == FEASIBLE).all(1), "start": dec & (st[:, 0] == INFEASIBLE)}
    kinds["later"] = dec & ~kinds["feasible"] & ~kinds["start"]
    print(f"{name}: {len(dec)} edges x {ms + 1} points, undecided {100 * share:.2f} %, decided feasible {int(kinds['feasible'].sum())}, "
          f"infeasible at the start {int(kinds['start'].sum())}, infeasible later {int(kinds['later'].sum())}")
    assert share <= gc.UNDECIDED_CAP
    for k in _INTENDS.get(name.split("/")[0], _INTENDS["default"]):
        assert kinds[k].any(), f"no decided edge of kind '{k}'"
    assert (band["index_lo"] <= band["index_hi"]).all() and (band["index"][dec] == band["index_lo"][dec]).all()
    if name == "zero_length":
        assert set(band["index"].tolist()) == {0, 1} and not kinds["later"].any()
    if name == "beyond_the_grid":
        assert len(dec) == gc.GRID_CAP + 37 and ms <= 8
        for part in (slice(0, gc.GRID_CAP), slice(gc.GRID_CAP, None)):
            assert kinds["feasible"][part].any() and kinds["start"][part].any() and kinds["later"][part].any()


@pytest.mark.parametrize("n", gc.POINT_SIZES)
def test_point_batch_is_inside_its_caps(n):
    state = gc.points_reference(n)
    share = float((state == UNDECIDED).mean())
    print(f"points {n}: undecided {100 * share:.3f} %, feasible {int((state == FEASIBLE).sum())}, infeasible {int((state == INFEASIBLE).sum())}")
    assert state.shape == (n,) and share <= gc.UNDECIDED_CAP
    if n > 1:
        assert (state == FEASIBLE).any() and (state == INFEASIBLE).any() and state[-1] == FEASIBLE
    if n > 16 * gc.GRID_CAP:
        tail = state[16 * gc.GRID_CAP:]
        assert (tail == FEASIBLE).any() and (tail == INFEASIBLE).any(), "both answers among the points of the second pass"


def test_fuzz_generator_stays_inside_its_caps():
    """tests/randomised/fuzz_graph.py at the suite's seed and count (tests/test_gpu_randomised_sweeps.py): on the device a case whose
    decided share is below 95 % fails, so the generator must not draw one"""
    spec = importlib.util.spec_from_file_location("_fuzz_graph", os.path.join(ROOT, "tests", "randomised", "fuzz_graph.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    for case, sc, kc in fz.generate(12, 5):
        ref = fz.steer_reference(sc)
        share = 1.0 - float(ref["band"]["decided"].mean())
        print(f"case {case}: {fz.describe_steer(sc)} undecided {100 * share:.2f} %")
        top = int(np.argmax(ref["steps"]))
        assert share <= gc.UNDECIDED_CAP and ref["max_steps"] == sc["max_steps"] <= 40 and ref["margin"][top] >= 0.25
        assert sc["start"].shape[0] * (ref["max_steps"] + 1) <= 100_000
        assert 1 <= kc["k"] <= min(64, kc["n_nodes"])
