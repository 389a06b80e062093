"""Pin tests/lbfgs_iteration_ref.py (the float64 restatement the GPU tests of the L-BFGS iteration compare against) on the CPU:
against the C oracle on the inputs of the GPU tests, against the reference's torch twins recorded in optim_golden.npz, and its
step scale against the reference's own scale_action + jit_get_x_set recorded in step_scale_golden.npz
(tests/golden/make_step_scale_golden.py, step_scale = 0.98).

A row whose comparisons the reference calls undecidable hides a failure, so the share of such rows is a condition: at most 5 % of
any case and 0.5 % of all rows, asserted here on the reference alone, on the recipe of the GPU tests at 64 rows per case
(V, N, strategy, family: 1008 cases up to V = 1023 and N = 64) and on the GPU tests' own small batches per V.
Measured here: worst case 1 of 64 rows, 6 of 64512 rows (0.009 %)."""

import os

import numpy as np
import pytest

import lbfgs_iteration_cases as C
import lbfgs_iteration_ref as R
from conftest import GOLDEN_DIR

F32 = np.float32


def _oracle_line_search(oracle, case, strong, approx, thr):
    B, N, V = case["search_gradient"].shape
    st = {k: v.copy() for k, v in case["state"].items()}
    st.update(converged=np.zeros(B, np.uint8), exploration_cost=np.zeros(B, F32), exploration_action=np.zeros((B, V), F32),
              exploration_gradient=np.zeros((B, V), F32), cost=np.zeros(B, F32), action=np.zeros((B, V), F32),
              gradient=np.zeros((B, V), F32), exploration_idx=np.zeros((B, N), np.int32), selected_idx=np.zeros((B, N), np.int32))
    oracle.line_search(st, case["search_cost"].reshape(B, N, 1), case["search_action"], case["search_gradient"],
                       case["step_direction"].reshape(B, 1, V), case["alphas"], C.LS["c_1"], C.LS["c_2"], strong, approx,
                       C.LS["convergence_iteration"], thr[0], thr[1])
    st["selected_cost"], st["selected_action"], st["selected_gradient"] = st["cost"], st["action"], st["gradient"]
    return st


def _reference_line_search(case, strong, approx, thr, dtype=np.float64):
    return R.line_search(case["state"], case["search_cost"], case["search_action"], case["search_gradient"], case["step_direction"],
                         case["alphas"], C.LS["c_1"], C.LS["c_2"], strong, approx, C.LS["convergence_iteration"], thr[0], thr[1], dtype)


@pytest.mark.parametrize("V", C.LS_V)
def test_line_search_agrees_with_the_oracle_on_the_gpu_tests_inputs(V, oracle):
    """integer outputs equal and copied tensors bit-equal on every unambiguous row; at most 5 % of the rows of this V flagged"""
    rows = flagged = 0
    for N, wolfe, thr, family, B, i in C.line_search_sweep(V):
        case = C.line_search_case(B, V, N, family, i)
        strong, approx = C.wolfe_flags(wolfe, N)
        ref, orc = _reference_line_search(case, strong, approx, thr), _oracle_line_search(oracle, case, strong, approx, thr)
        ok = ~ref["ambiguous"]
        rows, flagged = rows + B, flagged + int(ref["ambiguous"].sum())
        for k in R.LS_INTEGER + R.LS_COPIED:
            assert np.array_equal(orc[k][ok], ref[k][ok], equal_nan=True), f"{k}: V={V} N={N} {wolfe} {thr} {family} B={B}"
    assert flagged <= 0.05 * rows, f"{flagged} of {rows} rows are ambiguous"


def test_ambiguity_caps_of_the_line_search_recipe():
    """64 rows per (V, N, strategy, family): at most 5 % of any case and 0.5 % of all rows may be ambiguous"""
    rows = flagged = 0
    worst = (0, None)
    for V in (1, 7, 63, 64, 65, 128, 129, 1023):
        for N in C.LS_N:
            for w, wolfe in enumerate(C.WOLFE):
                for f, family in enumerate(C.LS_FAMILIES):
                    case = C.line_search_case(64, V, N, family, w)
                    n = int(_reference_line_search(case, *C.wolfe_flags(wolfe, N), C.THRESHOLDS[(w + f) % 2])["ambiguous"].sum())
                    rows, flagged = rows + 64, flagged + n
                    worst = max(worst, (n, (V, N, wolfe, family)), key=lambda t: t[0])
    print(f"ambiguous rows: {flagged} of {rows} ({100.0 * flagged / rows:.3f} %), worst case {worst[0]} of 64 at {worst[1]}")
    assert worst[0] <= 0.05 * 64, worst
    assert flagged <= 0.005 * rows


def test_ambiguity_is_raised_at_a_threshold_and_not_by_nan():
    """a candidate whose cost sits exactly on the Armijo line flips with the rounding of g.d: ambiguous; the same row with a NaN
    dot product compares false everywhere: decidable"""
    rng = np.random.default_rng(0)
    V, N = 65, 4
    case = C.line_search_case(3, V, N, "random", 0)
    g, d = case["search_gradient"], case["step_direction"]
    gd0 = (g[:, 0].astype(np.float64) * d).sum(-1)
    ca = F32(C.LS["c_1"]) * case["alphas"]
    case["search_cost"][:, 0] = 0  # (next to a cost of O(1) the rounding of g.d is far below the cost's own ulp)
    case["search_cost"][:, 2] = (np.float64(ca[2]) * gd0).astype(F32)
    amb = _reference_line_search(case, False, False, (0.0, 0.0))["ambiguous"]
    assert amb.all()
    g[:, 0, int(rng.integers(V))] = np.nan
    assert not _reference_line_search(case, False, False, (0.0, 0.0))["ambiguous"].any()
    # update_best: rel within 4 ulp of a non-zero threshold.  rel moves in steps of ulp(cost) / (thr best): search a pair that lands there
    thr = F32(1e-3)
    bc = np.linspace(1.0, 2.0, 4001)[1:-1].astype(F32)
    sc = (bc - np.round(np.float64(thr) * (bc + 1e-6) / 2.0 ** -23) * 2.0 ** -23).astype(F32)
    rel = ((bc - sc).astype(F32).astype(np.float64) / (bc + F32(1e-6)).astype(F32)).astype(F32)
    hit = np.flatnonzero(np.abs(rel.astype(np.float64) - float(thr)) <= 4 * np.spacing(thr))[:3]
    assert len(hit) == 3
    case = C.line_search_case(3, V, N, "random", 1)
    case["search_cost"][:] = sc[hit, None]
    case["state"]["best_cost"] = bc[hit]
    assert _reference_line_search(case, True, False, (0.0, 1e-3))["ambiguous"].all()
    assert not _reference_line_search(case, True, False, (0.0, 0.0))["ambiguous"].any()
    assert not _reference_line_search(case, True, False, (1.0, 1e-3))["ambiguous"].any()  # (delta fails: rel does not matter)


def _run_step_chain(oracle, B, V, m, stable):
    """three consecutive steps on the oracle's own state; per step the reference in float64 and float32 from that state"""
    case = C.lbfgs_case(B, V, m, seed=V + m)
    st = {k: case[k].copy() for k in ("rho", "y", "s", "x_0", "grad_0")}
    q, g = case["q"], case["grad_q"]
    step = np.zeros((B, V), F32)
    out = []
    for it in range(3):
        r64 = R.lbfgs_step(st["rho"], st["y"], st["s"], q, g, st["x_0"], st["grad_0"], C.EPSILON, stable)
        r32 = R.lbfgs_step(st["rho"], st["y"], st["s"], q, g, st["x_0"], st["grad_0"], C.EPSILON, stable, np.float32)
        oracle.lbfgs_step(step, st["rho"], st["y"], st["s"], q, g, st["x_0"], st["grad_0"], C.EPSILON, stable)
        out.append((r64, r32, dict({k: v.copy() for k, v in st.items()}, step=step.copy())))
        q, g = C.lbfgs_next(case, q, step, st["x_0"], st["grad_0"], it)
    return out


@pytest.mark.parametrize("stable", [True, False])
def test_lbfgs_step_agrees_with_the_oracle(stable, oracle):
    rows = flagged = 0
    worst = 0.0
    for V in (1,) + C.STEP_V:
        for i, m in enumerate((5,) if V == 1 else C.STEP_M):
            B = C.BATCHES[(V + i) % len(C.BATCHES)]
            for it, (r64, r32, got) in enumerate(_run_step_chain(oracle, B, V, m, stable)):
                w, f, _ = R.check_step(r64, r32, got, f"V={V} m={m} B={B} stable={stable} step {it}")
                worst, rows, flagged = max(worst, w), rows + B, flagged + f
                if stable and m > 0 and B > 1 and it == 0:
                    assert r64["rho"][-1, 1] == 0 and got["rho"][-1, 1] == 0, "negative curvature must give rho = 0"
                if m > 0 and B >= 3 and it == 2:  # the planted exact zero is decidable and compared
                    assert not r64["flagged"][-1] and (r64["rho"][-1, -1] == 0 if stable else np.isinf(r64["rho"][-1, -1]))
    print(f"stable={stable}: worst error / bound {worst:.3f}, flagged {flagged} of {rows} rows")
    assert flagged <= 0.005 * rows


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN_DIR, "optim_golden.npz"))


@pytest.mark.parametrize("name", ["ik", "trajopt"])
def test_lbfgs_step_matches_the_reference_torch_twin(name, gold):
    q, g, step_ref = gold[f"lbfgs_{name}_q"], gold[f"lbfgs_{name}_g"], gold[f"lbfgs_{name}_step"]
    iters, b, v = q.shape
    m = gold[f"lbfgs_{name}_y"].shape[0]
    st = dict(y=np.zeros((m, b, v), F32), s=np.zeros((m, b, v), F32), rho=np.zeros((m, b), F32),
              x_0=gold[f"lbfgs_{name}_init_x0"].astype(F32), grad_0=gold[f"lbfgs_{name}_init_g0"].astype(F32))
    for it in range(iters):
        r = R.lbfgs_step(st["rho"], st["y"], st["s"], q[it], g[it], st["x_0"], st["grad_0"], 0.01, True)
        scale = np.abs(step_ref[it]).max()
        np.testing.assert_allclose(r["step"], step_ref[it], atol=2e-4 * scale, rtol=2e-3, err_msg=f"iteration {it}")
        st = {k: r[k].astype(F32) for k in st}
    np.testing.assert_allclose(st["y"], gold[f"lbfgs_{name}_y"], atol=1e-6)
    np.testing.assert_allclose(st["s"], gold[f"lbfgs_{name}_s"], atol=1e-6)
    np.testing.assert_allclose(st["rho"], gold[f"lbfgs_{name}_rho"], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("kind", ["wolfe", "strong_wolfe", "approx_wolfe"])
def test_line_search_matches_the_reference_torch_twin(kind, gold):
    """as test_oracle_optim.py holds the C oracle: exploration state identical; the selected index equal wherever the twin found
    a full-Wolfe step (it keeps 0 where the kernel falls back to the Armijo index), everywhere for strong Wolfe"""
    p = f"ls_{kind}_"
    x_set, d, c, g_x, al = (gold[p + k] for k in ("x_set", "d", "c", "g_x", "alphas"))
    b, nls, v = x_set.shape
    state = dict(best_cost=np.full(b, 1e9, F32), best_action=np.zeros((b, v), F32), best_iteration=np.zeros(b, np.int16),
                 current_iteration=np.zeros(b, np.int16))
    r = R.line_search(state, c.reshape(b, nls), x_set, g_x, d.reshape(b, v), al, 1e-5, 0.9, kind == "strong_wolfe",
                      kind == "approx_wolfe", 5, 0.0, 0.001)
    ok = ~r["ambiguous"]
    assert ok.mean() >= 0.95
    assert np.array_equal(r["exploration"][ok], gold[p + "exploration"][ok])
    for k in ("exploration_cost", "exploration_action", "exploration_gradient"):
        np.testing.assert_array_equal(r[k][ok], gold[p + k].reshape(r[k].shape)[ok])
    sel, tsel = r["selected"][ok], gold[p + "torch_selected"][ok]
    assert np.array_equal(sel[tsel > 0], tsel[tsel > 0])
    if kind == "strong_wolfe":
        assert np.array_equal(sel, tsel)
    assert (r["current_iteration"] == 1).all() and (r["best_iteration"] == 1).all() and not r["converged"].any()
    np.testing.assert_array_equal(r["best_cost"], r["selected_cost"])


@pytest.mark.parametrize("ad", [1, 7, 14])
def test_step_scale_matches_the_reference(ad):
    """scale_action + jit_get_x_set of the reference at step_scale = 0.98: a dominating element on each action dimension, none,
    a zero direction, random large steps.  The float64 runs agree to rounding, the float32 runs to a few ulp."""
    gs = np.load(os.path.join(GOLDEN_DIR, "step_scale_golden.npz"))
    x, d, step_max, al = (gs[f"ad{ad}_{k}"] for k in ("x", "d", "step_max", "alphas"))
    r = R.prepare_search_points(x, d, step_max, al, ad, True)
    np.testing.assert_allclose(r["d_out"], gs[f"ad{ad}_d_out_f64"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(r["x_set"], gs[f"ad{ad}_x_set_f64"], rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(r["d_out"], gs[f"ad{ad}_d_out_f32"], rtol=4 * R.ULP, atol=0)
    # the rows were built for it: a scale above 1 on the first `ad` rows, exactly 1 on the next two
    assert (r["scale"][:ad] > 2.5).all() and (r["scale"][ad:ad + 2] == 1).all()
    assert np.array_equal(r["d_out"][ad:ad + 2].astype(F32), d[ad:ad + 2])
    for a in range(ad):  # the dominating element lands on +-step_max of ITS action dimension
        v = int(np.argmax(np.abs(d[a].reshape(-1, ad) / step_max).reshape(-1)))
        assert v % ad == a
        np.testing.assert_allclose(abs(r["d_out"][a, v]), step_max[a], rtol=1e-12)
    off = R.prepare_search_points(x, d, step_max, al, ad, False)
    assert np.array_equal(off["d_out"], d.astype(np.float64)) and (off["scale"] == 1).all()
