"""The optimiser side of the L-BFGS iteration (csrc/optimization.hip) against the float64 restatement of the reference's own
definitions, tests/lbfgs_iteration_ref.py, at the shapes where the kernels branch: prepare_search_points, launch_line_search,
launch_lbfgs_step and launch_lbfgs_iteration_tail in every form (16-lane rows, a wavefront per problem, a workgroup per problem
and its staging boundary, the plain kernel, both compile-time shapes with the switch on and off).

Integer outputs are equal and copied tensors bit-equal on every row whose comparisons the reference calls decidable; an
ambiguous row must still copy, bit for bit, the candidates its own indices name, and its float outputs are compared along the
candidate it explored.  Float tolerances: the candidates from the 2.5 ulp quotient documented at div_frexp_rcp (d_out 6 ulp,
x_set 6 ulp of alpha_k d_out + 1 ulp of the result); the two-loop result, which cannot be bounded a priori, within four times
the distance of the reference's float32 run from its float64 run on the same input (floor: 16 ulp of the tensor's largest
magnitude).  Consecutive iterations evaluate the reference from the device's own state, so rounding does not compound.  Every
case prints its float32 gap, bound, device error and flagged rows.  At most 5 % of the rows of a test and 0.5 % of all rows of
the file may be flagged.

Non-finite directions: the kernels take the step scale with fmaxf, which skips a NaN element where torch.max hands it on, so on
a direction with a NaN element the device scales by the finite elements and the reference returns a row of NaN.  Such rows are
compared where the reference is finite (nowhere), must agree bit for bit between the three launches and the one-launch tail,
and must leave their neighbours untouched.

Largest values on the MI355X (step direction, per launch; 19831 rows in 78 tests, 1 flagged: line search V = 257):
launch_lbfgs_step: error 0.377 of the bound (V = 129, stable mode: float32 gap 4.6e-6, bound 4.6e-5, error 1.7e-5); largest gap
3.5e-5 with error 1.2e-4 under a bound of 6.7e-4 (V = 64, stable mode off).  One-launch tail: error 0.702 of the bound in the row
form (V = 16, m = 16, N = 2, B = 17, third iteration: gap 6.2e-4, bound 2.5e-3, error 1.7e-3), at most 0.23 of it in every other
form; largest gap of any launch 1.8e-3.  The candidates and the line search passed at every shape; nothing in
csrc/optimization.hip had to change.
"""

import numpy as np
import pytest
import torch

import lbfgs_iteration_cases as C
import lbfgs_iteration_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32


class _Tally:
    """rows seen and rows flagged, per test and over the file"""

    file_rows = file_flagged = 0

    def __init__(self):
        self.rows = self.flagged = 0
        self.worst = (0.0, 0.0, 0.0, 0.0)  # error / bound of the step, gap, bound, error

    def add(self, rows, flagged, figures=None):
        self.rows, self.flagged = self.rows + rows, self.flagged + flagged
        _Tally.file_rows, _Tally.file_flagged = _Tally.file_rows + rows, _Tally.file_flagged + flagged
        if figures is not None and figures[1] > 0:
            self.worst = max(self.worst, (figures[2] / figures[1],) + tuple(figures))

    def close(self, what):
        print(f"{what}: flagged {self.flagged} of {self.rows} rows; worst step error / bound {self.worst[0]:.3f} "
              f"(gap {self.worst[1]:.3e} bound {self.worst[2]:.3e} error {self.worst[3]:.3e})")
        assert self.flagged <= 0.05 * self.rows, f"{self.flagged} of {self.rows} rows flagged"


def _up(a, device):
    return torch.as_tensor(np.array(a, copy=True, order="C"), device=device)


def _down(t):
    return t.detach().cpu().numpy().copy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------------------------------------------------- a. candidates
PREP_V = (1, 7, 63, 64, 65, 128, 129, 1023)
PREP_N = (1, 4, 5, 64)
PREP_FAMILIES = ("below", "exactly_one", "dominating", "odd_step_max", "zero", "tiny_and_huge", "non_finite")


def _prepare_inputs(family, B, V, ad, seed):
    """x, d [B, V], step_max [ad]; ``exact``: the scale is exactly 1 on every row"""
    rng = np.random.default_rng([seed, B, V, ad, PREP_FAMILIES.index(family)])
    step_max = rng.uniform(0.05, 0.6, size=ad).astype(F32)
    if family == "odd_step_max":  # one action dimension far tighter than all the others
        step_max[:] = 0.5
        step_max[ad - 1] = 0.01
    sm = np.tile(step_max, V // ad)
    x = rng.normal(size=(B, V)).astype(F32)
    d = (0.9 * rng.uniform(-1, 1, size=(B, V)) * sm).astype(F32)  # every |d| / step_max below 1
    if family == "exactly_one":
        for r in range(B):
            v = int(rng.integers(V))
            d[r, v] = sm[v] * (-1) ** r
    if family == "dominating":  # one element far above its limit, at the ends of the lanes' strides
        spots = [v for v in (0, 63, 64, V - 1) if v < V]
        for r in range(B):
            v = spots[(r + seed) % len(spots)]
            d[r, v] = F32((-1) ** r * rng.uniform(3.0, 30.0) * sm[v])
    if family == "odd_step_max":  # 0.45 on the tight dimension: scale 45; read with any other dimension's limit: 0.9 -> no scale
        for r in range(B):
            v = (ad - 1) + ad * int(rng.integers(V // ad))
            d[r] = (0.5 * d[r]).astype(F32)
            d[r, v] = F32(0.45 * (-1) ** r)
    if family == "zero":
        d[:] = 0
    if family == "tiny_and_huge":
        mag = np.where(np.arange(B) % 2 == 0, 1e-30, 1e30)[:, None]
        d = (rng.normal(size=(B, V)) * mag).astype(F32)
        x = (x * mag).astype(F32)
    return x, d, step_max, family in ("below", "zero")


def _device_prepare(device, x, d, step_max, al, ad, scale):
    from curobo_amd.backends import optimization as O

    B, V = d.shape
    N = len(al)
    x_set = torch.full((B, N, V), 7.0, device=device)
    d_out = torch.full((B, V), 7.0, device=device)
    O.prepare_search_points(x_set, d_out, _up(x, device), _up(d, device), _up(step_max, device), _up(al, device), B, N, V, ad, scale)
    return _down(d_out), _down(x_set)


def _check_prepare(ref, d_out, x_set, al, rows, what):
    """d_out within 6 ulp (3 of the scale, 3 of the quotient), x_set within 6 ulp of alpha_k d_out + 1 ulp of the result, where
    the reference is finite"""
    with np.errstate(invalid="ignore", over="ignore"):
        a = ref["d_out"][rows]
        fin = np.isfinite(a)
        err = np.abs(d_out[rows].astype(np.float64) - a)
        assert np.isfinite(d_out[rows][fin]).all() and (err[fin] <= 6 * R.ULP * np.abs(a[fin])).all(), \
            f"d_out: {float((err[fin] / np.maximum(np.abs(a[fin]), 1e-300)).max() / R.ULP):.2f} ulp: {what}"
        xs = ref["x_set"][rows]
        bound = 6 * R.ULP * np.abs(al.astype(np.float64)[None, :, None] * a[:, None, :]) + R.ULP * np.abs(xs)
        fin = np.isfinite(xs)
        err = np.abs(x_set[rows].astype(np.float64) - xs)
        assert np.isfinite(x_set[rows][fin]).all() and (err[fin] <= bound[fin]).all(), \
            f"x_set: {float((err[fin] / np.maximum(bound[fin], 1e-300)).max()):.2f} of its bound: {what}"


@pytest.mark.parametrize("V", PREP_V)
def test_prepare_search_points(V, device):
    i = 0
    for ad in sorted({1, 7 if V % 7 == 0 else 1, V}):
        for N in PREP_N:
            al = C.alphas_for(N)
            for scale in (True, False):
                for family in PREP_FAMILIES:
                    i += 1
                    B = C.BATCHES[i % len(C.BATCHES)]
                    what = f"V={V} action_dim={ad} N={N} scale={scale} {family} B={B}"
                    if family == "non_finite":
                        _prepare_non_finite(device, max(B, 3), V, ad, al, scale, i, what)
                        continue
                    x, d, step_max, exact = _prepare_inputs(family, B, V, ad, i)
                    ref = R.prepare_search_points(x, d, step_max, al, ad, scale)
                    d_out, x_set = _device_prepare(device, x, d, step_max, al, ad, scale)
                    _check_prepare(ref, d_out, x_set, al, np.ones(B, bool), what)
                    if exact or not scale:  # scale exactly 1: the direction comes back bit for bit and x_set is one fma
                        assert (ref["scale"] == 1).all()
                        assert np.array_equal(_bits(d_out), _bits(d)), f"d_out is not d: {what}"
                        err = np.abs(x_set.astype(np.float64) - ref["x_set"])
                        assert (err <= 0.5 * np.spacing(np.abs(x_set)) * (1 + 1e-6)).all(), f"x_set is not one fma: {what}"
                    elif family in ("dominating", "odd_step_max"):
                        assert (ref["scale"] > 2.5).all()


def _prepare_non_finite(device, B, V, ad, al, scale, seed, what):
    """row 1 holds a NaN and a +inf element, the last row a +inf element alone; the finite rows equal, bit for bit, the same rows of
    a batch without them"""
    x, d, step_max, _ = _prepare_inputs("dominating", B, V, ad, seed)
    clean = _device_prepare(device, x, d, step_max, al, ad, scale)
    bad = d.copy()
    bad[1, 0], bad[1, V - 1] = np.nan, np.inf  # (V = 1: the +inf replaces the NaN)
    bad[B - 1, V // 2] = np.inf
    got = _device_prepare(device, x, bad, step_max, al, ad, scale)
    finite_rows = np.isfinite(bad).all(-1)
    assert finite_rows.sum() == B - 2
    for a, b, k in zip(got, clean, ("d_out", "x_set")):
        assert np.array_equal(_bits(a[finite_rows]), _bits(b[finite_rows])), f"{k}: a finite row changed next to a non-finite one: {what}"
    ref = R.prepare_search_points(x, bad, step_max, al, ad, scale)
    _check_prepare(ref, got[0], got[1], al, np.ones(B, bool), what)
    if scale and V > 1:  # +inf alone: scale = inf, every finite element -> 0 and x_set = x there
        v = np.arange(V) != V // 2
        assert (got[0][B - 1, v] == 0).all() and np.array_equal(got[1][B - 1][:, v], np.broadcast_to(x[B - 1, v], (len(al), v.sum())))


# ---------------------------------------------------------------------------------------------------------- b. line search
_LS_OUT = dict(exploration_cost="b", exploration_action="bv", exploration_gradient="bv", selected_cost="b", selected_action="bv",
               selected_gradient="bv")


def _device_line_search(device, case, strong, approx, thr):
    from curobo_amd.backends import optimization as O

    B, N, V = case["search_gradient"].shape
    dv = {k: _up(v, device) for k, v in case["state"].items()}
    dv["converged"] = torch.full((B,), 9, dtype=torch.uint8, device=device)
    for k, shape in _LS_OUT.items():
        dv[k] = torch.full((B, V) if shape == "bv" else (B,), 7.0, device=device)
    dv["exploration_idx"] = torch.full((B * N,), -7, dtype=torch.int32, device=device)
    dv["selected_idx"] = torch.full((B * N,), -7, dtype=torch.int32, device=device)
    O.launch_line_search(dv["best_cost"], dv["best_action"], dv["best_iteration"], dv["current_iteration"], dv["converged"],
                         C.LS["convergence_iteration"], thr[0], thr[1], dv["exploration_cost"], dv["exploration_action"],
                         dv["exploration_gradient"], dv["exploration_idx"], dv["selected_cost"], dv["selected_action"],
                         dv["selected_gradient"], dv["selected_idx"], _up(case["search_cost"].reshape(B, N, 1), device),
                         _up(case["search_action"], device), _up(case["search_gradient"], device), _up(case["step_direction"], device),
                         _up(case["alphas"], device), C.LS["c_1"], C.LS["c_2"], strong, approx, N, V, B)
    out = {k: _down(v) for k, v in dv.items()}
    out["exploration_idx"], out["selected_idx"] = out["exploration_idx"].reshape(B, N), out["selected_idx"].reshape(B, N)
    return out


def _check_line_search(ref, got, state, cost, action, gradient, what):
    """unambiguous rows: integers equal, copies bit-equal to the rows the reference's indices select.  Ambiguous rows: the indices
    are one candidate each and the copies are bit-equal to the rows THEY select.  No non-finite best cost anywhere."""
    B, N, V = gradient.shape
    ok = ~ref["ambiguous"]
    for k in R.LS_INTEGER:
        assert np.array_equal(got[k][ok], ref[k][ok]), f"{k}: {what}: {got[k][ok].tolist()} != {ref[k][ok].tolist()}"
    for k in R.LS_COPIED:
        assert np.array_equal(_bits(got[k][ok]), _bits(np.ascontiguousarray(ref[k][ok]))), f"{k} is not the selected row: {what}"
    assert np.isfinite(got["best_cost"]).all(), f"a non-finite cost reached best_cost: {what}"
    rows = np.arange(B)
    cost = cost.reshape(B, N)
    for r in rows[~ok]:
        e, s = int(got["exploration_idx"][r, 0]), int(got["selected_idx"][r, 0])
        assert 0 <= e < N and 0 <= s < N and (got["exploration_idx"][r] == e).all() and (got["selected_idx"][r] == s).all(), what
        for k, src, i in (("exploration_cost", cost, e), ("selected_cost", cost, s), ("exploration_action", action, e),
                          ("exploration_gradient", gradient, e), ("selected_action", action, s), ("selected_gradient", gradient, s)):
            assert np.array_equal(_bits(got[k][r]), _bits(src[r, i])), f"{k} of the ambiguous row {r} is not its own row {i}: {what}"
        assert got["current_iteration"][r] == state["current_iteration"][r] + 1
        kept = np.array_equal(_bits(got["best_cost"][r]), _bits(state["best_cost"][r]))
        assert np.array_equal(_bits(got["best_action"][r]), _bits(state["best_action"][r] if kept else action[r, s])), what


@pytest.mark.parametrize("V", C.LS_V)
def test_line_search(V, device):
    tally = _Tally()
    for N, wolfe, thr, family, B, i in C.line_search_sweep(V):
        case = C.line_search_case(B, V, N, family, i)
        strong, approx = C.wolfe_flags(wolfe, N)
        ref = R.line_search(case["state"], case["search_cost"], case["search_action"], case["search_gradient"], case["step_direction"],
                            case["alphas"], C.LS["c_1"], C.LS["c_2"], strong, approx, C.LS["convergence_iteration"], thr[0], thr[1])
        got = _device_line_search(device, case, strong, approx, thr)
        _check_line_search(ref, got, case["state"], case["search_cost"], case["search_action"], case["search_gradient"],
                           f"V={V} N={N} {wolfe} thresholds={thr} {family} B={B}")
        tally.add(B, int(ref["ambiguous"].sum()))
    tally.close(f"line search V={V}")


# ---------------------------------------------------------------------------------------------------------- c. L-BFGS step
def _shifted(before, after, m, what):
    """slots 0 .. m-2 are the old slots 1 .. m-1, bit for bit"""
    for k in ("y", "s", "rho"):
        if m > 1:
            assert np.array_equal(_bits(after[k][:m - 1]), _bits(before[k][1:])), f"{k}: the history did not shift by one: {what}"


@pytest.mark.parametrize("stable", [True, False])
@pytest.mark.parametrize("V", (1,) + C.STEP_V)
def test_lbfgs_step(V, stable, device):
    from curobo_amd.backends import optimization as O

    tally = _Tally()
    for i, m in enumerate((5,) if V == 1 else C.STEP_M):
        B = C.BATCHES[(V + i) % len(C.BATCHES)]
        case = C.lbfgs_case(B, V, m, seed=V + m)
        dv = {k: _up(case[k], device) for k in ("rho", "y", "s", "x_0", "grad_0")}
        dv["step"] = torch.full((B, V), 7.0, device=device)
        q, g = case["q"], case["grad_q"]
        for it in range(3):
            st = {k: _down(v) for k, v in dv.items()}
            what = f"V={V} m={m} B={B} stable={stable} step {it}"
            r64 = R.lbfgs_step(st["rho"], st["y"], st["s"], q, g, st["x_0"], st["grad_0"], C.EPSILON, stable)
            r32 = R.lbfgs_step(st["rho"], st["y"], st["s"], q, g, st["x_0"], st["grad_0"], C.EPSILON, stable, np.float32)
            O.launch_lbfgs_step(dv["step"], dv["rho"], dv["y"], dv["s"], _up(q, device), _up(g, device), dv["x_0"], dv["grad_0"], C.EPSILON,
                                B, m, V, stable, True)
            got = {k: _down(v) for k, v in dv.items()}
            worst, flagged, fig = R.check_step(r64, r32, got, what)
            _shifted(st, got, m, what)
            print(f"{what}: gap {fig[0]:.3e} bound {fig[1]:.3e} error {fig[2]:.3e} worst error / bound {worst:.3f} flagged {flagged}")
            tally.add(B, flagged, fig)
            if stable and m > 0 and B > 1 and it == 0:
                assert got["rho"][-1, 1] == 0, f"negative curvature must give rho = 0: {what}"
            if m > 0 and B >= 3 and it == 2:  # the planted exact zero: decidable, compared above, and of the expected kind
                assert not r64["flagged"][-1] and (got["rho"][-1, -1] == 0 if stable else np.isinf(got["rho"][-1, -1])), what
            q, g = C.lbfgs_next(case, q, got["step"], got["x_0"], got["grad_0"], it)
    tally.close(f"L-BFGS step V={V} stable={stable}")


# ---------------------------------------------------------------------------------------------------------- d. one launch
_TAIL_STATE = ("y", "s", "rho", "x_0", "grad_0", "step_direction", "x_set", "step_scaled", "exploration_cost", "exploration_action",
               "exploration_gradient", "exploration_idx", "selected_cost", "selected_action", "selected_gradient", "selected_idx",
               "best_cost", "best_action", "best_iteration", "current_iteration", "converged")


def _tail_device_state(case, device):
    B, N, V = case["x_set"].shape
    dv = {k: _up(case[k], device) for k in ("y", "s", "rho", "x_0", "grad_0", "step_direction", "x_set", "step_scaled", "best_cost",
                                            "best_action", "best_iteration", "current_iteration")}
    for k, shape in _LS_OUT.items():
        dv[k] = torch.full((B, V) if shape == "bv" else (B,), 7.0, device=device)
    dv["converged"] = torch.full((B,), 9, dtype=torch.uint8, device=device)
    dv["exploration_idx"] = torch.full((B, N), -7, dtype=torch.int32, device=device)
    dv["selected_idx"] = torch.full((B, N), -7, dtype=torch.int32, device=device)
    return dv


def _ls_args(dv, cost, grad, case, cfg):
    B, N, V = case["x_set"].shape
    strong, approx = C.wolfe_flags(cfg["wolfe"], N)
    return (dv["best_cost"], dv["best_action"], dv["best_iteration"], dv["current_iteration"], dv["converged"],
            C.LS["convergence_iteration"], cfg["thr"][0], cfg["thr"][1], dv["exploration_cost"], dv["exploration_action"],
            dv["exploration_gradient"], dv["exploration_idx"].view(-1), dv["selected_cost"], dv["selected_action"],
            dv["selected_gradient"], dv["selected_idx"].view(-1), cost, dv["x_set"], grad, dv["step_scaled"], cfg["alphas"],
            C.LS["c_1"], C.LS["c_2"], strong, approx, N, V, B)


def _run_tail(device, tally, B, V, m, N, overlapped, expect, wolfe="approx", thr=C.THRESHOLDS[1], stable=True, scale=True,
              non_finite=False, seed=0):
    """three consecutive one-launch iterations; after each, every output against iteration_tail of the reference evaluated from the
    state the device held before it"""
    from curobo_amd.backends import optimization as O

    case = C.tail_case(B, V, m, N, seed)
    ad = case["action_dim"]
    assert O.tail_form(V, m, N, ad, B, overlapped) == expect, f"V={V} m={m} N={N} B={B} overlapped={overlapped}"
    dv = _tail_device_state(case, device)
    cfg = dict(wolfe=wolfe, thr=thr, alphas=_up(case["alphas"], device))
    step_max = _up(case["step_max"], device)
    strong, approx = C.wolfe_flags(wolfe, N)
    for it in range(3):
        what = f"form={expect} V={V} m={m} N={N} B={B} overlapped={overlapped} {wolfe} stable={stable} scale={scale} " \
               f"non_finite={non_finite} iteration {it}"
        st = {k: _down(dv[k]) for k in _TAIL_STATE}
        cost, grad = C.tail_rollout(case, st["x_set"], it, non_finite)
        d_cost, d_grad = _up(cost.reshape(B, N, 1), device), _up(grad, device)
        if non_finite:  # the three launches from the same state: the kernels' rule for a NaN direction is one rule
            three = {k: v.clone() for k, v in dv.items()}
            O.launch_line_search(*_ls_args(three, d_cost, d_grad, case, cfg))
            O.launch_lbfgs_step(three["step_direction"], three["rho"], three["y"], three["s"], three["exploration_action"],
                                three["exploration_gradient"], three["x_0"], three["grad_0"], C.EPSILON, B, m, V, stable, True)
            O.prepare_search_points(three["x_set"], three["step_scaled"], three["exploration_action"], three["step_direction"], step_max,
                                    cfg["alphas"], B, N, V, ad, scale)
        O.launch_lbfgs_iteration_tail(*_ls_args(dv, d_cost, d_grad, case, cfg), dv["step_direction"], dv["rho"], dv["y"], dv["s"],
                                      dv["x_0"], dv["grad_0"], C.EPSILON, m, stable, step_max, ad, scale, overlapped=overlapped)
        got = {k: _down(dv[k]) for k in _TAIL_STATE}
        if non_finite:
            for k in _TAIL_STATE:
                assert np.array_equal(_bits(got[k]), _bits(_down(three[k]))), f"{k}: the one launch and the three launches differ: {what}"
        args = (cost, grad, case["alphas"], case["step_max"], ad, scale, C.LS["c_1"], C.LS["c_2"], strong, approx,
                C.LS["convergence_iteration"], thr[0], thr[1], C.EPSILON, stable)
        r64 = R.iteration_tail(st, *args, device_exploration=got["exploration_idx"][:, 0])
        follow = np.where(r64["ambiguous"], np.clip(got["exploration_idx"][:, 0], 0, N - 1), r64["line_search"]["exploration"])
        r32 = R.iteration_tail(st, *args, dtype=np.float32, device_exploration=follow, follow=np.ones(B, bool))
        _check_line_search(r64["line_search"], got, st, cost, st["x_set"], grad, what)
        _, _, fig = R.check_step(r64["lbfgs"], r32["lbfgs"], dict(got, step=got["step_direction"]), what)
        _shifted(st, got, m, what)
        ok = ~r64["lbfgs"]["flagged"]
        # (a row whose direction has a NaN element: the kernel scales by the finite ones, the reference returns NaN)
        R.check_close("step_scaled", r64["prepare"]["d_out"], r32["prepare"]["d_out"], got["step_scaled"], ok, what, same_pattern=False)
        R.check_close("x_set", r64["prepare"]["x_set"], r32["prepare"]["x_set"], got["x_set"], ok, what, same_pattern=False)
        finite_dir = np.isfinite(got["step_direction"]).all(-1) & ok
        R.check_close("step_scaled", r64["prepare"]["d_out"], r32["prepare"]["d_out"], got["step_scaled"], finite_dir, what)
        R.check_close("x_set", r64["prepare"]["x_set"], r32["prepare"]["x_set"], got["x_set"], finite_dir, what)
        flagged = int((r64["ambiguous"] | r64["lbfgs"]["flagged"]).sum())
        print(f"{what}: gap {fig[0]:.3e} bound {fig[1]:.3e} error {fig[2]:.3e} flagged {flagged}")
        tally.add(B, flagged, fig)


def _rotate(i):
    return dict(wolfe=C.WOLFE[i % 3], thr=C.THRESHOLDS[i % 2], stable=i % 4 != 3, scale=i % 5 != 4, seed=i)


@pytest.mark.parametrize("V", [1, 7, 16])
def test_tail_row_form(V, device):
    from curobo_amd.backends.optimization import TAIL_ROW

    tally = _Tally()
    for i, m in enumerate((0, 1, 16)):
        for j, B in enumerate((1, 5, 17)):
            N = (1, 2, 4)[(i + j) % 3]
            shape = 2 if (V, m, N) == (7, 7, 4) else 0
            _run_tail(device, tally, B, V, m, N, bool(j & 1), (TAIL_ROW, shape), non_finite=(m == 1 and B == 17), **_rotate(3 * i + j))
    tally.close(f"tail, row form V={V}")


@pytest.mark.parametrize("overlapped", [False, True])
@pytest.mark.parametrize("V", [1, 17, 63, 64, 65, 84, 128])
def test_tail_wavefront_and_workgroup_forms(V, overlapped, device):
    from curobo_amd.backends.optimization import TAIL_WAVE, TAIL_WORKGROUP

    tally = _Tally()
    form = TAIL_WAVE if overlapped else TAIL_WORKGROUP
    for i, m in enumerate((31,) if V == 1 else (0, 1, 2, 17, 27, 31)):
        B, N = C.BATCHES[(i + V) % len(C.BATCHES)], (1, 2, 4)[(i + V) % 3]
        if (V, m) == (84, 27):
            N = 2  # (N = 4 is the compile-time shape: test_tail_compile_time_shapes)
        _run_tail(device, tally, B, V, m, N, overlapped, (form, 0), non_finite=(V == 65 and m in (0, 2)), **_rotate(i + V))
    tally.close(f"tail, {'wavefront' if overlapped else 'workgroup'} form V={V}")


@pytest.mark.parametrize("m", [19, 20])
def test_tail_workgroup_staging_boundary(m, device):
    """V = 128: m = 19 moves 18 x 128 = 12 x 192 floats per array, exactly the 12 rounds of the smaller instantiation; m = 20 takes
    the 20-round one"""
    from curobo_amd.backends.optimization import TAIL_WORKGROUP

    tally = _Tally()
    for i, B in enumerate((1, 3, 5)):
        _run_tail(device, tally, B, 128, m, (4, 2, 1)[i], False, (TAIL_WORKGROUP, 0), **_rotate(i + m))
    tally.close(f"tail, workgroup form V=128 m={m}")


@pytest.mark.parametrize("N", [5, 16, 17, 64])
def test_tail_plain_kernel(N, device):
    from curobo_amd.backends.optimization import TAIL_PLAIN

    tally = _Tally()
    for i, (V, m) in enumerate(((7, 7), (84, 27), (65, 2), (16, 16), (128, 31))):
        _run_tail(device, tally, C.BATCHES[(i + N) % len(C.BATCHES)], V, m, N, bool(i & 1), (TAIL_PLAIN, 0),
                  non_finite=(V == 65 and N in (5, 64)) or (V == 7 and N == 16), **_rotate(i + N))
    tally.close(f"tail, plain kernel N={N}")


@pytest.mark.parametrize("enabled", [True, False])
@pytest.mark.parametrize("name", ["trajopt_wave", "trajopt_workgroup", "ik_row"])
def test_tail_compile_time_shapes(name, enabled, device):
    from curobo_amd.backends.optimization import TAIL_ROW, TAIL_WAVE, TAIL_WORKGROUP, set_tail_shapes_enabled

    V, m, N, overlapped, form, shape, batches = {
        "trajopt_wave": (84, 27, 4, True, TAIL_WAVE, 1, (3, 4, 5)),
        "trajopt_workgroup": (84, 27, 4, False, TAIL_WORKGROUP, 1, (1, 3, 5)),
        "ik_row": (7, 7, 4, False, TAIL_ROW, 2, (4, 5, 17)),
    }[name]
    tally = _Tally()
    set_tail_shapes_enabled(enabled)
    try:
        for i, B in enumerate(batches):
            _run_tail(device, tally, B, V, m, N, overlapped, (form, shape if enabled else 0), non_finite=(i == 2), **_rotate(i))
    finally:
        set_tail_shapes_enabled(True)
    tally.close(f"tail, shape {name} enabled={enabled}")


def test_zz_flagged_rows_of_the_file():
    """a flagged row hides a failure: at most 0.5 % of all rows the tests above compared"""
    print(f"flagged {_Tally.file_flagged} of {_Tally.file_rows} rows")
    assert _Tally.file_flagged <= 0.005 * _Tally.file_rows
