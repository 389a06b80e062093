"""The optimiser side of one L-BFGS iteration, restated in NumPy from the reference's own definitions: the candidate
generation of ``scale_action`` + ``jit_get_x_set`` (optim/gradient/line_search_strategy.py:281-328), the Wolfe line search
and its best / convergence bookkeeping (line_search_helpers.cuh:18-316) and the L-BFGS step (lbfgs_step_helpers.cuh:37-470).

Every function takes the float32 arrays the device sees and computes in ``dtype``: float64 is the reference, float32 measures how far
plain float32 arithmetic moves from it (the tolerance of the two-loop result is four times that gap, ``tolerance``).

Which rows are comparable.  The integer outputs hang on comparisons of rounded quantities, so every function also says, row by
row, whether its comparisons are decidable:

* the only inexact inputs of the Wolfe tests are the dot products g_k . d.  A float32 evaluation of one is within
  ``(ceil(V / 16) + 8) 2^-24 sum|g_v d_v|`` of the exact value (terms per lane of the narrowest lane group, the reduction steps, 2
  to spare).  Each comparison is evaluated in float32, as written (``cv <= c0 + c_1 alpha gd0`` with product and sum rounded
  separately and contracted into one rounding; ``gd_k >= c_2 gd0`` or ``|gd_k| <= c_2 |gd0|``), at the float64 dot products and
  at both ends of their error intervals.  A comparison whose outcomes differ makes the row AMBIGUOUS.  A comparison with a NaN is
  false everywhere and never ambiguous;
* ``update_best = delta > thr_d && rel > thr_r``: ``delta`` is one correctly rounded subtraction, ``rel`` a quotient that is
  good to 2.5 ulp on the device: ambiguous only when ``rel`` lies within 4 ulp of a non-zero ``thr_r``;
* the L-BFGS step flags a row when y.s or y.y is inside its own rounding bound of zero without being exactly zero (the sign of
  y.s and the finiteness of y.s / y.y are then not decided).  An exact zero (g = grad_0, x = x_0) is decidable.
"""

import numpy as np

F32 = np.float32
ULP = 2.0 ** -23  # spacing of float32 relative to the binade's lower end
_EPS_DOT = 2.0 ** -24


def _sum(a, dtype):
    """sum over the last axis in ``dtype``; the float32 run adds in index order (no pairwise tree), as the oracle does: the gap it
    measures is that of plain float32 code"""
    if dtype == np.float64:
        return a.sum(-1, dtype=dtype)
    return np.cumsum(a, axis=-1, dtype=dtype)[..., -1]


def dot_error_bound(a, b):
    """bound on |float32 evaluation - exact value| of sum_v a_v b_v over the last axis (any order, fused or not)"""
    V = a.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.ceil(V / 16.0) + 8.0) * _EPS_DOT * np.abs(a.astype(np.float64) * b.astype(np.float64)).sum(-1)


# ---------------------------------------------------------------------------------------------------------- candidates
def prepare_search_points(x, d, step_max, alphas, action_dim, apply_scale, dtype=np.float64):
    """scale_action (step_scale not in {0, 1} <=> apply_scale; no fix_terminal_action) then jit_get_x_set.
    x, d [B, V]; step_max [action_dim]; alphas [N].  Returns scale [B], d_out [B, V], x_set [B, N, V]; a NaN in a row of
    d makes the whole row NaN, as torch.max and torch.clamp propagate it."""
    B, V = d.shape
    assert V % action_dim == 0 and step_max.shape == (action_dim,)
    xd, dd, al = x.astype(dtype), d.astype(dtype), alphas.astype(dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if apply_scale:
            diff = np.abs(dd).reshape(B, V // action_dim, action_dim) / step_max.astype(dtype).reshape(1, 1, action_dim)
            scale = np.maximum(diff.reshape(B, -1).max(-1), dtype(1.0))  # (np.max and np.maximum propagate NaN like torch)
            d_out = dd / scale[:, None]
        else:
            scale, d_out = np.ones(B, dtype), dd
        x_set = xd[:, None, :] + al[None, :, None] * d_out[:, None, :]
    return dict(scale=scale, d_out=d_out, x_set=x_set)


# ---------------------------------------------------------------------------------------------------------- line search
def _armijo(cv, c0, ca, gd0):
    """cv <= c0 + (c_1 alpha) gd0 in float32: separate roundings and one contracted rounding"""
    with np.errstate(invalid="ignore", over="ignore"):
        sep = cv <= (c0 + (ca * gd0).astype(F32)).astype(F32)
        fma = cv <= (c0.astype(np.float64) + ca.astype(np.float64) * gd0.astype(np.float64)).astype(F32)
    return sep, fma


def _curvature(gdk, gd0, c_2, strong):
    with np.errstate(invalid="ignore", over="ignore"):
        if strong:
            return np.abs(gdk) <= (c_2 * np.abs(gd0)).astype(F32)
        return gdk >= (c_2 * gd0).astype(F32)


def line_search(state, search_cost, search_action, search_gradient, step_direction, alphas, c_1, c_2, strong_wolfe,
                approx_wolfe, convergence_iteration, cost_delta_threshold, cost_relative_threshold, dtype=np.float64):
    """state: best_cost [B], best_action [B, V], best_iteration, current_iteration (int16 [B]).  search_cost [B, N],
    search_action / search_gradient [B, N, V], step_direction [B, V], alphas [N].  Returns the new state and outputs in a
    dictionary (nothing is modified) with ``ambiguous`` [B] and the row indices ``selected`` / ``exploration`` [B]."""
    B, N, V = search_gradient.shape
    cost = search_cost.reshape(B, N).astype(F32)
    c_1, c_2, thr_d, thr_r = F32(c_1), F32(c_2), F32(cost_delta_threshold), F32(cost_relative_threshold)
    with np.errstate(invalid="ignore", over="ignore"):
        gd = _sum(search_gradient.astype(dtype) * step_direction.astype(dtype)[:, None, :], dtype)  # [B, N]
    mid = gd.astype(F32)
    if dtype == np.float64:
        err = dot_error_bound(search_gradient, np.broadcast_to(step_direction[:, None, :], search_gradient.shape))
        with np.errstate(invalid="ignore", over="ignore"):
            variants = [(gd - err).astype(F32), mid, (gd + err).astype(F32)]
    else:
        variants = [mid]
    ca = (c_1 * alphas.astype(F32)).astype(F32)[None, :]
    c0 = cost[:, :1]
    w1 = w2 = None
    amb = np.zeros(B, bool)
    for g0v in variants:
        for form in _armijo(cost, c0, ca, g0v[:, :1]):
            if w1 is None:
                w1 = _armijo(cost, c0, ca, mid[:, :1])[0]
            amb |= (form != w1).any(-1)
        for gkv in variants:
            # candidate 0 is compared with itself: the same evaluation on both sides
            gk = np.concatenate([g0v[:, :1], gkv[:, 1:]], axis=1)
            c = _curvature(gk, g0v[:, :1], c_2, strong_wolfe)
            if w2 is None:
                w2 = _curvature(mid, mid[:, :1], c_2, strong_wolfe)
            amb |= (c != w2).any(-1)
    both = w1 & w2
    idx = np.arange(N)[None, :]
    id1 = np.where(w1, idx, 0).max(-1)  # largest passing index, 0 if none passes
    idb = np.where(both, idx, 0).max(-1)
    sel = idb if strong_wolfe else np.where(idb == 0, id1, idb)  # Armijo-only fallback unless strong Wolfe
    expl = np.where(sel == 0, 1, sel) if (approx_wolfe and not strong_wolfe) else sel
    rows = np.arange(B)
    sc, ec = cost[rows, sel], cost[rows, expl]
    bc = state["best_cost"].astype(F32)
    cur = state["current_iteration"].astype(np.int64) + 1
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        delta = (bc - sc).astype(F32)
        den = (bc + F32(1e-6)).astype(F32)
        rel = (delta.astype(np.float64) / den.astype(np.float64)).astype(F32)
        pass_d = delta > thr_d
        update = pass_d & (rel > thr_r)
        if thr_r != 0 and dtype == np.float64:
            amb |= pass_d & (np.abs(rel.astype(np.float64) - float(thr_r)) <= 4.0 * np.spacing(thr_r))
    bi = np.where(update, cur, state["best_iteration"].astype(np.int64))
    out = dict(
        ambiguous=amb, selected=sel, exploration=expl, update_best=update,
        exploration_cost=ec, selected_cost=sc,
        exploration_action=search_action[rows, expl], exploration_gradient=search_gradient[rows, expl],
        selected_action=search_action[rows, sel], selected_gradient=search_gradient[rows, sel],
        exploration_idx=np.repeat(expl[:, None], N, 1).astype(np.int32), selected_idx=np.repeat(sel[:, None], N, 1).astype(np.int32),
        best_cost=np.where(update, sc, bc).astype(F32),
        best_action=np.where(update[:, None], search_action[rows, sel], state["best_action"]).astype(F32),
        best_iteration=bi.astype(np.int16), current_iteration=cur.astype(np.int16),
        converged=(bi + int(convergence_iteration) < cur).astype(np.uint8))
    return out


LS_INTEGER = ("selected_idx", "exploration_idx", "best_iteration", "current_iteration", "converged")
LS_COPIED = ("exploration_cost", "selected_cost", "exploration_action", "exploration_gradient", "selected_action",
             "selected_gradient", "best_cost", "best_action")


# ---------------------------------------------------------------------------------------------------------- L-BFGS step
def lbfgs_step(rho, y, s, q, grad_q, x_0, grad_0, epsilon, stable_mode, dtype=np.float64):
    """rho [m, B], y / s [m, B, V], q / grad_q / x_0 / grad_0 [B, V] (nothing is modified).  History shift and append,
    rho = 1 / (y.s) with the stable-mode rule y.s <= 0 -> rho = 0, two-loop recursion, gamma = relu(y.s / y.y) with epsilon in
    place of a quotient that is not finite (stable mode).  Returns step, rho, y, s, x_0, grad_0 in ``dtype`` and ``flagged`` [B]."""
    m, (B, V) = y.shape[0], q.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = grad_q.astype(dtype)
        y_new, s_new = g - grad_0.astype(dtype), q.astype(dtype) - x_0.astype(dtype)
        num = _sum(y_new * s_new, dtype)
        den = _sum(y_new * y_new, dtype)
        # the device forms y and s in float32 (one rounding each) before the products: two more ulp on every term
        e_num = dot_error_bound(y_new.astype(F32), s_new.astype(F32)) + 2 * ULP * np.abs(y_new * s_new).sum(-1)
        e_den = dot_error_bound(y_new.astype(F32), y_new.astype(F32)) + 2 * ULP * den
        flagged = ((num != 0) & (np.abs(num) <= e_num)) | ((den != 0) & (np.abs(den) <= e_den))
        Y, S, R = y.astype(dtype), s.astype(dtype), rho.astype(dtype)
        if m > 0:
            Y = np.concatenate([Y[1:], y_new[None]], 0)
            S = np.concatenate([S[1:], s_new[None]], 0)
            r_new = dtype(1.0) / num
            if stable_mode:
                r_new = np.where(num <= 0, dtype(0.0), r_new)
            R = np.concatenate([R[1:], r_new[None]], 0)
        gq = g.copy()
        alpha = np.zeros((m, B), dtype)
        for i in range(m - 1, -1, -1):
            alpha[i] = _sum(gq * S[i], dtype) * R[i]
            gq = gq - alpha[i][:, None] * Y[i]
        if m > 0:
            var1 = num / den
            if stable_mode:
                bad = ~np.isfinite(var1)
                if dtype == np.float64:  # finite here, not finite in float32: not decided
                    flagged |= ~bad & ~np.isfinite(var1.astype(F32))
                var1 = np.where(bad, dtype(epsilon), var1)
            gamma = np.where(var1 < 0, dtype(0.0), var1)
            gq = gamma[:, None] * gq
        for i in range(m):
            beta = alpha[i] - _sum(gq * Y[i], dtype) * R[i]
            gq = gq + beta[:, None] * S[i]
    return dict(step=-gq, rho=R, y=Y, s=S, x_0=q.astype(dtype), grad_0=g, flagged=flagged)


LBFGS_FLOAT = ("step", "rho", "y", "s")


# ---------------------------------------------------------------------------------------------------------- one iteration
def iteration_tail(st, search_cost, search_gradient, alphas, step_max, action_dim, apply_scale, c_1, c_2, strong_wolfe, approx_wolfe,
                   convergence_iteration, cost_delta_threshold, cost_relative_threshold, epsilon, stable_mode, dtype=np.float64,
                   device_exploration=None, follow=None):
    """LBFGSOpt._opt_step's optimiser side: line search over the evaluated candidates ``st["x_set"]`` along
    ``st["step_scaled"]``, the L-BFGS step from the exploration point, the next candidates from it.
    st: best_cost, best_action, best_iteration, current_iteration, x_set, step_scaled, rho, y, s, x_0, grad_0."""
    ls = line_search(st, search_cost, st["x_set"], search_gradient, st["step_scaled"], alphas, c_1, c_2, strong_wolfe, approx_wolfe,
                     convergence_iteration, cost_delta_threshold, cost_relative_threshold, dtype)
    x_e, g_e = ls["exploration_action"], ls["exploration_gradient"]
    if device_exploration is not None:  # an ambiguous row (or every row of ``follow``) takes the candidate it is given
        B, N = search_gradient.shape[:2]
        k = np.where(ls["ambiguous"] if follow is None else follow, np.clip(device_exploration, 0, N - 1), ls["exploration"])
        x_e, g_e = st["x_set"][np.arange(B), k], search_gradient[np.arange(B), k]
    lb = lbfgs_step(st["rho"], st["y"], st["s"], x_e, g_e, st["x_0"], st["grad_0"], epsilon, stable_mode, dtype)
    # (the candidates are made from the step in ``dtype``, not from its float32 rounding: the device hands it over in registers)
    pr = prepare_search_points(x_e, lb["step"], step_max, alphas, action_dim, apply_scale, dtype)
    return dict(line_search=ls, lbfgs=lb, prepare=pr, ambiguous=ls["ambiguous"], flagged=ls["ambiguous"] | lb["flagged"])


# ---------------------------------------------------------------------------------------------------------- tolerance
def tolerance(ref64, ref32, rows):
    """(gap, bound) for one tensor with the problem axis first (``rows_first``); ``rows`` [B] selects the problems that count.
    gap = largest |float32 run - float64 run| over the finite entries of those rows; bound = max(4 gap, 16 ulp of the tensor's
    largest magnitude)."""
    a, b = np.asarray(ref64, np.float64)[rows], np.asarray(ref32, np.float64)[rows]
    fin = np.isfinite(a) & np.isfinite(b)
    gap = float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0
    fa = np.isfinite(a)
    mag = float(np.abs(a[fa]).max()) if fa.any() else 0.0
    return gap, max(4.0 * gap, 16.0 * ULP * mag)


def rows_first(name, a):
    """the problem axis of a state tensor first: rho [m, B] -> [B, m]; y / s [m, B, V] -> [B, m, V]"""
    a = np.asarray(a)
    if name == "rho":
        return a.T
    if name in ("y", "s"):
        return a.transpose(1, 0, 2)
    return a


def check_close(name, ref64, ref32, got, rows, what, same_pattern=True):
    """one float tensor (problem axis first) against the reference on the problems ``rows``: the finite pattern equal (or, with
    same_pattern off, only the entries the reference leaves finite looked at), the finite entries within ``tolerance``.
    Returns (gap, bound, error)."""
    gap, bound = tolerance(ref64, ref32, rows)
    a, c = np.asarray(ref64, np.float64)[rows], np.asarray(got, np.float64)[rows]
    fin = np.isfinite(a)
    if same_pattern:
        assert np.array_equal(np.isfinite(c), fin), f"{name}: finite pattern differs: {what}"
    else:
        assert np.isfinite(c[fin]).all(), f"{name}: not finite where the reference is: {what}"
    err = float(np.abs(a[fin] - c[fin]).max()) if fin.any() else 0.0
    assert err <= bound, f"{name}: error {err:.3e} above the bound {bound:.3e} (float32 gap {gap:.3e}): {what}"
    return gap, bound, err


def check_step(r64, r32, got, what):
    """the outputs of one L-BFGS step (got: step, rho, y, s, x_0, grad_0 as float32) against the float64 run r64 within four
    times its distance from the float32 run r32; x_0 / grad_0 are copies: exact.  y and s do not hang on the flagged decisions
    and are compared on every row, step and rho on the unflagged ones.  Returns (worst error / bound, flagged rows, figures of
    the step: gap, bound, error)."""
    ok = ~r64["flagged"]
    worst, of_step = 0.0, (0.0, 0.0, 0.0)
    for k in ("x_0", "grad_0"):
        assert np.array_equal(np.asarray(got[k]).view(np.int32), r64[k].astype(F32).view(np.int32)), f"{k} is not a copy: {what}"
    for k in LBFGS_FLOAT:
        a, b, c = (rows_first(k, t[k]) for t in (r64, r32, got))
        g = check_close(k, a, b, c, ok if k in ("step", "rho") else np.ones_like(ok), what)
        if g[1] > 0:
            worst = max(worst, g[2] / g[1])
        if k == "step":
            of_step = g
    return worst, int(r64["flagged"].sum()), of_step
