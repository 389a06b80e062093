"""Inputs of the L-BFGS iteration tests, shared by the CPU pins of the reference (test_lbfgs_iteration_ref_host.py), the GPU
tests (test_gpu_lbfgs_iteration.py) and the fuzzer (randomised/fuzz_lbfgs_iteration.py): NumPy only, float32 as the device sees
them, every array a pure function of its arguments."""

import numpy as np

F32 = np.float32
BATCHES = (1, 3, 4, 5, 17)  # ragged 4-problem workgroups, ragged 16-problem row workgroups, the 16 / 17 row boundary
LS = dict(c_1=1e-5, c_2=0.9, convergence_iteration=5)
THRESHOLDS = ((0.0, 0.0), (1e-4, 1e-3))
WOLFE = ("weak", "strong", "approx")
EPSILON = 0.01

# ---------------------------------------------------------------------------------------------------------- line search
LS_V = (1, 7, 16, 17, 63, 64, 65, 128, 129, 257)
LS_N = (1, 2, 4, 5, 16, 17, 64)
LS_FAMILIES = ("random", "equal", "tied", "rising", "zero_direction", "non_finite")


def alphas_for(N):
    return np.array([1.0], F32) if N == 1 else np.concatenate([[0.0], np.geomspace(0.01, 2.0, N - 1)]).astype(F32)


def wolfe_flags(wolfe, N):
    """(strong, approx); approximate Wolfe explores candidate 1, which a single candidate does not have: weak there"""
    return wolfe == "strong", wolfe == "approx" and N > 1


def quadratic(curv, x_set, noise_cost, noise_grad):
    """cost [B, N] and gradient [B, N, V] of 0.5 sum curv x^2 at the candidates, plus noise (NaN candidates stay NaN)"""
    with np.errstate(invalid="ignore", over="ignore"):
        xs = x_set.astype(np.float64)
        cost = 0.5 * (curv[:, None, :] * xs * xs).sum(-1) + noise_cost
        grad = curv[:, None, :] * xs + noise_grad
    return cost.astype(F32), grad.astype(F32)


def poison(cost, grad, seed):
    """the non-finite family: NaN or +inf cost on one candidate of every second row (candidate 0 in every fourth), a NaN gradient
    element in every fifth row"""
    B, N, V = grad.shape
    rng = np.random.default_rng(seed)
    for r in range(B):
        t = r + seed
        if t % 2 == 0:
            k = 0 if t % 4 == 0 else int(rng.integers(N))
            cost[r, k] = np.nan if (t // 4) % 2 == 0 else np.inf
        if t % 5 == 0:
            grad[r, int(rng.integers(N)), int(rng.integers(V))] = np.nan


def line_search_case(B, V, N, family, seed):
    """the recipe of randomised/fuzz_opt.py at any (B, V, N), plus the non-finite family"""
    rng = np.random.default_rng([seed, B, V, N, LS_FAMILIES.index(family)])
    al = alphas_for(N)
    x = rng.normal(size=(B, 1, V)).astype(F32)
    d = rng.normal(size=(B, 1, V)).astype(F32)
    half = (np.arange(B) + seed) % 2 == 0
    if family == "zero_direction":
        d[half] = 0
    sa = (x + al[None, :, None] * d).astype(F32)
    curv = rng.uniform(0.1, 3.0, size=(B, V))
    scost, sg = quadratic(curv, sa, rng.normal(size=(B, N)), 0.3 * rng.normal(size=sa.shape))
    if family == "equal":
        scost[half] = scost[half][:, :1]
    if family == "tied" and N >= 3:
        scost[:, 2] = scost[:, 1]
    if family == "rising":
        scost = np.sort(scost, axis=1)
    if family == "non_finite":
        poison(scost, sg, seed)
    state = dict(best_cost=(1e3 * rng.uniform(0, 1, size=B)).astype(F32), best_action=rng.normal(size=(B, V)).astype(F32),
                 best_iteration=np.zeros(B, np.int16), current_iteration=rng.integers(0, 30, size=B).astype(np.int16))
    return dict(state=state, search_cost=scost, search_action=sa, search_gradient=sg, step_direction=d[:, 0].copy(), alphas=al)


def line_search_sweep(V):
    """every (N, wolfe, thresholds, family) of one V with a batch size that rotates through BATCHES"""
    i = 0
    for N in LS_N:
        for wolfe in WOLFE:
            for thr in THRESHOLDS:
                for family in LS_FAMILIES:
                    yield N, wolfe, thr, family, BATCHES[i % len(BATCHES)], i
                    i += 1


# ---------------------------------------------------------------------------------------------------------- L-BFGS step
STEP_V = (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
STEP_M = (0, 1, 2, 31)


def history(rng, curv, m, B, V):
    """m curvature pairs of the quadratic: s small and random, y = curv s, rho = 1 / (y.s)"""
    s = (0.1 * rng.normal(size=(m, B, V))).astype(F32)
    y = (curv[None] * s).astype(F32)
    with np.errstate(divide="ignore"):
        rho = (1.0 / (y.astype(np.float64) * s).sum(-1)).astype(F32)
    return y, s, rho.reshape(m, B)


def lbfgs_case(B, V, m, seed):
    """state and first (q, grad_q) of a descent on a diagonal quadratic; row 1 (where there is one) has negative curvature in
    the new pair: y = -curv s, so y.s < 0"""
    rng = np.random.default_rng([seed, B, V, m])
    curv = rng.uniform(0.1, 3.0, size=(B, V))
    y, s, rho = history(rng, curv, m, B, V)
    x0 = rng.normal(size=(B, V)).astype(F32)
    g0 = (curv * x0).astype(F32)
    q = (x0 + 0.1 * rng.normal(size=(B, V))).astype(F32)
    g = (curv * q + 1e-3 * rng.normal(size=(B, V))).astype(F32)
    if B > 1:
        g[1] = (g0[1] - curv[1] * (q[1].astype(np.float64) - x0[1])).astype(F32)
    return dict(curv=curv, y=y, s=s, rho=rho, x_0=x0, grad_0=g0, q=q, grad_q=g, rng=rng)


def lbfgs_next(case, q, step, x_0, grad_0, it):
    """the next (q, grad_q): a move of 0.1 (largest element, row by row) along the step; in the second step the last row repeats
    its previous iterate and gradient exactly (y = s = 0: y.s = 0 and y.y = 0 are exact zeros)"""
    rng, curv = case["rng"], case["curv"]
    st = np.nan_to_num(step.astype(np.float64))
    big = np.abs(st).max(-1, keepdims=True)
    qn = (q + 0.1 * st / np.where(big > 0, big, 1.0)).astype(F32)
    gn = (curv * qn + 1e-3 * rng.normal(size=qn.shape)).astype(F32)
    if it == 1 and q.shape[0] >= 3:
        qn[-1], gn[-1] = x_0[-1], grad_0[-1]
    return qn, gn


# ---------------------------------------------------------------------------------------------------------- one iteration
def action_dim_for(V):
    return next(d for d in (7, 5, 4, 1) if V % d == 0)


def tail_case(B, V, m, N, seed):
    """the optimiser-side state of B problems in the middle of a descent on a diagonal quadratic: a consistent history, the
    previous iterate, the candidates x + alpha_k d along a scaled descent direction"""
    rng = np.random.default_rng([seed, B, V, m, N])
    curv = rng.uniform(0.1, 3.0, size=(B, V))
    y, s, rho = history(rng, curv, m, B, V)
    x = rng.normal(size=(B, V)).astype(F32)
    x0 = (x + 0.05 * rng.normal(size=(B, V))).astype(F32)
    ad = action_dim_for(V)
    al = alphas_for(N)
    d = (-0.3 * curv * x + 0.05 * rng.normal(size=(B, V))).astype(F32)
    x_set = (x[:, None, :] + al[None, :, None] * d[:, None, :]).astype(F32)
    return dict(curv=curv, rng=rng, action_dim=ad, alphas=al, step_max=(rng.uniform(0.05, 0.55, size=ad)).astype(F32),
                y=y, s=s, rho=rho, x_0=x0, grad_0=(curv * x0).astype(F32), x_set=x_set, step_scaled=d,
                step_direction=np.zeros((B, V), F32),
                best_cost=(0.5 * (curv * x.astype(np.float64) ** 2).sum(-1) * rng.uniform(0.5, 1.5, size=B)).astype(F32),
                best_action=x.copy(), best_iteration=rng.integers(0, 3, size=B).astype(np.int16),
                current_iteration=rng.integers(3, 9, size=B).astype(np.int16))


def tail_rollout(case, x_set, it, non_finite):
    """what the rollout would hand the line search at the device's own candidates"""
    rng = case["rng"]
    B, N, V = x_set.shape
    cost, grad = quadratic(case["curv"], x_set, 0.01 * rng.normal(size=(B, N)), 0.01 * rng.normal(size=x_set.shape))
    if non_finite and it < 2:
        poison(cost, grad, it)
    return cost, grad
