"""The one-launch L-BFGS iteration tail against the three separate launches it replaces (line search, L-BFGS step, next
candidates), bit for bit, in every form the dispatch reaches: 16-lane rows, a wavefront per problem, a workgroup per
problem, the plain kernel, and each compile-time shape of csrc/tail_shapes.hpp with the switch on and off.

No rollout: search costs and gradients are random, the history, rho, x_0 and grad_0 start from random finite values, and
both paths run the same consecutive iterations on their own copy of the state.  Every state and output tensor is compared
as raw bits after every iteration (NaN-safe array_equal)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

_STATE = ("y", "s", "rho", "x_0", "grad_0", "step_direction", "x_set", "step_scaled", "exploration_cost", "exploration_action",
          "exploration_gradient", "exploration_idx", "selected_cost", "selected_action", "selected_gradient", "selected_idx",
          "best_cost", "best_action", "best_iteration", "current_iteration", "converged")


def _action_dim(V):
    return next(d for d in (7, 5, 4, 1) if V % d == 0)


class _Problem:
    """the optimiser-side state of B problems (LBFGSOpt._alloc), filled with random finite values"""

    def __init__(self, B, V, m, N, device, seed):
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g).to(device)  # noqa: E731
        self.dims = (B, V, m, N)
        self.y, self.s, self.rho = r(m, B, V), r(m, B, V), r(m, B)
        self.x_0, self.grad_0 = r(B, V), r(B, V)
        self.step_direction, self.step_scaled = r(B, V), r(B, V)
        self.x_set = r(B, N, V)
        self.exploration_cost, self.exploration_action, self.exploration_gradient = r(B), r(B, V), r(B, V)
        self.selected_cost, self.selected_action, self.selected_gradient = r(B), r(B, V), r(B, V)
        self.best_cost, self.best_action = r(B).abs() * 2.0, r(B, V)
        self.best_iteration = torch.randint(0, 3, (B,), generator=g).to(device, torch.int16)
        self.current_iteration = torch.randint(3, 9, (B,), generator=g).to(device, torch.int16)
        self.converged = torch.zeros(B, dtype=torch.uint8, device=device)
        self.exploration_idx = torch.full((B, N), -1, dtype=torch.int32, device=device)
        self.selected_idx = torch.full((B, N), -1, dtype=torch.int32, device=device)
        ad = _action_dim(V)
        self.action_dim = ad
        self.step_max = (torch.rand(ad, generator=g) * 0.5 + 0.05).to(device)  # small: the step scale is above 1 for most problems
        self.alphas = torch.tensor([0.0, 0.1, 0.5, 1.0, 2.0][:N] if N > 1 else [1.0], device=device)

    def copy(self):
        import copy

        c = copy.copy(self)
        for k in _STATE:
            setattr(c, k, getattr(self, k).clone())
        return c


_LS = dict(convergence_iteration=2, cost_delta_threshold=1e-4, cost_relative_threshold=1e-3, c_1=1e-3, c_2=0.9)


def _line_search_args(p, cost, grad, wolfe):
    B, V, m, N = p.dims
    return (p.best_cost, p.best_action, p.best_iteration, p.current_iteration, p.converged, _LS["convergence_iteration"],
            _LS["cost_delta_threshold"], _LS["cost_relative_threshold"], p.exploration_cost, p.exploration_action, p.exploration_gradient,
            p.exploration_idx.view(-1), p.selected_cost, p.selected_action, p.selected_gradient, p.selected_idx.view(-1), cost, p.x_set,
            grad, p.step_scaled, p.alphas, _LS["c_1"], _LS["c_2"], wolfe == "strong", wolfe == "approx", N, V, B)


def _one_launch(p, cost, grad, wolfe, stable, scale, overlapped):
    from curobo_amd.backends import optimization as O

    B, V, m, N = p.dims
    O.launch_lbfgs_iteration_tail(*_line_search_args(p, cost, grad, wolfe), p.step_direction, p.rho, p.y, p.s, p.x_0, p.grad_0, 0.01, m,
                                  stable, p.step_max, p.action_dim, scale, overlapped=overlapped)


def _three_launches(p, cost, grad, wolfe, stable, scale):
    from curobo_amd.backends import optimization as O

    B, V, m, N = p.dims
    O.launch_line_search(*_line_search_args(p, cost, grad, wolfe))
    O.launch_lbfgs_step(p.step_direction, p.rho, p.y, p.s, p.exploration_action, p.exploration_gradient, p.x_0, p.grad_0, 0.01, B, m, V,
                        stable, True)
    O.prepare_search_points(p.x_set, p.step_scaled, p.exploration_action, p.step_direction, p.step_max, p.alphas, B, N, V, p.action_dim,
                            scale)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _run(device, B, V, m, N, overlapped, wolfe="approx", stable=True, scale=True, zero_ys=False, seed=0, expect=None):
    """m + 2 consecutive iterations when m <= 2 (the history fills, then shifts), 3 otherwise; raw-bit equality after each"""
    if N == 1 and wolfe == "approx":
        wolfe = "weak"  # (approx_wolfe explores candidate 1 when candidate 0 is kept: it needs two candidates)
    if expect is not None:
        from curobo_amd.backends.optimization import tail_form

        assert tail_form(V, m, N, _action_dim(V), B, overlapped) == expect
    one = _Problem(B, V, m, N, device, seed)
    three = one.copy()
    g = torch.Generator().manual_seed(seed + 1)
    for it in range(m + 2 if m <= 2 else 3):
        cost = torch.rand(B, N, 1, generator=g).to(device)
        grad = torch.randn(B, N, V, generator=g).to(device)
        if zero_ys and it == 1:  # y = g - grad_0 = 0 whatever candidate is kept: y.s = 0 -> rho = 0, y.y = 0 -> 0 / 0 -> epsilon
            grad = one.grad_0.unsqueeze(1).expand(B, N, V).contiguous()
        _one_launch(one, cost, grad, wolfe, stable, scale, overlapped)
        _three_launches(three, cost, grad, wolfe, stable, scale)
        for k in _STATE:
            a, b = _bits(getattr(one, k)), _bits(getattr(three, k))
            assert torch.equal(a, b), f"{k} differs in iteration {it}: B={B} V={V} m={m} NLS={N} overlapped={overlapped} " \
                                      f"({int((a != b).sum())} of {a.numel()} elements)"
        if zero_ys and it == 1 and stable and m > 0:
            assert bool((one.rho[m - 1] == 0).all()), "the zero-curvature pair must have reached rho = 0"


@pytest.mark.parametrize("overlapped", [False, True])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 84, 128])
def test_wavefront_sized_problems_match_the_three_launches(V, overlapped, device):
    """the workgroup form (single stream) and the wavefront form (between seed shards); B = 3 and 5 are ragged in the
    four-problem workgroup of the wavefront form; V = 1 with m <= 16 lands in the row form"""
    from curobo_amd.backends.optimization import TAIL_ROW, TAIL_WAVE, TAIL_WORKGROUP

    for m in (0, 1, 2, 27, 31):
        for B in (1, 3, 5):
            for N in (1, 2, 4):
                form = TAIL_ROW if (V <= 16 and m <= 16) else (TAIL_WAVE if overlapped else TAIL_WORKGROUP)
                shape = 1 if (V, m, N) == (84, 27, 4) else 0
                _run(device, B, V, m, N, overlapped, seed=B + 10 * N, expect=(form, shape))


@pytest.mark.parametrize("V", [1, 7, 16])
def test_row_sized_problems_match_the_three_launches(V, device):
    from curobo_amd.backends.optimization import TAIL_ROW

    for m in (0, 1, 15, 16):
        for B in (1, 5, 17):
            for N in (1, 2, 4):
                _run(device, B, V, m, N, overlapped=bool(B & 1 and N == 2), seed=B + N, expect=(TAIL_ROW, 0))


@pytest.mark.parametrize("V,m", [(7, 7), (84, 27), (65, 2), (16, 16)])
def test_five_candidates_take_the_plain_kernel(V, m, device):
    from curobo_amd.backends.optimization import TAIL_PLAIN

    for B in (1, 5):
        _run(device, B, V, m, 5, overlapped=False, expect=(TAIL_PLAIN, 0))


@pytest.mark.parametrize("enabled", [True, False])
@pytest.mark.parametrize("name", ["trajopt_wave", "trajopt_workgroup", "ik_row"])
def test_builtin_shapes_match_with_the_switch_on_and_off(name, enabled, device):
    """each compile-time shape at a batch one short of and one past a workgroup boundary of its form (4 problems per
    workgroup in the wavefront form, 16 in the row form, 1 in the workgroup form), and through the run-time kernels"""
    from curobo_amd.backends.optimization import TAIL_ROW, TAIL_WAVE, TAIL_WORKGROUP, set_tail_shapes_enabled

    V, m, N, overlapped, form, shape, batches = {
        "trajopt_wave": (84, 27, 4, True, TAIL_WAVE, 1, (3, 4, 5, 63, 65)),
        "trajopt_workgroup": (84, 27, 4, False, TAIL_WORKGROUP, 1, (1, 2, 65)),
        "ik_row": (7, 7, 4, False, TAIL_ROW, 2, (15, 16, 17, 33)),
    }[name]
    set_tail_shapes_enabled(enabled)
    try:
        for B in batches:
            for wolfe in ("approx", "strong", "weak"):
                _run(device, B, V, m, N, overlapped, wolfe=wolfe, seed=B, expect=(form, shape if enabled else 0))
    finally:
        set_tail_shapes_enabled(True)


@pytest.mark.parametrize("scale", [True, False])
@pytest.mark.parametrize("V,m,B,overlapped", [(84, 27, 5, True), (84, 27, 3, False), (7, 7, 17, False), (65, 2, 3, True), (16, 15, 5, False)])
def test_zero_curvature_and_step_scale(V, m, B, overlapped, scale, device):
    """stable_mode with y.s = 0 in the second iteration: rho = 0 and the epsilon branch of the scaling are reached and the
    third iteration runs on that history; apply_step_scale on and off"""
    _run(device, B, V, m, 4, overlapped, stable=True, scale=scale, zero_ys=True, seed=3)
