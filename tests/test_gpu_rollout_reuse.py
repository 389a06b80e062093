"""Reuse of held evaluations in the fused trajectory launches (``memo``: csrc/fused_device.hpp ``fused_reuse_known_row``) and
in ``LBFGSOpt`` (``LBFGSOptCfg.reuse_exploration_point``).

Launch level: a row whose knots have the bits of its memo row must come back as the memo's (sentinel) cost and gradient --
copied, not computed -- and every other row bit for bit as a launch without memo computes it.  Optimiser level: the whole
state after 12 iterations is bit for bit the same with reuse on and off, eager, captured and sharded over streams."""

import dataclasses

import numpy as np
import pytest
import torch

from conftest import load_model, sample_q

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


@pytest.fixture(scope="module")
def franka_c2(device):
    from curobo_amd.robot.kinematics_params import KinematicsParams
    from curobo_amd.scene import SceneData, cuboid_scene_arrays
    from curobo_amd.workloads import c2_world, start_configuration

    model = load_model("franka")
    kin = KinematicsParams.from_model(model, device)
    scene = SceneData.from_arrays(cuboid_scene_arrays(c2_world()), device)
    return model, kin, scene, torch.as_tensor(start_configuration(model), device=device)


def _collision_rollout(franka_c2, B, **cfg_kw):
    from curobo_amd.rollout import CollisionRollout, CollisionRolloutCfg
    from curobo_amd.workloads import seed_knots

    model, kin, scene, start = franka_c2
    ro = CollisionRollout(kin, scene, B, CollisionRolloutCfg(**cfg_kw))  # Franka, C2 world, horizon 33
    ro.update_start_state(start)
    x = torch.as_tensor(seed_knots(model, B, ro.cfg.n_knots, seed=11), device=kin.device).reshape(B, -1).contiguous()
    return ro, x


def _flip_last_bit(t, row, col):
    t.view(torch.int32)[row, col] ^= 1


def _memo_of(x, stride, slot, differ=()):
    """(memo_x, memo_cost, memo_grad): the rows ``slot`` of every group of ``stride``, the groups in ``differ`` off by the last
    bit of one element; distinct sentinels per memo row"""
    mx = x[slot::stride].clone()
    for g in differ:
        _flip_last_bit(mx, g, (7 * g + 3) % mx.shape[1])
    n = mx.shape[0]
    mc = SENTINEL + torch.arange(n, device=x.device, dtype=torch.float32)
    mg = (2 * SENTINEL + torch.arange(n, device=x.device, dtype=torch.float32)).unsqueeze(1).expand(n, x.shape[1]).contiguous()
    return mx, mc, mg


def _launch(ro, x, memo=None, **kw):
    act = x.view(ro.batch_size, ro.cfg.n_knots, -1)
    c, g = ro.cost_and_gradient_fused(act, **kw) if memo is None else ro.cost_and_gradient_fused(act, memo=memo, **kw)
    torch.cuda.synchronize()
    return c.clone(), g.reshape(ro.batch_size, -1).clone()


def _check(c0, g0, c1, g1, memo, stride, slot, copied_groups):
    """rows ``stride * g + slot`` of ``copied_groups`` hold the sentinels; every other row equals the launch without memo"""
    _, mc, mg = memo
    B = c0.shape[0]
    copied = {stride * g + slot for g in copied_groups}
    for b in range(B):
        if b in copied:
            assert float(c1[b]) == float(mc[b // stride]), f"row {b}: cost was computed, not copied"
            assert torch.equal(g1[b], mg[b // stride]), f"row {b}: gradient was computed, not copied"
        else:
            assert torch.equal(c1[b], c0[b]) and torch.equal(g1[b], g0[b]), f"row {b} differs from the launch without memo"
    assert torch.isfinite(c0).all() and float(c0.max()) > 0.0  # (the comparison is of real collision costs)


@pytest.mark.parametrize("shapes", [True, False])
@pytest.mark.parametrize("B,stride,slot,differ", [
    (8, 4, 0, (1,)),   # the base case: group 0 copied, group 1 one bit off -> evaluated
    (8, 4, 2, (0,)),   # another slot of the group
    (3, 1, 0, (1,)),   # stride 1: every row has a memo row
    (6, 3, 0, (1,)),   # a stride that is no power of two
    (6, 3, 2, ()),     # ... its last slot, every group copied
])
def test_rows_with_equal_bits_are_copied_all_others_evaluated(franka_c2, shapes, B, stride, slot, differ):
    from curobo_amd.backends.rollout import set_fused_shapes_enabled

    ro, x = _collision_rollout(franka_c2, B)
    set_fused_shapes_enabled(shapes)
    try:
        c0, g0 = _launch(ro, x)
        memo = _memo_of(x, stride, slot, differ)
        c1, g1 = _launch(ro, x, memo=(*memo, stride, slot))
        c2, g2 = _launch(ro, x)  # and a launch without memo afterwards is a full evaluation again
    finally:
        set_fused_shapes_enabled(True)
    _check(c0, g0, c1, g1, memo, stride, slot, [g for g in range(B // stride) if g not in differ])
    assert torch.equal(c2, c0) and torch.equal(g2, g0)


def test_negative_zero_is_not_positive_zero(franka_c2):
    ro, x = _collision_rollout(franka_c2, 8)
    x[0, 5] = -0.0
    c0, g0 = _launch(ro, x)
    memo = _memo_of(x, 4, 0)
    memo[0][0, 5] = 0.0
    assert float(memo[0][0, 5]) == float(x[0, 5]) and not torch.equal(memo[0].view(torch.int32)[0], x.view(torch.int32)[0])
    c1, g1 = _launch(ro, x, memo=(*memo, 4))
    _check(c0, g0, c1, g1, memo, 4, 0, [1])  # group 0 evaluated (equal as floats, different bits), group 1 copied


def test_equal_nan_bits_are_copied(franka_c2):
    """(the reference launch runs on finite knots: row 0 is changed afterwards, and only row 0 depends on it)"""
    ro, x = _collision_rollout(franka_c2, 8)
    c0, g0 = _launch(ro, x)
    x[0, 5] = float("nan")
    memo = _memo_of(x, 4, 0)
    assert torch.equal(memo[0].view(torch.int32)[0], x.view(torch.int32)[0]) and not bool((memo[0][0] == x[0]).all())
    c1, g1 = _launch(ro, x, memo=(*memo, 4))
    _check(c0, g0, c1, g1, memo, 4, 0, [0, 1])


def test_reuse_follows_the_trajectory_not_the_workgroup(franka_c2):
    """Longest-first dispatch on: the copied rows take no time, so the orders built from these launches put them last and a
    later launch runs trajectory b in a workgroup with another blockIdx.  Results stay keyed by b, the copied workgroups
    still report their durations, and both order tables stay permutations of 0..B-1."""
    B = 8
    ro, x = _collision_rollout(franka_c2, B, longest_first_dispatch=True)
    c0, g0 = _launch(ro, x)
    memo = _memo_of(x, 4, 0, differ=(1,))
    used_orders = []
    for it in range(4):
        ws = ro._dispatch.ws.view(4, B).cpu().numpy().copy()
        used_orders.append(ws[ro._dispatch._phase ^ 1])  # the order the next launch reads (DispatchOrder.next flips the phase)
        c1, g1 = _launch(ro, x, memo=(*memo, 4))
        _check(c0, g0, c1, g1, memo, 4, 0, [0])
        ws = ro._dispatch.ws.view(4, B).cpu().numpy()
        for p in (0, 1):
            assert np.array_equal(np.sort(ws[p]), np.arange(B)), f"order[{p}] is not a permutation after launch {it}"
    assert any(not np.array_equal(o, np.arange(B)) for o in used_orders[2:]), "no launch ran with b != blockIdx"
    assert used_orders[-1][-1] == 0, "the copied row (the shortest workgroup by far) is not dispatched last"
    assert (ws[2:4] >= 0).all()


def test_copied_rows_stamp_the_profile_buffer(franka_c2):
    """the development hook that stamps phase boundaries per trajectory (bench.py --full reads launch start = min of stamp 0,
    end = max of stamp 4): a copied row stamps its start and its end like every other row, and the results do not change"""
    from curobo_amd._lib import check, load

    B = 8
    ro, x = _collision_rollout(franka_c2, B)
    c0, g0 = _launch(ro, x)
    memo = _memo_of(x, 4, 0, differ=(1,))
    stamps = torch.zeros(B, 16, dtype=torch.int64, device=x.device)
    check(load().curobo_hip_rollout_fused_set_profile_buffer(stamps.data_ptr()))
    try:
        c1, g1 = _launch(ro, x, memo=(*memo, 4))
    finally:
        check(load().curobo_hip_rollout_fused_set_profile_buffer(None))
    _check(c0, g0, c1, g1, memo, 4, 0, [0])
    t = stamps.cpu().numpy()
    assert (t[:, 0] > 0).all() and (t[:, 4] >= t[:, 0]).all()
    assert (t[0, 1:] == t[0, 4]).all()  # the copied row: one end time on every later boundary
    span = t[:, 4].max() - t[:, 0].min()
    assert 0 < span < 100 * 1000  # 100 MHz ticks: the launch took less than a millisecond


def test_memo_is_refused_where_a_copied_row_cannot_stand_in(franka_c2):
    ro, x = _collision_rollout(franka_c2, 8, fused_materialize=True)
    memo = _memo_of(x, 4, 0)
    assert not ro.offers_reuse(4)
    with pytest.raises(ValueError, match="offers no reuse"):
        ro.cost_and_gradient_fused(x.view(8, ro.cfg.n_knots, -1), memo=(*memo, 4))
    ro, x = _collision_rollout(franka_c2, 8)
    assert ro.offers_reuse(4) and ro.offers_reuse(1) and not ro.offers_reuse(3)
    ro.start_idx[1] = 0  # written, still equal within the groups
    assert ro.offers_reuse(4)
    ro.env_query_idx[5] = 1  # rows of one group that read different per-trajectory state: no reuse
    assert not ro.offers_reuse(4) and ro.offers_reuse(1)


def _trajopt_rollout(franka_c2, B, oracle):
    from curobo_amd.rollout import TrajOptRollout, TrajOptRolloutCfg
    from curobo_amd.workloads import seed_knots

    model, kin, scene, start = franka_c2
    goals = oracle.kinematics_forward(sample_q(model, 2, seed=6, scale=0.7), model.as_dict())
    ro = TrajOptRollout(kin, scene, B, TrajOptRolloutCfg())
    ro.update_start_state(start)
    idx = torch.arange(B, device=kin.device, dtype=torch.int32) // 4  # one goal per group of four
    ro.update_goals(torch.as_tensor(goals["link_pos"].reshape(2, 1, 1, 3)), torch.as_tensor(goals["link_quat"].reshape(2, 1, 1, 4)), idx)
    x = torch.as_tensor(seed_knots(model, B, ro.cfg.n_knots, seed=4, spread=0.6), device=kin.device).reshape(B, -1).contiguous()
    return ro, x


@pytest.mark.parametrize("shapes", [True, False])
def test_terms_launch_reuses_rows(franka_c2, oracle, shapes):
    """the TERMS instantiation (tool pose + c-space STATE) through TrajOptRollout, batch 8, one goal per group"""
    from curobo_amd.backends.rollout import set_fused_shapes_enabled

    ro, x = _trajopt_rollout(franka_c2, 8, oracle)
    assert ro.fused_available() and ro.offers_reuse(4)
    set_fused_shapes_enabled(shapes)
    try:
        c0, g0 = _launch(ro, x)
        memo = _memo_of(x, 4, 0, differ=(1,))
        c1, g1 = _launch(ro, x, memo=(*memo, 4))
        with pytest.raises(ValueError, match="materialised outputs"):  # per-term outputs: refused by the entry point
            ro.cost_and_gradient_fused(x.view(8, ro.cfg.n_knots, -1), with_metrics=True, memo=(*memo, 4))
    finally:
        set_fused_shapes_enabled(True)
    _check(c0, g0, c1, g1, memo, 4, 0, [0])
    ro.idxs_goal[1] = 1  # a group whose rows aim at different goals
    assert not ro.offers_reuse(4)


# ------------------------------------------------------------------------------------------------ optimiser level
STATE = ["best_cost", "best_action", "x_set", "search_cost", "search_gradient", "y", "s", "rho", "exploration_action",
         "exploration_cost", "exploration_gradient"]


def _optimise(franka_c2, mode, reuse, scale):
    """4 problems x 4 candidates, 12 iterations; returns the optimiser state and how many launches carried a memo"""
    from curobo_amd.backends import rollout as rollout_hip
    from curobo_amd.optim import LBFGSOpt, LBFGSOptCfg, PipelinedLBFGS
    from curobo_amd.rollout import CollisionRollout, CollisionRolloutCfg
    from curobo_amd.workloads import seed_knots

    model, kin, scene, start = franka_c2
    device = kin.device
    cfg = CollisionRolloutCfg()
    ocfg = LBFGSOptCfg(num_problems=4, inner_iters=4, num_iters=12, line_search_scale=list(scale), reuse_exploration_point=reuse)
    bounds = (kin.joint_limits_position[0], kin.joint_limits_position[1])

    def make(batch):
        ro = CollisionRollout(kin, scene, batch, cfg)
        ro.update_start_state(start)
        return ro.cost_and_gradient

    import inspect

    with_memo = []
    real = rollout_hip._rollout_trajectory
    signature = inspect.signature(real)

    def counting(*a, **kw):
        with_memo.append(signature.bind(*a, **kw).arguments.get("memo") is not None)
        return real(*a, **kw)

    rollout_hip._rollout_trajectory = counting
    try:
        seed = torch.as_tensor(seed_knots(model, 4, cfg.n_knots, seed=2), device=device)
        if mode == "pipelined":
            opt = PipelinedLBFGS(ocfg, make, cfg.n_knots, kin.num_dof, bounds, device, n_shards=2)
            opts = opt.opts
        else:
            opt = LBFGSOpt(ocfg, make(16), cfg.n_knots, kin.num_dof, bounds, device, use_cuda_graph=(mode == "captured"))
            opts = [opt]
        opt.optimize(seed)
        torch.cuda.synchronize()
    finally:
        rollout_hip._rollout_trajectory = real
    return {k: torch.cat([getattr(o, k).clone() for o in opts], dim=(1 if k in ("y", "s", "rho") else 0)) for k in STATE}, sum(with_memo)


@pytest.mark.parametrize("scale", [(0.0, 0.1, 0.5, 1.0), (0.01, 0.1, 0.5, 1.0)])
@pytest.mark.parametrize("mode", ["eager", "captured", "pipelined"])
def test_optimiser_state_is_bit_identical_with_reuse(franka_c2, mode, scale):
    on, n_on = _optimise(franka_c2, mode, True, scale)
    off, n_off = _optimise(franka_c2, mode, False, scale)
    assert n_off == 0
    # a zero first step: the iterations hand the exploration buffers over; any other scale list: nothing is offered
    assert (n_on > 0) == (scale[0] == 0.0), n_on
    for k in STATE:
        assert torch.equal(on[k], off[k]), f"{k} differs with reuse on ({mode}, scale {scale})"
    assert torch.isfinite(on["best_cost"]).all()
