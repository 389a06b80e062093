"""The one-launch seed-IK iteration (``curobo_hip_seed_ik_iterate``, csrc/seed_ik.hip: LM step, FK, tool Jacobian, tool-pose
error, J^T e and state update on a 16-lane row with the state in LDS) against the CPU restatement of the reference's iteration
(oracle/seed_ik_ref.py), PER SEED, in every instantiation and with every option the launch takes.

Cases (tests/seed_ik_variants.py; n = 13 problems x 7 seeds = 91 rows: the last workgroup and the last wavefront are partial):

    case  model                                    D, T   instantiation
    A     franka                                   7, 1   <7,1>   registers
    B     ur10e                                    6, 1   <6,1>   registers
    C     franka + panda_link6                     7, 2   <0,0>   run-time sizes, row-distributed Cholesky, broadcast solves
    D     ur10e + wrist_1_link, wrist_3_link       6, 3   <0,0>
    E     franka, panda_joint5 / _joint7 locked    5, 1   <0,0>   D < 6
    F     the joint zoo (tests/joint_zoo.py)       6, 4   <0,0>   prismatic joints behind revolute ones, multipliers outside
                                                                  {+-1}, biases, two dofs with two links (atomicAdd columns)

Bounds.  k = 0 (the initial evaluation): those the launch sequence meets in tests/test_gpu_seed_ik.py.  k >= 1: the accept
decision is a threshold, so rows whose trust ratio comes within 1e-3 (1 + |rho|) of ``rho_min`` in the oracle's run are left out
(at most 2 % of the rows, asserted; with these inputs: none); on every other row the decisions and the success flag are exact,
``lambda_damping`` (which only moves by factors of 2) rtol 1e-6, ``joint_position`` / position / orientation error 2e-4.
``jacobian`` and ``jTerror`` are allowed 8 times the arithmetic's own sensitivity: the largest difference, in units of max |value|,
between the fp32 oracle and the same iteration with the LM solve in float64, measured on the CPU
(``seed_ik_variants.MEASURED``, checked there by tests/test_oracle_seed_ik.py):

    case   jacobian  k = 1     2        4        jTerror  k = 1     2        4
    A                9.6e-7   1.4e-6   3.1e-6             8.1e-7   1.2e-6   2.2e-6
    B                8.8e-7   4.3e-6   7.6e-6             1.2e-6   1.7e-6   3.0e-6
    C                1.6e-6   3.6e-6   2.2e-5             7.4e-7   3.6e-6   4.8e-6
    D                2.1e-6   5.8e-6   7.8e-6             1.7e-6   2.5e-6   4.6e-6
    E                7.1e-7   3.1e-6   3.4e-6             6.1e-7   1.5e-6   1.4e-6
    F                2.3e-6   2.9e-6   1.7e-6             2.2e-6   3.5e-6   2.0e-6

(joint positions of those two CPU runs differ by at most 6.0e-6, 1.1e-5 and 2.3e-5 after 1, 2 and 4 iterations; their decisions
and dampings are identical.)

Out of scope: D in 8..16 -- no robot here that fits the launch's LDS has them.
"""

import functools

import numpy as np
import pytest
import torch

import seed_ik_variants as V

pytestmark = pytest.mark.gpu

STATE = ("q", "jacobian", "jTerror", "error_norm", "position_error", "orientation_error", "lambda_damping", "success", "improvement")


@functools.lru_cache(maxsize=None)
def _kin(case, device):
    from curobo_amd.robot.kinematics_params import KinematicsParams

    kin = KinematicsParams.from_model(V.case_model(case), device)
    kin.validate_shapes()
    return kin


def _solver(device, case, x, num_problems=V.P, num_seeds=V.S, velocity_weight=0.0, acceleration_weight=0.0):
    """a solver of the case with the problem ``x`` (``seed_ik_variants.inputs``) in its buffers and fresh state"""
    from curobo_amd.solver.seed_ik import SeedIKSolver, SeedIKSolverCfg

    cfg = SeedIKSolverCfg(num_seeds=num_seeds, use_cuda_graph=False, velocity_weight=velocity_weight,
                          acceleration_weight=acceleration_weight)
    s = SeedIKSolver(_kin(case, device), num_problems, cfg, num_goalset=x["G"])
    assert s._fused_ok()  # the launch is what runs, not the sequence
    t = lambda a: torch.as_tensor(np.array(a), device=device)  # noqa: E731  (a copy: the shared inputs are read-only)
    s.goal_position.copy_(t(x["goal_position"]))
    s.goal_quat.copy_(t(x["goal_quat"]))
    if "permuted" not in x:
        assert np.array_equal(s.idxs_goal.cpu().numpy(), x["idxs_goal"])  # as the solver builds it
    s.idxs_goal.copy_(t(x["idxs_goal"]))
    e = x["extra"]
    s._vel_active = "current_position" in e
    if s._vel_active:
        s._vel_current.copy_(t(e["current_position"]))
        s._vel_dt.copy_(t(e["dt"]))
        if "current_velocity" in e:
            s._vel_velocity.copy_(t(e["current_velocity"]))
    s.lambda_damping.fill_(cfg.lambda_initial)
    return s


def _state(s):
    torch.cuda.synchronize()
    return {k: getattr(s, k).cpu().numpy().copy() for k in STATE}


def _launch(device, case, x, k, **kw):
    """initial evaluation + k iterations in ONE launch, from fresh state buffers"""
    s = _solver(device, case, x, **kw)
    s._iterate_fused(k, torch.as_tensor(np.array(x["seeds"]), device=device))
    return _state(s)


def _compare(got, ref, x, case, k, keep=None):
    """the state of the launch against the oracle's (module docstring); ``keep``: rows that an option leaves in"""
    n = ref["joint_position"].shape[0]
    keep = np.ones(n, bool) if keep is None else keep
    if k == 0:
        np.testing.assert_allclose(got["jacobian"][keep], ref["jacobian"][keep], rtol=1e-4, atol=2e-6)
        np.testing.assert_allclose(got["jTerror"][keep], ref["jTerror"][keep], rtol=1e-4, atol=2e-5)
        np.testing.assert_allclose(got["error_norm"][keep], ref["error_norm"][keep], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(got["position_error"][keep], ref["position_errors"][keep], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(got["orientation_error"][keep], ref["orientation_errors"][keep], rtol=1e-4, atol=1e-5)
        np.testing.assert_array_equal(got["q"], x["seeds"])
        np.testing.assert_array_equal(got["lambda_damping"], np.full(n, np.float32(0.2)))
    else:
        knife = V.knife_edge(ref)
        assert knife.mean() <= V.KNIFE_CAP, knife.mean()
        keep = keep & ~knife
        np.testing.assert_allclose(got["lambda_damping"][keep], ref["lambda_damping"][keep], rtol=1e-6)
        np.testing.assert_allclose(got["q"][keep], ref["joint_position"][keep], rtol=0, atol=2e-4)
        np.testing.assert_allclose(got["position_error"][keep], ref["position_errors"][keep], rtol=0, atol=2e-4)
        np.testing.assert_allclose(got["orientation_error"][keep], ref["orientation_errors"][keep], rtol=0, atol=2e-4)
        mJ, mg = V.MEASURED[case][k]
        for key, name, m in (("jacobian", "jacobian", mJ), ("jTerror", "jTerror", mg)):
            want = ref[key][keep]
            diff = np.abs(got[name][keep] - want).max() / np.abs(want).max()
            print(f"case {case} k {k} {key}: {diff:.3e} of max |value| (allowed {V.SENSITIVITY_FACTOR * m:.3e})")
            assert diff <= V.SENSITIVITY_FACTOR * m, (key, diff, V.SENSITIVITY_FACTOR * m)
    np.testing.assert_array_equal(got["improvement"][keep].astype(bool), ref["improvement"][keep])
    np.testing.assert_array_equal(got["success"][keep].astype(bool), ref["success"][keep])


# ------------------------------------------------------------------------------------------------ per seed, every instantiation
@pytest.mark.parametrize("k", [0, 1, 2, 4])
@pytest.mark.parametrize("case", list(V.CASES))
def test_fused_iterations_match_oracle_per_seed(oracle, device, case, k):
    x = V.inputs(case)
    ref = V.reference(case, k)
    if k > 0:  # both branches of the accept decision and live joint-limit rows (a condition on the inputs)
        acc = V.reference(case, 4)["accepted"]
        assert acc.any() and (~acc).any()
        assert (ref["jacobian"][:, 6 * x["md"]["tool_frame_map"].shape[0]:] != 0).any(axis=(1, 2)).mean() > 0.1
    _compare(_launch(device, case, x, k), ref, x, case, k)


@pytest.mark.parametrize("k", [0, 1, 2, 4])
def test_five_launch_sequence_matches_oracle_on_the_joint_zoo(oracle, device, k):
    """case F through the five-launch iteration (LM step, FK with Jacobian from kinematics.hip, tool-pose distance, FK VJP,
    state update): the same oracle run, the same bounds as the one-launch iteration"""
    x = V.inputs("F")
    s = _solver(device, "F", x)
    s._evaluate_candidate(torch.as_tensor(np.array(x["seeds"]), device=device), initial=True)
    for _ in range(k):
        s._lm_iteration()
    _compare(_state(s), V.reference("F", k), x, "F", k)


@pytest.mark.parametrize("case", list(V.CASES))
def test_success_flag_and_strict_bounds(oracle, device, case):
    """nothing converges to 1e-5 in four iterations from random seeds, so: one evaluation whose seeds ARE the goal
    configurations (clipped 1e-3 inside the action bounds, one problem per row).  Every row succeeds, except the one with a
    joint exactly on ``action_max``: the comparison with the bounds is strict."""
    from oracle import seed_ik_ref as R

    model = V.case_model(case)
    md, cfg, n = model.as_dict(), R.SeedIKRefCfg(), V.P * V.S
    lo, hi = R.action_bounds(md, cfg)
    rng = np.random.default_rng(2)
    q = np.clip((lo + (hi - lo) * rng.random((n, lo.shape[0]))).astype(np.float32), lo + np.float32(1e-3), hi - np.float32(1e-3))
    row, joint = 37, lo.shape[0] - 2
    q[row, joint] = hi[joint]
    fk = oracle.kinematics_forward(q, md, compute_spheres=False)
    T = md["tool_frame_map"].shape[0]
    x = dict(goal_position=fk["link_pos"].reshape(n, T, 1, 3), goal_quat=fk["link_quat"].reshape(n, T, 1, 4), seeds=q,
             idxs_goal=np.arange(n, dtype=np.int32), extra={}, G=1, md=md)
    ref = R.iterate(oracle, md, cfg, q, x["goal_position"], x["goal_quat"], x["idxs_goal"], 0)
    # (the oracle on its own FK: position error 0, orientation error 6.0e-8 to 6.7e-8 here -- the rounding of a unit
    # quaternion's product, at most one fp32 ulp of 1 -- against a convergence tolerance of 1e-5)
    assert ref["position_errors"].max() == 0 and ref["orientation_errors"].max() <= 2.0 ** -23
    want = np.arange(n) != row
    assert np.array_equal(ref["success"], want)
    s = _solver(device, case, x, num_problems=n, num_seeds=1)
    np.testing.assert_array_equal(s.action_max.cpu().numpy(), hi)  # the same bounds, to the bit
    np.testing.assert_array_equal(s.action_min.cpu().numpy(), lo)
    s._iterate_fused(0, torch.as_tensor(q, device=device))
    got = _state(s)
    np.testing.assert_array_equal(got["success"].astype(bool), want)
    _compare(got, ref, x, case, 0)


# ------------------------------------------------------------------------------------------------ options inside the launch
@pytest.mark.parametrize("k", [0, 2])
@pytest.mark.parametrize("option", ["goalset", "goalset_permuted"])
@pytest.mark.parametrize("case", ["A", "C"])
def test_fused_goal_sets(oracle, device, case, option, k):
    """three goal poses per frame; ``goalset_permuted``: a row's goal is not ``row // S``.  The member a frame is pulled to is
    the oracle's ``goalset_idx``; seeds whose two best members tie to 1e-4 (relative) in any evaluation are left out"""
    x = dict(V.inputs(case, option))
    if option == "goalset_permuted":
        x["permuted"] = True
        assert (x["idxs_goal"] != np.arange(V.P * V.S) // V.S).mean() > 0.5
    ref = V.reference(case, k, option)
    keep = ref["goalset_margin"] > V.GOALSET_MARGIN
    assert keep.mean() >= V.GOALSET_KEEP, keep.mean()
    assert len(np.unique(ref["goalset_idx"])) == 3  # every member is somebody's
    _compare(_launch(device, case, x, k), ref, x, case, k, keep)


@pytest.mark.parametrize("k", [0, 2])
@pytest.mark.parametrize("case", ["A", "D"])
def test_fused_velocity_clamped_bounds(oracle, device, case, k):
    """``current_position`` + ``dt`` = 0.2: joint-limit rows against the bounds one step can reach"""
    x = V.inputs(case, "clamped")
    ref = V.reference(case, k, "clamped")
    assert np.abs(V.reference(case, 0, "clamped")["error_norm"] - V.reference(case, 0)["error_norm"]).max() > 0.1
    _compare(_launch(device, case, x, k), ref, x, case, k)


@pytest.mark.parametrize("k", [0, 2])
@pytest.mark.parametrize("wv,wa", [(0.5, 0.0), (0.0, 0.005), (0.5, 0.005)])
@pytest.mark.parametrize("case", ["A", "E"])
def test_fused_velocity_and_acceleration_rows(oracle, device, case, wv, wa, k):
    """the velocity / acceleration residual rows, folded into the joint-limit rows (dt = 0.2)"""
    x = V.inputs(case, "velacc")
    ref = V.reference(case, k, "velacc", wv, wa)
    assert np.abs(V.reference(case, 0, "velacc", wv, wa)["jTerror"] - V.reference(case, 0, "clamped")["jTerror"]).max() > 0.1
    _compare(_launch(device, case, x, k, velocity_weight=wv, acceleration_weight=wa), ref, x, case, k)


# ------------------------------------------------------------------------------------------------ state between launches
@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_state_handed_through_global_memory_is_bit_equal(oracle, device, case):
    """initial + 4 iterations in one launch == initial, then four launches of one iteration == (initial + 2), then 2: the
    same instantiation runs the same arithmetic, the state only travels through global memory in between"""
    x = V.inputs(case)
    seeds = torch.as_tensor(np.array(x["seeds"]), device=device)
    one = _launch(device, case, x, 4)
    for first, rest in ((0, (1, 1, 1, 1)), (2, (2,))):
        s = _solver(device, case, x)
        s._iterate_fused(first, seeds)
        for k in rest:
            s._iterate_fused(k)
        got = _state(s)
        for key in STATE:
            assert np.array_equal(got[key].view(np.uint8), one[key].view(np.uint8)), (first, rest, key)
    assert one["improvement"].any() and not one["improvement"].all()


@pytest.mark.parametrize("num_problems,num_seeds", [(V.P, V.S), (3, 1)])
def test_stop_flag_and_blocks_run(oracle, device, num_problems, num_seeds):
    """flag set: a non-initial launch changes no byte of the state and does not count itself; flag clear: ``blocks_run``
    grows by exactly 1 per launch whatever the grid (6 workgroups at n = 91, 1 at n = 3)"""
    md, gp, gq, seeds, idx = V.problem(oracle, V.case_model("A"), num_problems, num_seeds)
    x = dict(goal_position=gp, goal_quat=gq, seeds=seeds, idxs_goal=idx, extra={}, G=1, md=md)
    s = _solver(device, "A", x, num_problems=num_problems, num_seeds=num_seeds)
    s._iterate_fused(1, torch.as_tensor(seeds, device=device))
    before = _state(s)
    s._blocks_run.fill_(5)
    s._stop_flag.fill_(1)
    s._iterate_fused(2)
    after = _state(s)
    for key in STATE:
        assert np.array_equal(before[key].view(np.uint8), after[key].view(np.uint8)), key
    assert int(s._blocks_run.item()) == 5
    s._stop_flag.zero_()
    for i in range(3):
        s._iterate_fused(1)
        assert int(s._blocks_run.item()) == 6 + i
    moved = _state(s)
    assert not np.array_equal(moved["q"], before["q"])  # ... and these launches did run
