"""The IK rollout with a current state (velocity-tightened joint limits + implied velocity / acceleration regularisation,
``curobo_hip_rollout_ik_fused_state`` and the kernel sequence) vs the oracle composition and vs each other, and the IK solver
with ``optimization_dt``: solutions one time step from the current state, on reachable and on unreachable goals, under graphs."""

import functools

import numpy as np
import pytest
import torch

from conftest import load_model, sample_q

pytestmark = pytest.mark.gpu

B, N_STATES = 53, 3  # three full 16-row workgroups and one of five rows
STATE_DT = np.array([0.1, 0.0, 0.05], np.float32)  # (state 1: dt = 0 must reproduce the plain term)


G1_SPARSE = "unitree_g1, every 8th sphere"


def _model(robot):
    """the packaged robots; 16 configurations of the G1 (674 spheres, 162 111 collision pairs) never fit the launch's LDS, so its
    49 joints go through the launch on a G1 with every 8th sphere (85 spheres, the pairs among them): 152 KB of the 160 KB"""
    import dataclasses

    if robot != G1_SPARSE:
        return load_model(robot)
    m = load_model("unitree_g1")
    keep = np.arange(0, m.num_spheres, 8)
    new = np.full(m.num_spheres, -1)
    new[keep] = np.arange(len(keep))
    pairs = new[m.collision_pairs.astype(np.int64)]
    return dataclasses.replace(m, link_spheres=np.ascontiguousarray(m.link_spheres[:, keep]),
                               link_sphere_idx_map=np.ascontiguousarray(m.link_sphere_idx_map[keep]),
                               sphere_padding=np.ascontiguousarray(m.sphere_padding[keep]),
                               collision_pairs=np.ascontiguousarray(pairs[(pairs >= 0).all(-1)].astype(np.int16)))


@functools.lru_cache(maxsize=None)
def _case(robot):
    """inputs of one robot and every oracle term that does not depend on the regularisation weights, computed once"""
    from oracle import load_oracle

    from curobo_amd.robot.kinematics_params import KinematicsParams
    from curobo_amd.rollout.ik_rollout import IKRolloutCfg
    from curobo_amd.scene import SceneData, cuboid_scene_arrays
    from curobo_amd.workloads import c1_world

    oracle, device = load_oracle(), torch.device("cuda:0")
    model = _model(robot)
    md = model.as_dict()
    kin = KinematicsParams.from_model(model, device)
    arrays = cuboid_scene_arrays(c1_world())
    scene = SceneData.from_arrays(arrays, device)
    D, T = model.num_dof, kin.num_pose_links
    rng = np.random.default_rng(17)
    q = sample_q(model, B, seed=5, scale=1.05)  # some joints violate the static limits
    cur = sample_q(model, N_STATES, seed=2)  # inside the limits
    curv = rng.normal(size=(N_STATES, D)).astype(np.float32)
    idxs_cur = rng.integers(0, N_STATES, size=B).astype(np.int32)  # rows of one workgroup read different states
    lo, hi = model.joint_limits_position.astype(np.float32)
    # velocity limits scaled per joint so that one step covers a good part of the joint's range: 0.35 (0.28 downwards) of it at
    # dt = 0.1, half that at dt = 0.05 -- q and the current position are uniform in the range, so the tightened bound decides
    # for roughly half of the (row, joint) pairs (the shares are asserted on the oracle's output below)
    v_hi = 0.35 * (hi - lo) / 0.1
    v_b = np.stack([-0.8 * v_hi, v_hi]).astype(np.float32)
    goals = oracle.kinematics_forward(sample_q(model, 4, seed=6, scale=0.7), md)
    gpos, gquat = goals["link_pos"].reshape(4, T, 1, 3), goals["link_quat"].reshape(4, T, 1, 4)
    idx = (np.arange(B) % 4).astype(np.int32)
    c = IKRolloutCfg()
    fk = oracle.kinematics_forward(q, md)
    pose = oracle.tool_pose_distance(fk["link_pos"].reshape(B, 1, T, 3), fk["link_quat"].reshape(B, 1, T, 4), gpos, gquat, idx,
                                     np.array(c.pose_weight, np.float32), np.ones((T, 6), np.float32), np.ones((T, 6), np.float32),
                                     np.full((T, 2), 1e-8, np.float32), np.full((T, 2), 1e-8, np.float32), np.zeros(T, np.uint8), 0)
    sph = fk["robot_spheres"].reshape(B, 1, -1, 4)
    sc = oracle.self_collision(sph, model.sphere_padding, model.collision_pairs, c.self_collision_weight)
    wc = oracle.scene_collision(sph, arrays, c.scene_collision_weight, c.scene_activation_distance)
    gs = sc["gradient"].reshape(B, -1, 4) + wc["gradient"].reshape(B, -1, 4) * np.array([1, 1, 1, 0], np.float32)
    grad_rest = oracle.kinematics_backward(md, fk["cumul_mat"], gs, pose["position_gradient"].reshape(B, T, 3),
                                           pose["rotation_gradient"].reshape(B, T, 4))
    cost_rest = pose["distance"].sum((1, 2)) + sc["distance"] + wc["distance"].sum((1, 2))
    return dict(oracle=oracle, model=model, kin=kin, scene=scene, q=q, cur=cur, curv=curv, idxs_cur=idxs_cur, v_b=v_b, gpos=gpos,
                gquat=gquat, idx=idx, cost_rest=cost_rest, grad_rest=grad_rest, p_b=np.stack([lo, hi]))


def _oracle_cspace(case, reg, with_state=True):
    from curobo_amd.rollout.ik_rollout import IKRolloutCfg

    c, D = IKRolloutCfg(), case["model"].num_dof
    kw = dict(current_position=case["cur"], current_velocity=case["curv"], idxs_current_state=case["idxs_cur"], v_b=case["v_b"],
              state_dt=STATE_DT, squared_l2_reg_weight=reg) if with_state else {}
    return case["oracle"].cspace_position_cost(case["q"].reshape(B, 1, D), case["p_b"], np.array(c.cspace_weight, np.float32),
                                               np.array(c.cspace_activation_distance, np.float32), **kw)


def _rollout(case, fused, reg, device, use_current_state=True):
    from curobo_amd.rollout.ik_rollout import IKRollout, IKRolloutCfg

    t = lambda a: torch.as_tensor(a, device=device)  # noqa: E731
    ro = IKRollout(case["kin"], case["scene"], B, IKRolloutCfg(use_fused=fused, squared_l2_regularization_weight=list(reg)),
                   use_current_state=use_current_state)
    ro.update_goals(t(case["gpos"]), t(case["gquat"]), t(case["idx"]))
    if use_current_state:
        ro._v_b = t(case["v_b"]).contiguous()  # (the test's scaled velocity limits instead of the robot's)
    return ro


METRICS = ("pose_cost", "pose_pos_dist", "pose_rot_dist", "goalset_idx", "link_pos", "link_quat", "robot_spheres", "cspace_cost")


def _run(ro, case, fused, device):
    q = torch.as_tensor(case["q"], device=device)
    if fused:
        cost, grad = ro.cost_and_gradient_fused(q, with_metrics=True)
    else:
        cost, grad = ro.cost_and_gradient(q)
    torch.cuda.synchronize()
    return [cost.clone(), grad.clone()] + [getattr(ro, m).clone() for m in METRICS]


@pytest.mark.parametrize("reg", [(0.5, 0.2), (0.0, 0.2), (0.5, 0.0), (0.0, 0.0)])
@pytest.mark.parametrize("robot", ["franka", "unitree_g1", G1_SPARSE])  # D = 7; D = 49: three full 16-lane joint passes + one lane of a fourth
def test_ik_rollout_with_state_matches_oracle_composition(robot, reg, device):
    """both paths against the oracle's composition, and the launch against the kernel sequence.  The packaged G1 takes the kernel
    sequence only (what its solvers run: see ``_model``)."""
    case = _case(robot)
    D = case["model"].num_dof
    t = lambda a: torch.as_tensor(a, device=device)  # noqa: E731
    cs = _oracle_cspace(case, reg)
    # the shares of (row, joint) pairs, among the rows whose state has dt > 0, where the tightened bound changes the bound term
    bound, plain = _oracle_cspace(case, (0.0, 0.0))["cost"].reshape(B, D), _oracle_cspace(case, reg, with_state=False)["cost"].reshape(B, D)
    moving = STATE_DT[case["idxs_cur"]] > 0
    active = (bound != plain)[moving]
    assert 0 < moving.sum() < B
    assert active.mean() >= 0.3 and (~active).mean() >= 0.3, active.mean()
    assert np.array_equal(bound[~moving], plain[~moving]), "dt = 0 is the plain term"
    assert (plain > 0).any()
    want_cost = case["cost_rest"] + cs["cost"].sum((1, 2))
    want_grad = case["grad_rest"] + cs["grad_position"].reshape(B, D)
    outs = {}
    for fused in (False, True):
        ro = _rollout(case, fused, reg, device)
        assert ro.fused_available() == (robot != "unitree_g1")
        if fused and not ro.fused_available():
            return
        ro.update_current_state(t(case["cur"]), t(case["curv"]), t(STATE_DT), t(case["idxs_cur"]))
        out = outs[fused] = _run(ro, case, fused, device)
        np.testing.assert_allclose(out[0].cpu().numpy(), want_cost, rtol=1e-4, atol=1e-2, err_msg=f"cost, fused={fused}")
        np.testing.assert_allclose(out[1].cpu().numpy(), want_grad, rtol=2e-3, atol=2e-5 * np.abs(want_grad).max(),
                                   err_msg=f"gradient, fused={fused}")
    # the launch against the kernel sequence: cost, gradient and every metric buffer, cspace_cost (the whole term) included
    ref, got = outs[False], outs[True]
    assert torch.equal(ref[5], got[5]), "goal-set indices must be exact"
    for i, (a_, b_) in enumerate(zip(ref, got)):
        if i == 5:
            continue
        tol = dict(rtol=2e-3, atol=2e-5 * float(a_.abs().max())) if i == 1 else dict(rtol=2e-5, atol=2e-5 * max(1.0, float(a_.abs().max())))
        torch.testing.assert_close(b_.reshape(a_.shape), a_, **tol)
    np.testing.assert_allclose(got[9].cpu().numpy().reshape(B, D), cs["cost"].reshape(B, D), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("robot", ["franka", G1_SPARSE])
def test_state_variant_switched_off_equals_plain_launch_bit_for_bit(robot, device):
    """zero weights and dt = 0 in every state: the state variant's cost, gradient and metric buffers are the plain launch's"""
    case = _case(robot)
    t = lambda a: torch.as_tensor(a, device=device)  # noqa: E731
    plain = _run(_rollout(case, True, (0.0, 0.0), device, use_current_state=False), case, True, device)
    ro = _rollout(case, True, (0.0, 0.0), device)
    for dt in (None, 0.0, torch.zeros(N_STATES)):
        ro.update_current_state(t(case["cur"]), t(case["curv"]), dt, t(case["idxs_cur"]))
        got = _run(ro, case, True, device)
        for name, a_, b_ in zip(("cost", "grad") + METRICS, plain, got):
            assert torch.equal(a_, b_), name


# ------------------------------------------------------------------------------------------------------------- the solver
P, DT = 4, 0.05


def _solver_problems(oracle, step):
    """q_prev free of self collision (by the oracle), q_goal = q_prev + step * v_max * dt * (random signs), free as well: the goal
    poses are the FK of q_goal, so a successful solution ``step`` of the one-step box away from q_prev exists by construction"""
    model = load_model("franka")
    md = model.as_dict()
    rng = np.random.default_rng(31)
    v_max = model.joint_limits_velocity[1].astype(np.float32)
    free = lambda q: oracle.self_collision(oracle.kinematics_forward(q, md)["robot_spheres"].reshape(len(q), 1, -1, 4),  # noqa: E731
                                           model.sphere_padding, model.collision_pairs, 1.0)["distance"] == 0
    cand = sample_q(model, 64, seed=23, scale=0.5)
    signs = rng.choice([-1.0, 1.0], size=cand.shape).astype(np.float32)
    goal = (cand + step * v_max * DT * signs).astype(np.float32)
    lo, hi = model.joint_limits_position
    ok = free(cand) & free(goal) & ((goal > lo) & (goal < hi)).all(-1)
    sel = np.nonzero(ok)[0][:P]
    assert len(sel) == P
    fk = oracle.kinematics_forward(goal[sel], md)
    return model, cand[sel], goal[sel], fk["link_pos"][:, 0], fk["link_quat"][:, 0], v_max


def _make_ik(optimization_dt, use_cuda_graph=True):
    from curobo_amd.solver.inverse_kinematics import InverseKinematics, InverseKinematicsCfg

    return InverseKinematics(InverseKinematicsCfg.create("franka.yml", scene_model=None, num_seeds=1, use_lm_seed=False, exit_early=False,
                                                         optimization_dt=optimization_dt, use_cuda_graph=use_cuda_graph))


def _solve(ik, q_prev, gp, gq, device):
    from curobo_amd.types import GoalToolPose, JointState

    t = lambda a: torch.as_tensor(a, device=device)  # noqa: E731
    goal = GoalToolPose(list(ik.tool_frames), t(gp).reshape(P, 1, 1, 1, 3), t(gq).reshape(P, 1, 1, 1, 4))
    res = ik.solve_pose(goal, seed_config=t(q_prev).reshape(P, 1, -1), current_state=JointState.from_position(t(q_prev)))
    torch.cuda.synchronize()
    return res


def test_solver_reaches_goals_inside_the_one_step_box(oracle, device):
    step = 0.4  # (of the box; to be shrunk, not the assertions, should a problem fail on hardware)
    model, q_prev, _, gp, gq, v_max = _solver_problems(oracle, step)
    res = _solve(_make_ik(DT), q_prev, gp, gq, device)
    q = res.solution.reshape(P, -1).cpu().numpy()
    print("success", res.success.reshape(-1).tolist(), "max |dq| / (v_max dt)", (np.abs(q - q_prev) / (v_max * DT)).max(-1))
    assert res.success.all()
    assert (np.abs(q - q_prev) <= v_max * DT * (1 + 1e-5)).all()
    np.testing.assert_allclose(res.js_solution.velocity.reshape(P, -1).cpu().numpy(), (q - q_prev) / DT, rtol=1e-5, atol=1e-6)


def test_solver_does_not_report_success_outside_the_box(oracle, device):
    model, q_prev, _, gp, gq, v_max = _solver_problems(oracle, 4.0)
    res = _solve(_make_ik(DT), q_prev, gp, gq, device)
    q, ok = res.solution.reshape(P, -1).cpu().numpy(), res.success.reshape(P).cpu().numpy()
    inside = (np.abs(q - q_prev) <= v_max * DT * (1 + 1e-5)).all(-1)
    print("success", ok.tolist(), "inside", inside.tolist())
    assert (~ok | inside).all(), "success implies a solution within one step of the current state"
    # the goals themselves are reachable: without the limit the same solver reaches all of them
    free = _solve(_make_ik(None), q_prev, gp, gq, device)
    assert free.success.all()


def test_one_graphed_solver_follows_the_current_state(oracle, device):
    """the current state lives in fixed buffers: a solver whose graphs were captured on the first solve gives, for other states
    and goals, what a fresh solver gives"""
    model, q_prev, q_goal, gp, gq, v_max = _solver_problems(oracle, 0.4)
    md = model.as_dict()
    problems = [(q_prev, gp, gq)]
    for k in (1, 2):  # other states, their goals again 0.4 of the box away
        prev = (q_prev + 0.3 * k * (q_goal - q_prev)).astype(np.float32)
        fk = oracle.kinematics_forward((prev + (q_goal - q_prev) * (1.0 if k == 1 else -1.0)).astype(np.float32), md)
        problems.append((prev, fk["link_pos"][:, 0], fk["link_quat"][:, 0]))
    one = _make_ik(DT)
    kept = [_solve(one, *p, device).solution.clone() for p in problems]
    assert not torch.equal(kept[0], kept[1]) and not torch.equal(kept[1], kept[2])
    for p, sol in zip(problems, kept):
        fresh = _solve(_make_ik(DT), *p, device).solution
        torch.testing.assert_close(sol, fresh, rtol=0, atol=1e-6)
