"""``MotionRetargeter`` end to end: a clip of tool-pose targets -> a joint trajectory whose every step is within what the joints can
do in one time step, on the Franka (targets reached, checked with the oracle) and on the Unitree G1 (four tool frames)."""

import functools

import numpy as np
import pytest
import torch

from conftest import load_model

pytestmark = pytest.mark.gpu

DT, E, F = 0.05, 2, 8


def _retargeter(robot, num_envs, **kw):
    from curobo_amd.kinematics import KinematicsCfg
    from curobo_amd.motion_retargeter import MotionRetargeter, MotionRetargeterCfg
    from curobo_amd.types import ToolPoseCriteria

    frames = KinematicsCfg.from_packaged(robot).kinematics_config.tool_frames
    crit = {f: ToolPoseCriteria.track_position_and_orientation() for f in frames}
    return MotionRetargeter(MotionRetargeterCfg.create(robot=f"{robot}.yml", tool_pose_criteria=crit, num_envs=num_envs,
                                                       optimization_dt=DT, num_seeds_global=16, global_ik_num_iters=100,
                                                       local_ik_num_iters=100, **kw))


def _clip(rt, q_traj):
    """joint clip [F, E, D] -> SequenceGoalToolPose of its tool poses (the retargeter's own kinematics, on the device)"""
    from curobo_amd.types import SequenceGoalToolPose

    n_f, n_e, D = q_traj.shape
    tp = rt.kinematics.compute_kinematics(q_traj.reshape(n_f * n_e, D)).tool_poses
    T = len(rt.tool_frames)
    return SequenceGoalToolPose(list(rt.tool_frames), tp.position.reshape(n_f, n_e, T, 1, 3).clone(),
                                tp.quaternion.reshape(n_f, n_e, T, 1, 4).clone())


@functools.lru_cache(maxsize=None)
def _franka():
    """the retargeter, the clip e = FK(q0 + t * 0.25 * v_max * dt * s_e) and the first solve_sequence, shared by the tests"""
    rt = _retargeter("franka", E)
    model = load_model("franka")
    v_max = torch.as_tensor(model.joint_limits_velocity[1], dtype=torch.float32, device="cuda:0")
    q0 = rt.default_joint_state.position.reshape(-1)
    rng = np.random.default_rng(3)
    s = torch.as_tensor(rng.choice([-1.0, 1.0], size=(E, model.num_dof)).astype(np.float32), device="cuda:0")
    t = torch.arange(F, device="cuda:0", dtype=torch.float32).view(F, 1, 1)
    q_traj = q0.view(1, 1, -1) + t * 0.25 * v_max * DT * s.view(1, E, -1)
    clip = _clip(rt, q_traj)
    res = rt.solve_sequence(clip)
    torch.cuda.synchronize()
    return rt, model, v_max, clip, res


def test_franka_sequence_tracks_the_clip_within_the_velocity_box(oracle, device):
    rt, model, v_max, clip, res = _franka()
    pos = res.joint_state.position
    assert pos.shape == (E, F, 7) and res.success.shape == (E, F) and res.success.dtype == torch.bool
    assert res.trajectory is None
    assert res.success.all(), res.success
    step = (pos[:, 1:] - pos[:, :-1]).abs()
    assert (step <= v_max * DT * (1 + 1e-5)).all(), float((step / (v_max * DT)).max())
    # the targets are reached within the configured tolerances: the device kinematics on every frame ...
    c = rt.config
    tp = rt.kinematics.compute_kinematics(pos.reshape(E * F, 7)).tool_poses
    want_p = clip.position.permute(1, 0, 2, 3, 4).reshape(E * F, 1, 3)
    want_q = clip.quaternion.permute(1, 0, 2, 3, 4).reshape(E * F, 1, 4)
    assert ((tp.position.reshape(E * F, 1, 3) - want_p).norm(dim=-1) < c.position_tolerance).all()
    dot = (tp.quaternion.reshape(E * F, 1, 4) * want_q).sum(-1).abs().clamp(max=1.0)
    assert (2 * torch.acos(dot) < c.orientation_tolerance).all()
    # ... and the oracle's on the first and the last
    md = model.as_dict()
    for f in (0, F - 1):
        fk = oracle.kinematics_forward(pos[:, f].cpu().numpy(), md)
        gp, gq = clip.position[f, :, 0, 0].cpu().numpy(), clip.quaternion[f, :, 0, 0].cpu().numpy()
        assert (np.linalg.norm(fk["link_pos"][:, 0] - gp, axis=-1) < c.position_tolerance).all()
        d = np.clip(np.abs((fk["link_quat"][:, 0] * gq).sum(-1)), 0, 1)
        assert (2 * np.arccos(d) < c.orientation_tolerance).all()


def test_franka_solve_frame_reset_and_batch_checks(device):
    from curobo_amd.types import GoalToolPose, SequenceGoalToolPose

    rt, model, v_max, clip, first = _franka()
    rt.reset()
    a = rt.solve_frame(clip.get_frame(0))  # global
    b = rt.solve_frame(clip.get_frame(1))  # warm-started at a, one time step from it
    assert a.joint_state.position.shape == (E, 7) and a.success.shape == (E,) and b.success.all()
    assert ((b.joint_state.position - a.joint_state.position).abs() <= v_max * DT * (1 + 1e-5)).all()
    assert rt._prev_solution is not None
    rt.reset()
    assert rt._prev_solution is None and rt._prev_velocity is None
    again = rt.solve_sequence(clip)  # (resets first; the global solver's seeds are the same set every solve)
    torch.testing.assert_close(again.joint_state.position, first.joint_state.position, rtol=0, atol=1e-5)
    assert torch.equal(again.success, first.success)
    one = clip.get_frame(0)
    with pytest.raises(ValueError, match="num_envs"):
        rt.solve_frame(GoalToolPose(one.tool_frames, one.position[:1], one.quaternion[:1]))
    with pytest.raises(ValueError, match="num_envs"):
        rt.solve_sequence(SequenceGoalToolPose(clip.tool_frames, clip.position[:, :1], clip.quaternion[:, :1]))
    assert rt.action_dim == rt.num_dof == 7 and rt.tool_frames == ["panda_hand"] and len(rt.joint_names) == 7


def test_g1_four_tool_frames(device):
    rt = _retargeter("unitree_g1", 1, self_collision_check=True)
    model = load_model("unitree_g1")
    D, n_f = model.num_dof, 3
    assert len(rt.tool_frames) == 4 and rt.action_dim == D
    v_max = torch.as_tensor(model.joint_limits_velocity[1], dtype=torch.float32, device=device)
    q0 = rt.default_joint_state.position.reshape(-1)
    s = torch.as_tensor(np.random.default_rng(4).choice([-1.0, 1.0], size=D).astype(np.float32), device=device)
    t = torch.arange(n_f, device=device, dtype=torch.float32).view(n_f, 1, 1)
    lo, hi = (torch.as_tensor(x, dtype=torch.float32, device=device) for x in model.joint_limits_position)
    q_traj = torch.minimum(torch.maximum(q0.view(1, 1, D) + t * 0.25 * v_max * DT * s.view(1, 1, D), lo), hi)
    res = rt.solve_sequence(_clip(rt, q_traj))
    torch.cuda.synchronize()
    pos = res.joint_state.position
    assert pos.shape == (1, n_f, D) and res.success.shape == (1, n_f)
    inside = ((pos[:, 1:] - pos[:, :-1]).abs() <= v_max * DT * (1 + 1e-5)).all(-1)
    print("G1 retarget success per frame:", res.success.tolist(), "share", float(res.success.float().mean()),
          "steps inside the box:", inside.tolist())
    assert (~res.success[:, 1:] | inside).all(), "success implies a step within the box"
