"""What the velocity-aware IK and the motion retargeter promise without a GPU: the new entry point in the ABI and its argument
checks, the clip type, the configuration defaults of the reference, and that the IK front end keeps the arguments it used to drop."""

import dataclasses

import pytest
import torch

from curobo_amd import _lib

SYMBOL = "curobo_hip_rollout_ik_fused_state"


def test_state_entry_point_is_declared_bound_and_exported():
    lib = _lib.load()
    assert SYMBOL in _lib.declared_symbols()
    sigs = _lib._signatures()
    assert SYMBOL in sigs
    # the arguments of curobo_hip_rollout_ik_fused in its order, then the current state, the stream last
    plain, state = sigs["curobo_hip_rollout_ik_fused"], sigs[SYMBOL]
    assert state[:len(plain) - 1] == plain[:-1] and len(state) == len(plain) + 7
    assert hasattr(lib, SYMBOL)
    assert lib.curobo_hip_abi_version() == 7


def _call(lib, state_args):
    """the entry point with NULL pointers and the dimensions of a 7-dof arm: only the argument checks run"""
    n_plain = len(_lib._signatures()["curobo_hip_rollout_ik_fused"]) - 1
    args = [None] * n_plain
    sig = _lib._signatures()[SYMBOL]
    import ctypes

    for i, t in enumerate(sig[:n_plain]):
        if t is ctypes.c_int:
            args[i] = 0
    return lib.curobo_hip_rollout_ik_fused_state(*args, *state_args, None)


def test_state_arguments_are_rejected_without_a_gpu():
    """argument validation happens before any launch"""
    lib = _lib.load()
    buf = torch.zeros(16)
    p = buf.data_ptr()
    # state_dt but no current_position
    rc = _call(lib, [p, None, None, None, None, p, 0])
    assert rc == 1 and b"given together or not at all" in lib.curobo_hip_last_error()
    with pytest.raises(ValueError, match="rollout_ik_fused_state"):
        _lib.check(rc)
    # no current state at all: the plain entry point is the launch without one
    rc = _call(lib, [p, None, None, None, None, None, 0])
    assert rc == 1 and b"needs a current state" in lib.curobo_hip_last_error()
    # acceleration regularisation configured, no current velocity
    rc = _call(lib, [p, p, None, p, p, p, 1])
    assert rc == 1 and b"current_velocity is required" in lib.curobo_hip_last_error()
    # no regularisation weights
    rc = _call(lib, [None, p, None, p, p, p, 0])
    assert rc == 1 and b"squared_l2_reg_weight" in lib.curobo_hip_last_error()


def test_backend_takes_the_state_as_keywords_after_the_existing_arguments():
    import inspect

    from curobo_amd.backends import rollout

    names = list(inspect.signature(rollout.rollout_ik_fused).parameters)
    i = names.index("use_multi_env")
    assert names[i + 1:] == ["squared_l2_reg_weight", "current_position", "current_velocity", "idxs_current_state",
                             "velocity_limits", "state_dt", "acceleration_regularization"]


def test_sequence_goal_tool_pose():
    from curobo_amd.types import GoalToolPose, SequenceGoalToolPose

    F, E, L, G = 5, 2, 3, 4
    pos, quat = torch.randn(F, E, L, G, 3), torch.randn(F, E, L, G, 4)
    seq = SequenceGoalToolPose(["a", "b", "c"], pos, quat)
    assert (seq.num_frames, seq.num_envs, seq.num_links, seq.num_goalset) == (F, E, L, G)
    assert seq.device == pos.device
    fr = seq.get_frame(3)
    assert isinstance(fr, GoalToolPose) and fr.horizon == 1 and fr.batch_size == E
    assert fr.position.shape == (E, 1, L, G, 3) and fr.quaternion.shape == (E, 1, L, G, 4)
    assert fr.position.data_ptr() == pos[3].data_ptr() and fr.quaternion.data_ptr() == quat[3].data_ptr(), "a view, no copy"
    pos[3, 1, 2, 0, 1] = 42.0
    assert float(fr.position[1, 0, 2, 0, 1]) == 42.0
    cl = seq.clone()
    assert cl.position.data_ptr() != pos.data_ptr() and torch.equal(cl.position, pos) and cl.tool_frames == seq.tool_frames
    with pytest.raises(ValueError, match="5D"):
        SequenceGoalToolPose(["a", "b", "c"], pos[0], quat)
    with pytest.raises(ValueError, match="5D"):
        SequenceGoalToolPose(["a", "b", "c"], pos, quat[0])
    with pytest.raises(ValueError, match="tool_frames"):
        SequenceGoalToolPose(["a", "b"], pos, quat)


# the reference's MotionRetargeterCfg.create defaults (motion_retargeter_cfg.py:140-165)
REFERENCE_CREATE_DEFAULTS = dict(
    num_envs=1, use_mpc=False, self_collision_check=True, scene_model=None, optimization_dt=0.05, num_seeds_global=64,
    load_collision_spheres=True, ik_optimizer_configs=["ik/lbfgs_retarget_ik.yml"],
    mpc_optimizer_configs=["mpc/lbfgs_retarget_mpc.yml"], num_seeds_local=1, num_control_points=12, steps_per_target=4,
    position_tolerance=0.005, orientation_tolerance=0.05, velocity_regularization_weight=None,
    acceleration_regularization_weight=None, collision_activation_distance=0.01, global_ik_num_iters=None,
    local_ik_num_iters=None, mpc_warm_start_num_iters=100, mpc_cold_start_num_iters=300)
# ... and of the dataclass itself where they differ (:88-98)
REFERENCE_FIELD_DEFAULTS = dict(REFERENCE_CREATE_DEFAULTS, num_control_points=None, steps_per_target=8)


def test_retargeter_cfg_defaults_are_the_references():
    import inspect

    from curobo_amd.motion_retargeter import MotionRetargeterCfg
    from curobo_amd.types import DeviceCfg, ToolPoseCriteria

    crit = {"panda_hand": ToolPoseCriteria.track_position_and_orientation()}
    cfg = MotionRetargeterCfg.create(robot="franka.yml", tool_pose_criteria=crit)
    for k, v in REFERENCE_CREATE_DEFAULTS.items():
        assert getattr(cfg, k) == v, k
    assert isinstance(cfg.device_cfg, DeviceCfg) and cfg.tool_frames == ["panda_hand"]
    plain = MotionRetargeterCfg(robot="franka.yml", tool_pose_criteria=crit)
    for k, v in REFERENCE_FIELD_DEFAULTS.items():
        assert getattr(plain, k) == v, k
    params = list(inspect.signature(MotionRetargeterCfg.create).parameters)
    assert params == ["robot", "tool_pose_criteria", "num_envs", "use_mpc", "self_collision_check", "scene_model",
                      "optimization_dt", "num_seeds_global", "load_collision_spheres", "ik_optimizer_configs",
                      "mpc_optimizer_configs", "num_seeds_local", "num_control_points", "steps_per_target", "position_tolerance",
                      "orientation_tolerance", "device_cfg", "velocity_regularization_weight",
                      "acceleration_regularization_weight", "collision_activation_distance", "global_ik_num_iters",
                      "local_ik_num_iters", "mpc_warm_start_num_iters", "mpc_cold_start_num_iters"]
    assert [f.name for f in dataclasses.fields(MotionRetargeterCfg)][:2] == ["robot", "tool_pose_criteria"]


def test_retarget_task_values():
    """the numbers of the reference's ik/lbfgs_retarget_ik.yml"""
    from curobo_amd.motion_retargeter import retarget_ik_task_cfg

    t = retarget_ik_task_cfg()
    assert t.rollout.pose_weight == [1000.0, 100.0] and t.rollout.cspace_weight == [10000.0, 0.0]
    assert t.rollout.squared_l2_regularization_weight == [0.01, 0.01]
    assert t.rollout.scene_collision_weight == 10000.0 and t.rollout.self_collision_weight == 10000.0
    o = t.optimizer
    assert (o.history, o.inner_iters, o.num_iters, o.fixed_iters) == (15, 20, 200, True)


def test_load_collision_spheres_rule():
    from curobo_amd.motion_retargeter import MotionRetargeterCfg

    assert MotionRetargeterCfg.create("franka.yml", {}, self_collision_check=False).load_collision_spheres is False
    assert MotionRetargeterCfg.create("franka.yml", {}, self_collision_check=True).load_collision_spheres is True
    assert MotionRetargeterCfg.create("franka.yml", {}, self_collision_check=False, scene_model={"cuboid": {}}).load_collision_spheres is True
    with pytest.raises(ValueError, match="load_collision_spheres"):
        MotionRetargeterCfg.create("franka.yml", {}, self_collision_check=True, load_collision_spheres=False)
    with pytest.raises(ValueError, match="load_collision_spheres"):
        MotionRetargeterCfg.create("franka.yml", {}, self_collision_check=False, scene_model={"cuboid": {}}, load_collision_spheres=False)


def test_use_mpc_is_refused_by_name():
    from curobo_amd.motion_retargeter import MotionRetargeter, MotionRetargeterCfg

    cfg = MotionRetargeterCfg.create("franka.yml", {}, use_mpc=True)  # (the configuration itself is the reference's: no error yet)
    with pytest.raises(NotImplementedError, match="use_mpc"):
        MotionRetargeter(cfg)


def test_ik_cfg_keeps_the_velocity_arguments():
    """optimization_dt and the regularisation weights used to vanish in **unused"""
    from curobo_amd.solver.inverse_kinematics import InverseKinematicsCfg
    from curobo_amd.types import DeviceCfg

    cfg = InverseKinematicsCfg.create("franka.yml", device_cfg=DeviceCfg(device="cpu"), optimization_dt=0.05,
                                      velocity_regularization_weight=0.3, override_optimizer_num_iters={"lbfgs": 110})
    assert cfg.optimization_dt == 0.05 and cfg.velocity_regularization_weight == 0.3
    assert cfg.acceleration_regularization_weight is None and cfg.override_optimizer_num_iters == {"lbfgs": 110}
    plain = InverseKinematicsCfg.create("franka.yml", device_cfg=DeviceCfg(device="cpu"))
    assert plain.optimization_dt is None and plain.velocity_regularization_weight is None and plain.override_optimizer_num_iters is None


def test_solver_and_rollout_cfg_defaults_leave_existing_objects_alone():
    from curobo_amd.rollout.ik_rollout import IKRolloutCfg
    from curobo_amd.solver import IKSolverCfg

    assert IKSolverCfg().optimization_dt is None
    assert IKRolloutCfg().squared_l2_regularization_weight == [0.0, 0.0]
    assert dataclasses.fields(IKRolloutCfg)[-1].name == "squared_l2_regularization_weight"


def test_facade_exports_exactly_the_reference_names():
    # loaded by path: other tests of the suite import the reference's ``curobo``, and this one must not put another in sys.modules
    import importlib.util
    import os

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location("_facade_curobo_motion_retargeter", os.path.join(ROOT, "curobo", "motion_retargeter.py"))
    facade = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(facade)
    assert sorted(facade.__all__) == ["GoalToolPose", "MotionRetargeter", "MotionRetargeterCfg", "RetargetResult", "SequenceGoalToolPose"]
    for n in facade.__all__:
        assert getattr(facade, n) is not None
    from curobo_amd.motion_retargeter import RetargetResult

    assert [f.name for f in dataclasses.fields(RetargetResult)] == ["joint_state", "trajectory", "success"]
