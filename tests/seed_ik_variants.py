"""Robot variants and deterministic problems of the fused seed-IK tests (TEST INFRASTRUCTURE ONLY, no GPU): the CPU
pins (tests/test_oracle_seed_ik.py) and the GPU test (tests/test_gpu_seed_ik_fused.py) build identical inputs from here and
share one oracle run per (case, option, iterations) (``reference``, cached).

``curobo_hip_seed_ik_iterate`` has three instantiations: ``<7,1>``, ``<6,1>`` (compile-time dof and frame count, normal
equations in registers) and ``<0,0>`` (run-time sizes, row-distributed Cholesky and broadcast solves).  The packaged robots
reach only the first two, so the variants below are derived from them with ``dataclasses.replace``: more tool frames, or
fewer dofs, land in ``<0,0>``.

    case  model                                    D, T   instantiation   fused LDS
    A     franka                                   7, 1   <7,1>           40 512 B
    B     ur10e                                    6, 1   <6,1>           32 384 B
    C     franka + panda_link6                     7, 2   <0,0>           46 656 B
    D     ur10e + wrist_1_link, wrist_3_link       6, 3   <0,0>           43 136 B
    E     franka, panda_joint5 / _joint7 locked    5, 1   <0,0>, D < 6    smaller than A
    F     the joint zoo (tests/joint_zoo.py)       6, 4   <0,0>           fits (asserted)

F is no packaged robot: prismatic joints behind revolute ones, multipliers outside {+-1}, biases and two dofs with two links
each (the ``atomicAdd`` Jacobian columns of the launch).
"""

import dataclasses
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

#: problems, seeds per problem: n = 91 rows = 5 * 16 + 11 = 22 * 4 + 3, so the last workgroup (16 rows) and the last
#: wavefront (4 rows) of the launch are both partial
P, S = 13, 7
#: a seed is on the knife edge when a trust ratio of the oracle's run is this close to ``rho_min``; at most KNIFE_CAP of the rows
KNIFE_MARGIN, KNIFE_CAP = 1e-3, 0.02
#: goal sets: a seed is kept when the two best members of every frame differ by more than this (relative) in every evaluation
GOALSET_MARGIN, GOALSET_KEEP = 1e-4, 0.95


# ------------------------------------------------------------------------------------------------ variants
def _chain(model, link):
    off = model.link_chain_offsets
    return set(int(x) for x in model.link_chain_data[int(off[link]):int(off[link + 1])])


def _affects(model, joint_map, num_dof, tool_frame_map):
    """[D, T] flattened: joint j affects frame t iff one of its links lies on the chain of the frame's link"""
    out = np.zeros((num_dof, len(tool_frame_map)), bool)
    for t, link in enumerate(tool_frame_map):
        chain = _chain(model, int(link))
        for j in range(num_dof):
            out[j, t] = any(int(i) in chain for i in np.nonzero(joint_map == j)[0])
    return out.reshape(-1).copy()


def with_tool_frames(model, extra_link_indices):
    """``model`` with the links ``extra_link_indices`` appended as tool frames"""
    tfm = np.concatenate([model.tool_frame_map, np.asarray(extra_link_indices, np.int16)]).astype(np.int16)
    return dataclasses.replace(
        model, tool_frame_map=tfm, tool_frames=list(model.tool_frames) + [model.link_names[int(i)] for i in extra_link_indices],
        joint_affects_endeffector=_affects(model, model.joint_map, model.num_dof, tfm))


def with_locked_joints(model, joint_indices):
    """``model`` without the dofs ``joint_indices`` (indices into ``joint_names``), held at value 0: their links become
    fixed (the joint's transform at ``multiplier * 0 + offset`` baked into ``fixed_transforms`` when the offset is not 0:
    a rotation by 0 is the identity, bit for bit), later joints are renumbered"""
    from curobo_amd.robot.loader import FIXED, _local_transform

    fixed, jm, jt = model.fixed_transforms.copy(), model.joint_map.copy(), model.joint_map_type.copy()
    off = model.joint_offset_map.reshape(-1, 2)
    drop = sorted(set(int(j) for j in joint_indices))
    for j in reversed(drop):
        for i in np.nonzero(jm == j)[0]:
            if off[i, 1] != 0.0:
                fixed[i] = _local_transform(fixed[i].astype(np.float64), int(jt[i]), float(off[i, 1])).astype(np.float32)
            jt[i], jm[i] = FIXED, -1
        jm[jm > j] -= 1
    keep = [j for j in range(model.num_dof) if j not in drop]
    D = len(keep)
    jl_data, jl_off = [], [0]
    for j in range(D):
        jl_data.extend(int(i) for i in np.nonzero(jm == j)[0])
        jl_off.append(len(jl_data))
    cspace = {k: ([v[j] for j in keep] if isinstance(v, (list, tuple)) and len(v) == model.num_dof else v)
              for k, v in model.cspace.items()}
    return dataclasses.replace(
        model, fixed_transforms=fixed, joint_map=jm, joint_map_type=jt, num_dof=D,
        joint_limits_position=model.joint_limits_position[:, keep].copy(),
        joint_limits_velocity=model.joint_limits_velocity[:, keep].copy(),
        joint_limits_effort=np.asarray(model.joint_limits_effort)[keep].copy(),
        joint_links_data=np.asarray(jl_data, np.int16), joint_links_offsets=np.asarray(jl_off, np.int16),
        joint_affects_endeffector=_affects(model, jm, D, model.tool_frame_map),
        joint_names=[model.joint_names[j] for j in keep], cspace=cspace,
        lock_joints={**model.lock_joints, **{model.joint_names[j]: 0.0 for j in drop}})


def _joint_zoo():
    import joint_zoo

    return joint_zoo.model()


#: case -> (packaged robot or a model factory, extra tool-frame links, locked joints, D, T, instantiation)
CASES = {
    "A": ("franka", (), (), 7, 1, "<7,1>"),
    "B": ("ur10e", (), (), 6, 1, "<6,1>"),
    "C": ("franka", (6,), (), 7, 2, "<0,0>"),          # + panda_link6
    "D": ("ur10e", (5, 7), (), 6, 3, "<0,0>"),          # + wrist_1_link, wrist_3_link
    "E": ("franka", (), (4, 6), 5, 1, "<0,0>"),         # panda_joint5 and panda_joint7 locked: D < 6
    "F": (_joint_zoo, (), (), 6, 4, "<0,0>"),           # no packaged robot: every joint type, mimic links, biases
}
#: seed of the problem's random draws per case (a case whose knife-edge share exceeded the cap would get another seed here)
PROBLEM_SEED = {"A": 0, "B": 0, "C": 0, "D": 0, "E": 0, "F": 0}


@functools.lru_cache(maxsize=None)
def packaged(name):
    from curobo_amd.robot import load_packaged_robot

    return load_packaged_robot(name)


@functools.lru_cache(maxsize=None)
def case_model(case):
    name, frames, locked, D, T, _ = CASES[case]
    m = name() if callable(name) else packaged(name)
    if frames:
        m = with_tool_frames(m, frames)
    if locked:
        m = with_locked_joints(m, locked)
    assert (m.num_dof, len(m.tool_frame_map)) == (D, T)
    return m


def fused_fits(model):
    from curobo_amd.backends import linalg

    return linalg.seed_ik_iterate_fits(model.num_dof, model.num_links, len(model.tool_frame_map), len(model.link_chain_data))


# ------------------------------------------------------------------------------------------------ problems
def problem(orc, model, num_problems=P, num_seeds=S, seed=0, num_goalset=1):
    """(model dictionary, goal positions [P, T, G, 3], goal quaternions [P, T, G, 4], seeds [P * S, D], idxs_goal): random
    seeds inside the joint limits, goals = FK of random configurations (``_problem`` of tests/test_gpu_seed_ik.py; with a
    goal set the further members are FK of further draws, made AFTER every draw of the single-goal problem)"""
    md = model.as_dict()
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(md["joint_limits_position"], np.float32)
    D, T = lo.shape[0], md["tool_frame_map"].shape[0]
    draw = lambda n: (lo + (hi - lo) * rng.random((n, D))).astype(np.float32)  # noqa: E731
    qg = draw(num_problems)
    seeds = draw(num_problems * num_seeds)
    members = [qg] + [draw(num_problems) for _ in range(num_goalset - 1)]
    fks = [orc.kinematics_forward(q, md, compute_spheres=False) for q in members]
    gp = np.stack([f["link_pos"].reshape(num_problems, T, 3) for f in fks], 2)
    gq = np.stack([f["link_quat"].reshape(num_problems, T, 4) for f in fks], 2)
    return md, np.ascontiguousarray(gp), np.ascontiguousarray(gq), seeds, np.repeat(np.arange(num_problems, dtype=np.int32), num_seeds)


def clamp_inputs(model, num_problems=P, num_seeds=S, seed=4, dt=0.2):
    """(current_position [n, D], dt [n], current_velocity [n, D]) per row, one current state per problem, as
    ``test_velocity_clamped_bounds_kernel_and_solver`` draws it: the middle half of the joint range"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(model.joint_limits_position, np.float32)
    D = lo.shape[0]
    cur = (lo + (hi - lo) * (0.25 + 0.5 * rng.random((num_problems, D)))).astype(np.float32)
    vmax = np.asarray(model.joint_limits_velocity, np.float32)[1]
    vel = (0.5 * vmax * (2 * rng.random((num_problems, D)) - 1)).astype(np.float32)
    n = num_problems * num_seeds
    return np.repeat(cur, num_seeds, 0), np.full(n, dt, np.float32), np.repeat(vel, num_seeds, 0)


_OPTIONS = ("plain", "goalset", "goalset_permuted", "clamped", "velacc")


@functools.lru_cache(maxsize=None)
def inputs(case, option="plain"):
    """the problem of a case under an option, as a dictionary: md, goal_position, goal_quat, seeds, idxs_goal and
    ``extra`` (keyword arguments of ``seed_ik_ref.evaluate``: current_position, dt, current_velocity)"""
    from oracle import load_oracle

    assert option in _OPTIONS, option
    model = case_model(case)
    G = 3 if option.startswith("goalset") else 1
    md, gp, gq, seeds, idx = problem(load_oracle(), model, seed=PROBLEM_SEED[case], num_goalset=G)
    if option == "goalset_permuted":  # a row's goal is not row // S
        idx = np.random.default_rng(11).permutation(idx).astype(np.int32)
    extra = {}
    if option in ("clamped", "velacc"):
        cur, dt, vel = clamp_inputs(model)
        extra = dict(current_position=cur, dt=dt)
        if option == "velacc":
            extra["current_velocity"] = vel
    return dict(model=model, md=md, goal_position=gp, goal_quat=gq, seeds=seeds, idxs_goal=idx, extra=extra, G=G)


@functools.lru_cache(maxsize=None)
def reference(case, iterations, option="plain", velocity_weight=0.0, acceleration_weight=0.0, lm_float64=False):
    """the oracle's state after the initial evaluation and ``iterations`` LM iterations (``seed_ik_ref.iterate``); shared,
    never modified"""
    from oracle import load_oracle
    from oracle import seed_ik_ref as R

    x = inputs(case, option)
    extra = dict(x["extra"])
    if option == "velacc":
        extra.update(velocity_weight=velocity_weight, acceleration_weight=acceleration_weight)
    st = R.iterate(load_oracle(), x["md"], R.SeedIKRefCfg(), x["seeds"], x["goal_position"], x["goal_quat"], x["idxs_goal"],
                   iterations, lm_float64=lm_float64, **extra)
    for v in st.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return st


#: case -> iterations -> (jacobian, jTerror): ``sensitivity`` as measured on the CPU (rounded up to two digits); the GPU test
#: allows SENSITIVITY_FACTOR times these, tests/test_oracle_seed_ik.py checks that they still are what the CPU measures
MEASURED = {
    "A": {1: (9.6e-7, 8.1e-7), 2: (1.4e-6, 1.2e-6), 4: (3.1e-6, 2.2e-6)},
    "B": {1: (8.8e-7, 1.2e-6), 2: (4.3e-6, 1.7e-6), 4: (7.6e-6, 3.0e-6)},
    "C": {1: (1.6e-6, 7.4e-7), 2: (3.6e-6, 3.6e-6), 4: (2.2e-5, 4.8e-6)},
    "D": {1: (2.1e-6, 1.7e-6), 2: (5.8e-6, 2.5e-6), 4: (7.8e-6, 4.6e-6)},
    "E": {1: (7.1e-7, 6.1e-7), 2: (3.1e-6, 1.5e-6), 4: (3.4e-6, 1.4e-6)},
    "F": {1: (2.3e-6, 2.2e-6), 2: (2.9e-6, 3.5e-6), 4: (1.7e-6, 2.0e-6)},
}
SENSITIVITY_FACTOR = 8.0


def knife_edge(ref, rho_min=1e-3):
    """rows [n] with a trust ratio of any iteration within KNIFE_MARGIN * (1 + |rho|) of the accept threshold"""
    rho = ref["rho"]
    if rho.shape[0] == 0:
        return np.zeros(rho.shape[1], bool)
    return (np.abs(rho - np.float32(rho_min)) <= KNIFE_MARGIN * (1 + np.abs(rho))).any(0)


def sensitivity(case, iterations, key):
    """largest difference of ``key`` between the fp32 oracle and the same iteration with the LM solve in float64, in units
    of max |value|: the arithmetic's own sensitivity, from which the k >= 1 bounds on ``jacobian`` / ``jTerror`` are taken"""
    a, b = reference(case, iterations), reference(case, iterations, lm_float64=True)
    return float(np.abs(a[key].astype(np.float64) - b[key]).max() / np.abs(b[key]).max())
