"""Deterministic inputs of the graph-planner tests (TEST INFRASTRUCTURE ONLY, no GPU): the CPU test of the oracle
(tests/test_oracle_graph.py) and the GPU test (tests/test_gpu_graph_planner.py) build byte-identical batches from here, and
share one oracle evaluation per batch (``steering_reference`` / ``points_reference``, cached).

Shapes are the smallest at which ``csrc/graph_planner.hip`` can still go wrong: a workgroup walks an edge 16 points at a time
(point counts 16, 17 and 40; first infeasible step at 0, 1, 15, 16, 17, 31, 32 and the last), the steering grid is capped at 2048
workgroups (2048 + 37 edges, 32768 + 5 points), a k-NN wave holds 64 slots and scans 64 nodes at a time (1, 63, 64, 65 nodes;
k = 64; query counts that are no multiple of the 4 waves of a workgroup).  THRESHOLD 0.05 keeps every batch at or below
about 100 k points, seconds for the CPU oracle."""

import functools
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

THRESHOLD = 0.05
#: share of a batch's edges / points that the oracle's band may leave undecided (a condition on the batches, checked on the CPU)
UNDECIDED_CAP = 0.05
GRID_CAP = 2048  # workgroups of one steering launch (curobo_hip_graph_steer)

PRIMITIVE_WORLD = {"cuboid": {"table": {"dims": [2.0, 2.0, 0.2], "pose": [0.0, 0.0, -0.1, 1, 0, 0, 0]}},
                   "sphere": {"ball": {"radius": 0.2, "pose": [0.45, 0.3, 0.5, 1, 0, 0, 0]}},
                   "capsule": {"rod": {"radius": 0.08, "base": [0, 0, -0.3], "tip": [0, 0, 0.3],
                                       "pose": [-0.3, -0.45, 0.6, 0.9238795, 0.3826834, 0, 0]}},
                   "cylinder": {"post": {"radius": 0.1, "height": 0.8, "pose": [0.1, -0.6, 0.4, 1, 0, 0, 0]}}}

ROBOTS = ("franka", "ur10e", "dual_ur10e", "unitree_g1")
SCENES = ("none", "c2", "voxels", "c3", "primitives", "slots40")  # (and "slots64", below, for the launch's large-LDS path)


# ------------------------------------------------------------------------------------------------ robots and scenes
@functools.lru_cache(maxsize=None)
def robot(name):
    from curobo_amd.robot import load_packaged_robot

    return load_packaged_robot(name)


def slots40_world(n_slots=40):
    """40 cuboid slots (``n_slots``: further disabled ones behind them), five enabled (0, 7, 31, 32, 39: both sides of the 32-obstacle link mask), the rest disabled; the
    disabled slots 5 and 35 hold a box around the robot's base that makes every configuration infeasible if it is honoured"""
    enabled = {0: {"dims": [2.2, 2.2, 0.2], "pose": [0.0, 0.0, -0.1, 1, 0, 0, 0]},
               7: {"dims": [0.1, 0.1, 1.5], "pose": [0.45, 0.0, 0.3, 1, 0, 0, 0]},
               31: {"dims": [0.3, 0.3, 0.3], "pose": [0.2, 0.55, 0.45, 0.9887711, 0, 0, 0.1494381]},
               32: {"dims": [0.25, 0.25, 0.25], "pose": [-0.2, -0.5, 0.7, 1, 0, 0, 0]},
               39: {"dims": [0.2, 0.4, 0.2], "pose": [-0.45, 0.3, 0.35, 1, 0, 0, 0]}}
    rng = np.random.default_rng(40)
    out = []
    for i in range(n_slots):
        if i in enabled:
            out.append(dict(enabled[i]))
        elif i in (5, 35):
            out.append({"dims": [1.0, 1.0, 1.6], "pose": [0.0, 0.0, 0.5, 1, 0, 0, 0], "enable": False})
        else:
            p = rng.uniform([-0.7, -0.7, 0.0], [0.7, 0.7, 1.0])
            out.append({"dims": [float(v) for v in rng.uniform(0.1, 0.5, 3)], "pose": [*(float(v) for v in p), 1, 0, 0, 0], "enable": False})
    return [out]


@functools.lru_cache(maxsize=None)
def scene_arrays(kind):
    """the oracle's scene dictionary (``None`` for no scene); ``scene_data`` uploads the same arrays"""
    from curobo_amd.scene import cuboid_scene_arrays
    from curobo_amd.scene.config import scene_arrays_from_config
    from curobo_amd.workloads import c2_world, c3_voxel_world

    if kind == "none":
        return None
    if kind == "c2":
        return cuboid_scene_arrays(c2_world())
    if kind == "voxels":  # no cuboid store at all: the launch's voxel-only instantiation
        return c3_voxel_world(64, 0.04)
    if kind == "c3":
        return {**cuboid_scene_arrays(c2_world()), **c3_voxel_world(64, 0.04)}
    if kind == "primitives":
        return scene_arrays_from_config(PRIMITIVE_WORLD)
    if kind == "slots40":
        return cuboid_scene_arrays(slots40_world())
    if kind == "slots64":  # the same world in 64 slots: with dual_ur10e the launch needs more than 60 KiB of LDS
        return cuboid_scene_arrays(slots40_world(64))
    raise ValueError(kind)


def obstacle_slots(kind):
    a = scene_arrays(kind)
    if a is None:
        return 0
    return (int(a["cuboid_dims"].shape[1]) if "cuboid_dims" in a else 0) + (int(a["voxel_params"].shape[1]) if "voxel_params" in a else 0)


def fused_lds_bytes(robot_name, scene_kind):
    """LDS bytes of the steering launch for this robot and scene (``rollout_ik_fused_lds_bytes``, what ``GraphFeasibility.uses_fused``
    and ``curobo_hip_graph_steer`` size the launch with)"""
    from curobo_amd.backends import rollout as rollout_hip

    m = robot(robot_name)
    return rollout_hip.rollout_ik_fused_lds_bytes(m.num_dof, m.num_links, m.num_spheres, int(np.asarray(m.collision_pairs).reshape(-1, 2).shape[0]),
                                                  int(m.link_chain_data.shape[0]), obstacle_slots(scene_kind))


def fits_fused(robot_name, scene_kind):
    """``GraphFeasibility.uses_fused`` without a device"""
    from curobo_amd.backends import rollout as rollout_hip

    m = robot(robot_name)
    return (fused_lds_bytes(robot_name, scene_kind) <= rollout_hip.FUSED_LDS_LIMIT - 64 and m.num_dof <= 64 and m.num_links <= 128
            and m.num_spheres < 4096)


def build_checker(device, robot_name, scene_kind):
    from curobo_amd.collision_checking import RobotCollisionChecker
    from curobo_amd.kinematics import KinematicsCfg
    from curobo_amd.scene import SceneData

    a = scene_arrays(scene_kind)
    scene = None if a is None else SceneData.from_arrays({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}, device)
    return RobotCollisionChecker(KinematicsCfg.from_packaged(robot_name, device=device), scene, 0.0)


@functools.lru_cache(maxsize=None)
def feasible_start(robot_name, scene_kind="none"):
    """a configuration the oracle finds surely feasible: the robot's default one, else the first of a fixed random stream"""
    from curobo_amd.workloads import start_configuration
    from oracle.graph_ref import FEASIBLE, feasible_band

    m = robot(robot_name)
    lo, hi = (np.asarray(v, np.float64) for v in m.joint_limits_position)
    rng = np.random.default_rng(17)
    cand = np.concatenate([start_configuration(m)[None].astype(np.float64), 0.5 * (lo + hi) + 0.3 * (hi - lo) * rng.uniform(-1, 1, (64, m.num_dof))])
    state = feasible_band(cand.astype(np.float32), m, scene_arrays(scene_kind))
    assert (state == FEASIBLE).any(), (robot_name, scene_kind)
    return cand[int(np.argmax(state == FEASIBLE))].astype(np.float32)


# ------------------------------------------------------------------------------------------------ steering batches
def _long_edge(m, max_steps, q0, threshold=THRESHOLD):
    """an edge along joint 0 about the middle of its range with ratio = max_steps - 1.5: ceil(ratio) + 1 = max_steps with the
    ratio half a step from the integers on either side"""
    lo, hi = (np.asarray(v, np.float64) for v in m.joint_limits_position)
    half = 0.5 * (max_steps - 1.5) * threshold
    mid = 0.5 * (lo[0] + hi[0])
    assert mid - half > lo[0] + 0.01 and mid + half < hi[0] - 0.01
    s, t = np.array(q0, np.float64), np.array(q0, np.float64)
    s[0], t[0] = mid - half, mid + half
    return s, t


def _case(robot_name, scene_kind, s, t, threshold=THRESHOLD, **extra):
    m = robot(robot_name)
    return dict(robot=robot_name, scene=scene_kind, start=np.ascontiguousarray(s, np.float32), target=np.ascontiguousarray(t, np.float32),
                weight=np.ones(m.num_dof, np.float32), threshold=threshold, **extra)


@functools.lru_cache(maxsize=None)
def random_edges(robot_name, scene_kind, n, max_steps, seed, zero_share=0.1, leaving_share=0.1, threshold=THRESHOLD):
    """roadmap-like batch: short edges between configurations inside the limits (many of them in collision where there is a scene),
    a share of zero-length edges, a share that leaves the joint limits, and edge 0 = the long edge that sets the step count.
    Every other edge is shorter than the long one."""
    m = robot(robot_name)
    D = m.num_dof
    lo, hi = (np.asarray(v, np.float64) for v in m.joint_limits_position)
    rng = np.random.default_rng(seed)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    s = mid + 0.95 * half * rng.uniform(-1, 1, (n, D))
    reach = (max_steps - 2.0) * threshold  # (ratio <= max_steps - 2 < the long edge's max_steps - 1.5)
    step = rng.uniform(-1, 1, (n, D)) * rng.uniform(0.2, 1.0, (n, 1)) * reach
    t = np.clip(s + step, lo + 0.01 * half, hi - 0.01 * half)
    kind = rng.random(n)
    zero = kind < zero_share
    leaving = (kind >= zero_share) & (kind < zero_share + leaving_share)
    # a start near one limit and a target past it (some start outside already)
    j = rng.integers(0, D, n)
    up = rng.random(n) < 0.5
    for e in np.flatnonzero(leaving):
        d = float(rng.uniform(0.3, 1.0)) * reach
        lim, sg = (hi[j[e]], 1.0) if up[e] else (lo[j[e]], -1.0)
        s[e, j[e]] = lim - sg * float(rng.uniform(-0.1, 0.9)) * d
        t[e] = s[e]
        t[e, j[e]] = s[e, j[e]] + sg * d
    s[0], t[0] = _long_edge(m, max_steps, feasible_start(robot_name, scene_kind), threshold)
    zero[0] = False
    s32, t32 = s.astype(np.float32), t.astype(np.float32)
    t32[zero] = s32[zero]
    return _case(robot_name, scene_kind, s32, t32, threshold=threshold, max_steps=max_steps, zero=zero, leaving=leaving)


#: the robot / scene pairs of ``test_steering_matches_the_oracle`` (every scene kind, every robot; unitree_g1 joins when the fused
#: launch takes it, see ``oracle_cases``)
ORACLE_PAIRS = (("franka", "c2"), ("franka", "primitives"), ("franka", "slots40"), ("franka", "voxels"), ("ur10e", "c3"), ("ur10e", "voxels"),
                ("ur10e", "none"), ("dual_ur10e", "none"), ("dual_ur10e", "c2"), ("dual_ur10e", "slots64"), ("unitree_g1", "none"))


def oracle_pairs():
    return [p for p in ORACLE_PAIRS if fits_fused(*p)]


def oracle_case(robot_name, scene_kind):
    """600 edges at 40 points each (24 k points)"""
    return random_edges(robot_name, scene_kind, 600, 39, seed=11)


PLACED_KSTAR = (0, 1, 15, 16, 17, 31, 32)


@functools.lru_cache(maxsize=None)
def placed_crossings(n_pts):
    """franka without a scene: edge 0 is the long feasible edge that sets ``max_steps = n_pts - 1``; every other edge moves one
    joint (0 or 6: a rotation about the arm's own axis, no other joint moves, so nothing but the limit can end it) across its
    upper or lower limit so that step k* is the first outside, by half a step length (0.02 rad) on either side of the limit.
    Returns the case with ``kstar`` and the expected indices ``expect`` = max(k* - 1, 0) (``max_steps`` for the long edge)."""
    m = robot("franka")
    lo, hi = (np.asarray(v, np.float64) for v in m.joint_limits_position)
    q0 = feasible_start("franka").astype(np.float64)
    ms = n_pts - 1
    d = 0.04  # joint step per point: ratio = 0.8 max_steps, below the long edge's max_steps - 1.5 for max_steps >= 8
    S, T, K = [_long_edge(m, ms, q0)[0]], [_long_edge(m, ms, q0)[1]], [n_pts]
    for kstar in sorted({k for k in PLACED_KSTAR if k <= ms} | {ms}):
        for j in (0, 6):
            for up in (True, False):
                s, t = q0.copy(), q0.copy()
                lim, sg = (hi[j], 1.0) if up else (lo[j], -1.0)
                s[j] = lim - sg * (kstar - 0.5) * d
                t[j] = s[j] + sg * ms * d
                S.append(s), T.append(t), K.append(kstar)
    K = np.asarray(K)
    expect = np.where(K < n_pts, np.maximum(K - 1, 0), ms)
    return _case("franka", "none", np.stack(S), np.stack(T), max_steps=ms, kstar=K, expect=expect)


@functools.lru_cache(maxsize=None)
def zero_length_batch():
    """every edge has t == s (franka, c2 world): starts inside the limits (free or in collision, as the oracle finds them) and
    a few outside the limits.  max_steps == 1; index 1 where the start is feasible, else 0."""
    m = robot("franka")
    lo, hi = (np.asarray(v, np.float64) for v in m.joint_limits_position)
    rng = np.random.default_rng(3)
    s = 0.5 * (lo + hi) + 0.5 * (hi - lo) * 0.9 * rng.uniform(-1, 1, (96, m.num_dof))
    s[::8, 2] = hi[2] + 0.05
    s[1] = feasible_start("franka", "c2")
    return _case("franka", "c2", s, s.copy(), max_steps=1)


def beyond_the_grid():
    """2048 + 37 short edges (max_steps 8) on the c2 world: the workgroups 0 .. 36 walk a second edge"""
    return random_edges("franka", "c2", GRID_CAP + 37, 8, seed=23, zero_share=0.05, leaving_share=0.1)


def row_stride_case():
    return random_edges("franka", "c2", 300, 20, seed=31)


def padded_rows(a, ld):
    """[n, D] -> [n, ld] with NaN in the padding columns"""
    out = np.full((a.shape[0], ld), np.nan, np.float32)
    out[:, :a.shape[1]] = a
    return out


def steering_batches():
    """name -> case, every steering batch of the suite (what the CPU test holds the caps on)"""
    out = {f"oracle/{r}/{s}": oracle_case(r, s) for r, s in oracle_pairs()}
    out.update({f"placed/{n}": placed_crossings(n) for n in (16, 17, 40)})
    out.update({"zero_length": zero_length_batch(), "beyond_the_grid": beyond_the_grid(), "row_stride": row_stride_case()})
    return out


_STEER_REF = {}


def steering_reference(case):
    """dict(steps [n], margin [n], max_steps, band = ``steer_band`` at that count) -- computed once per batch and left unchanged"""
    from oracle.graph_ref import steer_band, steer_num_steps_ref

    key = id(case["start"])
    if key not in _STEER_REF:
        steps, margin = steer_num_steps_ref(case["start"], case["target"], case["weight"], case["threshold"])
        ms = int(steps.max())
        _STEER_REF[key] = dict(steps=steps, margin=margin, max_steps=ms, case=case,
                               band=steer_band(case["start"], case["target"], ms, robot(case["robot"]), scene_arrays(case["scene"])))
    return _STEER_REF[key]


# ------------------------------------------------------------------------------------------------ point mode
POINT_SIZES = (1, 15, 16, 17, 1000, 16 * GRID_CAP + 5)


@functools.lru_cache(maxsize=None)
def point_batch(n):
    """n configurations (franka, c2 world): 85 % inside the limits, the rest pushed past one limit"""
    m = robot("franka")
    lo, hi = (np.asarray(v, np.float64) for v in m.joint_limits_position)
    rng = np.random.default_rng(100 + n)
    q = 0.5 * (lo + hi) + 0.5 * (hi - lo) * 0.95 * rng.uniform(-1, 1, (n, m.num_dof))
    out = np.flatnonzero(rng.random(n) < 0.15)
    j = rng.integers(0, m.num_dof, out.shape[0])
    q[out, j] = np.where(rng.random(out.shape[0]) < 0.5, hi[j] + rng.uniform(0.001, 0.2, out.shape[0]), lo[j] - rng.uniform(0.001, 0.2, out.shape[0]))
    q = q.astype(np.float32)
    if n > 1:
        q[-1] = feasible_start("franka", "c2")  # (the last row of the last, partly filled workgroup)
    return dict(robot="franka", scene="c2", q=q)


@functools.lru_cache(maxsize=None)
def points_reference(n):
    from oracle.graph_ref import feasible_band

    c = point_batch(n)
    return feasible_band(c["q"], robot(c["robot"]), scene_arrays(c["scene"]))


# ------------------------------------------------------------------------------------------------ k-NN sets
KNN_GRID_SHAPES = tuple((N, k, Q) for (N, k, Q) in ((1, 1, 5), (63, 63, 5), (64, 64, 5), (65, 64, 5), (1000, 64, 1), (1000, 64, 5), (1000, 64, 255)))
KNN_DOFS = (1, 7, 12)


def knn_ids():
    return [f"grid-N{N}-k{k}-Q{Q}-D{D}" for (N, k, Q) in KNN_GRID_SHAPES for D in KNN_DOFS] + ["identical", "continuous"]


def grid_knn_set(rng, N, k, Q, D, tail=3):
    """N searched nodes, then Q query rows and ``tail`` more unsearched rows, see ``knn_set``"""
    rows = N + Q + tail
    buf = np.zeros((rows, D + 1), np.float64)
    buf[:, :D] = rng.integers(-512, 513, (rows, D)) / 256.0
    if N >= 4:
        rep = rng.integers(0, N, N // 4)
        buf[rng.integers(0, N, N // 4), :D] = buf[rep, :D]
    buf[N:, :D] = np.clip(buf[N:, :D], -2.0, 2.0 - 1.0 / 256) + 1.0 / 512
    buf[:, D] = np.arange(rows)  # the index column of the planner's node buffer
    w = rng.integers(8, 25, D) / 16.0
    return dict(buffer=buf.astype(np.float32), query_rows=(N, Q), weight=w.astype(np.float32), n_nodes=N, k=k, D=D, exact=True)


@functools.lru_cache(maxsize=None)
def knn_set(name):
    """dict(buffer [rows, D + 1] fp32, query_rows (first row, count) or queries [Q, D], weight [D], n_nodes, k, D, exact).
    grid sets: coordinates on multiples of 2^-8 in [-2, 2], weights on multiples of 2^-4 in [0.5, 1.5] -- every float64 product
    and sum of the distance is exact, so ties are exact ties and the stable order is the only right answer, with or without
    fma contraction.  The queries are rows of the node buffer past the searched prefix (row stride D + 1), half a grid step off
    the grid: closer to themselves than any searched node is, so a search that runs past ``n_nodes`` returns them.  A quarter
    of the searched nodes repeat earlier ones."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name.startswith("grid"):
        N, k, Q, D = (int(p[1:]) for p in name.split("-")[1:])
        return grid_knn_set(rng, N, k, Q, D)
    if name == "identical":
        D = 7
        buf = np.zeros((200, D + 1), np.float32)
        buf[:, :D] = rng.integers(-512, 513, D) / 256.0
        buf[:, D] = np.arange(200)
        return dict(buffer=buf, query_rows=(100, 5), weight=(rng.integers(8, 25, D) / 16.0).astype(np.float32), n_nodes=200, k=64, D=D, exact=True)
    if name == "continuous":  # uniform fp32 values, as tests/test_gpu_graph_planner.py::test_knn_matches_fp64_numpy draws them
        D, N, Q = 7, 1000, 255
        buf = rng.uniform(-2, 2, (N, D + 1)).astype(np.float32)
        return dict(buffer=buf, queries=rng.uniform(-2, 2, (Q, D)).astype(np.float32), weight=rng.uniform(0.5, 1.5, D).astype(np.float32),
                    n_nodes=N, k=64, D=D, exact=False)
    raise ValueError(name)


def knn_queries(c):
    """the queries as an array [Q, >= D] (a view of the buffer's rows for the grid sets)"""
    if "queries" in c:
        return c["queries"]
    r0, Q = c["query_rows"]
    return c["buffer"][r0:r0 + Q]


def knn_reference(c):
    from oracle.graph_ref import knn_ref

    return knn_ref(knn_queries(c), c["buffer"], c["weight"], c["n_nodes"], c["k"])


# ------------------------------------------------------------------------------------------------ device side (GPU test, sweep)
def run_steer(checker, case, ld=None):
    """the steering launch through ``backends.graph.graph_steer`` -> (out_node [n, D + 1], out_index [n], max_steps) as numpy.
    ``ld``: row stride of the start / target buffers (padding columns NaN); default contiguous rows."""
    import torch

    from curobo_amd.backends import graph as graph_hip

    kin = checker.kinematics.kinematics_config
    dev, D = kin.joint_limits_position.device, int(kin.num_dof)
    s, t = case["start"], case["target"]
    if ld is not None:
        s, t = padded_rows(s, ld), padded_rows(t, ld)
    s, t = torch.as_tensor(s, device=dev), torch.as_tensor(t, device=dev)
    n = s.shape[0]
    node = torch.full((n, D + 1), -7.0, device=dev)
    idx = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ws = torch.full((1,), -7, dtype=torch.int32, device=dev)
    graph_hip.graph_steer(node, idx, None, ws, s, t, torch.as_tensor(case["weight"], device=dev), float(case["threshold"]), False, kin,
                          None if checker.scene is None else checker.scene.struct)
    torch.cuda.synchronize()
    return node.cpu().numpy(), idx.cpu().numpy(), int(ws.item())


def run_points(checker, q, ld=None):
    """point mode -> uint8 flags [n] as numpy"""
    import torch

    from curobo_amd.backends import graph as graph_hip

    kin = checker.kinematics.kinematics_config
    dev = kin.joint_limits_position.device
    qt = torch.as_tensor(q if ld is None else padded_rows(q, ld), device=dev)
    out = torch.full((qt.shape[0],), 7, dtype=torch.uint8, device=dev)
    graph_hip.graph_steer(None, None, out, None, qt, None, None, THRESHOLD, True, kin, None if checker.scene is None else checker.scene.struct)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_knn(device, c):
    import torch

    from curobo_amd.backends import graph as graph_hip

    buf = torch.as_tensor(c["buffer"], device=device)
    if "queries" in c:
        q = torch.as_tensor(c["queries"], device=device)
    else:
        r0, Q = c["query_rows"]
        q = buf[r0:r0 + Q]  # rows of the node buffer: ld_q = D + 1
    out = torch.full((q.shape[0], c["k"]), -7, dtype=torch.int32, device=device)
    graph_hip.graph_knn(out, q, buf, torch.as_tensor(c["weight"], device=device), c["n_nodes"], c["D"], c["k"])
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_steer(ref, node, idx, max_steps):
    """the launch's outputs against ``steering_reference``; raises AssertionError.  Returns the undecided share."""
    from oracle.graph_ref import steer_points_fp32

    case, band = ref["case"], ref["band"]
    D = case["weight"].shape[0]
    assert max_steps == ref["max_steps"], f"max_steps {max_steps}, reference {ref['max_steps']}"
    dec = band["decided"]
    share = 1.0 - float(dec.mean())
    assert share <= UNDECIDED_CAP, f"{100 * share:.2f} % of the edges are undecided"
    idx = idx.astype(np.int64)
    off = np.flatnonzero(dec & (idx != band["index"]))
    assert off.size == 0, (f"{off.size} of {int(dec.sum())} decided edges disagree, first {off[:8].tolist()}: launch {idx[off[:8]].tolist()} "
                           f"oracle {band['index'][off[:8]].tolist()}")
    out = np.flatnonzero((idx < band["index_lo"]) | (idx > band["index_hi"]))
    assert out.size == 0, f"{out.size} undecided edges outside the band's span, first {out[:8].tolist()}"
    want = steer_points_fp32(case["start"], case["target"], max_steps, idx)
    err = np.abs(node[:, :D].astype(np.float64) - want)
    assert np.isfinite(node).all() and float(err.max()) <= 1e-6, f"out_node differs from the point formula by {float(err.max()):.3e}"
    assert (node[:, D] == 0).all(), "index column of out_node is not 0"
    return share


def check_points(state, flags):
    from oracle.graph_ref import FEASIBLE, UNDECIDED

    share = float((state == UNDECIDED).mean())
    assert share <= UNDECIDED_CAP, f"{100 * share:.2f} % of the points are undecided"
    assert set(np.unique(flags)) <= {0, 1}, f"flags hold {np.unique(flags).tolist()}"
    ok = state != UNDECIDED
    off = np.flatnonzero(ok & ((flags == 1) != (state == FEASIBLE)))
    assert off.size == 0, f"{off.size} of {int(ok.sum())} decided points disagree, first {off[:8].tolist()}"
    return share


def check_knn(c, got):
    """exact sets: equal to the stable reference.  Continuous values: the index where the reference's key is more than 1e-12
    (relative) from both neighbouring keys of the sorted list, the distance of the returned node elsewhere."""
    order, dist = knn_reference(c)
    assert got.min() >= 0 and got.max() < c["n_nodes"], f"indices outside the searched prefix: {int(got.min())} .. {int(got.max())}"
    if c["exact"]:
        np.testing.assert_array_equal(got, order)
        return
    full = np.sort(dist, axis=1)
    key = full[:, :c["k"]]
    nxt = np.concatenate([full[:, 1:c["k"] + 1], np.full((full.shape[0], max(0, c["k"] + 1 - full.shape[1])), np.inf)], 1)[:, :c["k"]]
    prv = np.concatenate([np.full((full.shape[0], 1), -np.inf), key[:, :-1]], 1)
    clear = (nxt - key > 1e-12 * key) & (key - prv > 1e-12 * key)
    np.testing.assert_array_equal(got[clear], order[clear])
    np.testing.assert_array_equal(np.take_along_axis(dist, got.astype(np.int64), 1)[~clear], key[~clear])
