"""float64 oracle of the two PRM graph-planner launches (``csrc/graph_planner.hip``), TEST INFRASTRUCTURE ONLY: NumPy for the
rules, the C oracle (``oracle/oracle.py``: FK, self collision, scene collision) for what a configuration costs.

k-NN       reference ``DistanceNeighborCalculator.jit_find_nearest_neighbors`` (graph_planner/graph/node_distance.py:128-155):
           distances over weighted configurations, then a stable top-k, smallest first.
steering   reference ``LinearConnector.steer_until_infeasible`` (graph_planner/graph/connector_linear.py:75-192): the batch-wide
           step count ``ceil(max |w (t - s)| / threshold) + 1`` (:132-136), the points ``s + (k / max_steps) (t - s)`` (:138-147)
           and the point before the first infeasible one, clamped to 0 (:151-180).

Feasibility is a sign decision (cost exactly zero or not) that fp32 FK on the device and here cannot agree on for a sphere that
just touches.  The oracle therefore answers in a band: every configuration is evaluated twice, with every enabled sphere
grown and shrunk by ``EPS``, and is *surely feasible*, *surely infeasible* or *undecided*; the device is held exactly on the first
two.  How many configurations may be undecided is capped by the tests from this side alone, before the device is looked at."""

from __future__ import annotations

from typing import Dict, Optional

import numpy as np

#: sphere-radius band [m].  Not a free number: the project holds FK positions (and with them sphere centres) to 1e-5 m
#: (tests/test_gpu_kernels.py::test_fk_forward); a pair distance involves two centres, hence twice that.
EPS = 2e-5
#: joint-limit band [rad]: a few fp32 ulps at joint values of a few radians (ulp(4) = 4.8e-7) -- the device interpolates the
#: point in fp32, the oracle in float64.
EPS_Q = 1e-6

FEASIBLE, UNDECIDED, INFEASIBLE = 1, 0, -1
_CHUNK = 16384


# ------------------------------------------------------------------------------------------------ k-NN
def knn_distances(queries, nodes, weight, n_nodes):
    """[Q, n_nodes] float64 squared weighted distances of the first ``len(weight)`` columns"""
    w = np.asarray(weight, np.float64)
    D = w.shape[0]
    q, x = np.asarray(queries)[:, :D].astype(np.float64), np.asarray(nodes)[:n_nodes, :D].astype(np.float64)
    return (((x[None] - q[:, None]) * w) ** 2).sum(-1)


def knn_ref(queries, nodes, weight, n_nodes, k):
    """indices [Q, k] (int64) of the k nearest of the first ``n_nodes`` rows of ``nodes`` to every query row: float64 squared
    weighted distance, stable argsort (equal keys keep the lower index first), first k.  Also returns the distances [Q, n_nodes]."""
    dist = knn_distances(queries, nodes, weight, n_nodes)
    return np.argsort(dist, axis=1, kind="stable")[:, :k], dist


# ------------------------------------------------------------------------------------------------ steering rules
def steer_num_steps_ref(start, target, weight, threshold):
    """per edge: ``ceil(max |w (t - s)| / threshold) + 1`` in float64 from the fp32 inputs (the threshold as the fp32 number the
    launch receives), and the distance of ``ratio = max |w (t - s)| / threshold`` from the nearest integer: an edge whose
    ratio is well away from an integer has the same count in fp32 and in float64"""
    w = np.asarray(weight, np.float32).astype(np.float64)
    D = w.shape[0]
    s, t = np.asarray(start, np.float32)[:, :D].astype(np.float64), np.asarray(target, np.float32)[:, :D].astype(np.float64)
    ratio = np.abs((t - s) * w).max(-1) / float(np.float32(threshold))
    return (np.ceil(ratio) + 1).astype(np.int64), np.abs(ratio - np.rint(ratio))


def steer_points_ref(start, target, max_steps):
    """[n, max_steps + 1, D] float64: ``s + (k / max_steps) (t - s)``"""
    s, t = np.asarray(start, np.float32).astype(np.float64), np.asarray(target, np.float32).astype(np.float64)
    coeff = np.arange(max_steps + 1, dtype=np.float64) / float(max_steps)
    return s[:, None] + coeff[None, :, None] * (t - s)[:, None]


def steer_points_fp32(start, target, max_steps, index=None):
    """the same points with every operation rounded to fp32 on its own (what the launch and torch compute); ``index`` [n]: only
    the point of that step of every edge, [n, D]"""
    s, t = np.asarray(start, np.float32), np.asarray(target, np.float32)
    k = np.arange(max_steps + 1, dtype=np.float32)[None, :, None] if index is None else np.asarray(index).astype(np.float32)[:, None]
    coeff = (k / np.float32(max_steps)).astype(np.float32)
    if index is None:
        return (s[:, None] + (coeff * (t - s)[:, None]).astype(np.float32)).astype(np.float32)
    return (s + (coeff * (t - s)).astype(np.float32)).astype(np.float32)


def index_from_first_bad(first, n_pts):
    """first infeasible step (``n_pts`` = none) -> the step before it clamped to 0, the last step when there is none"""
    first = np.asarray(first, np.int64)
    return np.where(first < n_pts, np.maximum(first - 1, 0), n_pts - 1)


def last_feasible_index_ref(mask):
    """mask [n, n_pts] (True = feasible) -> [n] (connector_linear.py:151-180)"""
    mask = np.asarray(mask, bool)
    n_pts = mask.shape[1]
    first = np.where((~mask).any(1), (~mask).argmax(1), n_pts)
    return index_from_first_bad(first, n_pts)


# ------------------------------------------------------------------------------------------------ feasibility band
def _cost(oracle, q32, md, padding, pairs, scene_arrays):
    out = np.zeros(q32.shape[0], np.float64)
    for i in range(0, q32.shape[0], _CHUNK):
        sph = oracle.kinematics_forward(q32[i:i + _CHUNK], md)["robot_spheres"]
        c = np.zeros(sph.shape[0], np.float64)
        if pairs is not None and np.asarray(pairs).size > 0:
            c += oracle.self_collision(sph, padding, pairs, 1.0, write_grad=False)["distance"]
        if scene_arrays is not None:
            c += oracle.scene_collision(sph[:, None], scene_arrays, 1.0, 0.0)["distance"].sum((1, 2))
        out[i:i + _CHUNK] = c
    return out


def feasible_band(q, model, scene_arrays: Optional[Dict] = None, eps: float = EPS, eps_q: float = EPS_Q, oracle=None):
    """q [n, D] (float64 or fp32; cast to fp32 for the oracle's FK) -> int8 [n]: FEASIBLE (zero self + scene cost, weights 1 and
    activation distance 0, with every positive sphere radius grown by ``eps``, and every joint inside its limits by ``eps_q``),
    INFEASIBLE (non-zero cost with the radii shrunk by ``eps``, or a joint outside its limits by ``eps_q``) or UNDECIDED.
    Spheres of radius <= 0 are disabled and stay as they are."""
    if oracle is None:
        from oracle import load_oracle

        oracle = load_oracle()
    q = np.asarray(q)
    q64, q32 = q.astype(np.float64), np.ascontiguousarray(q, np.float32)
    md = dict(model.as_dict())
    base = np.asarray(md["link_spheres"], np.float32)
    cost = []
    for sign in (1.0, -1.0):
        sph = base.copy()
        on = base[..., 3] > 0
        sph[..., 3][on] = (base[..., 3][on].astype(np.float64) + sign * eps).astype(np.float32)
        md["link_spheres"] = sph
        cost.append(_cost(oracle, q32, md, model.sphere_padding, model.collision_pairs, scene_arrays))
    lo, hi = (np.asarray(v, np.float64) for v in model.joint_limits_position)
    inside = ((q64 >= lo + eps_q) & (q64 <= hi - eps_q)).all(-1)
    outside = ((q64 < lo - eps_q) | (q64 > hi + eps_q)).any(-1)
    state = np.full(q.shape[0], UNDECIDED, np.int8)
    state[(cost[0] == 0) & inside] = FEASIBLE
    state[(cost[1] > 0) | outside] = INFEASIBLE
    return state


def steer_band(start, target, max_steps, model, scene_arrays: Optional[Dict] = None, eps: float = EPS, eps_q: float = EPS_Q,
               oracle=None):
    """every point ``s + (k / max_steps)(t - s)``, k = 0 .. max_steps, interpolated in float64 and classified by ``feasible_band``.
    Returns a dictionary: ``state`` [n, max_steps + 1]; ``index`` [n] the expected last-feasible step; ``decided`` [n]: no
    point up to and including the edge's first surely-infeasible one is undecided (without an infeasible point: no point
    at all); ``index_lo`` / ``index_hi`` [n]: the steps the band allows (equal to ``index`` on decided edges -- the first
    infeasible step lies between the first point that is not surely feasible and the first surely infeasible one)."""
    n_pts = int(max_steps) + 1
    D = int(model.num_dof)
    pts = steer_points_ref(np.asarray(start)[:, :D], np.asarray(target)[:, :D], max_steps)
    n = pts.shape[0]
    state = feasible_band(pts.reshape(n * n_pts, D), model, scene_arrays, eps, eps_q, oracle).reshape(n, n_pts)
    not_sure = state != FEASIBLE
    bad = state == INFEASIBLE
    first_not_sure = np.where(not_sure.any(1), not_sure.argmax(1), n_pts)
    first_bad = np.where(bad.any(1), bad.argmax(1), n_pts)
    return {"state": state, "decided": first_not_sure == first_bad, "index": index_from_first_bad(first_bad, n_pts),
            "index_lo": index_from_first_bad(first_not_sure, n_pts), "index_hi": index_from_first_bad(first_bad, n_pts)}
