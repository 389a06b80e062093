"""PRM graph planner host logic (no GPU): shortest paths, the ellipsoid transform, the steering rules, shortcut pruning,
the built-in settings and the opt-in switch of MotionPlannerCfg."""

import math
import os

import numpy as np
import pytest
import torch

from curobo_amd.graph_planner import PRMGraphPlanner, PRMGraphPlannerCfg, RoadmapGraph
from curobo_amd.graph_planner.prm import (last_feasible_index, linear_interpolate_waypoints, steer_num_steps, steer_points,
                                          transform_unit_ball_to_ellipsoid_householder)

EDGES = [(0, 1, 1.0), (1, 2, 1.0), (0, 2, 2.5), (2, 3, 1.0), (1, 3, 3.0), (4, 5, 1.0), (3, 6, 0.5), (0, 6, 4.0)]


def test_dijkstra_on_hand_built_graphs():
    g = RoadmapGraph()
    g.add_edges(EDGES)
    assert g.num_edges == len(EDGES)
    assert g.shortest_path(0, 3) == ([0, 1, 2, 3], 3.0)
    assert g.shortest_path(0, 6) == ([0, 1, 2, 3, 6], 3.5)
    assert g.shortest_path(3, 0) == ([3, 2, 1, 0], 3.0)
    assert g.shortest_path(0, 0) == ([0], 0.0)
    p, d = g.shortest_path(0, 5)
    assert p is None and math.isinf(d)
    assert g.path_exists(4, 5) and not g.path_exists(0, 4) and not g.path_exists(0, 99)
    g.add_edges([(0, 3, 0.5)])  # a new edge updates the search
    assert g.shortest_path(0, 6) == ([0, 3, 6], 1.0)
    g.reset()
    assert g.num_edges == 0 and not g.path_exists(0, 3)


def test_dijkstra_against_networkx():
    nx = pytest.importorskip("networkx")
    rng = np.random.default_rng(3)
    g, ref = RoadmapGraph(), nx.Graph()
    edges = [(int(a), int(b), float(w)) for a, b, w in zip(rng.integers(0, 60, 300), rng.integers(0, 60, 300), rng.uniform(0.1, 2, 300))
             if a != b]
    g.add_edges(edges)
    ref.add_weighted_edges_from(edges)
    for s, t in zip(rng.integers(0, 60, 40), rng.integers(0, 60, 40)):
        s, t = int(s), int(t)
        p, d = g.shortest_path(s, t)
        if not (ref.has_node(s) and ref.has_node(t) and nx.has_path(ref, s, t)):
            assert p is None
            continue
        assert d == pytest.approx(nx.shortest_path_length(ref, s, t, weight="weight"), rel=1e-12)
        assert p[0] == s and p[-1] == t and sum(ref[a][b]["weight"] for a, b in zip(p[:-1], p[1:])) == pytest.approx(d, rel=1e-12)


def test_householder_ellipsoid_keeps_samples_inside():
    torch.manual_seed(0)
    D = 7
    xs, xg = torch.rand(D) - 0.5, torch.rand(D) + 0.5
    w = torch.rand(D) + 0.5
    c_min = float(torch.norm((xg - xs) * w))
    c_max = 1.3 * c_min
    ball = torch.randn(500, D)
    ball = ball / torch.norm(ball, dim=-1, keepdim=True) * torch.rand(500, 1)
    big = torch.full((D,), 1e9)
    x = transform_unit_ball_to_ellipsoid_householder(xs, xg, w, torch.tensor(c_max), ball, -big, big, clamp=False)
    # back to the ellipsoid's frame: the reflection is its own inverse
    d = (xg - xs) / c_min
    e1 = torch.zeros(D)
    e1[0] = 1
    v = d - e1 if d[0] >= 0 else d + e1
    v = v / torch.norm(v)
    H = torch.eye(D) - 2 * torch.outer(v, v)
    y = ((x - (xs + xg) / 2) * w) @ H
    scale = torch.tensor([c_max / 2] + [(c_max ** 2 - c_min ** 2) / 2] * (D - 1))
    r = torch.norm(y / scale, dim=-1)
    assert float(r.max()) <= 1.0 + 1e-5
    torch.testing.assert_close(r, torch.norm(ball, dim=-1), atol=1e-5, rtol=1e-5)
    lo, hi = xs - 0.1, xg + 0.1
    xc = transform_unit_ball_to_ellipsoid_householder(xs, xg, w, torch.tensor(c_max), ball, lo, hi)
    assert bool(((xc >= lo) & (xc <= hi)).all())


def test_step_count_and_batch_wide_interpolation():
    s = torch.tensor([[0.0, 0.0], [0.0, 0.0], [1.0, 1.0]])
    t = torch.tensor([[0.012, -0.001], [0.0, 0.0], [1.0, 1.125]])
    w = torch.tensor([1.0, 2.0])
    n = steer_num_steps(s, t, w, 0.005)
    assert n.tolist() == [4.0, 1.0, 51.0]  # ceil(0.012 / 0.005) + 1, a zero-length edge, ceil(0.25 / 0.005) + 1
    ms = int(n.max())
    pts = steer_points(s, t, ms)
    assert pts.shape == (3, ms + 1, 2)
    # every edge at the batch-wide count: coefficient k / max_steps, first point the start, last the target
    torch.testing.assert_close(pts[0, 1], s[0] + (1.0 / ms) * (t[0] - s[0]))
    torch.testing.assert_close(pts[:, 0], s)
    torch.testing.assert_close(pts[:, -1], t)
    assert bool((pts[1] == 0).all())


def test_last_feasible_index_rule():
    T, F = True, False
    mask = torch.tensor([[T, T, T, T, T],   # none infeasible: the end point
                         [F, T, T, T, T],   # first infeasible: clamped to 0
                         [T, T, F, T, T],   # the point before the first infeasible one
                         [T, F, F, F, F],
                         [T, T, T, T, F],
                         [F, F, F, F, F]])
    assert last_feasible_index(mask).tolist() == [4, 0, 1, 0, 3, 0]


def test_shortcut_pruning_edge_set():
    assert PRMGraphPlanner.shortcut_edge_pairs([[1, 2, 3]]) == [(1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]
    pairs = PRMGraphPlanner.shortcut_edge_pairs([[4, 5], [7, 8, 9, 10]])
    assert len(pairs) == 3 + 10  # n (n + 1) / 2 per path (search/path_pruner.py:94-147)
    assert (4, 5) in pairs and (7, 10) in pairs and (10, 7) not in pairs


def test_linear_waypoint_interpolation():
    wp = np.array([[0.0, 0.0], [1.0, 2.0], [3.0, 2.0]], np.float32)
    out = linear_interpolate_waypoints(wp, 5)
    np.testing.assert_allclose(out, [[0, 0], [0.5, 1], [1, 2], [2, 2], [3, 2]], atol=1e-6)
    np.testing.assert_allclose(linear_interpolate_waypoints(wp[:2], 3), [[0, 0], [0.5, 1], [1, 2]], atol=1e-6)


YAML = "/root/reference/curobo/content/configs/task/graph_planner/exact_graph_planner.yml"


@pytest.mark.skipif(not os.path.isfile(YAML), reason="the reference's task settings are not on this machine")
def test_builtin_settings_equal_the_reference_yaml():
    import yaml

    ref = yaml.safe_load(open(YAML))["graph_planner"]
    cfg = PRMGraphPlannerCfg()
    assert sorted(ref) == sorted(PRMGraphPlannerCfg.yaml_keys())
    for k, v in ref.items():
        assert getattr(cfg, k) == v, k


def test_motion_planner_cfg_builds_no_graph_planner_without_the_switch(monkeypatch):
    from curobo_amd import motion_planner as mp

    class _To:
        scene = None

    monkeypatch.setattr(mp.TrajectoryOptimizerCfg, "create", staticmethod(lambda *a, **k: _To()))
    assert mp.MotionPlannerCfg.create("franka.yml").graph_planner_config is None
    # the graph-planner arguments are no longer swallowed: the switch builds the settings
    assert isinstance(mp.MotionPlannerCfg.create("franka.yml", use_graph_planner=True).graph_planner_config, PRMGraphPlannerCfg)
    custom = PRMGraphPlannerCfg(max_nodes=500)
    assert mp.MotionPlannerCfg.create("franka.yml", use_graph_planner=True, graph_planner_config=custom).graph_planner_config is custom
    # multi-environment planners get none (the reference's graph planner is single-environment)
    monkeypatch.setattr(_To, "scene", type("S", (), {"num_envs": 2})())
    assert mp.MotionPlannerCfg.create("franka.yml", use_graph_planner=True, multi_env=True, max_batch_size=2).graph_planner_config is None
