"""The support-polygon kernels (csrc/support_polygon.hip) against the float64 restatement (tests/support_polygon_ref.py), the
autograd function, and the term inside the IK rollout.

Tolerance of the cost kernel.  Not fixed in advance: tests/golden/support_polygon.npz holds what the reference's own code
returns in float32 and in float64 on these inputs; ``g`` is the largest gap between the two, per quantity, over the points of
all four shapes of one mode (pooled: the (1, 1, 3) shape has one point, whose gap alone says nothing), and the kernel must lie
within ``4 g`` of the float64 restatement -- the 4 covers another ``exp`` and FMA contraction, nothing more.  Points whose
smallest edge distance is below 1e-5 are left out of the comparison (the sign may flip between precisions there; the two
points placed exactly on a vertex are such points) and must be finite; they may be at most 1 % of a shape's points.
Measured on the MI355X (weight 2.5; 275 of 277 points compared; the test prints every figure before it asserts):

    quantity                  mode             g (reference fp32)   kernel gap
    signed distance           padded, counts   8.28e-7              8.28e-7  (1.00 g)
    cost, both branches       padded, counts   2.07e-6              2.07e-6  (1.00 g)
    gradient, both branches   padded           9.53e-5              4.97e-5  (0.52 g)
    gradient, both branches   counts           4.52e-5              9.65e-5  (2.13 g)

Hulls: counts equal and every coordinate within 0.50 ulp of the restatement on all nine cases.
"""

import os

import numpy as np
import pytest
import torch

import support_polygon_ref as R
from conftest import load_model, sample_q

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "support_polygon.npz")
SHAPES = {0: (1, 1, 3), 1: (5, 3, 8), 2: (257, 1, 9), 3: (2, 2, 32)}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _ulp_gap(got: np.ndarray, want64: np.ndarray) -> float:
    """largest |got - want| in units of the float32 spacing at want"""
    want32 = want64.astype(np.float32)
    return float((np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(want32)).astype(np.float64)).max())


@pytest.mark.parametrize("name", sorted(R.hull_cases()))
def test_hull_kernel_equals_the_restatement(name, device):
    from curobo_amd.backends import cost as C

    points, padding = R.hull_cases()[name]
    padding = float(np.float32(padding))  # the launch takes the padding as a C float: both sides get that value (0.05 + 7.5e-10)
    want, want_counts = R.hulls_padded(points, padding)
    N, n, _ = points.shape
    hulls, counts = torch.full((N, n, 2), float("nan"), device=device), torch.full((N,), -1, dtype=torch.int32, device=device)
    C.convex_hull_2d(hulls, counts, torch.as_tensor(points, device=device), padding)
    got, got_counts = hulls.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(got_counts, want_counts), name
    assert np.isfinite(got).all()
    full = np.concatenate([want, np.repeat(want[:, -1:], n - want.shape[1], 1)], 1)  # rows past the count repeat the last vertex
    gap = _ulp_gap(got, full)
    print(f"hull {name}: N {N} n {n} counts {got_counts.min()}..{got_counts.max()} gap {gap:.2f} ulp")
    assert gap <= 1.0, name
    if not padding > 0:
        assert np.array_equal(got, full.astype(np.float32))  # unpadded vertices are input points


def _run_cost(device, points, hulls, counts, idxs, weight, icw, mode=0):
    from curobo_amd.backends import cost as C

    B, H, _ = points.shape
    com = torch.zeros(B, H, 4, device=device)
    com[..., :2] = torch.as_tensor(points, device=device)
    com[..., 2], com[..., 3] = 0.7, 30.0  # (height and mass: must not enter)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)  # noqa: E731
    cost, grad, sd = (torch.full(s, float("nan"), device=device) for s in ((B, H), (B, H, 4), (B, H)))
    C.support_polygon_cost(cost, grad, sd, com, t(hulls), None if counts is None else t(counts), t(idxs),
                           torch.tensor([weight], device=device), icw, cost_mode=mode)
    return cost.cpu().numpy(), grad.cpu().numpy(), sd.cpu().numpy()


@pytest.mark.parametrize("mode", ["padded", "counts"])
def test_cost_kernel_within_four_times_the_references_own_float32_gap(mode, golden, device):
    g, W = golden, float(golden["weight"])
    gaps = {}   # quantity -> [reference fp32 gap, kernel gap]
    for k, (B, H, M) in SHAPES.items():
        pts, hulls, idxs = g[f"c{k}_points"], g[f"c{k}_hulls"], g[f"c{k}_idxs"]
        assert pts.shape == (B, H, 2) and hulls.shape[1] == M
        counts = g[f"c{k}_counts"] if mode == "counts" else None
        for i, icw in ((1, 0.001), (0, 0.0)):
            want = R.support_polygon(pts, hulls, idxs, counts, W, icw)
            cost, grad, sd = _run_cost(device, pts, hulls, counts, idxs, W, icw)
            assert np.isfinite(cost).all() and np.isfinite(grad).all() and np.isfinite(sd).all(), (k, i)
            assert np.array_equal(grad[..., 2:], np.zeros((B, H, 2), np.float32))
            keep = want["boundary"] >= 1e-5
            assert (~keep).sum() <= 0.01 * B * H, (k, (~keep).sum())
            # exactly nothing where the reference's cost is flat
            flat = keep & (want["sd"] < (-0.1 - 1e-4 if i == 1 else -1e-4))
            assert (cost[flat] == 0).all() and (grad[flat] == 0).all()
            if k == 2:
                assert (~keep).sum() == 2 and flat.sum() >= 8 and (want["sd"] > 4.0).sum() == 4
            for q, got, w64, ref32 in (("sd", sd, want["sd"], g[f"c{k}_{mode}_sd32"]),
                                       (f"cost{i}", cost, want["cost"], g[f"c{k}_{mode}_cost{i}_32"]),
                                       (f"grad{i}", grad[..., :2], want["grad"], g[f"c{k}_{mode}_grad{i}_32"])):
                # (the golden's float64 rows are the restatement's to 1e-12: test_support_polygon_ref.py)
                e = gaps.setdefault(q, [0.0, 0.0])
                e[0] = max(e[0], float(np.abs(ref32.astype(np.float64) - w64)[keep].max()))
                e[1] = max(e[1], float(np.abs(got.astype(np.float64) - w64)[keep].max()))
    for q, (gref, ghip) in gaps.items():
        print(f"support polygon {mode} {q}: reference fp32 gap g = {gref:.3e}, kernel gap = {ghip:.3e} ({ghip / gref:.2f} g)")
    for q, (gref, ghip) in gaps.items():
        assert ghip <= 4.0 * gref, (mode, q, gref, ghip)


def test_distance_mode_returns_the_signed_distance_and_its_gradient(golden, device):
    g = golden
    pts, hulls, idxs = g["c1_points"], g["c1_hulls"], g["c1_idxs"]
    want = R.support_polygon(pts, hulls, idxs, None, 1.0, 0.0)
    cost, grad, sd = _run_cost(device, pts, hulls, None, idxs, 1.0, 0.0, mode=1)
    assert np.array_equal(cost, sd)
    np.testing.assert_allclose(sd, want["sd"], atol=1e-6)
    gsd = np.stack([[R.signed_distance_point(pts[b, h], hulls[idxs[b]])[1] for h in range(3)] for b in range(5)])
    np.testing.assert_allclose(grad[..., :2], gsd, atol=2e-4)


def test_autograd_returns_the_kernels_gradient(golden, device):
    from curobo_amd.cost import ConvexPolygon2DHelper, CostSupportPolygon, CostSupportPolygonCfg

    g = golden
    B, H = 5, 3
    verts = torch.as_tensor(g["c1_vertices"], device=device)  # 4 sets of 12 points
    S = 20
    spheres = torch.zeros(B, H, S, 4, device=device)
    foot = torch.tensor([3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14], device=device)
    spheres[:, :, foot, :2] = verts[torch.tensor([2, 0, 2, 3, 1], device=device)][:, None]
    com = torch.zeros(B, H, 3, device=device)
    com[..., :2] = torch.as_tensor(g["c1_points"], device=device)
    com.requires_grad_(True)
    cost = CostSupportPolygon(CostSupportPolygonCfg(weight=2.5, foot_sphere_indices=foot), device)
    out = cost.forward(com, spheres)
    assert tuple(out.shape) == (B, H)
    scale = torch.arange(1, B * H + 1, device=device, dtype=torch.float32).view(B, H)
    (out * scale).sum().backward()
    assert torch.equal(com.grad[..., :2], (cost._out_grad * scale.unsqueeze(-1))[..., :2]) and (com.grad[..., 2] == 0).all()
    # the lazily built hulls are the reference's (padding 0.05, one per row) and so is the cost
    hulls = cost._polygon_helper._cached_convex_hulls.cpu().numpy()
    assert hulls.shape == (B, 8, 2) and np.abs(hulls - g["c1_hulls"][g["c1_idxs"]]).max() < 1e-7
    np.testing.assert_allclose(out.detach().cpu().numpy(), g["c1_padded_cost1_64"], atol=1e-6)
    np.testing.assert_allclose(cost.signed_distance.cpu().numpy(), g["c1_padded_sd64"], atol=1e-6)
    # the helper's distance query, differentiable in the points
    helper = ConvexPolygon2DHelper(device)
    helper.build_convex_hull(verts, 0.05)
    assert tuple(helper._cached_convex_hulls.shape) == (4, 8, 2)
    pts = torch.as_tensor(g["c1_points"], device=device).view(B, H, 1, 2).clone().requires_grad_(True)
    sd = helper.compute_point_hull_distance(pts, torch.as_tensor(g["c1_idxs"], device=device))
    assert tuple(sd.shape) == (B, H, 1)
    np.testing.assert_allclose(sd.detach().cpu().numpy()[..., 0], g["c1_padded_sd64"], atol=1e-6)
    sd.sum().backward()
    assert torch.isfinite(pts.grad).all() and float(pts.grad.norm(dim=-1).max()) > 0.5
    two = ConvexPolygon2DHelper(device)
    two.build_convex_hull(verts[:, :2], 0.05)  # fewer than 3 points: kept as they are, as the reference does
    assert torch.equal(two._cached_convex_hulls, verts[:, :2])


# ---------------------------------------------------------------------------------------------------------------- rollout
def _rollout_case(robot, device, B):
    from curobo_amd.robot.kinematics_params import KinematicsParams
    from curobo_amd.scene import SceneData, cuboid_scene_arrays
    from curobo_amd.workloads import c1_world

    model = load_model(robot)
    kin = KinematicsParams.from_model(model, device)
    scene = SceneData.from_arrays(cuboid_scene_arrays(c1_world()), device) if robot == "franka" else None
    T = kin.num_pose_links
    rng = np.random.default_rng(B)
    q = torch.as_tensor(sample_q(model, B, seed=B, scale=0.6), device=device)
    gp = torch.as_tensor(rng.uniform(-0.5, 0.5, (2, T, 1, 3)).astype(np.float32), device=device)
    gq = torch.zeros(2, T, 1, 4, device=device)
    gq[..., 0] = 1.0
    idx = torch.as_tensor(np.arange(B, dtype=np.int32) % 2, device=device)
    return kin, scene, q, gp, gq, idx


def _polygons(rng, centres):
    """one set of 10 points around every centre [P, 2]: quadrilaterals to octagons of ~0.15 m"""
    centres = np.asarray(centres, np.float64).reshape(-1, 2)
    return (centres[:, None] + rng.uniform(-0.15, 0.15, (len(centres), 10, 2))).astype(np.float32)


def _expected_term(ro, verts, idxs, W, icw):
    """the restatement's term on the rollout's own centre-of-mass buffer, pulled back by the FK VJP launch alone"""
    hulls, counts = R.hulls_padded(verts, 0.05)
    want = R.support_polygon(ro.com[..., :2].cpu().numpy(), hulls, idxs, counts, W, icw)
    g = torch.zeros_like(ro.sp_grad)
    g[..., :2] = torch.as_tensor(want["grad"].astype(np.float32), device=g.device)
    keep = ro.grad_q.clone()
    ro._fk_backward(torch.zeros_like(ro.pose_grad_pos), torch.zeros_like(ro.pose_grad_quat), None, None, grad_com=g)
    gq = ro.grad_q.clone().view(ro.batch_size, -1)
    ro.grad_q.copy_(keep)
    return want, gq


@pytest.mark.parametrize("robot", ["franka", "unitree_g1"])
@pytest.mark.parametrize("B", [16, 17])
def test_rollout_adds_the_term_and_its_gradient(robot, B, device):
    from curobo_amd.rollout.ik_rollout import IKRollout, IKRolloutCfg

    kin, scene, q, gp, gq, idx = _rollout_case(robot, device, B)
    W, icw = 5000.0, 0.001
    off = IKRollout(kin, scene, B, IKRolloutCfg(use_fused=False))
    off.update_goals(gp, gq, idx)
    c0, g0 = (t.clone() for t in off.cost_and_gradient(q))
    on = IKRollout(kin, scene, B, IKRolloutCfg(support_polygon_weight=W, support_polygon_inside_cost_weight=icw))
    on.update_goals(gp, gq, idx)
    with pytest.raises(ValueError, match="call update_support_polygon first"):
        on.cost_and_gradient(q)
    on._fk_forward(q, compute_com=True)
    # polygon p around the centre of mass of row p: rows inside and rows outside
    rng = np.random.default_rng(3)
    verts, pidx = _polygons(rng, on.com[:3, 0, :2].cpu().numpy()), (np.arange(B) % 3).astype(np.int32)
    on.update_support_polygon(torch.as_tensor(verts), torch.as_tensor(pidx, device=device))
    c1, g1 = (t.clone() for t in on.cost_and_gradient(q))
    assert float(on.com[:, 0, 3].min()) > 1.0  # the total mass: the forward did compute the centre of mass
    want, gq_term = _expected_term(on, verts, pidx, W, icw)
    inside = want["sd"] < 0
    print(f"{robot} B {B}: {int(inside.sum())} rows inside, term {want['cost'].min():.3g}..{want['cost'].max():.3g}, "
          f"|grad term| max {float(gq_term.abs().max()):.3g}, cost without {float(c0.min()):.3g}..{float(c0.max()):.3g}")
    assert inside.any() and (~inside).any() and float(gq_term.abs().max()) > 1.0
    np.testing.assert_allclose(on.sp_distance.cpu().numpy(), want["sd"], atol=1e-5)
    np.testing.assert_allclose(c1.cpu().numpy(), c0.cpu().numpy() + want["cost"][:, 0], rtol=1e-4, atol=1e-2)
    expect = (g0 + gq_term).cpu().numpy()
    np.testing.assert_allclose(g1.cpu().numpy(), expect, rtol=2e-3, atol=2e-5 * np.abs(expect).max())
    # without the gradient: the same cost
    assert torch.equal(on.evaluate(q.view(B, 1, -1), with_gradient=False), c1)


@pytest.mark.parametrize("robot", ["franka", "unitree_g1"])
def test_weight_zero_is_todays_rollout(robot, device, monkeypatch):
    """the switch off: no new launch is made (the shims raise if called) and the numbers are those of a default rollout, bit
    for bit, on the fused launch and on the kernel sequence"""
    from curobo_amd.backends import cost as C
    from curobo_amd.rollout.ik_rollout import IKRollout, IKRolloutCfg

    B = 17
    kin, scene, q, gp, gq, idx = _rollout_case(robot, device, B)
    outs = {}
    for fused in (True, False):
        ro = IKRollout(kin, scene, B, IKRolloutCfg(use_fused=fused))
        ro.update_goals(gp, gq, idx)
        outs[fused] = [t.clone() for t in ro.cost_and_gradient(q)]

    def never(*a, **k):
        raise AssertionError("a support-polygon launch with the weight at 0")

    for fn in ("support_polygon_cost", "convex_hull_2d", "rollout_point_aggregate_terms"):
        monkeypatch.setattr(C, fn, never)
    for fused in (True, False):
        ro = IKRollout(kin, scene, B, IKRolloutCfg(use_fused=fused, support_polygon_weight=0.0))
        ro.update_goals(gp, gq, idx)
        com_before = ro.com.clone()
        c, g = ro.cost_and_gradient(q)
        assert torch.equal(c, outs[fused][0]) and torch.equal(g, outs[fused][1])
        assert torch.equal(ro.com, com_before) and not hasattr(ro, "sp_cost")  # FK ran without the centre of mass
        with pytest.raises(ValueError, match="support_polygon_weight = 0"):
            ro.update_support_polygon(torch.zeros(1, 4, 2))


def test_captured_graph_follows_a_new_polygon(device):
    from curobo_amd.rollout.ik_rollout import IKRollout, IKRolloutCfg
    from curobo_amd.util.graph_capture import capture_graph

    B = 16
    kin, scene, q, gp, gq, idx = _rollout_case("unitree_g1", device, B)
    cfg = IKRolloutCfg(support_polygon_weight=5000.0)
    ro = IKRollout(kin, scene, B, cfg)
    ro.update_goals(gp, gq, idx)
    ro._fk_forward(q, compute_com=True)
    centre = ro.com[0, 0, :2].cpu().numpy()
    rng = np.random.default_rng(11)
    first, second = _polygons(rng, centre), _polygons(rng, centre + 0.2)[:, :7]  # another place, another point count
    ro.update_support_polygon(torch.as_tensor(first))
    graph, (cost, grad) = capture_graph(lambda: ro.cost_and_gradient(q))
    graph.replay()
    torch.cuda.synchronize()
    fresh = IKRollout(kin, scene, B, cfg)
    fresh.update_goals(gp, gq, idx)
    for verts in (first, second):
        ro.update_support_polygon(torch.as_tensor(verts))
        graph.replay()
        torch.cuda.synchronize()
        fresh.update_support_polygon(torch.as_tensor(verts))
        c, g = fresh.cost_and_gradient(q)
        assert torch.equal(cost, c) and torch.equal(grad, g)
        if verts is first:
            c_first = c.clone()
    assert not torch.equal(c_first, cost)  # the second polygon changed the numbers


# ----------------------------------------------------------------------------------------------------------------- solver
LEFT_FOOT = "left_ankle_roll_link"


def _g1_ik(device, weight, P, stance):
    from curobo_amd.solver.inverse_kinematics import InverseKinematics, InverseKinematicsCfg

    ik = InverseKinematics(InverseKinematicsCfg.create(
        robot="unitree_g1.yml", scene_model=None, num_seeds=16, max_batch_size=P, support_polygon_weight=weight,
        foot_link_names=[LEFT_FOOT]))
    ik.disable_tool_pose_tracking([f for f in ik.tool_frames if "ankle" not in f])  # the hands are free
    if weight:
        ik.update_support_polygon(joint_state=stance)  # one polygon per problem: the left foot's spheres in its stance
    return ik


def test_g1_ik_shifts_the_weight_onto_one_foot(device):
    """Unitree G1, 4 problems x 16 seeds: both ankle frames pinned at their stance poses, the hands free, the polygon the hull of
    the LEFT foot's spheres only.  Without the term the solutions stand between the feet (outside that polygon); with it every
    solution reported successful has its centre of mass over the left foot and the ankles within the thresholds."""
    from curobo_amd.types import GoalToolPose

    P, W = 4, 20000.0
    off = _g1_ik(device, None, P, None)
    rng = np.random.default_rng(4)
    stance = off.default_joint_position.to(device).reshape(1, -1).repeat(P, 1)
    stance[:, 6:] += torch.as_tensor(rng.uniform(-0.03, 0.03, (P, stance.shape[1] - 6)).astype(np.float32), device=device)
    goal = off.compute_kinematics(stance).tool_poses.as_goal()
    assert isinstance(goal, GoalToolPose)
    r_off = off.solve_pose(goal)
    assert r_off.support_polygon_distance is None
    on = _g1_ik(device, W, P, stance)
    r_on = on.solve_pose(goal)
    # the distance of the term-off solutions: the term-on solver's metrics rollout on them (every seed row of a problem alike)
    slv = on._solver(P)
    m = slv.metrics_rollout
    m.evaluate(r_off.solution[:, 0].repeat_interleave(slv.S, 0).view(P * slv.S, 1, -1).contiguous(), with_gradient=False)
    sd_off = m.sp_distance.view(P, slv.S)[:, 0].cpu().numpy()
    ok, sd_on = r_on.success[:, 0].cpu().numpy(), r_on.support_polygon_distance[:, 0].cpu().numpy()
    pe, re = r_on.position_error[:, 0].cpu().numpy(), r_on.rotation_error[:, 0].cpu().numpy()
    print(f"g1 balance: off success {r_off.success[:, 0].tolist()} sd {sd_off.tolist()}; on success {ok.tolist()} sd {sd_on.tolist()} "
          f"pos err {pe.tolist()} rot err {re.tolist()} optimizer ran {r_on.debug_info}")
    assert (sd_off > 0).sum() >= P / 2, "without the term the centre of mass should be off the left foot, else this shows nothing"
    assert (sd_on[ok] <= 0).all()
    assert (pe[ok] < on.config.position_tolerance).all() and (re[ok] < on.config.orientation_tolerance).all()
    assert ok.any(), "at least one problem is solved with the weight on one foot"


def test_randomised_sweep_of_the_support_polygon_kernels():
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "randomised", "fuzz_support_polygon.py"), "6", "5"],
                         capture_output=True, text=True, timeout=300, cwd=root)
    text = out.stdout + out.stderr
    print(text[-3000:])
    assert out.returncode == 0, text[-2000:]
    assert ", 0 failed" in text, text[-2000:]
