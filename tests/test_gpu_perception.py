"""curobo_amd.perception on the GPU against the reference's recorded outputs (tests/golden/perception_golden.npz, made by
make_perception_golden.py from the reference's own Warp kernels and torch functions), and the live voxel update against
scenes built from scratch.

Tolerances: filtered depth relative 1e-5 on pixels valid in both (the project's tolerance for fp32 kernels); valid mask and
robot mask identical except on the pixel sets the golden script stored (decisive comparison within 1e-6 m / 1e-5 m of its
threshold, computed there from the reference's values alone).  The same holds on perception_edges_golden.npz: images wider
than one 64 x 16 tile of the filter, kernel sizes 1 and 31, minimum distance 0, and for the mask 1 and 1023 pixels, no sphere,
more spheres than one pass holds and the batched / shared combinations the first file lacks."""

import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, load_model

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(GOLDEN_DIR, "perception_golden.npz"))
FILTER_CASES = [str(n) for n in G["filter_case_names"]]
SEG_CASES = [str(n) for n in G["seg_case_names"]]
E = np.load(os.path.join(GOLDEN_DIR, "perception_edges_golden.npz"))
EDGE_FILTER_CASES = [str(n) for n in E["filter_case_names"]]
EDGE_SEG_CASES = [str(n) for n in E["seg_case_names"]]


def _filter_from_params(prm, shape, B, device):
    from curobo_amd.perception import FilterDepth

    dmin, dmax, fly, ksize, ss, sd = prm[:6]
    return FilterDepth(shape, dmin, dmax, None if fly < 0 else fly, None if ksize == 0 else int(ksize), ss, sd, device=str(device), num_batch=B)


def _check_filter(g, cases, name, device):
    prm = g["filter_case_params"][cases.index(name)]
    depth = g[f"{name}/depth"]
    B, H, W = depth.shape
    fd = _filter_from_params(prm, (H, W), B, device)
    filtered, valid = fd(torch.as_tensor(depth, device=device))
    torch.cuda.synchronize()
    assert valid.dtype == torch.bool and filtered.data_ptr() == fd._depth_out.data_ptr()
    filtered, valid = filtered.cpu().numpy(), valid.cpu().numpy()
    ref_f, ref_v, excluded = g[f"{name}/filtered"], g[f"{name}/valid"].astype(bool), g[f"{name}/excluded"]
    both = valid & ref_v
    rel = np.abs(filtered[both] - ref_f[both]) / np.abs(ref_f[both])
    print(f"{name}: valid {int(valid.sum())} ref {int(ref_v.sum())} mask mismatches outside the excluded set "
          f"{int((valid != ref_v)[~excluded].sum())} (excluded {int(excluded.sum())}), max rel depth error {rel.max():.3e}")
    assert np.array_equal(valid[~excluded], ref_v[~excluded])
    assert rel.max() <= 1e-5
    assert (filtered[~valid] == 0).all()  # rejected pixels carry depth 0
    # a second call into caller-owned buffers of another batch size (fresh scratch images inside) gives the same image
    out, msk = torch.full((1, H, W), -1.0, device=device), torch.zeros((1, H, W), dtype=torch.uint8, device=device)
    f1, v1 = fd(torch.as_tensor(depth[:1], device=device), out, msk)
    assert f1.data_ptr() == out.data_ptr()
    assert np.array_equal(f1.cpu().numpy()[0], filtered[0]) and np.array_equal(v1.cpu().numpy()[0], valid[0])


@pytest.mark.parametrize("name", FILTER_CASES)
def test_filter_depth_matches_reference(name, device):
    _check_filter(G, FILTER_CASES, name, device)


@pytest.mark.parametrize("name", EDGE_FILTER_CASES)
def test_filter_depth_matches_reference_at_the_edges(name, device):
    """widths 64, 65 and 130 (the x halo reads the neighbouring tile), kernel sizes 1 and 31 (the halo is wider than a tile is
    high), and minimum distance 0 with a separable size: the 0 of a rejected pixel is in range in the two 1-d passes, which
    smooth it like any pixel (the reference returns up to 1.9 cm there, valid 0); the launch returns 0 where valid is 0"""
    _check_filter(E, EDGE_FILTER_CASES, name, device)


class _FixedSpheres:
    """a kinematics stand-in that hands the segmenter a recorded sphere set (the golden's spheres came from the oracle's FK on
    the CPU: bf16 rounding of spheres that differ in the last fp32 bit would not be the recorded arithmetic)"""

    joint_names = None
    base_link = "base"

    def __init__(self, spheres):
        self.spheres = spheres

    def get_active_js(self, js):
        return js

    def compute_kinematics(self, q):
        import types

        return types.SimpleNamespace(robot_spheres=self.spheres.unsqueeze(1))


def _seg_inputs(name, device):
    from curobo_amd.types import CameraObservation, Pose

    im, ki, pi, si = ([i for i in row if i >= 0] for row in G[f"seg/{name}/index"])
    t = lambda k, idx: torch.as_tensor(G[k][idx], device=device)  # noqa: E731
    obs = CameraObservation(depth_image=t("seg/depth", im), intrinsics=t("seg/intrinsics", ki), depth_to_meter=float(G["seg/depth_to_meter"]),
                            pose=Pose(t("seg/cam_position", pi), t("seg/cam_quaternion", pi)))
    return obs, t("seg/spheres", si), im


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", SEG_CASES)
def test_robot_mask_matches_reference(name, mode, graph, device):
    from curobo_amd.perception import RobotSegmenter
    from curobo_amd.types import JointState

    obs, spheres, _ = _seg_inputs(name, device)
    seg = RobotSegmenter(_FixedSpheres(spheres), float(G["seg/distance_threshold"]), use_cuda_graph=graph,
                         ops_dtype=torch.float32 if mode == "fp32" else torch.bfloat16)
    js = JointState.from_position(torch.zeros(spheres.shape[0], 7, device=device))
    for call in range(2 if graph else 1):  # the second call replays the captured graph
        mask, filtered = seg.get_robot_mask(obs, js)
        torch.cuda.synchronize()
        assert mask.dtype == torch.bool and mask.shape == obs.depth_image.shape
        mask, filtered = mask.cpu().numpy(), filtered.cpu().numpy()
        key = f"seg/{name}/{mode}"
        ref_m, ref_f, excluded = G[f"{key}/mask"].astype(bool), G[f"{key}/filtered"], G[f"{key}/excluded"]
        print(f"{key} graph={graph} call {call}: masked {int(mask.sum())} ref {int(ref_m.sum())} mismatches outside the excluded set "
              f"{int((mask != ref_m)[~excluded].sum())} (excluded {int(excluded.sum())})")
        assert np.array_equal(mask[~excluded], ref_m[~excluded])
        assert np.array_equal(filtered[~excluded], ref_f[~excluded])
        assert not mask[obs.depth_image.cpu().numpy() == 0].any()


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("name", EDGE_SEG_CASES)
def test_robot_mask_matches_reference_at_the_edges(name, mode, device):
    """the launch itself on the recorded rays: 1 and 1023 pixels (less than the 1024 of a workgroup), 2049 spheres with enabled
    ones at 0, 2047 and 2048 (the second pass over the sphere table), rays shared with poses and spheres per image and the
    reverse.  No sphere at all: the reference raises (recorded); the launch masks nothing."""
    from curobo_amd.backends import perception as P

    t = lambda k: torch.as_tensor(E[f"{name}/{k}"], device=device)  # noqa: E731
    depth = t("depth")
    m, o = torch.full(depth.shape, 7, dtype=torch.uint8, device=device), torch.full_like(depth, -7.0)
    P.robot_mask(m, o, depth, t("rays"), t("cam_position"), t("cam_quaternion"), t("spheres"), float(E["seg/distance_threshold"]),
                 P.MASK_FP32 if mode == "fp32" else P.MASK_BF16_OPS)
    torch.cuda.synchronize()
    assert set(np.unique(m.cpu().numpy())) <= {0, 1}
    mask, filtered = m.cpu().numpy().astype(bool), o.cpu().numpy()
    if f"{name}/reference_raises" in E:
        assert E[f"{name}/spheres"].shape[1] == 0
        assert not mask.any() and np.array_equal(filtered, E[f"{name}/depth"])
        return
    key = f"{name}/{mode}"
    ref_m, ref_f, excluded = E[f"{key}/mask"].astype(bool), E[f"{key}/filtered"], E[f"{key}/excluded"]
    print(f"{key}: masked {int(mask.sum())} ref {int(ref_m.sum())} mismatches outside the excluded set "
          f"{int((mask != ref_m)[~excluded].sum())} (excluded {int(excluded.sum())})")
    assert np.array_equal(mask[~excluded], ref_m[~excluded])
    assert np.array_equal(filtered[~excluded], ref_f[~excluded])
    assert not mask[E[f"{name}/depth"] == 0].any()


def test_disabled_sphere_masks_nothing_and_enabled_it_would(device):
    """the golden's sphere sets hold one slot with radius -100 lying on the table: it masks nothing, also when the reference's
    formula would (a small negative radius inside the threshold); with a positive radius the same slot masks table pixels"""
    from curobo_amd.backends import perception as P

    obs, spheres, _ = _seg_inputs("b1", device)
    obs.update_projection_rays()
    k = int(G["seg/disabled_sphere"])

    def run(radius):
        s = spheres.clone()
        s[:, k, 3] = radius
        m, o = torch.empty(obs.depth_image.shape, dtype=torch.uint8, device=device), torch.empty_like(obs.depth_image)
        P.robot_mask(m, o, obs.depth_image, obs.projection_rays, obs.pose.position, obs.pose.quaternion, s, 0.05, P.MASK_FP32)
        return m.cpu().numpy().astype(bool)

    ref = G["seg/b1/fp32/mask"].astype(bool)
    assert np.array_equal(run(-100.0), ref) and np.array_equal(run(-0.01), ref)
    on = run(float(G["seg/unmasked_radius"][0]))
    assert (on & ~ref).sum() > 10 and (G["seg/label"][[0]][on & ~ref] == 2).all()


def test_robot_segmenter_with_franka_kinematics_and_graph_replay(device):
    """FK on the GPU: every rendered robot pixel is masked, scene pixels farther than threshold + the largest radius from every
    sphere are not, zero depth never is; a new joint state through the replayed graph gives that state's mask"""
    from curobo_amd.kinematics import Kinematics, KinematicsCfg
    from curobo_amd.perception import RobotSegmenter
    from curobo_amd.types import JointState

    kin = Kinematics(KinematicsCfg.from_packaged("franka", device=device))
    k = int(G["seg/disabled_sphere"])
    kin.kinematics_config.link_spheres[:, k, 3] = -100.0  # the slot the fixture was rendered without
    q = torch.as_tensor(G["seg/q"], device=device)
    label, depth = G["seg/label"], G["seg/depth"]
    results = {}
    for graph in (True, False):
        seg = RobotSegmenter(kin, 0.05, use_cuda_graph=graph, ops_dtype=torch.float32)
        for c in (0, 1, 0):
            obs, _, _ = _seg_inputs("b1" if c == 0 else "b1_second", device)
            if seg.ready:  # another camera through the SAME segmenter: new intrinsics into the rays the graph reads
                seg.update_camera_projection(obs)
            mask, filtered = seg.get_robot_mask(obs, JointState.from_position(q[[c]], kin.joint_names))
            torch.cuda.synchronize()
            mask, filtered = mask.cpu().numpy()[0], filtered.cpu().numpy()[0]
            results.setdefault(c, []).append(mask)
            assert mask[label[c] == 1].all(), "a rendered robot pixel is not masked"
            assert not mask[depth[c] == 0].any()
            far = (label[c] >= 2) & (G[f"seg/{'b1' if c == 0 else 'b1_second'}/fp32/distance"][0] < -(0.05 + 0.2))
            assert far.sum() > 500 and not mask[far].any()
            assert np.array_equal(filtered, np.where(mask, 0.0, depth[c]).astype(np.float32))
    for c, masks in results.items():
        assert all(np.array_equal(m, masks[0]) for m in masks), "graph replay and eager launches disagree"
    assert not np.array_equal(results[0][0], results[1][0])


def _wall_sdf(p):
    q = np.abs(p - np.array([0.5, 0.0, 0.35])) - np.array([0.08, 0.08, 0.35])
    return np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)


def _voxel_arrays(sdf, name="map"):
    from curobo_amd.scene import cuboid_scene_arrays, voxel_grid_from_sdf

    table = {"dims": [2.0, 2.0, 0.2], "pose": [0.0, 0.0, -0.1, 1, 0, 0, 0], "name": "table"}
    grid = voxel_grid_from_sdf(sdf, (32, 32, 48), 0.02, pose7=[0.5, 0.0, 0.45, 1, 0, 0, 0], max_distance=10.0, name=name)
    return {**cuboid_scene_arrays([[table]]), **grid}


@pytest.mark.parametrize("coarse", [True, False])
@pytest.mark.parametrize("how", ["features", "data"])
def test_live_voxel_update_is_bit_identical_to_a_fresh_scene(how, coarse, oracle, device):
    from conftest import sample_q

    from curobo_amd.backends import collision as Cn
    from curobo_amd.scene import SceneData
    from curobo_amd.scene.types import VoxelGrid

    model = load_model("franka")
    empty, wall = _voxel_arrays(lambda p: np.full(len(p), 1.0)), _voxel_arrays(_wall_sdf)
    b, h = 32, 9
    q0, q1 = sample_q(model, b, seed=5, scale=0.7)[:, None], sample_q(model, b, seed=6, scale=0.7)[:, None]
    tt = np.linspace(0, 1, h, dtype=np.float32)[None, :, None]
    sph = oracle.kinematics_forward((q0 * (1 - tt) + q1 * tt).reshape(b * h, -1), model.as_dict(), horizon=h)["robot_spheres"].reshape(b, h, -1, 4)
    S = sph.shape[2]
    sph_t = torch.as_tensor(sph, device=device)

    def run(scene):
        dist, grad = torch.full((b, h, S), 3.0, device=device), torch.full((b, h, S, 4), 3.0, device=device)
        Cn.sphere_obstacle_collision(dist, grad, sph_t, scene.struct, torch.tensor([1.0], device=device), torch.tensor([0.02], device=device),
                                     None, b, h, S, False, 3, True, torch.tensor([0.05], device=device))
        torch.cuda.synchronize()
        return dist.cpu().numpy(), grad.cpu().numpy()

    live = SceneData.from_arrays(empty, device, coarse_culling=coarse)
    before = run(live)
    ptrs = (live.struct.voxel_features, live.struct.voxel_coarse_min, live.struct.voxel_params, live.struct.voxel_inv_pose)
    if how == "features":
        live.update_voxel_features("map", torch.as_tensor(wall["voxel_features"], device=device).reshape(32, 32, 48))
    else:
        live.update_voxel_data(VoxelGrid(name="map", pose=[0.5, 0.0, 0.45, 1, 0, 0, 0], dims=[0.64, 0.64, 0.96], voxel_size=0.02,
                                         feature_tensor=torch.as_tensor(wall["voxel_features"]).reshape(-1)))
    after = run(live)
    fresh = run(SceneData.from_arrays(wall, device, coarse_culling=coarse))
    assert ptrs == (live.struct.voxel_features, live.struct.voxel_coarse_min, live.struct.voxel_params, live.struct.voxel_inv_pose)
    assert (fresh[0] > before[0]).mean() > 0.002, "the wall must change the cost of these trajectories"
    assert np.array_equal(after[0], fresh[0]) and np.array_equal(after[1], fresh[1])


def test_solver_captured_on_an_empty_grid_sees_the_wall(oracle, device):
    """a TrajOptSolver whose optimiser graphs were captured against an empty grid, the grid then updated in place to hold a pillar
    between start and goal: the next solve equals that of a new solver built on the pillar grid (same success flags,
    trajectories within the solver tests' 1e-4), and differs from the solve through the empty grid"""
    from curobo_amd.robot.kinematics_params import KinematicsParams
    from curobo_amd.scene import SceneData
    from curobo_amd.solver import TrajOptSolver, TrajOptSolverCfg

    model = load_model("franka")
    kin = KinematicsParams.from_model(model, device)
    start = np.array([-0.9, 0.3, 0.0, -1.9, 0.0, 2.2, 0.8], np.float32)
    goals = np.stack([start, start]).copy()
    goals[0, 0], goals[1, 0] = 0.9, 0.7
    fk = oracle.kinematics_forward(goals, model.as_dict())
    gp, gq = torch.as_tensor(fk["link_pos"][:, 0]), torch.as_tensor(fk["link_quat"][:, 0])
    empty, wall = _voxel_arrays(lambda p: np.full(len(p), 1.0)), _voxel_arrays(_wall_sdf)
    cfg = dict(num_seeds=4, num_ik_goals=4)
    live_scene = SceneData.from_arrays(empty, device)
    live = TrajOptSolver(kin, live_scene, 2, TrajOptSolverCfg(**cfg))
    r_empty = live.solve_pose(torch.as_tensor(start), gp, gq)
    torch.cuda.synchronize()
    p_empty = r_empty.position.cpu().numpy().copy()
    live_scene.update_voxel_features("map", wall["voxel_features"].reshape(-1))
    live.reset_seed()  # the seed samplers advance with every solve: both solvers draw their first solve's seeds
    r_live = live.solve_pose(torch.as_tensor(start), gp, gq)
    torch.cuda.synchronize()
    fresh = TrajOptSolver(KinematicsParams.from_model(model, device), SceneData.from_arrays(wall, device), 2, TrajOptSolverCfg(**cfg))
    r_fresh = fresh.solve_pose(torch.as_tensor(start), gp, gq)
    torch.cuda.synchronize()
    s_live, s_fresh = r_live.success.cpu().numpy(), r_fresh.success.cpu().numpy()
    p_live, p_fresh = r_live.position.cpu().numpy(), r_fresh.position.cpu().numpy()
    print("success empty / live / fresh", r_empty.success.cpu().numpy(), s_live, s_fresh, "max |live - fresh|", np.abs(p_live - p_fresh).max(),
          "max |live - empty|", np.abs(p_live - p_empty).max())
    assert r_empty.success.cpu().numpy().all()
    assert np.array_equal(s_live, s_fresh)
    np.testing.assert_allclose(p_live, p_fresh, atol=1e-4)
    assert np.abs(p_live - p_empty).max() > 0.05, "the pillar must change the plan"
    ok = s_live.astype(bool)
    assert ok.any()
    H = p_live.shape[1]
    sph = oracle.kinematics_forward(p_live[ok].reshape(-1, 7), model.as_dict(), horizon=H)["robot_spheres"].reshape(int(ok.sum()), H, -1, 4)
    assert (oracle.scene_collision(sph, wall, 1.0, 0.0)["distance"].sum((1, 2)) == 0).all()
    through = oracle.kinematics_forward(p_empty.reshape(-1, 7), model.as_dict(), horizon=H)["robot_spheres"].reshape(2, H, -1, 4)
    assert oracle.scene_collision(through, wall, 1.0, 0.0)["distance"].sum() > 0, "the plan through the empty grid must hit the pillar"


def test_depth_to_voxel_front_end(device):
    """rendered depth -> FilterDepth -> RobotSegmenter -> back-projection: no surviving point lies within the threshold of a
    robot sphere (up to the 1e-5 m rounding band of the mask test), and at least 95 % of the table / box pixels farther than
    the threshold from the robot survive (the golden script checked both on the reference's output)"""
    from curobo_amd.kinematics import Kinematics, KinematicsCfg
    from curobo_amd.perception import FilterDepth, RobotSegmenter
    from curobo_amd.types import CameraObservation, JointState, Pose

    kin = Kinematics(KinematicsCfg.from_packaged("franka", device=device))
    kin.kinematics_config.link_spheres[:, int(G["seg/disabled_sphere"]), 3] = -100.0
    depth = torch.as_tensor(G["pipe/depth"], device=device)
    prm = G["pipe/filter_params"]
    fd = FilterDepth(tuple(depth.shape[1:]), prm[0], prm[1], prm[2], int(prm[3]), prm[4], prm[5], device=str(device))
    clean, valid = fd(depth)
    obs = CameraObservation(depth_image=clean, intrinsics=torch.as_tensor(G["seg/intrinsics"][[0]], device=device), depth_to_meter=1.0,
                            pose=Pose(torch.as_tensor(G["seg/cam_position"][[0]], device=device), torch.as_tensor(G["seg/cam_quaternion"][[0]], device=device)))
    seg = RobotSegmenter(kin, 0.05, use_cuda_graph=True, ops_dtype=torch.float32)
    q = torch.as_tensor(G["seg/q"][[0]], device=device)
    mask, rest = seg.get_robot_mask(obs, JointState.from_position(q, kin.joint_names))
    torch.cuda.synchronize()
    obs.depth_image = rest
    points = obs.get_pointcloud(project_to_pose=True)[0].double().cpu().numpy()
    keep = rest[0].reshape(-1).cpu().numpy() > 0
    spheres = kin.compute_kinematics(q).robot_spheres.reshape(-1, 4).double().cpu().numpy()
    spheres = spheres[spheres[:, 3] >= 0]
    d = np.linalg.norm(points[keep, None, :] - spheres[None, :, :3], axis=-1) - spheres[None, :, 3]
    kept = keep.reshape(G["pipe/far_scene"].shape)[G["pipe/far_scene"]].mean()
    print(f"front end: {int(keep.sum())} surviving pixels, closest to a sphere {d.min():.6f} m, far scene pixels kept {kept:.4f} "
          f"(reference {float(G['pipe/kept_fraction']):.4f})")
    assert d.min() >= 0.05 - 1e-5
    assert kept >= 0.95
