"""The ray launches of csrc/mapper_raycast.hip, the renderer, the pose refiner and the Mapper's render calls on the device, against
the float64 restatement tests/mapper_raycast_ref.py and the analytic scene.  States, views, references and bounds:
tests/mapper_raycast_cases.py (the bounds' origin: tests/test_oracle_mapper_raycast.py, docs/NOTEBOOK.md)."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mapper_cases as C
import mapper_raycast_cases as RC
import mapper_raycast_ref as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mapper(device, state_name=None):
    """a Mapper over the grid of mapper_cases, the named state of mapper_raycast_cases written straight into its TSDF"""
    from curobo_amd.perception.mapper import Mapper, MapperCfg

    mapper = Mapper(MapperCfg(**C.CFG))
    if state_name is not None:
        sw, w, visible, _ = RC.state(state_name)
        t = mapper.tsdf
        t.block_data.copy_(torch.as_tensor(np.stack([sw, w], -1)))
        t.block_visible.zero_()
        t.block_visible[: len(visible)] = torch.as_tensor(visible.astype(np.uint8))
    return mapper


def _raycast(mapper, K, pos, quat, shape, t_min, t_max, min_weight, accelerated, z_depth=False):
    from curobo_amd.backends import mapper as B

    dev = mapper.tsdf.block_data.device
    n = shape[0] * shape[1]
    out = (torch.full((n, 3), 7.0, device=dev), torch.full((n, 3), 7.0, device=dev), torch.full((n,), 7.0, device=dev),
           torch.full((n,), 7, dtype=torch.uint8, device=dev))  # (not zero: every word must be written)
    t = mapper.tsdf
    B.mapper_raycast(*out, torch.as_tensor(K, device=dev), torch.as_tensor(pos, device=dev), torch.as_tensor(quat, device=dev), t.block_data,
                     t.block_visible, t.params, min_weight, t_min, t_max, shape, accelerated, z_depth)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


@pytest.fixture(scope="module")
def mappers(device):
    return {name: _mapper(device, name) for name in ("integrated", "injected")}


# ---------------------------------------------------------------------------------------------------- 1: render parity
@pytest.mark.parametrize("state,view,accelerated", [(s, v, a) for s in ("integrated", "injected") for v in RC.VIEWS for a in (0, 1)])
def test_render_parity(mappers, state, view, accelerated):
    ref = RC.render_ref(state, view, accelerated)
    K, pos, quat = RC.VIEWS[view]
    mw = RC.state(state)[3]
    out = _raycast(mappers[state], K, pos, quat, (RC.VH, RC.VW), RC.T_MIN, RC.T_MAX, mw, accelerated)
    assert RC.compare_render(*out, ref) == ""
    assert out[3].sum() >= 25
    z = _raycast(mappers[state], K, pos, quat, (RC.VH, RC.VW), RC.T_MIN, RC.T_MAX, mw, accelerated, z_depth=True)
    for a, b in zip(out[:2] + out[3:], z[:2] + z[3:]):
        assert np.array_equal(a, b)
    assert np.allclose(z[2], out[2].astype(np.float64) * ref["ray_cam_z"], rtol=2e-6, atol=0) and (z[2] <= out[2]).all()


# ---------------------------------------------------------------------------------------------------- 2: analytic truth
@pytest.mark.parametrize("accelerated", [False, True])
def test_rendered_range_against_the_exact_scene(device, accelerated):
    """the device's own integration of the three frames, rendered by the renderer from camera 2, which integrated nothing"""
    from curobo_amd.perception.mapper import BlockSparseTSDFRenderer
    from curobo_amd.types import CameraObservation, Pose

    mapper = _mapper(device)
    t = lambda a: torch.as_tensor(a, device=device)  # noqa: E731
    for cams in C.FRAMES:
        depth, K, pos, quat = C.frame(*cams)
        mapper.integrate(CameraObservation(depth_image=t(depth), intrinsics=t(K), pose=Pose(t(pos), t(quat))))
    K, pos, quat, _ = C.camera(2)
    renderer = BlockSparseTSDFRenderer(mapper, use_block_acceleration=accelerated)
    depth, normals, valid = renderer.render(t(K), Pose(t(pos).view(1, 3), t(quat).view(1, 4)), (C.H, C.W))
    exact, keep = RC.camera2_truth()
    keep = keep & ~RC.camera2_ref(int(accelerated))["ambiguous"]
    got, hit = depth.cpu().numpy().reshape(-1).astype(np.float64), valid.cpu().numpy().reshape(-1)
    assert keep.sum() > 600 and hit[keep].all()
    err = np.abs(got - exact)[keep]
    print(f"accelerated {accelerated}: range error max {err.max():.5f} m over {keep.sum()} pixels (bound {2 * RC.ANALYTIC_RANGE_ERROR})")
    assert err.max() <= 2 * RC.ANALYTIC_RANGE_ERROR
    n = normals.cpu().numpy().reshape(-1, 3)[keep]
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5)


# ---------------------------------------------------------------------------------------------------- 3: edges
@pytest.mark.parametrize("accelerated", [0, 1])
def test_edges_render_all_miss(mappers, device, accelerated):
    K, pos, quat = RC.VIEWS["outside"]
    shape = (RC.VH, RC.VW)
    g = RC.grid()
    empty = _mapper(device)
    away = RR.R.look_at(pos, 2 * np.asarray(pos, np.float64), 0.0).astype(np.float32)  # the grid is behind the camera
    for what, out in (("an empty map", _raycast(empty, K, pos, quat, shape, 0.1, 2.0, g.min_weight, accelerated)),
                      ("a camera looking away", _raycast(mappers["integrated"], K, pos, away, shape, 0.1, 2.0, g.min_weight, accelerated)),
                      ("a range that ends before the grid", _raycast(mappers["integrated"], K, pos, quat, shape, 0.1, 0.5, g.min_weight, accelerated)),
                      ("a camera far away", _raycast(mappers["integrated"], K, np.float32([3e9, -2e9, 1e9]), quat, shape, 0.1, 2.0, g.min_weight, accelerated)),
                      ("a pose that is not finite", _raycast(mappers["integrated"], K, np.float32([np.inf, 0, 0]), quat, shape, 0.1, 2.0, g.min_weight, accelerated))):
        for o in out:
            assert not o.any(), what
    assert np.linalg.norm(pos) - 0.5 * np.linalg.norm([1.0, 0.96, 0.4]) > 0.5  # (0.5 m does end before the grid)


@pytest.mark.parametrize("shape", [(1, 1), (13, 17)])
@pytest.mark.parametrize("accelerated", [0, 1])
def test_image_shapes_that_are_no_multiple_of_a_tile(mappers, shape, accelerated):
    K = np.array([[12.0, 0.0, 0.5 * shape[1] - 0.2], [0.0, 12.0, 0.5 * shape[0] + 0.1], [0.0, 0.0, 1.0]], np.float32)
    _, pos, quat = RC.VIEWS["outside"]
    sw, w, visible, mw = RC.state("integrated")
    ref = RR.raycast(RC.grid(), sw, w, visible, K, pos, quat, *shape, 0.1, 2.0, mw, accelerated)
    out = _raycast(mappers["integrated"], K, pos, quat, shape, 0.1, 2.0, mw, accelerated)
    assert RC.compare_render(*out, ref) == ""
    assert out[3].sum() > 0 and ref["mask"].sum() > 0


# ---------------------------------------------------------------------------------------------------- 4: alignment rows
def _align(mapper, pos, quat, n_samples, depth=None):
    from curobo_amd.backends import mapper as B
    from curobo_amd.backends import perception as P

    dev = mapper.tsdf.block_data.device
    depth = RC.align_depth(0) if depth is None else depth
    n = B.ray_align_samples(depth.shape, RC.ALIGN_CFG["stride"], n_samples)
    ws = torch.full((P.pose_sdf_ws_bytes(n) // 4,), 3.0, device=dev)  # (not zero: every row must be written)
    t = mapper.tsdf
    B.mapper_ray_align(ws, torch.as_tensor(depth, device=dev), torch.as_tensor(C.K, device=dev), torch.as_tensor(pos, device=dev),
                       torch.as_tensor(quat, device=dev), t.block_data, t.block_visible, t.params, RC.ALIGN_MIN_WEIGHT, RC.ALIGN_CFG["depth_min"],
                       RC.ALIGN_CFG["depth_max"], RC.ALIGN_CFG["distance_threshold"], RC.ALIGN_CFG["stride"], n_samples)
    torch.cuda.synchronize()
    return ws.cpu().numpy().reshape(-1, 32)


@pytest.mark.parametrize("pose", ["true", "off"])
@pytest.mark.parametrize("n_samples", [1, 5])
def test_alignment_rows(mappers, pose, n_samples):
    pos, quat = RC.align_pose(pose)
    rows = _align(mappers["integrated"], pos, quat, n_samples)
    assert rows.shape[0] == -(-1200 * n_samples // 256) and not rows[:, 29:].any()
    assert RC.compare_rows(rows, RC.align_ref(pose, n_samples)) == ""
    again = _align(mappers["integrated"], pos, quat, n_samples)
    assert np.array_equal(rows.view(np.uint32), again.view(np.uint32)), "two launches are bit-identical"


def test_alignment_of_a_pose_that_is_not_finite(mappers):
    pos, quat = RC.align_pose("true")
    for p, q in ((np.float32([np.nan, 0, 0]), quat), (pos, np.float32([1, np.inf, 0, 0])), (np.full(3, np.nan, np.float32), np.full(4, np.nan, np.float32))):
        rows = _align(mappers["integrated"], p, q, 5)
        assert not rows.view(np.uint32).any(), "count 0 and zero sums"


# ---------------------------------------------------------------------------------------------------- 5: the refiner
def _pose(pos, quat, device):
    from curobo_amd.types import Pose

    return Pose(torch.as_tensor(pos, device=device).view(1, 3), torch.as_tensor(quat, device=device).view(1, 4))


def test_refiner(mappers, device):
    from curobo_amd.perception.mapper import BlockSparseRaycastPoseRefiner, BlockSparseRaycastRefinerCfg

    mapper = mappers["integrated"]
    cfg = BlockSparseRaycastRefinerCfg(**RC.refiner_cfg())
    K = torch.as_tensor(C.K, device=device)
    depth0 = torch.as_tensor(C.camera(0)[3], device=device)  # the image of mapper_cases, through pixel centres
    start = RC.perturbed_pose(0)
    refiner = BlockSparseRaycastPoseRefiner(mapper, cfg)
    pose, final_error, n_iterations = refiner.refine_pose(depth0, K, _pose(*start, device))
    assert n_iterations == cfg.outer_iterations * cfg.inner_iterations == 20
    # the initial error: a refiner that stops after the first evaluation
    _, initial_error, none = BlockSparseRaycastPoseRefiner(mapper, BlockSparseRaycastRefinerCfg(**RC.refiner_cfg(max_iterations=0))).refine_pose(
        depth0, K, _pose(*start, device))
    assert none == 0 and np.isfinite(initial_error) and final_error <= initial_error
    _, pos_true, quat_true, _ = C.camera(0)
    p, q = pose.position.cpu().numpy().reshape(3), pose.quaternion.cpu().numpy().reshape(4)
    d0, d1 = RC.pose_distance(*start, pos_true, quat_true), RC.pose_distance(p, q, pos_true, quat_true)
    rp, rq, ref_final, ref_initial = RC.refiner_ref(0)
    dr = RC.pose_distance(rp, rq, pos_true, quat_true)
    print(f"start {d0[0]:.4f} m {d0[1]:.4f} rad, device {d1[0]:.4f} m {d1[1]:.4f} rad, float64 restatement {dr[0]:.4f} m {dr[1]:.4f} rad; "
          f"error {initial_error:.5f} -> {final_error:.5f} (restatement {ref_initial:.5f} -> {ref_final:.5f})")
    assert d1[0] < d0[0] and d1[1] < d0[1], "nearer the truth than the start, in translation and in angle"
    assert d1[0] <= 2 * dr[0] and d1[1] <= 2 * dr[1]
    assert initial_error == pytest.approx(ref_initial, rel=1e-3)
    # the replayed graph reads the new image and the new pose: camera 1 on the same refiner against a fresh one, bit for bit
    depth1, start1 = torch.as_tensor(C.camera(1)[3], device=device), RC.perturbed_pose(1)
    second = refiner.refine_pose(depth1, K, _pose(*start1, device))
    fresh = BlockSparseRaycastPoseRefiner(mapper, cfg).refine_pose(depth1, K, _pose(*start1, device))
    assert torch.equal(second[0].position, fresh[0].position) and torch.equal(second[0].quaternion, fresh[0].quaternion)
    assert second[1:] == fresh[1:] and not torch.equal(second[0].position, pose.position)
    _, pos1, quat1, _ = C.camera(1)
    e0 = RC.pose_distance(*start1, pos1, quat1)
    e1 = RC.pose_distance(second[0].position.cpu().numpy().reshape(3), second[0].quaternion.cpu().numpy().reshape(4), pos1, quat1)
    r1 = RC.refiner_ref(1)
    er = RC.pose_distance(r1[0], r1[1], pos1, quat1)
    print(f"camera 1: start {e0[0]:.4f} m {e0[1]:.4f} rad, device {e1[0]:.4f} m {e1[1]:.4f} rad, float64 restatement {er[0]:.4f} m {er[1]:.4f} rad")
    assert e1[0] < e0[0] and e1[1] < e0[1] and e1[0] <= 2 * er[0] and e1[1] <= 2 * er[1]
    eager = BlockSparseRaycastPoseRefiner(mapper, cfg, use_graph=False).refine_pose(depth1, K, _pose(*start1, device))
    assert torch.equal(eager[0].position, fresh[0].position) and torch.equal(eager[0].quaternion, fresh[0].quaternion) and eager[1:] == fresh[1:]
    # too few valid depth pixels
    estimate = _pose(*start, device)
    out = refiner.refine_pose(torch.zeros_like(depth0), K, estimate)
    assert out[0] is estimate and out[1] == float("inf") and out[2] == 0


def test_refiner_without_a_valid_sample_reports_inf(device):
    from curobo_amd.perception.mapper import BlockSparseRaycastPoseRefiner, BlockSparseRaycastRefinerCfg

    refiner = BlockSparseRaycastPoseRefiner(_mapper(device), BlockSparseRaycastRefinerCfg(**RC.refiner_cfg(max_iterations=4)))  # an empty map
    start = RC.perturbed_pose(0)
    pose, error, n = refiner.refine_pose(torch.as_tensor(C.camera(0)[3], device=device), torch.as_tensor(C.K, device=device), _pose(*start, device))
    assert error == float("inf") and n == 4
    assert np.array_equal(pose.position.cpu().numpy().reshape(3), start[0]) and np.array_equal(pose.quaternion.cpu().numpy().reshape(4), start[1])


# ---------------------------------------------------------------------------------------------------- 6: the Mapper's calls
def test_mapper_delegation(mappers, device):
    from curobo_amd.perception.mapper import BlockSparseTSDFRenderer

    mapper = mappers["integrated"]
    K, pos, quat, _ = C.camera(2)
    k4 = torch.tensor([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    pose, shape = _pose(pos, quat, device), (C.H, C.W)
    own = BlockSparseTSDFRenderer(mapper).render_depth(torch.as_tensor(K), pose, shape).clone()
    depth = mapper.render_depth(k4, pose, shape)  # [fx, fy, cx, cy], on the host
    assert mapper._get_renderer() is mapper._get_renderer() and mapper._get_renderer().config.use_block_acceleration
    assert torch.equal(depth, own) and tuple(depth.shape) == shape and depth.dtype == torch.float32
    d, normals, valid = mapper.render(torch.as_tensor(K), pose, shape)
    assert torch.equal(d, own) and tuple(normals.shape) == (*shape, 3) and valid.dtype == torch.bool and 1000 < int(valid.sum()) < C.H * C.W
    assert torch.equal(valid, own > 0)
    z = mapper.render_depth(k4, pose, shape, z_depth=True).clone()
    assert (z[valid] < own[valid]).all() and not z[~valid].any()
    _, _, color, v2 = mapper.render_color(k4, pose, shape)
    only = mapper.render_color_only(k4, pose, shape)
    for c in (color, only):
        assert c.dtype == torch.uint8 and tuple(c.shape) == (*shape, 3) and not c.any()
    assert torch.equal(v2, valid)
    shaded, dmap, nmap = mapper.render_shaded(k4, pose, shape), mapper.render_depth_colormap(k4, pose, shape), mapper.render_normal_colormap(k4, pose, shape)
    for img in (shaded, dmap, nmap):
        assert img.dtype == torch.uint8 and tuple(img.shape) == (*shape, 3)
    assert not shaded[~valid].any() and not dmap[~valid].any() and (nmap[~valid] == 128).all()
    assert (shaded[valid] >= 76).all()  # ambient 0.3 of 255 at the least
    with pytest.raises(NotImplementedError, match="colour channel"):
        mapper.render_shaded(k4, pose, shape, use_color=True)


def test_renderer_buffers_grow_and_are_views(mappers, device):
    from curobo_amd.perception.mapper import BlockSparseTSDFRenderer

    r = BlockSparseTSDFRenderer(mappers["integrated"])
    K, pos, quat = RC.VIEWS["outside"]
    pose = _pose(pos, quat, device)
    small = r.render_depth(torch.as_tensor(K), pose, (RC.VH, RC.VW))
    kept = small.clone()
    assert small.data_ptr() == r._hit_depths.data_ptr() and r._buffer_size == RC.VH * RC.VW
    K2, pos2, quat2, _ = C.camera(2)
    big = r.render_depth(torch.as_tensor(K2), _pose(pos2, quat2, device), (C.H, C.W))
    assert r._buffer_size == C.H * C.W and tuple(big.shape) == (C.H, C.W)
    again = r.render_depth(torch.as_tensor(K), pose, (RC.VH, RC.VW))
    assert r._buffer_size == C.H * C.W and torch.equal(again, kept)


# ---------------------------------------------------------------------------------------------------- the randomised sweep
def test_randomised_sweep_of_the_ray_launches():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "randomised", "fuzz_mapper_raycast.py"), "4", "3"], capture_output=True,
                         text=True, timeout=600, cwd=ROOT)
    text = out.stdout + out.stderr
    print(text[-3000:])
    assert out.returncode == 0, text[-2000:]
    assert ", 0 failed" in text, text[-2000:]
