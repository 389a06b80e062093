"""curobo_amd.perception on the host: the C entry points validate before any launch, FilterDepth / RobotSegmenter /
CameraObservation bookkeeping, the projection helpers against the reference's recorded values
(tests/golden/perception_golden.npz, made by make_perception_golden.py), and the live voxel update's error paths."""

import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

from curobo_amd import _lib

G = np.load(os.path.join(GOLDEN_DIR, "perception_golden.npz"))
F32, U8 = torch.float32, torch.uint8


def test_symbols_declared_exported_and_abi_unchanged():
    lib = _lib.load()
    for n in ("curobo_hip_filter_depth", "curobo_hip_robot_mask"):
        assert n in _lib.declared_symbols() and hasattr(lib, n)
        assert n in _lib._signatures()
    assert lib.curobo_hip_abi_version() == 7


def test_facade_modules_export_the_perception_names():
    """curobo/perception.py and curobo/types.py, loaded by path (other tests of the suite put the reference's ``curobo`` in sys.modules)"""
    import importlib.util

    from conftest import ROOT

    def load(rel):
        spec = importlib.util.spec_from_file_location("_facade_" + rel.replace("/", "_").replace(".py", ""), os.path.join(ROOT, rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    from curobo_amd.perception import FilterDepth, RobotSegmenter
    from curobo_amd.types import CameraObservation

    per = load("curobo/perception.py")
    assert per.__all__ == ["FilterDepth", "RobotSegmenter"] and per.FilterDepth is FilterDepth and per.RobotSegmenter is RobotSegmenter
    assert not hasattr(per, "Mapper")
    assert load("curobo/types.py").CameraObservation is CameraObservation


def test_filter_depth_arguments_are_validated_without_a_gpu():
    lib = _lib.load()
    d, o, t1, t2 = (torch.zeros(1, 8, 8) for _ in range(4))
    m = torch.zeros(1, 8, 8, dtype=U8)
    p = lambda t: t.data_ptr()  # noqa: E731
    call = lambda *a: lib.curobo_hip_filter_depth(*a, None)  # noqa: E731
    tail = (0.1, 10.0, 1, 0.02)
    assert call(p(o), p(m), p(d), None, None, 1, 8, 8, *tail, 4, 8.0, 0.005) == 1
    assert b"bilateral_kernel_size must be odd, got 4" in lib.curobo_hip_last_error()
    assert call(p(o), p(m), p(d), None, None, 1, 0, 8, *tail, 5, 8.0, 0.005) == 1 and b"(B, H, W)" in lib.curobo_hip_last_error()
    assert call(None, p(m), p(d), None, None, 1, 8, 8, *tail, 5, 8.0, 0.005) == 1 and b"must not be null" in lib.curobo_hip_last_error()
    assert call(p(d), p(m), p(d), None, None, 1, 8, 8, *tail, 5, 8.0, 0.005) == 1 and b"alias" in lib.curobo_hip_last_error()
    assert call(p(o), p(m), p(d), None, None, 1, 8, 8, *tail, 7, 8.0, 0.005) == 1 and b"scratch" in lib.curobo_hip_last_error()
    assert call(p(o), p(m), p(d), p(t1), p(t2), 1, 8, 8, *tail, 33, 8.0, 0.005) == 1 and b"at most 31" in lib.curobo_hip_last_error()
    assert call(p(o), p(m), p(d), None, None, 1, 8, 8, *tail, 5, 0.0, 0.005) == 1 and b"positive" in lib.curobo_hip_last_error()
    with pytest.raises(ValueError, match="must be odd"):
        _lib.check(call(p(o), p(m), p(d), None, None, 1, 8, 8, *tail, 2, 8.0, 0.005))
    assert call(p(o), p(m), p(d), None, None, 0, 8, 8, *tail, 5, 8.0, 0.005) == 0  # an empty batch launches nothing


def test_robot_mask_arguments_are_validated_without_a_gpu():
    lib = _lib.load()
    d, o, rays = torch.zeros(2, 4, 4), torch.zeros(2, 4, 4), torch.zeros(1, 16, 3)
    m, pos, quat, sph = torch.zeros(2, 4, 4, dtype=U8), torch.zeros(1, 3), torch.zeros(1, 4), torch.zeros(1, 5, 4)
    p = lambda t: t.data_ptr()  # noqa: E731

    def call(mask=p(m), out=p(o), depth=p(d), r=p(rays), cp=p(pos), cq=p(quat), s=p(sph), B=2, H=4, W=4, S=5, rb=1, pb=1, sb=1, mode=0):
        return lib.curobo_hip_robot_mask(mask, out, depth, r, cp, cq, s, B, H, W, S, rb, pb, sb, 0.05, mode, None)

    assert call(sb=3) == 1 and b"robot_spheres batch must be 1 or match points batch: got 3 vs 2" in lib.curobo_hip_last_error()
    assert call(rb=3) == 1 and b"projection rays batch" in lib.curobo_hip_last_error()
    assert call(pb=5) == 1 and b"camera pose batch" in lib.curobo_hip_last_error()
    assert call(mask=None) == 1 and b"must not be null" in lib.curobo_hip_last_error()
    assert call(s=None) == 1 and b"robot_spheres must not be null" in lib.curobo_hip_last_error()
    assert call(W=0) == 1 and b"(B, H, W)" in lib.curobo_hip_last_error()
    assert call(mode=2) == 1 and b"arithmetic mode" in lib.curobo_hip_last_error()
    assert call(S=-1) == 1 and b"num_spheres" in lib.curobo_hip_last_error()
    assert call(B=0) == 0
    from curobo_amd.backends import perception as P

    with pytest.raises(ValueError, match=r"projection_rays must be \(B or 1, 16, 3\)"):
        P.robot_mask(m, o, d, torch.zeros(1, 15, 3), pos, quat, sph, 0.05)
    with pytest.raises(ValueError, match="contiguous"):
        P.robot_mask(m, o, d.transpose(1, 2), rays, pos, quat, sph, 0.05)
    with pytest.raises(ValueError, match=r"depth must be \(B, H, W\)"):
        P.filter_depth(o, m, d[0, 0], None, None, 0.1, 10.0, True, 0.02, 5, 8.0, 0.005)


def test_filter_depth_constants_equal_the_reference():
    from curobo_amd.perception import FilterDepth
    from curobo_amd.perception import FilterDepthConfig

    for name, prm in zip(G["filter_case_names"], G["filter_case_params"]):
        dmin, dmax, fly, ksize, ss, sd, en_f, tol, en_b, radius, ss2, sd2, sep = prm
        fd = FilterDepth((40, 56), dmin, dmax, None if fly < 0 else fly, None if ksize == 0 else int(ksize), ss, sd, device="cpu")
        assert (fd._enable_flying, fd._enable_bilateral, fd._bilateral_radius, fd._use_separable) == (int(en_f), int(en_b), int(radius), bool(sep)), name
        assert fd._flying_tolerance == tol and fd._sigma_spatial_sq2 == ss2 and fd._sigma_depth_sq2 == sd2, name
        assert (fd._depth_temp is not None) == bool(sep) and fd._depth_out.shape == (1, 40, 56) and fd._valid_mask_out.dtype == U8
    fd = FilterDepth((40, 56), device="cpu", num_batch=2)
    assert fd.config.bilateral_sigma_spatial == 10.0 and fd.config.bilateral_sigma_depth == 0.1  # the constructor's defaults
    assert FilterDepthConfig().bilateral_sigma_spatial == 2.0 and FilterDepthConfig().bilateral_sigma_depth == 0.05
    fd.update_config(depth_minimum_distance=0.3, flying_pixel_threshold=0, bilateral_sigma_depth=0.2)
    assert fd.config.depth_minimum_distance == 0.3 and fd.config.flying_pixel_threshold is None and fd._enable_flying == 0
    assert fd._sigma_depth_sq2 == 2.0 * 0.2 ** 2
    fd.update_config(flying_pixel_threshold=1.0)
    assert abs(fd._flying_tolerance - 0.005) < 1e-12 and fd._enable_flying == 1
    fd2 = FilterDepth.from_config(FilterDepthConfig(bilateral_kernel_size=9, flying_pixel_threshold=None), (8, 8), device="cpu", num_batch=3)
    assert fd2._use_separable and fd2._depth_temp.shape == (3, 8, 8) and fd2.config.bilateral_sigma_spatial == 2.0


def test_filter_depth_buffers_and_messages():
    from curobo_amd.perception import FilterDepth

    with pytest.raises(ValueError, match="bilateral_kernel_size must be odd, got 4"):
        FilterDepth((8, 8), bilateral_kernel_size=4, device="cpu")
    fd = FilterDepth((8, 10), device="cpu", num_batch=2)
    with pytest.raises(ValueError, match=r"FilterDepth expects a batched depth tensor of shape \(B, H, W\); got \(8, 10\)\. For a single image, pass depth.unsqueeze\(0\)\."):
        fd(torch.zeros(8, 10))
    d, m = fd._acquire_buffers(2, 8, 10, None, None)
    assert d is fd._depth_out and m is fd._valid_mask_out  # the constructor's shape: the pre-allocated buffers
    d, m = fd._acquire_buffers(1, 8, 10, None, None)
    assert d is not fd._depth_out and d.shape == (1, 8, 10) and m.dtype == U8  # another shape: new ones
    mine = torch.zeros(2, 8, 10)
    d, m = fd._acquire_buffers(2, 8, 10, mine, None)
    assert d is mine and m is fd._valid_mask_out
    with pytest.raises(ValueError, match=r"depth_out must have shape \(B, H, W\)=\(2, 8, 10\); got \(1, 8, 10\)"):
        fd._acquire_buffers(2, 8, 10, torch.zeros(1, 8, 10), None)
    with pytest.raises(ValueError, match="valid_mask_out must have shape"):
        fd._acquire_buffers(2, 8, 10, None, torch.zeros(2, 8, 9, dtype=U8))


def test_projection_helpers_equal_the_reference_exactly():
    from curobo_amd.util.cv import get_projection_rays, project_depth_using_rays

    K, depth = torch.as_tensor(G["seg/intrinsics"]), torch.as_tensor(G["seg/depth"])
    H, W = depth.shape[1:]
    for name in ("b1", "b2_each"):
        idx = G[f"seg/{name}/index"]
        ki = [i for i in idx[1] if i >= 0]
        rays = get_projection_rays(H, W, K[ki], float(G["seg/depth_to_meter"]))
        assert rays.shape == (len(ki), H * W, 3) and np.array_equal(rays.numpy(), G[f"seg/{name}/rays"])
    rays = get_projection_rays(H, W, K[[0]], 1.0)
    pts = project_depth_using_rays(depth[[0]], rays)
    assert np.array_equal(pts.numpy(), G["seg/b1/points"])
    assert np.array_equal(get_projection_rays(H, W, K[[0]], 0.001).numpy(), (rays * 0.001).numpy())
    cut = project_depth_using_rays(torch.tensor([[[0.005, 2.0]]]), torch.ones(1, 2, 3), filter_origin=True)
    assert cut.tolist() == [[[0.0, 0.0, 0.0], [2.0, 2.0, 2.0]]]


def test_camera_observation_members():
    from curobo_amd.types import CameraObservation, Pose

    K, depth = torch.as_tensor(G["seg/intrinsics"]), torch.as_tensor(G["seg/depth"])
    pose = Pose(torch.as_tensor(G["seg/cam_position"][[0]]), torch.as_tensor(G["seg/cam_quaternion"][[0]]))
    obs = CameraObservation(depth_image=depth[[0]].clone(), intrinsics=K[0], pose=pose, depth_to_meter=1.0)
    assert obs.depth_to_meter == 1.0 and CameraObservation().depth_to_meter == 0.001 and CameraObservation().name == "camera_image"
    pts = obs.get_pointcloud()
    assert np.array_equal(pts.numpy(), G["seg/b1/points"]) and np.array_equal(obs.projection_rays.numpy(), G["seg/b1/rays"])
    world = obs.get_pointcloud(project_to_pose=True)
    torch.testing.assert_close(world, pose.batch_transform_points(pts))
    c = obs.clone()
    c.depth_image[0, 10, 10] = 0.004
    c.filter_depth(0.01)
    assert float(c.depth_image[0, 10, 10]) == 0.0 and float(obs.depth_image[0, 10, 10]) == float(depth[0, 10, 10])
    obs.copy_(c)
    assert torch.equal(obs.depth_image, c.depth_image)
    both = obs.stack(c)
    assert both.depth_image.shape == (2, 1, *depth.shape[1:]) and both.pose.position.shape == (2, 3)
    assert obs.to("cpu") is obs
    with pytest.raises(ValueError, match="depth_image is None, cannot generate pointcloud"):
        CameraObservation().get_pointcloud()
    with pytest.raises(ValueError, match="intrinsics is None"):
        CameraObservation(depth_image=depth[[0]]).update_projection_rays()
    with pytest.raises(ValueError, match="rgb_image is None"):
        CameraObservation().shape


def test_robot_segmenter_host_logic():
    from curobo_amd.perception import RobotSegmenter
    from curobo_amd.types import CameraObservation, JointState, Pose

    import inspect

    assert list(inspect.signature(RobotSegmenter.__init__).parameters)[1:] == ["kinematics", "distance_threshold", "use_cuda_graph", "ops_dtype"]
    sig = inspect.signature(RobotSegmenter.__init__).parameters
    assert sig["distance_threshold"].default == 0.05 and sig["use_cuda_graph"].default is True and sig["ops_dtype"].default == torch.bfloat16
    seg = RobotSegmenter.from_robot_file("franka.yml", collision_sphere_buffer=0.01, device_cfg=type("D", (), {"device": "cpu"})())
    from curobo_amd.robot import load_packaged_robot

    base = np.asarray(load_packaged_robot("franka").as_dict()["link_spheres"])[0, :, 3]
    got = seg.kinematics.kinematics_config.link_spheres[0, :, 3].numpy()
    np.testing.assert_allclose(got[base >= 0], base[base >= 0] + 0.01, rtol=0, atol=1e-7)
    assert np.array_equal(got[base < 0], base[base < 0])
    assert seg.base_link == seg.kinematics.base_link and seg.distance_threshold == 0.05 and not seg.ready
    with pytest.raises(ValueError, match="robot_file must be a string path or dict"):
        RobotSegmenter.from_robot_file(3)
    with pytest.raises(ValueError, match="ops_dtype"):
        RobotSegmenter(seg.kinematics, ops_dtype=torch.float16)
    K, depth = torch.as_tensor(G["seg/intrinsics"]), torch.as_tensor(G["seg/depth"])
    obs = CameraObservation(depth_image=depth[[0]], intrinsics=K[0], depth_to_meter=1.0,
                            pose=Pose(torch.as_tensor(G["seg/cam_position"][[0]]), torch.as_tensor(G["seg/cam_quaternion"][[0]])))
    seg32 = RobotSegmenter(seg.kinematics, ops_dtype=torch.float32, use_cuda_graph=False)
    pts = seg32.get_pointcloud_from_depth(obs)
    assert seg32.ready and np.array_equal(pts.numpy(), G["seg/b1/points"])
    rays_buffer = seg32._projection_rays
    seg32.update_camera_projection(obs)
    assert seg32._projection_rays is rays_buffer  # same shape: updated in place
    assert seg.get_pointcloud_from_depth(obs).dtype == torch.bfloat16
    with pytest.raises(ValueError, match=r"Send depth image as \(batch, height, width\)"):
        seg32.get_robot_mask(CameraObservation(depth_image=depth[0], intrinsics=K[0], pose=obs.pose), JointState.from_position(torch.zeros(1, 7)))


def test_update_voxel_errors_and_host_side_effects():
    from curobo_amd.scene import SceneData, voxel_grid_from_sdf
    from curobo_amd.scene.types import VoxelGrid

    a = voxel_grid_from_sdf(lambda p: -np.ones(len(p)), (10, 12, 8), 0.05, name="map")
    scene = SceneData.from_arrays(a, "cpu")
    ptrs = (scene.tensors["voxel_features"].data_ptr(), scene.tensors["voxel_coarse_min"].data_ptr(), scene.struct.voxel_features,
            scene.struct.voxel_coarse_min, scene.struct.voxel_params)
    with pytest.raises(ValueError, match="Voxel grid 'nope' not found in environment 0"):
        scene.update_voxel_features("nope", torch.zeros(960))
    with pytest.raises(ValueError, match=r"Feature tensor size 100 doesn't match grid dims \[10, 12, 8\] = 960"):
        scene.update_voxel_features("map", torch.zeros(100))
    big = VoxelGrid(name="map", pose=[0, 0, 0, 1, 0, 0, 0], dims=[1.0, 1.0, 1.0], voxel_size=0.05, feature_tensor=torch.zeros(8000))
    with pytest.raises(ValueError, match=r"Feature tensor too large for buffer: capacity=960 new=8000\. Increase max_voxels_per_layer\."):
        scene.update_voxel_data(big)
    with pytest.raises(ValueError, match="not found"):
        scene.update_voxel_data(big, name="other")
    wrong = VoxelGrid(name="map", pose=[0, 0, 0, 1, 0, 0, 0], dims=[0.4, 0.4, 0.4], voxel_size=0.05, feature_tensor=torch.zeros(500))
    with pytest.raises(ValueError, match="doesn't match grid dims"):
        scene.update_voxel_data(wrong)
    with pytest.raises(ValueError, match="no voxel store"):
        SceneData.from_arrays(None, "cpu").update_voxel_features("map", torch.zeros(1))
    # an update lands in the buffers the descriptor already points at, and equals a scene built from the new grid
    b = voxel_grid_from_sdf(lambda p: 0.1 - np.abs(p[:, 0]), (10, 12, 8), 0.05, name="map")
    scene.update_voxel_features("map", torch.as_tensor(b["voxel_features"]).reshape(10, 12, 8).float())
    fresh = SceneData.from_arrays(b, "cpu")
    for k in ("voxel_features", "voxel_coarse_min", "voxel_params", "voxel_inv_pose", "voxel_enable"):
        assert torch.equal(scene.tensors[k], fresh.tensors[k]), k
    assert np.array_equal(scene.arrays["voxel_features"], b["voxel_features"])
    small = VoxelGrid(name="map", pose=[0.1, 0.0, 0.2, 1, 0, 0, 0], dims=[0.4, 0.4, 0.4], voxel_size=0.05, feature_tensor=torch.full((8, 8, 8), -0.3))
    scene.enable_obstacle("map", False)
    scene.update_voxel_data(small)
    assert scene.arrays["voxel_params"][0, 0].tolist() == [8.0, 8.0, 8.0, np.float32(0.05)] and int(scene.tensors["voxel_enable"][0, 0]) == 1
    np.testing.assert_allclose(scene.tensors["voxel_inv_pose"][0, 0, :7].numpy(), [-0.1, 0, -0.2, 1, 0, 0, 0], atol=1e-7)
    assert float(scene.tensors["voxel_features"].reshape(-1)[511]) == pytest.approx(-0.3, abs=1e-3) and float(scene.tensors["voxel_features"].reshape(-1)[512]) == 0.0
    assert float(scene.tensors["voxel_coarse_min"][0, 0, 7]) == pytest.approx(-0.3, abs=1e-3) and float(scene.tensors["voxel_coarse_min"][0, 0, 8]) == -65504.0
    assert ptrs == (scene.tensors["voxel_features"].data_ptr(), scene.tensors["voxel_coarse_min"].data_ptr(), scene.struct.voxel_features,
                    scene.struct.voxel_coarse_min, scene.struct.voxel_params)
    with pytest.raises(ValueError, match="add_obstacle takes cuboids"):
        scene.add_obstacle(small)
