"""The mapper's lidar path on the host: the restatement tests/mapper_lidar_ref.py on hand-computed cases and against the reference's
unmodified kernels (through tests/golden/warp_emulator, where the reference tree is present); the public surface's checks; and the
conditions tests/test_gpu_mapper_lidar.py presupposes of its scene, asserted here with the restatement alone, where they cost no
GPU time.

The conditions.  (a) Every path of the integration launch is taken by at least 20 voxels of sensor A's frame that the device test
compares: bilinear accepted, guard rejected then nearest accepted, a corner invalid then nearest accepted, nearest rejected by the ray
distance, a column from across the seam, clamped at +truncation, dropped below -truncation.  (b) In every frame of every run the
excluded voxels are at most 1 % of the voxels of sure blocks, possible-minus-sure at most 1 % of the possible blocks.  (c) In the
decay tests at most 1 % of all blocks are *either*, at least 20 visible blocks are sure in and 20 sure out, and no block sum is
within tolerance of the recycle threshold.  (d) The forgetting test's turned sensor leaves more than 100 blocks of the first
frame unmarked, and they go within a few frames."""

import ctypes
import dataclasses
import importlib.util
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mapper_cases as C
import mapper_decay_cases as DC
import mapper_decay_ref as DR
import mapper_lidar_cases as LC
import mapper_lidar_ref as LR
import mapper_ref as R
from curobo_amd import _lib
from curobo_amd.backends import mapper as B
from curobo_amd.perception.mapper import DenseTSDF, Mapper, MapperCfg, MapperLidarCfg
from curobo_amd.perception.mapper import decay as D
from curobo_amd.types import LidarObservation, Pose

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0])


# ---------------------------------------------------------------------------------------------------- the rules by hand
def test_pixel_rays_and_their_inverse():
    rays = LR.pixel_rays(5, 8, -0.4, 0.4)
    assert np.allclose(rays[2, 4], [1.0, 0.0, 0.0], atol=1e-6), "the middle row and column W / 2 look along +x"
    assert np.allclose(rays[2, 0], [-1.0, 0.0, 0.0], atol=1e-6) and np.allclose(rays[2, 6], [0.0, 1.0, 0.0], atol=1e-6)
    assert np.allclose(rays[0, 4], [math.cos(0.4), 0.0, math.sin(0.4)], atol=1e-6), "row 0 is the highest elevation"
    assert np.allclose(np.linalg.norm(rays, axis=-1), 1.0)
    u, v, el, band = LR.voxel_uv(rays * 0.7, 5, 8, -0.4, 0.4)
    py, px = np.meshgrid(np.arange(5), np.arange(8), indexing="ij")
    # (the far side of the seam: column 0 comes back as 0 or as W, a rounding of pi decides)
    assert np.allclose(np.minimum(np.abs(u - px), np.abs(u - px - 8)), 0.0, atol=1e-5) and np.allclose(v, py, atol=1e-5) and band[1:-1].all()
    assert np.allclose(LR.pixel_rays(1, 8, -0.3, -0.3)[0, 4], [math.cos(-0.3), 0.0, math.sin(-0.3)], atol=1e-6), "a planar scan looks along min_elev"
    u, v, el, band = LR.voxel_uv(np.array([[1.0, 0.0, 5.0]]), 1, 8, -0.3, -0.3)
    assert v[0] == 0.0 and band[0] and abs(u[0] - 4.0) < 1e-5, "a planar sensor takes every elevation, v = 0"
    assert LR.PI == float(np.float32(math.pi)) and LR.PI != math.pi


def _one_voxel(rng, point, H=3, W=8, elev=(-0.4, 0.4), linear=0.04, nearest=0.01):
    v = np.array([point], np.float64)
    u, vv, _, band = LR.voxel_uv(v, H, W, *elev)
    assert band[0]
    return {k: (a[0] if isinstance(a, np.ndarray) else a) for k, a in
            LR.sensor_range(np.asarray(rng, np.float64), v, u, vv, H, W, 0.1, 5.0, *elev, linear, nearest).items()}


def test_interpolation_rules_by_hand():
    H, W = 3, 8
    rays = LR.pixel_rays(H, W, -0.4, 0.4)
    flat = np.full((H, W), 1.0)
    between = rays[1, 4] + rays[1, 5] + rays[2, 4] + rays[2, 5]
    between = 0.8 * between / np.linalg.norm(between)   # inside the four pixels (1..2, 4..5)
    s = _one_voxel(flat, between)
    assert s["bilinear"] and s["ok"] and abs(s["surface"] - 1.0) < 1e-12
    step = flat.copy()
    step[:, 5] = 1.2                                     # a range step of 0.2 m between the columns: the guard of 0.04 m refuses
    s = _one_voxel(step, between)
    assert not s["bilinear"] and s["nearest_rejected"] and not s["ok"], "refused, and the voxel is far from any pixel's ray"
    near = 0.8 * rays[1, 4] + np.array([0.0, 0.004, 0.0])  # 4 mm off the ray of pixel (1, 4): nearest accepts within 10 mm
    s = _one_voxel(step, near)
    assert s["guard_then_nearest"] and s["ok"] and s["surface"] == 1.0
    hole = flat.copy()
    hole[2, 5] = 0.0                                     # an invalid corner
    s = _one_voxel(hole, near)
    assert s["corner_then_nearest"] and s["ok"] and not s["bilinear"]
    s = _one_voxel(hole, 0.8 * rays[1, 4] + np.array([0.0, 0.02, 0.0]), nearest=0.01)
    assert s["nearest_rejected"] and not s["ok"], "20 mm off the ray"
    # the seam: a voxel between the last column and the first interpolates across it
    seam = rays[1, 7] + rays[1, 0] + rays[2, 7] + rays[2, 0]
    ramp = flat.copy()
    ramp[:, 0], ramp[:, 7] = 1.02, 1.0
    s = _one_voxel(ramp, 0.8 * seam / np.linalg.norm(seam))
    assert s["bilinear"] and s["seam"] and 1.0 < s["surface"] < 1.02
    # the planar sensor never interpolates
    s = _one_voxel(np.full((1, W), 1.0), 0.8 * LR.pixel_rays(1, W, -0.3, -0.3)[0, 3] + np.array([0.0, 0.0, 0.003]), H=1, elev=(-0.3, -0.3))
    assert s["ok"] and not s["bilinear"] and not s["guard_then_nearest"]


def test_integrate_by_hand_and_its_ambiguity_flags():
    g = R.Grid(8, 8, 8, 4, [0.0, 0.0, 0.0], 0.02, 0.08, 0.1, 5.0, 0.1)
    zero = np.zeros((g.n_blocks, 64), np.float16)
    pos, quat = np.array([[-0.5, 0.003, 0.001]]), IDENTITY[None]
    rng = np.full((1, 9, 64), 0.5, np.float32)           # a sphere of 0.5 m about the sensor: the surface crosses the grid near x = 0
    args = (rng, pos, quat, np.array([[0.1, 5.0]]), np.array([[-0.5, 0.5]]), 0.04, 0.01)
    sw, w, upd, amb = LR.integrate(g, zero, zero, np.ones(g.n_blocks, bool), *args)
    rho = np.linalg.norm(g.voxel_centres() - pos[0], axis=-1)
    want = np.clip(0.5 - rho, None, 0.08)
    assert upd.all() and (w == 1).all(), "every voxel is within the truncation distance behind the surface or in front of it"
    assert np.abs(sw.astype(np.float64) - want).max() < 1e-4
    _, _, upd_none, _ = LR.integrate(g, zero, zero, np.zeros(g.n_blocks, bool), *args)
    assert not upd_none.any(), "only the blocks handed over are written"
    far = (np.full((1, 9, 64), 0.3, np.float32), *args[1:])
    assert not LR.integrate(g, zero, zero, np.ones(g.n_blocks, bool), *far)[2].any(), "all voxels more than the truncation behind the surface"
    # a voxel whose range is within 1e-5 of the lower bound is flagged and its neighbours are not
    centre = g.voxel_centres()[0, 0]
    bound = np.array([[np.float32(np.linalg.norm(centre - pos[0]) + 4e-6), 5.0]])
    _, _, upd_b, amb_b = LR.integrate(g, zero, zero, np.ones(g.n_blocks, bool), rng, pos, quat, bound, *args[4:])
    assert amb_b[0, 0] and amb_b.sum() < 8


@pytest.mark.parametrize("centre,H,inside,why", [
    ((1.0, 0.0, 0.0), 32, True, "in the band, on the horizon"),
    ((0.02, 0.0, 0.0), 32, False, "short of the range band: 0.02 + 0.069 < 0.1"),
    ((0.04, 0.0, 0.0), 32, True, "its sphere reaches the near bound; the sensor sits in it: angular radius pi"),
    ((5.1, 0.0, 0.0), 32, False, "beyond the far bound"),
    ((0.0, -5.05, 0.0), 32, True, "its sphere reaches back over the far bound, at any azimuth"),
    ((0.5, 0.0, 0.5), 32, False, "elevation 0.785, angular radius 0.098: above the band's 0.5"),
    ((0.5, 0.0, 0.33), 32, True, "elevation 0.583 - 0.116 <= 0.5"),
    ((-0.5, 0.0, -0.5), 32, False, "below the band's -0.6 by more than its angular radius"),
    ((1.0, 0.0, 0.05), 1, True, "planar at elevation 0: 0.05 rad off, angular radius 0.069"),
    ((1.0, 0.0, 0.1), 1, False, "planar: 0.0997 rad off"),
])
def test_lidar_frustum_rule_by_hand(centre, H, inside, why):
    elev = (-0.6, 0.5) if H > 1 else (0.0, 0.0)
    got, either = LR.lidar_flags(np.array([centre], np.float64), 4, 0.02, (0.0, 0.0, 0.0), IDENTITY, (0.1, 5.0), elev, H)
    assert not either[0] and bool(got[0]) is inside, why


def test_frustum_flags_unite_cameras_and_lidars():
    g = LC.grid()
    lidars = LC.decay_lidars("band")
    cams = (*DC.frustum_cameras(), C.H, C.W, *DC.FRUSTUM_DEPTH)
    l_in, l_out = LR.frustum_flags(g, lidars=lidars)
    c_in, c_out = LR.frustum_flags(g, cameras=cams)
    assert np.array_equal(c_in, DC.frustum_sets(4)[0]) and np.array_equal(c_out, DC.frustum_sets(4)[1]), "the camera part is mapper_decay_ref's"
    u_in, u_out = LR.frustum_flags(g, cameras=cams, lidars=lidars)
    assert np.array_equal(u_in, l_in | c_in) and np.array_equal(u_out, l_out & c_out)
    none_in, none_out = LR.frustum_flags(g)
    assert not none_in.any() and none_out.all()


@pytest.mark.skipif(not os.path.isdir("/root/reference/curobo/_src/perception/mapper"), reason="the reference's Warp sources are not on this machine")
def test_restatement_against_the_reference_kernels():
    """tests/mapper_lidar_warp_check.py: lidar_compute_block_keys_only_kernel, lidar_integrate_voxels_kernel and
    mark_lidar_blocks_in_frustum_kernel of the reference, unmodified, on this scene"""
    out = subprocess.run([sys.executable, os.path.join(REPO, "tests", "mapper_lidar_warp_check.py")], capture_output=True, text=True, timeout=900,
                         cwd=REPO)
    print(out.stdout)
    assert out.returncode == 0 and ", 0 failed" in out.stdout and "answers compared" in out.stdout, (out.stdout + out.stderr)[-2000:]


def test_warp_check_says_so_without_the_reference_tree(tmp_path):
    """the script exits 0 with a message where the reference is absent (its path rewritten to one that does not exist)"""
    text = open(os.path.join(REPO, "tests", "mapper_lidar_warp_check.py")).read()
    assert text.count('REFERENCE = "/root/reference"') == 1
    script = tmp_path / "check.py"
    script.write_text(text.replace('REFERENCE = "/root/reference"', f'REFERENCE = "{tmp_path / "absent"}"'))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "no reference tree here" in out.stdout and "0 failed" in out.stdout


# ---------------------------------------------------------------------------------------------------- the public surface
def test_lidar_cfg_checks():
    cfg = MapperLidarCfg(num_sensors=2, image_height=32, image_width=256)
    assert cfg.linear_interpolation_max_allowable_difference_vox == 2.0 and cfg.nearest_interpolation_max_allowable_dist_to_ray_vox == 0.5
    assert cfg.max_support_pixels_per_block_lidar == 8 and cfg.max_visible_blocks_per_lidar_integration is None
    assert MapperLidarCfg(image_height=1, image_width=360).num_sensors == 1
    for kw, match in ((dict(num_sensors=0), "num_sensors"), (dict(num_sensors=True), "plain int"), (dict(num_sensors=1.0), "plain int"),
                      (dict(image_height=0), "image_height"), (dict(image_width=-3), "image_width"), (dict(image_height=32.0), "plain int"),
                      (dict(image_width=None), "image_height and image_width"),
                      (dict(linear_interpolation_max_allowable_difference_vox=0.0), "linear_interpolation"),
                      (dict(nearest_interpolation_max_allowable_dist_to_ray_vox=-1.0), "nearest_interpolation"),
                      (dict(max_support_pixels_per_block_lidar=0), "max_support_pixels"), (dict(max_visible_blocks_per_lidar_integration=0), "max_visible")):
        with pytest.raises(ValueError, match=match):
            MapperLidarCfg(**{**dict(num_sensors=1, image_height=32, image_width=256), **kw})
    assert "no effect" in MapperLidarCfg.__doc__ and "MapperLidarCfg" in MapperCfg.__doc__ and "MapperLidarCfg" in Mapper.__doc__
    assert "follow-up" in MapperCfg.__doc__ and "follow-up" in Mapper.__doc__


def test_mapper_cfg_still_refuses_lidar_sensors():
    with pytest.raises(NotImplementedError, match="lidar_num_sensors"):
        MapperCfg(**C.CFG, lidar_num_sensors=1)


def _host_cfg():
    return MapperCfg(**{**C.CFG, "device": "cpu"})


def _observation(names=("A",)):
    rng, pos, quat, valid_range, elev_range = (torch.as_tensor(a) for a in LC.frame(*names))
    return LidarObservation(range_image=rng, pose=Pose(pos, quat), valid_range_m=valid_range, elevation_range_rad=elev_range)


def test_a_mapper_without_lidars_still_refuses_and_says_how_to_enable_them():
    mapper = Mapper(_host_cfg())
    assert mapper.lidar_config is None
    for kw in (dict(lidar_observation=_observation()), dict(observation=_observation()), dict(lidar_observation=object())):
        with pytest.raises(NotImplementedError, match="lidar") as e:
            mapper.integrate(**kw)
        assert "MapperLidarCfg" in str(e.value)
    with pytest.raises(NotImplementedError, match="lidar"):
        mapper.integrate(_observation())
    assert mapper.get_stats()["frame_count"] == 0
    with pytest.raises(TypeError, match="MapperLidarCfg"):
        Mapper(_host_cfg(), lidar=dict(num_sensors=1))
    with pytest.raises(ValueError, match="max_visible_blocks_per_lidar_integration"):
        Mapper(_host_cfg(), lidar=MapperLidarCfg(image_height=32, image_width=256, max_visible_blocks_per_lidar_integration=10 ** 6))
    with pytest.raises(TypeError):
        Mapper(_host_cfg()).integrate(_observation(), lidar_observation=_observation())


def test_observation_is_validated_before_any_launch():
    mapper = Mapper(_host_cfg(), use_graph=False, lidar=MapperLidarCfg(num_sensors=1, image_height=LC.H, image_width=LC.W))
    assert mapper.lidar_config.num_sensors == 1
    tensors = mapper._lidar_tensors(_observation())
    assert [tuple(t.shape) for t in tensors] == [(1, LC.H, LC.W), (1, 3), (1, 4), (1, 2), (1, 2)] and all(t.dtype == torch.float32 for t in tensors)
    for field, value, match in (("range_image", None, "range_image is required"), ("range_image", torch.zeros(LC.H, LC.W), "num_lidars, H, W"),
                                ("range_image", torch.zeros(2, LC.H, LC.W), "shape mismatch"), ("range_image", torch.zeros(1, LC.H, LC.W + 1), "shape mismatch"),
                                ("range_image", torch.zeros(1, LC.H, LC.W, dtype=torch.float64), "float32"),
                                ("rgb_image", torch.zeros(1, LC.H, LC.W, 4, dtype=torch.uint8), "rgb_image shape mismatch"),
                                ("rgb_image", torch.zeros(1, LC.H, LC.W, 3), "uint8"), ("pose", None, "pose is required"),
                                ("valid_range_m", None, "valid_range_m is required"), ("valid_range_m", torch.zeros(2), "valid_range_m must be"),
                                ("valid_range_m", torch.zeros(1, 2, dtype=torch.float64), "valid_range_m dtype"),
                                ("elevation_range_rad", None, "elevation_range_rad is required"),
                                ("elevation_range_rad", torch.zeros(1, 3), "elevation_range_rad must be")):
        obs = _observation()
        setattr(obs, field, value)
        with pytest.raises(ValueError, match=match):
            mapper.integrate(lidar_observation=obs)
    obs = _observation()
    obs.feature_grid = torch.zeros(1, 4, 4, 8, dtype=torch.float16)
    with pytest.raises(NotImplementedError, match="feature_dim"):
        mapper.integrate(obs)
    obs = _observation()
    obs.pose = Pose(torch.zeros(2, 3), torch.tensor([[1.0, 0, 0, 0]] * 2))
    with pytest.raises(ValueError, match="pose holds 2"):
        mapper.integrate(obs)
    planar = Mapper(_host_cfg(), lidar=MapperLidarCfg(image_height=1, image_width=LC.W))
    obs = _observation(("P",))
    planar._lidar_tensors(obs)
    obs.elevation_range_rad = torch.tensor([[-0.3, 0.2]])
    with pytest.raises(ValueError, match="Planar"):
        planar.integrate(obs)
    assert mapper.get_stats()["frame_count"] == 0


def test_lidar_observation_methods():
    obs = _observation(("A", "B"))
    assert obs.name == "lidar_range_image" and tuple(obs.shape) == (2, LC.H, LC.W)
    assert [f.name for f in dataclasses.fields(LidarObservation)] == ["name", "range_image", "rgb_image", "feature_grid", "pose", "valid_range_m",
                                                                      "elevation_range_rad", "timestamp"]
    assert all(f.default is None for f in dataclasses.fields(LidarObservation)[1:])
    with pytest.raises(ValueError, match="range_image is None"):
        LidarObservation().shape
    copy = obs.clone()
    assert copy is not obs and copy.range_image.data_ptr() != obs.range_image.data_ptr() and torch.equal(copy.range_image, obs.range_image)
    assert copy.rgb_image is None and copy.timestamp is None and torch.equal(copy.pose.position, obs.pose.position)
    copy.range_image += 1.0
    copy.valid_range_m[:, 1] = 9.0
    assert not torch.equal(copy.range_image, obs.range_image)
    kept = obs.range_image
    assert obs.copy_(copy) is obs and obs.range_image is kept and torch.equal(obs.range_image, copy.range_image) and obs.valid_range_m[0, 1] == 9.0
    moved = obs.to(torch.device("cpu"))
    assert moved is obs and obs.range_image.device.type == "cpu" and obs.pose.position.device.type == "cpu"
    assert LidarObservation().clone().range_image is None and LidarObservation().to("cpu").pose is None


def test_exports():
    from curobo_amd.perception import mapper as M
    import curobo_amd.perception as P

    assert M.MapperLidarCfg is MapperLidarCfg and M.decay_frustum_aware_multi_sensor is D.decay_frustum_aware_multi_sensor
    assert {"MapperLidarCfg", "decay_frustum_aware_multi_sensor", "decay_frustum_aware_multi_camera", "Mapper", "MapperCfg"} <= set(M.__all__)
    assert P.__all__ == ["FilterDepth", "FilterDepthConfig", "RobotSegmenter", "DetectionResult", "RobotMesh", "SDFDetectorCfg", "SDFPoseDetector"]
    facade = {}
    for name in ("perception", "types"):
        spec = importlib.util.spec_from_file_location(f"_facade_{name}_lidar", os.path.join(REPO, "curobo", f"{name}.py"))
        facade[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(facade[name])
    per, types = facade["perception"], facade["types"]
    assert per.__all__ == ["FilterDepth", "RobotSegmenter"] and not hasattr(per, "Mapper")  # as the older host tests pin the facade
    assert per.decay_frustum_aware_multi_sensor is D.decay_frustum_aware_multi_sensor
    assert types.LidarObservation is LidarObservation and "LidarObservation" in types.__all__ and "CameraObservation" in types.__all__
    sig = inspect.signature(D.decay_frustum_aware_multi_sensor)
    assert list(sig.parameters) == ["tsdf", "camera_intrinsics", "camera_positions", "camera_quaternions", "camera_img_shape",
                                    "camera_depth_minimum_distance", "camera_depth_maximum_distance", "lidar_positions", "lidar_quaternions",
                                    "lidar_valid_range_m", "lidar_elevation_range_rad", "lidar_img_shape", "time_decay", "frustum_decay", "num_blocks"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in list(sig.parameters.values())[1:])
    assert [sig.parameters[k].default for k in ("camera_depth_minimum_distance", "camera_depth_maximum_distance", "time_decay", "frustum_decay")] \
        == [0.1, 10.0, 1.0, 0.5]
    names = [f.name for f in dataclasses.fields(DenseTSDF)]
    assert "lidar_frame_visible" in names and names[-1] == "block_recycled"
    p = B.make_params((20, 48, 50), 4, (0.0, 0.0, 0.0), 0.02, 0.08, 0.1, 5.0, 0.1)
    tsdf = DenseTSDF(block_data=torch.zeros((p.n_blocks, 64, 2), dtype=torch.float16), block_visible=torch.zeros(780, dtype=torch.uint8),
                     frame_visible=torch.zeros(780, dtype=torch.uint8), params=p)
    assert tsdf.lidar_frame_visible.dtype == torch.uint8 and tsdf.lidar_frame_visible.shape == (780,)
    mapper = Mapper(_host_cfg())
    mb = mapper.memory_usage_mb()
    assert mb * 2 ** 20 >= mapper.tsdf.block_data.numel() * 2 + 4 * mapper.tsdf.lidar_frame_visible.numel()
    mapper.tsdf.lidar_frame_visible.fill_(1)
    mapper.reset()
    assert not mapper.tsdf.lidar_frame_visible.any()


# ---------------------------------------------------------------------------------------------------- validation before any launch
def test_entry_points_validate_before_any_launch():
    lib = _lib.load()
    err = lib.curobo_hip_last_error
    names = ("curobo_hip_mapper_lidar_mark_blocks", "curobo_hip_mapper_lidar_integrate", "curobo_hip_mapper_decay_sensors")
    assert set(names) <= set(_lib.declared_symbols()) and set(names) <= set(_lib._signatures()) and lib.curobo_hip_abi_version() == 7
    p = B.make_params((20, 48, 50), 4, (0.0, 0.0, 0.0), 0.02, 0.08, 0.1, 5.0, 0.1)
    assert ctypes.sizeof(p) == 68, "curobo_hip_mapper_params is as it was: the sensor-side settings are plain arguments"
    pp = ctypes.addressof(p)
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    mark, integrate, decay = (getattr(lib, n) for n in names)
    assert mark(a, a, a, a, a, a, a, a, None, 1, 32, 256, None) == 1 and b"params must not be null" in err()
    assert mark(a, a, a, None, a, a, a, a, pp, 1, 32, 256, None) == 1 and b"range" in err() and b"must not be null" in err()
    assert mark(a, a, a, a, a, a, a, None, pp, 1, 32, 256, None) == 1 and b"elevation_range" in err()
    assert mark(None, a, a, a, a, a, a, a, pp, 1, 32, 256, None) == 1 and b"lidar_mask" in err()
    assert mark(a, a, a, a, a, a, a, a, pp, 0, 32, 256, None) == 1 and b"(n_lidars, H, W)" in err()
    assert mark(a, a, a, a, a, a, a, a, pp, 1, 32, 0, None) == 1 and b"(1, 32, 0)" in err()
    assert mark(a, a, a, a, a, a, a, a, pp, 1 << 12, 1 << 10, 1 << 10, None) == 1 and b"2^31 pixels" in err()
    assert integrate(None, a, a, a, a, a, a, pp, 1, 32, 256, 0.04, 0.01, None) == 1 and b"block_data and lidar_mask" in err()
    assert integrate(a + 2, a, a, a, a, a, a, pp, 1, 32, 256, 0.04, 0.01, None) == 1 and b"4-byte aligned" in err()
    assert integrate(a, a, a, a, None, a, a, pp, 1, 32, 256, 0.04, 0.01, None) == 1 and b"lidar_quaternion" in err()
    assert integrate(a, a, a, a, a, a, a, pp, 1, 32, 256, 0.0, 0.01, None) == 1 and b"linear_max_diff_m" in err()
    assert integrate(a, a, a, a, a, a, a, pp, 1, 32, 256, 0.04, float("nan"), None) == 1 and b"nearest_max_dist_m" in err()
    cams, lidars, tail = (None, None, None, 0, 0, 0), (a, a, a, a, 1, 32), (0.5, 0.5, 0.00125, pp, None)
    assert decay(a, a, a, *cams, *lidars, 0.5, 0.5, 0.00125, None, None) == 1 and b"params must not be null" in err()
    assert decay(a, a, a, *cams, a, a, a, a, -1, 32, *tail) == 1 and b"n_lidars" in err()
    assert decay(a, a, a, *cams, a, a, a, None, 1, 32, *tail) == 1 and b"lidar_elevation_range" in err()
    assert decay(a, a, a, *cams, a, a, a, a, 1, 0, *tail) == 1 and b"lidar_height" in err()
    assert decay(a, a, a, a, a, None, 1, 60, 80, *lidars, *tail) == 1 and b"cam_quaternion" in err()
    assert decay(a, a, None, *cams, *lidars, *tail) == 1 and b"recycled" in err() and b"mapper_decay_sensors" in err()
    assert decay(a, a, a, *cams, *lidars, 0.5, 1.5, 0.00125, pp, None) == 1 and b"[0, 1]" in err()


def test_bindings_validate_before_any_launch():
    p = B.make_params((20, 48, 50), 4, (0.0, 0.0, 0.0), 0.02, 0.08, 0.1, 5.0, 0.1)
    data, mask = torch.zeros((p.n_blocks, 64, 2), dtype=torch.float16), torch.zeros(780, dtype=torch.uint8)
    rng, pos, quat, vr, er = torch.zeros(1, 32, 256), torch.zeros(1, 3), torch.zeros(1, 4), torch.zeros(1, 2), torch.zeros(1, 2)
    with pytest.raises(ValueError, match="range_image must be"):
        B.mapper_lidar_mark_blocks(mask, mask, mask, rng[0], pos, quat, vr, er, p)
    with pytest.raises(ValueError, match="lidar_quaternion must have shape"):
        B.mapper_lidar_mark_blocks(mask, mask, mask, rng, pos, quat[:, :3], vr, er, p)
    with pytest.raises(ValueError, match="holds 2 lidars"):
        B.mapper_lidar_mark_blocks(mask, mask, mask, rng, torch.zeros(2, 3), torch.zeros(2, 4), torch.zeros(2, 2), torch.zeros(2, 2), p)
    with pytest.raises(ValueError, match="lidar_mask"):
        B.mapper_lidar_mark_blocks(mask[:10], mask, mask, rng, pos, quat, vr, er, p)
    with pytest.raises(ValueError, match="valid_range"):
        B.mapper_lidar_integrate(data, mask, rng, pos, quat, vr.double(), er, p, 0.04, 0.01)
    with pytest.raises(ValueError, match="block_data"):
        B.mapper_lidar_integrate(data.float(), mask, rng, pos, quat, vr, er, p, 0.04, 0.01)
    with pytest.raises(ValueError, match="nearest_max_dist_m"):
        B.mapper_lidar_integrate(data, mask, rng, pos, quat, vr, er, p, 0.04, 0.0)
    args = (data, mask, mask.clone(), p, 0.5, 0.5, 0.00125)
    with pytest.raises(ValueError, match="elevation_range is required"):
        B.mapper_decay_sensors(*args, lidar_position=pos, lidar_quaternion=quat, lidar_valid_range=vr, lidar_height=32)
    with pytest.raises(ValueError, match="lidar_height"):
        B.mapper_decay_sensors(*args, lidar_position=pos, lidar_quaternion=quat, lidar_valid_range=vr, lidar_elevation_range=er)
    with pytest.raises(ValueError, match="come together"):
        B.mapper_decay_sensors(*args, intrinsics=torch.zeros(1, 3, 3))
    with pytest.raises(ValueError, match="factor_outside"):
        B.mapper_decay_sensors(data, mask, mask.clone(), p, -0.5, 0.5, 0.00125)
    tsdf = DenseTSDF(block_data=data, block_visible=mask, frame_visible=mask.clone(), params=p)
    with pytest.raises(ValueError, match="lidar_positions requires"):
        D.decay_frustum_aware_multi_sensor(tsdf, lidar_positions=pos, time_decay=0.9, frustum_decay=0.5)
    with pytest.raises(ValueError, match="camera_intrinsics requires"):
        D.decay_frustum_aware_multi_sensor(tsdf, camera_intrinsics=torch.zeros(1, 3, 3), time_decay=0.9, frustum_decay=0.5)
    with pytest.raises(ValueError, match="height must be positive"):
        D.decay_frustum_aware_multi_sensor(tsdf, lidar_positions=pos, lidar_quaternions=quat, lidar_valid_range_m=vr, lidar_elevation_range_rad=er,
                                           lidar_img_shape=(0, 256), time_decay=0.9, frustum_decay=0.5)
    with pytest.raises(ValueError, match="frustum_decay"):
        D.decay_frustum_aware_multi_sensor(tsdf, frustum_decay=0.0)
    with pytest.raises(ValueError, match="time_decay must be <= 1"):
        D.decay_frustum_aware_multi_sensor(tsdf, time_decay=1.5, frustum_decay=0.5)


# ---------------------------------------------------------------------------------------------------- conditions of the device tests
def test_scene_takes_every_path():
    """sensor A's frame, over the voxels the device test compares (sure blocks, not ambiguous)"""
    g = LC.grid()
    s = LC.oracle_run("single")[0]
    keep = s["sure"][:, None] & ~s["ambiguous"]
    counts = {name: int(np.sum(m & keep)) for name, m in s["paths"].items()}
    counts["updated"] = int((s["updated"] & keep).sum())
    print(f"sensor A, {int(s['sure'].sum())} sure blocks: {counts}")
    assert set(counts) == {"updated", "bilinear", "guard_then_nearest", "corner_then_nearest", "nearest_rejected", "seam", "clamped", "dropped"}
    assert min(counts.values()) >= 20, counts
    rng = LC.sensor("A")[0]
    assert (rng == 0).any() and (rng > 0).any(), "rays that leave the grid's scene return nothing"
    # the seam's columns carry the nearest surface: the sphere
    assert 0 < rng[LC.H // 2, 0] < 0.4 and 0 < rng[LC.H // 2, LC.W - 1] < 0.4
    planar = LC.oracle_run("planar")[0]
    assert (planar["updated"] & planar["sure"][:, None] & ~planar["ambiguous"]).sum() >= 200


@pytest.mark.parametrize("run", sorted(LC.RUNS))
def test_conditions_of_the_integration_tests(run):
    clean, ever_sure, amb = True, False, False
    for k, s in enumerate(LC.oracle_run(run)):
        gap = int((s["possible"] & ~s["sure"]).sum())
        assert gap <= 0.01 * s["possible"].sum()
        for kind in ("cam", "lidar"):
            clean = clean & (s[kind + "_sure"] | ~s[kind + "_possible"])
        ever_sure, amb = ever_sure | s["sure"], amb | s["ambiguous"]
        excluded = (~(clean[:, None] & ~amb))[ever_sure].mean()
        share = s["ambiguous"][s["updated"]].mean()
        print(f"{run} frame {k}: {int(s['sure'].sum())} sure blocks, {gap} possible only, {int(s['updated'].sum())} voxels updated, excluded "
              f"{excluded:.4f}, ambiguous among the updated {share:.4f}")
        assert excluded <= 0.01 and s["sure"].sum() >= 20


@pytest.mark.parametrize("lidars,cameras", [("band", False), ("planar", False), ("band", True)])
def test_conditions_of_the_decay_tests(lidars, cameras):
    g = LC.grid()
    last = LC.oracle_run("pair")[-1]
    data, visible = np.stack([last["sw"], last["w"]], -1), last["sure"]
    cams = (*DC.frustum_cameras(), C.H, C.W, *DC.FRUSTUM_DEPTH) if cameras else None
    sure_in, sure_out = LR.frustum_flags(g, cameras=cams, lidars=LC.decay_lidars(lidars))
    either = ~sure_in & ~sure_out
    print(f"lidars '{lidars}'{' and cameras' if cameras else ''}: {int((sure_in & visible).sum())} visible blocks sure in, "
          f"{int((sure_out & visible).sum())} sure out, {int(either.sum())} either of {g.n_blocks}")
    assert either.sum() <= 0.01 * g.n_blocks and (sure_in & visible).sum() >= 20 and (sure_out & visible).sum() >= 20
    if cameras:
        lidar_in, camera_in = LR.frustum_flags(g, lidars=LC.decay_lidars(lidars))[0], LR.frustum_flags(g, cameras=cams)[0]
        assert (camera_in & ~lidar_in & visible).sum() >= 5 and (lidar_in & ~camera_in & visible).sum() >= 5
    for flags in (np.ones_like(visible), np.zeros_like(visible)):
        assert not DR.step_frame(data, visible, g.bs, flags, LC.TIME_DECAY, LC.FRUSTUM_DECAY)[3].any(), "a block sum within 1e-4 of the threshold"


def test_conditions_of_the_forgetting_test():
    run = LC.forgetting()
    region = run["first"] & ~run["turned_possible"]
    print(f"{run['frames']} turned frames until {int(region.sum())} blocks are gone; the turned sensor marks {int(run['turned_sure'].sum())}")
    assert region.sum() > 100 and 2 <= run["frames"] <= 10 and not run["either_sum"]
    assert run["turned_sure"].sum() >= 10 and np.array_equal(run["turned_sure"], run["turned_possible"])
    assert np.array_equal(run["first"], run["first_possible"])
