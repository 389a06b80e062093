"""The mapper's decay and recycling on the host: the restatement tests/mapper_decay_ref.py on hand-computed cases, against torch's
own arithmetic written out, and against the reference's unmodified frustum kernel (through tests/golden/warp_emulator, where the
reference tree is present); the public surface's checks; and the conditions tests/test_gpu_mapper_decay.py presupposes of its
scene, asserted here with the restatement alone, where they cost no GPU time.

The conditions.  (a) In the frustum-path test (two close cameras, depth range 0.1 .. 0.6 m; block sizes 2, 4, 8) at most 1 % of the
visible blocks are *either* and at least 20 are sure in and 20 sure out.  In the per-frame test the frames' own cameras look at the
sphere from 1.2 m with the whole grid in view: there every visible block is sure IN (asserted as that), so the out factor is the
frustum-path test's to cover.  (b) No block is *either* at the recycle threshold in any decay step of those tests, evaluated on the
oracle's states (the device tests assert the same of the device's states before they compare).  (c) The forgetting test's turned
camera marks no block that touches the sphere's bounding box and has every such block sure out."""

import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mapper_cases as C
import mapper_decay_cases as DC
import mapper_decay_ref as DR
import mapper_ref as R
from curobo_amd import _lib
from curobo_amd.backends import mapper as B
from curobo_amd.perception.mapper import DenseTSDF, Mapper, MapperCfg
from curobo_amd.perception.mapper import decay as D

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.array([[60.0, 0.0, 40.0], [0.0, 60.0, 30.0], [0.0, 0.0, 1.0]])
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0])
RADIUS = DR.SPHERE_FACTOR * 4 * 0.02  # 0.06928 m; at z = 1 its disc is 4.157 px


def _flag(centre, quat=IDENTITY, pos=(0.0, 0.0, 0.0), depth=(0.1, 5.0)):
    inside, either = DR.camera_flags(np.array([centre], np.float64), 4, 0.02, K, pos, quat, 60, 80, *depth)
    assert not either[0]
    return bool(inside[0])


# ---------------------------------------------------------------------------------------------------- the frustum rule by hand
@pytest.mark.parametrize("centre,depth,inside,why", [
    ((0.0, 0.0, 1.0), (0.1, 5.0), True, "on the axis"),
    ((0.0, 0.0, 0.02), (0.1, 5.0), False, "behind the near bound: 0.02 + 0.069 < 0.1"),
    ((0.0, 0.0, 0.04), (0.1, 5.0), True, "its sphere reaches the near bound: 0.04 + 0.069 >= 0.1"),
    ((0.0, 0.0, 5.1), (0.1, 5.0), False, "beyond the far bound: 5.1 - 0.069 > 5"),
    ((0.0, 0.0, 5.05), (0.1, 5.0), True, "its sphere reaches back over the far bound"),
    ((10.0, -7.0, 0.005), (0.05, 5.0), True, "z_cam < 0.01 is inside at once, wherever it projects"),
    ((10.0, -7.0, -0.015), (0.05, 5.0), True, "... behind the camera too, while its sphere reaches the near bound"),
    ((-0.8, 0.0, 1.0), (0.1, 5.0), False, "left: u = -8, -8 + 4.157 < 0"),
    ((0.8, 0.0, 1.0), (0.1, 5.0), False, "right: u = 88, 88 - 4.157 > 80"),
    ((0.0, -0.6, 1.0), (0.1, 5.0), False, "top: v = -6"),
    ((0.0, 0.6, 1.0), (0.1, 5.0), False, "bottom: v = 66, 66 - 4.157 > 60"),
    ((-0.7, 0.0, 1.0), (0.1, 5.0), True, "centre off the image at u = -2, its disc reaches in"),
    ((0.0, 0.55, 1.0), (0.1, 5.0), True, "centre off the image at v = 63, its disc reaches in"),
])
def test_frustum_rule_by_hand(centre, depth, inside, why):
    assert _flag(centre, depth=depth) is inside, why


def test_frustum_rule_rotates_into_the_camera_and_unites_the_cameras():
    q = np.array([np.sqrt(0.5), 0.0, np.sqrt(0.5), 0.0])  # the camera's +z is the world's +x
    assert _flag((1.5, 0.0, 0.3), q, pos=(0.5, 0.0, 0.3)) and not _flag((-0.5, 0.0, 0.3), q, pos=(0.5, 0.0, 0.3))
    # eight blocks of 4 voxels of 0.02 m about (0, 0, 1): centres at +-0.04
    g = R.Grid(8, 8, 8, 4, [0.0, 0.0, 1.0], 0.02, 0.08, 0.1, 5.0, 0.1)
    c = DR.block_centres(g)
    assert np.allclose(c[0], [-0.04, -0.04, 0.96]) and np.allclose(c[7], [0.04, 0.04, 1.04]) and np.allclose(c[1], [0.04, -0.04, 0.96])
    Ks, pos, quat = np.stack([K, K]), np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0]]), np.stack([IDENTITY, IDENTITY])
    sure_in, sure_out = DR.frustum_flags(g, Ks, pos, quat, 60, 80, 0.1, 5.0)
    assert sure_in.all() and not sure_out.any()  # the first camera sees them, the second has them behind it
    sure_in, sure_out = DR.frustum_flags(g, Ks[1:], pos[1:], quat[1:], 60, 80, 0.1, 5.0)
    assert sure_out.all() and not sure_in.any()
    # a block whose depth test is within 1e-5 m of its bound is neither
    sure_in, sure_out = DR.frustum_flags(g, Ks[:1], pos[:1], quat[:1], 60, 80, 0.1, 0.96 - RADIUS + 5e-6)
    assert not sure_in[:4].any() and not sure_out[:4].any() and sure_in[4:].sum() + sure_out[4:].sum() == 4


@pytest.mark.skipif(not os.path.isdir("/root/reference/curobo/_src/perception/mapper"), reason="the reference's Warp sources are not on this machine")
def test_frustum_flags_against_the_reference_kernel():
    """tests/mapper_decay_warp_check.py: mark_blocks_in_frustum_kernel of the reference's builder_decay.py, unmodified, on every block
    of the scene at block sizes 2, 4, 8 for the tests' cameras"""
    out = subprocess.run([sys.executable, os.path.join(REPO, "tests", "mapper_decay_warp_check.py")], capture_output=True, text=True, timeout=600,
                         cwd=REPO)
    print(out.stdout)
    assert out.returncode == 0 and ", 0 failed" in out.stdout and "flags compared" in out.stdout, (out.stdout + out.stderr)[-2000:]


# ---------------------------------------------------------------------------------------------------- arithmetic and threshold
def test_the_two_decay_expressions_are_what_the_kernel_is_told():
    """torch's mul_ on an fp16 tensor, written out: times a Python scalar the product is formed in fp32 with the scalar as fp32;
    times an fp16 tensor the factor was rounded to fp16 first.  The launch multiplies in fp32 by the float the host passes."""
    rng = np.random.default_rng(2)
    data = np.concatenate([rng.uniform(-60, 60, 3000), rng.uniform(-1e-4, 1e-4, 3000), [0.0, 65504.0, 6e-8, -6e-8]]).astype(np.float16)
    data = data[: 6000].reshape(15, 200, 2)
    f32, f16 = lambda x: np.float32(x), lambda x: np.float32(np.float16(x))  # noqa: E731
    with np.errstate(under="ignore"):
        assert np.array_equal(DR.decay_uniform(data, 0.9).view(np.uint16), (data.astype(np.float32) * f32(0.9)).astype(np.float16).view(np.uint16))
        assert np.array_equal(DR.decay_uniform(data, 1.0).view(np.uint16), data.view(np.uint16))
        flags = np.arange(15) % 3 == 0
        want = data.astype(np.float32) * np.where(flags, f16(0.97 * 0.5), f16(0.97))[:, None, None]
        assert np.array_equal(DR.decay_frustum(data, flags, 0.97, 0.5).view(np.uint16), want.astype(np.float16).view(np.uint16))
    assert f32(0.9) != f16(0.9) and D._f32(0.9) == float(f32(0.9)) and D._f16(0.97 * 0.5) == float(f16(0.97 * 0.5))
    assert (DR.decay_uniform(data, 0.9) != (data.astype(np.float32) * f16(0.9)).astype(np.float16)).any(), "the two roundings differ on this data"


@pytest.mark.parametrize("block_size,threshold", [(2, 1.5625e-4), (4, 1.25e-3), (8, 1e-2)])
def test_recycle_threshold_scales_with_the_voxels_of_a_block(block_size, threshold):
    assert DR.empty_threshold(block_size) == pytest.approx(threshold, rel=1e-12)
    assert B.decay_empty_threshold(block_size) == float(np.float32(threshold))
    v = block_size ** 3
    data = np.zeros((4, v, 2), np.float16)
    data[0, 0, 1], data[1, 0, 1], data[2, :, 1] = threshold * 0.5, threshold * 2.0, threshold / v * 0.5  # below, above, below as a sum
    data[3, 0, 1] = threshold * 0.5                                                                   # below, but never visible
    out, visible, recycled, either = DR.recycle(data, [True, True, True, False], block_size)
    assert recycled.tolist() == [True, False, True, False] and visible.tolist() == [False, True, False, False] and not either.any()
    assert not out[0].any() and not out[2].any() and out[1, 0, 1] == data[1, 0, 1] and out[3, 0, 1] == data[3, 0, 1]
    # two weights that sum to the threshold as nearly as fp16 allows (the second is a subnormal, in steps of 6e-8): *either*
    a = np.float16(threshold * 0.999)
    data[1, 0, 1], data[1, 1, 1] = a, threshold - float(a)
    gap = abs(data[1, :, 1].astype(np.float64).sum() - threshold) / threshold
    assert DR.recycle(data, [True] * 4, block_size)[3].tolist() == [False, bool(gap <= DR.SUM_TOL), False, False]
    assert gap <= DR.SUM_TOL or block_size == 2, gap


# ---------------------------------------------------------------------------------------------------- the public surface
@pytest.mark.parametrize("kw", [dict(time_decay=0.0), dict(time_decay=1.5), dict(frustum_decay=-0.5), dict(frustum_decay=1.0001),
                                dict(time_decay=float("nan"))])
def test_mapper_validates_its_factors(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        Mapper(MapperCfg(**C.CFG), **kw)


def test_decay_functions_validate_before_any_launch():
    p = B.make_params((20, 48, 50), 4, (0.0, 0.0, 0.0), 0.02, 0.08, 0.1, 5.0, 0.1)
    tsdf = DenseTSDF(block_data=torch.zeros((p.n_blocks, 64, 2), dtype=torch.float16), block_visible=torch.zeros(780, dtype=torch.uint8),
                     frame_visible=torch.zeros(780, dtype=torch.uint8), params=p)
    assert tsdf.block_recycled.dtype == torch.uint8 and tsdf.block_recycled.shape == (780,) and tsdf.n_blocks == 780
    with pytest.raises(ValueError, match="decay_factor"):
        D.decay_and_recycle(tsdf, 0.0)
    cams = (torch.zeros(1, 3, 3), torch.zeros(1, 3), torch.zeros(1, 4))
    with pytest.raises(ValueError, match="time_decay"):
        D.decay_frustum_aware_multi_camera(tsdf, *cams, (60, 80), time_decay=1.5, frustum_decay=0.5)
    with pytest.raises(ValueError, match="frustum_decay"):
        D.decay_frustum_aware_multi_camera(tsdf, *cams, (60, 80), frustum_decay=0.0)
    args = (tsdf.block_data, tsdf.block_visible, tsdf.block_recycled, p)
    with pytest.raises(ValueError, match="factor_inside"):
        B.mapper_decay(*args, 0.5, 1.5, 0.00125)
    with pytest.raises(ValueError, match="recycled"):
        B.mapper_decay(tsdf.block_data, tsdf.block_visible, torch.zeros(10, dtype=torch.uint8), p, 0.5, 0.5, 0.00125)
    with pytest.raises(ValueError, match="block_data"):
        B.mapper_decay(torch.zeros((780, 64, 2)), tsdf.block_visible, tsdf.block_recycled, p, 0.5, 0.5, 0.00125)
    with pytest.raises(ValueError, match="come together"):
        B.mapper_decay(*args, 0.5, 0.5, 0.00125, intrinsics=cams[0])
    with pytest.raises(ValueError, match="cam_quaternion"):
        B.mapper_decay(*args, 0.5, 0.5, 0.00125, cams[0], cams[1], torch.zeros(1, 3), (60, 80))
    with pytest.raises(ValueError, match="image_shape"):
        B.mapper_decay(*args, 0.5, 0.5, 0.00125, *cams, image_shape=(0, 80))


def test_entry_point_validates_before_any_launch():
    lib = _lib.load()
    err = lib.curobo_hip_last_error
    assert "curobo_hip_mapper_decay" in _lib.declared_symbols() and "curobo_hip_mapper_decay" in _lib._signatures()
    p = B.make_params((20, 48, 50), 4, (0.0, 0.0, 0.0), 0.02, 0.08, 0.1, 5.0, 0.1)
    pp = ctypes.addressof(p)
    buf = (ctypes.c_uint32 * 64)()
    a = ctypes.addressof(buf)
    decay = lib.curobo_hip_mapper_decay
    assert decay(a, a, a, None, None, None, 0, 0, 0, 0.5, 0.5, 0.00125, None, None) == 1 and b"params must not be null" in err()
    assert decay(a, a, None, None, None, None, 0, 0, 0, 0.5, 0.5, 0.00125, pp, None) == 1 and b"recycled" in err()
    assert decay(a, a, a, None, None, None, -1, 0, 0, 0.5, 0.5, 0.00125, pp, None) == 1 and b"n_cameras" in err()
    assert decay(a, a, a, a, a, None, 1, 60, 80, 0.5, 0.5, 0.00125, pp, None) == 1 and b"cam_quaternion" in err()
    assert decay(a, a, a, a, a, a, 1, 60, 0, 0.5, 0.5, 0.00125, pp, None) == 1 and b"positive" in err()
    assert decay(a, a, a, None, None, None, 0, 0, 0, 0.5, 1.5, 0.00125, pp, None) == 1 and b"[0, 1]" in err()
    assert decay(a, a, a, None, None, None, 0, 0, 0, float("nan"), 0.5, 0.00125, pp, None) == 1 and b"[0, 1]" in err()
    assert decay(a, a, a, None, None, None, 0, 0, 0, 0.5, 0.5, -1.0, pp, None) == 1 and b"empty_threshold" in err()
    big = B.make_params((20, 48, 50), 8, (0.0, 0.0, 0.0), 0.02, 0.08, 0.1, 5.0, 0.1)
    assert decay(a + 4, a, a, None, None, None, 0, 0, 0, 0.5, 0.5, 0.01, ctypes.addressof(big), None) == 1 and b"16-byte aligned" in err()


def test_mapper_cfg_still_refuses_and_says_where_to_set_the_factors():
    for field in ("decay_factor", "frustum_decay_factor"):
        with pytest.raises(NotImplementedError, match=field):
            MapperCfg(**C.CFG, **{field: 0.9})
    assert "time_decay" in MapperCfg.__doc__ and "time_decay" in Mapper.__doc__ and "MapperCfg" in Mapper.__doc__


def test_exports():
    from curobo_amd.perception import mapper as M

    assert M.decay_and_recycle is D.decay_and_recycle and M.decay_frustum_aware_multi_camera is D.decay_frustum_aware_multi_camera
    assert {"decay_and_recycle", "decay_frustum_aware_multi_camera"} <= set(M.__all__)
    spec = importlib.util.spec_from_file_location("_facade_perception_decay", os.path.join(REPO, "curobo", "perception.py"))
    per = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(per)
    assert per.decay_and_recycle is D.decay_and_recycle and per.decay_frustum_aware_multi_camera is D.decay_frustum_aware_multi_camera
    assert per.__all__ == ["FilterDepth", "RobotSegmenter"] and not hasattr(per, "Mapper")  # as the older host tests pin the facade
    import dataclasses
    import inspect

    assert [f.name for f in dataclasses.fields(DenseTSDF)][-1] == "block_recycled"
    sig = inspect.signature(D.decay_frustum_aware_multi_camera)
    assert list(sig.parameters) == ["tsdf", "intrinsics", "cam_positions", "cam_quaternions", "img_shape", "depth_minimum_distance",
                                    "depth_maximum_distance", "time_decay", "frustum_decay", "num_blocks"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[5:]] == [0.1, 10.0, 1.0, 0.5, None]
    assert inspect.signature(D.decay_and_recycle).parameters["decay_factor"].default == 0.95
    init = inspect.signature(Mapper.__init__).parameters
    assert list(init)[1:] == ["config", "use_graph", "time_decay", "frustum_decay"] and init["time_decay"].default == init["frustum_decay"].default == 1.0


# ---------------------------------------------------------------------------------------------------- conditions of the device tests
@pytest.fixture(scope="module", params=DC.BLOCK_SIZES)
def oracle_state(request):
    """(block size, grid, fp16 [n_blocks, bs^3, 2], visible) after mapper_cases.FRAMES on the oracle"""
    g = DC.grid(request.param)
    last = C.oracle_run(g)[-1]
    return request.param, g, np.stack([last["sw"], last["w"]], -1), DC.marked(request.param)[0]


def test_conditions_of_the_frustum_path_test(oracle_state):
    bs, g, data, visible = oracle_state
    sure, possible = DC.marked(bs)
    sure_in, sure_out = DC.frustum_sets(bs)
    either = ~sure_in & ~sure_out
    print(f"block size {bs}: {int(possible.sum())} visible blocks, {int((sure_in & sure).sum())} sure in, {int((sure_out & sure).sum())} sure out, "
          f"{int((either & possible).sum())} either")
    assert (either & possible).sum() <= 0.01 * possible.sum()
    assert (sure_in & sure).sum() >= 20 and (sure_out & sure).sum() >= 20
    # out by the image and (at blocks of 2 and 4) out by the far bound alone both occur among them: the open range has fewer
    open_out = DR.frustum_flags(g, *DC.frustum_cameras(), C.H, C.W, DC.FRUSTUM_DEPTH[0], 5.0)[1]
    assert 0 < (open_out & sure).sum() < (sure_out & sure).sum() + (bs == 8)
    for step in (DR.step_uniform(data, visible, bs, 0.9), DR.step_frame(data, visible, bs, sure_in, DC.TIME_DECAY, DC.FRUSTUM_DECAY)):
        assert not step[3].any(), "a block sum within 1e-4 of the threshold"


def test_conditions_of_the_recycling_test(oracle_state):
    bs, g, data, visible = oracle_state
    steps, counts = 0, []
    while visible.any():
        data, visible, recycled, either = DR.step_uniform(data, visible, bs, 0.5)
        assert not either.any(), f"step {steps}: a block sum within 1e-4 of the threshold"
        counts.append(int(recycled.sum()))
        steps += 1
        assert steps <= 40
    print(f"block size {bs}: recycled per step {counts}")
    assert sum(1 for c in counts if c) >= 3, "the blocks go over several steps"
    assert not data.any()


def test_conditions_of_the_per_frame_test():
    g = DC.grid()
    visible = np.zeros(g.n_blocks, bool)
    states = list(DR.frame_sequence(g, [C.frame(*cams) for cams in C.FRAMES], 0.9, 0.5, C.H, C.W))
    for k, (cams, s) in enumerate(zip(C.FRAMES, states)):
        _, Ks, pos, quat = C.frame(*cams)
        sure_in, _ = DR.frustum_flags(g, Ks, pos, quat, C.H, C.W, g.depth_min, g.depth_max)
        assert (sure_in | ~visible).all(), "every visible block is sure in the frusta of the frames' own cameras"
        assert not s["either_frustum"].any() and not s["either_sum"].any()
        assert s["recycled"].any() == (k > 0), "blocks that were marked and received no weight go at the next frame's decay"
        visible = s["visible"]
    assert states[0]["recycled"].sum() == 0 and (np.asarray(states[2]["w"], np.float32) > 1.0).any()


def test_conditions_of_the_forgetting_test():
    g, box = DC.grid(), DC.sphere_blocks()
    run = DC.forgetting()
    states, n = run["states"], run["frames"]
    depth, Ks, pos, quat = DC.turned_frame()
    assert (depth > 0).all(), "the turned camera sees the ground in every pixel"
    _, sure_out = DR.frustum_flags(g, Ks, pos, quat, C.H, C.W, g.depth_min, g.depth_max)
    first = states[0]["visible"]
    assert (first & box).sum() > 100 and (sure_out | ~(first & box)).all(), "every visible block at the sphere is sure out for the turned camera"
    assert not (states[1]["possible"] & box).any() and states[1]["sure"].sum() >= 20
    print(f"{n} turned frames until the first frame's blocks are gone; visible per frame {[int(s['visible'].sum()) for s in states]}")
    assert 10 <= n <= 30 and len(states) == n + 1
    for s in states:
        assert not s["either_sum"].any() and (s["possible"] == s["sure"]).all()
    assert (states[n - 1]["visible"] & ~states[n - 1]["possible"]).any() and (states[n - 2]["visible"] & box).any(), "it takes that many"
    assert np.array_equal(states[n]["visible"], states[n]["sure"]) and not (states[n]["visible"] & box).any()
