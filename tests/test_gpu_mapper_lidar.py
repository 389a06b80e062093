"""Lidar range images into the mapper on the GPU (csrc/mapper_lidar.hip, and the lidar frustum of csrc/mapper.hip's decay) against
the float64 restatement tests/mapper_lidar_ref.py, on the scene of tests/mapper_lidar_cases.py.

What is compared, and why those bounds -- those of tests/test_gpu_mapper.py.  Which blocks a frame marks is exact outside the
restatement's possible-minus-sure set.  Which voxels a frame updates is exact on sure blocks outside the restatement's ambiguous
voxels.  There the stored pair is one fp32 add and one rounding to fp16 per pair-add launch that touched the voxel away from the
float64 value (the launch forms the sdf in double from the same fp32 inputs and the same two widened constants, so its gap to
the float64 value is far below an fp16 step and only a near-tie can land on the neighbour): <= k fp16 steps after k launches, a
frame that carries cameras and lidars being two launches.  Untouched voxels are bit-identical.  The decay's words are the
restatement's torch arithmetic on the device's own state, bit for bit; which factor a block takes is exact on the restatement's
sure-in and sure-out blocks, and an *either* block carries one of the two as a whole.  tests/test_mapper_lidar_host.py asserts,
without a GPU, that the scene meets the conditions these comparisons presuppose."""

import numpy as np
import pytest
import torch

import mapper_cases as C
import mapper_decay_cases as DC
import mapper_decay_ref as DR
import mapper_lidar_cases as LC
import mapper_lidar_ref as LR
import mapper_ref as R

pytestmark = pytest.mark.gpu


def _cfg():
    from curobo_amd.perception.mapper import MapperCfg

    return MapperCfg(**C.CFG)


def _lidar_cfg(names):
    from curobo_amd.perception.mapper import MapperLidarCfg

    return MapperLidarCfg(num_sensors=len(names), image_height=LC.SENSORS[names[0]][2], image_width=LC.W)


def _lidar_obs(names, device):
    from curobo_amd.types import LidarObservation, Pose

    rng, pos, quat, valid_range, elev_range = LC.frame(*names)
    t = lambda a: torch.as_tensor(a, device=device)  # noqa: E731
    return LidarObservation(range_image=t(rng), pose=Pose(t(pos), t(quat)), valid_range_m=t(valid_range), elevation_range_rad=t(elev_range))


def _camera_obs(cams, device):
    from curobo_amd.types import CameraObservation, Pose

    depth, K, pos, quat = C.frame(*cams)
    t = lambda a: torch.as_tensor(a, device=device)  # noqa: E731
    return CameraObservation(depth_image=t(depth), intrinsics=t(K), pose=Pose(t(pos), t(quat)))


def _integrate(mapper, cams, lidars, device):
    kw = {}
    if cams is not None:
        kw["camera_observation"] = _camera_obs(cams, device)
    if lidars is not None:
        kw["lidar_observation"] = _lidar_obs(lidars, device)
    mapper.integrate(**kw)


def _snap(mapper):
    """dict(sw, w fp16 [n_blocks, bs^3]; ever, frame, lidar, recycled bool [n_blocks]) on the host"""
    torch.cuda.synchronize()
    t = mapper.tsdf
    mask = lambda m: m.cpu().numpy()[: t.n_blocks] != 0  # noqa: E731
    data = t.block_data.cpu().numpy()
    return dict(data=data, sw=data[..., 0], w=data[..., 1], ever=mask(t.block_visible), frame=mask(t.frame_visible),
                lidar=mask(t.lidar_frame_visible), recycled=mask(t.block_recycled))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.fixture(scope="module")
def grid():
    return LC.grid()


@pytest.fixture(scope="module")
def device_runs(device):
    """every run of mapper_lidar_cases.RUNS on the device, each on a mapper of its own: name -> (mapper, the state after every frame)"""
    from curobo_amd.perception.mapper import Mapper

    out = {}
    for name, frames in LC.RUNS.items():
        mapper = Mapper(_cfg(), lidar=_lidar_cfg(frames[0][1]))
        states = []
        for cams, lidars in frames:
            _integrate(mapper, cams, lidars, device)
            states.append(_snap(mapper))
        out[name] = (mapper, states)
    return out


# ---------------------------------------------------------------------------------------------------- 1: blocks
@pytest.mark.parametrize("run", sorted(LC.RUNS))
def test_visible_masks(run, device_runs):
    ever_sure = ever_possible = False
    for k, (ref, got) in enumerate(zip(LC.oracle_run(run), device_runs[run][1])):
        print(f"{run} frame {k}: {int(got['frame'].sum())} blocks on the device ({int(got['lidar'].sum())} by lidars), {int(ref['sure'].sum())} sure, "
              f"{int(ref['possible'].sum())} possible")
        assert (ref["possible"] & ~ref["sure"]).sum() <= 0.01 * ref["possible"].sum()
        assert (ref["sure"] <= got["frame"]).all() and (got["frame"] <= ref["possible"]).all(), "the frame's union"
        assert (ref["lidar_sure"] <= got["lidar"]).all() and (got["lidar"] <= ref["lidar_possible"]).all(), "what the lidar integration reads"
        ever_sure, ever_possible = ever_sure | ref["sure"], ever_possible | ref["possible"]
        assert (ever_sure <= got["ever"]).all() and (got["ever"] <= ever_possible).all()
    assert ever_sure.sum() >= 20


# ---------------------------------------------------------------------------------------------------- 2: voxels and the stored pair
@pytest.mark.parametrize("run", sorted(LC.RUNS))
def test_updated_voxels_and_the_stored_pair(run, grid, device_runs):
    shape = (grid.n_blocks, grid.bs ** 3)
    clean_block, ever_sure = np.ones(grid.n_blocks, bool), np.zeros(grid.n_blocks, bool)
    amb, touches = np.zeros(shape, bool), np.zeros(shape, np.int64)
    prev = (np.zeros(shape, np.float16), np.zeros(shape, np.float16))
    for k, (ref, got) in enumerate(zip(LC.oracle_run(run), device_runs[run][1]), start=1):
        for kind in ("cam", "lidar"):  # a block counts while each kind's marking of it was certain in every frame so far
            clean_block &= ref[kind + "_sure"] | ~ref[kind + "_possible"]
        ever_sure |= ref["sure"]
        amb |= ref["ambiguous"]
        touches += ref["cam_updated"].astype(np.int64) + ref["lidar_updated"]  # pair-add launches that touched the voxel
        keep = clean_block[:, None] & ~amb
        excluded = (~keep)[ever_sure].mean()
        assert excluded <= 0.01, f"{excluded:.4f} of the voxels of sure blocks are excluded: change the scene"
        sw, w = got["sw"], got["w"]
        changed = (_bits(sw) != _bits(prev[0])) | (_bits(w) != _bits(prev[1]))
        assert np.array_equal(changed[keep], ref["updated"][keep]), "which voxels the frame updated"  # (an update adds weight >= 1)
        steps_sw, steps_w = R.half_steps(sw, ref["sw"]), R.half_steps(w, ref["w"])
        print(f"{run} after {k} frames: {int(ref['updated'][keep].sum())} voxels updated ({int(ref['lidar_updated'][keep].sum())} by lidars), excluded "
              f"{excluded:.4f}, fp16 steps from the oracle: sum {int(steps_sw[keep].max())} (differing {float((steps_sw[keep] > 0).mean()):.5f}), "
              f"weight {int(steps_w[keep].max())}, at most {int(touches[keep].max())} launches on a voxel")
        assert (steps_sw <= touches)[keep].all() and (steps_w <= touches)[keep].all()
        still = keep & ~ref["updated"]
        assert np.array_equal(_bits(sw[still]), _bits(prev[0][still])) and np.array_equal(_bits(w[still]), _bits(prev[1][still]))
        prev = (sw, w)
    assert ref["lidar_updated"][keep].sum() >= 200
    if run == "mixed":
        assert (touches[keep] == 2).sum() > 1000, "voxels that the camera launch and the lidar launch both touched"
        only_cam = ref["cam_sure"] & ~ref["lidar_possible"]
        assert only_cam.sum() >= 20 and not ref["lidar_updated"][only_cam].any(), "lidar sums go to lidar-marked blocks only"
    if run == "pair":
        assert (np.asarray(ref["w"], np.float32)[keep] == 2.0).sum() > 500, "voxels that both sensors of the frame saw"


def test_frame_count_and_stats(device_runs):
    mapper, states = device_runs["mixed"]
    stats = mapper.get_stats()
    assert stats["frame_count"] == 1, "a camera and a lidar observation in one call are one frame"
    assert stats["last_frame_blocks"] == int(states[0]["frame"].sum()) and stats["visible_blocks"] == int(states[0]["ever"].sum())
    assert device_runs["single"][0].get_stats()["frame_count"] == 2
    mapper.reset()
    s = _snap(mapper)
    assert not s["data"].any() and not s["ever"].any() and not s["frame"].any() and not s["lidar"].any() and mapper.get_stats()["frame_count"] == 0


def test_integrate_validates_the_observation(device):
    from curobo_amd.perception.mapper import Mapper

    mapper = Mapper(_cfg(), lidar=_lidar_cfg(("A",)))
    good = _lidar_obs(("A",), device)
    mapper.integrate(good)                      # positional
    mapper.integrate(observation=good)          # the older keyword
    good.rgb_image = torch.zeros((1, LC.H, LC.W, 3), dtype=torch.uint8, device=device)
    mapper.integrate(lidar_observation=good)    # colour is checked and not used
    assert mapper.get_stats()["frame_count"] == 3
    for field, value, match in (("range_image", good.range_image[:, :-1], "range_image shape mismatch"),
                                ("range_image", good.range_image.double(), "float32"),
                                ("rgb_image", torch.zeros((1, LC.H, LC.W, 3), device=device), "uint8"),
                                ("valid_range_m", None, "valid_range_m is required"),
                                ("elevation_range_rad", good.elevation_range_rad.reshape(2), "elevation_range_rad must be"),
                                ("pose", None, "pose is required")):
        bad = good.clone()
        setattr(bad, field, value)
        with pytest.raises(ValueError, match=match):
            mapper.integrate(bad)
    bad = good.clone()
    bad.feature_grid = torch.zeros((1, 4, 4, 8), dtype=torch.float16, device=device)
    with pytest.raises(NotImplementedError, match="feature_dim"):
        mapper.integrate(bad)
    with pytest.raises(ValueError, match="range_image shape mismatch"):
        mapper.integrate(_lidar_obs(("A", "B"), device))  # two sensors into a mapper configured for one
    planar = Mapper(_cfg(), lidar=_lidar_cfg(("P",)))
    bad = _lidar_obs(("P",), device)
    bad.elevation_range_rad = torch.tensor([[-0.3, 0.1]], device=device)
    with pytest.raises(ValueError, match="Planar"):
        planar.integrate(bad)
    assert mapper.get_stats()["frame_count"] == 3 and planar.get_stats()["frame_count"] == 0


# ---------------------------------------------------------------------------------------------------- 3: decay
def _mapper_with(state, device, **kw):
    """a new mapper holding a snapshot's words and ever-visible mask"""
    from curobo_amd.perception.mapper import Mapper

    mapper = Mapper(_cfg(), **kw)
    t = mapper.tsdf
    t.block_data.copy_(torch.as_tensor(state["data"]))
    t.block_visible[: t.n_blocks] = torch.as_tensor(state["ever"].astype(np.uint8))
    return mapper


@pytest.mark.parametrize("lidars,cameras", [("band", False), ("planar", False), ("band", True)])
def test_frustum_decay_over_lidars_and_cameras(lidars, cameras, grid, device_runs, device):
    from curobo_amd.perception.mapper import decay_frustum_aware_multi_sensor

    state = device_runs["pair"][1][-1]
    data, visible = state["data"], state["ever"]
    pos, quat, valid_range, elev_range, H = LC.decay_lidars(lidars)
    cams = (*DC.frustum_cameras(), C.H, C.W, *DC.FRUSTUM_DEPTH) if cameras else None
    sure_in, sure_out = LR.frustum_flags(grid, cameras=cams, lidars=(pos, quat, valid_range, elev_range, H))
    either = ~sure_in & ~sure_out
    assert (either & visible).sum() <= 0.01 * visible.sum() and (sure_in & visible).sum() >= 20 and (sure_out & visible).sum() >= 20
    if cameras:  # the union is more than either kind's: blocks only the cameras have in, and blocks only the lidars have
        lidar_in = LR.frustum_flags(grid, lidars=(pos, quat, valid_range, elev_range, H))[0]
        camera_in = LR.frustum_flags(grid, cameras=cams)[0]
        assert (camera_in & ~lidar_in & visible).sum() >= 5 and (lidar_in & ~camera_in & visible).sum() >= 5
    as_in = DR.step_frame(data, visible, grid.bs, np.ones_like(visible), LC.TIME_DECAY, LC.FRUSTUM_DECAY)
    as_out = DR.step_frame(data, visible, grid.bs, np.zeros_like(visible), LC.TIME_DECAY, LC.FRUSTUM_DECAY)
    assert not as_in[3].any() and not as_out[3].any() and np.array_equal(as_in[2], as_out[2]), "no block sum near the threshold under either factor"
    gone = as_in[2]  # (blocks that were marked and never received weight: sum 0)
    mapper = _mapper_with(state, device)
    t = lambda a: torch.as_tensor(a, device=device)  # noqa: E731
    kw = dict(lidar_positions=t(pos), lidar_quaternions=t(quat), lidar_valid_range_m=t(valid_range), lidar_elevation_range_rad=t(elev_range),
              lidar_img_shape=(H, LC.W), time_decay=LC.TIME_DECAY, frustum_decay=LC.FRUSTUM_DECAY)
    if cameras:
        K, cpos, cquat = (t(a) for a in DC.frustum_cameras())
        kw.update(camera_intrinsics=K, camera_positions=cpos, camera_quaternions=cquat, camera_img_shape=(C.H, C.W),
                  camera_depth_minimum_distance=DC.FRUSTUM_DEPTH[0], camera_depth_maximum_distance=DC.FRUSTUM_DEPTH[1])
    assert decay_frustum_aware_multi_sensor(mapper.tsdf, **kw) is None
    after = _snap(mapper)
    got = after["data"]
    is_in = (_bits(got) == _bits(as_in[0])).all((1, 2))
    is_out = (_bits(got) == _bits(as_out[0])).all((1, 2))
    differ = (_bits(as_in[0]) != _bits(as_out[0])).any((1, 2))
    assert differ[visible & ~gone].mean() > 0.9, "the two factors give different words in nearly every visible block"
    assert is_in[sure_in].all(), "every sure-in block carries the in factor"
    assert is_out[sure_out].all(), "every sure-out block carries the out factor"
    assert (is_in | is_out)[either].all(), "an either block carries one of the two, as a whole"
    print(f"lidars '{lidars}'{' and two cameras' if cameras else ''}: {int((sure_in & visible).sum())} visible blocks sure in, "
          f"{int((sure_out & visible).sum())} sure out, {int((either & visible).sum())} either")
    assert not got[~visible].any(), "never-visible blocks stay all zero"
    assert np.array_equal(after["ever"], visible & ~gone) and np.array_equal(after["recycled"], gone)


def test_the_camera_entry_and_the_sensor_entry_without_lidars_agree(device_runs, device):
    from curobo_amd.backends import mapper as B

    state = device_runs["pair"][1][-1]
    cams = tuple(torch.as_tensor(a, device=device) for a in DC.frustum_cameras())
    thr = B.decay_empty_threshold(4)
    results = []
    for entry in (B.mapper_decay, B.mapper_decay_sensors):
        for with_cameras in (True, False):
            t = _mapper_with(state, device).tsdf
            args = (*cams, (C.H, C.W)) if with_cameras else ()
            entry(t.block_data, t.block_visible, t.block_recycled, t.params, 0.5, 0.25, thr, *args)
            torch.cuda.synchronize()
            results.append((t.block_data.clone(), t.block_visible.clone(), t.block_recycled.clone()))
    for k in (0, 1):
        a, b = results[k], results[k + 2]
        assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert not torch.equal(results[0][0].view(torch.int16), results[1][0].view(torch.int16)), "the cameras' frusta changed some block's factor"
    assert not torch.equal(results[0][0].view(torch.int16), torch.as_tensor(state["data"], device=device).view(torch.int16))


def test_integrate_decays_once_over_the_union_of_both_kinds_of_frusta(grid, device):
    """the per-frame path: a second frame that carries a camera and a lidar starts with ONE decay over the union of their frusta,
    then integrates; held to the restatement's decay of the device's state followed by the oracle's frame"""
    from curobo_amd.perception.mapper import Mapper

    mapper = Mapper(_cfg(), lidar=_lidar_cfg(("A",)), time_decay=0.9, frustum_decay=0.5)
    _integrate(mapper, (1,), ("B",), device)
    first = _snap(mapper)
    data, visible = first["data"], first["ever"]
    depth, K, cpos, cquat = C.frame(0)
    rng, pos, quat, valid_range, elev_range = LC.frame("A")
    sure_in, sure_out = LR.frustum_flags(grid, cameras=(K, cpos, cquat, C.H, C.W, grid.depth_min, grid.depth_max),
                                         lidars=(pos, quat, valid_range, elev_range, LC.H))
    either_f = visible & ~sure_in & ~sure_out
    assert either_f.sum() <= 0.01 * visible.sum() and (sure_in & visible).sum() >= 20
    start, start_visible, recycled, either_s = DR.step_frame(data, visible, grid.bs, sure_in, 0.9, 0.5)
    assert not either_s.any()
    _integrate(mapper, (0,), ("A",), device)
    got = _snap(mapper)
    assert mapper.get_stats()["frame_count"] == 2
    ok = ~either_f
    assert np.array_equal(got["recycled"][ok], recycled[ok])
    ref = LC.oracle_frame(grid, start[..., 0], start[..., 1], (0,), ("A",))
    assert (ref["sure"] <= got["frame"]).all() and (got["frame"] <= ref["possible"]).all()
    clean = ok & (ref["cam_sure"] | ~ref["cam_possible"]) & (ref["lidar_sure"] | ~ref["lidar_possible"])
    keep = clean[:, None] & ~ref["ambiguous"]
    assert (~keep)[ref["sure"]].mean() <= 0.01
    changed = (_bits(got["sw"]) != _bits(start[..., 0])) | (_bits(got["w"]) != _bits(start[..., 1]))
    assert np.array_equal(changed[keep], ref["updated"][keep]), "which voxels the frame updated, from the decayed state"
    touches = ref["cam_updated"].astype(np.int64) + ref["lidar_updated"]
    assert (R.half_steps(got["sw"], ref["sw"]) <= touches)[keep].all() and (R.half_steps(got["w"], ref["w"]) <= touches)[keep].all()
    assert ref["lidar_updated"][keep].sum() > 1000 and ref["cam_updated"][keep].sum() > 1000


# ---------------------------------------------------------------------------------------------------- 4: forgetting, ESDF
def test_what_the_lidar_no_longer_sees_is_forgotten(device):
    from curobo_amd.perception.mapper import Mapper

    run = LC.forgetting()  # (the restatement's run; tests/test_mapper_lidar_host.py holds its conditions)
    region = run["first"] & ~run["turned_possible"]
    forgetful, keeper = Mapper(_cfg(), lidar=_lidar_cfg(("A",)), time_decay=LC.FORGET_TIME_DECAY), Mapper(_cfg(), lidar=_lidar_cfg(("A",)))
    for m in (forgetful, keeper):
        m.integrate(_lidar_obs(("A",), device))
    assert (_snap(forgetful)["ever"] & region).sum() == region.sum() > 100
    turned = _lidar_obs(("T",), device)
    for _ in range(run["frames"]):
        for m in (forgetful, keeper):
            m.integrate(lidar_observation=turned)
    s = _snap(forgetful)
    assert not (s["ever"] & region).any() and not s["data"][region].any(), "the region the sensor turned away from is recycled"
    assert np.array_equal(s["ever"], s["frame"]) and (run["turned_sure"] <= s["frame"]).all() and (s["frame"] <= run["turned_possible"]).all()
    assert not s["data"][~s["ever"]].any() and forgetful.get_stats()["visible_blocks"] == int(s["frame"].sum())
    kept = _snap(keeper)
    assert (kept["ever"] & region).sum() == region.sum() and kept["w"][region].any()


def test_esdf_after_lidar_frames(device_runs, device):
    """negative inside the sphere, positive in the free space the lidars looked through"""
    mapper = device_runs["pair"][0]
    out = mapper.compute_esdf(esdf_origin=torch.tensor(C.ESDF_ORIGIN))
    torch.cuda.synchronize()
    dist = out.feature_tensor.cpu().numpy().astype(np.float64)
    centres = R.esdf_centres(C.ESDF_SHAPE, C.ESDF_ORIGIN, C.CFG["esdf_voxel_size"])
    true = R.scene_distance(centres)
    cell = C.CFG["esdf_voxel_size"]
    negative = dist < 0
    # (the lidars see two cells deep, the truncation distance: the float64 oracle has 20 negative cells here, 17 of them in the sphere)
    assert negative.sum() >= 10 and (true[negative] < cell).all(), "negative cells lie in the sphere or the ground (to within a cell)"
    inside_sphere = negative & (np.linalg.norm(centres, axis=-1) < R.SPHERE_RADIUS)
    assert inside_sphere.sum() >= 8
    # cells on sensor A's line of sight to the sphere (0.25 m of free space), from the near bound of its range to 0.06 m before the
    # surface: a cell's centre is at most 0.035 m from a point in it, so still outside the sphere
    eye = np.asarray(LC.SENSORS["A"][0])
    toward = -eye / np.linalg.norm(eye)
    reach = np.linalg.norm(eye) - R.SPHERE_RADIUS
    ts = np.arange(LC.VALID_RANGE[0], reach - 0.06, 0.02)
    assert len(ts) >= 4
    idx = np.floor((eye + ts[:, None] * toward - np.asarray(C.ESDF_ORIGIN)) / cell + 0.5 * np.asarray(C.ESDF_SHAPE)).astype(int)
    free = dist[idx[:, 0], idx[:, 1], idx[:, 2]]
    print("ESDF along sensor A's line of sight to the sphere:", free)
    assert (free > 0).all() and (free < 1.0).all()
