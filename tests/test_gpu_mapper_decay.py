"""The mapper's weight decay and block recycling on the GPU (csrc/mapper.hip: curobo_hip_mapper_decay) against the restatement
tests/mapper_decay_ref.py, on the scene of tests/mapper_cases.py with the cameras of tests/mapper_decay_cases.py.

What is compared, and why those bounds.  The decay is one fp32 product per word, rounded to fp16: the restatement forms it with
torch on the CPU in the reference's own expressions, FROM THE DEVICE'S STATE before the launch, and the words are compared bit for
bit.  Which blocks are in the frusta is exact on the restatement's sure blocks; an *either* block (a compared quantity within 1e-5 m
or 1e-3 px of its bound) must carry one of the two factors as a whole.  Which blocks are recycled is exact, because every test first
asserts that no block sum lies within 1e-4 relative of the threshold (the fp32 sum of a block is within 2e-6 of the float64 one).
An integration that follows a decay is held to the oracle's integration of that frame from the decayed state under the comparison
of tests/test_gpu_mapper.py for one frame: the updated voxels exact and the pair within one fp16 step on sure blocks outside the
oracle's ambiguous voxels.  tests/test_mapper_decay_host.py asserts, without a GPU, that the scene meets these conditions."""

import numpy as np
import pytest
import torch

import mapper_cases as C
import mapper_decay_cases as DC
import mapper_decay_ref as DR
import mapper_ref as R

pytestmark = pytest.mark.gpu


def _cfg(block_size=4):
    from curobo_amd.perception.mapper import MapperCfg

    return MapperCfg(**DC.cfg_dict(block_size))


def _obs(f, device):
    from curobo_amd.types import CameraObservation, Pose

    depth, K, pos, quat = f
    t = lambda a: torch.as_tensor(a, device=device)  # noqa: E731
    return CameraObservation(depth_image=t(depth), intrinsics=t(K), pose=Pose(t(pos), t(quat)))


def _snap(mapper):
    """(fp16 [n_blocks, bs^3, 2], visible, frame, recycled) on the host"""
    torch.cuda.synchronize()
    t = mapper.tsdf
    mask = lambda m: m.cpu().numpy()[: t.n_blocks] != 0  # noqa: E731
    return t.block_data.cpu().numpy(), mask(t.block_visible), mask(t.frame_visible), mask(t.block_recycled)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _assert_same_words(got, want, before, what):
    """bit for bit, and on a mismatch which words: (block, voxel, word), the word before, the device's and the restatement's"""
    bad = np.argwhere(_bits(got) != _bits(want))
    for i in map(tuple, bad[:8]):
        print(f"{what}: word {i}: before {before[i]!r} ({_bits(before)[i]:#06x}), device {got[i]!r} ({_bits(got)[i]:#06x}), "
              f"restatement {want[i]!r} ({_bits(want)[i]:#06x})")
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} words differ from the restatement"


def _after_frames(block_size, device, **kw):
    from curobo_amd.perception.mapper import Mapper

    mapper = Mapper(_cfg(block_size), **kw)
    for cams in C.FRAMES:
        mapper.integrate(_obs(C.frame(*cams), device))
    return mapper


def _check_integration(g, start, after, f, exclude=None, what=""):
    """the device's integration of frame ``f`` from the state ``start`` (which the device held bit for bit) against the oracle's"""
    data0, visible0 = start
    data1, visible1, frame1, _ = after
    sure, possible = R.mark_blocks(g, *f)
    assert (possible & ~sure).sum() <= 0.01 * possible.sum()
    assert (sure <= frame1).all() and (frame1 <= possible).all(), what
    ok = np.ones(g.n_blocks, bool) if exclude is None else ~exclude
    assert np.array_equal(visible1[ok], (visible0 | frame1)[ok]), what
    sw, w, upd, amb = R.integrate(g, data0[..., 0], data0[..., 1], sure, *f)
    keep = (ok & (sure | ~possible))[:, None] & ~amb
    assert (~keep)[sure].mean() <= 0.01
    changed = (_bits(data1[..., 0]) != _bits(data0[..., 0])) | (_bits(data1[..., 1]) != _bits(data0[..., 1]))
    assert np.array_equal(changed[keep], upd[keep]), f"{what}: which voxels the frame updated"
    steps = max(R.half_steps(data1[..., 0], sw)[keep].max(), R.half_steps(data1[..., 1], w)[keep].max())
    print(f"{what}: {int(upd[keep].sum())} voxels updated, at most {int(steps)} fp16 steps from the oracle")
    assert steps <= 1 and upd[keep].sum() > 1000


# ---------------------------------------------------------------------------------------------------- 1: the uniform path
@pytest.mark.parametrize("block_size", DC.BLOCK_SIZES)
def test_uniform_decay_is_torch_bit_for_bit(block_size, device):
    """After the three frames the map holds blocks that a frame marked and gave no weight (behind the surface by more than the
    truncation distance: 87 of 2521, 4 of 431 and 0 of 74 on the oracle at blocks of 2, 4, 8).  Their sum is 0, below any threshold, so ANY recycle launch frees them,
    as the reference's does; recycle_empty_blocks() takes them out first (test 3 holds that call to the restatement), so that this
    test's subject is the decay alone: the words bit for bit, the masks unchanged, the call returning 0."""
    mapper = _after_frames(block_size, device)
    mapper.recycle_empty_blocks()
    data, visible, frame, _ = _snap(mapper)
    want, visible_ref, recycled_ref, either = DR.step_uniform(data, visible, block_size, 0.9)
    assert not either.any() and not recycled_ref.any() and visible.sum() >= 60
    mapper.compute_esdf()
    assert mapper._last_voxel_grid is not None
    assert mapper.decay_and_recycle(0.9) == 0 and mapper._last_voxel_grid is None
    got, visible1, frame1, recycled1 = _snap(mapper)
    _assert_same_words(got, want, data, "decay_and_recycle(0.9)")
    assert (_bits(got) != _bits(data)).mean() > 0.05
    assert np.array_equal(visible1, visible) and np.array_equal(frame1, frame) and not recycled1.any()
    assert not got[~visible].any(), "never-visible blocks stay zero"


# ---------------------------------------------------------------------------------------------------- 2: the frustum path
@pytest.mark.parametrize("block_size", DC.BLOCK_SIZES)
def test_frustum_decay_gives_each_block_its_factor(block_size, device):
    from curobo_amd.perception.mapper import decay_frustum_aware_multi_camera

    mapper = _after_frames(block_size, device)
    data, visible, frame, _ = _snap(mapper)
    sure_in, sure_out = DC.frustum_sets(block_size)
    either = ~sure_in & ~sure_out
    assert (either & visible).sum() <= 0.01 * visible.sum() and (sure_in & visible).sum() >= 20 and (sure_out & visible).sum() >= 20
    as_in = DR.step_frame(data, visible, block_size, np.ones_like(visible), DC.TIME_DECAY, DC.FRUSTUM_DECAY)
    as_out = DR.step_frame(data, visible, block_size, np.zeros_like(visible), DC.TIME_DECAY, DC.FRUSTUM_DECAY)
    assert not as_in[3].any() and not as_out[3].any() and np.array_equal(as_in[2], as_out[2]), "no block sum near the threshold under either factor"
    gone = as_in[2]  # (blocks that were marked and never received weight: sum 0)
    assert not data[gone, :, 1].any() and gone.sum() <= 0.05 * visible.sum()
    K, pos, quat = (torch.as_tensor(a, device=device) for a in DC.frustum_cameras())
    out = decay_frustum_aware_multi_camera(mapper.tsdf, K, pos, quat, (C.H, C.W), *DC.FRUSTUM_DEPTH, time_decay=DC.TIME_DECAY,
                                           frustum_decay=DC.FRUSTUM_DECAY, num_blocks=17)
    assert out is None
    got, visible1, frame1, recycled1 = _snap(mapper)
    is_in = (_bits(got) == _bits(as_in[0])).all((1, 2))
    is_out = (_bits(got) == _bits(as_out[0])).all((1, 2))
    differ = (_bits(as_in[0]) != _bits(as_out[0])).any((1, 2))
    assert differ[visible].mean() > 0.9, "the two factors give different words in nearly every visible block"
    assert is_in[sure_in].all(), "every sure-in block carries the in factor"
    assert is_out[sure_out].all(), "every sure-out block carries the out factor"
    assert (is_in | is_out)[either].all(), "an either block carries one of the two, as a whole"
    print(f"block size {block_size}: {int((sure_in & visible).sum())} visible blocks sure in, {int((sure_out & visible).sum())} sure out, "
          f"{int((either & visible).sum())} either")
    assert not got[~visible].any(), "never-visible blocks stay all zero"
    assert np.array_equal(visible1, visible & ~gone) and np.array_equal(recycled1, gone) and np.array_equal(frame1, frame)


# ---------------------------------------------------------------------------------------------------- 3: recycling
@pytest.mark.parametrize("block_size", DC.BLOCK_SIZES)
def test_blocks_are_recycled_as_the_restatement_says(block_size, device):
    mapper = _after_frames(block_size, device)
    data, visible, frame, _ = _snap(mapper)
    # nothing below the threshold but the blocks that were marked and received no weight: they go, and a second call changes no byte
    _, _, empty, either = DR.recycle(data, visible, block_size)
    assert not either.any()
    assert mapper.recycle_empty_blocks() == int(empty.sum())
    data, visible, _, recycled = _snap(mapper)
    assert np.array_equal(recycled, empty) and not (visible & empty).any()
    assert mapper.recycle_empty_blocks() == 0
    again = _snap(mapper)
    assert np.array_equal(_bits(again[0]), _bits(data)) and np.array_equal(again[1], visible) and not again[3].any()
    steps, stepped = 0, []
    while visible.any():
        want, visible_ref, recycled_ref, either = DR.step_uniform(data, visible, block_size, 0.5)
        assert not either.any(), f"step {steps}: a block sum within 1e-4 of the threshold"
        count = mapper.decay_and_recycle(0.5)
        got, visible1, frame1, recycled1 = _snap(mapper)
        assert np.array_equal(recycled1, recycled_ref), f"step {steps}: the recycled set"
        assert np.array_equal(visible1, visible_ref) and not got[recycled_ref].any(), "recycled blocks have mask 0 and all-zero words"
        assert count == int(recycled_ref.sum()) == mapper.get_stats()["recycled_blocks"]
        _assert_same_words(got, want, data, f"step {steps}: kept blocks bit for bit, recycled ones zero")
        assert np.array_equal(frame1, frame), "frame_visible is not touched"
        stepped.append(count)
        data, visible, steps = got, visible1, steps + 1
        assert steps <= 40
    print(f"block size {block_size}: recycled per step {stepped}")
    assert sum(1 for c in stepped if c) >= 3 and mapper.get_stats()["visible_blocks"] == 0 and not data.any()


# ---------------------------------------------------------------------------------------------------- 4: re-observation
def test_a_recycled_block_is_integrated_as_an_empty_one(device):
    from curobo_amd.perception.mapper import Mapper

    g = DC.grid()
    mapper = Mapper(_cfg())
    f = C.frame(0)
    mapper.integrate(_obs(f, device))
    first = _snap(mapper)
    for _ in range(8):
        if mapper.get_stats()["visible_blocks"] == 0:
            break
        mapper.decay_and_recycle(0.01)
    data, visible, _, _ = _snap(mapper)
    assert not visible.any() and not data.any(), "everything the frame saw was recycled"
    mapper.integrate(_obs(f, device))
    again = _snap(mapper)
    _check_integration(g, (np.zeros_like(data), np.zeros_like(visible)), again, f, what="the frame again, after recycling")
    assert np.array_equal(_bits(again[0]), _bits(first[0])) and np.array_equal(again[1], first[1]), "and exactly as into a new map"


# ---------------------------------------------------------------------------------------------------- 5: the per-frame path
def test_integrate_decays_before_every_frame_but_the_first(device):
    from curobo_amd.backends import mapper as B
    from curobo_amd.perception.mapper import Mapper

    g = DC.grid()
    frames = [C.frame(*cams) for cams in C.FRAMES]
    mapper, plain = Mapper(_cfg(), time_decay=0.9, frustum_decay=0.5), Mapper(_cfg())
    mapper.integrate(_obs(frames[0], device))
    plain.integrate(_obs(frames[0], device))
    cur, first = _snap(mapper), _snap(plain)
    assert np.array_equal(_bits(cur[0]), _bits(first[0])) and np.array_equal(cur[1], first[1]), "no decay before the first frame"
    for k in (1, 2):
        data, visible = cur[0], cur[1]
        sure_in, sure_out = DR.frustum_flags(g, *frames[k][1:], C.H, C.W, g.depth_min, g.depth_max)
        either_f = visible & ~sure_in & ~sure_out
        assert either_f.sum() <= 0.01 * visible.sum()
        start, start_visible, recycled, either_s = DR.step_frame(data, visible, g.bs, sure_in, 0.9, 0.5)
        assert not either_s.any()
        mapper.integrate(_obs(frames[k], device))
        cur = _snap(mapper)
        assert np.array_equal(cur[3][~either_f], recycled[~either_f]) and mapper.get_stats()["recycled_blocks"] == int(cur[3].sum())
        _check_integration(g, (start, start_visible), cur, frames[k], exclude=either_f, what=f"frame {k} after its decay")
        plain.integrate(_obs(frames[k], device))
    assert (_bits(cur[0]) != _bits(_snap(plain)[0])).mean() > 0.05, "the decayed map differs from the plain one"
    # reset(): the next frame is a first frame again
    mapper.reset()
    assert mapper.get_stats()["recycled_blocks"] == 0
    mapper.integrate(_obs(frames[0], device))
    cur = _snap(mapper)
    assert np.array_equal(_bits(cur[0]), _bits(first[0])) and np.array_equal(cur[1], first[1]) and np.array_equal(cur[2], first[2])
    # default factors: bit-identical to the three launches called directly, which never touch the new code
    p = plain.tsdf.params
    raw = torch.zeros_like(plain.tsdf.block_data)
    ever, now = torch.zeros_like(plain.tsdf.block_visible), torch.zeros_like(plain.tsdf.block_visible)
    for f in frames:
        depth, K, pos, quat = (torch.as_tensor(a, device=device).contiguous() for a in f)
        B.mapper_clear_mask(now)
        B.mapper_mark_blocks(now, ever, depth, K, pos, quat, p)
        B.mapper_integrate(raw, now, depth, K, pos, quat, p)
    torch.cuda.synchronize()
    t = plain.tsdf
    assert torch.equal(t.block_data.view(torch.int16), raw.view(torch.int16)) and torch.equal(t.block_visible, ever) and torch.equal(t.frame_visible, now)
    assert not t.block_recycled.any() and plain.get_stats()["recycled_blocks"] == 0


# ---------------------------------------------------------------------------------------------------- 6: forgetting, end to end
def _in_box(points):
    return (np.abs(points) <= R.SPHERE_RADIUS).all(-1)


def _read_outs(mapper, device):
    """(negative ESDF cells, seed cells, mesh vertices) inside the sphere's bounding box"""
    from curobo_amd.backends import mapper as B

    out = mapper.compute_esdf(esdf_origin=torch.tensor(C.ESDF_ORIGIN))
    t = mapper.tsdf
    sites = torch.empty(int(np.prod(C.ESDF_SHAPE)), dtype=torch.int32, device=device)
    B.mapper_esdf_seed(sites, t.block_data, t.block_visible, mapper._esdf_origin, mapper._esdf_voxel_size, t.params, C.ESDF_SHAPE)
    torch.cuda.synchronize()
    box = _in_box(R.esdf_centres(C.ESDF_SHAPE, C.ESDF_ORIGIN, C.CFG["esdf_voxel_size"]))
    dist = out.feature_tensor.cpu().numpy()
    vertices = mapper.extract_mesh().vertices.cpu().numpy()
    return int((np.signbit(dist) & box).sum()), int(((sites.cpu().numpy().reshape(C.ESDF_SHAPE) >= 0) & box).sum()), int(_in_box(vertices).sum())


def test_what_is_no_longer_seen_is_forgotten(device):
    from curobo_amd.perception.mapper import Mapper

    n = DC.forgetting()["frames"]  # (the restatement's count; tests/test_mapper_decay_host.py holds it to 10 .. 30)
    box = DC.sphere_blocks()
    forgetful, keeper = Mapper(_cfg(), time_decay=DC.FORGET_TIME_DECAY), Mapper(_cfg())
    assert forgetful._use_graph
    for m in (forgetful, keeper):
        m.integrate(_obs(C.frame(0), device))
    assert (_snap(forgetful)[1] & box).sum() > 100
    seen = _read_outs(forgetful, device)  # (records the ESDF graph before the map changes)
    assert min(seen) > 0, seen
    turned = _obs(DC.turned_frame(), device)
    for _ in range(n):
        for m in (forgetful, keeper):
            m.integrate(turned)
    data, visible, frame, _ = _snap(forgetful)
    assert np.array_equal(visible, frame) and 20 <= frame.sum() <= 30, "visible_blocks holds the blocks of the current view only"
    assert not (visible & box).any() and not data[~visible].any() and forgetful.get_stats()["visible_blocks"] == int(frame.sum())
    assert _read_outs(forgetful, device) == (0, 0, 0), "no negative cell, no site and no vertex within the sphere's bounding box"
    kept = _snap(keeper)
    assert (kept[1] & box).sum() > 100 and np.array_equal(kept[2], frame)
    still = _read_outs(keeper, device)
    print(f"after {n} turned frames: without decay {still} negative cells, seeds and vertices at the sphere, with decay none")
    assert min(still) > 0


# ---------------------------------------------------------------------------------------------------- 7: graph safety
def test_the_decay_launch_replays_from_a_graph(device):
    from curobo_amd.backends import mapper as B
    from curobo_amd.util.graph_capture import capture_graph

    eager, graphed = _after_frames(4, device), _after_frames(4, device)
    cams = tuple(torch.as_tensor(a, device=device) for a in DC.frustum_cameras())
    thr = B.decay_empty_threshold(4)

    def launch(m):
        t = m.tsdf
        B.mapper_decay(t.block_data, t.block_visible, t.block_recycled, t.params, 0.5, 0.25, thr, *cams, image_shape=(C.H, C.W))

    t = graphed.tsdf
    graph, _ = capture_graph(lambda: launch(graphed), restore=[t.block_data, t.block_visible, t.block_recycled], device=torch.device(device))
    before = _snap(graphed)
    assert np.array_equal(_bits(before[0]), _bits(_snap(eager)[0])), "the recording left the map as it was"
    for k in range(2):
        launch(eager)
        graph.replay()
        a, b = _snap(eager), _snap(graphed)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), f"call {k}"
    assert (_bits(b[0]) != _bits(before[0])).mean() > 0.05
