"""curobo_amd.perception.mapper.Mapper on the GPU against the float64 oracle tests/mapper_ref.py, on the scene of tests/mapper_cases.py.

What is compared, and why those bounds: which blocks a frame marks is exact outside the oracle's possible-minus-sure set; which
voxels a frame updates is exact on sure blocks outside the oracle's ambiguous voxels; there the stored pair is one fp32 add and
one rounding to fp16 per frame away from the float64 value (the fp32 / float64 gap is far below an fp16 step, so only a near-tie
can land on the neighbour): <= k fp16 steps after k frames.  The seed set, the sign and the squared integer distances of the
nearest-site transform are exact; the fp16 distance is sqrt in fp32 (<= 2.5 ulp of fp32) rounded once: <= 1 fp16 step."""

import numpy as np
import pytest
import torch

import mapper_cases as C
import mapper_ref as R

pytestmark = pytest.mark.gpu


def _cfg(**over):
    from curobo_amd.perception.mapper import MapperCfg

    return MapperCfg(**{**C.CFG, **over})


def _obs(cams, device):
    from curobo_amd.types import CameraObservation, Pose

    depth, K, pos, quat = C.frame(*cams)
    t = lambda a: torch.as_tensor(a, device=device)  # noqa: E731
    return CameraObservation(depth_image=t(depth), intrinsics=t(K), pose=Pose(t(pos), t(quat)))


def _state(mapper):
    t = mapper.tsdf
    data = t.block_data.cpu().numpy()
    return data[..., 0], data[..., 1], t.block_visible.cpu().numpy()[: t.n_blocks] != 0, t.frame_visible.cpu().numpy()[: t.n_blocks] != 0


@pytest.fixture(scope="module")
def grid():
    return R.Grid.from_cfg(_cfg())


@pytest.fixture(scope="module")
def oracle_frames(grid):
    return C.oracle_run(grid)


@pytest.fixture(scope="module")
def device_frames(device):
    """the k = 3 run on the device: the state after every frame"""
    from curobo_amd.perception.mapper import Mapper

    mapper = Mapper(_cfg())
    out = []
    for cams in C.FRAMES:
        mapper.integrate(_obs(cams, device))
        torch.cuda.synchronize()
        out.append(_state(mapper))
    return out


# ---------------------------------------------------------------------------------------------------- 1, 2: integrate
def test_visible_mask(oracle_frames, device_frames):
    ever_sure, ever_possible = False, False
    for k, (ref, (_, _, ever, frame)) in enumerate(zip(oracle_frames, device_frames)):
        sure, possible = ref["sure"], ref["possible"]
        print(f"frame {k}: {int(frame.sum())} blocks on the device, {int(sure.sum())} sure, {int(possible.sum())} possible")
        assert (possible & ~sure).sum() <= 0.01 * possible.sum()
        assert (sure <= frame).all() and (frame <= possible).all()
        ever_sure, ever_possible = ever_sure | sure, ever_possible | possible
        assert (ever_sure <= ever).all() and (ever <= ever_possible).all()
    assert ever_sure.sum() > 300


def test_tsdf_after_one_and_three_frames(grid, oracle_frames, device_frames):
    clean_block = np.ones(grid.n_blocks, bool)   # the block's visibility was certain in every frame so far
    ever_sure = np.zeros(grid.n_blocks, bool)
    amb = np.zeros((grid.n_blocks, grid.bs ** 3), bool)
    prev = (np.zeros_like(amb, np.float16), np.zeros_like(amb, np.float16))
    for k, (ref, (sw, w, _, _)) in enumerate(zip(oracle_frames, device_frames), start=1):
        clean_block &= ref["sure"] | ~ref["possible"]
        ever_sure |= ref["sure"]
        amb |= ref["ambiguous"]
        keep = clean_block[:, None] & ~amb
        excluded = (~keep)[ever_sure].mean()
        assert excluded <= 0.01, f"{excluded:.4f} of the voxels of sure blocks are excluded: change the scene"
        changed = (sw != prev[0]) | (w != prev[1])
        assert np.array_equal(changed[keep], ref["updated"][keep]), "which voxels the frame updated"  # (an update adds weight >= 1)
        steps_sw, steps_w = R.half_steps(sw, ref["sw"])[keep], R.half_steps(w, ref["w"])[keep]
        print(f"after {k} frames: {int(ref['updated'][keep].sum())} voxels updated, excluded {excluded:.4f}, fp16 steps from the oracle: "
              f"sum {int(steps_sw.max())} (differing {float((steps_sw > 0).mean()):.5f}), weight {int(steps_w.max())}")
        assert steps_sw.max() <= k and steps_w.max() <= k
        # untouched voxels of clean blocks are still exactly zero or what they were
        still = keep & ~ref["updated"]
        assert np.array_equal(sw[still], prev[0][still]) and np.array_equal(w[still], prev[1][still])
        prev = (sw, w)
    assert ref["updated"].sum() > 10000 and (np.asarray(oracle_frames[1]["w"], np.float32) > 2.0).any()


# ---------------------------------------------------------------------------------------------------- 3: ESDF stages on injected states
def _inject(mapper, grid, rng, empty=False):
    """a random TSDF written straight into mapper.tsdf, every sdf well away from the seed thresholds 0.9 vs and trunc - 1.1 vs"""
    n, v, vs, tr = grid.n_blocks, grid.bs ** 3, grid.vs, grid.trunc
    kind = rng.integers(0, 6, (n, v))
    lo = np.select([kind == 2, kind == 3, kind == 4, kind == 5], [-0.5 * vs, 1.3 * vs, -tr, -(tr - 1.5 * vs)], 0.0)
    hi = np.select([kind == 2, kind == 3, kind == 4, kind == 5], [0.5 * vs, tr, -(tr - 0.8 * vs), -1.3 * vs], 0.0)
    sdf = lo + (hi - lo) * rng.random((n, v))
    w = np.select([kind == 0, kind == 1], [0.0, 0.0625], rng.integers(1, 40, (n, v)) * 0.5).astype(np.float16)  # 0.0625 <= min weight
    if empty:
        w[:] = 0
    sw = (sdf * w.astype(np.float64)).astype(np.float16)
    visible = rng.random(n) < 0.8
    t = mapper.tsdf
    t.block_data.copy_(torch.as_tensor(np.stack([sw, w], -1)))
    t.block_visible.zero_()
    t.block_visible[:n] = torch.as_tensor(visible.astype(np.uint8))
    return sw, w, visible


@pytest.mark.parametrize("empty", [False, True])
def test_esdf_stages_on_injected_states(grid, device, empty):
    from curobo_amd.backends import mapper as B
    from curobo_amd.perception.mapper import Mapper

    mapper = Mapper(_cfg(), use_graph=False)
    sw, w, visible = _inject(mapper, grid, np.random.default_rng(11), empty)
    vs = C.CFG["esdf_voxel_size"]
    ref = R.esdf(grid, sw, w, visible, C.ESDF_SHAPE, C.ESDF_ORIGIN, vs)
    assert not ref["ambiguous"].any(), "the injected state and the ESDF origin keep every probe and sdf off the thresholds"
    out = mapper.compute_esdf(esdf_origin=torch.tensor(C.ESDF_ORIGIN))
    sites = torch.empty(int(np.prod(C.ESDF_SHAPE)), dtype=torch.int32, device=device)
    t = mapper.tsdf
    B.mapper_esdf_seed(sites, t.block_data, t.block_visible, mapper._esdf_origin, mapper._esdf_voxel_size, t.params, C.ESDF_SHAPE)
    sites = sites.cpu().numpy().reshape(C.ESDF_SHAPE)
    assert np.array_equal(sites >= 0, ref["seed"])
    own = R.pack_sites(np.stack(np.meshgrid(*[np.arange(n) for n in C.ESDF_SHAPE], indexing="ij"), -1))
    assert np.array_equal(sites[sites >= 0], own[sites >= 0]) and (sites[sites < 0] == -1).all()
    dist = out.feature_tensor.cpu().numpy()
    assert dist.dtype == np.float16 and dist.shape == C.ESDF_SHAPE
    if empty:
        assert not ref["seed"].any() and (dist == np.float16(1e4)).all()
        return
    assert 200 < ref["seed"].sum() < ref["seed"].size and ref["inside"].sum() > 100 and (~ref["inside"]).sum() > 100
    assert np.array_equal(np.signbit(dist), ref["inside"]), "negative exactly where the TSDF at the cell's centre is observed and < 0"
    assert R.half_steps(dist, ref["distance"]).max() <= 1


OVERHANG_ESDF_SHAPE = (10, 10, 10)
OVERHANG_ESDF_ORIGIN = (-0.005, -0.005, -0.005)


def _overhanging_state(seed=5):
    """(grid, sw, w, visible): 8^3 voxels of 0.02 m in blocks of 4 about the origin, minimum weight 0.5, every block visible, the
    voxels drawn as ``_inject`` draws them except that the low-weight kind carries weight EXACTLY the minimum (and sdf 0: a seed
    if it were read)"""
    vs, tr = float(np.float32(0.02)), float(np.float32(0.08))
    g = R.Grid(8, 8, 8, 4, [0.0, 0.0, 0.0], vs, tr, 0.1, 5.0, 0.5)
    rng = np.random.default_rng(seed)
    n, v = g.n_blocks, g.bs ** 3
    kind = rng.integers(0, 6, (n, v))
    lo = np.select([kind == 2, kind == 3, kind == 4, kind == 5], [-0.5 * vs, 1.3 * vs, -tr, -(tr - 1.5 * vs)], 0.0)
    hi = np.select([kind == 2, kind == 3, kind == 4, kind == 5], [0.5 * vs, tr, -(tr - 0.8 * vs), -1.3 * vs], 0.0)
    sdf = lo + (hi - lo) * rng.random((n, v))
    w = np.select([kind == 0, kind == 1], [0.0, 0.5], rng.integers(1, 40, (n, v)) * 0.5).astype(np.float16)
    sw = (sdf * w.astype(np.float64)).astype(np.float16)
    return g, sw, w, np.ones(n, bool)


def _overhanging_device(g, sw, w, visible, device):
    from curobo_amd.backends import mapper as B

    p = B.make_params((g.nz, g.ny, g.nx), g.bs, g.origin, g.vs, g.trunc, g.depth_min, g.depth_max, g.min_weight)
    data = torch.as_tensor(np.stack([sw, w], -1), device=device)
    mask = torch.zeros(B.mask_bytes(p), dtype=torch.uint8, device=device)
    mask[: g.n_blocks] = torch.as_tensor(visible.astype(np.uint8), device=device)
    return p, data, mask


def test_esdf_probe_rule_outside_the_grid_and_at_the_minimum_weight(device):
    """The two things the ESDF path's voxel read does otherwise than the mesh and the renderer's, where they show: the ESDF grid
    overhangs the TSDF grid by a cell on every side, its lowest centres at continuous voxel coordinate -0.75, which the cast
    toward zero puts in voxel 0 (floor: outside, builder_esdf.py:279-282); and a sixth of the voxels weigh exactly the minimum,
    which ``>`` leaves unobserved (wp_tsdf_sample.py:49; ``>=`` would seed at each: their sdf is 0).  Measured on the oracle for
    this draw of the state (seed 5, drawn as ``_overhanging_state`` does): 640 of the 1000 cells are seeds and 300 inside; floor changes 172 seed cells, ``>=`` 164 and 97 occupied flags."""
    from curobo_amd.backends import mapper as B

    g, sw, w, visible = _overhanging_state()
    shape, origin = OVERHANG_ESDF_SHAPE, OVERHANG_ESDF_ORIGIN
    lowest = (R.esdf_centres(shape, origin, g.vs)[0, 0, 0] - np.asarray(g.origin)) / g.vs + 0.5 * g.nx
    assert np.allclose(lowest, -0.75, atol=1e-6) and (w == np.float16(g.min_weight)).sum() > 50
    ref = R.esdf(g, sw, w, visible, shape, origin, g.vs)
    assert not ref["ambiguous"].any(), "the injected state and the ESDF origin keep every probe and sdf off the thresholds"
    p, data, mask = _overhanging_device(g, sw, w, visible, device)
    n = int(np.prod(shape))
    o, vs = torch.tensor(origin, device=device), torch.tensor([g.vs], dtype=torch.float32, device=device)
    sites = torch.empty(n, dtype=torch.int32, device=device)
    B.mapper_esdf_seed(sites, data, mask, o, vs, p, shape)
    got = sites.cpu().numpy().reshape(shape)
    assert np.array_equal(got >= 0, ref["seed"])
    own = R.pack_sites(np.stack(np.meshgrid(*[np.arange(k) for k in shape], indexing="ij"), -1))
    assert np.array_equal(got[got >= 0], own[got >= 0]) and (got[got < 0] == -1).all()
    nearest = B.mapper_edt(sites, torch.empty_like(sites), shape)
    out = torch.zeros(n, dtype=torch.float16, device=device)
    B.mapper_esdf_distance(out, nearest, data, mask, o, vs, p, shape)
    dist = out.cpu().numpy().reshape(shape)
    assert 200 < ref["seed"].sum() < ref["seed"].size and ref["inside"].sum() > 100 and (~ref["inside"]).sum() > 100
    assert np.array_equal(np.signbit(dist), ref["inside"]), "negative exactly where the TSDF at the cell's centre is observed and < 0"
    assert R.half_steps(dist, ref["distance"]).max() <= 1
    for kw in (dict(), dict(surface_only=True)):
        flags = torch.full((g.n_blocks * g.bs ** 3,), 7, dtype=torch.uint8, device=device)
        B.mapper_occupied_flags(flags, data, mask, p, kw.get("surface_only", False), g.vs)
        want = R.occupied(g, sw, w, visible, **kw)
        assert want.sum() > 50 and np.array_equal(flags.cpu().numpy().reshape(want.shape) != 0, want)


# ---------------------------------------------------------------------------------------------------- 4: the nearest-site transform
def _site_sets(shape, rng):
    cells = int(np.prod(shape))
    none = np.zeros(shape, bool)
    corner = none.copy()
    corner[-1, -1, -1] = True
    origin = none.copy()
    origin[0, 0, 0] = True
    plane = none.copy()
    plane[:, shape[1] // 2, :] = True
    tie = none.copy()          # two seeds as far apart as the grid allows: every cell between them chooses, many at a tie
    tie[0, 0, 0] = tie[-1, 0, 0] = True
    envelope = none.copy()     # seeds on a parabola-like stair: every line's lower envelope has many short pieces
    for x in range(shape[0]):
        envelope[x, (x * x) % shape[1], (3 * x) % shape[2]] = True
    sets = {"none": none, "corner": corner, "origin": origin, "all": np.ones(shape, bool), "plane": plane, "tie": tie, "envelope": envelope,
            "sparse": rng.random(shape) < max(2.0 / cells, 0.002), "medium": rng.random(shape) < 0.03}
    if cells <= 4096:
        sets["dense"] = rng.random(shape) < 0.5
    return sets


@pytest.mark.parametrize("shape", [(5, 7, 9), (16, 16, 16), (33, 20, 17), (64, 8, 8), (1024, 2, 2)])
def test_nearest_site_transform_is_exact(shape, device):
    from curobo_amd.backends import mapper as B

    rng = np.random.default_rng(sum(shape))
    cells = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1)
    own = R.pack_sites(cells)
    n = int(np.prod(shape))
    for name, seeds in _site_sets(shape, rng).items():
        a = torch.as_tensor(np.where(seeds, own, -1).astype(np.int32).reshape(-1), device=device)
        b = torch.full((n,), -7, dtype=torch.int32, device=device)
        packed = B.mapper_edt(a, b, shape).cpu().numpy().reshape(shape)
        want = R.edt_brute(seeds)
        if not seeds.any():
            assert (packed == -1).all(), name
            continue
        assert (packed >= 0).all(), name
        site = R.unpack_sites(packed)
        assert (site < np.array(shape)).all() and seeds[tuple(site[..., k] for k in range(3))].all(), f"{name}: every returned site is a seed"
        d2 = ((cells - site) ** 2).sum(-1)
        assert np.array_equal(d2, want), f"{name}: squared distance to the returned site against brute force"
        if name == "all":
            assert np.array_equal(packed, own)
        if name == "corner":  # (for 1024 cells along x: the top coordinate of the 10-bit packing)
            assert (site == np.array(shape) - 1).all()


@pytest.mark.parametrize("shape", [(5, 7, 9), (33, 20, 17), (1024, 2, 2)])
def test_distance_field_of_injected_sites(shape, grid, device):
    """stage 3 on sites that the transform produced from injected seeds, over an empty TSDF (every cell outside): the fp16 field
    against the oracle's, 1e4 exact where there is no site"""
    from curobo_amd.backends import mapper as B

    rng = np.random.default_rng(3)
    p = B.make_params((grid.nz, grid.ny, grid.nx), grid.bs, grid.origin, grid.vs, grid.trunc, grid.depth_min, grid.depth_max, grid.min_weight)
    data = torch.zeros((p.n_blocks, p.block_voxels, 2), dtype=torch.float16, device=device)
    mask = torch.zeros(B.mask_bytes(p), dtype=torch.uint8, device=device)
    origin, vs = torch.tensor(C.ESDF_ORIGIN, device=device), torch.tensor([0.04], device=device)
    n = int(np.prod(shape))
    for seeds in (rng.random(shape) < 0.004, np.zeros(shape, bool)):
        d2, site = R.edt(seeds)
        out = torch.zeros(n, dtype=torch.float16, device=device)
        B.mapper_esdf_distance(out, torch.as_tensor(R.pack_sites(site).reshape(-1), device=device), data, mask, origin, vs, p, shape)
        want = np.where(d2 < 0, 1e4, np.sqrt(np.maximum(d2, 0)) * float(np.float32(0.04))).astype(np.float16)
        got = out.cpu().numpy().reshape(shape)
        assert np.array_equal(got == np.float16(1e4), d2 < 0) and not np.signbit(got).any()
        assert R.half_steps(got, want).max() <= 1


# ---------------------------------------------------------------------------------------------------- 5: end to end
def test_end_to_end_into_a_scene(grid, oracle_frames, device):
    from curobo_amd.backends import collision as Cn
    from curobo_amd.perception.mapper import Mapper
    from curobo_amd.scene import SceneData, cuboid_scene_arrays, voxel_grid_from_sdf

    mapper = Mapper(_cfg())
    mapper.integrate(_obs(C.FRAMES[0], device))
    out = mapper.compute_esdf(esdf_origin=torch.tensor(C.ESDF_ORIGIN))
    vs = C.CFG["esdf_voxel_size"]
    assert out.name == "block_sparse_esdf_grid" and out.voxel_size == vs and out.get_grid_shape()[0] == list(C.ESDF_SHAPE)
    assert out.pose == pytest.approx([*C.ESDF_ORIGIN, 1, 0, 0, 0]) and out.feature_tensor.dtype == torch.float16
    # the oracle's ESDF stages on the device's own TSDF (its differences from the oracle's are the subject of the tests above)
    sw, w, ever, _ = _state(mapper)
    ref0 = oracle_frames[0]
    assert (ref0["sure"] <= ever).all() and (ever <= ref0["possible"]).all()
    ref = R.esdf(grid, sw, w, ever, C.ESDF_SHAPE, C.ESDF_ORIGIN, vs)
    ok = ~ref["ambiguous"]  # (real data may put an sdf within 1e-6 m of a seed threshold; no probe is near a voxel face)
    assert ok.mean() >= 0.99
    from curobo_amd.backends import mapper as B

    t = mapper.tsdf
    sites = torch.empty(int(np.prod(C.ESDF_SHAPE)), dtype=torch.int32, device=device)
    B.mapper_esdf_seed(sites, t.block_data, t.block_visible, mapper._esdf_origin, mapper._esdf_voxel_size, t.params, C.ESDF_SHAPE)
    seeds = sites.cpu().numpy().reshape(C.ESDF_SHAPE) >= 0
    assert np.array_equal(seeds[ok], ref["seed"][ok])
    d2, _ = R.edt(seeds)  # the transform and the distance over the device's seed set (it may differ on a flagged cell)
    want, inside = R.distance(grid, sw, w, ever, d2, C.ESDF_ORIGIN, vs)
    dist = out.feature_tensor.cpu().numpy()
    assert np.array_equal(np.signbit(dist), inside) and R.half_steps(dist, want).max() <= 1
    assert ref["seed"].sum() > 500 and ref["inside"].sum() > 100
    # ... and into a scene whose voxel store was built with a grid of that name and shape
    table = {"dims": [0.2, 0.2, 0.2], "pose": [0.0, 0.0, -5.0, 1, 0, 0, 0], "name": "far"}
    empty = voxel_grid_from_sdf(lambda p: np.full(len(p), 1.0), C.ESDF_SHAPE, vs, pose7=[0, 0, 0, 1, 0, 0, 0], max_distance=10.0,
                                name="block_sparse_esdf_grid")
    scene = SceneData.from_arrays({**cuboid_scene_arrays([[table]]), **empty}, device)
    toward = np.asarray(C.EYES[0][0]) / np.linalg.norm(C.EYES[0][0])
    spheres = np.array([[*(R.SPHERE_RADIUS * toward), 0.03], [*((R.SPHERE_RADIUS + 0.3) * toward), 0.03]], np.float32)  # surface; free space
    sph = torch.as_tensor(spheres, device=device).reshape(1, 1, 2, 4)

    def query():
        d, g = torch.full((1, 1, 2), 3.0, device=device), torch.full((1, 1, 2, 4), 3.0, device=device)
        Cn.sphere_obstacle_collision(d, g, sph, scene.struct, torch.tensor([1.0], device=device), torch.tensor([0.02], device=device), None, 1, 1, 2,
                                     False)
        torch.cuda.synchronize()
        return d.cpu().numpy().reshape(2)

    assert (query() == 0).all(), "nothing collides with the empty grid"
    scene.update_voxel_data(out)
    d = query()
    print("penetration of the sphere at the surface and of the one 0.3 m in front of it:", d)
    assert d[0] > 0 and d[1] == 0


# ---------------------------------------------------------------------------------------------------- 6: capture
def test_compute_esdf_replays_its_graph(device):
    from curobo_amd.perception.mapper import Mapper

    graphed, eager = Mapper(_cfg()), Mapper(_cfg(), use_graph=False)
    origin = torch.tensor(C.ESDF_ORIGIN)
    results = []
    for k, cams in enumerate(((0,), (2,))):
        fields = []
        for m in (graphed, eager):
            m.integrate(_obs(cams, device))
            out = m.compute_esdf(esdf_origin=origin) if k == 0 else m.compute_esdf()
            torch.cuda.synchronize()
            fields.append(out.feature_tensor)
        assert torch.equal(fields[0].view(torch.int16), fields[1].view(torch.int16)), "replay and plain launches agree bit for bit"
        results.append((fields[0].data_ptr(), fields[0].clone()))
    assert graphed._graph is not None and eager._graph is None
    assert results[0][0] == results[1][0], "the returned tensor is the mapper's own buffer"
    assert not torch.equal(results[0][1], results[1][1]), "the second frame changed the field"
    # a moved window is read from the device tensors by the same graph
    g = graphed._graph
    moved = [a + 0.08 for a in C.ESDF_ORIGIN]
    a, b = graphed.compute_esdf(esdf_origin=torch.tensor(moved)), eager.compute_esdf(esdf_origin=torch.tensor(moved))
    torch.cuda.synchronize()
    assert graphed._graph is g and a.pose[:3] == pytest.approx(moved)
    assert torch.equal(a.feature_tensor.view(torch.int16), b.feature_tensor.view(torch.int16))
    assert not torch.equal(a.feature_tensor, results[1][1])


# ---------------------------------------------------------------------------------------------------- 7: editing and read-outs
def _voxel_index(centres, grid):
    g = (np.asarray(centres, np.float64) - np.asarray(grid.origin)) / grid.vs + 0.5 * np.array([grid.nx, grid.ny, grid.nz]) - 0.5
    assert np.abs(g - np.rint(g)).max() < 1e-3
    return {tuple(v) for v in np.rint(g).astype(int)}


def test_clear_region_reset_and_occupied_voxels(grid, device):
    from curobo_amd.perception.mapper import Mapper

    mapper = Mapper(_cfg())
    mapper.integrate(_obs(C.FRAMES[1], device))
    sw, w, ever, _ = _state(mapper)
    nbx, nby, _ = grid.nb
    for kw in (dict(), dict(surface_only=True), dict(surface_only=True, sdf_threshold=0.011)):
        want = R.occupied(grid, sw, w, ever, **kw)
        b, loc = np.nonzero(want)
        idx = np.stack([(b % nbx) * grid.bs + loc % grid.bs, ((b // nbx) % nby) * grid.bs + (loc // grid.bs) % grid.bs,
                        (b // (nbx * nby)) * grid.bs + loc // (grid.bs * grid.bs)], -1)
        got = mapper.extract_occupied_voxels(**kw).cpu().numpy()
        assert got.shape == (int(want.sum()), 3) and want.sum() > 200
        assert _voxel_index(got, grid) == {tuple(v) for v in idx}
    stats = mapper.get_stats()
    assert stats["frame_count"] == 1 and stats["visible_blocks"] == int(ever.sum()) and stats["total_blocks"] == grid.n_blocks
    assert mapper.memory_usage_mb() > grid.n_blocks * 64 * 4 / 2 ** 20
    mapper.compute_esdf()
    assert mapper._last_voxel_grid is not None
    lo, hi = (-0.1, -0.1, -0.2), (0.13, 0.05, 0.0)
    touched = R.blocks_touching(grid, lo, hi)
    assert 0 < (touched & ever).sum() < ever.sum() and (touched & ~ever).any()
    assert mapper.clear_region(lo, hi) == int((touched & ever).sum())
    assert mapper._last_voxel_grid is None
    sw2, w2, ever2, _ = _state(mapper)
    assert np.array_equal(ever2, ever), "cleared blocks stay ever-visible"
    assert not sw2[touched].any() and not w2[touched].any()
    assert np.array_equal(sw2[~touched], sw[~touched]) and np.array_equal(w2[~touched], w[~touched])
    assert mapper.clear_region((5.0, 5.0, 5.0), (6.0, 6.0, 6.0)) == 0
    mapper.reset()
    sw3, w3, ever3, frame3 = _state(mapper)
    assert not sw3.any() and not w3.any() and not ever3.any() and not frame3.any() and mapper.get_stats()["frame_count"] == 0
    assert mapper.extract_occupied_voxels().shape == (0, 3)
    assert (mapper.compute_esdf().feature_tensor == 1e4).all()


def test_integrate_argument_forms(device):
    from curobo_amd.perception.mapper import Mapper

    mapper = Mapper(_cfg())
    obs = _obs((0,), device)
    mapper.integrate(obs)
    mapper.integrate(camera_observation=obs)
    mapper.integrate(observation=obs)
    assert mapper.get_stats()["frame_count"] == 3
    with pytest.raises(TypeError):
        mapper.integrate()
    with pytest.raises(TypeError):
        mapper.integrate(obs, camera_observation=obs)
    with pytest.raises(TypeError):
        mapper.integrate(3.0)
    with pytest.raises(NotImplementedError, match="lidar"):
        mapper.integrate(lidar_observation=object())
    with pytest.raises(ValueError, match="depth_image"):
        mapper.integrate(_obs((0, 1, 2), device))  # three cameras into a mapper configured for two
