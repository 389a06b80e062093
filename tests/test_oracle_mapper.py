"""tests/mapper_ref.py against itself: the separable nearest-site transform against brute force, the seed and sign rules on
hand-made TSDF states, and the whole pipeline's ESDF against the analytic distance of the scene it was rendered from.  This
establishes that the oracle the device is held to (tests/test_gpu_mapper.py) is plausible; it runs no device code."""

import numpy as np
import pytest

import mapper_cases as C
import mapper_ref as R


@pytest.mark.parametrize("shape", [(5, 7, 9), (16, 16, 16), (33, 20, 17), (64, 8, 8), (1024, 2, 2)])
@pytest.mark.parametrize("density", [0.002, 0.05, 0.5])
def test_separable_transform_is_exact(shape, density):
    rng = np.random.default_rng(hash((shape, density)) % 2 ** 32)
    seeds = rng.random(shape) < density
    d2, site = R.edt(seeds)
    assert np.array_equal(d2, R.edt_brute(seeds))
    if seeds.any():
        cells = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1)
        assert seeds[tuple(site[..., a] for a in range(3))].all(), "every site is a seed"
        assert np.array_equal(((cells - site) ** 2).sum(-1), d2)
    else:
        assert (d2 == -1).all() and (site == -1).all()


def test_transform_edge_site_sets():
    shape = (6, 5, 4)
    none = np.zeros(shape, bool)
    assert (R.edt(none)[0] == -1).all()
    corner = none.copy()
    corner[5, 4, 3] = True
    d2, site = R.edt(corner)
    assert d2[0, 0, 0] == 25 + 16 + 9 and (site == [5, 4, 3]).all()
    assert (R.edt(np.ones(shape, bool))[0] == 0).all()
    plane = none.copy()
    plane[:, 2, :] = True
    assert np.array_equal(R.edt(plane)[0], np.broadcast_to(((np.arange(5) - 2) ** 2)[None, :, None], shape))
    assert np.array_equal(R.unpack_sites(R.pack_sites(site)), site)
    assert R.pack_sites(np.array([[1023, 1023, 1023]]))[0] == 0x3fffffff


def _small_grid():
    # 8 x 8 x 8 voxels of 0.02 in blocks of 4; ESDF cells of 0.02 centred a quarter voxel off, so cell i probes voxel i
    g = R.Grid(8, 8, 8, 4, [0.0, 0.0, 0.0], 0.02, 0.08, 0.1, 5.0, 0.1)
    return g, np.zeros((8, 64), np.float16), np.zeros((8, 64), np.float16), np.ones(8, bool)


def _put(g, sw, w, voxel, sdf, weight=1.0):
    x, y, z = voxel
    b = ((z // 4) * 2 + y // 4) * 2 + x // 4
    loc = ((z % 4) * 4 + y % 4) * 4 + x % 4
    sw[b, loc], w[b, loc] = sdf * weight, weight
    return b


def test_seed_rule_on_hand_made_states():
    g, sw, w, vis = _small_grid()
    shape, origin = (8, 8, 8), (0.005, 0.005, 0.005)
    _put(g, sw, w, (2, 2, 2), 0.0)               # a surface voxel
    _put(g, sw, w, (5, 5, 5), 0.03)              # free space, |sdf| > 0.9 vs: no seed
    _put(g, sw, w, (6, 1, 1), -0.07)             # past -(trunc - 1.1 vs) = -0.058: the truncation boundary seeds
    _put(g, sw, w, (1, 6, 1), -0.04)             # inside, between the two rules: no seed
    _put(g, sw, w, (1, 1, 6), 0.0, weight=0.1)   # weight not above minimum_tsdf_weight: unobserved
    s, amb = R.seed(g, sw, w, vis, shape, origin, 0.02)
    assert not amb.any()
    # a cell of the voxel's size, a quarter voxel off, probes its own voxel (centre, - half) and the next one (+ half)
    expect = np.zeros(shape, bool)
    for v in ((2, 2, 2), (6, 1, 1)):
        expect[v] = True
        for a in range(3):
            n = list(v)
            n[a] -= 1
            expect[tuple(n)] = True
    assert np.array_equal(s, expect)
    hidden = vis.copy()
    hidden[0] = False  # the block of (2, 2, 2) never visible: its voxel no longer seeds
    s2, _ = R.seed(g, sw, w, hidden, shape, origin, 0.02)
    assert not s2[2, 2, 2] and s2[6, 1, 1]


def test_sign_rule_on_hand_made_states():
    g, sw, w, vis = _small_grid()
    shape, origin = (8, 8, 8), (0.005, 0.005, 0.005)
    _put(g, sw, w, (2, 2, 2), 0.0)
    _put(g, sw, w, (3, 2, 2), -0.02)             # observed inside: negative distance
    _put(g, sw, w, (1, 2, 2), 0.02)              # observed outside
    e = R.esdf(g, sw, w, vis, shape, origin, 0.02)
    d = e["distance"].astype(np.float64)
    assert d[2, 2, 2] == 0 and d[1, 2, 2] == 0   # (1, 2, 2) is itself a seed: its + probe hits the surface voxel
    assert d[3, 2, 2] == -np.float16(0.02)       # one cell from the seed (2, 2, 2), and inside
    assert e["inside"][3, 2, 2] and not e["inside"][1, 2, 2] and not e["inside"][7, 7, 7]
    assert d[7, 7, 7] == np.float16(np.sqrt(75.0) * 0.02)  # nearest seed (2, 2, 2); an unobserved cell counts as outside
    empty = R.esdf(g, np.zeros_like(sw), np.zeros_like(w), vis, shape, origin, 0.02)
    assert (empty["distance"] == np.float16(1e4)).all() and (empty["d2"] == -1).all()


def test_pipeline_esdf_is_close_to_the_analytic_distance():
    """one frame of the scene through every stage of the oracle.  Over the ESDF cells that the camera observed as free space (a
    valid positive TSDF sample at the centre) outside the sphere, the ESDF is compared with the distance to the nearer of the
    sphere and the ground.  Measured: max error 1.20 esdf_voxel_size, mean 0.35 (the gather rule's seed band is about 1.5
    cells thick and a cell centre is up to sqrt(3) / 2 cells from its probes); asserted: 1.5."""
    from curobo_amd.perception.mapper import MapperCfg

    g = R.Grid.from_cfg(MapperCfg(**C.CFG))
    f = C.oracle_run(g, frames=C.FRAMES[:1])[0]
    vs = C.CFG["esdf_voxel_size"]
    e = R.esdf(g, f["sw"], f["w"], f["sure"], C.ESDF_SHAPE, C.ESDF_ORIGIN, vs)
    assert not e["ambiguous"].any() and e["seed"].sum() > 500 and e["inside"].sum() > 100
    centres = R.esdf_centres(C.ESDF_SHAPE, C.ESDF_ORIGIN, vs)
    sdf, _ = R.tsdf_sample(g, f["sw"], f["w"], f["sure"], centres)
    sel = (sdf < 1e9) & (sdf > 0) & (np.linalg.norm(centres, axis=-1) > R.SPHERE_RADIUS) & (e["d2"] >= 0)
    assert sel.sum() > 1000
    err = np.abs(e["distance"].astype(np.float64) - R.scene_distance(centres))[sel] / vs
    print(f"max error {err.max():.3f} cells, mean {err.mean():.3f}, over {int(sel.sum())} cells")
    assert err.max() <= 1.5


def test_scene_meets_the_conditions_of_the_device_tests():
    """what tests/test_gpu_mapper.py presupposes of the scene, checked where it costs no GPU time: at most 1 % of the possible
    blocks are not sure, and at most 1 % of the voxels of sure blocks are ambiguous in some frame of the k = 3 run"""
    from curobo_amd.perception.mapper import MapperCfg

    g = R.Grid.from_cfg(MapperCfg(**C.CFG))
    run = C.oracle_run(g)
    ever_sure, amb = np.zeros(g.n_blocks, bool), np.zeros((g.n_blocks, g.bs ** 3), bool)
    for f in run:
        assert (f["sure"] <= f["possible"]).all()
        assert (f["possible"] & ~f["sure"]).sum() <= 0.01 * f["possible"].sum()
        assert f["updated"].sum() > 10000
        ever_sure |= f["sure"]
        amb |= f["ambiguous"]
    assert len(C.FRAMES[1]) == 2
    assert amb[ever_sure].mean() <= 0.01, amb[ever_sure].mean()
    assert ever_sure.reshape(5, 12, 13)[:, :, 12].any(), "the padded last block along x must be visible"
