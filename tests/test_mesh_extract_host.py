"""The float64 oracle of Mapper.extract_mesh (tests/mesh_extract_ref.py) held to what a mesh for the collision path must be:
closed and consistently oriented; and the two fields scene.types.Mesh gained."""

import numpy as np
import pytest

import mapper_ref as R
import mesh_extract_ref as M

VS, TRUNC = float(np.float32(0.02)), float(np.float32(0.08))


def _grid(nx, ny, nz, bs):
    return R.Grid(nx, ny, nz, bs, [0.0, 0.0, 0.0], VS, TRUNC, 0.1, 5.0, 0.5)


@pytest.fixture(scope="module")
def sphere():
    g = _grid(**M.SPHERE_GRID)
    sw, w, visible = M.sphere_tsdf(g)
    return g, sw, w, visible, M.extract(g, sw, w, visible)


def test_sphere_is_closed_oriented_and_round(sphere):
    """radius bound: the chord error h^2 / (8 r) = 2e-4 m of a 0.02 m voxel on a 0.25 m sphere plus two fp16 steps of a value up to
    0.08 m (2 x 6.1e-5), rounded up to 5e-4"""
    _, _, _, _, out = sphere
    v, t = out["vertices"], out["triangles"]
    assert out["ambiguous_cubes"] == 0 and out["ambiguous_triangles"] == 0
    assert len(t) == out["n_raw_triangles"] > 5000, "nothing dropped: the sphere lies inside the grid and no triangle is tiny"
    assert M.is_closed_and_oriented(t), "every directed edge occurs once and has its opposite"
    assert M.euler_characteristic(t) == 2
    volume, analytic = M.signed_volume(v, t), 4.0 / 3.0 * np.pi * R.SPHERE_RADIUS ** 3
    radial = np.abs(np.linalg.norm(v - np.asarray(M.SPHERE_CENTRE), axis=1) - R.SPHERE_RADIUS).max()
    print(f"{len(v)} vertices, {len(t)} triangles, volume {volume:.5f} m^3 (analytic {analytic:.5f}), max | |v| - r | = {radial:.3e} m")
    assert volume > 0 and abs(volume - analytic) <= 0.01 * analytic
    assert radial <= 5e-4
    # the normals are central differences over two voxels of a clipped, quantised field: within a few degrees of the radius
    outward = (v - np.asarray(M.SPHERE_CENTRE)) / R.SPHERE_RADIUS
    assert (np.einsum("ij,ij->i", out["normals"], outward) > 0.99).all()
    assert np.abs(np.linalg.norm(out["normals"], axis=1) - 1.0).max() < 1e-12


def test_sphere_in_float32_and_with_refinement(sphere):
    """a vertex interpolated between two voxel centres already is the zero of the trilinear field along its edge, so the Newton
    steps stop at once; float32 decides as float64 does on this input"""
    g, sw, w, visible, out = sphere
    single = M.extract(g, sw, w, visible, dtype=np.float32)
    assert single["vertices"].dtype == np.float32 and np.array_equal(single["triangles"], out["triangles"])
    refined = M.extract(g, sw, w, visible, refine_iterations=2)
    assert np.array_equal(refined["triangles"], out["triangles"]) and np.abs(refined["vertices"] - out["vertices"]).max() < 1e-9
    level = M.extract(g, *M.sphere_tsdf(g, centre=M.SPHERE_CENTRE_LEVEL)[:2], visible, level=0.01, surface_only=True)
    assert level["ambiguous_cubes"] == 0 and level["ambiguous_triangles"] == 0
    r = np.linalg.norm(level["vertices"] - np.asarray(M.SPHERE_CENTRE_LEVEL), axis=1)
    assert np.abs(r - (R.SPHERE_RADIUS + 0.01)).max() <= 5e-4


def test_random_field_is_closed():
    """a seeded random +-field of 6^3 voxels inside a two-voxel positive margin: many distinct cases side by side, the ambiguous
    faces among them; the mesh is closed whatever the cases (|value| >= 2e-3 m: no triangle near the area rule)"""
    g = _grid(10, 10, 10, 4)
    field = M.random_field(g, seed=5)
    sw, w = M.stored_pair(g, field, np.full(field.shape, 2.0))
    out = M.extract(g, sw, w, np.ones(g.n_blocks, bool))
    assert out["ambiguous_cubes"] == 0 and out["ambiguous_triangles"] == 0 and out["dropped_missing"] == 0
    assert (out["case_histogram"] > 0).sum() > 100 and len(out["triangles"]) == out["n_raw_triangles"] > 500
    assert M.is_closed_and_oriented(out["triangles"])
    assert M.signed_volume(out["vertices"], out["triangles"]) > 0, "the negative cells are enclosed, normals outward"


def test_rim_of_the_observed_region_and_the_weight_rule():
    """a never-visible block and unobserved voxels cut the surface open: triangles whose owner cube is not meshed are dropped, the
    rest stays oriented; weight == minimum counts as observed (>=)"""
    g = _grid(10, 10, 10, 4)
    field = M.random_field(g, seed=5)
    weight = np.full(field.shape, 2.0)
    weight[3:5, 3:6, 4] = 0.0
    weight[3, 6, 6] = g.min_weight  # (outside block 13 = voxels 4..7 of every axis)
    sw, w = M.stored_pair(g, field, weight)
    visible = np.ones(g.n_blocks, bool)
    visible[13] = False
    out = M.extract(g, sw, w, visible)
    whole = M.extract(g, *M.stored_pair(g, field, np.full(field.shape, 2.0)), np.ones(g.n_blocks, bool))
    assert 0 < len(out["triangles"]) < len(whole["triangles"]) and out["dropped_missing"] > 0
    e = M.directed_edges(out["triangles"])
    n = int(e.max()) + 1
    assert len(np.unique(e[:, 0] * n + e[:, 1])) == len(e), "no directed edge twice: still consistently oriented"
    assert not M.is_closed_and_oriented(out["triangles"])
    below = weight.copy()
    below[3, 6, 6] = 0.499
    fewer = M.extract(g, *M.stored_pair(g, field, below), visible)
    assert len(fewer["triangles"]) < len(out["triangles"])


def test_mesh_fields_and_inputs():
    import torch

    from curobo_amd.scene.types import Mesh

    v = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    f = [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]
    plain = Mesh(name="m", pose=[0, 0, 0, 1, 0, 0, 0], vertices=v, faces=f)
    assert plain.vertex_normals is None and plain.vertex_colors is None
    want_v, want_f = plain.get_mesh_data()
    assert want_v.dtype == np.float32 and want_f.dtype == np.int32 and want_f.shape == (4, 3)
    for vv, ff in ((np.asarray(v), np.asarray(f)), (torch.tensor(v), torch.tensor(f, dtype=torch.int32)),
                   (torch.tensor(v, dtype=torch.float64), torch.tensor(f).reshape(-1))):
        got_v, got_f = Mesh(name="m", pose=[0, 0, 0, 1, 0, 0, 0], vertices=vv, faces=ff).get_mesh_data()
        assert got_v.dtype == np.float32 and got_f.dtype == np.int32
        assert np.array_equal(got_v, want_v) and np.array_equal(got_f, want_f)
    scaled = Mesh(name="m", pose=[0, 0, 0, 1, 0, 0, 0], vertices=torch.tensor(v), faces=f, scale=[2.0, 1.0, 1.0])
    assert np.array_equal(scaled.get_mesh_data()[0], want_v * np.array([2.0, 1.0, 1.0], np.float32))
    both = Mesh(name="m", pose=[0, 0, 0, 1, 0, 0, 0], vertices=v, faces=f, vertex_normals=np.ones((4, 3)), vertex_colors=np.zeros((4, 3), np.uint8))
    assert both.vertex_normals.shape == (4, 3) and both.vertex_colors.dtype == np.uint8
    assert np.array_equal(both.get_cuboid().dims, [1.0, 1.0, 1.0])
