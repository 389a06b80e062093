"""Mapper.extract_mesh on the GPU against the float64 oracle tests/mesh_extract_ref.py.

The oracle is fed THE DEVICE'S OWN TSDF copied to the CPU, so only the extraction is compared.  Which cubes are meshed, their
cases, the vertices they own and the table triangles are integer decisions on values float32 and float64 agree on wherever
the oracle's ambiguous-cube set is empty, which every test asserts of its input; the triangle list is then compared index for
index and the vertex count exactly.  A triangle the oracle flags at the area rule (|cross|^2 within a factor 4 of the
threshold) may be kept or dropped: the synthetic inputs and the spheres are built to have none, which is asserted; the
integrated scene has a handful (7 of 11 000 with the oracle's own integration), bounded at 0.1 %.

Positions without refinement: p_a + t (p_b - p_a) with coordinates below 0.5 m, a few float32 ulp (3e-8 m each) plus the
error of t times the 0.02 m voxel: 1e-6 m.  Normals: quotients of fp16 pairs differenced over two voxels and normalised,
1e-5 per component wherever the six probes pick the same voxels (vertices within the face window are flagged) and the
gradient is not tiny (flagged below 1e-3).

The sphere cases use the 30^3 grid of tests/test_mesh_extract_host.py (30 = 7 blocks of 4 + 2 voxels: the padded last block
is live there as well): the 50 x 48 x 20 grid of the other cases is 0.4 m high and cannot hold a closed 0.25 m sphere."""

import numpy as np
import pytest
import torch

import mapper_cases as C
import mapper_ref as R
import mesh_extract_ref as M

pytestmark = pytest.mark.gpu

SPHERE_CFG = dict(extent_meters_xyz=(0.6, 0.6, 0.6), extent_esdf_meters_xyz=(0.6, 0.6, 0.6))
SMALL_CFG = dict(extent_meters_xyz=(0.32, 0.32, 0.16), extent_esdf_meters_xyz=(0.32, 0.32, 0.16))  # 16 x 16 x 8 voxels


def _cfg(**over):
    from curobo_amd.perception.mapper import MapperCfg

    return MapperCfg(**{**C.CFG, **over})


def _mapper(**over):
    from curobo_amd.perception.mapper import Mapper

    cfg = _cfg(**over)
    return Mapper(cfg, use_graph=False), R.Grid.from_cfg(cfg)


def _inject(mapper, sw, w, visible):
    t = mapper.tsdf
    t.block_data.copy_(torch.as_tensor(np.stack([sw, w], -1)))
    t.block_visible.zero_()
    t.block_visible[: len(visible)] = torch.as_tensor(np.asarray(visible, np.uint8))


def _state(mapper):
    t = mapper.tsdf
    data = t.block_data.cpu().numpy()
    return data[..., 0], data[..., 1], t.block_visible.cpu().numpy()[: t.n_blocks] != 0


def _extract(mapper, **kw):
    out = mapper.extract_mesh_tensors(**kw)
    torch.cuda.synchronize()
    v, t, n, c = out
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and n.dtype == torch.float32 and c.dtype == torch.uint8
    assert v.shape == n.shape == c.shape and v.shape[1:] == t.shape[1:] == (3,) and all(x.device == mapper.tsdf.block_data.device for x in out)
    assert not c.any(), "no colour channel: zeros"
    return v.cpu().numpy(), t.cpu().numpy(), n.cpu().numpy()


def _check(got, ref, what, position_tol=1e-6, normal_tol=1e-5, flagged_max=0.01, near_max=0.0):
    v, t, n = got
    assert ref["ambiguous_cubes"] == 0, f"{what}: {ref['ambiguous_cubes']} cubes hang on a value float32 may see otherwise: change the input"
    near = ref["ambiguous_triangles"] / max(len(ref["triangles"]), 1)
    assert near <= near_max, f"{what}: {ref['ambiguous_triangles']} triangles at the area threshold: change the scene"
    assert len(v) == len(ref["vertices"]) > 0, f"{what}: vertex count"
    assert M.same_triangles(t, ref), f"{what}: triangles, index for index ({len(t)} against {len(ref['triangles'])})"
    position = np.abs(v - ref["vertices"]).max()
    flagged = ref["normal_flag"]
    assert flagged.mean() <= flagged_max, f"{what}: {flagged.mean():.4f} of the vertices are flagged: change the scene"
    normal = np.abs(n - ref["normals"])[~flagged].max()
    print(f"{what}: {len(v)} vertices, {len(t)} triangles ({ref['n_raw_triangles']} from the table, {ref['dropped_missing']} at the rim, "
          f"{ref['ambiguous_triangles']} flagged), position {position:.3e} m, normals {normal:.3e} outside {int(flagged.sum())} flagged vertices")
    assert position <= position_tol, what
    assert normal <= normal_tol, what


def synthetic_field(g: R.Grid, seed: int = 9):
    """(sw, w, visible): the seeded random +-field inside a two-voxel positive margin, a patch of unobserved voxels, one block never
    visible in the middle of the surface, one voxel at exactly the minimum weight"""
    field = M.random_field(g, seed)
    weight = np.full(field.shape, 2.0)
    cx, cy, cz = g.nx // 2, g.ny // 2, g.nz // 2
    weight[cx - 5:cx - 2, cy - 4:cy - 1, cz - 2:cz] = 0.0
    weight[cx - 6, cy + 3, cz - 3] = g.min_weight
    sw, w = M.stored_pair(g, field, weight)
    visible = np.ones(g.n_blocks, bool)
    nbx, nby, nbz = g.nb
    if g.n_blocks > 1:
        visible[((nbz // 2) * nby + nby // 2) * nbx + nbx // 2] = False
    return sw, w, visible


# ---------------------------------------------------------------------------------------------------- 1: the integrated scene
@pytest.fixture(scope="module")
def integrated(device):
    from curobo_amd.types import CameraObservation, Pose

    mapper, grid = _mapper()
    for cams in C.FRAMES:
        depth, K, pos, quat = C.frame(*cams)
        t = lambda a: torch.as_tensor(a, device=device)  # noqa: E731
        mapper.integrate(CameraObservation(depth_image=t(depth), intrinsics=t(K), pose=Pose(t(pos), t(quat))))
    torch.cuda.synchronize()
    return mapper, grid, _state(mapper)


@pytest.mark.parametrize("surface_only", [False, True])
def test_integrated_scene(integrated, surface_only):
    mapper, grid, (sw, w, ever) = integrated
    assert (grid.nx, grid.ny, grid.nz, grid.bs) == (50, 48, 20, 4)
    ref = M.extract(grid, sw, w, ever, surface_only=surface_only)
    assert len(ref["triangles"]) > 5000 and ref["dropped_missing"] > 100, "a surface with a rim"
    _check(_extract(mapper, surface_only=surface_only), ref, f"integrated scene, surface_only={surface_only}", near_max=1e-3)


# ---------------------------------------------------------------------------------------------------- 2, 3: synthetic fields
@pytest.mark.parametrize("shape, block_size", [("scene", 4), ("small", 1), ("small", 8), ("small", 16)])
def test_synthetic_field(device, shape, block_size):
    """block size 1: every neighbour lies in another block; 8: the 256-lane classify path; 16: eight classify tiles per block"""
    mapper, grid = _mapper(block_size=block_size, minimum_tsdf_weight=0.5, **({} if shape == "scene" else SMALL_CFG))
    assert (grid.nx, grid.ny, grid.nz) == ((50, 48, 20) if shape == "scene" else (16, 16, 8)) and grid.min_weight == 0.5
    sw, w, visible = synthetic_field(grid)
    _inject(mapper, sw, w, visible)
    ref = M.extract(grid, sw, w, visible)
    assert ref["dropped_missing"] > 0 and (ref["case_histogram"] > 0).sum() > 100
    assert (w == np.float16(0.5)).sum() == 1 and (w == 0).sum() > 0 and visible.all() == (grid.n_blocks == 1)
    _check(_extract(mapper), ref, f"synthetic field {shape}, blocks of {block_size}")
    # the voxel at the minimum weight is observed (>=): just below it the mesh loses the cubes that touch it
    w2 = np.where(w == np.float16(0.5), np.float16(0.4995), w)
    _inject(mapper, sw, w2, visible)
    fewer = M.extract(grid, sw, w2, visible)
    assert len(fewer["triangles"]) < len(ref["triangles"])
    _check(_extract(mapper), fewer, f"synthetic field {shape}, blocks of {block_size}, below the minimum weight")


# ---------------------------------------------------------------------------------------------------- 4, 5, 6: the sphere
@pytest.fixture(scope="module")
def sphere(device):
    mapper, grid = _mapper(**SPHERE_CFG)
    assert (grid.nx, grid.ny, grid.nz, grid.bs) == (30, 30, 30, 4)
    sw, w, visible = M.sphere_tsdf(grid)
    _inject(mapper, sw, w, visible)
    return mapper, grid, (sw, w, visible)


def test_sphere_at_a_level(device):
    mapper, grid = _mapper(**SPHERE_CFG)
    sw, w, visible = M.sphere_tsdf(grid, centre=M.SPHERE_CENTRE_LEVEL)
    _inject(mapper, sw, w, visible)
    sdf = sw.astype(np.float64) / w.astype(np.float64)
    assert np.abs(sdf - 0.01).min() > 1e-6, "no corner value within 1e-6 of the level"
    ref = M.extract(grid, sw, w, visible, level=0.01)
    _check(_extract(mapper, level=0.01), ref, "sphere, level 0.01")
    r = np.linalg.norm(ref["vertices"] - np.asarray(M.SPHERE_CENTRE_LEVEL), axis=1)
    assert np.abs(r - (R.SPHERE_RADIUS + 0.01)).max() <= 5e-4


def test_sphere_refined(sphere):
    """refine_iterations = 2.  Measured on the CPU for this input: the oracle in float32 is at most 1.7e-8 m from the oracle in
    float64 (the interpolated vertex already is the zero of the trilinear field along its edge, so the Newton loop stops at its
    first sample; the gap is that of the interpolation); the device may fuse and reorder where NumPy does not: 4 x that,
    6.8e-8 m with the figure above.  The test measures the gap again and uses what it measures.  The face window for the
    normals is that bound in voxels."""
    mapper, grid, (sw, w, visible) = sphere
    exact = M.extract(grid, sw, w, visible, refine_iterations=2)
    single = M.extract(grid, sw, w, visible, refine_iterations=2, dtype=np.float32)
    assert np.array_equal(single["triangles"], exact["triangles"])
    gap = float(np.abs(single["vertices"].astype(np.float64) - exact["vertices"]).max())
    bound = 4.0 * gap
    print(f"float32 oracle against float64 oracle: {gap:.3e} m; bound {bound:.3e} m")
    assert 0.0 < gap < 1e-7
    ref = M.extract(grid, sw, w, visible, refine_iterations=2, face_tol=bound / grid.vs)
    assert ref["ambiguous_triangles"] == 0, "no triangle at the area threshold"
    _check(_extract(mapper, refine_iterations=2), ref, "sphere, two refinement steps", position_tol=bound, flagged_max=0.02)


def test_sphere_mesh_is_closed_and_feeds_the_mesh_store(sphere, device):
    from curobo_amd.scene.mesh import MeshStore

    mapper, _, _ = sphere
    mesh = mapper.extract_mesh()
    torch.cuda.synchronize()
    assert mesh.name == "block_sparse_tsdf_mesh" and list(mesh.pose) == [0, 0, 0, 1, 0, 0, 0]
    assert mesh.vertices.is_cuda and mesh.vertex_normals.shape == mesh.vertices.shape == mesh.vertex_colors.shape
    v, t = mesh.get_mesh_data()
    assert v.dtype == np.float32 and t.dtype == np.int32 and len(t) > 5000
    assert M.is_closed_and_oriented(t) and M.euler_characteristic(t) == 2
    radial = np.abs(np.linalg.norm(v.astype(np.float64) - np.asarray(M.SPHERE_CENTRE), axis=1) - R.SPHERE_RADIUS).max()
    volume = M.signed_volume(v, t)
    print(f"device sphere: {len(v)} vertices, {len(t)} triangles, max | |v| - r | = {radial:.3e} m, volume {volume:.5f} m^3")
    assert radial <= 5e-4 and volume > 0
    store = MeshStore([[{"name": mesh.name, "vertices": v, "faces": t, "pose": list(mesh.pose)}]], device)
    torch.cuda.synchronize()
    assert store is not None


# ---------------------------------------------------------------------------------------------------- 7: empty maps, determinism
def test_empty_maps_determinism_and_untouched_buffers(integrated, device):
    mapper, grid = _mapper()
    for out in (mapper.extract_mesh_tensors(), mapper.extract_mesh_tensors(refine_iterations=2, surface_only=True)):
        assert [tuple(x.shape) for x in out] == [(0, 3)] * 4 and [x.dtype for x in out] == [torch.float32, torch.int32, torch.float32, torch.uint8]
    # everything observed, no sign change
    _inject(mapper, *M.stored_pair(grid, np.full([k * grid.bs for k in grid.nb], 0.03), np.full([k * grid.bs for k in grid.nb], 2.0)),
            np.ones(grid.n_blocks, bool))
    assert [tuple(x.shape) for x in mapper.extract_mesh_tensors()] == [(0, 3)] * 4
    assert mapper.extract_mesh().get_mesh_data()[0].shape == (0, 3)
    # visible blocks, nothing observed
    mapper.tsdf.block_data.zero_()
    assert [tuple(x.shape) for x in mapper.extract_mesh_tensors()] == [(0, 3)] * 4
    full, _, _ = integrated
    full.compute_esdf()
    t = full.tsdf
    before = [x.clone() for x in (t.block_data, t.block_visible, t.frame_visible, full._dist_field, full._sites, full._sites_scratch)]
    a = full.extract_mesh_tensors(refine_iterations=2)
    b = full.extract_mesh_tensors(refine_iterations=2)
    torch.cuda.synchronize()
    assert len(a[1]) > 5000
    for x, y in zip(a, b):
        assert x.data_ptr() != y.data_ptr() and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), "two calls, bit-identical tensors"
    for x, y in zip(before, (t.block_data, t.block_visible, t.frame_visible, full._dist_field, full._sites, full._sites_scratch)):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), "extraction writes none of the mapper's buffers"
