"""Mesh collision against the REFERENCE's own Warp kernels.

``tests/golden/mesh_warp_golden.npz`` holds inputs and outputs of the reference's unmodified
``sphere_obstacle_collision_kernel`` / ``swept_sphere_obstacle_collision_kernel`` / ``apply_speed_metric`` over mesh obstacles
(data_mesh.py ``compute_local_sdf_with_grad``: the ``max(half bounding-box diagonal, radius_adjusted)`` search range, the
``(max_distance, 0)`` answer when nothing is found, the gradient ``-(closest - p) / |closest - p|`` on both sides, the sweep
over mesh samples, cuboids launched before meshes), executed thread by thread on the CPU through the Warp stand-in of
``tests/golden/warp_emulator`` with Warp's mesh intrinsics restated (generator: ``tests/golden/make_mesh_warp_golden.py``).

Worlds: closed meshes (subdivided box, ball, torus, L prism, a box smaller than the spheres' reach) at rotated poses in two
environments with a disabled slot and ``count < max_n``; cuboids + meshes; the open and flipped fixtures of
``test_gpu_mesh.py``; and two closed boxes whose top face has a T-junction closed by a zero-area / near-zero-area sliver.
Spheres whose queries sit on a knife edge (see the generator) are outside the per-case ``mask``; those whose closest
triangle is tied with another one only outside ``grad_mask``.

CPU: the emulator's point query against the oracle's and the closest feature; the oracle reproduces every case at 1e-6 under
the reference's ray sign.  GPU: the HIP mesh launch on every path -- tree walk, cell lists, workgroup per sphere, the
``SceneData.from_arrays(meshes=)`` entry -- at 1e-5, in the reference's gradient mode, and the consistent mode's distances.

The sliver boxes: the cell-list and workgroup kernels decide the side of a closed mesh by the sign of the summed side terms
of the triangles at the minimum, the tree walk casts rays when its closest feature has no verdict, so a sum of exactly zero
(a zero-area face has no normal) would make the lists say "outside" where the walk says "inside".  On these fixtures the sum
did not come out zero on an MI355X: all four paths reproduce the golden there.  The likely reason: Ericson's closest-point
test files a point next to a collinear triangle under one of its edges or vertices (its face branch needs three rounding
residues of one sign), whose pseudonormals come from the neighbouring faces; and where the sliver's face branch is taken,
its candidate point lies off the true closest point, so a neighbour with a well-defined normal wins the minimum.  The cases
stand as agreement tests of the three paths and the reference there.
"""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "mesh_warp_golden.npz")
G = np.load(GOLD)
CASES = [str(x) for x in G["case_names"]]
STATS = [str(x) for x in G["stats_names"]]


def _emulator():
    spec = importlib.util.spec_from_file_location("_warp_emulator_mesh", os.path.join(HERE, "golden", "warp_emulator", "warp", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _case(name):
    i = CASES.index(name)
    w = str(G["case_world"][i])
    wgt, eta, multi, swept, dt = G["case_params"][i]
    return w, float(wgt), float(eta), bool(multi), bool(swept), (float(dt) if dt > 0 else None)


def _meshes(w):
    names = [str(x) for x in G[f"{w}/mesh_names"]]
    return [(n, G[f"{w}/mesh{k}/vertices"], G[f"{w}/mesh{k}/faces"]) for k, n in enumerate(names)]


def _envs(w):
    """the world as MeshStore takes it: per environment the first ``count`` slots (disabled ones included)"""
    meshes = _meshes(w)
    envs = []
    for e in range(G[f"{w}/count"].shape[0]):
        obs = []
        for i in range(int(G[f"{w}/count"][e])):
            n, v, f = meshes[int(G[f"{w}/mesh_id"][e, i])]
            obs.append({"name": f"slot{i}", "mesh_name": n, "vertices": v, "faces": f, "pose": G[f"{w}/pose"][e, i].astype(np.float64),
                        "enable": bool(G[f"{w}/enable"][e, i])})
        envs.append(obs)
    return envs


def _cuboids(w):
    keys = [k for k in G.files if k.startswith(f"{w}/cuboid_")]
    return {k.split("/", 1)[1]: G[k] for k in keys} or None


def _oracle_scene(w):
    meshes = _meshes(w)
    voff, foff = np.cumsum([0] + [len(v) for _n, v, _f in meshes]), np.cumsum([0] + [len(f) for _n, _v, f in meshes])
    scene = {"mesh_id": G[f"{w}/mesh_id"], "mesh_dims": G[f"{w}/dims"], "mesh_inv_pose": G[f"{w}/inv_pose"], "mesh_enable": G[f"{w}/enable"],
             "mesh_count": G[f"{w}/count"], "mesh_vertices": np.concatenate([v for _n, v, _f in meshes]),
             "mesh_faces": np.concatenate([f for _n, _v, f in meshes]), "mesh_vert_offset": voff.astype(np.int32),
             "mesh_face_offset": foff.astype(np.int32)}
    scene.update(_cuboids(w) or {})
    return scene


def _compare(name, dist, grad, tol):
    want_d, want_g, mask = G[f"{name}/distance"], G[f"{name}/gradient"], G[f"{name}/mask"]
    assert dist.shape == want_d.shape
    scale_d, scale_g = max(1.0, float(want_d.max())), max(1.0, float(np.abs(want_g).max()))
    assert np.array_equal((dist > 0)[mask], (want_d > 0)[mask]), (name, "different spheres in collision",
                                                                    np.argwhere(((dist > 0) != (want_d > 0)) & mask)[:8])
    np.testing.assert_allclose(dist[mask], want_d[mask], rtol=0, atol=tol * scale_d, err_msg=name)
    # the direction (p - closest) / |p - closest| carries the rounding of the closest point (fp32 barycentrics in Warp, a + v ab
    # in the oracle and the kernels: up to ~5e-7 m) divided by the distance: a term of its own for spheres that graze a surface
    err = np.abs(grad[..., :3] - want_g[..., :3]).max(-1)
    lim = tol * scale_g + 5e-7 * np.abs(want_g[..., :3]).max(-1) / np.maximum(G[f"{name}/near"], 1e-9)
    gm = G[f"{name}/grad_mask"]
    assert (err <= lim)[gm].all(), (name, np.argwhere((err > lim) & gm)[:8], err[(err > lim) & gm][:8])


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_golden_covers_the_branches():
    """hits and free spheres in every case; found inside / outside, nothing found, the query_distance branch; knife edges
    absent or masked (a handful at most); the special spheres did what they were placed for"""
    for name in CASES:
        w, *_ = _case(name)
        st = dict(zip(STATS, G[f"{name}/stats"]))
        d, g, mask, sp = G[f"{name}/distance"], G[f"{name}/gradient"], G[f"{name}/mask"], G[f"{w}/spheres"]
        assert (d > 0).sum() > 20 and st["found"] > 50 and st["not_found"] > 50, (name, st)
        assert st["inside"] > 20, (name, st)
        gm = G[f"{name}/grad_mask"]
        assert (~mask).sum() <= st["knife"] + st["ray"] and (~mask).mean() < 0.05, (name, st)
        assert not (gm & ~mask).any() and (~gm).sum() <= (~mask).sum() + st["tie"] and (~gm).mean() < 0.1, (name, st)
        assert np.all(d[sp[..., 3] < 0] == 0) and np.all(g[sp[..., 3] < 0] == 0), name
        assert np.all(g[..., 3] == 0), name
        if not w.startswith("sliver"):
            assert st["outside"] > 50 and (d == 0).sum() > 20, (name, st)
    for name in ("closed_static", "closed_swept"):
        st = dict(zip(STATS, G[f"{name}/stats"]))
        assert st["beyond_half_diag"] > 5  # found only thanks to radius_adjusted > half the tiny box's diagonal
        d = G[f"{name}/distance"]
        assert np.all(d[0, :, 0] == 0)        # far outside: nothing found
        assert np.all(d[2, :, 1] > 0) and np.all(d[2, :, 2] > 0)  # deep inside the box, inside the ball
        assert np.all(d[2, :, 3] > 0)         # over the tiny box, reached through radius_adjusted only
    # the disabled slot (5) and the slots past env 1's count never collide
    hit = G["closed_static/slots_hit"]
    assert not (hit & (1 << 5)).any() and not (hit[1::2] & ~0b111).any()
    assert (hit[0::2] & (1 << 4)).any() and (hit[1::2] & (1 << 2)).any()
    assert not np.array_equal(G["closed_swept/distance"], G["closed_static/distance"])
    assert not np.array_equal(G["closed_env0_only/distance"], G["closed_static/distance"])
    # the sliver spheres are inside their boxes
    assert (G["sliver_static/side"] == -1).all()


def test_sliver_fixtures_are_closed_oriented_boxes_with_a_degenerate_face():
    from test_oracle_mesh import is_closed_and_oriented

    from curobo_amd.backends.mesh import mesh_is_closed_and_oriented

    area = {}
    for n, v, f in _meshes("sliver"):
        assert is_closed_and_oriented(f) and mesh_is_closed_and_oriented(v, f), n  # -> sign rule 0 and the cell lists
        a, b, c = (v[f[:, k]] for k in range(3))
        area[n] = np.linalg.norm(np.cross(b - a, c - a), axis=1)
        vol = np.einsum("ij,ij->i", a.astype(np.float64), np.cross(b.astype(np.float64), c.astype(np.float64))).sum() / 6
        assert abs(vol - 0.2 * 0.15 * 0.1) < 1e-8, n
    assert area["sliver_zero_area"].min() == 0.0
    assert 0.0 < area["sliver_near_zero_area"].min() < 1e-3 * area["sliver_near_zero_area"].max()


def test_emulator_point_query_is_the_oracle_ray_rule_and_the_closest_feature(oracle):
    """the emulator's ``mesh_query_point`` + ``mesh_eval_position`` on random points against the oracle's brute force under
    the "rays" sign rule (distance, gradient, sign) and against the fp64 closest feature (distance, closest point): the
    golden does not rest on one restatement of Warp's query"""
    from mesh_sign_rules import closest_feature

    wp = _emulator()
    rng = np.random.default_rng(3)
    for n, v, f in _meshes("closed")[:4] + _meshes("open")[2:] + _meshes("sliver"):
        mesh = wp.Mesh(points=wp.array(v, dtype=wp.vec3), indices=wp.array(f.reshape(-1), dtype=wp.int32))
        p = rng.uniform(v.min(0) - 0.05, v.max(0) + 0.05, size=(120, 3)).astype(np.float32)
        max_d = np.float32(0.5 * np.linalg.norm(v.max(0) - v.min(0)))
        sdf = np.empty(len(p), np.float32)
        cp = np.empty((len(p), 3), np.float32)
        for i, x in enumerate(p):
            q = wp.mesh_query_point(mesh.id, wp.vec3(x), max_d)
            if not q.result:
                sdf[i], cp[i] = max_d, np.nan
                continue
            c = wp.mesh_eval_position(mesh.id, q.face, q.u, q.v)
            cp[i] = np.array(c.v, np.float32)
            sdf[i] = np.float32(np.linalg.norm((cp[i] - x).astype(np.float32))) * q.sign
        oracle.set_mesh_sign_rule("rays")
        try:
            ref, ref_g = oracle.mesh_query(p, v, f, float(max_d))
        finally:
            oracle.set_mesh_sign_rule("winding")
        _t, _r, q64, d64 = closest_feature(p, v, f)
        found = np.isfinite(cp[:, 0])
        assert found.sum() > 30 and (sdf < 0).sum() > 5 or n == "single_sided_plate", n
        assert np.array_equal(found, ref != max_d) and np.array_equal(found, d64 < max_d), n
        np.testing.assert_allclose(sdf, ref, atol=2e-7, rtol=1e-5, err_msg=n)
        np.testing.assert_allclose(np.abs(sdf[found]), d64[found], atol=2e-7, rtol=1e-5, err_msg=n)
        np.testing.assert_allclose(cp[found], q64[found], atol=1e-6, err_msg=n)
        g = (p - cp) / np.maximum(np.linalg.norm(p - cp, axis=1, keepdims=True), 1e-30)
        err = np.abs(g - ref_g).max(1)[found]
        assert (err <= 1e-6 + 5e-7 / np.maximum(d64[found], 1e-9)).all(), (n, err.max())  # (see _compare)


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_reference_warp_mesh_kernels(name, oracle):
    w, wgt, eta, multi, swept, dt = _case(name)
    oracle.set_mesh_sign_rule("rays")
    try:
        r = oracle.scene_collision(G[f"{w}/spheres"], _oracle_scene(w), wgt, eta, G[f"{w}/env_query_idx"], multi, sweep=swept,
                                   enable_speed_metric=dt is not None, speed_dt=dt if dt is not None else 0.02)
    finally:
        oracle.set_mesh_sign_rule("winding")
    _compare(name, r["distance"], r["gradient"], 1e-6)


def test_reference_mesh_gradient_points_away_from_the_surface_for_centres_outside(oracle):
    """what ``MeshStore.REFERENCE_GRADIENT`` says of data_mesh.py's gradient, by a run: for a sphere whose colliding queries
    all have their centre OUTSIDE the mesh, a small step along the golden gradient LOWERS the cost (the vector points away
    from the surface, against the cost's derivative); for centres INSIDE the step raises it, as the cuboid's gradient does"""
    w, wgt, eta, multi, _swept, _dt = _case("closed_static")
    sp, side, d, g = G[f"{w}/spheres"], G["closed_static/side"], G["closed_static/distance"], G["closed_static/gradient"]
    sel = G["closed_static/mask"] & (d > 1e-3) & (np.linalg.norm(g[..., :3], axis=-1) > 1e-3)
    step = np.zeros_like(sp)
    step[..., :3] = 1e-4 * g[..., :3] / np.maximum(np.linalg.norm(g[..., :3], axis=-1, keepdims=True), 1e-30)
    oracle.set_mesh_sign_rule("rays")
    try:
        moved = oracle.scene_collision(sp + step, _oracle_scene(w), wgt, eta, G[f"{w}/env_query_idx"], multi)["distance"]
    finally:
        oracle.set_mesh_sign_rule("winding")
    out, inside = sel & (side == 1), sel & (side == -1)
    assert out.sum() > 20 and inside.sum() > 10
    assert (moved[out] < d[out]).all()
    assert (moved[inside] > d[inside]).all()


# ------------------------------------------------------------------------------------------------------------------ GPU
PATHS = ["walk", "cells", "wide", "scene_entry"]


def _run_gpu(name, path, device, gradient_mode=None):
    import torch

    from curobo_amd.backends import collision as Cn
    from curobo_amd.scene import MeshStore, SceneData

    w, wgt, eta, multi, swept, dt = _case(name)
    envs = _envs(w)
    if path == "scene_entry":
        scene = SceneData.from_arrays(_cuboids(w), device, meshes=envs)  # as a scene configuration reaches the kernels
        store = scene.meshes
    else:
        cells = {"walk": False, "cells": None, "wide": {"pad": 0.0, "gather_cap": 1}}[path]
        store = MeshStore(envs, device, cells=cells, max_n=G[f"{w}/mesh_id"].shape[1],
                          gradient_mode=MeshStore.REFERENCE_GRADIENT if gradient_mode is None else gradient_mode)
        # the golden's own slot arrays (the reference's get_bounds dims, its inverse poses), in place: the struct keeps the pointers
        store.dims.copy_(torch.as_tensor(G[f"{w}/dims"]))
        store.inv_pose.copy_(torch.as_tensor(G[f"{w}/inv_pose"]))
        scene = SceneData.from_arrays(_cuboids(w), device, meshes=store)
    assert store.gradient_mode == (MeshStore.REFERENCE_GRADIENT if gradient_mode is None else gradient_mode)
    used = np.arange(store.max_n)[None, :] < G[f"{w}/count"][:, None]  # (the entry sizes its store by the longest environment)
    np.testing.assert_allclose(store.dims.cpu().numpy()[used], G[f"{w}/dims"][:, :store.max_n][used], rtol=0, atol=1e-7)
    np.testing.assert_allclose(store.inv_pose.cpu().numpy()[used], G[f"{w}/inv_pose"][:, :store.max_n][used], rtol=0, atol=1e-6)
    sp = G[f"{w}/spheres"]
    b, h, S, _ = sp.shape
    dist = torch.full((b, h, S), 7.0, device=device)  # every entry must be written
    grad = torch.full((b, h, S, 4), 7.0, device=device)
    Cn.sphere_obstacle_collision(
        dist, grad, torch.as_tensor(sp, device=device), scene.struct, torch.tensor([wgt], device=device),
        torch.tensor([eta], device=device), torch.as_tensor(G[f"{w}/env_query_idx"], device=device), b, h, S, multi, 3 if swept else 0,
        dt is not None, torch.tensor([dt if dt is not None else 0.02], device=device))
    torch.cuda.synchronize()
    ws = next(iter(dist._curobo_mesh_ws.values()))
    counters = ws[:16].view(torch.int32).cpu().numpy()  # [heavy, handed to the tree walk, light, handed to a workgroup of its own]
    return dist.cpu().numpy(), grad.cpu().numpy(), counters, store


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", CASES)
def test_hip_mesh_paths_reproduce_the_reference_warp_kernels(name, path, device):
    w = _case(name)[0]
    d, g, cnt, store = _run_gpu(name, path, device)
    assert not (d == 7.0).any() and not (g == 7.0).any()
    _compare(name, d, g, 1e-5)
    live = int(cnt[0]) + int(cnt[2])
    assert live > 10, cnt  # spheres went through the mesh launch's queue
    signed_by_rays = w == "open"
    if path == "walk":
        assert all(m.cell_start is None for m in store.meshes) and cnt[3] == 0, cnt
    elif path == "wide" and not signed_by_rays:
        assert cnt[3] > 0, cnt  # cells without a list: a workgroup per sphere
    elif path in ("cells", "scene_entry"):
        assert all(m.cell_start is not None for m in store.meshes)
        if signed_by_rays:
            assert cnt[1] > 0, cnt  # (a mesh signed by the reference's rays: the lists hand its queries to the tree walk)
        else:
            assert cnt[1] + cnt[3] < live, cnt  # the lists answered spheres themselves


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_consistent_gradient_mode_has_the_reference_distances(name, device):
    """``CONSISTENT_GRADIENT`` (the solvers' default) changes only the direction for centres outside the mesh: the same costs
    as the golden, and where every colliding query of a sphere had its centre outside a mesh (and no cuboid), the opposite
    gradient"""
    from curobo_amd.scene import MeshStore

    w = _case(name)[0]
    d, g, _cnt, _store = _run_gpu(name, "cells", device, gradient_mode=MeshStore.CONSISTENT_GRADIENT)
    want_d, want_g, mask = G[f"{name}/distance"], G[f"{name}/gradient"], G[f"{name}/mask"]
    scale_d, scale_g = max(1.0, float(want_d.max())), max(1.0, float(np.abs(want_g).max()))
    assert np.array_equal((d > 0)[mask], (want_d > 0)[mask])
    np.testing.assert_allclose(d[mask], want_d[mask], rtol=0, atol=1e-5 * scale_d)
    if _cuboids(w) is None and _case(name)[5] is None:  # (the speed metric adds a term of its own to the gradient)
        side = G[f"{name}/side"]
        lim = 1e-5 * scale_g + 5e-7 * np.abs(want_g[..., :3]).max(-1) / np.maximum(G[f"{name}/near"], 1e-9)  # (see _compare)
        for s, sgn in ((side == 1, -1.0), (side == -1, 1.0)):
            sel = G[f"{name}/grad_mask"] & s
            assert sel.sum() > 5 or not s.any(), name  # (the sliver spheres are all inside)
            assert (np.abs(g[..., :3] - sgn * want_g[..., :3]).max(-1) <= lim)[sel].all(), name
