"""The link-pair sweep kernel and the self-collision matrix built on it, on the MI355X, against the float64 restatement of
``collision_matrix_ref.py`` on the very same fp32 sphere tensors."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from collision_matrix_ref import matrix_ref, sweep_ref  # noqa: E402
from conftest import load_model, sample_q  # noqa: E402

pytestmark = pytest.mark.gpu

_kin, _fk, _ref = {}, {}, {}


def kin_of(robot, device):
    from curobo_amd.kinematics import Kinematics, KinematicsCfg

    if robot not in _kin:
        _kin[robot] = Kinematics(KinematicsCfg.from_packaged(robot, device=device))
    return _kin[robot]


def fk_spheres(robot, n, device):
    """the project's FK on ``sample_q(model, n, seed=3)``: a device tensor [n, S, 4] of its own (computed once per case)"""
    import torch

    if (robot, n) not in _fk:
        kin = kin_of(robot, device)
        q = torch.as_tensor(sample_q(kin.config.model, n, seed=3), device=device)
        _fk[(robot, n)] = kin.compute_kinematics(q).robot_spheres.reshape(n, -1, 4).clone()
    return _fk[(robot, n)]


def sweep_table(model):
    """candidate table of the model + (franka) the placeholder link: a group whose pairs all have one disabled sphere, and a last
    group made of disabled spheres only"""
    from curobo_amd.robot.collision_matrix import candidate_link_pairs, link_pair_table

    link_pairs, locs, grp = candidate_link_pairs(model)
    G = len(link_pairs)
    dead = []
    if "attached_object" in model.link_names:
        a = model.link_names.index("attached_object")
        assert (model.link_spheres[0][np.asarray(model.link_sphere_idx_map) == a, 3] < 0).all()
        link_pairs = np.concatenate([link_pairs, [[model.link_names.index("panda_link0"), a]]])
        locs, grp = link_pair_table(model, link_pairs)
        s = np.nonzero(np.asarray(model.link_sphere_idx_map) == a)[0]
        only = np.asarray([(s[x], s[y]) for x in range(len(s)) for y in range(x + 1, len(s))], np.int16)
        locs = np.concatenate([locs, only])
        grp = np.concatenate([grp, np.full(len(only), G + 1, np.int32)])
        dead, G = [G, G + 1], G + 2
    return locs, grp, G, dead


def tolerance(sph, padding):
    """16 * 2^-23 * max(1, max |coordinate| + max radius): fp32 rounding of three differences, a sum of squares, a root and two
    sums"""
    r = sph[..., 3] + np.asarray(padding)[None]
    return 16.0 * 2.0 ** -23 * max(1.0, float(np.abs(sph[..., :3]).max()) + float(r[r >= 0].max()))


def run_sweep(sph_d, padding, locs, grp, G, device, **kw):
    import torch

    from curobo_amd.backends.geometry import link_pair_sweep

    mx = torch.full((G,), 7.0, device=device)
    cnt = torch.full((G,), 7, dtype=torch.int32, device=device)
    link_pair_sweep(mx, cnt, sph_d, torch.as_tensor(np.asarray(padding, np.float32), device=device), torch.as_tensor(locs, device=device),
                    torch.as_tensor(grp, device=device), G, **kw)
    torch.cuda.synchronize()
    return mx, cnt


@pytest.mark.parametrize("robot,n,padded", [("ur10e", 1, False), ("ur10e", 3, False), ("franka", 130, False), ("dual_ur10e", 65, False),
                                            ("unitree_g1", 5, False), ("franka", 130, True)])
def test_sweep_against_float64(robot, n, padded, device):
    """Largest |max_penetration - float64| seen on the MI355X, per case in the order below: 6.7e-8, 4.6e-8, 1.5e-8, 3.4e-8,
    4.2e-8 and 2.3e-8 m, against tolerances of 1.9e-6 to 1.7e-5 m; no group came within the tolerance of zero at any point, so
    every count was compared."""
    model = load_model(robot)
    locs, grp, G, dead = sweep_table(model)
    if robot == "unitree_g1":
        assert G == 1128 and len(locs) > 200000 and len(locs) % 64 != 0
    padding = np.random.default_rng(11).uniform(0.0, 0.03, model.num_spheres).astype(np.float32) if padded else model.sphere_padding
    sph_d = fk_spheres(robot, n, device)
    sph = sph_d.cpu().numpy()
    key = (robot, n, padded)
    if key not in _ref:
        _ref[key] = sweep_ref(sph, padding, locs, grp, G)
    want_max, want_cnt, point = _ref[key]
    mx, cnt = run_sweep(sph_d, padding, locs, grp, G, device)
    got_max, got_cnt = mx.cpu().numpy(), cnt.cpu().numpy()
    tol = tolerance(sph, padding)
    finite = np.isfinite(want_max)
    assert np.array_equal(np.isneginf(got_max), ~finite) and not np.isnan(got_max).any()
    for g in dead:
        assert got_max[g] == -np.inf and got_cnt[g] == 0
    err = np.abs(got_max[finite].astype(np.float64) - want_max[finite])
    near = (np.abs(point) <= tol).any(axis=0)
    print(f"link_pair_sweep {robot} N={n} padded={padded}: G={G} P={len(locs)} max err {err.max():.3e} (tolerance {tol:.3e}), "
          f"{int(near.sum())} groups within the tolerance of zero at some point, {int((want_cnt > 0).sum())} colliding groups")
    assert err.max() <= tol
    assert near.sum() <= 0.01 * G
    assert np.array_equal(got_cnt[~near], want_cnt[~near])
    assert (want_cnt > 0).any() or n < 65, "the larger inputs must contain self collisions"


def test_sweep_split_invariance_and_determinism(device):
    import torch

    model = load_model("franka")
    locs, grp, G, _ = sweep_table(model)
    sph_d = fk_spheres("franka", 130, device)
    base = run_sweep(sph_d, model.sphere_padding, locs, grp, G, device)
    for kw in ({}, {"points_per_workgroup": 1}, {"points_per_workgroup": 7}, {"points_per_workgroup": 130}):
        mx, cnt = run_sweep(sph_d, model.sphere_padding, locs, grp, G, device, **kw)
        assert torch.equal(mx.view(torch.int32), base[0].view(torch.int32)) and torch.equal(cnt, base[1]), kw
    # accumulate: two halves folded on the device give the whole
    from curobo_amd.backends.geometry import link_pair_sweep

    t = lambda a: torch.as_tensor(a, device=device)  # noqa: E731
    mx, cnt = run_sweep(sph_d[:60].contiguous(), model.sphere_padding, locs, grp, G, device)
    link_pair_sweep(mx, cnt, sph_d[60:].contiguous(), t(model.sphere_padding), t(locs), t(grp), G, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(mx.view(torch.int32), base[0].view(torch.int32)) and torch.equal(cnt, base[1])


def test_sweep_limits(device):
    import torch

    from curobo_amd.backends.geometry import link_pair_sweep

    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=device)  # noqa: E731
    with pytest.raises(ValueError, match="1024"):
        link_pair_sweep(z(1), z(1, dt=torch.int32), z(2, 1025, 4), z(1025), z(1, 2, dt=torch.int16), z(1, dt=torch.int32), 1)
    with pytest.raises(ValueError, match="4096"):
        link_pair_sweep(z(4097), z(4097, dt=torch.int32), z(2, 8, 4), z(8), z(1, 2, dt=torch.int16), z(1, dt=torch.int32), 4097)


def pairs_of(ignore, skip=()):
    return {frozenset((a, b)) for a, v in ignore.items() for b in v} - {frozenset(p) for p in skip}


@pytest.mark.parametrize("robot,m", [("ur10e", 512), ("franka", 512), ("unitree_g1", 64)])
def test_matrix_against_float64(robot, m, device):
    """default_colliding, never_colliding and ignore equal the float64 four-step result on the same fp32 spheres.  A link pair
    may be left out when its float64 maximum over the samples is within 1e-4 m of zero: the project's FK sphere tolerance of
    1e-5 on two centres and two radii (about 5.5e-5 m), rounded up; at most 2 % of the candidates."""
    import torch

    from curobo_amd.robot.collision_matrix import compute_self_collision_matrix

    kin = kin_of(robot, device)
    model = kin.config.model
    q = sample_q(model, m, seed=3)
    got = compute_self_collision_matrix(kin, samples=torch.as_tensor(q), batch_size=200)
    s_sph = kin.compute_kinematics(torch.as_tensor(q, device=device)).robot_spheres.reshape(m, -1, 4).cpu().numpy()
    d_sph = kin.compute_kinematics(kin.default_joint_position.view(1, -1)).robot_spheres.reshape(1, -1, 4).cpu().numpy()
    ref = matrix_ref(model, d_sph, s_sph)
    assert got.link_pairs == ref["link_pairs"] and got.num_samples == m
    G = len(got.link_pairs)
    out = [p for p, v in zip(ref["link_pairs"], ref["max_penetration"]) if abs(v) <= 1e-4]
    print(f"self-collision matrix {robot} M={m}: G={G}, {len(out)} link pairs within 1e-4 m of zero, {len(ref['default_colliding'])} default-"
          f"colliding, {len(ref['never_colliding'])} never colliding, max |max_penetration - float64| "
          f"{np.abs(got.max_penetration - ref['max_penetration']).max():.3e}")
    assert len(out) <= 0.02 * G
    keep = lambda ps: [p for p in ps if p not in out]  # noqa: E731
    assert keep(got.default_colliding) == keep(ref["default_colliding"])
    assert keep(got.never_colliding) == keep(ref["never_colliding"])
    assert pairs_of(got.ignore, out) == pairs_of(ref["ignore"], out)
    assert np.abs(got.max_penetration - ref["max_penetration"]).max() <= tolerance(s_sph, model.sphere_padding)
    live = np.asarray([p not in out for p in ref["link_pairs"]])
    assert np.array_equal(got.collision_count[live] > 0, ref["collision_count"][live] > 0)


def self_cost(sph_d, pairs, padding, device):
    import torch

    from curobo_amd.backends import geometry as G

    n, S = sph_d.shape[0], sph_d.shape[1]
    P = len(pairs)
    out_d = torch.full((n, 1), -1.0, device=device)
    G.self_collision_distance(out_d, torch.zeros(n, S, 4, device=device), torch.zeros(1, device=device),
                              torch.zeros(n, S, dtype=torch.uint8, device=device), sph_d, torch.as_tensor(padding, device=device),
                              torch.ones(1, device=device), torch.as_tensor(np.ascontiguousarray(pairs), device=device),
                              torch.zeros(1, device=device), torch.zeros(2, dtype=torch.int16, device=device), 1, 256, n, 1, S, P, False, False)
    torch.cuda.synchronize()
    return out_d


def test_nothing_lost_by_pruning(device):
    """at every sampled configuration the self-collision cost over the pruned pairs is the cost over all candidates but the
    default-colliding ones"""
    import torch

    from curobo_amd.robot.collision_matrix import candidate_link_pairs, compute_self_collision_matrix, pruned_collision_pairs

    kin = kin_of("ur10e", device)
    model = kin.config.model
    q = torch.as_tensor(sample_q(model, 256, seed=3))
    matrix = compute_self_collision_matrix(kin, samples=q, batch_size=200)
    assert matrix.never_colliding and len(matrix.never_colliding) < len(matrix.link_pairs)
    pruned, padding = pruned_collision_pairs(model, matrix)
    link_pairs, locs, grp = candidate_link_pairs(model)
    names = [(model.link_names[a], model.link_names[b]) for a, b in link_pairs]
    keep = np.asarray([n not in matrix.default_colliding for n in names])
    full = locs[keep[grp]]
    assert np.array_equal(padding, model.sphere_padding)
    sph_d = kin.compute_kinematics(q.to(device)).robot_spheres.reshape(256, -1, 4).clone()
    a, b = self_cost(sph_d, pruned, padding, device), self_cost(sph_d, full, model.sphere_padding, device)
    assert torch.equal(a, b) and (b > 0).any()


def test_halton_path_is_reproducible(device):
    from curobo_amd.robot.collision_matrix import compute_self_collision_matrix

    kin = kin_of("franka", device)
    a = compute_self_collision_matrix(kin, num_samples=2, batch_size=300)
    b = compute_self_collision_matrix(kin, num_samples=2, batch_size=300)
    assert a.num_samples == 600 and b.num_samples == 600
    assert a.link_pairs == b.link_pairs and a.ignore == b.ignore and a.default_colliding == b.default_colliding
    assert a.never_colliding == b.never_colliding and np.array_equal(a.collision_count, b.collision_count)
    assert np.array_equal(a.max_penetration.view(np.int32), b.max_penetration.view(np.int32))
    assert len(a.link_pairs) == 46 and 0 < len(a.never_colliding) < 46 and (a.collision_count <= 600).all()


def test_robot_builder_end_to_end(tmp_path, device):
    import torch

    from curobo_amd.kinematics import Kinematics, KinematicsCfg
    from curobo_amd.robot.builder import RobotBuilder
    from test_collision_matrix_host import ARM_SPHERES, write_arm

    b = RobotBuilder(write_arm(tmp_path), tool_frames=["tip"], device=str(device))
    b.set_collision_spheres(ARM_SPHERES)
    ignore = b.compute_collision_matrix(num_samples=2, batch_size=200)
    stats = b.collision_matrix_statistics
    assert stats.num_samples == 400 and stats.link_pairs == [("base", "l2"), ("base", "l3"), ("l1", "l3")]
    # (base, l2) cannot collide: closed form in test_collision_matrix_host, here over the joint range widened by 0.1 rad, where the
    # bound is 0.08 - sqrt(0.3^2 + 0.25^2 + 2 * 0.3 * 0.25 * cos(2.6)) = -0.0748; (base, l3) does (8 of these 400 samples)
    assert ("base", "l2") in stats.never_colliding and stats.max_penetration[0] < -0.074
    assert "l2" in ignore["base"] and "l3" not in ignore["base"] and b.collision_matrix is ignore
    assert stats.collision_count[1] > 0 and stats.max_penetration[1] <= 0.09 + 1e-6
    cfg = b.build()
    kin = Kinematics(KinematicsCfg.from_data_dict(cfg, device=str(device)))
    pairs = kin.kinematics_config.self_collision.collision_pairs.cpu().numpy()
    assert [0, 2] not in pairs.tolist() and [0, 3] not in pairs.tolist()
    t = 2.0 * np.pi / 3.0
    q = torch.tensor([[0.0, 0.0, 0.0], [0.3, t, t]], device=device)
    sph_d = kin.compute_kinematics(q).robot_spheres.reshape(2, -1, 4).clone()
    cost = self_cost(sph_d, pairs, kin.config.model.sphere_padding, device).cpu().numpy().reshape(-1)
    # the closed triangle puts l3's sphere on the base's: cost = 0.5 * (r^2 - d^2) = 0.5 * 0.09^2
    assert cost[0] == 0.0 and abs(cost[1] - 0.5 * 0.09 ** 2) < 1e-5
