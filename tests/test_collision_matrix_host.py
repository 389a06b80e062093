"""What the self-collision matrix builder promises without a GPU: the candidate link pairs and their sphere-pair table, the
float64 restatement of the sweep against a closed-form case, the RobotBuilder dictionary round trip and its members."""

import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from collision_matrix_ref import matrix_ref, sweep_ref  # noqa: E402
from conftest import load_model  # noqa: E402

# A planar arm of four links that carry spheres, base - l1 - l2 - l3, three revolute joints about z with limits +-2.5 rad;
# every link is LEN long (the next joint sits at (LEN, 0, 0) of its parent); a sphere-less tool frame `tip` is fixed to l3.
LEN = 0.3
ARM_URDF = """<?xml version="1.0"?>
<robot name="planar_arm">
  <link name="base"/><link name="l1"/><link name="l2"/><link name="l3"/><link name="tip"/>
  <joint name="j1" type="revolute"><parent link="base"/><child link="l1"/><origin xyz="0 0 0" rpy="0 0 0"/>
    <axis xyz="0 0 1"/><limit lower="-2.5" upper="2.5" velocity="1.0" effort="10.0"/></joint>
  <joint name="j2" type="revolute"><parent link="l1"/><child link="l2"/><origin xyz="0.3 0 0" rpy="0 0 0"/>
    <axis xyz="0 0 1"/><limit lower="-2.5" upper="2.5" velocity="1.0" effort="10.0"/></joint>
  <joint name="j3" type="revolute"><parent link="l2"/><child link="l3"/><origin xyz="0.3 0 0" rpy="0 0 0"/>
    <axis xyz="0 0 1"/><limit lower="-2.5" upper="2.5" velocity="1.0" effort="10.0"/></joint>
  <joint name="j_tip" type="fixed"><parent link="l3"/><child link="tip"/><origin xyz="0.3 0 0" rpy="0 0 0"/></joint>
</robot>
"""
# hand-placed spheres: base at its origin, l1 and l2 at mid-link, l3 at its far end (+ one disabled placeholder)
ARM_SPHERES = {
    "base": [{"center": [0.0, 0.0, 0.0], "radius": 0.05}],
    "l1": [{"center": [0.15, 0.0, 0.0], "radius": 0.04}],
    "l2": [{"center": [0.15, 0.0, 0.0], "radius": 0.04}, {"center": [0.25, 0.0, 0.0], "radius": 0.03}],
    "l3": [{"center": [0.3, 0.0, 0.0], "radius": 0.04}, {"center": [0.1, 0.0, 0.0], "radius": -100.0}],
}


def write_arm(tmp_path):
    path = os.path.join(str(tmp_path), "planar_arm.urdf")
    with open(path, "w") as fh:
        fh.write(ARM_URDF)
    return path


def arm_builder(tmp_path):
    from curobo_amd.robot.builder import RobotBuilder

    b = RobotBuilder(write_arm(tmp_path), tool_frames=["tip"], device="cpu")
    b.set_collision_spheres(ARM_SPHERES)
    return b


def arm_model(tmp_path):
    from curobo_amd.robot import build_robot_model
    from curobo_amd.robot.urdf import load_urdf

    b = arm_builder(tmp_path)
    cfg = b.build()
    return build_robot_model(cfg, load_urdf(cfg["urdf_path"]))


def planar_spheres(q):
    """closed-form world spheres [N, 6, 4] (float64) of the arm in the model's sphere order: joint k sits at the end of link
    k - 1, link k points along the sum of the first k angles"""
    q = np.atleast_2d(np.asarray(q, np.float64))
    a1, a2, a3 = q[:, 0], q[:, 0] + q[:, 1], q[:, 0] + q[:, 1] + q[:, 2]
    u = lambda a: np.stack([np.cos(a), np.sin(a), 0 * a], -1)  # noqa: E731
    j2 = LEN * u(a1)
    j3 = j2 + LEN * u(a2)
    out = np.zeros((len(q), 6, 4))
    out[:, 0, 3] = 0.05
    out[:, 1, :3], out[:, 1, 3] = 0.15 * u(a1), 0.04
    out[:, 2, :3], out[:, 2, 3] = j2 + 0.15 * u(a2), 0.04
    out[:, 3, :3], out[:, 3, 3] = j2 + 0.25 * u(a2), 0.03
    out[:, 4, :3], out[:, 4, 3] = j3 + 0.3 * u(a3), 0.04
    out[:, 5, :3], out[:, 5, 3] = j3 + 0.1 * u(a3), -100.0
    return out


def test_candidate_link_pairs_on_the_planar_arm(tmp_path):
    from curobo_amd.robot.collision_matrix import candidate_link_pairs, neighbor_ignore

    model = arm_model(tmp_path)
    assert model.link_names == ["base", "l1", "l2", "l3", "tip"]
    # the reference's neighbour table: every link but the base ignores its parent and the parent ignores it, in link order
    assert neighbor_ignore(model) == {"l1": ["base", "l2"], "base": ["l1"], "l2": ["l1", "l3"], "l3": ["l2", "tip"], "tip": ["l3"]}
    link_pairs, locs, grp = candidate_link_pairs(model)
    names = [(model.link_names[a], model.link_names[b]) for a, b in link_pairs]
    assert names == [("base", "l2"), ("base", "l3"), ("l1", "l3")]  # 4 links with spheres: 6 pairs - 3 neighbours; tip has none
    # spheres: base 0; l1 1; l2 2, 3; l3 4, 5 (5 is disabled: it stays in the table, the kernel skips it)
    assert locs.dtype == np.int16 and grp.dtype == np.int32
    assert locs.tolist() == [[0, 2], [0, 3], [0, 4], [0, 5], [1, 4], [1, 5]]
    assert grp.tolist() == [0, 0, 1, 1, 2, 2]
    # an ignore counts in either direction
    for ignore in ({"base": ["l3"]}, {"l3": ["base"]}):
        lp, lo, gr = candidate_link_pairs(model, ignore)
        assert [(model.link_names[a], model.link_names[b]) for a, b in lp] == [("base", "l2"), ("l1", "l3")]
        assert lo.tolist() == [[0, 2], [0, 3], [1, 4], [1, 5]] and gr.tolist() == [0, 0, 1, 1]
    # a link whose only spheres are disabled is no candidate
    model.link_spheres[0][4, 3] = -100.0
    lp, _, _ = candidate_link_pairs(model)
    assert [(model.link_names[a], model.link_names[b]) for a, b in lp] == [("base", "l2")]


@pytest.mark.parametrize("robot,groups", [("ur10e", 10), ("franka", 46), ("dual_ur10e", 81), ("unitree_g1", 1128)])
def test_candidate_groups_are_contiguous_runs(robot, groups):
    from curobo_amd.robot.collision_matrix import candidate_link_pairs

    model = load_model(robot)
    link_pairs, locs, grp = candidate_link_pairs(model)
    assert len(link_pairs) == groups
    assert (np.diff(grp) >= 0).all() and grp[0] == 0 and grp[-1] == groups - 1 and len(np.unique(grp)) == groups
    assert (locs[:, 0] < locs[:, 1]).all()
    key = grp.astype(np.int64) * (1 << 32) + locs[:, 0].astype(np.int64) * (1 << 16) + locs[:, 1]
    assert (np.diff(key) > 0).all(), "ordered by group, then (i, j), no pair twice"
    sl = np.asarray(model.link_sphere_idx_map, np.int64)
    assert (np.sort(sl[locs.astype(np.int64)], axis=1) == link_pairs[grp]).all()


def test_packaged_franka_pairs_are_candidates():
    """46 groups; every packaged sphere pair that can ever contribute (both spheres enabled) is among the candidates.  The
    other packaged pairs all involve one of the four disabled placeholder spheres of ``attached_object``, a link that carries
    no enabled sphere and is therefore no candidate link."""
    from curobo_amd.robot.collision_matrix import candidate_link_pairs

    model = load_model("franka")
    link_pairs, locs, _ = candidate_link_pairs(model)
    assert len(link_pairs) == 46
    have = {(int(i), int(j)) for i, j in locs}
    r = model.link_spheres[0][:, 3]
    packaged = [(int(i), int(j)) for i, j in model.collision_pairs]
    live = [p for p in packaged if r[p[0]] >= 0 and r[p[1]] >= 0]
    assert len(live) == 818 - 124 and all(p in have for p in live)
    placeholder = set(np.nonzero(np.asarray(model.link_sphere_idx_map) == model.link_names.index("attached_object"))[0].tolist())
    assert all(p[0] in placeholder or p[1] in placeholder for p in packaged if p not in have)


def test_reference_sweep_closed_form(tmp_path, oracle):
    """The float64 restatement on the planar arm.

    (base, l3) MEETS: with q2 = q3 = 2 pi / 3 (inside +-2.5) the three links close an equilateral triangle of side LEN, so
    the far end of l3 -- where its sphere sits -- returns to the base origin, where the base sphere sits: distance 0,
    penetration 0.05 + 0.04 = 0.09 m, for every q1.
    (base, l2) CANNOT: joint 2 is always LEN = 0.3 from the base origin and the l2 spheres are 0.15 / 0.25 along l2 from joint
    2, so by the triangle inequality they are at least 0.3 - 0.15 = 0.15 / 0.3 - 0.25 = 0.05 from the origin; the penetrations are
    at most 0.05 + 0.04 - 0.15 = -0.06 and 0.05 + 0.03 - 0.05 = +0.03.  The second bound would collide, but it needs |q2| = pi;
    within |q2| <= 2.5 the 0.25 sphere is sqrt(0.3^2 + 0.25^2 + 2 * 0.3 * 0.25 * cos(2.5)) = 0.17992 from the origin:
    penetration <= 0.08 - 0.17992 = -0.09992 there, and the 0.15 sphere gives 0.09 - sqrt(0.09 + 0.0225 + 0.09 cos(2.5)) =
    -0.11110: the pair's maximum over the whole joint range is -0.09992 m, attained at q2 = +-2.5."""
    from curobo_amd.robot.collision_matrix import candidate_link_pairs

    model = arm_model(tmp_path)
    _, locs, grp = candidate_link_pairs(model)
    t = 2.0 * math.pi / 3.0
    q = np.array([[0.0, 0.0, 0.0], [0.4, t, t], [-1.1, -t, -t], [0.3, 2.5, 0.0], [0.0, -2.5, 1.0], [0.2, 1.0, -0.7]])
    sph = planar_spheres(q)
    # the closed-form spheres are the model's (the project's FK oracle on the model built from the URDF, fp32)
    fk = oracle.kinematics_forward(q.astype(np.float32), model.as_dict())["robot_spheres"]
    np.testing.assert_allclose(fk, sph, atol=2e-6)
    mx, cnt, point = sweep_ref(sph, model.sphere_padding, locs, grp, 3)
    assert point.shape == (6, 3)
    np.testing.assert_allclose(point[1:3, 1], 0.09, atol=1e-12)  # (base, l3) at the two closing configurations
    assert abs(mx[1] - 0.09) < 1e-12 and cnt[1] == 2
    far = math.sqrt(0.3 ** 2 + 0.25 ** 2 + 2 * 0.3 * 0.25 * math.cos(2.5))
    np.testing.assert_allclose(point[3:5, 0], 0.08 - far, atol=1e-12)  # (base, l2) at |q2| = 2.5: its maximum
    assert abs(mx[0] - (0.08 - far)) < 1e-12 and cnt[0] == 0
    # over a grid of the whole joint range (base, l2) never exceeds that bound and (base, l3) does collide
    g = np.linspace(-2.5, 2.5, 21)
    grid = np.stack(np.meshgrid([0.0], g, g, indexing="ij"), -1).reshape(-1, 3)
    mx, cnt, _ = sweep_ref(planar_spheres(grid), model.sphere_padding, locs, grp, 3)
    assert abs(mx[0] - (0.08 - far)) < 1e-12 and cnt[0] == 0 and cnt[1] > 0
    # a group of disabled spheres only: -inf, 0; padding is added to both radii
    mx, cnt, _ = sweep_ref(sph, model.sphere_padding, np.array([[0, 5]], np.int16), np.array([0], np.int32), 1)
    assert mx[0] == -np.inf and cnt[0] == 0
    pad = np.full(6, 0.01, np.float32)
    mx, _, _ = sweep_ref(sph, pad, locs, grp, 3)
    assert abs(mx[1] - (0.09 + 2 * float(pad[0]))) < 1e-12


def test_reference_matrix_on_the_planar_arm(tmp_path):
    model = arm_model(tmp_path)
    g = np.linspace(-2.5, 2.5, 21)
    grid = np.stack(np.meshgrid([0.0], g, g, indexing="ij"), -1).reshape(-1, 3)
    t = 2.0 * math.pi / 3.0
    samples = planar_spheres(np.concatenate([grid, [[0.0, t, t]]]))
    ref = matrix_ref(model, planar_spheres([0.0, 0.0, 0.0]), samples)
    assert ref["link_pairs"] == [("base", "l2"), ("base", "l3"), ("l1", "l3")]
    assert ref["default_colliding"] == [] and ("base", "l2") in ref["never_colliding"] and ("base", "l3") not in ref["never_colliding"]
    assert "l2" in ref["ignore"]["base"] and "l3" not in ref["ignore"]["base"]
    # a default position that closes the triangle: (base, l3) is a false positive of the sphere model and joins the table
    ref2 = matrix_ref(model, planar_spheres([0.0, t, t]), samples, custom_ignore={"l3": ["l1"]}, prune_collisions=False)
    assert ref2["link_pairs"] == [("base", "l2"), ("base", "l3")]  # (l1, l3) left through custom_ignore, written l3 -> l1
    assert ref2["default_colliding"] == [("base", "l3")] and ref2["ignore"]["base"] == ["l1", "l3"]
    assert ref2["never_colliding"] == [("base", "l2")] and "l2" not in ref2["ignore"]["base"]  # found, not pruned


def test_robot_builder_round_trip(tmp_path):
    """build() -> build_robot_model gives the collision pairs of pruned_collision_pairs under the same matrix, also through a
    saved file"""
    from curobo_amd.robot import build_robot_model, load_robot_model
    from curobo_amd.robot.builder import RobotBuilder
    from curobo_amd.robot.collision_matrix import SelfCollisionMatrix, pruned_collision_pairs
    from curobo_amd.robot.urdf import load_urdf

    b = arm_builder(tmp_path)
    assert b.tool_frames == ["tip"] and b.collision_link_names == ["base", "l1", "l2", "l3"] and b.num_spheres == 6
    assert b.collision_matrix is None and b.collision_spheres["l3"][1]["radius"] == -100.0
    model = arm_model(tmp_path)
    g = np.linspace(-2.5, 2.5, 11)
    grid = np.stack(np.meshgrid([0.0], g, g, indexing="ij"), -1).reshape(-1, 3)
    ref = matrix_ref(model, planar_spheres([0.0, 0.0, 0.0]), planar_spheres(grid))
    matrix = SelfCollisionMatrix(ref["link_pairs"], ref["max_penetration"], ref["collision_count"], len(grid), ref["default_colliding"],
                                 ref["never_colliding"], ref["ignore"])
    for k, v in matrix.ignore.items():
        b.add_collision_ignore(k, v)
    assert b.collision_matrix == matrix.ignore
    cfg = b.build()
    assert cfg["self_collision_ignore"] == matrix.ignore and cfg["collision_link_names"] == ["base", "l1", "l2", "l3"]
    want_pairs, want_pad = pruned_collision_pairs(model, matrix)
    built = build_robot_model(cfg, load_urdf(cfg["urdf_path"]))
    assert np.array_equal(built.collision_pairs, want_pairs) and np.array_equal(built.sphere_padding, want_pad)
    assert want_pairs.tolist() == [[0, 4], [0, 5], [1, 4], [1, 5]]  # (base, l2) never collides: only l3's pairs are left
    # ... and through YAML: save -> load_robot_model, save -> from_config -> build
    out = os.path.join(str(tmp_path), "out", "planar_arm.yml")
    b.save(cfg, out)
    assert np.array_equal(load_robot_model(out, "").collision_pairs, want_pairs)
    b2 = RobotBuilder.from_config(out, device="cpu")
    assert b2.collision_matrix == matrix.ignore and b2.collision_spheres == b.collision_spheres and b2.tool_frames == ["tip"]
    cfg2 = b2.build()
    assert {k: cfg2[k] for k in cfg} == cfg


def test_add_and_remove_collision_ignore(tmp_path):
    b = arm_builder(tmp_path)
    b.add_collision_ignore("base", ["l2", "l3"])
    b.add_collision_ignore("base", ["l3"])  # no duplicate
    b.add_collision_ignore("l1", ["l3"])
    assert b.collision_matrix == {"base": ["l2", "l3"], "l1": ["l3"]}
    b.remove_collision_ignore("base", ["l2", "tip"])  # (an entry that is not there is left alone)
    b.remove_collision_ignore("l2", ["l3"])
    assert b.collision_matrix == {"base": ["l3"], "l1": ["l3"]}
    assert b.build()["self_collision_ignore"] == {"base": ["l3"], "l1": ["l3"]}
    with pytest.raises(ValueError, match="nolink"):
        b.set_collision_spheres({"nolink": []})


@pytest.mark.parametrize("member,missing", [("fit_collision_spheres", "mesh sphere fitting"), ("refit_link_spheres", "mesh sphere fitting"),
                                            ("visualize", "viewer"), ("save_xrdf", "XRDF writer")])
def test_members_this_library_lacks_say_so(tmp_path, member, missing):
    with pytest.raises(NotImplementedError, match=missing):
        getattr(arm_builder(tmp_path), member)()


def test_build_without_a_matrix_ignores_neighbours(tmp_path):
    cfg = arm_builder(tmp_path).build()
    assert cfg["self_collision_ignore"] == {"l1": ["base", "l2"], "base": ["l1"], "l2": ["l1", "l3"], "l3": ["l2", "tip"], "tip": ["l3"]}


def test_sweep_limits_are_refused_before_any_launch():
    """S <= 1024, G <= 4096: ValueError from the wrapper, on host tensors (nothing is launched)"""
    import torch

    from curobo_amd.backends.geometry import link_pair_sweep

    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)  # noqa: E731
    with pytest.raises(ValueError, match="1024"):
        link_pair_sweep(z(1), z(1, dt=torch.int32), z(2, 1025, 4), z(1025), z(1, 2, dt=torch.int16), z(1, dt=torch.int32), 1)
    with pytest.raises(ValueError, match="4096"):
        link_pair_sweep(z(4097), z(4097, dt=torch.int32), z(2, 8, 4), z(8), z(1, 2, dt=torch.int16), z(1, dt=torch.int32), 4097)


def test_facade_and_abi():
    import importlib.util

    from curobo_amd import _lib

    assert "curobo_hip_link_pair_sweep" in _lib.declared_symbols() and hasattr(_lib.load(), "curobo_hip_link_pair_sweep")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_facade_curobo_robot_builder", os.path.join(root, "curobo", "robot_builder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from curobo_amd.robot.builder import RobotBuilder

    assert mod.RobotBuilder is RobotBuilder
