"""Every kinematics and dynamics launch on the joint-zoo robot (tests/joint_zoo.py: all six joint types, a prismatic joint
behind a rotation, multipliers outside {+-1}, biases, two dofs with two links each) against the float64 restatements.

Bound: ``g`` is the largest gap between the reference's own fp32 result (tests/golden/joint_zoo.npz, recorded from the
reference's kernels) and float64 for the quantity, pooled over the golden's 65 points; the HIP result must lie within 4 g of
float64 (4: another summation order and FMA contraction).  Gradients and torques are taken relative to the largest float64
entry.  Where the reference is wrong (tests/test_oracle_joint_zoo.py) g is taken where it is right: dJ/dq on the tool frames
without a mimic link, RNEA without velocity on the prismatic dofs; the HIP kernels are held to float64 everywhere.  Every
comparison prints g and the kernel's gap first (``pytest -s``).  Batches: 1 point, 17 (a ragged last 16-lane row group), 65 (one
point past a 64-point workgroup)."""

import dataclasses

import numpy as np
import pytest
import torch

import joint_zoo as Z
from joint_zoo import gap, held

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kp(device):
    from curobo_amd.robot.kinematics_params import KinematicsParams

    return KinematicsParams.from_model(Z.model(), device)


def _forward(kp, q, mode, com=True):
    """mode: "pose" | "spheres" | "jacobian" -> dictionary of numpy arrays"""
    from curobo_amd.backends import kinematics as K

    dev = kp.device
    n, d = q.shape
    T, S, L = kp.num_pose_links, kp.num_spheres, kp.num_links
    tq = torch.as_tensor(np.array(q), device=dev)  # (a copy: the shared inputs are read-only)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731  (every output must be written)
    o = dict(link_pos=nan(n, T, 3), link_quat=nan(n, T, 4), com=nan(n, 4), cumul=nan(n, L, 3, 4))
    env = torch.zeros(n, dtype=torch.int32, device=dev)
    if mode == "pose":
        K.launch_kinematics_forward(o["link_pos"], o["link_quat"], o["com"], o["cumul"], tq, kp.fixed_transforms, kp.link_masses_com,
                                    kp.joint_map_type, kp.joint_map, kp.link_map, kp.tool_frame_map, kp.joint_offset_map, n, 1, d, com)
    elif mode == "spheres":
        o["spheres"] = nan(n, S, 4)
        K.launch_kinematics_forward_spheres(
            o["link_pos"], o["link_quat"], o["spheres"], o["com"], o["cumul"], tq, kp.fixed_transforms, kp.link_spheres,
            kp.link_masses_com, kp.joint_map_type, kp.joint_map, kp.link_map, kp.tool_frame_map, kp.link_sphere_idx_map,
            kp.joint_offset_map, env, kp.num_envs, n, 1, d, S, 32, True, com)
    else:
        o["spheres"], o["jac"] = nan(n, S, 4), nan(n, T, 6, d)
        K.launch_kinematics_forward_spheres_jacobian(
            o["link_pos"], o["link_quat"], o["spheres"], o["com"], o["jac"], o["cumul"], tq, kp.fixed_transforms, kp.link_spheres,
            kp.link_masses_com, kp.joint_map_type, kp.joint_map, kp.link_map, kp.tool_frame_map, kp.link_sphere_idx_map,
            kp.link_chain_data, kp.link_chain_offsets, kp.joint_links_data, kp.joint_links_offsets, kp.joint_affects_endeffector,
            kp.joint_offset_map, env, kp.num_envs, n, 1, d, S, 32, True, com)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("n", Z.BATCHES)
@pytest.mark.parametrize("mode", ["pose", "spheres", "jacobian"])
def test_forward(mode, n, kp):
    m, z, e = Z.model(), Z.golden(), Z.expected()
    g = e["g"]
    got = _forward(kp, z["q"][:n], mode)
    tag = f"{mode} n={n}"
    held(f"{tag} tool positions", got["link_pos"], e["pos"][:n], g["pos"])
    held(f"{tag} tool rotations R(quat)", Z.quat_to_matrix(got["link_quat"]), e["rot"][:n], g["rot"])
    np.testing.assert_allclose(np.linalg.norm(got["link_quat"], axis=-1), 1.0, rtol=0, atol=4e-7)
    held(f"{tag} cumulative transforms", got["cumul"], e["T"][:n, :, :3], g["cumul"])
    held(f"{tag} centre of mass", got["com"][:, :3], e["com"][:n, :3], g["com"])
    np.testing.assert_allclose(got["com"][:, 3], e["com"][:n, 3], rtol=6e-7)  # the total mass: 10 fp32 additions, an ulp each
    if mode != "pose":
        held(f"{tag} spheres", got["spheres"][..., :3], e["spheres"][:n, :, :3], g["spheres"])
        np.testing.assert_array_equal(got["spheres"][..., 3], np.broadcast_to(m.link_spheres[0, :, 3], (n, m.num_spheres)))
        assert (got["spheres"][..., 3] == -100.0).sum() == n  # the disabled radius is kept
    if mode == "jacobian":
        held(f"{tag} Jacobian", got["jac"], e["jacobian"][:n], g["jacobian"])


def _backward(kp, fwd, n, g_s=None, g_b=None, g_p=None, g_q=None, g_c=None, g_j=None):
    from curobo_amd.backends import kinematics as K

    dev = kp.device
    T, S, d = kp.num_pose_links, kp.num_spheres, kp.num_dof
    t = lambda a, *shape: torch.zeros(n, *shape, device=dev) if a is None else torch.as_tensor(np.array(a), device=dev)  # noqa: E731
    out = torch.full((n, d), float("nan"), device=dev)
    env = torch.zeros(n, dtype=torch.int32, device=dev)
    gp = t(g_p, T, 3)
    K.launch_kinematics_backward(
        out, gp, t(g_q, T, 4), t(g_s, S, 4), t(g_c, 4), torch.as_tensor(fwd["com"], device=dev), gp if g_j is None else t(g_j),
        torch.as_tensor(fwd["cumul"], device=dev), kp.link_spheres, kp.link_masses_com, kp.link_map, kp.joint_map, kp.joint_map_type,
        kp.tool_frame_map, kp.link_sphere_idx_map, kp.link_chain_data, kp.link_chain_offsets, kp.joint_links_data,
        kp.joint_links_offsets, kp.joint_affects_endeffector, kp.joint_offset_map, env, kp.num_envs, n, 1, d, S, g_c is not None,
        g_j is not None, grad_spheres_b=None if g_b is None else t(g_b))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n", Z.BATCHES)
def test_backward_per_link_form(n, kp):
    """the zoo's sphere table is grouped by link: the launch takes the per-link form of the sphere VJP"""
    m, z, e = Z.model(), Z.golden(), Z.expected()
    assert np.all(np.diff(m.link_sphere_idx_map) >= 0)
    q = z["q"][:n]
    fwd = _forward(kp, q, "jacobian")
    c = {k: z[k][:n] for k in ("g_spheres", "g_spheres_b", "g_pos", "g_quat", "g_com")}
    g = e["g"]["vjp"]
    # the golden's cotangents (what the reference's backward ran on)
    got = _backward(kp, fwd, n, c["g_spheres"], None, c["g_pos"], c["g_quat"], c["g_com"])
    scale = np.abs(e["vjp"]).max()
    held(f"VJP n={n}, spheres + position + quaternion + CoM", got / scale, e["vjp"][:n] / scale, g)
    # ... with the second sphere buffer on top
    both = c["g_spheres"].astype(np.float64) + c["g_spheres_b"] * np.array([1, 1, 1, 0.0])
    want = Z.vjp64(m, q, both, c["g_pos"], c["g_quat"], c["g_com"])
    got = _backward(kp, fwd, n, c["g_spheres"], c["g_spheres_b"], c["g_pos"], c["g_quat"], c["g_com"])
    held(f"VJP n={n}, all five cotangents", got / scale, want / scale, g)
    # each alone
    for name, kw64, kw in (("spheres", dict(g_spheres=c["g_spheres"]), dict(g_s=c["g_spheres"])),
                           ("second sphere buffer", dict(g_spheres=c["g_spheres_b"]), dict(g_b=c["g_spheres_b"])),
                           ("position", dict(g_pos=c["g_pos"]), dict(g_p=c["g_pos"])),
                           ("quaternion", dict(g_quat=c["g_quat"]), dict(g_q=c["g_quat"])),
                           ("CoM", dict(g_com=c["g_com"]), dict(g_c=c["g_com"]))):
        held(f"VJP n={n}, {name} alone", _backward(kp, fwd, n, **kw) / scale, Z.vjp64(m, q, **kw64) / scale, g)


@pytest.mark.parametrize("n", Z.BATCHES)
def test_backward_per_sphere_form(n, kp, device):
    """a sphere table that is NOT grouped by link (a seeded permutation): the per-sphere form, as in
    test_gpu_kernels.py::test_fk_backward_spheres_not_grouped_by_link"""
    m, z, e = Z.model(), Z.golden(), Z.expected()
    perm = np.random.default_rng(7).permutation(m.num_spheres)
    link_of = m.link_sphere_idx_map
    assert np.any(np.diff(link_of[perm]) < 0)
    kp_p = dataclasses.replace(kp, link_spheres=torch.as_tensor(np.ascontiguousarray(m.link_spheres[:, perm]), device=device),
                               link_sphere_idx_map=torch.as_tensor(np.ascontiguousarray(link_of[perm]), device=device).to(torch.int16))
    q = z["q"][:n]
    fwd = _forward(kp, q, "spheres")
    g_s = z["g_spheres"][:n]  # the cotangent of the UNPERMUTED spheres; sphere perm[i] sits at row i of the permuted table
    got = _backward(kp_p, fwd, n, np.ascontiguousarray(g_s[:, perm]))
    want = Z.vjp64(m, q, g_spheres=g_s)
    scale = np.abs(e["vjp"]).max()
    held(f"VJP n={n}, permuted sphere table", got / scale, want / scale, e["g"]["vjp"])


@pytest.mark.parametrize("n", Z.BATCHES)
def test_jacobian_gradient_on_all_tool_frames(n, kp):
    """dJ/dq on EVERY tool frame, the three behind the mimic link included, where the reference's kernel is wrong"""
    z, e = Z.golden(), Z.expected()
    fwd = _forward(kp, z["q"][:n], "jacobian")
    got = _backward(kp, fwd, n, g_j=z["w_jac"][:n])
    scale = np.abs(e["jac_grad"]).max()
    held(f"dJ/dq n={n}, all tool frames", got / scale, e["jac_grad"][:n] / scale, e["g"]["jac_grad"])


def test_jacobian_gradient_arm_by_arm(kp):
    """one launch of 6 x 17 points, block k with the cotangent on the Jacobian column of dof k alone: entry (k, i) of the result
    is then one arm of the kernel's dJ/dq, and float64 says that each arm contributes"""
    m, z, e = Z.model(), Z.golden(), Z.expected()
    n, D = 17, m.num_dof
    q, w = z["q"][:n], Z.column_cotangents(z["w_jac"][:n])
    want = Z.jacobian_grad_per_column64(m, q, z["w_jac"][:n])  # [D (k), n, D (i)]
    fwd = _forward(kp, np.tile(q, (D, 1)), "jacobian")
    got = _backward(kp, fwd, D * n, g_j=w.reshape(D * n, *w.shape[2:])).reshape(D, n, D)
    big = np.abs(want).max()
    for name, k, i in Z.JAC_GRAD_ARMS:
        assert np.abs(want[k, :, i]).max() > 0.02 * big, name
        held(f"dJ/dq arm '{name}' (column {k}, d/dq{i})", got[k, :, i] / big, want[k, :, i] / big, e["g"]["jac_grad"])
    held("dJ/dq, every (column, dof) pair", got / big, want / big, e["g"]["jac_grad"])


# ------------------------------------------------------------------------------------------------ inverse dynamics
def _rnea_args(kp, device):
    grav = torch.tensor([0, 0, 0, 0, 0, 9.81], device=device)
    return (kp.fixed_transforms, kp.link_masses_com, kp.link_inertias, kp.joint_map_type, kp.joint_map, kp.link_map,
            kp.joint_offset_map, grav, kp.link_level_offsets, kp.link_level_data)


@pytest.mark.parametrize("n", Z.BATCHES)
def test_rnea(n, kp, device, oracle):
    from curobo_amd.backends import dynamics as Dy

    m, z, e = Z.model(), Z.golden(), Z.expected()
    L, D = kp.num_links, kp.num_dof
    t = lambda a: torch.as_tensor(np.array(a), device=device)  # noqa: E731
    q, qd, qdd, w = (t(z[k][:n]) for k in ("q", "qd", "qdd", "w_tau"))
    args = _rnea_args(kp, device)
    new = lambda fill: [torch.full((n, D), fill, device=device) for _ in range(3)]  # noqa: E731

    def run(scratch, flags=0, fill=7.0, f_ext=None, want_gfe=False):
        tau, cache = torch.full((n, D), float("nan"), device=device), torch.zeros(n, L * 20, device=device)
        Dy.launch_rnea_forward(tau, q, qd, qdd, *args, cache, n, L, D, kp.n_tree_levels, 1, f_ext, scratch=scratch)
        gr = new(fill)
        gfe = torch.zeros(n, L, 6, device=device) if want_gfe else None
        Dy.launch_rnea_backward(*gr, w, q, qd, *args, cache, n, L, D, kp.n_tree_levels, 1, gfe, scratch=scratch,
                                scratch_holds_q_qd=bool(flags & 1), accumulate=bool(flags & 2))
        torch.cuda.synchronize()
        return tau, gr, gfe

    tau0, g0, _ = run(None)
    scale = np.abs(e["tau"]).max()
    held(f"RNEA n={n} torques", tau0.cpu().numpy() / scale, e["tau"][:n] / scale, e["g"]["tau"])
    for k, got, want in zip(("q", "qd", "qdd"), g0, e["rnea_vjp"]):
        scale = np.abs(want).max()
        held(f"RNEA n={n} VJP d/d{k}", got.cpu().numpy() / scale, want[:n] / scale, e["g"][f"rnea_grad_{k}"])
    # the scratch launches (flags 0, 1, 2) against the staged ones, as test_rnea_scratch_launches_equal_the_staged_ones demands
    scratch = torch.full((3 * n * D,), float("nan"), device=device)
    tau1, g1, _ = run(scratch, 0)
    torch.testing.assert_close(tau0, tau1, rtol=1e-5, atol=1e-5 * float(tau0.abs().max()))
    for a, b in zip(g0, g1):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5 * float(a.abs().max()))
    _, g2, _ = run(scratch, 1)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    _, g3, _ = run(scratch, 1 | 2, fill=0.5)
    for a, b in zip(g1, g3):
        torch.testing.assert_close(b, a + 0.5, rtol=1e-6, atol=1e-6 * float(a.abs().max()))
    for k, got, want in zip(("q", "qd", "qdd"), g1, e["rnea_vjp"]):
        scale = np.abs(want).max()
        held(f"RNEA n={n} scratch VJP d/d{k}", got.cpu().numpy() / scale, want[:n] / scale, e["g"][f"rnea_grad_{k}"])
    # with an external wrench per link the Lagrangian has nothing to say: the C oracle, at the tolerances of
    # test_gpu_dynamics.py::test_rnea_forward_backward_match_oracle
    fe = z["f_ext"][:n]
    md = m.as_dict()
    tau_ref, cache_ref = oracle.rnea_forward(z["q"][:n], z["qd"][:n], z["qdd"][:n], md, f_ext=fe)
    ref_g = oracle.rnea_backward(z["w_tau"][:n], z["q"][:n], z["qd"][:n], cache_ref, md, want_f_ext_grad=True)
    tau_f, g_f, gfe = run(None, f_ext=t(fe), want_gfe=True)
    assert gap(tau_ref, tau0.cpu().numpy()) > 0.1  # the wrench takes part
    np.testing.assert_allclose(tau_f.cpu().numpy(), tau_ref, rtol=1e-4, atol=1e-5 * max(1.0, np.abs(tau_ref).max()))
    for ours, ref in zip(g_f, ref_g[:3]):
        np.testing.assert_allclose(ours.cpu().numpy(), ref, rtol=1e-3, atol=1e-4 * max(1.0, np.abs(ref).max()))
    np.testing.assert_allclose(gfe.cpu().numpy(), ref_g[3], rtol=1e-4, atol=1e-5 * max(1.0, np.abs(ref_g[3]).max()))


# ------------------------------------------------------------------------------------------------ composed paths
@pytest.mark.parametrize("B", [16, 17])
def test_ik_rollout_fused_equals_the_sequence(B, kp, device, monkeypatch):
    """IKRollout's one-launch form (fused_device.hpp, run-time shapes: D = 6, T = 4) against the kernel sequence on the zoo;
    three goals (one pose per tool frame each), no scene; tolerances of tests/test_gpu_support_polygon.py"""
    from curobo_amd.backends import rollout as rollout_hip
    from curobo_amd.rollout.ik_rollout import IKRollout, IKRolloutCfg
    from conftest import sample_q

    m = Z.model()
    T = kp.num_pose_links
    goal_T = Z.fk64(m, sample_q(m, 3, seed=31, scale=0.8))
    pos, rot = Z.tool_pose64(m, goal_T)
    gp = torch.as_tensor(pos.reshape(3, T, 1, 3).astype(np.float32), device=device)
    gq = torch.as_tensor(Z.matrix_to_quat(rot).reshape(3, T, 1, 4).astype(np.float32), device=device)
    idx = torch.as_tensor(np.arange(B, dtype=np.int32) % 3, device=device)
    q = torch.as_tensor(sample_q(m, B, seed=B, scale=0.9), device=device)
    calls = []
    real = rollout_hip.rollout_ik_fused
    monkeypatch.setattr(rollout_hip, "rollout_ik_fused", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    out = {}
    for fused in (False, True):
        ro = IKRollout(kp, None, B, IKRolloutCfg(use_fused=fused))
        ro.update_goals(gp, gq, idx)
        if fused:  # a fused launch that refuses the zoo would be a finding, not a reason to skip
            assert ro.fused_available(), "the fused IK launch refuses the joint zoo"
        out[fused] = [t.clone().cpu().numpy() for t in ro.cost_and_gradient(q)]
        assert len(calls) == int(fused), "the fused launch was not the one taken"
    (c0, g0), (c1, g1) = out[False], out[True]
    print(f"[joint zoo] IKRollout B={B}: cost {c0.min():.3g}..{c0.max():.3g}, fused - sequence {np.abs(c1 - c0).max():.2e}; "
          f"|grad| max {np.abs(g0).max():.3g}, fused - sequence {np.abs(g1 - g0).max():.2e}")
    assert c0.min() > 0 and np.abs(g0).max(0).min() > 0  # every dof takes part
    np.testing.assert_allclose(c1, c0, rtol=1e-4, atol=1e-2)
    np.testing.assert_allclose(g1, g0, rtol=2e-3, atol=2e-5 * np.abs(g0).max())


def test_collision_rollout_fused_equals_the_sequence(kp, device, monkeypatch):
    """CollisionRollout's fused launch against the kernel sequence on the zoo, one cuboid that the arm reaches; the comparison
    and tolerances of tests/test_gpu_fused.py"""
    from curobo_amd.backends import rollout as rollout_hip
    from curobo_amd.rollout import CollisionRollout, CollisionRolloutCfg
    from curobo_amd.scene import SceneData, cuboid_scene_arrays
    from curobo_amd.workloads import seed_knots, start_configuration
    from test_gpu_fused import _compare

    m = Z.model()
    seeds, n_knots = 9, 12
    knots = seed_knots(m, seeds, n_knots, seed=11)
    start = start_configuration(m)
    # a cuboid around where the tool frame l5 is halfway along the first seed
    centre = Z.tool_pose64(m, Z.fk64(m, knots[0, n_knots // 2][None]))[0][0, 0]
    world = [[{"dims": [0.3, 0.3, 0.3], "pose": [float(centre[0]), float(centre[1]), float(centre[2]), 1, 0, 0, 0]}]]
    scene = SceneData.from_arrays(cuboid_scene_arrays(world), device)
    calls = []
    real = rollout_hip.rollout_trajectory_fused
    monkeypatch.setattr(rollout_hip, "rollout_trajectory_fused", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ros = []
    for fused in (False, True):
        ro = CollisionRollout(kp, scene, seeds, CollisionRolloutCfg(use_fused=fused, fused_materialize=True, n_knots=n_knots))
        ro.update_start_state(torch.as_tensor(start, device=device))
        ros.append(ro)
    assert ros[1].fused_available(), "the fused rollout launch refuses the joint zoo"
    c0, g0, c1, g1 = _compare(ros[0], ros[1], knots, device)
    assert len(calls) == 1, "the fused launch was not the one taken"
    print(f"[joint zoo] CollisionRollout: cost max {c0.max():.3g}, fused - sequence {np.abs(c1 - c0).max():.2e}; "
          f"|grad| max {np.abs(g0).max():.3g}, fused - sequence {np.abs(g1 - g0).max():.2e}")
    assert c0.max() > 0
    # the spheres of the fused launch against float64: its point FK is fused_device.hpp's, not kinematics.hip's
    pos = ros[1].position.cpu().numpy().reshape(-1, m.num_dof)
    held("fused rollout spheres", ros[1].robot_spheres.cpu().numpy().reshape(len(pos), -1, 4)[..., :3],
         Z.spheres64(m, Z.fk64(m, pos))[..., :3], Z.expected()["g"]["spheres"])
    np.testing.assert_allclose(c1, c0, rtol=2e-5, atol=1e-3)
    np.testing.assert_allclose(g1, g0, rtol=1e-3, atol=2e-5 * np.abs(g0).max())
