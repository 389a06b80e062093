"""The joint-zoo robot (tests/joint_zoo.py) on the CPU: its tables, the float64 restatements against the C oracle, the steps of
their finite differences, and the reference's own kernels (where oracle/_ref is built) against the restatements -- with the
two quantities that the reference gets WRONG on this robot stated as tests, so that a later reader learns that the differences
are known and on whose side they lie:

  * dJ/dq (``kinematics_backward_kernel<..., COMPUTE_JACOBIAN_GRAD>``) on every tool frame whose chain passes a mimic link;
  * the RNEA torques wherever a prismatic joint moves in a rotating parent frame: ``motion_cross_S`` writes the Coriolis
    acceleration ``omega x axis * qd`` of a prismatic joint into the angular rows of the spatial acceleration, not the linear
    ones.  The packaged robots have prismatic joints on the floating base only (omega = 0 there), so they never show it.

Bounds: ``g`` (joint_zoo.expected) is the reference's own fp32 gap to float64 per quantity, pooled over the golden's 65 points;
the fp32 C oracle is held to 4 g like the HIP kernels (tests/test_gpu_joint_zoo.py; 4: another summation order and FMA
contraction, docs/ORACLE_PINS.md)."""

import numpy as np
import pytest

import joint_zoo as Z
from joint_zoo import gap, held
from oracle import ref_kernels

needs_ref = pytest.mark.skipif(not ref_kernels.available(), reason="oracle/_ref/libcurobo_ref.so not built")


# ------------------------------------------------------------------------------------------------ tables
def test_tables_hold_what_the_packaged_robots_lack():
    m = Z.model()  # (asserts the properties itself)
    assert m.link_names == ["base", "l1", "l2", "l3", "l3f", "l4", "l5", "l6", "fa", "fb"]
    assert m.joint_map_type.tolist() == [-1, 5, 0, 4, -1, 2, 3, 5, 1, 1]
    assert m.joint_map.tolist() == [-1, 0, 1, 2, -1, 3, 4, 0, 5, 5]
    off = m.joint_offset_map.reshape(-1, 2)
    np.testing.assert_array_equal(off[:, 0], np.array([1, 1, 1, -1, 1, -1, 1, 0.5, 1, -1.5], np.float32))
    np.testing.assert_array_equal(off[:, 1], np.array([0, 0, 0, 0, 0, 0, 0, 0.3, 0, 0.01], np.float32))
    assert m.num_dof == 6 and m.joint_links_offsets.tolist() == [0, 2, 3, 4, 5, 6, 8]
    assert m.tool_frames == ["l5", "l6", "fa", "fb"] and m.link_map.tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7, 7]
    assert Z.mimic_free_frames(m) == [0]
    assert Z.revolute_dofs(m).tolist() == [1, 0, 1, 0, 1, 0]
    assert m.link_masses_com[4, 3] == np.float32(0.01)  # l3f: the loader's default mass
    assert np.abs(m.fixed_transforms[1:, :, :3] - np.eye(3)).reshape(9, -1).max(1).min() > 0.01  # every joint origin is rotated


def test_golden_inputs_are_the_generators():
    z, want = Z.golden(), Z.make_inputs()
    for k, v in want.items():
        np.testing.assert_array_equal(z[k], v, err_msg=k)
    lo, hi = Z.model().joint_limits_position
    assert ((z["q"] >= lo) & (z["q"] <= hi)).all() and z["q"].shape == (Z.N, 6)
    np.testing.assert_array_equal(z["qd_revolute_only"], z["qd"] * Z.revolute_dofs(Z.model()))
    # the float64 quaternion's sign (w >= 0) is the kernels' on every point: no tool frame is near w = 0
    assert np.abs(Z.matrix_to_quat(Z.expected()["rot"])[..., 0]).min() > 1e-3


# ------------------------------------------------------------------------------------------------ the C oracle
def test_oracle_forward(oracle):
    m, z, e = Z.model(), Z.golden(), Z.expected()
    f = oracle.kinematics_forward(z["q"], m.as_dict(), compute_jacobian=True, compute_com=True)
    g = e["g"]
    held("oracle transforms", f["cumul_mat"], e["T"][:, :, :3], g["cumul"])
    held("oracle tool positions", f["link_pos"], e["pos"], g["pos"])
    held("oracle tool rotations", Z.quat_to_matrix(f["link_quat"]), e["rot"], g["rot"])
    np.testing.assert_allclose(np.linalg.norm(f["link_quat"], axis=-1), 1.0, atol=4e-7)
    held("oracle spheres", f["robot_spheres"], e["spheres"], g["spheres"])
    np.testing.assert_array_equal(f["robot_spheres"][..., 3], np.broadcast_to(m.link_spheres[0, :, 3], (Z.N, 18)))
    held("oracle centre of mass", f["com"], e["com"], g["com"])
    held("oracle Jacobian", f["jacobian"], e["jacobian"], g["jacobian"])


def test_oracle_backward(oracle):
    m, z, e = Z.model(), Z.golden(), Z.expected()
    md = m.as_dict()
    f = oracle.kinematics_forward(z["q"], md, compute_com=True)
    got = oracle.kinematics_backward(md, f["cumul_mat"], z["g_spheres"], z["g_pos"], z["g_quat"], z["g_com"], f["com"])
    held("oracle VJP", got, e["vjp"], e["g"]["vjp"], relative=True)
    scale = np.abs(e["vjp"]).max()
    zero = dict(g_spheres=np.zeros_like(z["g_spheres"]), g_pos=np.zeros_like(z["g_pos"]), g_quat=None, g_com=None)
    for only in ("g_spheres", "g_pos", "g_quat", "g_com"):
        a = dict(zero, **{only: z[only]})
        got = oracle.kinematics_backward(md, f["cumul_mat"], a["g_spheres"], a["g_pos"], a["g_quat"], a["g_com"], f["com"] if only == "g_com" else None)
        want = Z.vjp64(m, z["q"], **{only: z[only]})
        assert np.abs(want).max() > 0.05 * scale, only  # the term takes part
        held(f"oracle VJP, {only} alone", got / scale, want / scale, e["g"]["vjp"])


def test_oracle_rnea(oracle):
    m, z, e = Z.model(), Z.golden(), Z.expected()
    md = m.as_dict()
    tau, cache = oracle.rnea_forward(z["q"], z["qd"], z["qdd"], md)
    held("oracle torques", tau, e["tau"], e["g"]["tau"], relative=True)
    # each term alone, in units of the largest torque: gravity, M qdd, Coriolis
    inertial, coriolis, gravity = Z.tau64(m, z["q"], z["qd"], z["qdd"], parts=True)
    scale, zq = np.abs(e["tau"]).max(), np.zeros_like(z["q"])
    for name, want, (qd, qdd, grav) in (("gravity", gravity, (zq, zq, 9.81)), ("M qdd", inertial, (zq, z["qdd"], 0.0)),
                                        ("Coriolis", coriolis, (z["qd"], zq, 0.0))):
        got, _ = oracle.rnea_forward(z["q"], qd, qdd, md, gravity=(0, 0, 0, 0, 0, grav))
        assert np.abs(want).max() > 0.2 * scale, name
        held(f"oracle torques, {name} alone", got / scale, want / scale, e["g"]["tau"])
    grads = oracle.rnea_backward(z["w_tau"], z["q"], z["qd"], cache, md)
    for k, got, want in zip(("q", "qd", "qdd"), grads, e["rnea_vjp"]):
        held(f"oracle RNEA VJP, d/d{k}", got, want, e["g"][f"rnea_grad_{k}"], relative=True)


def test_inertia_rotation_takes_part():
    """the anisotropic inertias are there so that a wrong inertia rotation shows: with the loader's isotropic default in their
    place the float64 torques move by far more than any tolerance used here"""
    import dataclasses

    m, z, e = Z.model(), Z.golden(), Z.expected()
    iso = m.link_inertias.copy()
    iso[:, :3], iso[:, 3:6] = iso[:, :3].mean(1, keepdims=True), 0.0
    tau = Z.tau64(dataclasses.replace(m, link_inertias=iso), z["q"], z["qd"], z["qdd"])
    assert gap(tau, e["tau"], relative=True) > 1e-3


# ------------------------------------------------------------------------------------------------ finite-difference steps
def test_halving_every_step_moves_nothing():
    """each central difference of the restatements, again with half its step: the result moves by less than a tenth of the
    tolerance (4 g) it is used with"""
    m, z, e = Z.model(), Z.golden(), Z.expected()
    g, q = e["g"], z["q"]
    moved = {
        "vjp": gap(Z.vjp64(m, q, z["g_spheres"], z["g_pos"], z["g_quat"], z["g_com"], h=Z.VJP_H / 2), e["vjp"], True) / g["vjp"],
        "jac_grad": gap(Z.jacobian_grad64(m, q, z["w_jac"], h=Z.JAC_GRAD_H / 2), e["jac_grad"], True) / g["jac_grad"],
        "tau": gap(Z.tau64(m, q, z["qd"], z["qdd"], h=Z.TAU_H / 2), e["tau"], True) / g["tau"],
    }
    outer = Z.rnea_vjp64(m, q, z["qd"], z["qdd"], z["w_tau"], h=Z.RNEA_VJP_H / 2)
    inner = Z.rnea_vjp64(m, q, z["qd"], z["qdd"], z["w_tau"], tau_h=Z.TAU_H / 2)
    for i, k in enumerate(("q", "qd", "qdd")):
        moved[f"rnea_grad_{k}, outer step"] = gap(outer[i], e["rnea_vjp"][i], True) / g[f"rnea_grad_{k}"]
        moved[f"rnea_grad_{k}, inner step"] = gap(inner[i], e["rnea_vjp"][i], True) / g[f"rnea_grad_{k}"]
    print("[joint zoo] halving the step moves the float64 side by (in units of g):", {k: f"{v:.1e}" for k, v in moved.items()})
    for k, v in moved.items():
        assert v < 0.1 * 4, (k, v)


def test_every_arm_of_the_jacobian_gradient_takes_part():
    """d/dq_i of the Jacobian column of dof k, cotangent on that column alone, on the frame ``fa`` (chain: every moving link but fb):
    the pairs (k, i) below single out the four arms of the kernel's dJ/dq (kinematics.hip, "geometric-Jacobian output") and the
    one combination it leaves out because it is zero"""
    m, z = Z.model(), Z.golden()
    per = Z.jacobian_grad_per_column64(m, z["q"][:17], z["w_jac"][:17])  # [D (k), n, D (i)]
    big = np.abs(per).max()
    for name, k, i in Z.JAC_GRAD_ARMS:
        assert np.abs(per[k, :, i]).max() > 0.02 * big, name
    for name, k, i in Z.JAC_GRAD_ZERO:
        assert np.abs(per[k, :, i]).max() < 1e-6 * big, name


# ------------------------------------------------------------------------------------------------ the reference's kernels
@needs_ref
def test_reference_is_the_golden_and_equals_float64_where_it_is_right():
    """the golden is what the reference's kernels return today, and on the forward pass, the Jacobian and the VJP the reference
    equals float64 to fp32 rounding: at most 2e-6 absolute on entries up to 1.5 over a chain of 9 products (about 20 ulp),
    gradients 2e-6 of the largest entry"""
    m, z, e = Z.model(), Z.golden(), Z.expected()
    md, ref = m.as_dict(), ref_kernels.ReferenceKernels()
    f = ref.kinematics_forward(z["q"], md, compute_jacobian=True, compute_com=True)
    for k in ("link_pos", "link_quat", "cumul_mat", "com", "robot_spheres", "jacobian"):
        np.testing.assert_array_equal(f[k], z[f"ref/{k}"], err_msg=k)
    got = ref.kinematics_backward(md, f["cumul_mat"], z["g_spheres"], z["g_pos"], z["g_quat"], z["g_com"], f["com"])
    np.testing.assert_array_equal(got, z["ref/vjp"])
    print("[joint zoo] g:", {k: f"{v:.2e}" for k, v in e["g"].items()})
    for k in ("pos", "rot", "cumul", "spheres", "com", "jacobian", "vjp"):
        assert e["g"][k] < 2e-6, k
    # the pose-only kernel: the same poses
    f0 = ref.kinematics_forward(z["q"], md, compute_spheres=False)
    assert gap(f0["link_pos"], e["pos"]) < 2e-6 and gap(Z.quat_to_matrix(f0["link_quat"]), e["rot"]) < 2e-6


@needs_ref
def test_reference_jacobian_gradient_is_wrong_behind_a_mimic_link():
    m, z, e = Z.model(), Z.golden(), Z.expected()
    md, ref = m.as_dict(), ref_kernels.ReferenceKernels()
    cumul = z["ref/cumul_mat"]
    T, free = len(m.tool_frame_map), Z.mimic_free_frames(m)
    for t in range(T):
        w = np.zeros_like(z["w_jac"])
        w[:, t] = z["w_jac"][:, t]
        got, want = ref.kinematics_backward_jacobian(md, cumul, w), Z.jacobian_grad64(m, z["q"], w)
        err = gap(got, want, relative=True)
        print(f"[joint zoo] reference dJ/dq on frame {m.tool_frames[t]}: off by {err:.2e} of the largest entry {np.abs(want).max():.2f}")
        if t in free:
            assert err < 2e-6
        else:  # known, and the reference's: float64 central differences of the analytic Jacobian say otherwise
            assert err > 0.1
            moving = np.abs(got - want).max(0) > 1e-4 * np.abs(want).max()
            assert not moving[[1, 3]].any()  # the plain prismatic dofs stay exact
    w = np.zeros_like(z["w_jac"])
    w[:, free] = z["w_jac"][:, free]
    np.testing.assert_array_equal(ref.kinematics_backward_jacobian(md, cumul, w), z["ref/jac_grad_mimic_free_frames"])
    assert e["g"]["jac_grad"] < 2e-6


@pytest.mark.skipif(not ref_kernels.rnea_instantiated(10, 6),
                    reason="oracle/_ref/libcurobo_ref.so not built, or built before the 10-link / 6-dof RNEA instantiation and not "
                           "rebuildable here (make -C oracle/cuda_on_cpu rebuilds it wherever the reference's sources are)")
def test_reference_rnea_is_wrong_for_a_prismatic_joint_in_a_rotating_frame():
    m, z, e = Z.model(), Z.golden(), Z.expected()
    md, ref = m.as_dict(), ref_kernels.ReferenceKernels()
    tau, cache = ref.rnea_forward(z["q"], z["qd"], z["qdd"], md)
    np.testing.assert_array_equal(tau, z["ref/tau"])
    err = gap(tau, e["tau"], relative=True)
    print(f"[joint zoo] reference torques: off by {err:.2e} of the largest torque {np.abs(e['tau']).max():.1f}")
    assert err > 0.1  # known, and the reference's: the float64 Lagrangian and the C oracle agree with each other
    # velocity on the revolute dofs only, or on the prismatic dofs only: the misplaced term is omega x axis * qd_prismatic
    rev = Z.revolute_dofs(m)
    for name, mask in (("revolute", rev), ("prismatic", 1 - rev)):
        got, c = ref.rnea_forward(z["q"], z["qd"] * mask, z["qdd"], md)
        want = Z.tau64(m, z["q"], z["qd"] * mask, z["qdd"])
        assert gap(got, want, relative=True) < 2e-6, name
        if name == "revolute":
            np.testing.assert_array_equal(got, z["ref/tau_revolute_velocity_only"])
            for k, gr in zip(("q", "qd", "qdd"), ref.rnea_backward(z["w_tau"], z["q"], z["qd_revolute_only"], c, md)):
                np.testing.assert_array_equal(gr, z[f"ref/rnea_grad_{k}_revolute_velocity_only"])
    for k in ("tau", "rnea_grad_q", "rnea_grad_qd", "rnea_grad_qdd"):
        assert e["g"][k] < 2e-6, k
