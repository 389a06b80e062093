"""CPU: the seed-IK restatement converges on reachable goals, and the Halton seed buffer is the
reference's (scipy scrambled Halton, same seed -> same points; checked against the reference's own
HaltonSequencer when the checkout is present)."""

import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_model


def test_seed_ik_restatement_converges(oracle):
    from oracle import seed_ik_ref as R

    md = load_model("franka").as_dict()
    rng = np.random.default_rng(0)
    lo, hi = np.asarray(md["joint_limits_position"], np.float32)
    P, S = 20, 8
    qg = (lo + (hi - lo) * rng.random((P, 7))).astype(np.float32)
    fk = oracle.kinematics_forward(qg, md, compute_spheres=False)
    seeds = (lo + (hi - lo) * rng.random((P * S, 7))).astype(np.float32)
    idx = np.repeat(np.arange(P, dtype=np.int32), S)
    st = R.solve(oracle, md, R.SeedIKRefCfg(), seeds, fk["link_pos"].reshape(P, 1, 1, 3), fk["link_quat"].reshape(P, 1, 1, 4), idx)
    ok = st["final_success"].reshape(P, S)
    assert ok.any(1).mean() >= 0.85
    # what is flagged solved is solved: FK of the solution is at the goal
    sol = st["joint_position"][st["final_success"]]
    goal = np.repeat(fk["link_pos"][:, 0], S, axis=0)[st["final_success"]]
    err = np.linalg.norm(oracle.kinematics_forward(sol, md, compute_spheres=False)["link_pos"][:, 0] - goal, axis=-1)
    assert (err < 0.005 + 1e-6).all()
    # the trust-region logic moved lambda both ways
    assert st["lambda_damping"].min() < 0.2 < st["lambda_damping"].max()


def test_joint_limit_block_matches_reference_golden():
    """oracle.seed_ik_ref.joint_limit_block == the reference's own _compute_joint_limit_errors
    (tests/golden/make_seed_ik_limits_golden.py), plain and with velocity-clamped bounds"""
    from conftest import GOLDEN_DIR
    from oracle import seed_ik_ref as R

    g = np.load(os.path.join(GOLDEN_DIR, "seed_ik_limits_golden.npz"))
    for name, kw in (("plain", {}), ("clamped", dict(current_position=g["current_position"], dt=g["dt"],
                                                      velocity_limits=g["velocity_limits"]))):
        jte, diag, err = R.joint_limit_block(g["q"], g["lo"], g["hi"], float(g["weight"]), **kw)
        np.testing.assert_array_equal(jte, g[f"{name}/jTerror"])
        np.testing.assert_array_equal(diag, np.diagonal(g[f"{name}/jacobian"], axis1=-2, axis2=-1))
        np.testing.assert_allclose(err, g[f"{name}/error"], rtol=1e-6)
    assert (g["clamped/jTerror"] != g["plain/jTerror"]).any()


def test_halton_seed_buffer_is_scipys_scrambled_halton():
    from scipy.stats.qmc import Halton

    from curobo_amd.solver.seed_ik import HaltonSeeds

    lo, hi = torch.tensor([-1.0, 0.0, 2.0]), torch.tensor([1.0, 0.5, 4.0])
    s = HaltonSeeds(3, lo, hi, seed=451)
    np.testing.assert_allclose(s.buffer.numpy(), Halton(d=3, seed=451, scramble=True).random(2000).astype(np.float32))
    a = s.get_samples(64)
    assert a.shape == (64, 3) and bool(((a >= lo) & (a <= hi)).all())
    s.reset()
    assert torch.equal(a, s.get_samples(64))
    ref_root = "/root/reference"
    if os.path.isdir(ref_root):
        sys.path.insert(0, ref_root)
        try:
            from curobo._src.util.sampling.sequencer_halton import HaltonSequencer
        except Exception as e:  # optional dependency of the reference missing
            pytest.skip(f"reference sampler not importable: {e}")
        finally:
            sys.path.remove(ref_root)
        np.testing.assert_allclose(s.buffer.numpy(), HaltonSequencer(ndims=3, seed=451).random(2000).astype(np.float32))


def _golden():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "seed_ik_update_golden.npz"))
    pick = lambda pre: {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith(pre + "/")}  # noqa: E731
    return g, pick("cfg"), pick("cur"), pick("cand"), pick("out")


def test_state_update_restatement_matches_reference_golden():
    """oracle/seed_ik_ref.update_state against the outputs of the reference's own
    SeedIterationStateManager.update_iteration_state (tests/golden/make_seed_ik_golden.py)"""
    from oracle import seed_ik_ref as R

    g, c, cur, cand, out = _golden()
    cfg = R.SeedIKRefCfg(rho_min=float(c["rho_min"]), lambda_factor=float(c["lambda_factor"]), lambda_min=float(c["lambda_min"]),
                         lambda_max=float(c["lambda_max"]), convergence_position_tolerance=float(c["convergence_position_tolerance"]),
                         convergence_orientation_tolerance=float(c["convergence_orientation_tolerance"]),
                         convergence_joint_limit_weight=float(c["convergence_joint_limit_weight"]))
    got = R.update_state(cur, cand, g["pred"], g["lo"], g["hi"], cfg)
    assert np.array_equal(got["improvement"], out["improvement"]) and np.array_equal(got["success"], out["success"])
    for k in ("joint_position", "jacobian", "jTerror", "error_norm", "position_errors", "orientation_errors"):
        np.testing.assert_array_equal(got[k], out[k], err_msg=k)
    np.testing.assert_allclose(got["lambda_damping"], out["lambda_damping"], rtol=1e-6)
    assert 0 < out["improvement"].sum() < len(out["improvement"]) and out["success"].any()


# ------------------------------------------------------------------------------------------------ fused-launch test inputs
def test_locked_joint_variant_is_the_original_with_those_joints_at_zero(oracle):
    """tests/seed_ik_variants.with_locked_joints: oracle FK of the variant == oracle FK of the original with the locked
    joints at 0, bit for bit, on every link and on the Jacobian columns of the joints that are left"""
    import seed_ik_variants as V

    for name, locked in (("franka", (4, 6)), ("ur10e", (0, 3)), ("dual_ur10e", (7,))):
        full = V.packaged(name)
        var = V.with_locked_joints(full, locked)
        keep = [j for j in range(full.num_dof) if j not in locked]
        assert var.num_dof == len(keep) and var.joint_names == [full.joint_names[j] for j in keep]
        assert all(len(v) == len(keep) for v in var.cspace.values()) and var.joint_limits_position.shape == (2, len(keep))
        assert sorted(x for x in var.joint_map.tolist() if x >= 0) == list(range(len(keep)))
        rng = np.random.default_rng(1)
        lo, hi = np.asarray(var.joint_limits_position, np.float32)
        qv = (lo + (hi - lo) * rng.random((33, len(keep)))).astype(np.float32)
        qf = np.zeros((33, full.num_dof), np.float32)
        qf[:, keep] = qv
        a = oracle.kinematics_forward(qv, var.as_dict(), compute_jacobian=True, compute_spheres=False)
        b = oracle.kinematics_forward(qf, full.as_dict(), compute_jacobian=True, compute_spheres=False)
        np.testing.assert_array_equal(a["cumul_mat"], b["cumul_mat"])
        np.testing.assert_array_equal(a["link_pos"], b["link_pos"])
        np.testing.assert_array_equal(a["link_quat"], b["link_quat"])
        np.testing.assert_array_equal(a["jacobian"], b["jacobian"][..., keep])


def test_extra_tool_frames_are_the_links_own_poses(oracle):
    """tests/seed_ik_variants.with_tool_frames: the poses of the extra frames are the original's ``cumul_mat`` rows, frame 0
    keeps its Jacobian, joints behind a frame's link have zero columns, and the extra frames' linear Jacobian is the
    derivative of their position (central differences)"""
    import seed_ik_variants as V

    for case in ("C", "D"):
        name, extra = V.CASES[case][0], V.CASES[case][1]
        full, var = V.packaged(name), V.case_model(case)
        assert var.tool_frames[1:] == [full.link_names[i] for i in extra]
        D, T = var.num_dof, len(var.tool_frame_map)
        q = sample_q_local(full, 29)
        a = oracle.kinematics_forward(q, var.as_dict(), compute_jacobian=True, compute_spheres=False)
        b = oracle.kinematics_forward(q, full.as_dict(), compute_jacobian=True, compute_spheres=False)
        np.testing.assert_array_equal(a["cumul_mat"], b["cumul_mat"])
        np.testing.assert_array_equal(a["link_pos"][:, 0], b["link_pos"][:, 0])
        np.testing.assert_array_equal(a["jacobian"][:, 0], b["jacobian"][:, 0])
        affects = var.joint_affects_endeffector.reshape(D, T)
        assert affects[:, 0].all() and not affects[:, 1:].all()
        for t, link in enumerate(extra, start=1):
            C = b["cumul_mat"][:, link]
            np.testing.assert_array_equal(a["link_pos"][:, t], C[:, :, 3])
            w, x, y, z = (a["link_quat"][:, t, i].astype(np.float64) for i in range(4))
            R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                          2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                          2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
            np.testing.assert_allclose(R, C[:, :, :3], atol=2e-6)
            assert (a["jacobian"][:, t][..., ~affects[:, t]] == 0).all()
            h = 1e-2
            for j in range(D):
                dq = np.zeros(D, np.float32)
                dq[j] = h
                fd = (oracle.kinematics_forward(q + dq, var.as_dict(), compute_spheres=False)["link_pos"][:, t].astype(np.float64)
                      - oracle.kinematics_forward(q - dq, var.as_dict(), compute_spheres=False)["link_pos"][:, t]) / (2 * h)
                np.testing.assert_allclose(a["jacobian"][:, t, :3, j], fd, atol=2e-4)  # (h^2 / 6 |p'''| <= 1.7e-5 |p|)


def sample_q_local(model, n, seed=6):
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(model.joint_limits_position, np.float32)
    return (lo + (hi - lo) * rng.random((n, lo.shape[0]))).astype(np.float32)


def test_variants_validate_and_fit_the_fused_launch_as_tabled():
    import seed_ik_variants as V
    from curobo_amd.robot.kinematics_params import KinematicsParams

    for case, (_, _, _, D, T, _) in V.CASES.items():
        m = V.case_model(case)
        kin = KinematicsParams.from_model(m, torch.device("cpu"))
        kin.validate_shapes()
        assert (kin.num_dof, kin.num_pose_links) == (D, T)
        assert V.fused_fits(m), case
    assert not V.fused_fits(V.packaged("dual_ur10e"))
    assert not V.fused_fits(V.packaged("unitree_g1"))


def test_velocity_acceleration_block_matches_reference_golden():
    """oracle.seed_ik_ref.velocity_acceleration_block == the reference's own _compute_velocity_errors /
    _compute_acceleration_errors (tests/golden/make_seed_ik_velacc_golden.py), at the bounds the HIP state-update kernel is
    held to in tests/test_gpu_seed_ik.py::test_velocity_and_acceleration_residual_rows"""
    from conftest import GOLDEN_DIR
    from oracle import seed_ik_ref as R

    g = np.load(os.path.join(GOLDEN_DIR, "seed_ik_velacc_golden.npz"))
    for wv, wa in ((float(g["velocity_weight"]), 0.0), (0.0, float(g["acceleration_weight"])),
                   (float(g["velocity_weight"]), float(g["acceleration_weight"]))):
        jt, d2, err = R.velocity_acceleration_block(g["q"], g["current_position"], g["current_velocity"], g["dt"], wv, wa)
        want_jt = (g["vel_jTerror"] if wv > 0 else 0) + (g["acc_jTerror"] if wa > 0 else 0)
        want_en = (g["vel_error"] if wv > 0 else 0) + (g["acc_error"] if wa > 0 else 0)
        want_d2 = (g["vel_jacobian_diag"] ** 2 if wv > 0 else 0) + (g["acc_jacobian_diag"] ** 2 if wa > 0 else 0)
        np.testing.assert_allclose(jt, want_jt, rtol=2e-5, atol=1e-5 * np.abs(want_jt).max())
        np.testing.assert_allclose(err, want_en, rtol=2e-5)
        np.testing.assert_allclose(d2, want_d2, rtol=5e-5)


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E", "F"])
def test_fused_test_inputs_stay_off_the_knife_edge(oracle, case):
    """conditions on the inputs of tests/test_gpu_seed_ik_fused.py, checked on the oracle alone: at most 2 % of the rows
    come within 1e-3 (1 + |rho|) of the accept threshold (every case, option and iteration count used there), goal sets keep
    at least 95 % of the seeds, and the tabled fp32-versus-float64 sensitivities are what this CPU measures"""
    import seed_ik_variants as V

    runs = [(k, "plain", 0.0, 0.0) for k in (1, 2, 4)]
    if case in ("A", "C"):
        runs += [(2, "goalset", 0.0, 0.0), (2, "goalset_permuted", 0.0, 0.0)]
    if case in ("A", "D"):
        runs += [(2, "clamped", 0.0, 0.0)]
    if case in ("A", "E"):
        runs += [(2, "velacc", wv, wa) for wv, wa in ((0.5, 0.0), (0.0, 0.005), (0.5, 0.005))]
    for k, option, wv, wa in runs:
        ref = V.reference(case, k, option, wv, wa)
        assert V.knife_edge(ref).mean() <= V.KNIFE_CAP, (k, option, wv, wa, V.knife_edge(ref).mean())
        if option.startswith("goalset"):
            assert (ref["goalset_margin"] > V.GOALSET_MARGIN).mean() >= V.GOALSET_KEEP
    for k in (1, 2, 4):
        a, b = V.reference(case, k), V.reference(case, k, lm_float64=True)
        assert np.array_equal(a["accepted"], b["accepted"]) and np.array_equal(a["lambda_damping"], b["lambda_damping"])
        assert np.abs(a["joint_position"] - b["joint_position"]).max() <= {1: 6.0e-6, 2: 1.2e-5, 4: 2.4e-5}[k]
        for key, tabled in zip(("jacobian", "jTerror"), V.MEASURED[case][k]):
            got = V.sensitivity(case, k, key)
            assert 0.9 * tabled <= got <= tabled, (k, key, got, tabled)
