"""Golden vectors on the joint-zoo robot of tests/joint_zoo.py, produced by THE REFERENCE'S OWN CUDA KERNELS run on the CPU through
oracle/_ref:

    python tests/golden/make_joint_zoo_golden.py        (from the repository root, after __graft_entry__.build())

Inputs (``joint_zoo.make_inputs``): q [65, 6] inside the joint limits, the cotangents of every kinematics output, qd, qdd, the
torque cotangent and an external wrench per link.  Recorded under ``ref/``: what the reference's kernels return in fp32 on them:
forward with Jacobian and centre of mass, the backward pass, dJ/dq with the cotangent restricted to the tool frames whose chain
holds no mimic link (``ref/jac_grad_mimic_free_frames``: on the others the reference's kernel departs from the derivative of its
own Jacobian, tests/test_oracle_joint_zoo.py), RNEA forward and backward.  The reference's RNEA puts the Coriolis acceleration of a
prismatic joint, omega x axis * qd, into the angular rows of the spatial acceleration instead of the linear ones, so its torques are
wrong wherever a prismatic joint moves in a rotating parent frame (same test module): ``ref/tau`` and ``ref/rnea_grad_*`` keep that
result as it is, and the keys ending in ``_revolute_velocity_only`` hold the same launches with qd zeroed on the prismatic dofs
(``qd_revolute_only``), where the term vanishes and the reference is right.  Arrays only.  Output: tests/golden/joint_zoo.npz.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import joint_zoo as Z  # noqa: E402

from oracle import ref_kernels  # noqa: E402


def main():
    ref = ref_kernels.ReferenceKernels()
    m = Z.model()
    md = m.as_dict()
    out = Z.make_inputs()
    q = out["q"]
    fk = ref.kinematics_forward(q, md, compute_jacobian=True, compute_com=True)
    for k in ("link_pos", "link_quat", "cumul_mat", "com", "robot_spheres", "jacobian"):
        out[f"ref/{k}"] = fk[k]
    out["ref/vjp"] = ref.kinematics_backward(md, fk["cumul_mat"], out["g_spheres"], out["g_pos"], out["g_quat"], out["g_com"], fk["com"])
    w = np.zeros_like(out["w_jac"])
    free = Z.mimic_free_frames(m)
    w[:, free] = out["w_jac"][:, free]
    out["mimic_free_frames"] = np.asarray(free, np.int32)
    out["ref/jac_grad_mimic_free_frames"] = ref.kinematics_backward_jacobian(md, fk["cumul_mat"], w)
    tau, cache = ref.rnea_forward(q, out["qd"], out["qdd"], md)
    out["ref/tau"] = tau
    out["ref/rnea_grad_q"], out["ref/rnea_grad_qd"], out["ref/rnea_grad_qdd"] = ref.rnea_backward(out["w_tau"], q, out["qd"], cache, md)
    qd_r = out["qd"] * Z.revolute_dofs(m)
    out["qd_revolute_only"] = qd_r
    tau, cache = ref.rnea_forward(q, qd_r, out["qdd"], md)
    out["ref/tau_revolute_velocity_only"] = tau
    for k, g in zip(("q", "qd", "qdd"), ref.rnea_backward(out["w_tau"], q, qd_r, cache, md)):
        out[f"ref/rnea_grad_{k}_revolute_velocity_only"] = g
    np.savez_compressed(Z.GOLDEN, **out)
    print(Z.GOLDEN, os.path.getsize(Z.GOLDEN))
    Z.golden.cache_clear(), Z.expected.cache_clear()
    for k, v in Z.expected()["g"].items():
        print(f"g[{k}] = {v:.2e}")


if __name__ == "__main__":
    main()
