"""CPU restatement of the reference's Levenberg-Marquardt seed-IK iteration (TEST INFRASTRUCTURE:
only tests/ may import this; the product path is curobo_amd/solver/seed_ik.py on the HIP kernels).

Follows, with the oracle's FK / Jacobian / FK-VJP / tool-pose / LM-step restatements as building blocks:
  curobo/_src/solver/seed_ik/seed_ik_error_calculator.py:128-231  error + Jacobian of a configuration
      :233-290  pose block: FK with Jacobian, ToolPoseCost (weights [pw, ow], unit axes weights, zero
                tolerance, use_lie_group=False), J^T e through the FK backward (use_backward=True)
      :292-305  position / orientation error = max over the tool frames, error norm = sum of the cost
      :338-387  joint-limit block (diagonal Jacobian rows)
      :464-495  combination
  curobo/_src/solver/seed_ik/seed_iteration_state_manager.py:74-260  state update
  curobo/_src/solver/seed_ik/seed_ik_solver.py:291-330,384-437     iteration / solve loop
The state update is pinned bit-exactly by the reference's own SeedIterationStateManager run on CPU
(tests/golden/seed_ik_update_golden.npz, tests/golden/make_seed_ik_golden.py), the joint-limit block
(with and without velocity clamping of the bounds) by the reference's own
SeedIKErrorCalculator._compute_joint_limit_errors (tests/golden/seed_ik_limits_golden.npz).  Parity of the other
pieces is pinned where they are defined (oracle/curobo_oracle.c); the LM step is pinned by the reference's own Warp
tile kernel run on the CPU through the stand-in of tests/golden/warp_emulator (tests/golden/lm_warp_golden.npz,
bit-equal) and against numpy.linalg.solve in tests/test_oracle_linalg.py.  The velocity / acceleration residual blocks
(seed_ik_error_calculator.py:389-456) are pinned by the reference's own _compute_velocity_errors / _compute_acceleration_errors
(tests/golden/seed_ik_velacc_golden.npz).
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict

import numpy as np


@dataclass
class SeedIKRefCfg:  # names and defaults: solver/seed_ik/seed_ik_solver_cfg.py:25-94
    max_iterations: int = 16
    inner_iterations: int = 4
    position_tolerance: float = 0.005
    orientation_tolerance: float = 0.05
    convergence_position_tolerance: float = 0.00001
    convergence_orientation_tolerance: float = 0.00001
    convergence_joint_limit_weight: float = 1.0
    lambda_initial: float = 0.2
    lambda_factor: float = 2.0
    lambda_max: float = 1.0e10
    lambda_min: float = 1e-5
    joint_limit_margin: float = 0.001
    joint_limit_weight: float = 1.0
    rho_min: float = 1e-3
    position_weight: float = 1.0
    orientation_weight: float = 1.0


def action_bounds(model: Dict[str, np.ndarray], cfg: SeedIKRefCfg):
    lo, hi = np.asarray(model["joint_limits_position"], np.float32)
    margin = (hi - lo) * np.float32(cfg.joint_limit_margin)
    return (lo + margin).astype(np.float32), (hi - margin).astype(np.float32)


def joint_limit_block(q, lo, hi, weight, current_position=None, dt=None, velocity_limits=None):
    """seed_ik_error_calculator.py:338-387: (J^T e contribution [n, D], Jacobian diagonal [n, D], summed
    error [n]).  With ``current_position`` [n, D], ``dt`` [n] and ``velocity_limits`` [2, D] (lower row
    negative) the bounds are tightened to what one step of ``dt`` can reach (:355-363)."""
    q = np.asarray(q, np.float32)
    lo = np.broadcast_to(np.asarray(lo, np.float32), q.shape)
    hi = np.broadcast_to(np.asarray(hi, np.float32), q.shape)
    if current_position is not None and dt is not None:
        v = np.asarray(velocity_limits, np.float32)
        dtc = np.asarray(dt, np.float32).reshape(-1, 1)
        cp = np.asarray(current_position, np.float32)
        lo = np.maximum(lo, cp + v[0] * dtc)
        hi = np.minimum(hi, cp + v[1] * dtc)
    uv, lv = np.maximum(q - hi, np.float32(0)), np.maximum(lo - q, np.float32(0))
    w = np.float32(weight)
    err = w * (lv + uv)
    diag = w * (np.where(lv > 0, -1.0, 0.0) + np.where(uv > 0, 1.0, 0.0)).astype(np.float32)
    return (diag * err).astype(np.float32), diag, err.sum(-1).astype(np.float32)


def velocity_acceleration_block(q, current_position, current_velocity, dt, velocity_weight, acceleration_weight):
    """seed_ik_error_calculator.py:389-456: (J^T r contribution [n, D], squared Jacobian diagonal [n, D], summed squared
    error [n]) of the velocity rows r_v = sqrt(w_v dt) v and the acceleration rows r_a = sqrt(w_a) (v - current_velocity),
    v = (q - current_position) / dt.  A block whose weight is 0 contributes nothing (the reference leaves it out)."""
    q = np.asarray(q, np.float32)
    cp = np.asarray(current_position, np.float32)
    dtc = np.maximum(np.asarray(dt, np.float32).reshape(-1, 1), np.float32(1e-10))
    inv_dt = (np.float32(1.0) / dtc).astype(np.float32)
    v = ((q - cp) * inv_dt).astype(np.float32)
    jtr, d2, err = np.zeros_like(q), np.zeros_like(q), np.zeros(q.shape[0], np.float32)
    if velocity_weight > 0:
        sw = np.sqrt(np.float32(velocity_weight) * dtc).astype(np.float32)
        e, jd = sw * v, np.broadcast_to(sw * inv_dt, q.shape)
        jtr, d2, err = jtr + jd * e, d2 + jd * jd, err + (e * e).sum(-1)
    if acceleration_weight > 0:
        sw = np.sqrt(np.float32(acceleration_weight))
        e, jd = sw * (v - np.asarray(current_velocity, np.float32)), np.broadcast_to(sw * inv_dt, q.shape)
        jtr, d2, err = jtr + jd * e, d2 + jd * jd, err + (e * e).sum(-1)
    return jtr.astype(np.float32), d2.astype(np.float32), err.astype(np.float32)


def evaluate(orc, model, cfg: SeedIKRefCfg, q, goal_position, goal_quat, idxs_goal, current_position=None, dt=None,
             current_velocity=None, velocity_weight=0.0, acceleration_weight=0.0):
    """error + Jacobian of configurations q[n, D] against goals [P, T, G, 3|4] (seed_ik_error_calculator.py:128-231);
    ``current_position`` / ``dt``: velocity clamping of the joint-limit bounds with the model's velocity limits, and, with
    ``velocity_weight`` / ``acceleration_weight`` (``current_velocity`` for the latter), the velocity / acceleration residual
    rows: diagonal like the joint-limit rows, so the three rows of a dof are stated as ONE of magnitude sqrt(diag^2 + d2)
    (same J^T J, same J^T r).  ``goalset_idx`` [n, T] is the goal-set member each frame is pulled to, ``goalset_margin`` [n]
    the smallest relative gap, over the frames, between the costs of the two best members (inf for one member)."""
    q = np.ascontiguousarray(q, np.float32)
    n, D = q.shape
    T = model["tool_frame_map"].shape[0]
    fk = orc.kinematics_forward(q, model, compute_jacobian=True, compute_spheres=False)
    one6 = np.ones(6, np.float32)

    def pose(gp, gq):
        return orc.tool_pose_distance(
            fk["link_pos"].reshape(n, 1, T, 3), fk["link_quat"].reshape(n, 1, T, 4), gp, gq, idxs_goal,
            np.array([cfg.position_weight, cfg.orientation_weight], np.float32), np.tile(one6, T), np.tile(one6, T),
            np.zeros(2 * T, np.float32), np.zeros(2 * T, np.float32), np.zeros(T, np.uint8), 0)

    tp = pose(goal_position, goal_quat)
    G = np.asarray(goal_position).shape[-2]
    margin = np.full(n, np.inf, np.float32)
    if G > 1:
        gp_all, gq_all = np.asarray(goal_position, np.float32), np.asarray(goal_quat, np.float32)
        member = np.stack([pose(np.ascontiguousarray(gp_all[:, :, g:g + 1]), np.ascontiguousarray(gq_all[:, :, g:g + 1]))
                           ["distance"].reshape(n, T, 2).sum(-1) for g in range(G)], -1)  # [n, T, G] cost per member
        two = np.sort(member, -1)[..., :2]
        margin = ((two[..., 1] - two[..., 0]) / np.maximum(two[..., 1], np.float32(1e-30))).min(-1).astype(np.float32)
    pose_jte = orc.kinematics_backward(model, fk["cumul_mat"], None, tp["position_gradient"].reshape(n, T, 3),
                                       tp["rotation_gradient"].reshape(n, T, 4))
    lo, hi = action_bounds(model, cfg)
    jl_jte, diag, jl_sum = joint_limit_block(q, lo, hi, cfg.joint_limit_weight, current_position, dt,
                                             model.get("joint_limits_velocity"))
    jte, err = (pose_jte + jl_jte).astype(np.float32), (tp["distance"].reshape(n, -1).sum(-1) + jl_sum).astype(np.float32)
    if current_position is not None and dt is not None and (velocity_weight > 0 or acceleration_weight > 0):
        va_jte, d2, va_sum = velocity_acceleration_block(q, current_position, current_velocity, dt, velocity_weight,
                                                         acceleration_weight)
        jte, err = (jte + va_jte).astype(np.float32), (err + va_sum).astype(np.float32)
        diag = np.where(d2 > 0, np.sqrt(diag * diag + d2), diag).astype(np.float32)
    J = np.zeros((n, 6 * T + D, D), np.float32)
    J[:, : 6 * T] = fk["jacobian"].reshape(n, 6 * T, D)
    J[:, 6 * T + np.arange(D), np.arange(D)] = diag
    return {
        "joint_position": q,
        "jacobian": J,
        "jTerror": jte,
        "error_norm": err,
        "position_errors": tp["position_distance"].reshape(n, T).max(-1),
        "orientation_errors": tp["rotation_distance"].reshape(n, T).max(-1),
        "pose_jacobian": fk["jacobian"].reshape(n, 6 * T, D), "pose_jTerror": pose_jte,
        "pose_cost": tp["distance"].reshape(n, T, 2) if tp["distance"].shape[-1] == 2 * T else tp["distance"],
        "position_distance": tp["position_distance"].reshape(n, T), "rotation_distance": tp["rotation_distance"].reshape(n, T),
        "goalset_idx": tp["goalset_idx"].reshape(n, T), "goalset_margin": margin,
    }


def update_state(cur, cand, pred_reduction, lo, hi, cfg: SeedIKRefCfg):
    """seed_iteration_state_manager.py:74-260 (cur carries lambda_damping)"""
    rho = (cur["error_norm"] - cand["error_norm"]) / (pred_reduction + np.float32(1e-8))
    acc = rho >= cfg.rho_min
    lam = np.where(acc, cur["lambda_damping"] / cfg.lambda_factor, cur["lambda_damping"] * cfg.lambda_factor)
    lam = np.clip(lam, cfg.lambda_min, cfg.lambda_max).astype(np.float32)
    sel = {k: np.where(acc.reshape((-1,) + (1,) * (cand[k].ndim - 1)), cand[k], cur[k])
           for k in ("joint_position", "jTerror", "jacobian", "position_errors", "orientation_errors")}
    return {**sel, "lambda_damping": lam, "error_norm": cand["error_norm"], "success": converged(sel, lo, hi, cfg),
            "improvement": acc, "rho": rho}


def converged(st, lo, hi, cfg: SeedIKRefCfg):
    """seed_iteration_state_manager.py:222-260: the convergence flag of a (selected) state; every comparison is strict"""
    ok = (st["position_errors"] < cfg.convergence_position_tolerance) & (
        st["orientation_errors"] < cfg.convergence_orientation_tolerance)
    if cfg.convergence_joint_limit_weight > 0:
        ok &= np.all((st["joint_position"] > lo) & (st["joint_position"] < hi), axis=-1)
    return ok


def lm_step_float64(jacobian, jTerror, lambda_damping, joint_position):
    """the LM step (levenberg_marquardt_step.py:146-199) with the normal equations formed and solved in float64: what the
    fp32 step is measured against (``iterate(..., lm_float64=True)``)"""
    J, g = np.asarray(jacobian, np.float64), np.asarray(jTerror, np.float64)
    lam = np.asarray(lambda_damping, np.float64)
    A = np.einsum("nrd,nre->nde", J, J) + lam[:, None, None] * np.eye(J.shape[-1])
    delta = np.linalg.solve(A, -g[..., None])[..., 0]
    pred = 0.5 * (delta * (lam[:, None] * delta - g)).sum(-1)
    return (np.asarray(joint_position, np.float64) + delta).astype(np.float32), pred.astype(np.float32)


def iterate(orc, model, cfg: SeedIKRefCfg, seeds, goal_position, goal_quat, idxs_goal, iterations, lm_float64=False, **extra):
    """the initial evaluation of ``seeds`` and ``iterations`` LM iterations (seed_ik_solver.py:291-330); ``extra``: the
    clamping / residual-row arguments of :func:`evaluate`.  The state carries, per iteration, the trust ratio (``rho``
    [iterations, n]) and accept decision (``accepted``), and the smallest goal-set margin of any evaluation."""
    lo, hi = action_bounds(model, cfg)
    st = evaluate(orc, model, cfg, seeds, goal_position, goal_quat, idxs_goal, **extra)
    n = st["joint_position"].shape[0]
    st["lambda_damping"] = np.full(n, cfg.lambda_initial, np.float32)
    st["success"] = converged(st, lo, hi, cfg)
    st["improvement"] = np.ones(n, bool)
    rho, acc, margin, member = [], [], st["goalset_margin"], st["goalset_idx"]
    for _ in range(iterations):
        step = lm_step_float64 if lm_float64 else orc.lm_step
        q_new, pred = step(st["jacobian"], st["jTerror"], st["lambda_damping"], st["joint_position"])
        cand = evaluate(orc, model, cfg, q_new, goal_position, goal_quat, idxs_goal, **extra)
        margin = np.minimum(margin, cand["goalset_margin"])
        st = update_state(st, cand, pred, lo, hi, cfg)
        rho.append(st["rho"])
        acc.append(st["improvement"])
    st["rho"], st["accepted"] = np.array(rho, np.float32).reshape(iterations, n), np.array(acc, bool).reshape(iterations, n)
    st["goalset_margin"], st["goalset_idx"] = margin, member  # (the members of the initial evaluation)
    return st


def solve(orc, model, cfg: SeedIKRefCfg, seeds, goal_position, goal_quat, idxs_goal, **extra):
    """all iterations, no early exit (seed_ik_solver.py:384-437 with batch_success_threshold never met)"""
    st = iterate(orc, model, cfg, seeds, goal_position, goal_quat, idxs_goal, cfg.max_iterations, **extra)
    ok = (st["position_errors"] < cfg.position_tolerance) & (st["orientation_errors"] < cfg.orientation_tolerance)
    lim_lo, lim_hi = np.asarray(model["joint_limits_position"], np.float32)
    ok &= np.all((st["joint_position"] > lim_lo) & (st["joint_position"] < lim_hi), axis=-1)
    st["final_success"] = ok
    return st
