"""Records tests/golden/fused_chain_bits.npz: the bits of the fused trajectory launch (csrc/fused_device.hpp) on inputs in which
everything a workgroup reads PER TRAJECTORY differs from row to row -- for tests/test_gpu_fused_chain_bits.py to hold a later
build to:

    python tests/golden/make_fused_chain_bits.py            (needs the GPU; rewrites the fixture)

What the other fixtures keep constant and this one varies: three start-state rows (position, velocity, acceleration, jerk) and two
goal-state rows picked through ``start_idx`` / ``goal_idx`` that are neither sorted nor constant; the two goal rows run at
different dt, one with the implicit goal (boundary knots from the goal state) and one with the explicit one (replicated last
knot).  Those are the values the launch's load chain fetches (indices -> dt, goal mode and state rows; the knots beside them)
and that its B-spline VJP reads again.  Franka, the four-cuboid C2 world, 5 trajectories of 12 knots of degree 3, knots uniform
within the joint limits; padded horizons 17 / 33 / 65 (1, 2 and 4 samples per knot interval) and 37 (a horizon of 36 that is no
multiple of the 16 knot intervals: 2 samples per interval, the points past 32 sit behind the last knot).  Every horizon runs the
collision launch (CollisionRollout) and the TERMS launch (TrajOptRollout: tool pose + c-space STATE), each with the compile-time
shapes on (padded horizon 33 takes the built-in shapes) and off (the generic kernel).

``replay(inputs, memo=...)`` with ``memo`` "even" / "odd" runs the same launches with a reuse memo of stride 1 (every row has a
memo row): the rows of that parity get a memo row with the bits of their knots, the other rows one that differs from theirs in
one word.  The first must come back as the memo's sentinels, the second as evaluated (the recorded bits).

The script refuses to write a file unless (``check``): every case took the fused launch; the index vectors are neither sorted nor
constant and use every state row; some trajectory of every case costs something and all outputs are finite; the two goal modes
and the two dt are both in use; both memo parities behave as described on the recording build; two replays in this process and
one in a fresh process agree word for word."""
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fused_chain_bits.npz")
DEV = "cuda:0"
B, N_KNOTS, DEGREE = 5, 12, 3
HORIZONS = (17, 33, 65, 37)  # padded
START_IDX, GOAL_IDX = (2, 0, 1, 0, 2), (1, 0, 0, 1, 0)
TRAJ_DT, IMPLICIT = (0.05, 0.08), (1, 0)
SENTINEL = 12345.0


def cases():
    """(name, padded horizon, TERMS launch, compile-time shapes enabled)"""
    return [(f"h{H}_{'terms' if terms else 'collision'}_{'shape' if shapes else 'generic'}", H, terms, shapes)
            for H in HORIZONS for terms in (False, True) for shapes in (True, False)]


def inputs():
    from curobo_amd.robot import load_packaged_robot

    model = load_packaged_robot("franka")
    rng = np.random.default_rng(23)
    lo, hi = [np.asarray(v, np.float32) for v in model.joint_limits_position]
    D = model.num_dof
    d = {"knots": (lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(B, N_KNOTS, D))).astype(np.float32)}
    for side, n in (("start", 3), ("goal", 2)):
        d[f"{side}_position"] = (lo + (hi - lo) * rng.uniform(0.2, 0.8, size=(n, D))).astype(np.float32)
        d[f"{side}_velocity"] = rng.uniform(-0.3, 0.3, size=(n, D)).astype(np.float32)
        d[f"{side}_acceleration"] = rng.uniform(-1.0, 1.0, size=(n, D)).astype(np.float32)
        d[f"{side}_jerk"] = rng.uniform(-2.0, 2.0, size=(n, D)).astype(np.float32)
    pos = rng.normal(size=(2, 1, 1, 3)).astype(np.float32) * 0.4
    quat = rng.normal(size=(2, 1, 1, 4)).astype(np.float32)
    d["pose_position"], d["pose_quat"] = pos, (quat / np.linalg.norm(quat, axis=-1, keepdims=True)).astype(np.float32)
    return d


def _cfg(base, H):
    """the rollout's Cfg at padded horizon H: 1 / 2 / 4 samples per knot interval, or a horizon that is no multiple of them"""
    per = (H - 1) // (N_KNOTS + DEGREE + 1)
    cfg = base(n_knots=N_KNOTS, bspline_degree=DEGREE, interpolation_steps=per)
    if cfg.padded_horizon != H:
        class Padded(base):
            padded_horizon = H

        cfg = Padded(n_knots=N_KNOTS, bspline_degree=DEGREE, interpolation_steps=per)
    assert cfg.padded_horizon == H
    return cfg


def _rollout(d, kin, scene, H, terms):
    from curobo_amd.rollout import CollisionRollout, CollisionRolloutCfg, TrajOptRollout, TrajOptRolloutCfg

    t = lambda k: torch.as_tensor(d[k], device=DEV).contiguous()  # noqa: E731
    if terms:
        ro = TrajOptRollout(kin, scene, B, _cfg(TrajOptRolloutCfg, H))
        ro.update_goals(t("pose_position"), t("pose_quat"), torch.as_tensor(GOAL_IDX, dtype=torch.int32, device=DEV))
    else:
        ro = CollisionRollout(kin, scene, B, _cfg(CollisionRolloutCfg, H))
    # the state rows, the indices, dt and goal mode exactly as the launch reads them (set before the first evaluation)
    ro.start_pos, ro.start_vel, ro.start_acc, ro.start_jerk = (t(f"start_{k}") for k in ("position", "velocity", "acceleration", "jerk"))
    ro.goal_pos, ro.goal_vel, ro.goal_acc, ro.goal_jerk = (t(f"goal_{k}") for k in ("position", "velocity", "acceleration", "jerk"))
    ro.start_idx.copy_(torch.as_tensor(START_IDX, dtype=torch.int32))
    ro.goal_idx.copy_(torch.as_tensor(GOAL_IDX, dtype=torch.int32))
    ro._traj_dt = torch.tensor(TRAJ_DT, device=DEV, dtype=torch.float32)
    ro._implicit_goal = torch.tensor(IMPLICIT, device=DEV, dtype=torch.uint8)
    if terms:
        ro.update_traj_dt(ro._traj_dt)  # (the c-space term's per-trajectory dt and the speed metric's follow)
    return ro


def _memo(x, parity):
    """stride 1: rows of ``parity`` get their own bits, the others a row that differs in one word; sentinels per row"""
    mx = x.clone()
    for b in range(B):
        if b % 2 != parity:
            mx.view(torch.int32)[b, (11 * b + 5) % mx.shape[1]] ^= 1
    mc = SENTINEL + torch.arange(B, device=x.device, dtype=torch.float32)
    mg = (2 * SENTINEL + torch.arange(B, device=x.device, dtype=torch.float32)).unsqueeze(1).expand(B, x.shape[1]).contiguous()
    return mx, mc, mg


def replay(d, memo=None, probe=None):
    """every case on the inputs ``d`` -> {name_cost / name_grad: int32 array}; ``memo``: None, "even" or "odd" (module docstring)"""
    from curobo_amd.backends import rollout as rollout_hip
    from curobo_amd.robot import load_packaged_robot
    from curobo_amd.robot.kinematics_params import KinematicsParams
    from curobo_amd.scene import SceneData, cuboid_scene_arrays
    from curobo_amd.workloads import c2_world

    bits = lambda t: t.detach().cpu().contiguous().numpy().view(np.int32).copy()  # noqa: E731
    kin = KinematicsParams.from_model(load_packaged_robot("franka"), DEV)
    scene = SceneData.from_arrays(cuboid_scene_arrays(c2_world()), DEV)
    x = torch.as_tensor(d["knots"], device=DEV).reshape(B, -1).contiguous()
    out = {}
    for name, H, terms, shapes in cases():
        ro = _rollout(d, kin, scene, H, terms)
        fused = bool(ro.cfg.use_fused and ro._fused_chosen())
        assert fused, f"{name}: not the fused launch"
        kw = {} if memo is None else dict(memo=(*_memo(x, 0 if memo == "even" else 1), 1, 0))
        rollout_hip.set_fused_shapes_enabled(shapes)
        try:
            cost, grad = ro.cost_and_gradient_fused(x.view(B, N_KNOTS, -1), **kw)
            torch.cuda.synchronize()
        finally:
            rollout_hip.set_fused_shapes_enabled(True)
        out[f"{name}_cost"], out[f"{name}_grad"] = bits(cost), bits(grad.reshape(B, -1))
        if probe is not None:
            probe[name] = dict(fused=fused, reuse=ro.offers_reuse(1))
    return out


def memo_differing(got, want, parity):
    """what a replay with the memo of ``parity`` must give: sentinels in the rows of that parity, the recorded bits elsewhere"""
    f32 = lambda v: np.asarray(v, np.float32).view(np.int32)  # noqa: E731
    bad = {}
    for name, *_ in cases():
        c, g = want[f"{name}_cost"].copy(), want[f"{name}_grad"].copy()
        for b in range(parity, B, 2):
            c[b] = f32([SENTINEL + b])[0]
            g[b] = f32([2 * SENTINEL + b])[0]
        for k, v in ((f"{name}_cost", c), (f"{name}_grad", g)):
            if not np.array_equal(got[k], v):
                bad[k] = int((got[k] != v).sum())
    return bad


def check(d, recorded, probe):
    broken = []
    assert sorted(START_IDX) != list(START_IDX) and sorted(GOAL_IDX) != list(GOAL_IDX)
    assert set(START_IDX) == {0, 1, 2} and set(GOAL_IDX) == {0, 1} and set(IMPLICIT) == {0, 1} and TRAJ_DT[0] != TRAJ_DT[1]
    for name, H, terms, shapes in cases():
        cost, grad = recorded[f"{name}_cost"].view(np.float32), recorded[f"{name}_grad"].view(np.float32)
        ok = probe[name]["fused"] and probe[name]["reuse"] and bool(np.isfinite(cost).all() and np.isfinite(grad).all()) and bool((cost > 0).any())
        print(f"{name}: padded horizon {H}, {int((cost > 0).sum())} of {B} trajectories cost something, max |grad| {np.abs(grad).max():.4g}")
        if not ok:
            broken.append(name)
    for H in HORIZONS:  # shape and generic kernel agree (what tests/test_fused_shapes.py holds at the built-in shapes)
        for kind in ("collision", "terms"):
            for part in ("cost", "grad"):
                if not np.array_equal(recorded[f"h{H}_{kind}_shape_{part}"], recorded[f"h{H}_{kind}_generic_{part}"]):
                    broken.append(f"h{H}_{kind}: shape != generic ({part})")
    assert not broken, f"cases that break the fixture's conditions: {broken}"
    for parity, word in ((0, "even"), (1, "odd")):
        bad = memo_differing(replay(d, memo=word), recorded, parity)
        assert not bad, f"memo rows of {word} parity: {bad}"


def differing(got, want):
    return {k: int((got[k] != want[k]).sum()) if got[k].shape == want[k].shape else -1 for k in want if not np.array_equal(got.get(k), want[k])}


def load(path=PATH):
    """(inputs, recorded outputs) of the file"""
    z = np.load(path)
    return {k[3:]: z[k] for k in z.files if k.startswith("in/")}, {k[4:]: z[k] for k in z.files if k.startswith("out/")}


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    if sys.argv[1:2] == ["--replay"]:  # the fresh process of the recorder: the file's inputs give the file's outputs
        given, recorded = load(sys.argv[2])
        diff = differing(replay(given), recorded)
        print(f"replay in a fresh process: differing {diff or 'none'}")
        sys.exit(1 if diff else 0)
    given, probe = inputs(), {}
    recorded = replay(given, probe=probe)
    assert all(v.dtype == np.int32 for v in recorded.values())
    check(given, recorded, probe)
    diff = differing(replay(given), recorded)
    assert not diff, f"two replays in one process differ: {diff}"
    target = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(target + ".tmp.npz", **{f"in/{k}": v for k, v in given.items()}, **{f"out/{k}": v for k, v in recorded.items()})
    try:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--replay", target + ".tmp.npz"], check=True, timeout=300)
        os.replace(target + ".tmp.npz", target)
    finally:
        if os.path.exists(target + ".tmp.npz"):
            os.remove(target + ".tmp.npz")
    assert os.path.getsize(target) <= 64 * 1024, os.path.getsize(target)
    print(f"{target}: {len(given)} inputs, {len(recorded)} outputs, {sum(v.size for v in recorded.values())} words, {os.path.getsize(target)} bytes")
