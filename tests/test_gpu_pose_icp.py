"""The ICP pose detector on the GPU (csrc/pose_icp.hip, curobo_amd/perception/pose_estimation/pose_detector.py) against the
float64 oracle tests/pose_icp_ref.py and the reference's recorded runs (tests/golden/pose_icp_golden.npz), under the bounds,
constants and exclusions tests/test_oracle_pose_icp.py established on the reference itself.

Every test prints the figures it asserts on (run with -s)."""

import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

import pose_icp_ref as R

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(GOLDEN_DIR, "pose_icp_golden.npz"))
CFG = dict(zip(G["cfg_names"].tolist(), G["cfg_values"].tolist()))
DEV = "cuda:0"

_spec = importlib.util.spec_from_file_location("fuzz_pose_icp", os.path.join(os.path.dirname(__file__), "randomised", "fuzz_pose_icp.py"))
FZ = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FZ)


def scene(m, o, h, seed, spread=0.004, duplicate=False):
    """m samples of a random surface, o observations of it at a pose, h hypotheses around that pose (distinct T each)"""
    rng = np.random.default_rng(seed)
    p, nrm = FZ.random_surface(rng, 12, m)
    truth = np.concatenate([FZ.random_rotations(rng, 1)[0], [[0.31], [-0.12], [0.45]]], 1)
    obs = p[rng.integers(0, m, o)] @ truth[:, :3].T + truth[:, 3] + rng.normal(0, spread, (o, 3))
    if duplicate:
        obs = obs[rng.integers(0, max(1, o // 3), o)]
    T = [(R.update_matrix(np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 3)])) @ np.vstack([truth, [0, 0, 0, 1]]))[:3].reshape(-1)
         for _ in range(h)]
    return dict(mesh_points=p.astype(np.float32), mesh_normals=nrm.astype(np.float32), observed=obs.astype(np.float32), T=np.asarray(T, np.float32))


# M around the 64-sample workgroup and the 256 of the other detector, O around the wavefront, a wavefront's slice (256) and the
# LDS tile (1024); H with distinct transforms
SHAPES = [(1, 1, 1), (255, 63, 3), (256, 64, 8), (257, 65, 1), (500, 1000, 3), (65, 1500, 1), (64, 257, 8), (500, 1, 3), (1, 1000, 8),
          (255, 1025, 1)]


@pytest.mark.parametrize("m,o,h", SHAPES)
@pytest.mark.parametrize("huber", [True, False])
def test_correspond_follows_the_oracle(m, o, h, huber):
    """index exact and distance within bound outside the excluded set; rows against the float64 sums of the kernel's own
    per-sample outputs; counts exact (FZ.check_case holds the rules)"""
    assert FZ.check_case(f"M {m} O {o} H {h}", **scene(m, o, h, seed=m * 7 + o), threshold=0.03, use_huber=huber, delta=0.01, step=False) == []


def test_duplicated_observations_give_the_lowest_index():
    s = scene(300, 1400, 2, seed=11, duplicate=True)
    idx, dist, rows, _, _ = FZ.hip_correspond(**s, threshold=np.inf, use_huber=True, delta=0.02)
    o = s["observed"]
    first = np.array([np.flatnonzero((o == o[k]).all(1))[0] for k in range(len(o))])
    assert (first != np.arange(len(o))).sum() > 500  # the fixture does repeat points
    assert np.array_equal(first[idx], idx), "a duplicate with a higher index was returned"
    assert FZ.check_case("duplicates", **s, threshold=np.inf, use_huber=True, delta=0.02, step=False) == []
    print("duplicated observations:", int((first != np.arange(len(o))).sum()), "of", len(o), "are repeats; every match is a first occurrence")


def test_zero_valid_and_an_infinite_threshold():
    s = scene(257, 300, 3, seed=5)
    far = dict(s, observed=s["observed"] + np.float32([2.0, 0, 0]))
    idx, dist, rows, _, _ = FZ.hip_correspond(**far, threshold=0.05, use_huber=True, delta=0.02)
    assert (idx == -1).all() and not rows[:, :, :27].any() and not rows[:, :, 28:].view(np.int32).any()
    assert (dist > 1.0).all() and np.allclose(rows[:, :, 27].sum(1), dist.sum(1), rtol=1e-5)  # the distances are summed all the same
    idx, dist, rows, _, _ = FZ.hip_correspond(**far, threshold=np.inf, use_huber=True, delta=0.02)
    assert (idx >= 0).all() and rows[:, :, 28].view(np.int32).sum(1).tolist() == [257, 257, 257]
    print("zero valid: sums and counts exactly zero; infinite threshold: 257 of 257 valid per hypothesis")


def test_a_stopped_hypothesis_is_left_alone_and_two_runs_are_bit_identical():
    from curobo_amd.backends import perception as P

    s = scene(300, 700, 3, seed=9)
    a = FZ.hip_correspond(**s, threshold=0.03, use_huber=True, delta=0.01)
    b = FZ.hip_correspond(**s, threshold=0.03, use_huber=True, delta=0.01)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    idx, dist, rows, state, ws = FZ.hip_correspond(**s, threshold=0.03, use_huber=True, delta=0.01, stopped=[0, 1, 0], ws_fill=7.0)
    assert (rows[1] == 7.0).all() and (idx[1] == -7).all() and (dist[1] == -1.0).all()  # untouched
    for h in (0, 2):
        assert np.array_equal(rows[h].view(np.int32), a[2][h].view(np.int32)) and np.array_equal(idx[h], a[0][h])
    before = state.clone()
    P.pose_icp_step(state, ws, 300, P.POSE_ICP_COARSE)
    torch.cuda.synchronize()
    assert torch.equal(state[1].view(torch.int32), before[1].view(torch.int32))
    assert FZ.state_field(state, "iterations")[:, 0].tolist() == [1, 0, 1] and not torch.equal(state[0], before[0])
    # without honour_stopped (the final error) the stopped hypothesis is evaluated like the others
    every = FZ.hip_correspond(**s, threshold=0.03, use_huber=True, delta=0.01, stopped=[0, 1, 0], honour_stopped=False)
    assert np.array_equal(every[2].view(np.int32), a[2].view(np.int32))
    print("stopped hypothesis: rows, outputs and state untouched; two runs bit-identical")


def forced_step(rows28, counts, T, mode):
    """curobo_hip_pose_icp_step on given sums: one 'hypothesis' per row, a workspace of one row each"""
    from curobo_amd.backends import perception as P

    n = len(rows28)
    ws = np.zeros((n, P.POSE_WS_ROW), np.float32)
    ws[:, :28] = rows28
    ws[:, 28] = np.asarray(counts, np.int32).view(np.float32)
    state, wsd = FZ.make_state(T), FZ.to_dev(ws.reshape(-1))
    P.pose_icp_step(state, wsd, 1, mode)
    torch.cuda.synchronize()
    return {k: FZ.state_field(state, k) for k in ("T", "x", "error", "iterations", "stopped", "solver_failed", "n_valid")}


@pytest.mark.parametrize("stage", ["coarse", "fine"])
def test_step_teacher_forced_on_every_recorded_iteration(stage):
    mode = R.COARSE if stage == "coarse" else R.FINE
    sel = np.nonzero(G[f"fp32/{stage}/solved"])
    rows, counts, T = G[f"fp32/{stage}/rows"][sel], G[f"fp32/{stage}/count"][sel], G[f"fp32/{stage}/T_before"][sel]
    out = forced_step(rows, counts, T, mode)
    worst, worst_T = 0.0, 0.0
    for k in range(len(rows)):
        A, rhs = R.unpack_row(rows[k])
        st = R.step(A, rhs, int(counts[k]), T[k], mode)
        bound = R.step_bound(st["cond"], st["x"])
        worst = max(worst, float(np.abs(out["x"][k] - st["x"]).max() / bound))
        assert out["solver_failed"][k, 0] == 0 and out["iterations"][k, 0] == 1 and out["n_valid"][k, 0] == counts[k]
        assert bool(out["stopped"][k, 0]) == st["stopped"], (stage, k)
        if st["stopped"]:
            assert np.array_equal(out["T"][k], T[k])
        else:  # the update's rounding next to entries of size <= 1 + |t| (the bound the reference's own T is held to)
            e = float(np.abs(out["T"][k] - st["T"].reshape(-1)).max())
            worst_T = max(worst_T, e / (2.0 * bound + 32 * R.EPS))
    print(f"{stage}: {len(rows)} recorded steps, x at {worst:.3f} of the K = {R.POSE_ICP_K} bound, T at {worst_T:.3f} of its bound")
    assert worst <= 1.0 and worst_T <= 1.0


def test_step_edges_count_translation_stop_planar_and_finalize():
    from curobo_amd.backends import perception as P

    sel = np.nonzero(G["fp32/coarse/solved"])
    row, T = G["fp32/coarse/rows"][sel][0], G["fp32/coarse/T_before"][sel][0]
    out = forced_step(np.stack([row, row]), [9, 10], np.stack([T, T]), R.COARSE)
    assert out["stopped"][:, 0].tolist() == [1, 0] and out["iterations"][:, 0].tolist() == [1, 1] and out["solver_failed"][:, 0].tolist() == [0, 0]
    assert np.array_equal(out["T"][0], T) and not np.array_equal(out["T"][1], T)
    # fine mode: the same system scaled until |t| < 1e-4 stops BEFORE the update; T bit-unchanged, the counter the reference's
    A, rhs = R.unpack_row(row)
    x, _ = R.solve(A, rhs)
    scale = np.float32(0.5e-4 / np.linalg.norm(x[3:]))
    small = row.copy()
    small[21:27] *= scale
    out = forced_step(np.stack([small, small, row]), [200, 200, 200], np.stack([T, T, T]), R.FINE)
    o2 = forced_step(np.stack([small]), [200], np.stack([T]), R.COARSE)
    assert out["stopped"][:, 0].tolist() == [1, 1, int(np.linalg.norm(x[3:]) < 1e-4)] and out["iterations"][:, 0].tolist() == [1, 1, 1]
    assert np.array_equal(out["T"][0].view(np.int32), T.view(np.int32)) and o2["stopped"][0, 0] == 0 and not np.array_equal(o2["T"][0], T)
    # a planar point set: J^T J of rank 3.  A finite T, or T unchanged with solver_failed; never a NaN
    rng = np.random.default_rng(2)
    p = np.c_[rng.uniform(-0.2, 0.2, (300, 2)), np.zeros(300)].astype(np.float32)
    n = np.tile(np.float32([0, 0, 1]), (300, 1))
    obs = (p + np.float32([0.002, -0.001, 0.004])).astype(np.float32)
    eye = np.eye(4, dtype=np.float32)[:3].reshape(-1)
    idx, dist, rows, state, ws = FZ.hip_correspond(p, n, obs, eye[None], np.inf, True, 0.02)
    P.pose_icp_step(state, ws, 300, P.POSE_ICP_COARSE)
    torch.cuda.synchronize()
    Tp, failed, stopped = FZ.state_field(state, "T")[0], int(FZ.state_field(state, "solver_failed")[0, 0]), int(FZ.state_field(state, "stopped")[0, 0])
    print("planar set: solver_failed", failed, "stopped", stopped, "T", Tp)
    assert np.isfinite(Tp).all() and np.isfinite(FZ.state_field(state, "x")).all()
    assert (failed == 1 and stopped == 1 and np.array_equal(Tp, eye)) or (failed == 0 and stopped == 0)
    # finalize: error = sum of distances / M; nothing else changes; +inf when nothing is valid
    before = state.clone()
    P.pose_icp_step(state, ws, 300, P.POSE_ICP_FINALIZE)
    torch.cuda.synchronize()
    err = float(FZ.state_field(state, "error")[0, 0])
    assert abs(err - dist.astype(np.float64).sum() / 300) <= 301 * R.EPS * dist.sum() / 300
    keep = [k for k in range(P.POSE_ICP_STATE_WORDS) if k != P.pose_icp_state_slice("error").start]
    assert torch.equal(state[:, keep].view(torch.int32), before[:, keep].view(torch.int32))
    empty = forced_step(np.zeros((1, 28), np.float32), [0], eye[None], R.FINALIZE)
    assert np.isposinf(empty["error"][0, 0]) and empty["iterations"][0, 0] == 0 and np.array_equal(empty["T"][0], eye)
    print(f"count 9 stops, 10 proceeds; fine stop leaves T bit-unchanged; finalize error {err * 1e3:.4f} mm, +inf with nothing valid")


def test_select_ties_inf_nan_and_one_hypothesis():
    from curobo_amd.backends import perception as P

    def select(errors):
        st = np.zeros((len(errors), P.POSE_ICP_STATE_WORDS), np.float32)
        st[:, 12] = errors
        st[:, 0] = np.arange(len(errors))  # T[0] tells the hypotheses apart
        state = FZ.to_dev(st)
        idx, err, T = torch.full((1,), -1, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV), torch.zeros(12, device=DEV)
        P.pose_icp_select(idx, state, err, T)
        torch.cuda.synchronize()
        assert float(T[0]) == float(idx.item())
        return int(idx.item()), float(err.item())

    inf, nan = np.inf, np.nan
    assert select([0.3, 0.1, 0.2, 0.1]) == (1, np.float32(0.1))             # the first of a tie
    assert select([nan, 0.5, nan, 0.4, 0.4])[0] == 3                         # a NaN never wins
    assert select([inf, inf, inf])[0] == 0 and select([nan, nan])[0] == 0    # nothing finite: hypothesis 0
    assert select([inf, 2.0, inf])[0] == 1
    assert select([0.7]) == (0, np.float32(0.7))                             # H = 1
    e = np.full(200, 1.0, np.float32)                                        # more hypotheses than lanes
    e[[70, 135, 199]] = 0.25
    assert select(e)[0] == 70
    e[3] = 0.25
    assert select(e)[0] == 3
    print("select: ties to the lowest index, NaN never, all-inf gives 0, H = 1 and H = 200")


# ---------------------------------------------------------------------------------------------------- end to end
class _Injected:
    """the golden's recorded samples, in place of the random parts"""

    def __init__(self):
        from curobo_amd.perception.pose_estimation import RobotMesh

        self.mesh = RobotMesh(G["vertices"], G["faces"], device=DEV)

    def get_dof(self):
        return 0

    def sample_surface_points(self, n):
        stage = "coarse" if n == int(CFG["n_mesh_points_coarse"]) else "fine"
        return torch.as_tensor(G[f"{stage}_mesh_points"]).to(DEV), torch.as_tensor(G[f"{stage}_mesh_normals"]).to(DEV)


def make_detector(save_iterations=False):
    from curobo_amd.perception.pose_estimation import DetectorCfg, PoseDetector

    ints = {k: int(v) for k, v in CFG.items() if k.startswith("n_")}
    cfg = DetectorCfg(**ints, distance_threshold_coarse=CFG["distance_threshold_coarse"], distance_threshold_fine=CFG["distance_threshold_fine"],
                      use_huber_loss=bool(CFG["use_huber_loss"]), huber_delta=CFG["huber_delta"], save_iterations=save_iterations)
    geometry = _Injected()
    det = PoseDetector(geometry, cfg)
    det._resample = lambda pts, n: torch.as_tensor(G["coarse_observed" if n == int(CFG["n_observed_points_coarse"]) else "fine_observed"]).to(DEV)
    det._sample_rotations = lambda n: torch.as_tensor(G["rotations"]).to(DEV)
    return det, geometry


def result_T(result):
    return result.pose.get_matrix()[0, :3].cpu().numpy()


@pytest.fixture(scope="module")
def end_to_end():
    det, geometry = make_detector()
    raw = torch.as_tensor(G["observed_raw"])
    first = det.detect_from_points(raw)
    coarse_errors = next(st for key, st in det._stages.items() if key[0] == 0).field("error")[:, 0].cpu().numpy()
    second = det.detect_from_points(raw)
    return det, geometry, first, second, coarse_errors


def test_end_to_end_against_the_truth(end_to_end):
    det, _, first, second, coarse_errors = end_to_end
    t_err, r_err = R.pose_error(result_T(first), G["T_true"])
    bound_t, bound_r = 2 * max(G["fp32/final_error"][0], G["fp64/final_error"][0]), 2 * max(G["fp32/final_error"][1], G["fp64/final_error"][1])
    print(f"end to end: {t_err * 1e3:.4f} mm (bound {bound_t * 1e3:.4f}), {np.degrees(r_err):.4f} deg (bound {np.degrees(bound_r):.4f}); "
          f"best hypothesis {first.best_hypothesis} (reference {int(G['fp32/best_hypothesis'])}), {first.n_iterations} fine iterations "
          f"(reference {int(G['fp32/n_iterations'])}), alignment error {first.alignment_error * 1e3:.4f} mm (reference {G['fp32/alignment_error'][1] * 1e3:.4f})")
    print("coarse errors (mm):", np.round(coarse_errors * 1e3, 3), "reference:", np.round(G["fp32/coarse/error"] * 1e3, 3))
    assert t_err <= bound_t and r_err <= bound_r
    # the lowest-index minimum of the detector's own per-hypothesis errors
    assert first.best_hypothesis == int(np.flatnonzero(coarse_errors == np.nanmin(coarse_errors))[0])
    assert first.coarse_iterations is None and first.fine_iterations is None and first.config is None
    assert first.confidence == 1.0 - min(first.alignment_error / 0.1, 1.0) and 1 <= first.n_iterations <= int(CFG["n_iterations_fine"])
    # the replayed graphs give the same bits
    assert len(det._stages) == 2 and all(st.graph is not None for st in det._stages.values())
    assert torch.equal(first.pose.position, second.pose.position) and torch.equal(first.pose.quaternion, second.pose.quaternion)
    assert first.alignment_error == second.alignment_error and first.best_hypothesis == second.best_hypothesis


def test_ungraphed_run_is_bit_identical_and_keeps_the_iterations(end_to_end):
    _, _, first, _, _ = end_to_end
    det, _ = make_detector(save_iterations=True)
    res = det.detect_from_points(torch.as_tensor(G["observed_raw"]))
    assert all(st.graph is None for st in det._stages.values())
    assert torch.equal(res.pose.position, first.pose.position) and torch.equal(res.pose.quaternion, first.pose.quaternion)
    assert res.best_hypothesis == first.best_hypothesis and res.n_iterations == first.n_iterations
    assert len(res.coarse_iterations) == int(CFG["n_iterations_coarse"]) + 1 and 1 <= len(res.fine_iterations) <= res.n_iterations + 1
    assert all(tuple(T.shape) == (4, 4) for T in res.coarse_iterations + res.fine_iterations)
    assert np.array_equal(res.fine_iterations[0][:3].numpy(), res.coarse_iterations[-1][:3].numpy())
    assert np.allclose(res.fine_iterations[-1][:3].numpy(), result_T(res), atol=1e-6)
    print("ungraphed: bit-identical pose,", len(res.coarse_iterations), "coarse and", len(res.fine_iterations), "fine transforms kept")


def test_initial_pose_runs_the_fine_stage_only_and_feeds_the_sdf_detector(end_to_end):
    from curobo_amd.perception.pose_estimation import SDFDetectorCfg, SDFPoseDetector

    _, geometry, first, _, _ = end_to_end
    det, _ = make_detector()
    raw = torch.as_tensor(G["observed_raw"])
    res = det.detect_from_points(raw, None, initial_pose=first.pose)
    assert res.best_hypothesis == 0 and [key[0] for key in det._stages] == [1]  # no coarse stage was built
    bound_t, bound_r = 2 * max(G["fp32/final_error"][0], G["fp64/final_error"][0]), 2 * max(G["fp32/final_error"][1], G["fp64/final_error"][1])
    t_err, r_err = R.pose_error(result_T(res), G["T_true"])
    print(f"from the first result as initial pose: {t_err * 1e3:.4f} mm, {np.degrees(r_err):.4f} deg")
    assert t_err <= bound_t and r_err <= bound_r
    sdf = SDFPoseDetector(geometry.mesh, SDFDetectorCfg(n_points=len(raw)))
    refined = sdf.detect_from_points(raw.to(DEV), initial_pose=first.pose)
    t_sdf, r_sdf = R.pose_error(result_T(refined), G["T_true"])
    print(f"SDFPoseDetector from the ICP result: {t_sdf * 1e3:.4f} mm, {np.degrees(r_sdf):.4f} deg (bounds {bound_t * 1e3:.4f} mm, {np.degrees(bound_r):.4f} deg)")
    assert t_sdf <= bound_t and r_sdf <= bound_r
