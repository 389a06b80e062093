"""The mesh-SDF pose detector on the GPU (csrc/pose_detect.hip, curobo_amd/perception/pose_estimation) against the float64 oracle
tests/pose_detector_ref.py and the reference's recorded run (tests/golden/pose_detector_golden.npz), under the bounds, constants and
exclusions tests/test_oracle_pose_detector.py established on the reference itself.

Every test prints the figures it asserts on (run with -s)."""

import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

import pose_detector_ref as R

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(GOLDEN_DIR, "pose_detector_golden.npz"))
EVAL = [str(n) for n in G["eval_case_names"]]
SEQ = [str(n) for n in G["sequence_names"]]
DEV = "cuda:0"

_spec = importlib.util.spec_from_file_location("fuzz_pose_detector", os.path.join(os.path.dirname(__file__), "randomised", "fuzz_pose_detector.py"))
FZ = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FZ)


def case_args(name):
    thr, maxd, hub, delta = G[f"{name}/params"]
    return dict(points=G[f"{name}/points"], position=G[f"{name}/position"], quaternion=G[f"{name}/quaternion"], vertices=G[f"{name}/vertices"],
                faces=G[f"{name}/faces"], max_distance=float(maxd), threshold=float(thr), use_huber=bool(hub), delta=float(delta))


@pytest.mark.parametrize("name", EVAL)
def test_evaluation_follows_the_oracle(name):
    """per point against the oracle; the reduced rows against the float64 sums of the kernel's own per-point outputs; count exact"""
    assert FZ.check_case(name, **case_args(name)) == []


def test_zero_valid_points_give_exact_zeros_and_many_workgroups_a_ragged_tail():
    dist, grad, valid, rows = FZ.hip_evaluate(**case_args("lsolid_zero_valid"))
    assert not valid.any() and not dist.any() and not grad.any() and not rows.any()
    dist, grad, valid, rows = FZ.hip_evaluate(**case_args("ico_n5003"))
    assert rows.shape == (20, 32) and rows[-1, 28:29].view(np.int32)[0] == valid[19 * 256:].sum() and valid[19 * 256:].size == 139
    assert [int(r[28:29].view(np.int32)[0]) for r in rows] == [int(valid[b * 256:(b + 1) * 256].sum()) for b in range(20)]
    assert not rows[:, 29:].any()


def test_two_runs_are_bit_identical():
    a, b = FZ.hip_evaluate(**case_args("ico_n5003")), FZ.hip_evaluate(**case_args("ico_n5003"))
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


def lm_step_on_device(name, it):
    """curobo_hip_pose_lm_step in update mode, forced onto the golden's state before iteration ``it`` and its candidate's sums"""
    from curobo_amd.backends import perception as P

    g = lambda k: G[f"{name}/{k}"][it]  # noqa: E731
    prm = G[f"{name}/params"]
    st = np.zeros(P.POSE_STATE_WORDS, np.float32)

    def put(field, val, integer=False):
        sl = P.pose_state_slice(field)
        st[sl] = np.asarray(val, np.int32).reshape(-1).view(np.float32) if integer else np.asarray(val, np.float32).reshape(-1)
    for f in ("best_position", "best_quaternion", "best_error", "best_sum_sq", "best_JtJ", "best_Jtr", "lambda_damping"):
        put(f, g(f"before_{f}"))
    put("best_n_valid", g("before_best_n_valid"), True)
    put("cand_position", g("cand_position"))
    put("cand_quaternion", g("cand_quaternion"))
    put("pred_reduction", g("pred"))
    row = np.zeros(P.POSE_WS_ROW, np.float32)
    cj = g("cand_JtJ").reshape(6, 6)
    row[:21] = [cj[u, v] for u in range(6) for v in range(u, 6)]
    row[21:27], row[27] = g("cand_Jtr"), g("cand_sum_sq")
    row[28:29] = np.asarray([g("cand_n_valid")], np.int32).view(np.float32)
    state, ws = torch.as_tensor(st).to(DEV), torch.as_tensor(row).to(DEV)
    P.pose_lm_step(state, ws, 1, P.POSE_LM_UPDATE, prm[4], prm[5], prm[6], prm[7], prm[8])
    out = state.cpu().numpy()
    get = lambda f: out[P.pose_state_slice(f)]  # noqa: E731
    return get, g, prm


@pytest.mark.parametrize("name", SEQ)
def test_lm_step_teacher_forced_on_every_recorded_iteration(name):
    skipped, worst = 0, 0.0
    for it in range(G[f"{name}/delta"].shape[0]):
        get, g, prm = lm_step_on_device(name, it)
        acc = bool(get("accepted").view(np.int32)[0])
        _, _, trust, err = R.trust_update(float(g("before_best_sum_sq")[0]), float(g("pred")), float(g("before_lambda_damping")[0]),
                                          float(g("cand_sum_sq")), int(g("cand_n_valid")), prm[5], prm[6], prm[7])
        if acc != bool(g("accepted")) and (abs(trust) < 1e-4 or int(g("cand_n_valid")) in (10, 11)):
            skipped += 1  # (the same rule as tests/test_oracle_pose_detector.py: skipped only where the decision differs inside the band)
            continue
        assert acc == bool(g("accepted")), (name, it, trust)
        assert get("lambda_damping")[0] == g("after_lambda_damping")[0], (name, it)
        for f in ("best_position", "best_quaternion", "best_sum_sq", "best_JtJ", "best_Jtr"):  # a selection: exact
            assert np.array_equal(get(f), g(f"after_{f}").reshape(-1).astype(np.float32)), (name, it, f)
        assert get("best_n_valid").view(np.int32)[0] == int(g("after_best_n_valid")[0])
        assert abs(float(get("best_error")[0]) - float(g("after_best_error")[0])) <= 4 * R.EPS * float(g("after_best_error")[0])
        # the next candidate, against the oracle on the selected state: the bound of the CPU test, doubled
        JtJ, Jtr = g("after_best_JtJ").reshape(6, 6), g("after_best_Jtr")
        cand = R.lm_candidate(JtJ, Jtr, float(g("after_lambda_damping")[0]), g("after_best_position"), g("after_best_quaternion"))
        assert cand["ok"]
        td, tp, tq, tr = (2.0 * t for t in R.lm_step_bounds(cand, JtJ, Jtr, g("after_best_position")))
        worst = max(worst, float(np.abs(get("delta") - cand["delta"]).max() / td))
        assert np.abs(get("delta") - cand["delta"]).max() <= td, (name, it)
        assert np.abs(get("cand_position") - cand["position"]).max() <= tp and np.abs(get("cand_quaternion") - cand["quaternion"]).max() <= tq
        assert abs(float(get("pred_reduction")[0]) - cand["pred"]) <= tr, (name, it)
    print(f"{name}: skipped {skipped}, delta at {worst:.3f} of its bound")
    assert skipped <= 2


def rotation_error(q, q_true):
    q, qt = np.asarray(q, np.float64), np.asarray(q_true, np.float64)
    vec = qt[0] * q[1:] - q[0] * qt[1:] - np.cross(qt[1:], q[1:])
    return float(2.0 * np.arctan2(np.linalg.norm(vec), abs(q @ qt)))


def detector(name, **cfg):
    from curobo_amd.perception import RobotMesh, SDFDetectorCfg, SDFPoseDetector

    return SDFPoseDetector(RobotMesh(G[f"{name}/vertices"], G[f"{name}/faces"], device=DEV), SDFDetectorCfg(n_points=400, **cfg))


def run(det, name):
    from curobo_amd.types import Pose

    init = Pose(torch.as_tensor(G[f"{name}/init_position"])[None], torch.as_tensor(G[f"{name}/init_quaternion"])[None])
    return det.detect_from_points(torch.as_tensor(G[f"{name}/points"]), initial_pose=init)


_results = {}


def result(name, graph=True):
    if (name, graph) not in _results:
        _results[(name, graph)] = run(detector(name, use_cuda_graph=graph), name)
    return _results[(name, graph)]


@pytest.mark.parametrize("name", ["seq_clean", "seq_noisy"])
def test_detect_from_points_end_to_end(name):
    res = result(name)
    p, q = res.pose.position[0].cpu().numpy(), res.pose.quaternion[0].cpu().numpy()
    t_err = float(np.linalg.norm(p.astype(np.float64) - G[f"{name}/true_position"]))
    r_err = rotation_error(q, G[f"{name}/true_quaternion"])
    ref_t, ref_r = G[f"{name}/final_error"]
    print(f"{name}: translation error {t_err:.3e} (reference {ref_t:.3e}), rotation error {r_err:.3e} (reference {ref_r:.3e}), "
          f"{res.n_iterations} iterations, alignment error {res.alignment_error:.3e}, confidence {res.confidence}, {res.compute_time * 1e3:.2f} ms")
    bound_t, bound_r = (max(2 * ref_t, 1e-5), max(2 * ref_r, 1e-5)) if name == "seq_clean" else (2 * ref_t, 2 * ref_r)
    assert t_err <= bound_t and r_err <= bound_r
    assert res.n_iterations % 25 == 0 and 25 <= res.n_iterations <= 100 and res.config is None and res.compute_time > 0
    # alignment_error and confidence follow from an evaluation at the final pose
    prm = G[f"{name}/params"]
    _, _, valid, rows = FZ.hip_evaluate(G[f"{name}/points"], p, q, G[f"{name}/vertices"], G[f"{name}/faces"], float(prm[1]), float(prm[0]), bool(prm[2]),
                                        float(prm[3]))
    _, _, ssq, n = FZ.reduce_rows(rows)
    assert res.confidence == min(1.0, (n / 400) / 0.1)
    assert abs(res.alignment_error - np.sqrt(ssq / (n + 1e-8))) <= 1e-6 * res.alignment_error + 1e-12


@pytest.mark.parametrize("name", ["seq_clean", "seq_noisy"])
def test_captured_and_eager_results_are_bit_identical(name):
    a, b = result(name, True), result(name, False)
    assert torch.equal(a.pose.position, b.pose.position) and torch.equal(a.pose.quaternion, b.pose.quaternion)
    assert (a.alignment_error, a.confidence, a.n_iterations) == (b.alignment_error, b.confidence, b.n_iterations)


def test_second_call_replays_the_graph_over_rewritten_buffers():
    det = detector("seq_clean")
    run(det, "seq_clean")
    graph = det._runs[400].graph
    second = run(det, "seq_noisy")  # other points, another result; the same mesh and initial pose family
    assert det._runs[400].graph is graph and graph is not None and list(det._runs) == [400]
    fresh = result("seq_noisy")
    assert torch.equal(second.pose.position, fresh.pose.position) and torch.equal(second.pose.quaternion, fresh.pose.quaternion)
    assert (second.alignment_error, second.n_iterations) == (fresh.alignment_error, fresh.n_iterations)
    from curobo_amd.types import Pose

    other = Pose(torch.as_tensor(G["seq_clean/true_position"])[None] + 0.004, torch.as_tensor(G["seq_clean/true_quaternion"])[None])
    third = det.detect_from_points(torch.as_tensor(G["seq_clean/points"]), initial_pose=other)
    again = detector("seq_clean").detect_from_points(torch.as_tensor(G["seq_clean/points"]), initial_pose=other)
    assert torch.equal(third.pose.position, again.pose.position) and torch.equal(third.pose.quaternion, again.pose.quaternion)


def test_more_points_than_n_points_are_subsampled():
    from curobo_amd.perception import RobotMesh, SDFDetectorCfg, SDFPoseDetector
    from curobo_amd.types import Pose

    name = "seq_clean"
    det = SDFPoseDetector(RobotMesh(G[f"{name}/vertices"], G[f"{name}/faces"], device=DEV), SDFDetectorCfg(n_points=300, max_iterations=25))
    torch.manual_seed(3)
    init = Pose(torch.as_tensor(G[f"{name}/init_position"])[None], torch.as_tensor(G[f"{name}/init_quaternion"])[None])
    res = det.detect_from_points(torch.as_tensor(G[f"{name}/points"]), initial_pose=init)
    assert list(det._runs) == [300] and det._runs[300].points.shape == (300, 3) and res.n_iterations == 25
    assert np.isfinite(res.alignment_error) and res.alignment_error < 1e-3


def test_randomised_sweep_of_the_evaluation():
    assert FZ.main(12, 20261018) == 0
