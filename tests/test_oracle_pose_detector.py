"""The reference's recorded fp32 pose-refinement output (tests/golden/pose_detector_golden.npz, made by
tests/golden/make_pose_detector_golden.py from the reference's own Warp kernels and LM functions) against the float64 oracle
tests/pose_detector_ref.py, under the bounds and exclusions stated there.  This is where the constants C and K the GPU tests
use are established (docs/ORACLE_PINS.md): the largest ratios the reference itself reaches are printed."""

import dataclasses
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

import pose_detector_ref as R

G = np.load(os.path.join(GOLDEN_DIR, "pose_detector_golden.npz"))
EVAL = [str(n) for n in G["eval_case_names"]]
SEQ = [str(n) for n in G["sequence_names"]]
_cache = {}


def oracle_eval(name):
    if name not in _cache:
        thr, maxd, hub, delta = G[f"{name}/params"]
        _cache[name] = R.evaluate(G[f"{name}/points"], G[f"{name}/position"], G[f"{name}/quaternion"], G[f"{name}/vertices"], G[f"{name}/faces"],
                                  float(np.float32(maxd)), float(np.float32(thr)), bool(hub), float(np.float32(delta)))
    return _cache[name]


def needed_c(name, dist, grad, valid):
    """asserts valid equal outside the excluded set and the excluded share; returns the smallest C that holds BOTH per-point
    bounds (distance within C 2^-24 S, gradient within 2 C 2^-24 S / dist + 4 2^-24) on this case"""
    ev = oracle_eval(name)
    keep = ~ev["excluded"]
    assert ev["excluded"].mean() <= 0.01, (name, ev["excluded"].mean())
    assert np.array_equal(np.asarray(valid).astype(bool)[keep], ev["valid"][keep]), name
    inv = keep & ~ev["valid"]
    assert (np.asarray(dist)[inv] == 0).all() and (np.asarray(grad)[inv] == 0).all(), name
    m = keep & ev["valid"]
    if not m.any():
        return 0.0
    cd = np.abs(np.asarray(dist, np.float64) - ev["dist"])[m] / (R.EPS * ev["S"][m])
    eg = np.abs(np.asarray(grad, np.float64) - ev["grad"]).max(1)[m]
    cg = np.maximum(eg - 4.0 * R.EPS, 0.0) * ev["raw_dist"][m] / (2.0 * R.EPS * ev["S"][m])
    return float(max(cd.max(), cg.max()))


@pytest.mark.parametrize("name", EVAL)
def test_reference_per_point_output_is_inside_the_bound(name):
    ev = oracle_eval(name)
    need = needed_c(name, G[f"{name}/dist"], G[f"{name}/grad"], G[f"{name}/valid"])
    print(f"{name}: needs C = {need:.3f} (C = {R.POSE_DISTANCE_C}), excluded {int(ev['excluded'].sum())} of {len(ev['valid'])}")
    assert need <= R.POSE_DISTANCE_C / 2, "the constant is twice the smallest power of two that holds the reference"


def test_distance_constant_is_twice_the_smallest_power_of_two():
    worst = max(needed_c(n, G[f"{n}/dist"], G[f"{n}/grad"], G[f"{n}/valid"]) for n in EVAL)
    print("largest C the reference needs over all cases:", worst)
    assert R.POSE_DISTANCE_C == 2.0 * 2.0 ** np.ceil(np.log2(worst)), worst


@pytest.mark.parametrize("name", EVAL)
def test_reference_sums_are_inside_the_order_free_bound(name):
    thr, maxd, hub, delta = G[f"{name}/params"]
    J, r, v = R.jacobian_from_outputs(G[f"{name}/points"], G[f"{name}/dist"], G[f"{name}/grad"], G[f"{name}/valid"], bool(hub), delta)
    s = R.sums_of(J, r, v)
    n = len(r)
    # the per-term rounding of the fp32 Jacobian entries (a few ulp of each product) rides on top of the summation bound
    k = (n + 8) * R.EPS
    assert int(G[f"{name}/n"][0]) == s["n"]
    assert (np.abs(G[f"{name}/JtJ"].astype(np.float64) - s["JtJ"]) <= k * s["abs_JtJ"] + 1e-45).all(), name
    assert (np.abs(G[f"{name}/Jtr"].astype(np.float64) - s["Jtr"]) <= k * s["abs_Jtr"] + 1e-45).all(), name
    assert abs(float(G[f"{name}/sum_sq"][0]) - s["sum_sq"]) <= k * s["abs_sum_sq"] + 1e-45, name
    if s["n"] == 0:
        assert not G[f"{name}/JtJ"].any() and not G[f"{name}/Jtr"].any() and float(G[f"{name}/sum_sq"][0]) == 0.0


def lm_iteration_ratios(name, it):
    """teacher-forced on the golden's state before iteration ``it``: returns None when the iteration is skipped, else the
    ratio of the reference's delta error to cond 2^-24 |delta|; asserts the rest"""
    g = lambda k: G[f"{name}/{k}"][it]  # noqa: E731
    prm = G[f"{name}/params"]
    JtJ, Jtr, lam = g("before_best_JtJ").reshape(6, 6), g("before_best_Jtr"), float(g("before_lambda_damping")[0])
    cand = R.lm_candidate(JtJ, Jtr, lam, g("before_best_position"), g("before_best_quaternion"))
    assert cand["ok"]
    tol_delta, tol_pos, tol_quat, tol_pred = R.lm_step_bounds(cand, JtJ, Jtr, g("before_best_position"))
    ratio = np.abs(g("delta") - cand["delta"]).max() / (cand["cond"] * R.EPS * np.abs(cand["delta"]).max() + 1e-30)
    assert np.abs(g("delta") - cand["delta"]).max() <= tol_delta, (name, it, ratio)
    assert np.abs(g("cand_position") - cand["position"]).max() <= tol_pos, (name, it)
    assert np.abs(g("cand_quaternion") - cand["quaternion"]).max() <= tol_quat, (name, it)
    assert abs(float(g("pred")) - cand["pred"]) <= tol_pred, (name, it)
    acc, lam_new, trust, err = R.trust_update(float(g("before_best_sum_sq")[0]), float(g("pred")), lam, float(g("cand_sum_sq")),
                                              int(g("cand_n_valid")), prm[5], prm[6], prm[7])
    # The only iterations that may be skipped are those whose trust ratio is within 1e-4 of 0 or whose count is 10 or 11; they
    # are held to the oracle all the same (it is forced onto the golden's own fp32 sums and prediction, so it nearly always
    # decides as the reference did) and skipped only where it does not.
    if acc != bool(g("accepted")) and (abs(trust) < 1e-4 or int(g("cand_n_valid")) in (10, 11)):
        return None
    assert acc == bool(g("accepted")), (name, it, trust)
    assert np.float32(lam_new) == g("after_lambda_damping")[0], (name, it)
    src = "cand" if acc else "before_best"
    assert np.array_equal(g("after_best_position"), g(f"{src}_position")) and np.array_equal(g("after_best_quaternion"), g(f"{src}_quaternion"))
    assert np.array_equal(g("after_best_JtJ"), g("cand_JtJ") if acc else g("before_best_JtJ"))
    assert np.array_equal(g("after_best_Jtr"), g("cand_Jtr") if acc else g("before_best_Jtr"))
    if acc:
        assert abs(float(g("after_best_error")[0]) - err) <= 4 * R.EPS * err and int(g("after_best_n_valid")[0]) == int(g("cand_n_valid"))
    return float(ratio)


@pytest.mark.parametrize("name", SEQ)
def test_reference_lm_iterations_follow_the_oracle(name):
    n_it = G[f"{name}/delta"].shape[0]
    ratios = [lm_iteration_ratios(name, it) for it in range(n_it)]
    skipped = sum(r is None for r in ratios)
    print(f"{name}: largest delta error / (cond 2^-24 |delta|) = {max([r for r in ratios if r is not None] or [0.0]):.3f} (K = {R.POSE_LM_K}), "
          f"skipped {skipped} of {n_it}")
    assert skipped <= 2
    if name in ("seq_clean", "seq_noisy"):
        assert n_it == 25
    worst = max([r for r in ratios if r is not None] or [0.0])
    assert worst <= R.POSE_LM_K / 2, "K is twice the smallest power of two that holds the reference"


def test_cfg_defaults_equal_the_recorded_ones():
    from curobo_amd.perception import SDFDetectorCfg

    ours = {f.name: getattr(SDFDetectorCfg(), f.name) for f in dataclasses.fields(SDFDetectorCfg) if f.name != "device_cfg"}
    assert list(ours) == [str(n) for n in G["cfg_default_names"]]
    assert [float(v) for v in ours.values()] == G["cfg_default_values"].tolist()
    assert SDFDetectorCfg(distance_threshold=0.3).max_distance == 0.3
