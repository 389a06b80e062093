"""The optimiser side of the L-BFGS iteration against tests/lbfgs_iteration_ref.py on random (B, V, m, N, form, strategy, family):
the candidates, the line search, the L-BFGS step and the one-launch tail in whatever form the dispatch takes for the drawn
dimensions, with the checks and tolerances of tests/test_gpu_lbfgs_iteration.py.
python tests/randomised/fuzz_lbfgs_iteration.py [cases] [seed]"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lbfgs_iteration_cases as C  # noqa: E402
import lbfgs_iteration_ref as R  # noqa: E402
import test_gpu_lbfgs_iteration as T  # noqa: E402
from curobo_amd.backends import optimization as O  # noqa: E402

dev = torch.device("cuda:0")
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
tally = T._Tally()


def draw_v(top):
    edges = [v for v in (1, 7, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024) if v <= top]
    return int(rng.choice(edges)) if rng.random() < 0.5 else int(rng.integers(1, top + 1))


def candidates():
    V, N = draw_v(1024), int(rng.choice([1, 2, 4, 5, 16, 17, 64]))
    ad = int(rng.choice([d for d in (1, 2, 7, V) if V % d == 0]))
    family = str(rng.choice(T.PREP_FAMILIES))
    B, scale, seed = int(rng.integers(1, 40)), bool(rng.random() < 0.7), int(rng.integers(1 << 30))
    what = f"candidates V={V} action_dim={ad} N={N} scale={scale} {family} B={B}"
    al = C.alphas_for(N)
    if family == "non_finite":
        T._prepare_non_finite(dev, max(B, 3), V, ad, al, scale, seed, what)
        return what
    x, d, step_max, _ = T._prepare_inputs(family, B, V, ad, seed)
    d_out, x_set = T._device_prepare(dev, x, d, step_max, al, ad, scale)
    T._check_prepare(R.prepare_search_points(x, d, step_max, al, ad, scale), d_out, x_set, al, np.ones(B, bool), what)
    return what


def line_search():
    B, V, N = int(rng.integers(1, 65)), draw_v(300), int(rng.integers(1, 65))
    family, wolfe, thr = str(rng.choice(C.LS_FAMILIES)), str(rng.choice(C.WOLFE)), C.THRESHOLDS[int(rng.integers(2))]
    what = f"line search V={V} N={N} {wolfe} thresholds={thr} {family} B={B}"
    case = C.line_search_case(B, V, N, family, int(rng.integers(1 << 30)))
    strong, approx = C.wolfe_flags(wolfe, N)
    ref = R.line_search(case["state"], case["search_cost"], case["search_action"], case["search_gradient"], case["step_direction"],
                        case["alphas"], C.LS["c_1"], C.LS["c_2"], strong, approx, C.LS["convergence_iteration"], thr[0], thr[1])
    got = T._device_line_search(dev, case, strong, approx, thr)
    T._check_line_search(ref, got, case["state"], case["search_cost"], case["search_action"], case["search_gradient"], what)
    tally.add(B, int(ref["ambiguous"].sum()))
    return what


def step():
    B, V, m, stable = int(rng.integers(1, 20)), draw_v(1024), int(rng.integers(0, 32)), bool(rng.random() < 0.5)
    what = f"L-BFGS step V={V} m={m} B={B} stable={stable}"
    case = C.lbfgs_case(B, V, m, int(rng.integers(1 << 30)))
    dv = {k: T._up(case[k], dev) for k in ("rho", "y", "s", "x_0", "grad_0")}
    dv["step"] = torch.zeros((B, V), device=dev)
    q, g = case["q"], case["grad_q"]
    for it in range(3):
        st = {k: T._down(v) for k, v in dv.items()}
        r64 = R.lbfgs_step(st["rho"], st["y"], st["s"], q, g, st["x_0"], st["grad_0"], C.EPSILON, stable)
        r32 = R.lbfgs_step(st["rho"], st["y"], st["s"], q, g, st["x_0"], st["grad_0"], C.EPSILON, stable, np.float32)
        O.launch_lbfgs_step(dv["step"], dv["rho"], dv["y"], dv["s"], T._up(q, dev), T._up(g, dev), dv["x_0"], dv["grad_0"], C.EPSILON, B, m, V,
                            stable, True)
        got = {k: T._down(v) for k, v in dv.items()}
        _, flagged, fig = R.check_step(r64, r32, got, f"{what} step {it}")
        T._shifted(st, got, m, what)
        tally.add(B, flagged, fig)
        q, g = C.lbfgs_next(case, q, got["step"], got["x_0"], got["grad_0"], it)
    return what


def tail():
    V, m = draw_v(128), int(rng.integers(0, 32))
    N = int(rng.choice([1, 2, 3, 4, 4, 4, 5, 16, 17, 64]))
    B, overlapped = int(rng.integers(1, 40)), bool(rng.random() < 0.5)
    if rng.random() < 0.2:
        V, m, N = (84, 27, 4) if rng.random() < 0.5 else (7, 7, 4)  # the compile-time shapes
    expect = O.tail_form(V, m, N, C.action_dim_for(V), B, overlapped)
    cfg = dict(wolfe=str(rng.choice(C.WOLFE)), thr=C.THRESHOLDS[int(rng.integers(2))], stable=bool(rng.random() < 0.7),
               scale=bool(rng.random() < 0.7), non_finite=bool(rng.random() < 0.25), seed=int(rng.integers(1 << 30)))
    what = f"tail form={expect} V={V} m={m} N={N} B={B} overlapped={overlapped} {cfg}"
    with contextlib.redirect_stdout(io.StringIO()):
        T._run_tail(dev, tally, B, V, m, N, overlapped, expect, **cfg)
    return what


bad = 0
kinds = (candidates, line_search, step, tail, tail)
for case in range(n_cases):
    kind = kinds[case % len(kinds)]
    state = rng.bit_generator.state
    try:
        kind()
    except AssertionError as e:
        bad += 1
        rng.bit_generator.state = state
        print(f"FAILED case {case} ({kind.__name__}): {str(e)[:600]}".replace("\n", " | "))
        rng.bit_generator.state = state
        rng.integers(1 << 30, size=64)  # (move on from the draw that failed)
print(f"flagged {tally.flagged} of {tally.rows} rows; worst step error / bound {tally.worst[0]:.3f}")
if tally.flagged > 0.005 * max(tally.rows, 1) and n_cases >= 20:
    bad += 1
    print("FAILED: more than 0.5 % of the rows flagged")
print(f"{n_cases} cases, {bad} failed")
sys.exit(1 if bad else 0)
