"""The two graph-planner launches (csrc/graph_planner.hip: edge steering / point feasibility, weighted k-NN) against the float64
oracle (oracle/graph_ref.py over the C oracle's FK, self and scene collision; held by tests/test_oracle_graph.py) on random
batches.   python tests/randomised/fuzz_graph.py [cases] [seed]

Every case draws a steering batch and a k-NN set (builders of tests/graph_cases.py).

steer   robot in {franka, ur10e, dual_ur10e} x scene in {none, c2 cuboids, voxel grid only, cuboids + voxels, analytic primitives,
        40 slots with 35 disabled, the same in 64 slots}; 1 .. 2200 edges (the grid holds 2048); threshold 0.05 .. 0.1 and a long
        edge that sets max_steps in 3 .. 40 with its ratio half a step from an integer; 0 .. 30 % zero-length edges, 0 .. 30 % edges
        that leave the joint limits; row stride dof, dof + 1 or dof + 3 (NaN in the padding).  The starts of the same batch go
        through point mode.  Held: max_steps equal; the index equal on every edge the oracle's band decides, inside the band's
        span on the others; out_node = the fp32 point formula at the returned index to 1e-6, index column 0; point flags equal on
        decided points.  A case whose decided share is below 95 % counts as failed.
knn     1 .. 3000 searched nodes of a longer buffer, k in 1 .. min(64, nodes), 1 .. 300 queries, 1 .. 14 joints; values on the
        2^-8 grid (exact float64 distances, plentiful ties: the stable order must be reproduced, queries are rows of the node
        buffer) or, one case in four, uniform fp32 values (index where the key is clear of its neighbours by 1e-12, distance
        elsewhere)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graph_cases as gc  # noqa: E402

ROBOTS = ("franka", "ur10e", "dual_ur10e")
SCENES = gc.SCENES + ("slots64",)


def draw_steer_case(rng, case):
    robot, scene = ROBOTS[int(rng.integers(len(ROBOTS)))], SCENES[int(rng.integers(len(SCENES)))]
    n = [1, 2047, 2048, 2049, 2200][case % 8] if case % 8 < 5 else int(rng.integers(1, 2201))
    threshold = float(rng.choice([0.05, 0.0625, 0.08, 0.1]))
    max_steps = int(rng.integers(3, 41))
    c = gc.random_edges(robot, scene, n, max_steps, seed=int(rng.integers(1 << 30)), zero_share=float(rng.uniform(0, 0.3)),
                        leaving_share=float(rng.uniform(0, 0.3)), threshold=threshold)
    D = c["weight"].shape[0]
    return dict(c, ld=D + int(rng.choice([0, 1, 3])))


def steer_reference(c):
    from oracle.graph_ref import steer_band, steer_num_steps_ref

    steps, margin = steer_num_steps_ref(c["start"], c["target"], c["weight"], c["threshold"])
    ms = int(steps.max())
    model, arrays = gc.robot(c["robot"]), gc.scene_arrays(c["scene"])
    band = steer_band(c["start"], c["target"], ms, model, arrays)
    return dict(steps=steps, margin=margin, max_steps=ms, case=c, band=band, start_state=band["state"][:, 0])


def describe_steer(c):
    return (f"steer {c['robot']} / {c['scene']} edges {c['start'].shape[0]} max_steps {c['max_steps']} threshold {c['threshold']} ld {c['ld']} "
            f"zero {int(c['zero'].sum())} leaving {int(c['leaving'].sum())}")


def draw_knn_case(rng, case):
    N = [1, 63, 64, 65][case % 8] if case % 8 < 4 else int(rng.integers(1, 3001))
    k = min(N, 64) if rng.random() < 0.4 else int(rng.integers(1, min(N, 64) + 1))
    Q, D = int(rng.integers(1, 301)), int(rng.integers(1, 15))
    if case % 4 == 3:
        buf = rng.uniform(-2, 2, (N + 40, D + 1)).astype(np.float32)
        return dict(buffer=buf, queries=rng.uniform(-2, 2, (Q, D)).astype(np.float32), weight=rng.uniform(0.5, 1.5, D).astype(np.float32),
                    n_nodes=N, k=k, D=D, exact=False)
    return gc.grid_knn_set(rng, N, k, Q, D, tail=int(rng.integers(0, 40)))


def describe_knn(c):
    return f"knn nodes {c['n_nodes']} of {c['buffer'].shape[0]} k {c['k']} queries {gc.knn_queries(c).shape[0]} dof {c['D']} {'grid' if c['exact'] else 'continuous'}"


def generate(n_cases, seed):
    rng = np.random.default_rng(seed)
    for case in range(n_cases):
        yield case, draw_steer_case(rng, case), draw_knn_case(rng, case)


def main():
    import torch

    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    dev = torch.device("cuda:0")
    bad, worst = 0, 0.0
    checkers = {}
    for case, sc, kc in generate(n_cases, seed):
        try:
            ref = steer_reference(sc)
            key = (sc["robot"], sc["scene"])
            if key not in checkers:
                checkers[key] = gc.build_checker(dev, *key)
            D = sc["weight"].shape[0]
            node, idx, ms = gc.run_steer(checkers[key], sc, ld=None if sc["ld"] == D else sc["ld"])
            worst = max(worst, gc.check_steer(ref, node, idx, ms))
            flags = gc.run_points(checkers[key], sc["start"], ld=None if sc["ld"] == D else sc["ld"])
            worst = max(worst, gc.check_points(ref["start_state"], flags))
        except (AssertionError, ValueError) as ex:
            bad += 1
            print(f"FAILED case {case}: {describe_steer(sc)}: {str(ex)[:300]}")
        except RuntimeError as ex:  # a launch error: nothing more is started on this device
            print(f"FAILED case {case}: {describe_steer(sc)}: {str(ex)[:300]}\n{n_cases} cases, stopped at case {case}, {bad + 1} failed")
            sys.exit(1)
        try:
            gc.check_knn(kc, gc.run_knn(dev, kc))
        except (AssertionError, ValueError) as ex:
            bad += 1
            print(f"FAILED case {case}: {describe_knn(kc)}: {str(ex)[:300]}")
        except RuntimeError as ex:
            print(f"FAILED case {case}: {describe_knn(kc)}: {str(ex)[:300]}\n{n_cases} cases, stopped at case {case}, {bad + 1} failed")
            sys.exit(1)
    print(f"{n_cases} cases, {bad} failed  (largest undecided share {100 * worst:.2f} %)")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
