"""Time the link-pair sweep against the only other way to its numbers: ``self_collision_distance(store_pair_distance=True)``
followed by a grouped maximum over ``pair_distance.view(N, P)`` in torch.  Unitree G1, all candidate link pairs.

    python tools/link_pair_sweep_timing.py [--robot unitree_g1] [--batch 1024] [--repeat 20] [--out profiles/link_pair_sweep_timing.jsonl]

Device events around each path, the two paths alternating inside one process after a warm-up of both; one JSON line per path with
the median / min / max time and the bytes each moves through global memory (computed from the shapes)."""

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="unitree_g1")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing on the CPU says nothing"
    from curobo_amd.backends import geometry as G
    from curobo_amd.kinematics import Kinematics, KinematicsCfg
    from curobo_amd.robot.collision_matrix import candidate_link_pairs

    dev = torch.device("cuda:0")
    kin = Kinematics(KinematicsCfg.from_packaged(a.robot, device=dev))
    model = kin.config.model
    link_pairs, locs, grp = candidate_link_pairs(model)
    n_groups, P, S, N = len(link_pairs), len(locs), model.num_spheres, a.batch
    rng = np.random.default_rng(3)
    lo, hi = model.joint_limits_position
    q = torch.as_tensor((lo + (hi - lo) * rng.uniform(size=(N, model.num_dof))).astype(np.float32), device=dev)
    sph = kin.compute_kinematics(q).robot_spheres.reshape(N, 1, S, 4).clone()
    pad = kin.kinematics_config.self_collision.sphere_padding
    d_locs, d_grp = torch.as_tensor(locs, device=dev), torch.as_tensor(grp, device=dev)
    mx = torch.empty(n_groups, device=dev)
    cnt = torch.empty(n_groups, dtype=torch.int32, device=dev)

    def sweep():
        G.link_pair_sweep(mx, cnt, sph, pad, d_locs, d_grp, n_groups)

    out_d = torch.zeros(N, 1, device=dev)
    out_g = torch.zeros(N, S, 4, device=dev)
    flags = torch.zeros(N, S, dtype=torch.uint8, device=dev)
    pd = torch.zeros(N, P, device=dev)
    w = torch.ones(1, device=dev)
    z1, z2 = torch.zeros(1, device=dev), torch.zeros(2, dtype=torch.int16, device=dev)
    index = d_grp.to(torch.int64).view(1, P).expand(N, P)
    base = {}

    def store_kernel():
        G.self_collision_distance(out_d, out_g, pd, flags, sph, pad, w, d_locs, z1, z2, 1, 256, N, 1, S, P, True, False)

    def grouped():
        point = torch.full((N, n_groups), float("-inf"), device=dev).scatter_reduce_(1, index, pd.view(N, P), "amax", include_self=True)
        base["max"], base["cnt"] = point.amax(0), (point > 0).sum(0)

    def baseline():
        store_kernel()
        grouped()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    paths = {"link_pair_sweep": sweep, "store_pair_distance+grouped_amax": baseline, "store_pair_distance kernel alone": store_kernel}
    for _ in range(3):
        for fn in paths.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(a.repeat):
        for k, fn in paths.items():
            times[k].append(timed(fn))
    # same decisions: the sign of the group maximum (the baseline's values are r^2 - d^2 with invalid pairs at 0, the sweep's are metres)
    agree = int(((mx > 0) == (base["max"] > 0)).sum())
    same_cnt = int((cnt == base["cnt"].to(torch.int32)).sum())
    chunks = -(-N // max(1, -(-N // G.SWEEP_TARGET_CHUNKS)))
    moved = {
        "link_pair_sweep": {"spheres_read": N * S * 16, "pair_table_read_per_point_through_L2": N * P * 8, "partials_written_and_read": 2 * chunks * n_groups * 8,
                            "result_written": n_groups * 8},
        "store_pair_distance+grouped_amax": {"spheres_read": N * S * 16, "pair_table_read": -(-N // 8) * P * 4, "pair_distance_written": N * P * 4,
                                             "pair_distance_read": N * P * 4, "group_index_read": N * P * 8, "point_max_written_and_read": 3 * N * n_groups * 4},
        "store_pair_distance kernel alone": {"spheres_read": N * S * 16, "pair_table_read": -(-N // 8) * P * 4, "pair_distance_written": N * P * 4},
    }
    lines = []
    for k, t in times.items():
        lines.append(json.dumps({"path": k, "robot": a.robot, "batch": N, "spheres": S, "pairs": P, "groups": n_groups, "repeat": a.repeat,
                                 "ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                                 "bytes": moved[k], "groups_with_the_same_sign": agree, "groups_with_the_same_count": same_cnt}))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
