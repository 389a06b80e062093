"""Planning with and without the PRM graph planner on identical seeded problems, and the fused steering launch against the
materialised path.

    python tools/planner_graph_seeding.py plan [--problems 40] [--delta 0.5] [--robots dual_ur10e unitree_g1] [--out FILE]
    python tools/planner_graph_seeding.py steer [--edges 300] [--steps 400] [--reps 20] [--out FILE]

plan: the problems of tools/r06/planner_other_robots_fair.py ("planning on the reference's other two benchmark
robots"), generator restated in ``make_problems``: after the planner's warmup, torch.manual_seed(3); 2n + 20 collision-free
configurations from ``sample_configs(rejection_ratio=50)`` in ``collision_table.yml``; starts = the first n, goals = the next
n; with ``--delta`` > 0 each goal is replaced by the first collision-free configuration among up to 200 batches of 64 draws
``start + U(-delta, delta)`` per joint (clamped 0.01 inside the limits).  delta 0.5 = the "near-start" set, 0 = the
across-joint-range set.  Two planners plan the same problems with ``plan_pose`` and its default attempts (5):
``use_graph_planner=False`` and ``True`` (roadmap seeds from the second attempt on, ``enable_graph_attempt=1``, the
reference's default).  One JSON line per problem while it runs, then one per (robot, delta, roadmap) with the success
percentage and the plan times of the solved problems.

steer: Franka in the C2 cuboid world, ``--edges`` edges from Halton samples whose batch-wide step count is ``--steps``.
Times the fused launch (``curobo_hip_graph_steer``) and the materialised path (every point interpolated, then
``RobotCollisionChecker.validate`` in chunks of 2000 points) with hip events, and checks both return the same indices.
Per-kernel times come from running this mode under rocprofv3 in a process of its own:
    rocprofv3 --kernel-trace --stats -d OUT -o steer -- python tools/planner_graph_seeding.py steer
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def make_problems(planner, n: int, delta: float):
    """tools/r06/planner_other_robots_fair.py's generator: the same calls in the same order, so the same random stream"""
    torch.manual_seed(3)
    q = planner.sample_configs(2 * n + 20, rejection_ratio=50)
    assert q.shape[0] >= 2 * n, q.shape
    starts, goals = q[:n], q[n:2 * n].clone()
    if delta > 0:
        chk = planner.trajopt_solver._sample_checker[1]
        lo, hi = planner.kinematics.kinematics_config.joint_limits_position
        # (that tool first counted how many unchecked draws collide: the same draw is made here to keep the stream)
        torch.rand(n, q.shape[1], device=q.device)
        for i in range(n):
            for _ in range(200):
                g = torch.minimum(torch.maximum(starts[i:i + 1] + delta * (2 * torch.rand(64, q.shape[1], device=q.device) - 1), lo + 0.01),
                                  hi - 0.01)
                ok = chk.validate(g.unsqueeze(1)).view(-1)
                if bool(ok.any()):
                    goals[i] = g[ok][0]
                    break
            else:
                raise RuntimeError(f"no collision-free goal near start {i}")
    return starts, goals


def plan(args):
    from curobo_amd.motion_planner import MotionPlanner, MotionPlannerCfg
    from curobo_amd.types import JointState

    for robot in args.robots:
        base = MotionPlanner(MotionPlannerCfg.create(robot=f"{robot}.yml", scene_model="collision_table.yml"))
        base.warmup()
        starts, goals = make_problems(base, args.problems, args.delta)
        graph = MotionPlanner(MotionPlannerCfg.create(robot=f"{robot}.yml", scene_model="collision_table.yml", use_graph_planner=True))
        graph.warmup()
        for name, planner in (("no_roadmap", base), ("roadmap", graph)):
            planner.reset_seed()
            ok, ms = 0, []
            for i in range(args.problems):
                cur = JointState.from_position(starts[i:i + 1].clone(), planner.joint_names)
                goal = planner.compute_kinematics(JointState.from_position(goals[i:i + 1].clone(), planner.joint_names)).tool_poses.as_goal()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = planner.plan_pose(goal, cur)
                torch.cuda.synchronize()
                dt = 1e3 * (time.perf_counter() - t0)
                good = r is not None and bool(r.success.any())
                ok += good
                if good:
                    ms.append(dt)
                gp = planner.graph_planner
                print(json.dumps({"robot": robot, "delta": args.delta, "mode": name, "problem": i, "success": good, "ms": round(dt, 2),
                                  "roadmap_nodes": gp.n_nodes if gp is not None else None}), flush=True)
            emit({"robot": robot, "dof": planner.action_dim, "problems": args.problems, "goal_delta": args.delta, "mode": name,
                  "success_percent": 100.0 * ok / args.problems, "plan_ms_median": float(np.median(ms)) if ms else None,
                  "plan_ms_max": float(np.max(ms)) if ms else None,
                  "fused_steering": planner.graph_planner.feasibility.uses_fused() if planner.graph_planner is not None else None}, args.out)


def steer(args):
    from curobo_amd.collision_checking import RobotCollisionChecker
    from curobo_amd.graph_planner.prm import GraphFeasibility, last_feasible_index, steer_num_steps, steer_points
    from curobo_amd.kinematics import KinematicsCfg
    from curobo_amd.scene import SceneData, cuboid_scene_arrays
    from curobo_amd.solver.seed_ik import HaltonSeeds
    from curobo_amd.workloads import c2_world

    dev = torch.device("cuda:0")
    thr = 0.005
    checker = RobotCollisionChecker(KinematicsCfg.from_packaged("franka", device=dev),
                                    SceneData.from_arrays(cuboid_scene_arrays(c2_world()), dev), 0.0)
    lim = checker.kinematics.kinematics_config.joint_limits_position
    lo, hi = lim[0].contiguous(), lim[1].contiguous()
    D = lo.numel()
    hs = HaltonSeeds(D, lo, hi, seed=5)
    s, t = hs.get_samples(args.edges), hs.get_samples(args.edges)
    d = t - s
    t = torch.minimum(torch.maximum(s + d / d.abs().max(1, keepdim=True).values.clamp_min(1e-6) * ((args.steps - 1) * thr), lo), hi)
    s, t = s.contiguous(), t.contiguous()
    w = torch.ones(D, device=dev)
    feas = GraphFeasibility(checker, thr, w, 2000)
    n_steps = int(steer_num_steps(s, t, w, thr).max().item())

    def fused():
        return feas.steer(s, t)[1]

    def materialised():
        pts = steer_points(s, t, n_steps)
        return last_feasible_index(feas.validate_materialised(pts.reshape(-1, D)).view(args.edges, n_steps + 1))

    res = {}
    for name, fn in (("fused", fused), ("materialised", materialised)):
        out = fn()  # warm-up (allocations, first launches)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            out = fn()
        b.record()
        torch.cuda.synchronize()
        res[name] = (a.elapsed_time(b) / args.reps, out.long())
    idx = res["fused"][1]
    emit({"robot": "franka", "world": "c2", "edges": args.edges, "max_steps": n_steps, "points_materialised": args.edges * (n_steps + 1),
          "edges_feasible_to_the_end": int((idx == n_steps).sum()), "mean_last_feasible_index": float(idx.float().mean()),
          "fused_ms": round(res["fused"][0], 4), "materialised_ms": round(res["materialised"][0], 4), "reps": args.reps,
          "index_agreement": f"{int((idx == res['materialised'][1]).sum())}/{args.edges}"}, args.out)


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("mode", choices=("plan", "steer"))
    p.add_argument("--problems", type=int, default=40)
    p.add_argument("--delta", type=float, default=0.5)
    p.add_argument("--robots", nargs="*", default=["dual_ur10e", "unitree_g1"])
    p.add_argument("--edges", type=int, default=300)
    p.add_argument("--steps", type=int, default=400)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default="")
    a = p.parse_args()
    plan(a) if a.mode == "plan" else steer(a)
