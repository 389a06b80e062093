"""Records tests/golden/fused_parent_bits.npz: the bits the three launches on the device machinery of csrc/fused_device.hpp give
on fixed inputs -- the fused trajectory rollout (csrc/rollout_fused.hip, csrc/rollout_fused_shape.hip), the one-launch IK rollout
(csrc/rollout_ik_fused.hip) and the PRM planner's steering (csrc/graph_planner.hip) -- for tests/test_gpu_fused_parent_bits.py to
hold a later build to:

    python tests/golden/make_fused_parent_bits.py            (needs the GPU; rewrites the fixture)

The parity tests hold these kernels to the kernel sequence and to the oracle inside bounds, which a changed rounding or a changed
tie rule passes; this fixture does not let it pass.  It is recorded from the build whose arithmetic is to be kept; a change that
alters arithmetic on purpose re-records it with this script and says so.  ``replay`` uses only curobo_amd: the robots are the
packaged ones, knots, start configurations and the C1 / C2 / C3 / C5 worlds come from curobo_amd.workloads with fixed seeds,
joint configurations, goals and edges from numpy generators with fixed seeds.  What is not reproducible that way -- the world of
analytic primitives (tests/test_scene_primitives.py), the 37-cuboid world and the cuboid + ESDF-grid world of tests/test_gpu_fused.py
-- is built by ``inputs()`` (record time only) and stored in the file under "in/...".  ``replay(inputs)`` runs every case of
``cases()`` and returns every output word as int32 (cost, knot or joint gradient; for steering the node, the step index, the
step count and the feasibility bytes), stored under "out/...".  ``load()`` gives both back.

The first word of a case's name is its launch (traj, ik, steer).  Trajectory cases: Franka, 24 trajectories, knots scaled by 1.6
(the arm pushed into itself); "lane" = the lane-dealt pair lists, "row" = the same launch with the lists taken off the pair tensor.

The script refuses to write a file unless (``check``): the leftover points of every trajectory case are what its name says (from
curobo_hip_rollout_fused_threads and the padded horizon: "left1" one, "left0" none, "leftn" between 2 and a quarter of the
rows); more than 0.3 of the trajectories of the self-only cases cost something, and the scene changes the cost of the others;
the many-obstacle world has more than 32 records, the voxel world a grid, the primitive world its tag, the TERMS case the fused
path; each IK case holds configurations in self collision, in scene collision and in neither (read off the kernel sequence's
per-term buffers); the steered edges hold one that stops early from a feasible start, one that reaches its end and one whose
start is infeasible; the point-mode batch holds both feasibility values; two replays in this process and one in a fresh process
agree word for word."""
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fused_parent_bits.npz")
DEV = "cuda:0"
SCALE = 1.6  # knots of the trajectory cases: pushes the arm into itself
THR = 0.005  # steering: c-space similarity threshold
H31 = dict(n_knots=10, interpolation_steps=2, bspline_degree=4)  # padded horizon 31 on 32 rows: no leftover point
H67 = dict(n_knots=18, interpolation_steps=3, bspline_degree=3)  # padded horizon 67 on 64 rows: three leftover points
SELF = dict(use_scene_collision=False)
DISCRETE = dict(use_sweep=False, use_speed_metric=False)


def cases():
    """(name, kind, world, options); kinds: traj (CollisionRollout), terms (TrajOptRollout), ik, steer, points"""
    out = []
    for form in ("lane", "row"):
        row = dict(rows=form == "row")
        out += [(f"traj_left1_{form}_self", "traj", None, dict(SELF, **row)), (f"traj_left1_{form}_scene", "traj", "c2", dict(row)),
                (f"traj_left0_{form}_self", "traj", None, dict(SELF, **H31, **row)), (f"traj_left0_{form}_scene", "traj", "c2", dict(H31, **row)),
                (f"traj_leftn_{form}_self", "traj", None, dict(SELF, **H67, **row)), (f"traj_leftn_{form}_scene", "traj", "c2", dict(H67, **row))]
    out += [("traj_left1_generic", "traj", "c2", dict(generic=True)),  # the same launch without the compile-time shapes
            ("traj_left1_rowpass", "traj", "many", dict(DISCRETE)), ("traj_left1_voxel", "traj", "voxel", {}),
            ("traj_left1_prim", "traj", "prim", {}), ("traj_left1_terms", "terms", "c1", {})]
    out += [("ik_cuboid", "ik", "c1", {}), ("ik_voxel", "ik", "voxel", {}), ("ik_grid", "ik", "c3", {}), ("ik_envs", "ik", "c5", dict(envs=2))]
    out += [("steer_edges", "steer", "c2", {}), ("steer_points", "points", "c2", {})]
    return out


def inputs():
    sys.path.insert(0, os.path.dirname(HERE))
    from test_scene_primitives import PRIM_WORLD

    from curobo_amd.scene import cuboid_scene_arrays, voxel_grid_from_sdf
    from curobo_amd.workloads import c2_world

    def stored(key, arrays):  # the numeric arrays of a world (names stay behind: nothing reads them)
        return {f"{key}/{k}": np.asarray(v) for k, v in arrays.items() if np.asarray(v).dtype.kind in "fiub"}

    d = stored("prim", cuboid_scene_arrays(PRIM_WORLD))
    rng = np.random.default_rng(4)  # (tests/test_gpu_fused.py::test_fused_many_obstacles_uses_the_row_pass)
    world = c2_world()[0]
    for _ in range(33):
        p = rng.uniform([-0.6, -0.6, 0.1], [0.7, 0.7, 0.9])
        world.append({"dims": rng.uniform(0.04, 0.12, 3).tolist(), "pose": [*p.tolist(), 1, 0, 0, 0]})
    d.update(stored("many", cuboid_scene_arrays([world])))
    grid = voxel_grid_from_sdf(lambda p: np.linalg.norm(p - np.array([0.35, -0.3, 0.5]), axis=-1) - 0.18, (40, 40, 40), 0.04,
                               pose7=(0.1, -0.1, 0.5, 1, 0, 0, 0), max_distance=100.0)  # (tests/test_gpu_fused.py::_pair(voxel=True))
    d.update(stored("voxel", {**cuboid_scene_arrays(c2_world()), **grid}))
    return d


def _scene(d, world, cache):
    from curobo_amd.scene import SceneData, cuboid_scene_arrays
    from curobo_amd.workloads import c1_world, c2_world, c3_voxel_world, c5_mixed_worlds

    if world is not None and world not in cache:
        arrays = {"c1": lambda: cuboid_scene_arrays(c1_world()), "c2": lambda: cuboid_scene_arrays(c2_world()),
                  "c3": lambda: c3_voxel_world(64, 0.04), "c5": lambda: c5_mixed_worlds(2, grid=32)}.get(
                      world, lambda: {k.split("/", 1)[1]: (v if v.ndim else float(v)) for k, v in d.items() if k.startswith(world + "/")})()
        cache[world] = SceneData.from_arrays(arrays, DEV)
    return cache.get(world)


def _sample_q(model, n, seed, scale):
    rng = np.random.default_rng(seed)
    lo, hi = model.joint_limits_position
    return (0.5 * (lo + hi) + 0.5 * (hi - lo) * scale * rng.uniform(-1, 1, size=(n, model.num_dof))).astype(np.float32)


def _goals(n, T, seed):
    rng = np.random.default_rng(seed)
    pos = rng.normal(size=(n, T, 1, 3)).astype(np.float32) * 0.4
    quat = rng.normal(size=(n, T, 1, 4)).astype(np.float32)
    return torch.as_tensor(pos, device=DEV), torch.as_tensor(quat / np.linalg.norm(quat, axis=-1, keepdims=True), device=DEV)


def _edges(model, n=32):
    """short edges; four that leave the joint limits; one whose start is outside them; one long edge that sets the step count"""
    rng = np.random.default_rng(7)
    lo, hi = [np.asarray(v, np.float32) for v in model.joint_limits_position]
    s = (lo + (hi - lo) * rng.uniform(0.1, 0.9, size=(n, model.num_dof))).astype(np.float32)
    t = (s + 0.1 * ((lo + (hi - lo) * rng.uniform(0.1, 0.9, size=s.shape)).astype(np.float32) - s)).astype(np.float32)
    t[:4] = s[:4] + 0.3 * (hi - lo)
    s[4] = hi + 0.01
    s[5], t[5] = lo + 0.3 * (hi - lo), lo + 0.6 * (hi - lo)
    return np.ascontiguousarray(s), np.ascontiguousarray(t)


def _ik_rollout(model, kin, scene, opt, fused):
    import dataclasses

    from curobo_amd.rollout.ik_rollout import IKRollout, IKRolloutCfg

    B, n_env = 64, opt.get("envs", 1)
    if n_env > 1:  # per-environment sphere sets, as tests/test_gpu_ik.py::test_ik_fused_multi_env_equals_kernel_sequence has them
        sph = kin.link_spheres.repeat(n_env, 1, 1).clone()
        sph[1, :, 3] = torch.where(sph[1, :, 3] > 0, sph[1, :, 3] * 1.3, sph[1, :, 3])
        kin = dataclasses.replace(kin, link_spheres=sph.contiguous())
    ro = IKRollout(kin, scene, B, IKRolloutCfg(use_fused=fused), num_goalset=1)
    gpos, gquat = _goals(4, kin.num_pose_links, seed=9)
    ro.update_goals(gpos, gquat, torch.as_tensor(np.arange(B, dtype=np.int32) % 4, device=DEV))
    if n_env > 1:
        ro.update_env_query_idx(torch.arange(n_env, dtype=torch.int32, device=DEV).repeat_interleave(B // n_env))  # runs of 32
    return ro, torch.as_tensor(_sample_q(model, B, seed=5, scale=1.05), device=DEV)


def replay(d, probe=None):
    """every case on the inputs ``d`` -> {name: int32 array}; ``probe`` (record time) collects what ``check`` looks at"""
    from curobo_amd.backends import rollout as rollout_hip
    from curobo_amd.collision_checking import RobotCollisionChecker
    from curobo_amd.graph_planner.prm import GraphFeasibility
    from curobo_amd.kinematics import KinematicsCfg
    from curobo_amd.robot import load_packaged_robot
    from curobo_amd.robot.kinematics_params import KinematicsParams
    from curobo_amd.rollout import CollisionRollout, CollisionRolloutCfg, TrajOptRollout, TrajOptRolloutCfg
    from curobo_amd.workloads import seed_knots, start_configuration

    bits = lambda t: t.detach().cpu().contiguous().numpy().view(np.int32).copy()  # noqa: E731
    model = load_packaged_robot("franka")
    kin = KinematicsParams.from_model(model, DEV)
    start = torch.as_tensor(start_configuration(model), device=DEV)
    pairs = kin.self_collision.collision_pairs
    lanes = pairs._self_lane_lists
    scenes, out = {}, {}
    probe = {} if probe is None else probe
    for name, kind, world, opt in cases():
        scene = _scene(d, world, scenes)
        if kind == "traj":
            B = 24
            cfg = CollisionRolloutCfg(**{k: v for k, v in opt.items() if k not in ("rows", "generic")})
            ro = CollisionRollout(kin, scene, B, cfg)
            ro.update_start_state(start)
            x = torch.as_tensor(seed_knots(model, B, cfg.n_knots, seed=11), device=DEV).reshape(B, -1) * SCALE
            assert ro.fused_available()
            try:
                if opt.get("rows"):
                    del pairs._self_lane_lists
                rollout_hip.set_fused_shapes_enabled(not opt.get("generic"))
                cost, grad = ro.cost_and_gradient(x)
                torch.cuda.synchronize()
            finally:
                pairs._self_lane_lists = lanes
                rollout_hip.set_fused_shapes_enabled(True)
            out[f"{name}_cost"], out[f"{name}_grad"] = bits(cost), bits(grad)
            probe[name] = dict(H=cfg.padded_horizon, records=rollout_hip_slots(scene), scene=scene,
                               lane_code=0 if opt.get("rows") else lanes[1], kin=kin, terms=0)
        elif kind == "terms":  # (tests/test_gpu_trajopt.py::test_trajopt_fused_equals_kernel_sequence's shape)
            B = 12
            ro = TrajOptRollout(kin, scene, B, TrajOptRolloutCfg(traj_dt=0.1))
            ro.update_start_state(start)
            gpos, gquat = _goals(3, 1, seed=2)
            ro.update_goals(gpos, gquat, torch.as_tensor(np.arange(B, dtype=np.int32) % 3, device=DEV))
            x = torch.as_tensor(seed_knots(model, B, 12, seed=8, spread=0.6), device=DEV).reshape(B, -1)
            assert ro.fused_available()
            cost, grad = ro.cost_and_gradient(x)
            torch.cuda.synchronize()
            out[f"{name}_cost"], out[f"{name}_grad"] = bits(cost), bits(grad)
            probe[name] = dict(H=ro.cfg.padded_horizon, records=rollout_hip_slots(scene), scene=scene, lane_code=lanes[1], kin=kin, terms=1,
                               fused=bool(ro.cfg.use_fused and ro._fused_chosen()))
        elif kind == "ik":
            ro, q = _ik_rollout(model, kin, scene, opt, True)
            assert ro.fused_available() and ro._env_runs_ok
            cost, grad = ro.cost_and_gradient(q)
            torch.cuda.synchronize()
            out[f"{name}_cost"], out[f"{name}_grad"] = bits(cost), bits(grad)
            probe[name] = dict(model=model, kin=kin, scene=scene, opt=opt)
        else:
            checker = RobotCollisionChecker(KinematicsCfg(kin, model), scene, 0.0)
            feas = GraphFeasibility(checker, THR, torch.ones(kin.num_dof, device=DEV), 4096)
            assert feas.uses_fused()
            if kind == "steer":
                s, t = [torch.as_tensor(v, device=DEV) for v in _edges(model)]
                node, idx = feas.steer(s, t)
                torch.cuda.synchronize()
                out[f"{name}_node"], out[f"{name}_index"], out[f"{name}_steps"] = bits(node), bits(idx), bits(feas._ws)
                out[f"{name}_start_feasible"] = feas.feasible(s).cpu().numpy().astype(np.int32)
            else:  # 40 configurations: two full workgroups and a ragged one
                ok = feas.feasible(torch.as_tensor(_sample_q(model, 40, seed=3, scale=1.0), device=DEV))
                out[f"{name}_feasible"] = ok.cpu().numpy().astype(np.int32)
    return out


def rollout_hip_slots(scene):
    from curobo_amd.rollout.base import obstacle_slots

    return obstacle_slots(scene)


def check(recorded, probe):
    """the conditions on the fixture (module docstring); prints what every case reaches"""
    from curobo_amd import _lib

    lib, broken = _lib.load(), []
    f32 = lambda k: recorded[k].view(np.float32)  # noqa: E731
    for name, kind, world, opt in cases():
        p = probe.get(name, {})
        if kind in ("traj", "terms"):
            k = p["kin"]
            threads = int(lib.curobo_hip_rollout_fused_threads(p["H"], k.num_dof, k.num_links, k.num_spheres,
                                                               int(k.self_collision.collision_pairs.shape[0]),
                                                               int(k.link_chain_data.shape[0]), int(p["lane_code"]), int(p["records"]), p["terms"]))
            rows = threads // 16
            left = p["H"] % rows
            if left * 4 > rows or p["H"] < rows:
                left = 0
            cost = f32(f"{name}_cost")
            ok = {"left1": left == 1, "left0": left == 0 and p["H"] <= rows, "leftn": 2 <= left <= rows // 4}[name.split("_")[1]]
            if name.endswith("_self"):
                ok = ok and float((cost > 0).mean()) > 0.3
            elif name.endswith("_scene"):
                ok = ok and float((cost != f32(name[:-6] + "_self_cost")).mean()) > 0.3
            if name.endswith("rowpass"):
                ok = ok and p["records"] > 32
            if name.endswith("voxel"):
                ok = ok and p["scene"].struct.max_voxel_grids > 0 and p["scene"].struct.max_cuboids > 0
            if name.endswith("prim"):
                ok = ok and bool(p["scene"].struct.cuboid_has_primitives)
            if kind == "terms":
                ok = ok and p["fused"]
            print(f"{name}: padded horizon {p['H']}, {threads} threads, {left} leftover point(s), {p['records']} records, "
                  f"{int((cost > 0).sum())} of {cost.size} trajectories cost something, all finite {bool(np.isfinite(cost).all())}")
            ok = ok and bool(np.isfinite(cost).all()) and bool(np.isfinite(f32(f"{name}_grad")).all())
        elif kind == "ik":  # the kernel sequence's per-term buffers say which configuration is in which collision
            ro, q = _ik_rollout(p["model"], p["kin"], p["scene"], p["opt"], False)
            ro.cost_and_gradient(q)
            torch.cuda.synchronize()
            in_self = (ro.self_dist.reshape(q.shape[0], -1) > 0).any(1).cpu().numpy()
            in_scene = (ro.scene_dist.reshape(q.shape[0], -1) > 0).any(1).cpu().numpy()
            print(f"{name}: {q.shape[0]} configurations, {int(in_self.sum())} in self collision, {int(in_scene.sum())} in scene collision, "
                  f"{int((~in_self & ~in_scene).sum())} in neither")
            ok = in_self.any() and in_scene.any() and (~in_self & ~in_scene).any() and bool(np.isfinite(f32(f"{name}_cost")).all())
            if p["opt"].get("envs", 1) > 1:
                ok = ok and ro.use_multi_env and ro.kin.num_envs > 1
        elif kind == "steer":
            idx, steps, free = recorded[f"{name}_index"], int(recorded[f"{name}_steps"][0]), recorded[f"{name}_start_feasible"] != 0
            early, end, blocked = int(((idx < steps) & free).sum()), int((idx == steps).sum()), int((~free).sum())
            print(f"{name}: {idx.size} edges of {steps} steps: {early} stop early from a feasible start, {end} reach their end, "
                  f"{blocked} start infeasible")
            ok = idx.size == 32 and early > 0 and end > 0 and blocked > 0 and bool((idx[~free] == 0).all())
        else:
            ok_flags = recorded[f"{name}_feasible"]
            print(f"{name}: {ok_flags.size} configurations, {int(ok_flags.sum())} feasible")
            ok = ok_flags.size == 40 and 0 < int(ok_flags.sum()) < 40
        if not ok:
            broken.append(name)
    assert not broken, f"cases that break the fixture's conditions: {broken}"


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
    recorded = replay(given, probe)
    assert all(v.dtype == np.int32 for v in recorded.values())
    check(recorded, probe)
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
    assert os.path.getsize(target) <= 256 * 1024, os.path.getsize(target)  # (the mesh fixture's size: these outputs are a few thousand words)
    print(f"{target}: {len(given)} inputs, {len(recorded)} outputs, {sum(v.size for v in recorded.values())} words, {os.path.getsize(target)} bytes")
