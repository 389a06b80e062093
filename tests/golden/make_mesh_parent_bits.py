"""Records tests/golden/mesh_parent_bits.npz: the bits the mesh-obstacle launches (csrc/mesh_bvh.hip, csrc/mesh_device.hpp) give
on fixed inputs, for tests/test_gpu_mesh_parent_bits.py to hold a later build to:

    python tests/golden/make_mesh_parent_bits.py            (needs the GPU; rewrites the fixture)

The oracle holds these kernels inside bounds and the forms to each other "except on ties", so a changed rounding passes them;
this fixture does not let it pass.  It is recorded from the build whose arithmetic is to be kept; a change that alters
arithmetic on purpose re-records it with this script and says so.  ``replay`` uses only curobo_amd.backends.mesh and
curobo_amd.scene; ``inputs()`` (record time only) takes the worlds and trajectories of the mesh tests (tests/test_oracle_mesh.py,
tests/test_gpu_mesh.py) and stores them in the file under "in/...".  ``replay(inputs)`` runs every case of ``cases()`` and returns
every output word (distance, gradient) as int32 and, for the queued forms, the four counter words of the launch's workspace
(stored under "out/..."; an output equal to an earlier one is stored once: "same" lists such names with the earlier one's).
``load()`` gives both back in full.

The forms: "one" = the one-kernel launch (no workspace), "walk" = the queued launch over meshes without cell lists (select +
tree walk), "cells" = the queued launch over meshes with their default cell lists (select + cell lists + workgroup per sphere +
tree walk of the rest).  A case's tag is sweep steps, speed metric, accumulate.

The script refuses to write a file unless: every queued case has live spheres (counter words 0 + 2 > 0); the ball cases send
more than 10 spheres to the workgroup-per-sphere kernel (word 3); the open-mesh cases hand spheres to the tree walk (word 1);
the cell-list cases of the mesh world hand (next to) none on (word 1 <= 2, as tests/test_gpu_mesh.py asserts, and words 1 + 3
at most a twentieth of the live ones); every case has spheres in penetration and -- except in the ball cases, whose spheres
all lie inside the ball as that test has them -- spheres that are not; two replays in this process and one in a fresh process
agree word for word."""
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "mesh_parent_bits.npz")
DEV = "cuda:0"
WEIGHT, ETA, SPEED_DT = 3.0, 0.02, 0.05
DIST0, GRAD0 = 0.25, 0.5  # what the output buffers hold before a launch
CELLS = {"one": None, "walk": False, "cells": None}  # MeshStore(cells=) of a form
TAGS = ((0, 0, 0), (3, 0, 0), (3, 1, 0), (3, 1, 1))  # (sweep steps, speed metric, accumulate)


def cases():
    """(name, world, spheres, form, (sweep, speed, accumulate), gradient_mode); the first word of a name is its group"""
    out = []
    for form in ("one", "walk", "cells"):
        out += [(f"world_{form}_{s}{v}{a}", "world", "traj6", form, (s, v, a), 0) for s, v, a in TAGS]
    out += [(f"ball_cells_{s}{v}0", "ball", "ball", "cells", (s, v, 0), 0) for s, v in ((0, 0), (3, 1))]
    out += [(f"open_cells_{s}00", "open", "open", "cells", (s, 0, 0), 0) for s in (0, 3)]
    # horizon 1: 128 trajectories x 3 slots per select workgroup, read per sphere; horizon 2: 23 x 3, staged in LDS
    out += [(f"env_{form}_h{h}", "envs", f"env_h{h}", form, (3 if h > 1 else 0, 0, 0), 0) for form in ("one", "cells") for h in (1, 2)]
    out += [(f"slots_cells_{s}00", "slots40", "traj4", "cells", (s, 0, 0), 0) for s in (0, 3)]
    out += [(f"gm_{form}_310", "world", "traj6", form, (3, 1, 0), 1) for form in ("walk", "cells")]
    return out


def _pack_world(d, key, envs):
    """a world as arrays: its distinct meshes, and per (environment, slot) mesh index, pose, enable"""
    names, n = [], max(len(e) for e in envs)
    mesh = np.full((len(envs), n), -1, np.int32)
    pose, enable = np.zeros((len(envs), n, 7), np.float32), np.zeros((len(envs), n), np.uint8)
    for e, obs in enumerate(envs):
        for i, o in enumerate(obs):
            name = o.get("mesh_name", o["name"])
            if name not in names:
                names.append(name)
                d[f"{key}_v{len(names) - 1}"], d[f"{key}_f{len(names) - 1}"] = np.asarray(o["vertices"], np.float32), np.asarray(o["faces"], np.int32)
            mesh[e, i], pose[e, i], enable[e, i] = names.index(name), o["pose"], o.get("enable", True)
    d[f"{key}_mesh"], d[f"{key}_pose"], d[f"{key}_enable"] = mesh, pose, enable


def _unpack_world(d, key):
    mesh = d[f"{key}_mesh"]
    return [[{"name": f"o{e}_{i}", "mesh_name": f"m{mesh[e, i]}", "vertices": d[f"{key}_v{mesh[e, i]}"], "faces": d[f"{key}_f{mesh[e, i]}"],
              "pose": [float(x) for x in d[f"{key}_pose"][e, i]], "enable": bool(d[f"{key}_enable"][e, i])}
             for i in range(mesh.shape[1]) if mesh[e, i] >= 0] for e in range(mesh.shape[0])]


def inputs():
    sys.path.insert(0, os.path.dirname(HERE))
    from conftest import load_model, sample_q
    from oracle import load_oracle
    from test_oracle_mesh import box_shape, mesh_world, sphere_shape
    from test_oracle_mesh_sign import without_faces_facing

    oracle, model = load_oracle(), load_model("franka")

    def trajectories(b, h, scale, span=1.0):  # (tests/test_gpu_mesh.py::_trajectory_spheres; span: the part of the way that is gone)
        q0, q1 = sample_q(model, b, seed=11)[:, None], sample_q(model, b, seed=12)[:, None]
        tt = np.linspace(0, span, h, dtype=np.float32)[None, :, None]
        sph = oracle.kinematics_forward((q0 * (1 - tt) + q1 * tt).reshape(b * h, -1) * scale, model.as_dict(), horizon=h)["robot_spheres"]
        return np.ascontiguousarray(sph.reshape(b, h, -1, 4), np.float32)

    d = {}
    w0 = mesh_world()[0]
    _pack_world(d, "world", [w0])
    d["sph_traj6"] = trajectories(6, 5, 0.5, 0.4)  # 1 950 spheres: two select workgroups, the last one ragged; steps of centimetres
    # ---- test_spheres_in_the_middle_of_a_ball_get_a_workgroup_each
    vs, fs = sphere_shape(0.2, 32, 64)
    _pack_world(d, "ball", [[{"name": "ball", "vertices": vs, "faces": fs, "pose": [0.1, -0.2, 0.3, 0.9238795, 0, 0.3826834, 0]}]])
    rng = np.random.default_rng(5)
    b, h, S = 6, 5, 16
    sph = np.zeros((b, h, S, 4), np.float32)
    sph[..., :3] = np.array([0.1, -0.2, 0.3], np.float32) + rng.normal(size=(b, 1, S, 3)).astype(np.float32) * np.array([0.004, 0.004, 0.06], np.float32)
    sph[..., :3] += (np.arange(h, dtype=np.float32)[None, :, None, None] - 2) * rng.normal(size=(b, 1, S, 3)).astype(np.float32) * 0.01
    sph[..., 3] = 0.03
    d["sph_ball"] = sph
    # ---- an open box (signed by the reference's rays), test_open_and_flipped_meshes_take_the_reference_ray_sign
    vb, fb = box_shape([0.3, 0.5, 0.2], 2)
    v, f = without_faces_facing(vb, fb, [0, 0, 1])
    _pack_world(d, "open", [[{"name": "m", "vertices": v, "faces": f, "pose": [0.05, -0.02, 0.3, 0.9659258, 0, 0.2588190, 0]}]])
    rng = np.random.default_rng(11)
    sph = np.concatenate([rng.uniform([-0.3, -0.4, 0.0], [0.4, 0.4, 0.6], size=(1500, 3)), rng.uniform(0.01, 0.05, size=(1500, 1))], 1)
    d["sph_open"] = sph.astype(np.float32).reshape(2, 5, 150, 4)
    # ---- two environments, an environment index per trajectory, horizon 1 and 2
    _pack_world(d, "envs", [[w0[0], w0[1]], [dict(w0[2]), dict(w0[3]), dict(w0[1], name="ball_b", mesh_name="ball")]])
    d["sph_env_h1"] = np.ascontiguousarray(trajectories(250, 1, 0.7)[:, :, 20:28])
    d["sph_env_h2"] = np.ascontiguousarray(trajectories(40, 2, 0.7)[:, :, 20:44])
    # ---- test_more_than_thirty_two_mesh_slots_run_as_slot_groups
    v, f = box_shape([0.08, 0.08, 0.08], 1)
    rng = np.random.default_rng(4)
    _pack_world(d, "slots40", [[{"name": f"cube{i}", "mesh_name": "cube", "vertices": v, "faces": f,
                                 "pose": [float(x) for x in rng.uniform([-0.6, -0.6, 0.1], [0.6, 0.6, 0.9])] + [1, 0, 0, 0], "enable": i % 7 != 3}
                                for i in range(40)]])
    d["sph_traj4"] = trajectories(4, 5, 0.5, 0.4)
    return d


def replay(d):
    """every case on the inputs ``d`` -> {name: int32 array}"""
    from curobo_amd.backends import mesh as M
    from curobo_amd.scene import MeshStore

    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV).contiguous()  # noqa: E731
    bits = lambda t: t.cpu().numpy().view(np.int32).copy()  # noqa: E731
    w, eta, dt = dev(np.float32([WEIGHT])), dev(np.float32([ETA])), dev(np.float32([SPEED_DT]))
    stores, out = {}, {}
    for name, world, spheres, form, (sweep, speed, accumulate), gradient_mode in cases():
        key = (world, form == "walk", gradient_mode)
        if key not in stores:
            stores[key] = MeshStore(_unpack_world(d, world), DEV, cells=CELLS[form], gradient_mode=gradient_mode)
        store = stores[key]
        sph = dev(d[f"sph_{spheres}"])
        b, h, S, _ = sph.shape
        multi = store.num_envs > 1
        idx = dev((np.arange(b) % store.num_envs).astype(np.int32)) if multi else None
        dist, grad = torch.full((b, h, S), DIST0, device=DEV), torch.full((b, h, S, 4), GRAD0, device=DEV)
        ws = False if form == "one" else torch.zeros(16 + 16 * b * h * S, dtype=torch.uint8, device=DEV)
        M.sphere_mesh_collision(dist, grad, sph, store.struct, w, eta, idx, b, h, S, multi, sweep, bool(speed), dt, accumulate=bool(accumulate),
                                workspace=ws)
        torch.cuda.synchronize()
        out[f"{name}_distance"], out[f"{name}_gradient"] = bits(dist), bits(grad)
        if form != "one":
            out[f"{name}_counters"] = bits(ws[:16].view(torch.int32))
    return out


def check(recorded):
    """the conditions on the fixture (module docstring); prints every case's counts"""
    broken = []
    for name, _, _, form, (_, _, accumulate), _ in cases():
        dist = recorded[f"{name}_distance"].view(np.float32)
        pen = int((dist > (DIST0 if accumulate else 0.0)).sum())
        cnt = recorded.get(f"{name}_counters")
        print(f"{name}: {dist.size} spheres, {pen} in penetration, counters {None if cnt is None else cnt.tolist()}")
        ok = pen > 0 and (pen < dist.size or name.startswith("ball_"))
        if cnt is not None:
            live = cnt[0] + cnt[2]
            ok = ok and live > 0 and (not name.startswith("ball_") or cnt[3] > 10) and (not name.startswith("open_") or cnt[1] > 0)
            if name.startswith("world_cells") or name.startswith("gm_cells"):
                ok = ok and cnt[1] <= 2 and live >= 20 * (cnt[1] + cnt[3])
        if not ok:
            broken.append(name)
    assert not broken, f"cases that break the fixture's conditions: {broken}"


def differing(got, want):
    return {k: int((got[k] != want[k]).sum()) if got[k].shape == want[k].shape else -1 for k in want if not np.array_equal(got.get(k), want[k])}


def pack(given, recorded):
    """the arrays of the file"""
    arrays, first, same = {f"in/{k}": v for k, v in given.items()}, {}, []
    for k, v in recorded.items():
        earlier = first.setdefault((v.shape, v.tobytes()), k)
        if earlier == k:
            arrays[f"out/{k}"] = v
        else:
            same.append((k, earlier))
    return dict(arrays, same=np.array(same).reshape(-1, 2))


def load(path=PATH):
    """(inputs, recorded outputs) of the file"""
    z = np.load(path)
    out = {k[4:]: z[k] for k in z.files if k.startswith("out/")}
    out.update({str(k): out[str(earlier)] for k, earlier in z["same"]})
    return {k[3:]: z[k] for k in z.files if k.startswith("in/")}, out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    if sys.argv[1:2] == ["--replay"]:  # the fresh process of the recorder: the file's inputs give the file's outputs
        given, recorded = load(sys.argv[2])
        diff = differing(replay(given), recorded)
        print(f"replay in a fresh process: differing {diff or 'none'}")
        sys.exit(1 if diff else 0)
    given = inputs()
    recorded = replay(given)
    check(recorded)
    diff = differing(replay(given), recorded)
    assert not diff, f"two replays in one process differ: {diff}"
    target = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(target + ".tmp.npz", **pack(given, recorded))
    try:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--replay", target + ".tmp.npz"], check=True, timeout=300)
        os.replace(target + ".tmp.npz", target)
    finally:
        if os.path.exists(target + ".tmp.npz"):
            os.remove(target + ".tmp.npz")
    assert os.path.getsize(target) <= 844 * 1024, os.path.getsize(target)  # (no larger than the largest golden: mppi_golden.npz)
    print(f"{target}: {len(given)} inputs, {len(recorded)} outputs, {sum(v.size for v in recorded.values())} words, {os.path.getsize(target)} bytes")
