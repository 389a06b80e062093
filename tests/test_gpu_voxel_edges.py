"""Voxel-grid scene collision on the device at the edges of the lookup (tests/voxel_cases.py): thin grids, every number of
valid corners, rotated poses, several grids per store, truncated and extreme values, sweeps across faces, the coarse cull
-- against the oracle (tests/sweep_allowance.py's bound, unchanged) and against the float64 restatement (tests/voxel_ref.py:
four times the oracle's own float32 gap, docs/ORACLE_PINS.md), in every kernel form the dispatcher has, which are bit-equal."""

import functools

import numpy as np
import pytest
import torch

import voxel_cases as VC
import voxel_ref as VR
from sweep_allowance import assert_scene_kernel_parity, device_frame_arithmetic

pytestmark = pytest.mark.gpu

CASE_NAMES = ["thin", "shell", "pose", "store_255", "store_256", "store_257", "store_333", "truncated_0.125", "truncated_0.1",
              "extremes", "sweep", "coarse", "step"]
FORMS = ("packed", "staged", "unstaged")
MODES = {"discrete": dict(sweep=False, enable_speed_metric=False), "swept": dict(sweep=True, enable_speed_metric=False),
         "speed": dict(sweep=True, enable_speed_metric=True)}
DT = 0.05


@functools.lru_cache(maxsize=None)
def _cases():
    cases = {c.name: c for c in VC.all_cases()}
    assert sorted(cases) == sorted(CASE_NAMES)
    return cases


def _family(name):
    return name.split("_")[0]


def _in_form(case, form, swept):
    """(arrays, spheres [B, H, S, 4], env [B] or None) that make the dispatcher take ``form``: packed = the case as it is;
    in-lane staged = at least 31 small cuboids 50 m away (more than 32 records); in-lane unstaged = one sphere per batch row (discrete)
    or as many far cuboids as push the staged records of a workgroup's batch rows past 32 KiB (swept: rows keep their horizon)"""
    arrays, sph, env = case.arrays, case.spheres, case.env
    b, h, s = sph.shape[:3]
    n_v = arrays["voxel_params"].shape[1]
    if form == "staged":
        arrays = VC.with_far_cuboids(arrays, max(31, 33 - n_v))  # (a store of one grid needs 32 of them to pass 32 records)
    elif form == "unstaged" and not swept:
        sph = sph.reshape(-1, 1, 1, 4)
        env = None if env is None else np.repeat(env, h * s).astype(np.int32)
        if n_v < 2:
            arrays = VC.with_far_cuboids(arrays, 1)
    elif form == "unstaged":
        slots = (256 + h * s - 1) // (h * s) + 1
        arrays = VC.with_far_cuboids(arrays, 32768 // (80 * slots) + 1 - n_v)
    return arrays, np.ascontiguousarray(sph), env


@functools.lru_cache(maxsize=None)
def _run(name, form, mode, coarse=True):
    """the kernel's (distance [B, H, S], gradient [B, H, S, 4]) in the case's own layout, computed once per session"""
    from curobo_amd.backends import collision as Cn
    from curobo_amd.scene import SceneData

    dev = torch.device("cuda:0")
    case = _cases()[name]
    kw = MODES[mode]
    arrays, sph, env = _in_form(case, form, kw["sweep"])
    scene = SceneData.from_arrays(arrays, dev, coarse_culling=coarse)
    assert (scene.struct.voxel_coarse_min is not None) == coarse
    b, h, s = sph.shape[:3]
    sweep_steps = 3 if kw["sweep"] else 0
    want = {"packed": Cn.SCENE_PACKED, "staged": Cn.SCENE_INLANE_STAGED, "unstaged": Cn.SCENE_INLANE}[form]
    assert Cn.scene_collision_form(scene.struct, b, h, s, sweep_steps) == want, (name, form, mode, (b, h, s))
    dist, grad = torch.full((b, h, s), 5.0, device=dev), torch.full((b, h, s, 4), 5.0, device=dev)
    Cn.sphere_obstacle_collision(dist, grad, torch.as_tensor(sph, device=dev), scene.struct, torch.tensor([case.weight], device=dev),
                                 torch.tensor([case.eta], device=dev), None if env is None else torch.as_tensor(env, device=dev), b, h, s,
                                 env is not None, sweep_steps, kw["enable_speed_metric"], torch.tensor([DT], device=dev))
    torch.cuda.synchronize()
    shape = case.spheres.shape[:3]
    return dist.cpu().numpy().reshape(shape), grad.cpu().numpy().reshape(*shape, 4)


def _oracle_kw(case, mode):
    return dict(**MODES[mode], speed_dt=DT, env_query_idx=case.env, use_multi_env=case.multi_env)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_parity(name, mode, oracle):
    """discrete, swept and swept with the speed metric.  The two families that are not 1-Lipschitz break the sweep cull's
    precondition: swept, a cull can only DROP samples the reference takes, so the kernel's cost is held
    from above; their discrete results match like everyone's."""
    case = _cases()[name]
    d, g = _run(name, "packed", mode)
    if mode != "discrete" and not case.lipschitz:
        with device_frame_arithmetic(oracle):
            ref = oracle.scene_collision(case.spheres, case.arrays, case.weight, case.eta, **_oracle_kw(case, mode))
        bound = 1e-5 * np.abs(ref["distance"]) + 5e-6 * case.weight
        if case.info.get("swept_slope"):
            # "extremes": +-65504 one voxel apart is a slope of 2e6 per metre.  A swept sample sits where the previous samples'
            # penetrations put it, t c + (1 - t) n in float32: 4 roundings of a coordinate below 1 m (2^-24 each) move it by
            # 2.4e-7 m on each of 3 axes, which that slope turns into 1.5 of cost, for each of up to 7 samples -- rounding, not
            # a lost sample (one whole sample in the -65504 slab costs 65504).  The discrete run above has no such term.
            cond = 7 * 3 * case.info["swept_slope"] * 4 * 2.0 ** -24 * case.weight
            if mode == "speed":
                p = case.spheres[..., :3].astype(np.float64)
                cond *= max(1.0, float(np.linalg.norm(p[:, 2:] - p[:, :-2], axis=-1).max() * 0.5 / DT))
            bound = bound + cond
        print(f"\n[{name} {mode}] not 1-Lipschitz: {int((d < ref['distance'] - bound).sum())} of {int((ref['distance'] > 0).sum())} colliding "
              f"spheres lost samples to the cull; largest excess over the oracle {float((d - ref['distance'] - bound).max()):.3e}")
        assert (d <= ref["distance"] + bound).all()
        return
    assert_scene_kernel_parity(oracle, d, g, case.spheres, case.arrays, case.weight, case.eta, f"{name} {mode}", voxel=True,
                               **_oracle_kw(case, mode))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_float64_parity(name):
    """the discrete kernel against the float64 restatement: four times the oracle's own float32 gap of the family (the margin
    tests/test_gpu_support_polygon.py grants a kernel: fma contraction and summation order, not a wrong weight), floored by
    the absolute terms of assert_scene_kernel_parity"""
    case = _cases()[name]
    d, g = _run(name, "packed", "discrete")
    ref = VR.scene_collision(case.spheres, case.arrays, case.weight, case.eta, case.env)
    gap_c, gap_g = VR.ORACLE_F32_GAP[_family(name)]
    tol_c, tol_g = max(4 * gap_c, 5e-6) * case.weight, max(4 * gap_g, 2e-4) * case.weight
    graze = np.abs(case.spheres[..., 3].astype(np.float64) + float(np.float32(case.eta)) - ref["sdf_min"]) < 5e-6
    e_c, e_g = np.abs(d - ref["distance"]), np.abs(g - ref["gradient"])
    print(f"\n[{name}] kernel against float64: cost {float(e_c.max() / case.weight):.3e} m (bound {tol_c / case.weight:.1e}), gradient "
          f"{float(e_g.max() / case.weight):.3e} (bound {tol_g / case.weight:.1e}); {int(graze.sum())} grazing")
    assert np.array_equal((d > 0)[~graze], (ref["distance"] > 0)[~graze])
    assert e_c.max() <= tol_c and e_g.max() <= tol_g


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", CASE_NAMES)
def test_kernel_forms_are_bit_equal(name, mode):
    """packed, in-lane staged and in-lane unstaged (each asserted through scene_collision_form): the same bits"""
    d0, g0 = _run(name, "packed", mode)
    assert (d0 > 0).any() and (d0 != 5.0).all()
    for form in FORMS[1:]:
        d, g = _run(name, form, mode)
        assert np.array_equal(d, d0) and np.array_equal(g, g0), f"{name} {mode}: {form} differs from packed in {int((d != d0).sum())} costs"


@pytest.mark.parametrize("mode", list(MODES))
def test_coarse_minimum_changes_no_bit(mode, oracle):
    case = _cases()["coarse"]
    with_c, without = _run("coarse", "packed", mode, True), _run("coarse", "packed", mode, False)
    assert np.array_equal(with_c[0], without[0]) and np.array_equal(with_c[1], without[1])
    for d, g in (with_c, without):
        assert_scene_kernel_parity(oracle, d, g, case.spheres, case.arrays, case.weight, case.eta, f"coarse {mode}", voxel=True,
                                   **_oracle_kw(case, mode))
    if mode != "discrete":  # sweep reach on both sides of (dilate - 1) voxels
        half = 0.5 * np.linalg.norm(np.diff(case.spheres[..., :3], axis=1), axis=-1)
        assert (half < 2 * VC.VS).any() and (half > 2 * VC.VS).any()


@pytest.mark.parametrize("name", ["store_255", "store_256", "store_257", "store_333"])
@pytest.mark.parametrize("form", FORMS)
def test_padding_and_unused_slots_are_never_read(name, form):
    """every feature row's padding, the disabled slot inside the count and the slot past the count hold -1.0 around the whole
    workspace: a sphere clear of every real grid reports no cost"""
    case = _cases()[name]
    ref = VR.scene_collision(case.spheres, case.arrays, case.weight, case.eta, case.env)
    clear = (ref["distance"] == 0) & (ref["sdf_min"] - case.spheres[..., 3] - case.eta > 1e-4)
    assert clear.sum() > 100 and (np.abs(case.spheres[clear][:, :3]) < 0.95).all(), "the clear spheres must lie inside the poison grids"
    d, g = _run(name, form, "discrete")
    assert (d[clear] == 0).all() and (g[clear] == 0).all()


@pytest.mark.parametrize("speed", [False, True])
def test_sweep_cull_keeps_its_slack(speed, oracle):
    """voxel_cases.slack_window: with less than 3.5 voxels (+ 0.2 % of the distance) between the centre's clearance and the
    half step the kernel must go on sampling and match the reference; beyond that it may only lose samples"""
    from curobo_amd.backends import collision as Cn
    from curobo_amd.scene import SceneData

    dev = torch.device("cuda:0")
    case, k = VC.slack_window()
    scene = SceneData.from_arrays(case.arrays, dev)
    b, h, s = case.spheres.shape[:3]
    dist, grad = torch.full((b, h, s), 5.0, device=dev), torch.full((b, h, s, 4), 5.0, device=dev)
    Cn.sphere_obstacle_collision(dist, grad, torch.as_tensor(case.spheres, device=dev), scene.struct, torch.tensor([case.weight], device=dev),
                                 torch.tensor([case.eta], device=dev), None, b, h, s, False, 3, speed, torch.tensor([DT], device=dev))
    torch.cuda.synchronize()
    d, g = dist.cpu().numpy(), grad.cpu().numpy()
    with device_frame_arithmetic(oracle):
        ref = oracle.scene_collision(case.spheres, case.arrays, case.weight, case.eta, sweep=True, enable_speed_metric=speed, speed_dt=DT)
    print(f"\n[slack window speed={speed}] slack voxels {k.tolist()}: kernel {d[0, 1].tolist()}, oracle {ref['distance'][0, 1].tolist()}")
    assert (ref["distance"][0, 1] > 0).all(), "the reference finds the occupied voxels in every column"
    keep = k < 3.5
    np.testing.assert_allclose(d[0, 1, keep], ref["distance"][0, 1, keep], rtol=1e-5, atol=5e-6 * case.weight)
    np.testing.assert_allclose(g[0, 1, keep], ref["gradient"][0, 1, keep], rtol=1e-3, atol=2e-4 * case.weight)
    assert (d <= ref["distance"] * (1 + 1e-5) + 5e-6 * case.weight).all()


# ------------------------------------------------------------------------------------------------ the fused launch
def _fused_pair(device, arrays, seeds=12, **cfg_kw):
    """fused launch and kernel sequence on the same scene (the _pair of tests/test_gpu_fused.py with a ready store)"""
    from conftest import load_model
    from curobo_amd.robot.kinematics_params import KinematicsParams
    from curobo_amd.rollout import CollisionRollout, CollisionRolloutCfg
    from curobo_amd.scene import SceneData
    from curobo_amd.workloads import seed_knots, start_configuration

    model = load_model("franka")
    kin = KinematicsParams.from_model(model, device)
    scene = SceneData.from_arrays(arrays, device)
    knots = seed_knots(model, seeds, 12, seed=11)
    start = start_configuration(model)
    ros = []
    for fused in (False, True):
        ro = CollisionRollout(kin, scene, seeds, CollisionRolloutCfg(use_fused=fused, fused_materialize=True, **cfg_kw))
        ro.update_start_state(torch.as_tensor(start, device=device))
        ros.append(ro)
    return knots, ros[0], ros[1]


def _workspace_grid(shape, pose, md, centre_local=(0.1, -0.05, 0.0), radius=0.15):
    return VC.make_grid(shape, pose, VC.ball(centre_local, radius), clip=md)


def _fused_world(which):
    rot = (0.35, -0.1, 0.45, 0.82, 0.25, -0.35, 0.38)  # 16^3 voxels of 6.25 cm: a 1 m cube whose faces cut the workspace
    if which == "rotated_truncated":
        return VC.stack_voxel_grids([[_workspace_grid((16, 16, 16), rot, 0.3)]], max_distance=0.3), {}
    if which == "two_grids":
        grids = [_workspace_grid((16, 16, 16), rot, None), _workspace_grid((9, 6, 5), (-0.3, 0.35, 0.4, 1, 0, 0, 0), None, (0, 0, 0), 0.1)]
        return VC.stack_voxel_grids([grids], max_distance=10.0), {}
    if which == "grid_and_33_cuboids":  # more than 32 records: the row pass (discrete, as test_fused_many_obstacles_uses_the_row_pass)
        from curobo_amd.scene import cuboid_scene_arrays

        rng = np.random.default_rng(4)
        world = [{"dims": rng.uniform(0.04, 0.12, 3).tolist(), "pose": [*rng.uniform([-0.6, -0.6, 0.1], [0.7, 0.7, 0.9]).tolist(), 1, 0, 0, 0]}
                 for _ in range(33)]
        return {**cuboid_scene_arrays([world]), **VC.stack_voxel_grids([[_workspace_grid((16, 16, 16), rot, None)]], max_distance=10.0)}, \
            dict(use_sweep=False, use_speed_metric=False)
    if which == "radius_reaches_max_distance":  # R + eta >= max_distance for every link ball: the bounding-ball mask is off
        return VC.stack_voxel_grids([[_workspace_grid((16, 16, 16), rot, 0.0625)]], max_distance=0.0625), {}
    raise KeyError(which)


@pytest.mark.parametrize("which", ["rotated_truncated", "two_grids", "grid_and_33_cuboids", "radius_reaches_max_distance"])
def test_fused_launch_equals_the_kernel_sequence(which, device):
    from test_gpu_fused import _compare

    arrays, cfg_kw = _fused_world(which)
    knots, ro_ref, ro_fused = _fused_pair(device, arrays, **cfg_kw)
    c0, g0, c1, g1 = _compare(ro_ref, ro_fused, knots, device)
    if which == "radius_reaches_max_distance":
        r = ro_fused.robot_spheres[..., 3]
        assert float((r[r >= 0] + ro_fused.cfg.activation_distance).max()) >= 0.0625
    np.testing.assert_allclose(c1, c0, rtol=2e-5, atol=1e-3)
    np.testing.assert_allclose(g1, g0, rtol=1e-3, atol=2e-5 * np.abs(g0).max())
