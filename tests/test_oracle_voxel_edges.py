"""The float64 restatement of the voxel lookup (tests/voxel_ref.py) against the oracle's float32 one on every case family of
tests/voxel_cases.py (CPU).  Two results: the restatement and the reference agree in every branch class (thin grids, 0 / 1 /
2 / 4 / 8 valid corners, truncated and extreme values, several grids per store), and the oracle's own float32 gap to float64
per family, which docs/ORACLE_PINS.md records and tests/test_gpu_voxel_edges.py grants the kernel four times over."""

import numpy as np
import pytest

import voxel_cases as VC
import voxel_ref as VR

GRAZE = 5e-6  # m: |r + eta - sdf| below this decides the hit in the last float32 bit


def oracle_discrete(oracle, case, arrays=None, spheres=None, env=None):
    sph = case.spheres if spheres is None else spheres
    env = case.env if env is None else env
    return oracle.scene_collision(sph, case.arrays if arrays is None else arrays, case.weight, case.eta, env_query_idx=env,
                                  use_multi_env=case.multi_env, sweep=False)


def float32_gap(case, ref32, ref64):
    """(cost, gradient) largest absolute difference, per unit weight"""
    return (float(np.abs(ref32["distance"] - ref64["distance"]).max() / case.weight),
            float(np.abs(ref32["gradient"][..., :3] - ref64["gradient"][..., :3]).max() / case.weight))


@pytest.mark.parametrize("fam", VC.FAMILIES)
def test_restatement_matches_oracle_and_pins_its_float32_gap(fam, oracle):
    gaps = []
    for case in VC.family(fam):
        ref32 = oracle_discrete(oracle, case)
        ref64 = VR.scene_collision(case.spheres, case.arrays, case.weight, case.eta, case.env)
        r_adj = case.spheres[..., 3].astype(np.float64) + float(np.float32(case.eta))
        graze = np.abs(r_adj - ref64["sdf_min"]) < GRAZE
        hit32, hit64 = ref32["distance"] > 0, ref64["distance"] > 0
        n_hit = int(hit64.sum())
        assert n_hit >= 20 or fam == "extremes" and n_hit > 0, f"{case.name}: only {n_hit} colliding spheres"
        share = float((graze & (hit32 | hit64)).sum() / max(n_hit, 1))
        assert share <= 0.02, f"{case.name}: {share:.3f} of the colliding spheres graze"
        assert np.array_equal(hit32[~graze], hit64[~graze]), f"{case.name}: hit sets differ outside the grazing band"
        w = case.weight
        e_d = np.abs(ref32["distance"] - ref64["distance"]) / (1e-5 * np.abs(ref64["distance"]) + 5e-6 * w)
        e_g = np.abs(ref32["gradient"] - ref64["gradient"]) / (1e-3 * np.abs(ref64["gradient"]) + 2e-4 * w)
        gap = float32_gap(case, ref32, ref64)
        gaps.append(gap)
        line = f"\n[{case.name}] {case.spheres[..., 0].size} spheres, {n_hit} colliding, {int(graze.sum())} grazing; oracle float32 against float64: " \
               f"cost {gap[0]:.3e} m, gradient {gap[1]:.3e} (per unit weight); {float(e_d.max()):.3f} / {float(e_g.max()):.3f} of the parity bounds"
        classes = case.info.get("classes")
        if classes is not None:
            for k in (0, 1, 2, 4, 8):
                m = classes == k
                line += f"\n    {k} valid corners: {int(m.sum())} queries, {int((m & hit64).sum())} colliding, cost gap {float(np.abs(ref32['distance'] - ref64['distance'])[m].max()):.2e}, " \
                        f"gradient gap {float(np.abs(ref32['gradient'] - ref64['gradient'])[m].max()):.2e}"
        print(line)
        assert e_d.max() <= 1.0 and e_g.max() <= 1.0, f"{case.name}: the restatement and the oracle disagree"
    pin = VR.ORACLE_F32_GAP[fam]
    worst = (max(g[0] for g in gaps), max(g[1] for g in gaps))
    print(f"[{fam}] measured float32 gap {worst[0]:.3e} m / {worst[1]:.3e}; pinned {pin[0]:.1e} / {pin[1]:.1e}")
    assert worst[0] <= pin[0] and worst[1] <= pin[1], f"{fam}: the oracle's float32 gap {worst} exceeds its pin {pin} (docs/ORACLE_PINS.md)"


def test_truncated_fields_store_max_distance_only_where_fp16_holds_it():
    a, b = VC.family("truncated")
    assert a.info["stored_reaches_max_distance"] and not b.info["stored_reaches_max_distance"]
    assert np.float16(0.1).astype(np.float32) < np.float32(0.1) and np.float16(0.125).astype(np.float32) == np.float32(0.125)


def test_spheres_that_reach_max_distance_collide_outside_the_grid(oracle):
    """r + eta >= max_distance: the constant outside a grid is a penetration"""
    case = VC.family("truncated")[1]
    r = oracle_discrete(oracle, case)["distance"]
    big = case.spheres[..., 3] + case.eta > 0.1
    assert big.any() and (r[big] > 0).all()


def test_store_padding_and_unused_slots_are_poison():
    arrays = VC.family("store")[0].arrays
    prm, feats = arrays["voxel_params"], arrays["voxel_features"]
    for e in range(2):
        for o in range(3):
            n = int(np.prod(prm[e, o, :3]))
            assert (feats[e, o, n:] == VC.POISON).all()
    assert arrays["voxel_enable"][0].tolist() == [1, 0, 1] and arrays["voxel_enable"][1, 2] == 1  # the unused slot WOULD collide
    assert (feats[1, 2] == VC.POISON).all() and (feats[0, 1] == VC.POISON).all()
