"""oracle/perception_ref.py (float64 NumPy) against the reference's recorded outputs, on the CPU: every filter and segmenter
case of tests/golden/perception_golden.npz and perception_edges_golden.npz (make_perception_golden.py), at the bounds
tests/test_gpu_perception.py holds the HIP kernels to: valid mask / robot mask / masked depth identical outside the stored
excluded sets, filtered depth within 1e-5 relative on the pixels valid in both; and the oracle's own band, computed from
the stored inputs alone, is the stored excluded set."""

import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR

from oracle.perception_ref import filter_depth_ref, mask_band_ref, robot_mask_ref

G = np.load(os.path.join(GOLDEN_DIR, "perception_golden.npz"))
E = np.load(os.path.join(GOLDEN_DIR, "perception_edges_golden.npz"))
FILTER = [("main", str(n)) for n in G["filter_case_names"]] + [("edges", str(n)) for n in E["filter_case_names"]]
SEG = [("main", str(n)) for n in G["seg_case_names"]] + [("edges", str(n)) for n in E["seg_case_names"]]


@pytest.mark.parametrize("which,name", FILTER)
def test_filter_oracle_matches_reference(which, name):
    g = G if which == "main" else E
    prm = g["filter_case_params"][[str(n) for n in g["filter_case_names"]].index(name)]
    depth = g[f"{name}/depth"]
    # columns 6 .. 11: the constants the reference derived (enable_flying, tolerance, enable_bilateral, radius, 2 sigma^2 x 2)
    ksize = int(prm[3])
    filtered, valid, band = filter_depth_ref(depth, prm[0], prm[1], bool(prm[6]), prm[7], ksize, prm[10], prm[11], with_band=True)
    ref_f, ref_v, excluded = g[f"{name}/filtered"], g[f"{name}/valid"].astype(bool), g[f"{name}/excluded"]
    assert np.array_equal(band, excluded)
    assert band.mean() <= 0.005
    both = valid & ref_v
    err = np.abs(filtered[both] - ref_f[both].astype(np.float64))
    worst = float((err / np.maximum(np.abs(ref_f[both]), 1e-300)).max())
    print(f"{name}: valid {int(valid.sum())} ref {int(ref_v.sum())} excluded {int(excluded.sum())} max rel depth error {worst:.3e}")
    assert np.array_equal(valid[~excluded], ref_v[~excluded])
    assert (err <= 1e-5 * np.abs(ref_f[both])).all()
    assert (filtered[~valid] == 0).all()


def _seg_case(which, name):
    """depth, rays, camera position, quaternion, spheres, threshold, key of the recorded outputs"""
    if which == "edges":
        return (E[f"{name}/depth"], E[f"{name}/rays"], E[f"{name}/cam_position"], E[f"{name}/cam_quaternion"], E[f"{name}/spheres"],
                float(E["seg/distance_threshold"]), name)
    from curobo_amd.util.cv import get_projection_rays

    im, ki, pi, si = ([i for i in row if i >= 0] for row in G[f"seg/{name}/index"])
    depth = G["seg/depth"][im]
    rays = get_projection_rays(depth.shape[1], depth.shape[2], torch.as_tensor(G["seg/intrinsics"][ki]), float(G["seg/depth_to_meter"])).numpy()
    if f"seg/{name}/rays" in G:
        assert np.array_equal(rays, G[f"seg/{name}/rays"])
    return depth, rays, G["seg/cam_position"][pi], G["seg/cam_quaternion"][pi], G["seg/spheres"][si], float(G["seg/distance_threshold"]), f"seg/{name}"


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("which,name", SEG)
def test_mask_oracle_matches_reference(which, name, mode):
    g = G if which == "main" else E
    depth, rays, pos, quat, spheres, threshold, key = _seg_case(which, name)
    mask, out, distance = robot_mask_ref(depth, rays, pos, quat, spheres, threshold, mode == "bf16")
    if f"{key}/reference_raises" in g:
        # no sphere at all: the reference's max over the spheres raises (recorded); this library's launch accepts the set, and
        # "within the threshold of some sphere" then holds for no pixel
        assert spheres.shape[1] == 0 and "IndexError" in str(g[f"{key}/reference_raises"])
        assert not mask.any() and np.array_equal(out, depth) and (distance == -np.inf).all()
        return
    ref_m, ref_f, excluded = g[f"{key}/{mode}/mask"].astype(bool), g[f"{key}/{mode}/filtered"], g[f"{key}/{mode}/excluded"]
    band = mask_band_ref(distance, threshold)
    ref_d = g[f"{key}/{mode}/distance"].astype(np.float64)
    live = np.isfinite(ref_d) & np.isfinite(distance)
    print(f"{key}/{mode}: masked {int(mask.sum())} ref {int(ref_m.sum())} excluded {int(excluded.sum())} oracle band {int(band.sum())} "
          f"max |distance - ref| {float(np.abs(distance - ref_d)[live].max()) if live.any() else 0.0:.3e}")
    assert excluded.mean() <= 0.001
    assert np.array_equal(band, excluded)
    assert np.array_equal(mask[~excluded], ref_m[~excluded])
    assert np.array_equal(out[~excluded], ref_f[~excluded])


@pytest.mark.parametrize("seed", [5, 6])
def test_fuzz_generator_stays_inside_its_caps(seed):
    """tests/randomised/fuzz_perception.py at the suite's case count (tests/test_gpu_randomised_sweeps.py): every case's filter band
    <= 0.5 % and mask band <= 0.1 % of its pixels, from the oracle alone, and (asserted inside the generator) every pass over
    the sphere table holds a sphere whose removal changes the oracle's mask.  A case outside is a generator bug."""
    import importlib.util

    from conftest import ROOT

    spec = importlib.util.spec_from_file_location("_fuzz_perception", os.path.join(ROOT, "tests", "randomised", "fuzz_perception.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    passes = combos = 0
    for case, fc, mc in fuzz.generate(24, seed):
        assert fc["band"].mean() <= 0.005, (case, fuzz.describe_filter(fc))
        assert mc["band"].mean() <= 0.001, (case, fuzz.describe_mask(mc))
        passes += len(mc["sole"])
        combos |= 1 << (4 * mc["sb"] + 2 * mc["pb"] + mc["rb"]) if mc["B"] > 1 else 0
    assert passes >= 2 and combos == 0xFF
