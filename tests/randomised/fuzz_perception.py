"""The two perception launches (csrc/perception.hip: depth filter, robot mask) against the float64 oracle (oracle/perception_ref.py,
pinned to the reference's recorded outputs by tests/test_oracle_perception.py) at the shapes where the kernels change how they
index.   python tests/randomised/fuzz_perception.py [cases] [seed]

Every case draws a filter case and a mask case.

filter  B in {1, 2, 5} x H in {1, 2, 15, 16, 17, 33, 48} x W in {1, 2, 63, 64, 65, 127, 128, 129, 200} (a tile is 64 x 16); kernel
        size none or odd 1 .. 31 (5, 7, 31 often: the widest fused halo, the narrowest and the widest 1-d halo); flying-pixel
        rejection on / off; sigmas from the goldens' ranges (2 .. 10 pixels, 0.05 .. 0.1 m); minimum distance 0 or 0.1.  Images:
        a slanted plane, planar patches whose steps lie on both sides of the flying tolerance (some ending ON x = 64 / 128 and
        y = 16), millimetre noise, blocks of 0 / NaN / +-inf / below-minimum / above-maximum pixels, some on the columns 63, 64,
        127, 128, the rows 15, 16 and the corners.  With minimum 0 an input of exactly 0 sits on the limit, that is inside the
        excluded band by its definition: the holes are below-minimum there and a near surface (0.3 m, a few sigma_depth from
        the 0 that rejected pixels carry into the 1-d passes) is added.  Half the cases call backends.perception.filter_depth,
        the others FilterDepth: with its own buffers, or built for another shape (with and without the caller's buffers).
        Held: valid identical outside the band, filtered depth within 1e-5 relative on the pixels valid in both, rejected
        pixels exactly 0.
mask    H x W from factorisations of {1, 255, 1023, 1024, 1025, 5000} pixels (a workgroup holds 1024), B in {1, 3} (3 in the first
        eight cases), rays / pose / spheres shared or per image in all eight combinations (case % 8), fp32 and bf16 ops
        alternating, threshold in {0, 0.02, 0.05}, random unit quaternions (either sign of qw), zeros and negatives in the depth,
        {0, 1, 65, 2047, 2048, 2049, 4100} spheres (a pass holds 2048): most disabled (radius -100), some with radius -0.01 ON a
        pixel's point (inside the threshold: they mask nothing), a few enabled ones with radii of 1 .. 4 cm on random pixels'
        points.  With more than one pass, every pass of every sphere set holds an enabled sphere put on a pixel that nothing
        else masks, and the oracle's mask is asserted to change when that sphere is removed: a skipped or misindexed pass cannot
        agree.  (One pixel cannot be masked by two spheres alone each: a 1-pixel image draws from the one-pass counts.)
        Held: mask and masked depth identical outside the band |distance + threshold| < 1e-5.

Caps on what may be skipped, from the oracle alone before the device result is looked at: filter band <= 0.5 % and mask band
<= 0.1 % of the case's pixels.  The generator redraws (noise / sphere placement, at most ``ATTEMPTS`` times) until a case is
inside; a case that is not is a generator bug and ends the run (tests/test_oracle_perception.py runs the generator for the
suite's seed and count on the CPU)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.perception_ref import (filter_depth_ref, mask_band_ref, robot_frame_points_ref, robot_mask_ref)  # noqa: E402

ATTEMPTS = 20
FILTER_B, FILTER_H, FILTER_W = (1, 2, 5), (1, 2, 15, 16, 17, 33, 48), (1, 2, 63, 64, 65, 127, 128, 129, 200)
KSIZES = [0] + list(range(1, 32, 2))
KWEIGHT = np.array([2.0] + [4.0 if k in (5, 7, 31) else 1.0 for k in range(1, 32, 2)])
MASK_SHAPES = {1: [(1, 1)], 255: [(15, 17), (1, 255)], 1023: [(31, 33), (3, 341)], 1024: [(32, 32), (16, 64)], 1025: [(25, 41), (5, 205)],
               5000: [(50, 100), (40, 125)]}
MASK_SPHERES, CHUNK = (0, 1, 65, 2047, 2048, 2049, 4100), 2048
DMAX = 10.0


def flying_tolerance(threshold):
    return 0.08 * (0.005 / 0.08) ** threshold  # FilterDepth._setup_kernel_params


# ------------------------------------------------------------------------------------------------ filter
def filter_image(rng, H, W, dmin, tol):
    v, u = np.mgrid[0:H, 0:W]
    d = rng.uniform(0.8, 3.0) + rng.uniform(-0.004, 0.004) * u + rng.uniform(-0.004, 0.004) * v
    step = tol if tol > 0 else 0.02

    def patch(y0, y1, x0, x1):
        y0, y1, x0, x1 = max(y0, 0), min(y1, H), max(x0, 0), min(x1, W)
        if y0 < y1 and x0 < x1:  # a step of 0.5 .. 3 x the tolerance, towards or away from the camera, and a slope of its own
            f = 1.0 + float(rng.choice([-1.0, 1.0])) * float(rng.choice([0.5, 0.8, 1.25, 3.0])) * step
            d[y0:y1, x0:x1] = d[y0:y1, x0:x1] * f + rng.uniform(-0.003, 0.003) * (u[y0:y1, x0:x1] - x0)

    for _ in range(int(rng.integers(2, 6))):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        patch(y, y + int(rng.integers(1, H // 2 + 2)), x, x + int(rng.integers(1, W // 2 + 2)))
    for seam in (64, 128):  # patches that end on / start at a tile seam, and one across it
        if W > seam - 8:
            y = int(rng.integers(0, H))
            kind = int(rng.integers(3))
            patch(y - 6, y + 6, *((seam - int(rng.integers(1, 20)), seam) if kind == 0 else (seam, seam + int(rng.integers(1, 20))) if kind == 1
                                  else (seam - 3, seam + 3)))
    if H > 12:
        x = int(rng.integers(0, W))
        patch(16 - int(rng.integers(1, 9)), 16, x - 10, x + 10)
    if dmin == 0.0:
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        ys, xs = slice(max(y - 5, 0), y + 5), slice(max(x - 10, 0), x + 10)
        d[ys, xs] = 0.3 + 0.001 * (u[ys, xs] - x) + 0.0005 * (v[ys, xs] - y)
    d = d + rng.normal(0.0, 0.001, d.shape)
    below, above = dmin - 0.05, DMAX + float(rng.uniform(0.5, 3.0))
    values = [0.0 if dmin > 0 else below, np.nan, np.inf, -np.inf, below, above]
    spots = [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(int(rng.integers(2, 9)))]
    spots += [(int(rng.integers(0, H)), x) for x in (63, 64, 127, 128) if x < W and rng.random() < 0.7]
    spots += [(y, int(rng.integers(0, W))) for y in (15, 16) if y < H and rng.random() < 0.7]
    spots += [c for c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)) if rng.random() < 0.4]
    for (y, x) in spots:
        d[y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 4))] = values[int(rng.integers(len(values)))]
    return d.astype(np.float32)


def draw_filter_case(rng, case):
    c = dict(B=int(rng.choice(FILTER_B)), H=int(rng.choice(FILTER_H)), W=int(rng.choice(FILTER_W)),
             ksize=int(rng.choice(KSIZES, p=KWEIGHT / KWEIGHT.sum())), flying=[None, 0.25, 0.5, 0.8][int(rng.integers(4))],
             sigma_spatial=float(rng.uniform(2.0, 10.0)), sigma_depth=float(rng.uniform(0.05, 0.1)), dmin=float(rng.choice([0.0, 0.1])),
             path="direct" if case % 2 == 0 else ["own_buffers", "other_shape", "other_shape_callers_buffers"][(case // 2) % 3])
    c["tol"] = flying_tolerance(c["flying"]) if c["flying"] is not None else 0.0
    for attempt in range(ATTEMPTS):
        depth = np.stack([filter_image(rng, c["H"], c["W"], c["dmin"], c["tol"]) for _ in range(c["B"])])
        ref = filter_depth_ref(depth, c["dmin"], DMAX, c["flying"] is not None, c["tol"], c["ksize"], 2.0 * c["sigma_spatial"] ** 2,
                               2.0 * c["sigma_depth"] ** 2, with_band=True)
        if ref[2].mean() <= 0.005:
            break
    c.update(depth=depth, ref_filtered=ref[0], ref_valid=ref[1], band=ref[2], attempts=attempt + 1)
    assert c["band"].mean() <= 0.005, f"generator bug: filter band {c['band'].mean():.4f} of case {case} after {ATTEMPTS} draws"
    return c


def describe_filter(c):
    return (f"filter B {c['B']} H {c['H']} W {c['W']} kernel {c['ksize']} flying {c['flying']} sigma_spatial {c['sigma_spatial']:.4f} "
            f"sigma_depth {c['sigma_depth']:.4f} dmin {c['dmin']} path {c['path']}")


# ------------------------------------------------------------------------------------------------ mask
def draw_mask_case(rng, case):
    import torch

    from curobo_amd.util.cv import get_projection_rays

    n_pixels = int(rng.choice(list(MASK_SHAPES)))
    H, W = MASK_SHAPES[n_pixels][int(rng.integers(len(MASK_SHAPES[n_pixels])))]
    B = 3 if case < 8 or rng.random() < 0.5 else 1
    rb, pb, sb = bool(case & 1), bool(case & 2), bool(case & 4)
    bf16 = bool((case + case // 8) & 1)
    threshold = float(rng.choice([0.0, 0.02, 0.05]))
    counts = [s for s in MASK_SPHERES if n_pixels > 1 or s <= CHUNK]
    S = int(rng.choice(counts))
    nb = lambda flag: B if flag else 1  # noqa: E731
    f = rng.uniform(0.5, 1.0, (nb(rb), 2)) * max(W, 8)
    K = np.zeros((nb(rb), 3, 3), np.float32)
    K[:, 0, 0], K[:, 1, 1], K[:, 2, 2] = f[:, 0], f[:, 1], 1.0
    K[:, 0, 2], K[:, 1, 2] = W / 2 + rng.uniform(-2, 2, nb(rb)), H / 2 + rng.uniform(-2, 2, nb(rb))
    rays = get_projection_rays(H, W, torch.as_tensor(K), 1.0).numpy()
    quat = rng.normal(size=(nb(pb), 4))
    quat = (quat / np.linalg.norm(quat, axis=1, keepdims=True)).astype(np.float32)  # (qw of either sign)
    pos = rng.uniform(-0.5, 0.5, (nb(pb), 3)).astype(np.float32)
    v, u = np.mgrid[0:H, 0:W]
    depth = np.stack([rng.uniform(0.6, 2.0) + rng.uniform(-0.3, 0.3) * u / max(W, 2) + rng.uniform(-0.3, 0.3) * v / max(H, 2) +
                      rng.normal(0, 0.002, (H, W)) for _ in range(B)])
    hole = rng.random(depth.shape)
    depth[hole < 0.08] = 0.0
    depth[(hole >= 0.08) & (hole < 0.12)] *= -1.0
    if S > CHUNK:
        depth[:, 0, :min(W, 4)] = np.abs(depth[:, 0, :min(W, 4)]) + 0.5  # pixels with depth for the spheres of every pass
    depth = depth.astype(np.float32)
    points = robot_frame_points_ref(depth, rays, pos, quat, bf16)           # (B, n, 3)
    has_depth = depth.reshape(B, -1) > 0
    chunks = [(s0, min(s0 + CHUNK, S)) for s0 in range(0, S, CHUNK)]
    for attempt in range(ATTEMPTS):
        spheres = np.zeros((nb(sb), S, 4), np.float32)
        spheres[..., :3] = points.reshape(-1, 3)[rng.integers(0, B * n_pixels, (nb(sb), S))] + rng.normal(0, 0.05, (nb(sb), S, 3))
        spheres[..., 3] = -100.0
        sole = []  # (sphere set, sphere index) of the spheres that must each mask a pixel of their own
        for j in range(nb(sb)):
            images = [j] if sb else list(range(B))  # the images this sphere set is used for
            pix = [(b, i) for b in images for i in np.flatnonzero(has_depth[b])]
            if S:
                near = rng.integers(0, S, min(S, 6))  # disabled spheres ON pixels' points, radius inside the threshold
                for k in near:
                    b, i = pix[int(rng.integers(len(pix)))] if pix else (images[0], 0)
                    spheres[j, k] = [*points[b, i], -0.01]
                for k in rng.choice(S, min(S, int(rng.integers(0, 7))), replace=False):  # enabled ones
                    b, i = pix[int(rng.integers(len(pix)))] if pix else (images[0], 0)
                    spheres[j, k] = [*(points[b, i] + rng.normal(0, 0.03, 3)), rng.uniform(0.01, 0.04)]
            if len(chunks) > 1:
                for (s0, s1) in chunks:
                    # a pixel that nothing of this set masks so far, clear of the band by more than the new sphere reaches
                    dist = robot_mask_ref(depth, rays, pos, quat, spheres, threshold, bf16)[2].reshape(B, -1)
                    free = [(b, i) for (b, i) in pix if dist[b, i] < -threshold - 0.005]
                    if not free:
                        break
                    b, i = free[int(rng.integers(len(free)))]
                    k = [s0, s1 - 1, int(rng.integers(s0, s1))][int(rng.integers(3))]  # the first, the last or any slot of the pass
                    spheres[j, k] = [*points[b, i], 0.02]
                    sole.append((j, k))
        mask, depth_out, distance = robot_mask_ref(depth, rays, pos, quat, spheres, threshold, bf16)
        band = mask_band_ref(distance, threshold)
        if band.mean() <= 0.001 and len(sole) == (len(chunks) if len(chunks) > 1 else 0) * nb(sb):
            break
    assert len(sole) == (len(chunks) if len(chunks) > 1 else 0) * nb(sb), f"generator bug: a pass of case {case} found no unmasked pixel in {ATTEMPTS} draws"
    assert band.mean() <= 0.001, f"generator bug: mask band {band.mean():.5f} of case {case} after {ATTEMPTS} draws"
    for (j, k) in sole:
        less = spheres.copy()
        less[j, k, 3] = -100.0
        m2 = robot_mask_ref(depth, rays, pos, quat, less, threshold, bf16)[0]
        assert (m2 != mask)[~band].any(), f"generator bug: sphere {k} of set {j} (case {case}) masks nothing of its own"
    return dict(B=B, H=H, W=W, S=S, rb=rb, pb=pb, sb=sb, bf16=bf16, threshold=threshold, depth=depth, rays=rays, pos=pos, quat=quat,
                spheres=spheres, ref_mask=mask, ref_depth=depth_out, distance=distance, band=band, sole=sole, attempts=attempt + 1)


def describe_mask(c):
    return (f"mask B {c['B']} H {c['H']} W {c['W']} spheres {c['S']} batched rays {c['rb']} pose {c['pb']} spheres {c['sb']} "
            f"bf16 {c['bf16']} threshold {c['threshold']} sole maskers {c['sole']}")


def generate(n_cases, seed):
    rng = np.random.default_rng(seed)
    for case in range(n_cases):
        yield case, draw_filter_case(rng, case), draw_mask_case(rng, case)


# ------------------------------------------------------------------------------------------------ device
def run_filter(c, dev):
    import torch

    from curobo_amd.backends import perception as P
    from curobo_amd.perception import FilterDepth

    depth = torch.as_tensor(c["depth"], device=dev)
    B, H, W, k = c["B"], c["H"], c["W"], c["ksize"]
    if c["path"] == "direct":
        out, valid = torch.full((B, H, W), -1.0, device=dev), torch.full((B, H, W), 7, dtype=torch.uint8, device=dev)
        ta, tb = (torch.full((B, H, W), -1.0, device=dev) for _ in range(2)) if k >= 7 else (None, None)
        P.filter_depth(out, valid, depth, ta, tb, c["dmin"], DMAX, c["flying"] is not None, c["tol"], k, 2.0 * c["sigma_spatial"] ** 2,
                       2.0 * c["sigma_depth"] ** 2)
    else:
        shape, nb = ((H, W), B) if c["path"] == "own_buffers" else ((H + 1, W + 3), B + 1)
        fd = FilterDepth(shape, c["dmin"], DMAX, c["flying"], k if k else None, c["sigma_spatial"], c["sigma_depth"], device=str(dev), num_batch=nb)
        if c["path"] == "other_shape_callers_buffers":
            out, valid = fd(depth, torch.full((B, H, W), -1.0, device=dev), torch.full((B, H, W), 7, dtype=torch.uint8, device=dev))
        else:
            out, valid = fd(depth)
    torch.cuda.synchronize()
    return out.cpu().numpy(), valid.cpu().numpy().astype(bool)


def run_mask(c, dev):
    import torch

    from curobo_amd.backends import perception as P

    t = lambda k: torch.as_tensor(c[k], device=dev).contiguous()  # noqa: E731
    depth = t("depth")
    mask, out = torch.full(depth.shape, 7, dtype=torch.uint8, device=dev), torch.full_like(depth, -7.0)
    P.robot_mask(mask, out, depth, t("rays"), t("pos"), t("quat"), t("spheres"), c["threshold"], P.MASK_BF16_OPS if c["bf16"] else P.MASK_FP32)
    torch.cuda.synchronize()
    return mask.cpu().numpy(), out.cpu().numpy()


def main():
    import torch

    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    dev = torch.device("cuda:0")
    bad, worst, skipped_f, skipped_m = 0, 0.0, 0.0, 0.0
    for case, fc, mc in generate(n_cases, seed):
        skipped_f, skipped_m = max(skipped_f, float(fc["band"].mean())), max(skipped_m, float(mc["band"].mean()))
        try:
            filtered, valid = run_filter(fc, dev)
            ok = ~fc["band"]
            assert np.array_equal(valid[ok], fc["ref_valid"][ok]), f"valid mask differs on {int((valid != fc['ref_valid'])[ok].sum())} pixels outside the band"
            both = valid & fc["ref_valid"]
            err, ref = np.abs(filtered[both] - fc["ref_filtered"][both]), np.abs(fc["ref_filtered"][both])
            if both.any():
                rel = float((err / np.maximum(ref, 1e-300)).max())
                worst = max(worst, rel)
                assert (err <= 1e-5 * ref).all(), f"filtered depth: max relative error {rel:.3e} on {int((err > 1e-5 * ref).sum())} pixels"
            assert (filtered[~valid] == 0).all(), f"{int((filtered[~valid] != 0).sum())} rejected pixels are not 0"
        except (AssertionError, ValueError, RuntimeError) as ex:
            bad += 1
            print(f"FAILED case {case}: {describe_filter(fc)}: {str(ex)[:300]}")
            continue
        try:
            mask, out = run_mask(mc, dev)
            ok = ~mc["band"]
            assert set(np.unique(mask)) <= {0, 1}, "mask holds values other than 0 / 1"
            assert np.array_equal(mask.astype(bool)[ok], mc["ref_mask"][ok]), (
                f"mask differs on {int((mask.astype(bool) != mc['ref_mask'])[ok].sum())} pixels outside the band")
            assert np.array_equal(out[ok], mc["ref_depth"][ok]), "masked depth differs outside the band"
        except (AssertionError, ValueError, RuntimeError) as ex:
            bad += 1
            print(f"FAILED case {case}: {describe_mask(mc)}: {str(ex)[:300]}")
    print(f"{n_cases} cases, {bad} failed  (largest relative error of the filtered depth {worst:.2e}; largest band skipped: filter "
          f"{100 * skipped_f:.3f} %, mask {100 * skipped_m:.3f} %)")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
