"""Randomised parity of the support-polygon kernels (csrc/support_polygon.hip) against the float64 restatement
tests/support_polygon_ref.py:

    python tests/randomised/fuzz_support_polygon.py <cases> <seed>

Per case: N random point sets of n_pts in 3..64 points (uniform, Gaussian or on a jittered circle) -> the hull launch; the vertex
counts must be the restatement's and every coordinate within 1 ulp of it (the restatement is handed the padding as the fp32
value the launch receives).  Then B x H random points, some of them metres away, against those hulls in both edge modes and
both cost branches.  Bounds, with L the largest coordinate and eps = 2^-24: an edge distance is a handful of fp32 operations
on numbers of size L, so the signed distance and the cost per unit weight lie within 16 eps L; the gradient divides
differences of distances by the smoothing length, in the soft-min weights and in the factor (d_k - s) / smoothing, so it lies
within 8 x 16 eps L / smoothing + 1e-6.  Points closer than 1e-5 to the boundary (the sign may differ) only have to be finite.
Exit status 0 when every case passes."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import support_polygon_ref as R  # noqa: E402

DEV = "cuda:0"
EPS = 2.0 ** -24


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def point_sets(rng, N, n):
    kind = rng.integers(0, 3)
    if kind == 0:
        p = rng.uniform(-0.3, 0.3, (N, n, 2))
    elif kind == 1:
        p = rng.normal(0, 0.15, (N, n, 2))
    else:
        ang = rng.uniform(0, 2 * np.pi, (N, n))
        p = np.stack([np.cos(ang), np.sin(ang)], -1) * rng.uniform(0.2, 0.3, (N, n, 1))
    return (p + rng.uniform(-1, 1, (N, 1, 2))).astype(np.float32)


def one_case(rng):
    from curobo_amd.backends import cost as C

    N, n = int(rng.integers(1, 40)), int(rng.integers(3, 65))
    padding = float(np.float32(rng.choice([0.0, 0.02, 0.05])))
    pts = point_sets(rng, N, n)
    want, want_counts = R.hulls_padded(pts, padding)
    hulls, counts = torch.empty(N, n, 2, device=DEV), torch.empty(N, dtype=torch.int32, device=DEV)
    C.convex_hull_2d(hulls, counts, dev(pts), padding)
    got, got_counts = hulls.cpu().numpy(), counts.cpu().numpy()
    if not np.array_equal(got_counts, want_counts):
        return f"hull counts differ: N {N} n {n}"
    full = np.concatenate([want, np.repeat(want[:, -1:], n - want.shape[1], 1)], 1)
    ulp = np.abs(got.astype(np.float64) - full) / np.spacing(np.abs(full.astype(np.float32))).astype(np.float64)
    if not ulp.max() <= 1.0:
        return f"hull off by {ulp.max():.2f} ulp: N {N} n {n} padding {padding}"
    M = int(want_counts.max())
    if M > 32:
        return None
    B, H = int(rng.integers(1, 300)), int(rng.integers(1, 4))
    idxs = rng.integers(0, N, B).astype(np.int32)
    centre = got[idxs, :1].astype(np.float64)
    p = (centre + rng.uniform(-0.5, 0.5, (B, H, 2)) * rng.choice([1.0, 1.0, 10.0], (B, 1, 1))).astype(np.float32)
    h32 = np.ascontiguousarray(got[:, :M])
    L = float(max(np.abs(p).max(), np.abs(h32).max()))
    tol_sd = 16 * EPS * L
    tol_grad = 8 * tol_sd / R.SMOOTHING + 1e-6
    com = np.zeros((B, H, 4), np.float32)
    com[..., :2] = p
    weight = float(np.float32(rng.uniform(0.5, 50.0)))
    for cnt in (None, got_counts):
        for icw in (0.001, 0.0):
            w = R.support_polygon(p, h32, idxs, cnt, weight, icw)
            cost, grad, sd = torch.empty(B, H, device=DEV), torch.empty(B, H, 4, device=DEV), torch.empty(B, H, device=DEV)
            C.support_polygon_cost(cost, grad, sd, dev(com), dev(h32), None if cnt is None else dev(cnt), dev(idxs),
                                   torch.tensor([weight], device=DEV), icw)
            cost, grad, sd = cost.cpu().numpy(), grad.cpu().numpy(), sd.cpu().numpy()
            if not (np.isfinite(cost).all() and np.isfinite(grad).all() and np.isfinite(sd).all()):
                return "not finite"
            keep = w["boundary"] >= 1e-5
            e_sd = np.abs(sd - w["sd"])[keep].max(initial=0.0)
            e_c = np.abs(cost - w["cost"])[keep].max(initial=0.0) / weight
            e_g = np.abs(grad[..., :2] - w["grad"])[keep].max(initial=0.0) / weight
            if e_sd > tol_sd or e_c > tol_sd or e_g > tol_grad or np.any(grad[..., 2:] != 0):
                return (f"cost kernel: B {B} H {H} M {M} counts {cnt is not None} icw {icw}: sd {e_sd:.2e} cost {e_c:.2e} (bound "
                        f"{tol_sd:.2e}) grad {e_g:.2e} (bound {tol_grad:.2e})")
    return None


def main():
    cases, seed = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (50, 0)
    rng = np.random.default_rng(seed)
    failed = 0
    for c in range(cases):
        msg = one_case(rng)
        if msg:
            failed += 1
            print(f"case {c}: {msg}")
    print(f"fuzz_support_polygon: {cases} cases, {failed} failed")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
