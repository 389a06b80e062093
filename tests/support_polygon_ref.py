"""Float64 NumPy restatement of the support-polygon term: the convex hull of a point set, the smooth signed distance of a
point to a hull, the cost and its analytic gradient.

Written from the reference's torch code (``geom/convex_polygon_helper.py``, ``cost/cost_support_polygon.py``) one operation
at a time; ``tests/golden/support_polygon.npz`` holds what that code itself returns and ``test_support_polygon_ref.py`` holds
this module to it.  The HIP kernels are then measured against this module on any input.

``hull`` is the reference's Graham scan.  ``hull_monotone_chain`` is the algorithm the kernel runs (sorted by x, lower then
upper chain, the same ``<= 1e-10`` rejection, rotated to the lowest vertex): the two give the same vertex sequence, which the
CPU tests check on every hull case of the GPU tests.
"""

from __future__ import annotations

import numpy as np

MARGIN_TARGET, SMOOTHING = 0.1, 0.01


def _turn(a, b, c) -> float:
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def pad_hull(h: np.ndarray, padding) -> np.ndarray:
    """every vertex moved by ``padding`` along the unit vector from the vertex mean (no move where its norm is <= 1e-8)"""
    if padding is None or not padding > 0 or len(h) <= 1:
        return h
    d = h - h.mean(axis=0)
    n = np.sqrt((d * d).sum(axis=1))
    out = h.copy()
    ok = n > 1e-8
    out[ok] = h[ok] + d[ok] / n[ok, None] * padding
    return out


def hull(points, padding=None) -> np.ndarray:
    """reference ``_compute_convex_hull_single``: [n, 2] -> [count, 2], counter-clockwise from the lowest point"""
    p = np.asarray(points, np.float64)
    n = len(p)
    if n < 3:
        return p
    y, x = p[:, 1], p[:, 0]
    start = int(np.argmin(np.where(np.abs(y - y.min()) < 1e-8, x, np.inf)))
    others = p[np.arange(n) != start]
    v = others - p[start]
    key = np.arctan2(v[:, 1], v[:, 0]) * 1e6 + np.sqrt((v * v).sum(axis=1))
    stack = [p[start]]
    for q in others[np.argsort(key, kind="stable")]:
        while len(stack) >= 2 and _turn(stack[-2], stack[-1], q) <= 1e-10:
            stack.pop()
        stack.append(q)
    return pad_hull(np.stack(stack), padding)


def hull_monotone_chain(points, padding=None) -> np.ndarray:
    """the kernel's algorithm in float64"""
    p = np.asarray(points, np.float64)
    n = len(p)
    if n < 3:
        return p
    P = p[np.lexsort((np.arange(n), p[:, 1], p[:, 0]))]
    H = []
    for q in P:
        while len(H) >= 2 and _turn(H[-2], H[-1], q) <= 1e-10:
            H.pop()
        H.append(q)
    t = len(H) + 1
    for q in P[-2::-1]:
        while len(H) >= t and _turn(H[-2], H[-1], q) <= 1e-10:
            H.pop()
        H.append(q)
    H = np.stack(H[:max(1, min(len(H) - 1, n))])
    y, x = H[:, 1], H[:, 0]
    start = int(np.argmin(np.where(np.abs(y - y.min()) < 1e-8, x, np.inf)))
    return pad_hull(np.roll(H, -start, axis=0), padding)


def hulls_padded(vertices, padding=None, algorithm=hull):
    """reference ``_compute_convex_hull_vectorized``: [N, n, 2] -> (hulls [N, max_count, 2] with the last vertex repeated,
    counts [N])"""
    hs = [algorithm(v, padding) for v in np.asarray(vertices, np.float64)]
    counts = np.array([len(h) for h in hs], np.int32)
    out = np.zeros((len(hs), counts.max(), 2))
    for i, h in enumerate(hs):
        out[i, :len(h)] = h
        out[i, len(h):] = h[-1]
    return out, counts


def hull_cases():
    """name -> (points [N, n, 2] fp32, padding): the hull cases of the GPU test.  The degenerate ones sit on a grid of 1/8, so
    a zero turn is zero in every precision."""
    rng = np.random.default_rng(7)
    f = lambda a: np.asarray(a, np.float32)  # noqa: E731
    cases = {
        "three_points": (f([[[0.25, 0.0], [-0.125, 0.375], [-0.25, -0.125]]]), 0.05),
        "one_interior": (f([[[0, 0], [1, 0], [0.25, 0.25], [0, 1]]]), 0.05),
        "collinear_triple": (f([[[0, 0], [0.5, 0], [1, 0], [1, 1], [0.5, 1], [0, 1], [0, 0.5]]]), 0.05),
        "repeated_point": (f([[[0, 0], [1, 0.125], [1, 0.125], [0.5, 1], [0, 0], [0.5, 1]]]), 0.05),
        "two_lowest": (f([[[0.75, -0.5], [-0.25, -0.5], [0.5, 0.5], [-0.5, 0.25], [0.25, -0.5]]]), 0.05),
        "n64": (rng.uniform(-0.3, 0.3, (3, 64, 2)).astype(np.float32), 0.05),
        "single_hull": (rng.uniform(-0.2, 0.2, (1, 12, 2)).astype(np.float32), 0.05),
        "many_hulls": (rng.uniform(-0.2, 0.2, (130, 12, 2)).astype(np.float32), 0.05),
        "no_padding": (rng.uniform(-0.2, 0.2, (5, 9, 2)).astype(np.float32), 0.0),
    }
    return cases


def edge_distances(p, h):
    """p [2], h [M, 2] -> (d [M], closest [M, 2], cross [M]) over the edges h[k] -> h[k + 1] (the last closing to h[0])"""
    a, b = h, np.roll(h, -1, axis=0)
    e, r = b - a, p - a
    t = np.clip((r * e).sum(axis=1) / np.maximum((e * e).sum(axis=1), 1e-8), 0.0, 1.0)
    c = a + t[:, None] * e
    d = np.sqrt(((p - c) ** 2).sum(axis=1))
    return d, c, e[:, 0] * r[:, 1] - e[:, 1] * r[:, 0]


def signed_distance_point(p, h, smoothing=SMOOTHING):
    """-> (signed distance, d signed distance / d p [2], smallest edge distance)"""
    p, h = np.asarray(p, np.float64), np.asarray(h, np.float64)
    d, c, cr = edge_distances(p, h)
    w = np.exp(-(d - d.min()) / smoothing)
    w = w / w.sum()
    s = float((w * d).sum())
    u = np.where(d[:, None] > 0, (p - c) / np.where(d > 0, d, 1.0)[:, None], 0.0)
    g = ((w * (1.0 - (d - s) / smoothing))[:, None] * u).sum(axis=0)
    inside = bool(np.all(cr >= -1e-8) or np.all(cr <= 1e-8))
    return (-s, -g, float(d.min())) if inside else (s, g, float(d.min()))


def cost_point(sd, gsd, weight, inside_cost_weight, margin_target=MARGIN_TARGET):
    """the reference's ``_compute_support_polygon_cost_vectorized`` on one signed distance, and the chain rule"""
    if inside_cost_weight > 0:
        if sd < 0:
            m = margin_target + sd
            return weight * inside_cost_weight * max(m, 0.0), weight * inside_cost_weight * (1.0 if m > 0 else 0.0) * gsd
        return weight * sd, weight * gsd
    return weight * max(sd, 0.0), weight * (1.0 if sd > 0 else 0.0) * gsd


def support_polygon(points, hulls, idxs, counts=None, weight=1.0, inside_cost_weight=0.001, margin_target=MARGIN_TARGET,
                    smoothing=SMOOTHING):
    """points [B, H, 2], hulls [N, M, 2], idxs [B], counts [N] or None (= all M rows, repeated ones included) ->
    dict(sd [B, H], cost [B, H], grad [B, H, 2], boundary [B, H] = smallest edge distance)"""
    pts, hs = np.asarray(points, np.float64), np.asarray(hulls, np.float64)
    B, H, _ = pts.shape
    out = dict(sd=np.zeros((B, H)), cost=np.zeros((B, H)), grad=np.zeros((B, H, 2)), boundary=np.zeros((B, H)))
    for b in range(B):
        h = hs[int(idxs[b])]
        if counts is not None:
            h = h[:int(counts[int(idxs[b])])]
        for t in range(H):
            sd, g, dmin = signed_distance_point(pts[b, t], h, smoothing)
            c, gc = cost_point(sd, g, weight, inside_cost_weight, margin_target)
            out["sd"][b, t], out["cost"][b, t], out["grad"][b, t], out["boundary"][b, t] = sd, c, gc, dmin
    return out
