"""Golden vectors for the support-polygon term (csrc/support_polygon.hip, curobo_amd/cost/support_polygon.py), produced by the
REFERENCE's own code on the CPU:

    python tests/golden/make_support_polygon_golden.py [path to the reference checkout]

``geom/convex_polygon_helper.py`` and ``cost/cost_support_polygon.py`` are loaded by path and run unmodified, in float64 AND in
float32.  They import only ``DeviceCfg``, the logger and ``BaseCost`` (for its ``config`` / ``_weight`` members): three stub
modules stand in for those, so nothing else of the reference (Warp, the CUDA extension) is imported.

Inputs are drawn here, rounded to fp32 and recorded, so both runs and every later test see identical numbers.

hull cases   ``hull_vertices`` [64, 12, 2]: 64 random 12-point sets -> ``hull_out64/32`` (padding 0.05), ``hull_counts``.
cost cases   ``c{k}_*`` for the (B, H, M) shapes of the GPU test: hull tensors built BY THE REFERENCE (fp32 run) from
             ``c{k}_vertices`` with mixed vertex counts, so rows repeat the last vertex as the reference pads them;
             ``c{k}_points`` [B, H, 2], ``c{k}_idxs`` [B].  For mode in (padded, counts) and inside_cost_weight in (0.001, 0):
             ``c{k}_{mode}_sd64/32``, ``..._cost{i}_64/32`` and ``..._grad{i}_64/32`` (autograd of cost.sum() in the point),
             i = 1 for 0.001, 0 for 0.  The weight is WEIGHT.  ``counts`` mode hands the reference each hull without its
             repeated rows.
Only arrays are written: tests/golden/support_polygon.npz."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
WEIGHT, PADDING = 2.5, 0.05


def _stub(name, **members):
    m = types.ModuleType(name)
    m.__dict__.update(members)
    m.__path__ = []
    sys.modules[name] = m
    return m


class _DeviceCfg:
    device, dtype = torch.device("cpu"), torch.float32


class _BaseCost:
    def __init__(self, config):
        self.config = config
        self._weight = torch.tensor([config.weight], dtype=config.dtype)


def _load_reference():
    for pkg in ("curobo", "curobo._src", "curobo._src.types", "curobo._src.util", "curobo._src.cost", "curobo._src.geom"):
        _stub(pkg)
    _stub("curobo._src.types.device_cfg", DeviceCfg=_DeviceCfg)
    _stub("curobo._src.util.logging", log_warn=print, log_and_raise=lambda m: (_ for _ in ()).throw(RuntimeError(m)))
    _stub("curobo._src.cost.cost_base", BaseCost=_BaseCost)
    mods = {}
    for name, rel in (("curobo._src.geom.convex_polygon_helper", "curobo/_src/geom/convex_polygon_helper.py"),
                      ("curobo._src.cost.cost_support_polygon", "curobo/_src/cost/cost_support_polygon.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["curobo._src.geom.convex_polygon_helper"].ConvexPolygon2DHelper, mods["curobo._src.cost.cost_support_polygon"].CostSupportPolygon


Helper, Cost = _load_reference()


def polygon_sets(rng, sizes, n_pts, radius=(0.28, 0.4)):
    """one n_pts-point set per entry of ``sizes``: a convex polygon of that many vertices (angles evenly spaced with a jitter
    below a third of the spacing, on an ellipse) and interior points for the rest"""
    out = np.zeros((len(sizes), n_pts, 2))
    for i, k in enumerate(sizes):
        ang = (np.arange(k) + rng.uniform(-0.3, 0.3, k)) * 2 * np.pi / k + rng.uniform(0, 2 * np.pi)
        rx, ry = rng.uniform(*radius, 2)
        poly = np.stack([rx * np.cos(ang), ry * np.sin(ang)], 1)
        inner = rng.uniform(-0.08, 0.08, (n_pts - k, 2))
        pts = np.concatenate([poly, inner])
        out[i] = pts[rng.permutation(n_pts)]
    return out.astype(np.float32)


def reference_hulls(vertices32, dtype):
    h = Helper()
    h.build_convex_hull(torch.as_tensor(vertices32).to(dtype), PADDING)
    return h._cached_convex_hulls.numpy()


def reference_counts(hulls):
    """vertices of every padded hull: rows before the first repeat of the last one"""
    return np.array([next(k for k in range(1, h.shape[0] + 1) if k == h.shape[0] or np.array_equal(h[k - 1], h[-1])) for h in hulls], np.int32)


def reference_cost(points32, hull_rows, dtype, inside_cost_weight):
    """the reference on rows that each bring their own hull: -> (sd, cost, grad)"""
    cfg = types.SimpleNamespace(weight=WEIGHT, dtype=dtype, device_cfg=_DeviceCfg(), inside_cost_weight=inside_cost_weight,
                                foot_sphere_indices=None)
    cost = Cost(cfg)
    cost._polygon_helper._cached_convex_hulls = torch.as_tensor(hull_rows).to(dtype)
    com = torch.as_tensor(points32).to(dtype).requires_grad_(True)
    B = com.shape[0]
    sd = cost._polygon_helper.compute_point_hull_distance(com.detach().unsqueeze(2), torch.arange(B)).squeeze(-1)
    c = cost._compute_support_polygon_cost_vectorized(com) * cost._weight.squeeze()
    c.sum().backward()
    return sd.numpy(), c.detach().numpy(), com.grad.numpy()


def run_case(points32, hulls32, idxs, counts):
    out = {}
    for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
        for i, icw in ((1, 0.001), (0, 0.0)):
            sd, c, g = reference_cost(points32, hulls32[idxs], dtype, icw)
            out[f"padded_sd{tag}"], out[f"padded_cost{i}_{tag}"], out[f"padded_grad{i}_{tag}"] = sd, c, g
            sd, c, g = np.zeros_like(sd), np.zeros_like(c), np.zeros_like(g)
            for h in np.unique(idxs):
                rows = np.nonzero(idxs == h)[0]
                r = reference_cost(points32[rows], np.repeat(hulls32[h:h + 1, :counts[h]], len(rows), 0), dtype, icw)
                sd[rows], c[rows], g[rows] = r
            out[f"counts_sd{tag}"], out[f"counts_cost{i}_{tag}"], out[f"counts_grad{i}_{tag}"] = sd, c, g
    return out


def main():
    rng = np.random.default_rng(20261020)
    g = {}
    # ---- hull cases: 64 random 12-point sets
    hv = rng.uniform(-0.2, 0.2, (64, 12, 2)).astype(np.float32)
    g["hull_vertices"] = hv
    g["hull_out64"], g["hull_out32"] = reference_hulls(hv, torch.float64), reference_hulls(hv, torch.float32)
    g["hull_counts"] = reference_counts(g["hull_out64"])
    assert g["hull_counts"].min() >= 3 and np.array_equal(g["hull_counts"], reference_counts(g["hull_out32"]))
    # ---- cost cases
    shapes = {0: (1, 1, [3]), 1: (5, 3, [4, 8, 6, 5]), 2: (257, 1, [9, 4, 7, 5, 8, 6]), 3: (2, 2, [32, 32])}
    idxs = {0: [0], 1: [2, 0, 2, 3, 1], 2: None, 3: [1, 0]}
    for k, (B, H, sizes) in shapes.items():
        verts = polygon_sets(rng, sizes, 3 if sizes == [3] else max(12, max(sizes)))
        h32, h64 = reference_hulls(verts, torch.float32), reference_hulls(verts, torch.float64)
        counts = reference_counts(h32)
        assert list(counts) == sizes and h32.shape[1] == max(sizes), (k, counts, h32.shape)
        ix = np.array(idxs[k], np.int32) if idxs[k] is not None else rng.integers(0, len(sizes), B).astype(np.int32)
        pts = rng.uniform(-0.6, 0.6, (B, H, 2))
        if k == 2:  # exactly on a vertex (2), 5 m away (4), the middle of the hull (8): the rest is the random mix
            for j in range(2):
                pts[j, 0] = h32[ix[j], j]
            ang = rng.uniform(0, 2 * np.pi, 4)
            pts[2:6, 0] = 5.0 * np.stack([np.cos(ang), np.sin(ang)], 1)
            pts[6:14, 0] = rng.uniform(-0.03, 0.03, (8, 2))
        pts = pts.astype(np.float32)
        g[f"c{k}_vertices"], g[f"c{k}_hulls"], g[f"c{k}_hulls64"], g[f"c{k}_counts"] = verts, h32, h64, counts
        g[f"c{k}_points"], g[f"c{k}_idxs"] = pts, ix
        for name, v in run_case(pts.reshape(B, H, 2), h32, ix, counts).items():
            g[f"c{k}_{name}"] = v
        inside = g[f"c{k}_padded_sd64"] < 0
        print(f"case {k}: B {B} H {H} M {h32.shape[1]} inside {int(inside.sum())} outside {int((~inside).sum())} "
              f"deeper than the margin {int((g[f'c{k}_padded_sd64'] < -0.1).sum())}")
    g["weight"], g["padding"] = np.float64(WEIGHT), np.float64(PADDING)
    out = os.path.join(HERE, "support_polygon.npz")
    np.savez_compressed(out, **g)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
