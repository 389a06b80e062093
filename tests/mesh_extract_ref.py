"""Float64 NumPy restatement of ``Mapper.extract_mesh`` (curobo_amd/csrc/mapper.hip, the ``mapper_mesh_*`` launches) on top of
tests/mapper_ref.py, with the reference's file:line next to each rule (paths under curobo/_src/perception/mapper/).  The
reference's rules are block-sparse; a block "exists" iff its ever-visible byte is set, a voxel exists iff it lies in the grid
PADDED to whole blocks and its block exists.  The case table is curobo_amd.perception.mapper.mc_table's, as on the device.

Two deliberate differences from the reference: cube corners are the voxel CENTRES, the points the TSDF
was sampled at (the reference: (g - N / 2) vs, kernel/builder/builder_mesh.py:477-512), and an edge is cut iff exactly one end
is negative (the reference: s_a s_b < 0, :416-420, which leaves a hole where a value is exactly 0).

Where float32 and float64 may legitimately decide differently ``extract`` says so instead of deciding:

* ``ambiguous_cubes``: cubes whose being a surface cube, or whose case, hangs on a corner value within ``VALUE_TOL`` of 0 or
  of +-truncation.  With ``level == 0`` the sign of ``sw / w`` is the sign of the stored fp16 sum in every precision (the
  smallest quotient of two fp16 values, 6e-8 / 65504, is far above the smallest float32), so nothing near 0 is flagged then;
  near the truncation a cube is flagged only where the decision "some corner is inside the band" hangs on such a corner;
* ``ambiguous_triangles``: triangles whose ``|cross|^2`` lies within a factor 4 of the area threshold;
* ``normal_flag`` per vertex: a coordinate of the final position within ``face_tol`` voxels of a voxel face (the six
  nearest-voxel probes of the normal sit one voxel off it: the interpolation ``t`` near a face, or a refined vertex there), or
  a gradient magnitude below ``GRADIENT_TOL``.

``extract(..., dtype=np.float32)`` runs the same statements in float32: the gap to float64 on one input is what the device
may differ by, up to fusing and reordering."""

from __future__ import annotations

import numpy as np

import mapper_ref as R
from curobo_amd.perception.mapper import mc_table as T

VALUE_TOL, GRADIENT_TOL, AREA_FACTOR = 1e-6, 1e-3, 4.0


class Dense:
    """the padded grid as arrays [PX + 2, PY + 2, PZ + 2] with one never-valid layer on every side: raw sdf and validity"""

    def __init__(self, g: R.Grid, sw, w, block_visible, dtype):
        nbx, nby, nbz = g.nb
        bs = g.bs
        sw = np.asarray(sw, np.float16).astype(dtype)
        w = np.asarray(w, np.float16).astype(dtype)
        valid = np.asarray(block_visible, bool)[: g.n_blocks, None] & (w >= dtype(g.min_weight))       # builder_raycast.py:78 (>=), :105-107
        sdf = sw / np.where(valid, w, dtype(1.0))                                                      # :79

        def dense(a):  # [n_blocks, bs^3] (block (bz nby + by) nbx + bx, voxel lz BS^2 + ly BS + lx) -> [PX, PY, PZ]
            a = a.reshape(nbz, nby, nbx, bs, bs, bs).transpose(2, 5, 1, 4, 0, 3).reshape(nbx * bs, nby * bs, nbz * bs)
            return np.pad(a, 1)

        self.g, self.dtype = g, dtype
        self.shape = np.array([nbx * bs, nby * bs, nbz * bs])
        self.valid, self.sdf = dense(valid), dense(np.where(valid, sdf, dtype(0.0)))
        self.origin = np.asarray(g.origin, dtype)
        self.half = np.asarray([g.nx, g.ny, g.nz], dtype) * dtype(0.5)
        self.vs, self.trunc = dtype(g.vs), dtype(g.trunc)

    def voxel(self, idx):
        """(raw sdf, valid) at integer voxel coordinates [..., 3]; anything outside the padded grid is invalid"""
        inside = ((idx >= 0) & (idx < self.shape)).all(-1)
        i = np.clip(idx, -1, self.shape) + 1
        return self.sdf[i[..., 0], i[..., 1], i[..., 2]], inside & self.valid[i[..., 0], i[..., 1], i[..., 2]]

    def continuous(self, world):
        return (world - self.origin) / self.vs + self.half                                             # builder_coord.py:45-54

    def nearest(self, world):
        """(sdf, valid): the voxel floor(v) of the continuous coordinate  (builder_raycast.py:92-109)"""
        return self.voxel(np.floor(self.continuous(world)).astype(np.int64))

    def trilinear(self, world):
        """(sdf, valid): lower corner floor(v - 0.5); an invalid corner contributes the truncation distance; invalid iff no corner
        is valid  (builder_raycast.py:168-258)"""
        D = self.dtype
        f = self.continuous(world) - D(0.5)                                                            # :186-188
        i0 = np.floor(f)                                                                               # :190-192
        t = f - i0                                                                                     # :194-196
        i0 = i0.astype(np.int64)
        tx, ty, tz = t[..., 0], t[..., 1], t[..., 2]
        one = D(1.0)
        total, any_valid = np.zeros(world.shape[:-1], D), np.zeros(world.shape[:-1], bool)
        for dz, wz in ((0, one - tz), (1, tz)):                                                        # :200-232, in that order
            for dy, wy in ((0, one - ty), (1, ty)):
                for dx, wx in ((0, one - tx), (1, tx)):
                    s, ok = self.voxel(i0 + np.array([dx, dy, dz]))
                    total = total + wx * wy * wz * np.where(ok, s, self.trunc)                         # :238-257
                    any_valid |= ok                                                                    # :234-236
        return total, any_valid

    def gradient(self, world, sample):
        """normalised central difference of six samples at +-voxel_size, (0, 0, 1) if one is invalid or the magnitude is below
        1e-6  (builder_raycast.py:277-325 trilinear, :327-375 nearest).  Returns (direction, magnitude, all six valid)"""
        D = self.dtype
        comp, ok = [], np.ones(world.shape[:-1], bool)
        for a in range(3):
            e = np.zeros(3, D)
            e[a] = self.vs
            sp, vp = sample(world + e)
            sm, vm = sample(world - e)
            comp.append((sp - sm) / (D(2.0) * self.vs))                                                # :317-319
            ok &= vp & vm                                                                              # :307-315
        grad = np.stack(comp, -1)
        mag = np.sqrt((grad * grad).sum(-1))
        use = ok & ~(mag < D(1e-6))                                                                    # :321-323
        up = np.array([0.0, 0.0, 1.0], D)
        return np.where(use[..., None], grad / np.where(use, mag, D(1.0))[..., None], up), mag, ok


def refine(d: Dense, pos, level, iterations):
    """builder_mesh.py:52-80: per iteration a trilinear sample; stop if it is invalid, if |sdf - level| < 1e-6 or sdf - level >
    100; else step clamp(sdf - level, +-voxel_size / 2) against the normalised trilinear gradient"""
    D = d.dtype
    pos = pos.copy()
    live = np.ones(len(pos), bool)
    for _ in range(int(iterations)):
        sdf, ok = d.trilinear(pos)
        val = sdf - D(level)
        live = live & ok & ~(np.abs(val) < D(1e-6)) & ~(val > D(100.0))                                 # :63-67
        direction, _, _ = d.gradient(pos, d.trilinear)                                                 # :69
        step = np.clip(val, -d.vs * D(0.5), d.vs * D(0.5))                                             # :74-78
        pos = np.where(live[:, None], pos - step[:, None] * direction, pos)                            # :79
    return pos


def extract(g: R.Grid, sw, w, block_visible, level=0.0, surface_only=False, refine_iterations=0, dtype=np.float64, face_tol=R.PROBE_TOL):
    """dict(vertices [V, 3], normals [V, 3], triangles int32 [T, 3], n_raw_triangles, ambiguous_cubes, ambiguous_triangles,
    normal_flag bool [V], case_histogram [256], dropped_missing; and every table triangle before the filter: raw int32 [n, 3], keep bool,
    near bool = flagged at the area threshold)"""
    D = dtype
    d = Dense(g, sw, w, block_visible, D)
    PX, PY, PZ = (int(v) for v in d.shape)
    bs, (nbx, nby, _) = g.bs, g.nb
    table, counts = T.triangle_table().astype(np.int64), T.triangle_counts()
    # the eight corner values of every cube of the padded grid, s = sw / w - level  (builder_mesh.py:86-141)
    corner_s, corner_ok = [], []
    for dx, dy, dz in T.CORNERS:
        sl = (slice(1 + dx, 1 + dx + PX), slice(1 + dy, 1 + dy + PY), slice(1 + dz, 1 + dz + PZ))
        corner_s.append(d.sdf[sl] - D(level))                                                          # :101
        corner_ok.append(d.valid[sl])
    s, ok = np.stack(corner_s, -1), np.stack(corner_ok, -1).all(-1)                                     # :187-190
    tol = D(VALUE_TOL)
    sign_sure = np.ones(s.shape, bool) if float(level) == 0.0 else np.abs(s) >= tol
    pos_sure, neg_sure = ((s > 0) & sign_sure).any(-1), ((s < 0) & sign_sure).any(-1)
    crossing = ok & (s > 0).any(-1) & (s < 0).any(-1)                                                   # :192-213
    crossing_maybe = ok & (((s > 0) | ~sign_sure).any(-1)) & (((s < 0) | ~sign_sure).any(-1))
    ambiguous = crossing_maybe & ~(pos_sure & neg_sure)               # being a crossing cube hangs on a corner near the level
    ambiguous |= crossing_maybe & (~sign_sure).any(-1)                # ... or its case does
    surface = crossing
    if surface_only:                                                                                   # :215-227, surface_band = truncation
        in_band = (np.abs(s) < d.trunc).any(-1)
        in_sure, in_maybe = (np.abs(s) < d.trunc - tol).any(-1), (np.abs(s) < d.trunc + tol).any(-1)
        ambiguous |= crossing_maybe & (in_sure != in_maybe)
        surface = surface & in_band
    neg = s < 0
    case = (neg * (1 << np.arange(8))).sum(-1)                                                          # :610-626
    # the deterministic order: (block row, voxel local index)
    gx, gy, gz = np.meshgrid(np.arange(PX), np.arange(PY), np.arange(PZ), indexing="ij")
    key = (((gz // bs) * nby + gy // bs) * nbx + gx // bs) * bs ** 3 + ((gz % bs) * bs + gy % bs) * bs + gx % bs
    # vertices: a surface cube owns its edges 0, 3, 8 and emits one for each that is cut  (:402-423, :520-547)
    cut = np.stack([surface & (neg[..., 0] != neg[..., c]) for c in (1, 3, 4)], -1)                     # (exactly one end negative)
    vkey = (key[..., None] * 3 + np.arange(3))[cut]
    order = np.argsort(vkey)
    cells = np.stack([a[..., None].repeat(3, -1)[cut] for a in (gx, gy, gz)], -1)[order]
    axis = np.broadcast_to(np.arange(3), cut.shape)[cut][order]
    s_a = s[..., 0][..., None].repeat(3, -1)[cut][order]
    s_b = np.stack([s[..., c] for c in (1, 3, 4)], -1)[cut][order]
    n_vertices = len(order)
    vertex_id = np.full((PX + 1, PY + 1, PZ + 1, 3), -1, np.int64)  # (one layer of "no such cube" on the far side)
    vertex_id[cells[:, 0], cells[:, 1], cells[:, 2], axis] = np.arange(n_vertices)
    p_a = d.origin + (cells.astype(D) + D(0.5) - d.half) * d.vs                                         # voxel centres, builder_coord.py:57-66
    p_b = d.origin + ((cells + np.eye(3, dtype=np.int64)[axis]).astype(D) + D(0.5) - d.half) * d.vs
    t = np.clip(-s_a / (s_b - s_a), D(0.0), D(1.0)) if n_vertices else np.zeros(0, D)                  # wp_mc_common.py:487-488
    vertices = p_a + t[:, None] * (p_b - p_a)                                                          # :489
    if refine_iterations > 0 and n_vertices:                                                           # builder_mesh.py:522-523
        vertices = refine(d, vertices, level, refine_iterations)
    if n_vertices:
        normals, mag, six = d.gradient(vertices, d.nearest)                                            # :524, builder_raycast.py:327-375
        v = d.continuous(vertices)
        normal_flag = (np.abs(v - np.rint(v)) < D(face_tol)).any(-1) | (six & (mag < D(GRADIENT_TOL)))
    else:
        normals, normal_flag = np.zeros((0, 3), D), np.zeros(0, bool)
    # triangles: every surface cube walks its table row; a corner is the vertex of the edge's owner cube  (:628-675)
    sx, sy, sz = np.nonzero(surface)
    o = np.argsort(key[sx, sy, sz])
    sx, sy, sz = sx[o], sy[o], sz[o]
    rows = table[case[sx, sy, sz]][:, :15].reshape(-1, 5, 3)                                            # [cubes, 5, 3] edges
    live = rows[..., 0] >= 0
    own = T.EDGE_OWNER[np.maximum(rows, 0)]                                                            # [cubes, 5, 3, 4]
    ids = vertex_id[sx[:, None, None] + own[..., 0], sy[:, None, None] + own[..., 1], sz[:, None, None] + own[..., 2], own[..., 3]]
    raw = ids[live]                                                                                    # (cube, table order)
    assert len(raw) == int(counts[case[sx, sy, sz]].sum())
    present = (raw >= 0).all(-1)                                                                       # wp_mc_filter.py:91-92
    distinct = (raw[:, 0] != raw[:, 1]) & (raw[:, 1] != raw[:, 2]) & (raw[:, 0] != raw[:, 2])          # :95-96
    safe = np.where(present[:, None], raw, 0)
    if n_vertices:
        p0, p1, p2 = vertices[safe[:, 0]], vertices[safe[:, 1]], vertices[safe[:, 2]]
        c = np.cross(p1 - p0, p2 - p0)                                                                 # :103-106
        area2 = (c * c).sum(-1)
    else:
        area2 = np.zeros(len(raw), D)
    threshold = (d.vs * D(1e-6)) ** 2                                                                   # :156
    keep = present & distinct & ~(area2 <= threshold)                                                  # :108
    near = present & distinct & (area2 > threshold / D(AREA_FACTOR)) & (area2 < threshold * D(AREA_FACTOR))
    return dict(vertices=vertices, normals=normals, triangles=raw[keep].astype(np.int32), n_raw_triangles=len(raw),
                ambiguous_cubes=int(ambiguous.sum()), ambiguous_triangles=int(near.sum()), normal_flag=normal_flag,
                case_histogram=np.bincount(case[sx, sy, sz], minlength=256), dropped_missing=int((~present).sum()),
                raw=raw.astype(np.int32), keep=keep, near=near)


def same_triangles(got, ref) -> bool:
    """``got`` [T, 3] is the oracle's list, index for index, where every triangle the oracle flags at the area threshold may be
    there or not"""
    if not ref["near"].any():
        return np.array_equal(got, ref["triangles"])
    sel = ref["keep"] | ref["near"]
    want, optional = ref["raw"][sel], ref["near"][sel]
    i = 0
    for j in range(len(want)):
        if i < len(got) and np.array_equal(got[i], want[j]):
            i += 1
        elif not optional[j]:
            return False
    return i == len(got)


# ---------------------------------------------------------------------------------------------------- properties of a mesh
def directed_edges(triangles):
    t = np.asarray(triangles, np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def is_closed_and_oriented(triangles) -> bool:
    """every directed edge occurs once and has its opposite"""
    e = directed_edges(triangles)
    if len(e) == 0:
        return False
    n = int(e.max()) + 1
    code, back = e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]
    return len(np.unique(code)) == len(code) and np.array_equal(np.sort(code), np.sort(back))


def euler_characteristic(triangles) -> int:
    e = np.sort(directed_edges(triangles), 1)
    return len(np.unique(triangles)) - len(np.unique(e, axis=0)) + len(triangles)


def signed_volume(vertices, triangles) -> float:
    v = np.asarray(vertices, np.float64)
    a, b, c = v[triangles[:, 0]], v[triangles[:, 1]], v[triangles[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


# ---------------------------------------------------------------------------------------------------- the synthetic inputs
def block_layout(g: R.Grid, dense):
    """[PX, PY, PZ] -> [n_blocks, bs^3]"""
    nbx, nby, nbz = g.nb
    bs = g.bs
    return np.ascontiguousarray(dense.reshape(nbx, bs, nby, bs, nbz, bs).transpose(4, 2, 0, 5, 3, 1)).reshape(g.n_blocks, bs ** 3)


def stored_pair(g: R.Grid, sdf_dense, weight_dense):
    """the fp16 pair (sw, w) [n_blocks, bs^3] of a dense sdf and weight over the padded grid"""
    w = block_layout(g, np.asarray(weight_dense, np.float64)).astype(np.float16)
    sw = (block_layout(g, np.asarray(sdf_dense, np.float64)) * w.astype(np.float64)).astype(np.float16)
    return sw, w


def padded_centres(g: R.Grid):
    """[PX, PY, PZ, 3] voxel centres of the padded grid"""
    n = [k * g.bs for k in g.nb]
    ax = [(np.arange(n[a]) + 0.5 - 0.5 * (g.nx, g.ny, g.nz)[a]) * g.vs + g.origin[a] for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1)


#: the sphere's centre, a few mm off the grid's.  The area rule (|cross|^2 <= (1e-6 voxel_size)^2 drops a triangle) removes the
#: tiny triangle that cuts off a corner whose value is within ~1e-4 m of the level, which leaves a pinhole: a sphere of this
#: size has some eight such corners at most centres.  These two were searched for on the CPU: at the first no triangle of the
#: level-0 mesh is dropped or within a factor 4 of the threshold (the mesh is closed), at the second none of the level-0.01
#: mesh is within that factor (some are dropped, on both sides alike).
SPHERE_CENTRE = (-0.0033, 0.0034, -0.0032)
SPHERE_CENTRE_LEVEL = (0.0017, -0.0048, -0.0039)
SPHERE_GRID = dict(nx=30, ny=30, nz=30, bs=4)  # 30 = 7 blocks + 2 voxels: the padded last block is live


def sphere_tsdf(g: R.Grid, radius=R.SPHERE_RADIUS, centre=SPHERE_CENTRE, weight=3.0):
    """(sw, w, visible): the exact sdf of a sphere clipped to +-truncation, weight 3, every block visible"""
    p = padded_centres(g)
    sdf = np.clip(np.linalg.norm(p - np.asarray(centre), axis=-1) - radius, -g.trunc, g.trunc)
    sw, w = stored_pair(g, sdf, np.full(sdf.shape, weight))
    return sw, w, np.ones(g.n_blocks, bool)


def random_field(g: R.Grid, seed: int, margin: int = 2):
    """dense sdf [PX, PY, PZ]: uniform in +-truncation with |sdf| >= 2e-3 inside, +0.5 truncation in a margin of ``margin`` voxels
    of the UNPADDED grid and in the padding"""
    rng = np.random.default_rng(seed)
    n = [k * g.bs for k in g.nb]
    mag = 2e-3 + (0.9 * g.trunc - 2e-3) * rng.random(n)
    sdf = np.where(rng.random(n) < 0.5, -mag, mag)
    inner = np.zeros(n, bool)
    inner[margin:g.nx - margin, margin:g.ny - margin, margin:g.nz - margin] = True
    return np.where(inner, sdf, 0.5 * g.trunc)
