"""The marching-cubes case table of ``Mapper.extract_mesh``, derived from the cube's geometry (pure NumPy; nothing is copied).

Cube corners 0..7 at (x, y, z) offsets ``CORNERS``, edges 0..11 between the corner pairs ``EDGES``; bit ``c`` of a case is set
iff the value at corner ``c`` is negative, and an edge is *cut* iff exactly one of its ends is.  Per case:

* on each of the six faces the cut edges are connected: two cut edges make one segment, four make two segments, **each
  cutting off one negative corner of that face** (the choice that makes two cubes which share a face agree on it);
* every cut edge lies in two faces and so has exactly two neighbours: the segments close into loops;
* a loop is oriented so that its Newell normal (vertices at the edge midpoints) has a positive sum of dot products with
  ``positive end - negative end`` over its edges: ``(v1 - v0) x (v2 - v0)`` of every triangle points to the positive side;
* a loop is fan-triangulated from its lowest-numbered edge; loops follow one another by their lowest edge.

``triangle_table()`` is int8 [256, 16]: up to 5 triangles as edge triples, then -1."""

from __future__ import annotations

from functools import lru_cache
from typing import List, Tuple

import numpy as np

#: corner -> (x, y, z)
CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.int64)
#: edge -> (corner a, corner b)
EDGES = np.array([(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)], np.int64)
#: edge -> (dx, dy, dz, axis): the cube that owns the edge as its own edge along x (0), y (1) or z (2) from its corner 0
EDGE_OWNER = np.array([(*np.minimum(CORNERS[a], CORNERS[b]), int(np.argmax(np.abs(CORNERS[a] - CORNERS[b])))) for a, b in EDGES], np.int64)


def _faces() -> List[Tuple[Tuple[int, ...], Tuple[int, ...]]]:
    """the six faces: (corners in cyclic order, the edge between corner i and corner i + 1 of that order)"""
    edge_of = {frozenset((int(a), int(b))): e for e, (a, b) in enumerate(EDGES)}
    out = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            ring = []
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[axis], p[u], p[v] = side, du, dv
                ring.append(int(np.flatnonzero((CORNERS == p).all(1))[0]))
            out.append((tuple(ring), tuple(edge_of[frozenset((ring[i], ring[(i + 1) % 4]))] for i in range(4))))
    return out


FACES = _faces()


def cut_edges(case: int) -> List[int]:
    return [e for e, (a, b) in enumerate(EDGES) if ((case >> a) & 1) != ((case >> b) & 1)]


def face_segments(case: int) -> List[Tuple[int, int]]:
    """the face rule: the undirected segments (edge, edge) of every face, each with the lower edge first"""
    segs = []
    for ring, edges in FACES:
        neg = [(case >> c) & 1 for c in ring]
        cut = [i for i in range(4) if neg[i] != neg[(i + 1) % 4]]
        if len(cut) == 2:
            segs.append((edges[cut[0]], edges[cut[1]]))
        elif len(cut) == 4:  # the signs alternate round the face: one segment round each negative corner
            segs.extend((edges[(i - 1) % 4], edges[i]) for i in range(4) if neg[i])
    return sorted(tuple(sorted(s)) for s in segs)


def case_loops(case: int) -> List[List[int]]:
    """the oriented loops of cut edges, each starting at its lowest edge, ordered by that edge"""
    nbr = {e: [] for e in cut_edges(case)}
    for a, b in face_segments(case):
        nbr[a].append(b)
        nbr[b].append(a)
    assert all(len(v) == 2 for v in nbr.values()), f"case {case}: a cut edge without exactly two neighbours"
    mid = 0.5 * (CORNERS[EDGES[:, 0]] + CORNERS[EDGES[:, 1]]).astype(np.float64)
    loops, seen = [], set()
    for start in sorted(nbr):
        if start in seen:
            continue
        loop, prev, cur = [start], None, start
        while True:
            seen.add(cur)
            nxt = nbr[cur][0] if nbr[cur][0] != prev else nbr[cur][1]  # (two edges share one face at most: the two differ)
            if nxt == start:
                break
            loop.append(nxt)
            prev, cur = cur, nxt
        p = mid[loop]
        q = np.roll(p, -1, axis=0)
        newell = np.stack([((p[:, 1] - q[:, 1]) * (p[:, 2] + q[:, 2])).sum(), ((p[:, 2] - q[:, 2]) * (p[:, 0] + q[:, 0])).sum(),
                           ((p[:, 0] - q[:, 0]) * (p[:, 1] + q[:, 1])).sum()])
        toward_positive = 0.0
        for e in loop:
            a, b = EDGES[e]
            pos, neg = (b, a) if (case >> a) & 1 else (a, b)
            toward_positive += float(newell @ (CORNERS[pos] - CORNERS[neg]))
        assert toward_positive != 0.0, f"case {case}: a loop without a side"
        if toward_positive < 0.0:
            loop = [loop[0]] + loop[:0:-1]
        loops.append(loop)
    return loops


@lru_cache(maxsize=None)
def _table() -> np.ndarray:
    table = np.full((256, 16), -1, np.int8)
    for case in range(256):
        row = [e for loop in case_loops(case) for i in range(1, len(loop) - 1) for e in (loop[0], loop[i], loop[i + 1])]
        assert len(row) <= 15, f"case {case}: {len(row) // 3} triangles"
        table[case, : len(row)] = row
    return table


def triangle_table() -> np.ndarray:
    """int8 [256, 16], a fresh copy"""
    return _table().copy()


def triangle_counts() -> np.ndarray:
    """int64 [256]: triangles per case"""
    return (_table() >= 0).sum(1) // 3
