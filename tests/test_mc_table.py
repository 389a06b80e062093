"""curobo_amd.perception.mapper.mc_table: the generated marching-cubes table, case by case, against the cube's geometry -- and,
where the reference is on this machine, against the boundary loops of the reference's own table."""

import os
import re

import numpy as np
import pytest

from curobo_amd.perception.mapper import mc_table as T

REFERENCE_TABLE = "/root/reference/curobo/_src/perception/mapper/marching_cubes/kernel/wp_mc_common.py"


def _triangles(row):
    row = [int(e) for e in row]
    n = row.index(-1) if -1 in row else len(row)
    assert n % 3 == 0 and all(e == -1 for e in row[n:]), "edge triples, then -1 to the end"
    return [tuple(row[i:i + 3]) for i in range(0, n, 3)]


def _boundary(triangles):
    """the directed boundary segments of a triangle list: directed edges whose opposite is not there"""
    edges = [(t[i], t[(i + 1) % 3]) for t in triangles for i in range(3)]
    assert len(set(edges)) == len(edges), "a directed edge twice"
    return sorted(e for e in edges if (e[1], e[0]) not in edges)


def _loops(segments):
    """directed segments -> the set of loops, each rotated to start at its lowest edge"""
    nxt = dict(segments)
    assert len(nxt) == len(segments) and sorted(nxt) == sorted(nxt.values()), "every edge is left once and reached once"
    loops, seen = set(), set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, cur = [], start
        while cur not in seen:
            seen.add(cur)
            loop.append(cur)
            cur = nxt[cur]
        assert cur == start
        loops.add(tuple(loop))
    return loops


def test_geometry_of_the_cube():
    assert T.CORNERS.shape == (8, 3) and T.EDGES.shape == (12, 2) and len(T.FACES) == 6
    assert (np.abs(T.CORNERS[T.EDGES[:, 0]] - T.CORNERS[T.EDGES[:, 1]]).sum(1) == 1).all(), "an edge joins neighbours"
    assert sorted(e for _, edges in T.FACES for e in edges) == sorted(list(range(12)) * 2), "every edge lies in two faces"
    # an edge's owner is the cube at the edge's lower end, and there the edge is the cube's own 0, 3 or 8
    for e, (dx, dy, dz, axis) in enumerate(T.EDGE_OWNER):
        a, b = T.CORNERS[T.EDGES[e]]
        assert tuple(np.minimum(a, b)) == (dx, dy, dz) and np.abs(a - b)[axis] == 1
    assert [tuple(o) for o in T.EDGE_OWNER[[0, 3, 8]]] == [(0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 0, 2)]


def test_every_case():
    table = T.triangle_table()
    assert table.shape == (256, 16) and table.dtype == np.int8
    assert np.array_equal(T.triangle_counts(), [len(_triangles(r)) for r in table]) and T.triangle_counts().max() == 5
    mid = 0.5 * (T.CORNERS[T.EDGES[:, 0]] + T.CORNERS[T.EDGES[:, 1]])
    for case in range(256):
        tris = _triangles(table[case])
        assert len(tris) <= 5
        cut = T.cut_edges(case)
        assert sorted({e for t in tris for e in t}) == cut, f"case {case}: the edges used are exactly the cut edges"
        assert (len(tris) == 0) == (case in (0, 255))
        boundary = _boundary(tris)
        for a, b in boundary:  # a boundary segment lies in one face of the cube
            assert any(a in edges and b in edges for _, edges in T.FACES), f"case {case}: segment {a}-{b} crosses the cube"
        assert sorted(tuple(sorted(s)) for s in boundary) == T.face_segments(case), f"case {case}: the boundary is the face rule"
        # orientation: no triangle's normal points from the positive corners to the negative ones (with the vertices at the edge
        # midpoints a triangle that lies in a face of the cube has no component along its own edges: 0), and the row's do point out
        total = 0.0
        for t in tris:
            n = np.cross(mid[t[1]] - mid[t[0]], mid[t[2]] - mid[t[0]])
            toward = sum(float(n @ (T.CORNERS[b] - T.CORNERS[a]) * (1 if (case >> a) & 1 else -1)) for a, b in T.EDGES[list(t)])
            assert toward >= 0, f"case {case}: triangle {t} faces the negative side"
            total += toward
        assert total > 0 or not tris


def test_two_cubes_agree_on_their_shared_face():
    """the segments a case leaves on a face depend on that face's four signs alone, and run against each other seen from the two
    cubes: x = 1 of one cube is x = 0 of the next (corners 1 2 6 5 <-> 0 3 7 4, edges 1 10 5 9 <-> 3 11 7 8), likewise y and z"""
    table = T.triangle_table()
    pairs = (({1: 0, 2: 3, 6: 7, 5: 4}, {1: 3, 10: 11, 5: 7, 9: 8}), ({3: 0, 2: 1, 6: 5, 7: 4}, {2: 0, 10: 9, 6: 4, 11: 8}),
             ({4: 0, 5: 1, 6: 2, 7: 3}, {4: 0, 5: 1, 6: 2, 7: 3}))
    for corner_map, edge_map in pairs:
        for signs in range(16):
            far = sum(((signs >> i) & 1) << c for i, c in enumerate(corner_map))
            near = sum(((signs >> i) & 1) << corner_map[c] for i, c in enumerate(corner_map))
            for other in (0, 0xFF, 0x5A):  # whatever the rest of the two cubes holds
                case_a = far | (other & ~sum(1 << c for c in corner_map))
                case_b = near | (other & ~sum(1 << c for c in corner_map.values()))
                seg_a = {(edge_map[a], edge_map[b]) for a, b in _boundary(_triangles(table[case_a])) if a in edge_map and b in edge_map}
                seg_b = {(a, b) for a, b in _boundary(_triangles(table[case_b])) if a in edge_map.values() and b in edge_map.values()}
                assert seg_a == {(b, a) for a, b in seg_b}, (signs, other)


@pytest.mark.skipif(not os.path.isfile(REFERENCE_TABLE), reason="the reference's marching-cubes table is not on this machine")
def test_boundary_loops_are_the_references_reversed():
    """the reference flips the winding of its table's triangles at the end (wp_mc_filter.py:116-119), so its rows' loops run the other
    way; the diagonals inside a loop may differ"""
    text = open(REFERENCE_TABLE).read()
    body = re.search(r"TRIANGLE_TABLE = np\.array\(\[(.*?)\], dtype", text, re.S).group(1)
    ref = np.array([int(v) for v in re.findall(r"-?\d+", body)]).reshape(256, 16)
    table = T.triangle_table()
    same = 0
    for case in range(256):
        ours, theirs = _triangles(table[case]), _triangles(ref[case])
        assert len(ours) == len(theirs), f"case {case}"
        same += _loops(_boundary(ours)) == _loops([(b, a) for a, b in _boundary(theirs)])
    assert same == 256
