"""Generates poseprobe_amd/csrc/pp_mc_table.h: the 256-case triangle table of the marching-cubes kernels (pp_mesh.hip).

    python tools/gen_mc_table.py            # rewrites the header
    python tools/gen_mc_table.py --check    # fails if the committed header differs from what this script generates

Numbering (also documented in include/poseprobe_hip.h next to pp_mc_table):
  corner c in 0..7 sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) of the cell; bit c of the case index is set iff that
  corner is below the threshold;
  edge e in 0..11 runs along axis a = e >> 2 (0 x, 1 y, 2 z); with j = e & 3 its lower endpoint sits at the offset whose two
  other coordinates, in ascending axis order, are (j & 1, j >> 1).

Construction: on each of the six faces the crossed edges are joined as marching squares joins them (a face whose four edges
are all crossed cuts off each BELOW corner on its own); every segment is directed so that, seen from outside the cube, the
below corners lie on one fixed side.  Every crossed edge then has one incoming and one outgoing segment, so the segments
chain into closed directed loops; each loop is fan-triangulated (fan(): no diagonal inside a cube face).  The side is chosen so that the
geometric normal (v1 - v0) x (v2 - v0) points toward the below corners.  Because a face's segments depend on that face's
four corner bits alone, and the two cells sharing a face see it from opposite sides, neighbouring cells meet without cracks
and with one orientation.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, '..', 'poseprobe_amd', 'csrc', 'pp_mc_table.h')


def corner_offset(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


def edge_endpoints(e):
    a, j = e >> 2, e & 3
    others = [b for b in range(3) if b != a]
    p0 = np.zeros(3, dtype=int)
    p0[others[0]], p0[others[1]] = j & 1, j >> 1
    p1 = p0.copy()
    p1[a] = 1
    return p0, p1


def corner_id(p):
    return int(p[0] + 2 * p[1] + 4 * p[2])


EDGES = [tuple(corner_id(p) for p in edge_endpoints(e)) for e in range(12)]
MID = [(edge_endpoints(e)[0] + edge_endpoints(e)[1]) / 2.0 for e in range(12)]


def face_segments(case, axis, side, below_left):
    """Directed segments (edge id -> edge id) on one face of the cube."""
    n = np.zeros(3)
    n[axis] = 1.0 if side else -1.0
    corners = [c for c in range(8) if corner_offset(c)[axis] == side]
    edges = [e for e in range(12) if EDGES[e][0] in corners and EDGES[e][1] in corners]
    below = lambda c: (case >> c) & 1
    crossed = [e for e in edges if below(EDGES[e][0]) != below(EDGES[e][1])]

    def directed(e1, e2, k, k_is_below):
        # the corner k lies to the left of e1 -> e2 (seen from outside) iff cross(Q - P, K - P) . n > 0
        left = np.dot(np.cross(MID[e2] - MID[e1], corner_offset(k) - MID[e1]), n) > 0
        keep = (left == k_is_below) == below_left
        return (e1, e2) if keep else (e2, e1)

    if len(crossed) == 0:
        return []
    if len(crossed) == 2:
        k = corners[0]
        return [directed(crossed[0], crossed[1], k, bool(below(k)))]
    assert len(crossed) == 4
    segs = []
    for k in corners:
        if below(k):
            e1, e2 = [e for e in edges if k in EDGES[e]]
            segs.append(directed(e1, e2, k, True))
    return segs


def case_triangles(case, below_left):
    nxt = {}
    for axis in range(3):
        for side in range(2):
            for a, b in face_segments(case, axis, side, below_left):
                assert a not in nxt
                nxt[a] = b
    tris, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3
        tris += fan(loop)
    return tris


def share_a_face(e1, e2):
    return any(all(p[axis] == side for e in (e1, e2) for p in edge_endpoints(e)) for axis in range(3) for side in range(2))


def fan(loop):
    """Fan triangulation of a directed loop from the first apex (in loop order from the smallest edge id) none of whose
    diagonals lies in a cube face: a diagonal inside a face could coincide with a diagonal or a segment of the cell beyond that
    face, and the side would then belong to more than two triangles."""
    for r in range(len(loop)):
        rot = loop[r:] + loop[:r]
        if not any(share_a_face(rot[0], rot[i]) for i in range(2, len(rot) - 1)):
            return [(rot[0], rot[i], rot[i + 1]) for i in range(1, len(rot) - 1)]
    raise AssertionError('no fan without an in-face diagonal: %r' % (loop,))


def normal_points_below(case, tris):
    below = np.mean([corner_offset(c) for c in range(8) if (case >> c) & 1], axis=0)
    v0, v1, v2 = (MID[e] for e in tris[0])
    return np.dot(np.cross(v1 - v0, v2 - v0), below - v0) > 0


def generate():
    below_left = normal_points_below(1, case_triangles(1, True))
    table = [case_triangles(case, below_left) for case in range(256)]
    assert not table[0] and not table[255] and max(len(t) for t in table) <= 5
    for c in range(8):
        assert normal_points_below(1 << c, table[1 << c])
        assert normal_points_below(255 ^ (1 << c), table[255 ^ (1 << c)])
    return table


def render(table):
    lines = ['// GENERATED by tools/gen_mc_table.py - do not edit.',
             '// PP_MC_TABLE_INIT: 256 cases x up to 5 triangles of edge ids, -1 terminated (%d triangles in total);'
             % sum(len(t) for t in table),
             '// PP_MC_NTRI_INIT: triangles per case.  Corner, edge and case numbering: include/poseprobe_hip.h (pp_mc_table).',
             '#pragma once', '', '#define PP_MC_TABLE_INIT { \\']
    for case, tris in enumerate(table):
        row = [e for t in tris for e in t]
        row += [-1] * (16 - len(row))
        lines.append('  {' + ', '.join('%2d' % v for v in row) + '}, /* %3d */ \\' % case)
    lines += ['}', '', '#define PP_MC_NTRI_INIT { \\']
    for r in range(0, 256, 32):
        lines.append('  ' + ', '.join(str(len(t)) for t in table[r:r + 32]) + ', \\')
    lines += ['}', '']
    return '\n'.join(lines)


if __name__ == '__main__':
    text = render(generate())
    if '--check' in sys.argv:
        sys.exit(0 if open(OUT).read() == text else 'pp_mc_table.h differs from the generated table')
    with open(OUT, 'w') as f:
        f.write(text)
    print(OUT)
