#!/usr/bin/env python3
"""Generates the marching-cubes case table of the TSDF mesh (include/adcensus_c_api.h: adc_tsdf_mesh_device) and writes
adcensus_amd/csrc/tsdf_mc_table.h.  The table is derived, not typed in: tests/tsdf_mesh_ref.py calls table() and a test holds the
committed header to header_text().

    python tools/gen_tsdf_mc_table.py            writes the header, prints M
    python tools/gen_tsdf_mc_table.py --check    exit 1 when the committed header differs

Corner c of a cell is (c & 1, (c >> 1) & 1, (c >> 2) & 1); bit c of the case index is set iff the corner is negative.  Edge
e = 4 * axis + m runs from its owner corner -- axis x: (0, m & 1, m >> 1), y: (m & 1, 0, m >> 1), z: (m & 1, m >> 1, 0) -- to the
owner's +axis neighbour.  For each case:
  1. face segments: a face with two sign-changing edges gets one segment joining them; a face with four (its negative corners on a
     diagonal) gets two, each joining the two edges that meet at a NEGATIVE corner.  The rule reads the face's four signs only, so
     the two cells that share a face draw the same segments.
  2. loops: every sign-changing edge has one segment on each of its two faces, so the segments chain into closed loops.  A segment is
     directed so that, seen from outside the cell, the negative corner it cuts off lies to its right: the geometric normal
     (v1 - v0) x (v2 - v0) of the triangles then points from the negative corners to the positive side, and case 1 is (e0, e4, e8).
     A loop starts at its lowest edge; loops are ordered by their lowest edge.
  3. triangles: the loop L0 .. L(m-1) becomes a fan (Ls, L(s+i), L(s+i+1)), i = 1 .. m - 2, indices modulo m.  The apex is L0
     wherever that is admissible (340 of the 358 loops): s is the smallest index whose fan has no diagonal joining two edges of ONE
     face of the cell.  Such a diagonal lies in a face that two cells share, and the cell on the other side can draw it as well; then
     it would carry four triangles.  Without one, every directed edge of a closed surface occurs exactly once.  Every loop has such an
     apex (asserted here).
A row is the triangle count followed by 3 * M edge numbers (unused entries 255), padded to a multiple of four bytes."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "adcensus_amd", "csrc", "tsdf_mc_table.h")
UNUSED = 255


def corner(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def corner_index(p):
    return p[0] | (p[1] << 1) | (p[2] << 2)


def edge_owner(e):
    """-> (owner corner offset (di, dj, dk), axis)"""
    axis, m = e >> 2, e & 3
    return ((0, m & 1, m >> 1), (m & 1, 0, m >> 1), (m & 1, m >> 1, 0))[axis], axis


def edge_corners(e):
    o, axis = edge_owner(e)
    b = list(o)
    b[axis] += 1
    return corner_index(o), corner_index(tuple(b))


def edge_mid(e):
    """twice the edge's midpoint (integers)"""
    a, b = (corner(c) for c in edge_corners(e))
    return tuple(a[i] + b[i] for i in range(3))


def faces():
    """-> [(outward normal, the face's four edges)]"""
    out = []
    for axis in range(3):
        for side in (0, 1):
            normal = tuple((2 * side - 1) if i == axis else 0 for i in range(3))
            on = [e for e in range(12) if all(corner(c)[axis] == side for c in edge_corners(e))]
            assert len(on) == 4
            out.append((normal, on))
    return out


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def case_loops(case):
    neg = [bool(case >> c & 1) for c in range(8)]

    def changing(e):
        a, b = edge_corners(e)
        return neg[a] != neg[b]

    def neg_end(e):
        a, b = edge_corners(e)
        return a if neg[a] else b

    succ = {}
    pred = {}
    for normal, on in faces():
        cut = [e for e in on if changing(e)]
        assert len(cut) in (0, 2, 4)
        if len(cut) == 2:
            pairs = [tuple(cut)]
        elif len(cut) == 4:
            by_corner = {}
            for e in cut:
                by_corner.setdefault(neg_end(e), []).append(e)
            assert len(by_corner) == 2 and all(len(v) == 2 for v in by_corner.values())
            pairs = [tuple(v) for v in by_corner.values()]
        else:
            pairs = []
        for ea, eb in pairs:
            ma, mb = edge_mid(ea), edge_mid(eb)
            d = tuple(mb[i] - ma[i] for i in range(3))
            cn = corner(neg_end(ea))
            to_neg = tuple(2 * cn[i] - ma[i] for i in range(3))
            side = dot(cross(normal, d), to_neg)
            assert side != 0
            if side > 0:
                ea, eb = eb, ea
            assert ea not in succ and eb not in pred
            succ[ea] = eb
            pred[eb] = ea
    cut = [e for e in range(12) if changing(e)]
    assert sorted(succ) == cut and sorted(pred) == cut
    loops, left = [], set(cut)
    while left:
        start = min(left)
        loop, e = [], start
        while True:
            loop.append(e)
            left.remove(e)
            e = succ[e]
            if e == start:
                break
        assert len(loop) >= 3
        loops.append(loop)
    return loops


def in_one_face(ea, eb):
    return any(ea in on and eb in on for _, on in faces())


def fan(loop):
    """the loop's triangles: the fan from the first apex none of whose diagonals joins two edges of one face"""
    m = len(loop)
    for s in range(m):
        L = loop[s:] + loop[:s]
        if not any(in_one_face(L[0], L[i]) for i in range(2, m - 1)):
            return [(L[0], L[i], L[i + 1]) for i in range(1, m - 1)]
    raise AssertionError("no admissible apex: %r" % (loop,))


def case_triangles(case):
    return [t for loop in case_loops(case) for t in fan(loop)]


_TABLE = None


def table():
    """-> (M, [list of (e0, e1, e2)] for each of the 256 cases)"""
    global _TABLE
    if _TABLE is None:
        rows = [case_triangles(case) for case in range(256)]
        assert rows[1] == [(0, 4, 8)], rows[1]
        _TABLE = (max(len(r) for r in rows), rows)
    return _TABLE


def row_bytes(M):
    return (1 + 3 * M + 3) // 4 * 4


def header_text():
    M, rows = table()
    R = row_bytes(M)
    lines = [
        "// tsdf_mc_table.h -- GENERATED by tools/gen_tsdf_mc_table.py; do not edit (tests/test_tsdf_mesh_api.py holds this file to the",
        "// generator's output).  The marching-cubes case table of the TSDF mesh (tsdf_cell.h; include/adcensus_c_api.h: adc_tsdf_mesh_device):",
        "// row = case index (bit c set iff corner c is negative), byte 0 the number of triangles, then three cell-edge numbers",
        "// e = 4 * axis + m per triangle, unused bytes %d.  The largest count the generator found is M = %d." % (UNUSED, M),
        "#pragma once",
        "#include <stdint.h>",
        "",
        "#define TSDF_MC_MAX_TRIS %d  // M" % M,
        "#define TSDF_MC_ROW %d       // bytes of a row: 1 + 3 * M rounded up to a multiple of 4" % R,
        "",
        "#if defined(__HIPCC__)",
        "#define TSDF_MC_STORAGE static __device__ const",
        "#else",
        "#define TSDF_MC_STORAGE static const",
        "#endif",
        "",
        "alignas(16) TSDF_MC_STORAGE uint8_t TSDF_MC_TABLE[256 * TSDF_MC_ROW] = {",
    ]
    for case, tris in enumerate(rows):
        b = [len(tris)] + [e for t in tris for e in t]
        b += [UNUSED] * (R - len(b))
        lines.append("    " + ", ".join("%3d" % v for v in b) + ",  // %d" % case)
    lines.append("};")
    return "\n".join(lines) + "\n"


def main(argv):
    text = header_text()
    if "--check" in argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("M = %d; %s" % (table()[0], "the committed header is current" if same else "the committed header DIFFERS"))
        return 0 if same else 1
    with open(HEADER, "w") as f:
        f.write(text)
    print("M = %d (%d bytes per row); wrote %s" % (table()[0], row_bytes(table()[0]), os.path.relpath(HEADER, ROOT)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
