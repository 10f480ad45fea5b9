"""Times of mesh -> signed distance grid (poseprobe_amd.mesh.signed_distance_grid, csrc/pp_mesh_sdf.hip) on the
synthetic scene's box: templates of 96^3 and 160^3 nodes from
  box         the 12-triangle cuboid of half the box
  icosphere   level 6 (81 920 triangles), radius 0.4
  mc256       the resolution-256 marching-cubes mesh of tools/time_mesh.py's 160^3 model (deformed field)
Stage by stage: binning (pp_msdf_bin_count, torch.cumsum, pp_msdf_bin_emit), the sort of the (cell, triangle) pairs (torch.sort
and the gather), the distance search (pp_msdf_nearest over the nodes), the crossing counts (pp_msdf_crossings) and the sign
(torch.cumsum along x, torch.where), then mesh.signed_distance_grid whole, host reads and allocations included; with the pair count
and the rings of cells a node visits.  Everything runs in ONE process; each stage is warmed up, then timed `--runs` times with
device events; medians with min .. max.

Baseline: the same closest-point arithmetic for ALL (node, triangle) pairs in chunked torch on the same GPU (no cell grid; at most
`--pair-budget` pairs per chunk).  Its cost is linear in the node count, so where the full grid would take too long
(more than `--baseline-pairs` pairs in all) it is timed on every s-th node along each axis and scaled by s^3; the output says where.

    python tools/time_mesh_sdf.py [--sizes 96 160] [--cases box icosphere mc256] [--runs 5] [--out FILE]

Needs a GPU: there is no CPU timing path.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_mesh import build_model, device_ms, fmt  # noqa: E402


def icosphere(level):
    p = (1 + 5 ** 0.5) / 2
    V = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, float) / np.linalg.norm(v) for v in V]
    for _ in range(level):
        cache, F2 = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = V[a] + V[b]
                V.append(m / np.linalg.norm(m))
                cache[k] = len(V) - 1
            return cache[k]
        for a, b, c in F:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            F2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = F2
    return np.array(V), np.array(F, np.int32)


def cuboid(lo, hi):
    v = np.array([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)], np.float32)
    q = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]
    return v, np.array([f for a, b, c, d in q for f in ((a, b, c), (a, c, d))], np.int32)


def make_mesh(name, lo, hi):
    """-> (vertices float32 [Nv,3], triangles int32 [Nt,3]) on the device, in the box lo .. hi."""
    from poseprobe_amd import mesh
    centre, half = (lo + hi) / 2, (hi - lo) / 2
    if name == 'box':
        v, t = cuboid(centre - half / 2, centre + half / 2)
    elif name == 'icosphere':
        v, t = icosphere(6)
        v = (v * 0.4 + centre[None]).astype(np.float32)
    elif name == 'mc256':
        v, t = mesh.voxurf_extract_deform_geometry(build_model(), lo, hi, resolution=256)
    else:
        raise ValueError(name)
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(t, np.int32)).cuda()


def _segment(q, u, e):
    """closest point of u + s e, 0 <= s <= 1, to q (broadcast [Q,T,3])."""
    den = (e * e).sum(-1)
    s = (((q - u) * e).sum(-1) / den.clamp_min(1e-38)).clamp(0, 1)
    return u + s[..., None] * e


def all_pairs(q, v, t, pair_budget):
    """min over ALL triangles of the kernel's closest-point arithmetic, chunked over the queries: -> dist [Q]."""
    a, b, c = (v[t[:, k].long()][None] for k in range(3))
    ab, ac, bc = b - a, c - a, c - b
    n = torch.linalg.cross(ab, ac)
    nn = (n * n).sum(-1)
    out = torch.empty(q.shape[0], device=q.device)
    step = max(1, pair_budget // t.shape[0])
    for s in range(0, q.shape[0], step):
        p = q[s:s + step, None]
        ap = p - a
        bv = (torch.linalg.cross(ap, ac.expand_as(ap)) * n).sum(-1) / nn
        bw = (torch.linalg.cross(ab.expand_as(ap), ap) * n).sum(-1) / nn
        foot = a + bv[..., None] * ab + bw[..., None] * ac
        d2 = ((foot - p) ** 2).sum(-1)
        d2 = torch.where((bv >= 0) & (bw >= 0) & (bv + bw <= 1) & (nn > 0), d2, torch.full_like(d2, float('inf')))
        for u, e in ((a, ab), (b, bc), (a, ac)):
            d2 = torch.minimum(d2, ((_segment(p, u, e) - p) ** 2).sum(-1))
        out[s:s + step] = d2.amin(1).sqrt()
    return out


def time_case(name, v, t, lo, hi, size, runs, pair_budget, baseline_pairs):
    from poseprobe_amd import mesh, ops
    ws = (size,) * 3
    axes = tuple(torch.from_numpy(x).cuda() for x in mesh.sdf_grid_axes(lo, hi, ws))
    X, Y, Z = ws
    Q, T = X * Y * Z, t.shape[0]
    info = {}
    sdf = mesh.signed_distance_grid(v, t, lo, hi, ws, check=False, info=info)
    out = [f'\n== {name}: {v.shape[0]} vertices, {T} triangles ({mesh.odd_edge_count(t)} odd edges) -> {size}^3 nodes ==',
           f'cell edge {info["cell_edge"]:.5g}, cells {info["cells"]}, {info["pairs"]} (cell, triangle) pairs = {info["pairs"] / T:.2f} per triangle; '
           f'rings per node: mean {info["rings_mean"]:.2f}, max {info["rings_max"]}; {int((sdf < 0).sum())} nodes inside']
    cells = mesh._TriangleCells(v, t)
    grid = cells.grid
    counts = torch.empty(T, dtype=torch.int64, device='cuda')
    keys, tris = torch.empty(cells.n_pairs, dtype=torch.int64, device='cuda'), torch.empty(cells.n_pairs, dtype=torch.int32, device='cuda')
    state = {}

    def binning():
        ops.msdf_bin_count(v, t, grid, counts)
        ends = torch.cumsum(counts, 0)
        ops.msdf_bin_emit(v, t, grid, (ends - counts).contiguous(), keys, tris, cells.n_pairs)

    def sort():
        k, perm = torch.sort(keys, stable=True)
        state['keys'], state['tris'] = k, tris[perm].contiguous()

    dist, closest, tri = torch.empty(Q, device='cuda'), torch.empty(Q, 3, device='cuda'), torch.empty(Q, dtype=torch.int32, device='cuda')
    cross = torch.empty(ops.msdf_crossing_slots(X, Y, Z), dtype=torch.int32, device='cuda')

    def nearest():
        ops.msdf_nearest(None, axes, v, t, cells.keys, cells.tris, grid, float('inf'), dist, closest, tri)

    def sign():
        inside = (torch.cumsum(cross.view(X + 1, Y, Z)[:X], 0, dtype=torch.int32) & 1).bool()
        state['sdf'] = torch.where(inside, -dist.view(X, Y, Z), dist.view(X, Y, Z))

    stages = (('binning: count + cumsum + emit', binning), ('sort: torch.sort + gather', sort), ('distance: pp_msdf_nearest', nearest),
              ('crossings: pp_msdf_crossings', lambda: ops.msdf_crossings(v, t, *axes, cross)), ('sign: cumsum + where', sign),
              ('mesh.signed_distance_grid, whole', lambda: mesh.signed_distance_grid(v, t, lo, hi, ws, check=False)))
    med = {}
    for label, fn in stages:
        ms = device_ms(fn, runs)
        med[label] = statistics.median(ms)
        out.append(f'{label:36s}{fmt(ms)}')
    assert torch.equal(state['keys'], cells.keys) and torch.equal(state['tris'], cells.tris) and torch.equal(state['sdf'], sdf)
    out.append(f'distance search: {Q / med["distance: pp_msdf_nearest"] / 1e3:.1f} M nodes/s')
    # ---- all pairs in chunked torch
    stride = 1
    while (Q // stride ** 3) * T > baseline_pairs:
        stride += 1
    nodes = torch.stack(torch.meshgrid(*(x[::stride] for x in axes), indexing='ij'), -1).reshape(-1, 3).contiguous()
    ms = device_ms(lambda: state.__setitem__('all', all_pairs(nodes, v, t, pair_budget)), min(runs, 3) if stride > 1 else runs)
    want = dist.view(X, Y, Z)[::stride, ::stride, ::stride].reshape(-1)
    err = float((state['all'] - want).abs().max())
    scale = Q / nodes.shape[0]
    whole = statistics.median(ms) * scale
    out.append(f'all pairs in torch, {nodes.shape[0]} nodes (every {stride}. node an axis) x {T} triangles   {fmt(ms)}; max |difference| {err:.3g}')
    out.append(f'all pairs for the {Q} nodes{"" if stride == 1 else f" (scaled by {scale:.1f}, linear in the node count)"}: {whole:.3f} ms = '
               f'{whole / med["distance: pp_msdf_nearest"]:.1f} x the distance search, '
               f'{whole / med["mesh.signed_distance_grid, whole"]:.1f} x signed_distance_grid whole (which also signs)')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[96, 160])
    ap.add_argument('--cases', nargs='+', default=['box', 'icosphere', 'mc256'])
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--pair-budget', type=int, default=1 << 24, help='(node, triangle) pairs per chunk of the torch baseline')
    ap.add_argument('--baseline-pairs', type=float, default=2e10, help='beyond this many pairs the baseline is timed on a sub-lattice')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from poseprobe_amd import synthetic as syn
    lo, hi = syn.XYZ_MIN.astype(np.float32), syn.XYZ_MAX.astype(np.float32)
    lines = [f'mesh -> signed distance grid, box {lo.tolist()} .. {hi.tolist()}, {torch.cuda.get_device_name(0)}',
             f'medians of {a.runs} runs in one process after one warm-up run per stage']
    for name in a.cases:
        v, t = make_mesh(name, lo, hi)
        for size in a.sizes:
            lines += time_case(name, v, t, lo, hi, size, a.runs, a.pair_budget, a.baseline_pairs)
            print('\n'.join(lines[-12:]), flush=True)
        del v, t
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
