"""Times of the DTU mesh evaluation (poseprobe_amd.dtu_eval) at the size of a real run: a sphere extracted at lattice resolution
512 (mesh.marching_cubes on an analytic field) and scaled to a 300 mm box, against a synthetic scan of `--scan` points on a noisy
shell around it.  Everything runs in ONE process; each stage is warmed up once, then timed `--runs` times with device events
around the whole call (its sorts, scans and host reads included); medians with the spread are reported.

  sample_mesh_points   thresh 0.2
  thin_points          the sampled points under a fixed permutation, radius 0.2
  nearest, d2s         the thinned points against the scan, max_dist 20
  nearest, s2d         the scan against the thinned points
  chamfer              the whole metric (no observation mask cut, no ground plane cut: every point takes part)

If sklearn imports, the host times of the reference's own three calls on the same inputs (lib/dtu_eval.py:98-106 radius_neighbors
and the loop, :145-146 and :158-159 kneighbors) are reported beside them, once each: for reading, not a pass criterion.

    python tools/time_dtu_eval.py [--resolution 512] [--scan 3000000] [--runs 5] [--no-host] [--out profiles/dtu_eval.txt]

Needs a GPU: there is no CPU timing path.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BOX = 300.0
RADIUS = 0.4           # of the box


def device_ms(fn, runs, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    return out


def fmt(ms):
    return f'{statistics.median(ms):10.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} runs)'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--scan', type=int, default=3000000)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from poseprobe_amd import dtu_eval, mesh
    res = a.resolution
    ax = torch.linspace(-0.5, 0.5, res, device='cuda')
    u = RADIUS - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    vertices, triangles = mesh.marching_cubes(u, 0.0)
    del u
    vertices = (vertices.double() / (res - 1.0)) * BOX                    # lattice -> millimetres in [0, 300]^3
    g = torch.Generator().manual_seed(0)
    d = torch.randn(a.scan, 3, generator=g)
    d /= d.norm(dim=1, keepdim=True)
    stl = (d * (RADIUS * BOX + 0.5 * torch.randn(a.scan, 1, generator=g)) + BOX / 2).float().cuda()
    lines = [f'DTU mesh evaluation, sphere of radius {RADIUS * BOX:.0f} mm at resolution {res}: {vertices.shape[0]} vertices, '
             f'{triangles.shape[0]} triangles; scan {a.scan} points; {torch.cuda.get_device_name(0)}',
             f'medians of {a.runs} runs in one process after one warm-up run per stage, device events around the whole call']
    box = {}
    ms = device_ms(lambda: box.__setitem__('pcd', dtu_eval.sample_mesh_points(vertices, triangles, 0.2)), a.runs)
    pcd = box['pcd']
    lines.append(f'sample_mesh_points  -> {pcd.shape[0]:9d} points      {fmt(ms)}')
    perm = torch.randperm(pcd.shape[0], generator=g)
    pcd = pcd[perm.cuda()].contiguous()
    info = {}
    ms = device_ms(lambda: box.__setitem__('keep', dtu_eval.thin_points(pcd, 0.2, info)), a.runs)
    down = pcd[box['keep']].contiguous()
    lines.append(f'thin_points         -> {down.shape[0]:9d} kept, {info["rounds"]:2d} rounds  {fmt(ms)}')
    ms = device_ms(lambda: box.__setitem__('d2s', dtu_eval.nearest(down, stl, 20.0)), a.runs)
    lines.append(f'nearest, d2s        {down.shape[0]:9d} queries x {stl.shape[0]} points  {fmt(ms)}')
    ms = device_ms(lambda: box.__setitem__('s2d', dtu_eval.nearest(stl, down, 20.0)), a.runs)
    lines.append(f'nearest, s2d        {stl.shape[0]:9d} queries x {down.shape[0]} points  {fmt(ms)}')
    obs = torch.ones(2, 2, 2, dtype=torch.bool, device='cuda')
    bb = torch.tensor([[0., 0., 0.], [BOX, BOX, BOX]])
    call = lambda: box.__setitem__('r', dtu_eval.chamfer(vertices, triangles, stl, obs, bb, BOX, [0., 0., 1., 1.], perm=perm))
    ms = device_ms(call, a.runs)
    lines.append(f'chamfer (whole)     {fmt(ms)}')
    lines.append(f'  -> {box["r"]}')

    def report():
        text = '\n'.join(lines)
        if a.out:
            with open(a.out, 'w') as f:
                f.write(text + '\n')
        return text

    report()                                                               # (the host part below takes minutes)
    try:
        import sklearn.neighbors as skln
    except ImportError:
        skln = None
    if skln is not None and not a.no_host:
        lines.append(f'\n== host: the reference\'s own calls on the same inputs (sklearn kd_tree, n_jobs=-1, {os.cpu_count()} CPUs visible), once each ==')
        data_pcd, stl_h = pcd.cpu().numpy().astype(np.float64), stl.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        nn = skln.NearestNeighbors(n_neighbors=1, radius=0.2, algorithm='kd_tree', n_jobs=-1)
        nn.fit(data_pcd)
        rnn = nn.radius_neighbors(data_pcd, radius=0.2, return_distance=False)
        t1 = time.perf_counter()
        mask = np.ones(data_pcd.shape[0], dtype=np.bool_)
        for curr, idxs in enumerate(rnn):
            if mask[curr]:
                mask[idxs] = 0
                mask[curr] = 1
        t2 = time.perf_counter()
        lines.append(f'radius_neighbors {t1 - t0:8.2f} s + loop {t2 - t1:8.2f} s   kept {int(mask.sum())} '
                     f'(device kept {down.shape[0]}; float64 against float32 distances)')
        del rnn
        data_down = data_pcd[mask]
        t0 = time.perf_counter()
        nn.fit(stl_h)
        dist_d2s, _ = nn.kneighbors(data_down, n_neighbors=1, return_distance=True)
        t1 = time.perf_counter()
        nn.fit(data_down)
        dist_s2d, _ = nn.kneighbors(stl_h, n_neighbors=1, return_distance=True)
        t2 = time.perf_counter()
        lines.append(f'kneighbors, d2s  {t1 - t0:8.2f} s   mean {dist_d2s[dist_d2s < 20].mean()!r}')
        lines.append(f'kneighbors, s2d  {t2 - t1:8.2f} s   mean {dist_s2d[dist_s2d < 20].mean()!r}')
    print(report())


if __name__ == '__main__':
    main()
