"""Times of the PnP-RANSAC pose initialisation (poseprobe_amd.pnp, csrc/pp_pnp.hip) at P = 512 and 2048 matches with H = 256 and
1024 hypotheses, on a 160^3 Voxurf model with the synthetic scene's box and cameras:

  - pp_pnp_ransac (three launches) and the whole PnPInitialiser call (rays, surface query, sample draw, PnP), with device
    events: one warm-up, then `--runs` calls, medians;
  - the three kernels one by one.  The entry point issues its launches back to back, so events can only bracket the call: the
    split comes from a kernel trace (rocprofv3 --kernel-trace) of a child process of its own that repeats the same calls.  Tracing
    slows the host, not the kernels; the traced process is not the one whose call times are reported.

There is nothing to compare these times with on this project: the reference's cv2.solvePnPRansac is not installed.

    python tools/time_pnp.py [--runs 5] [--out FILE] [--no-trace]

Needs a GPU: there is no CPU timing path.
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.time_mesh import build_model, device_ms, fmt  # noqa: E402

CONFIGS = [(512, 256), (512, 1024), (2048, 256), (2048, 1024)]
KERNELS = ('k_pnp_hypotheses', 'k_pnp_score', 'k_pnp_finish')
RK = dict(near=0.24, far=4.8, bg=0, stepsize=1.5, inverse_y=True, flip_x=False, flip_y=False)


def scene(model, P, seed=0):
    """Matches between the first two synthetic cameras: a sub-pixel grid of P pixels in view A over the object, the surface points
    of the model's own query projected under the pose of view B with half a pixel of noise, a quarter replaced by uniform pixels.
    -> (world [P,3], pix_a, pix_b [P,2], hit [P], Ks [3,3,3], w2c_a, w2c_b)"""
    from poseprobe_amd import camera, recon_utils
    from poseprobe_amd import synthetic as syn
    dev = 'cuda'
    cams = syn.cameras(3)
    w2c_a, w2c_b = torch.tensor(cams[0], device=dev), torch.tensor(cams[1], device=dev)
    Ks = torch.tensor(syn.intrinsics(3, 400, 400), device=dev)
    n = int(np.ceil(P ** 0.5))
    assert n * n >= P
    ax = torch.linspace(125.0, 275.0, n, device=dev) + 0.25
    pix_a = torch.stack(torch.meshgrid(ax, ax, indexing='xy'), -1).reshape(-1, 2)[:P].contiguous()
    o, d = recon_utils.get_ray_dir(pix_a[None], Ks[:1], c2w=camera.pose.invert(w2c_a[None]), inverse_y=True, flip_x=False,
                                   flip_y=False, mode='no_center')
    world, hit, _ = model.query_sdf_point_wocuda(o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous(), global_step=None,
                                                 keep_dim=True, **RK)
    cam = world @ w2c_b[:, :3].T + w2c_b[:, 3]
    pix_b = torch.stack([Ks[1, 0, 0] * cam[:, 0] / cam[:, 2] + Ks[1, 0, 2], Ks[1, 1, 1] * cam[:, 1] / cam[:, 2] + Ks[1, 1, 2]], -1)
    g = torch.Generator().manual_seed(seed)
    pix_b = pix_b + 0.5 * torch.randn(P, 2, generator=g).to(dev)
    swap = (torch.rand(P, generator=g) < 0.25).to(dev)
    pix_b = torch.where(swap[:, None], (400.0 * torch.rand(P, 2, generator=g)).to(dev), pix_b)
    pix_b = torch.where(hit[:, None], pix_b, torch.zeros_like(pix_b)).contiguous()
    return world.contiguous(), pix_a, pix_b, hit, Ks, w2c_a, w2c_b


def raw_call(model, P, H):
    """-> (a closure that issues one pp_pnp_ransac call on fixed inputs, its info tensor)."""
    from poseprobe_amd import ops, pnp
    from poseprobe_amd.pnp import intrinsics_rows
    world, _, pix_b, hit, Ks, w2c_a, _ = scene(model, P)
    valid = hit.to(torch.uint8)
    samples = pnp.draw_samples(valid, H, torch.Generator(device='cuda').manual_seed(1))
    intr = intrinsics_rows(Ks)[1].contiguous()
    work = torch.empty(ops.pnp_workspace(P, H), dtype=torch.uint8, device='cuda')
    w2c, inliers, info = torch.empty(3, 4, device='cuda'), torch.empty(P, dtype=torch.uint8, device='cuda'), \
        torch.empty(2, dtype=torch.int32, device='cuda')
    return (lambda: ops.pnp_ransac(world, pix_b, valid, intr, samples, 8.0, 10, 6, w2c_a, work, w2c, inliers, info)), info, int(hit.sum())


def trace_child(runs):
    """Under the tracer: per configuration, in the order of CONFIGS, one warm-up call and `runs` calls - nothing else that launches
    a k_pnp kernel."""
    model = build_model()
    for P, H in CONFIGS:
        call, _, _ = raw_call(model, P, H)
        for _ in range(runs + 1):
            call()
        torch.cuda.synchronize()


def kernel_split(runs):
    """{(P, H): {kernel: [us per timed call]}} from a kernel trace of a child process, or a string saying why there is none."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', tmp, '--', sys.executable, os.path.abspath(__file__),
               '--trace-child', '--runs', str(runs)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        except (OSError, subprocess.TimeoutExpired) as e:
            return f'not measured: {type(e).__name__}: {e}'
        if p.returncode != 0:
            return f'not measured: the traced run ended with status {p.returncode}: {p.stderr.strip().splitlines()[-1:]}'
        files = glob.glob(os.path.join(tmp, '**', '*kernel_trace.csv'), recursive=True)
        if not files:
            return 'not measured: the tracer wrote no kernel_trace.csv'
        rows = []
        for f in files:
            for r in csv.DictReader(open(f)):
                name = r.get('Kernel_Name', '')
                k = next((k for k in KERNELS if k in name), None)
                if k is not None:
                    rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), k))
    rows.sort()
    per = 3 * (runs + 1)
    if len(rows) != per * len(CONFIGS) or any(rows[i][2] != KERNELS[i % 3] for i in range(len(rows))):
        return f'not measured: {len(rows)} k_pnp dispatches in the trace, {per * len(CONFIGS)} in the expected order were expected'
    out = {}
    for c, cfg in enumerate(CONFIGS):
        mine = rows[c * per + 3:(c + 1) * per]                     # (without the warm-up call)
        out[cfg] = {k: [(e - s) / 1e3 for s, e, kk in mine if kk == k] for k in KERNELS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--trace-child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    if a.trace_child:
        return trace_child(a.runs)
    from poseprobe_amd import pnp
    model = build_model()
    lines = [f'PnP-RANSAC pose initialisation, Voxurf 160^3, {torch.cuda.get_device_name(0)}',
             f'device events, medians of {a.runs} calls in one process after one warm-up call; reproj_error 8 px, 10 Gauss-Newton '
             'steps, min_inliers 6; a quarter of the matches replaced by uniform pixels, 0.5 px noise on the rest']
    for P, H in CONFIGS:
        call, info, n_hit = raw_call(model, P, H)
        ms = device_ms(call, a.runs)
        count, best = info.tolist()
        lines.append(f'\n== P = {P} matches ({n_hit} on the surface), H = {H} hypotheses: {count} inliers, hypothesis {best} ==')
        lines.append(f'pp_pnp_ransac (three launches)          {fmt(ms)}')
        _, pix_a, pix_b, hit, Ks, w2c_a, w2c_b = scene(model, P)
        init = pnp.PnPInitialiser(model, {1: (pix_a, pix_b, torch.ones(P, device='cuda'))}, Ks, RK, n_hypotheses=H, seed=0)
        prev = w2c_a.cpu()
        ms = device_ms(lambda: init(1, prev), a.runs)
        err = float((init(1, prev) - w2c_b).abs().max())
        lines.append(f'PnPInitialiser call (rays + surface query + draw + PnP)  {fmt(ms)}   |pose - generating pose| = {err:.1e}')
    split = 'not measured: --no-trace' if a.no_trace else kernel_split(a.runs)
    lines.append('\n== the three kernels (kernel trace of a child process repeating the pp_pnp_ransac calls above) ==')
    if isinstance(split, str):
        lines.append(split)
    else:
        for (P, H), per in split.items():
            for k in KERNELS:
                us = per[k]
                lines.append(f'P = {P:5d} H = {H:5d}  {k:18s} {statistics.median(us):9.1f} us  (min {min(us):.1f}, max {max(us):.1f}, '
                             f'{len(us)} calls)')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
