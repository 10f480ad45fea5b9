"""Times the SSIM kernel (csrc/pp_ssim.hip through evaluation.rgb_ssim's wrapper, ops.ssim) on one GPU.

    python tools/time_ssim.py [--out profiles/ssim.txt] [--runs 5]

Per shape (400 x 400 and 1200 x 1600, three channels, V = 1 and a batch) and per form (value only / value and map): the
median of `runs` timed launches with min .. max, each between two events on the stream after a warm-up launch, on buffers
allocated once.  Beside it the same quantity composed from torch on the same device - float32 F.conv2d with the separable
filter over the five moment images, the per-pixel formula and the mean - which is the only other implementation at hand; it
works in float32, the kernel accumulates in float64.  The kernel's rate is given for the bytes that must move - both images
read once, the map written only when asked - as a fraction of the achievable HBM rate of MI355X_MICROARCH.md (6.3 TB/s)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from poseprobe_amd import ops      # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def torch_ssim(x, y, f, c1, c2, want_map):
    """x, y [V,H,W,C] float32 -> [V] (and the map): F.conv2d with the separable filter f [fs], channels as the batch."""
    V, H, W, C = x.shape

    def blur(z):
        z = z.permute(0, 3, 1, 2).reshape(V * C, 1, H, W)
        z = F.conv2d(F.conv2d(z, f.reshape(1, 1, -1, 1)), f.reshape(1, 1, 1, -1))
        return z.reshape(V, C, z.shape[-2], z.shape[-1])

    mu0, mu1 = blur(x), blur(y)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = (blur(x * x) - mu00).clamp_min(0)
    s11 = (blur(y * y) - mu11).clamp_min(0)
    s01 = blur(x * y) - mu01
    s01 = torch.sign(s01) * torch.minimum(torch.sqrt(s00 * s11), s01.abs())
    m = ((2 * mu01 + c1) * (2 * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))
    return m.reshape(V, -1).mean(1), (m.permute(0, 2, 3, 1).contiguous() if want_map else None)


def timed(fn, runs):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ssim.txt'))
    ap.add_argument('--runs', type=int, default=5)
    a = ap.parse_args()
    fs, sigma = 11, 1.5
    hw = fs // 2
    filt = np.exp(-0.5 * ((np.arange(fs) - hw + (2 * hw - fs + 1) / 2) / sigma) ** 2)
    f = torch.tensor(filt / filt.sum(), dtype=torch.float32, device='cuda')
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    lines = [f'SSIM (filter 11, sigma 1.5, 3 channels) on {torch.cuda.get_device_name(0)}: medians of {a.runs} launches (min .. max), '
             f'each between two stream events after one warm-up launch; rates for the bytes that must move against '
             f'{HBM_ACHIEVABLE / 1e12} TB/s', '']
    gen = torch.Generator(device='cuda').manual_seed(0)
    for H, W, V in ((400, 400, 1), (400, 400, 8), (1200, 1600, 1), (1200, 1600, 4)):
        x = torch.rand(V, H, W, 3, device='cuda', generator=gen)
        y = (x + 0.1 * torch.randn(V, H, W, 3, device='cuda', generator=gen)).clamp(0, 1)
        work = torch.empty(ops.ssim_workspace(V, H, W, fs), dtype=torch.uint8, device='cuda')
        out = torch.empty(V, device='cuda')
        smap = torch.empty(V, H - fs + 1, W - fs + 1, 3, device='cuda')
        for want_map in (False, True):
            k = timed(lambda: ops.ssim(x, y, 1., fs, sigma, 0.01, 0.03, work, out, smap if want_map else None), a.runs)
            t = timed(lambda: torch_ssim(x, y, f, c1, c2, want_map), a.runs)
            tv, _ = torch_ssim(x, y, f, c1, c2, False)
            nbytes = 2 * x.numel() * 4 + (smap.numel() * 4 if want_map else 0)
            rate = nbytes / (k[0] * 1e-3)
            lines.append(f'{H:4d} x {W:4d}  V = {V}  {"value + map" if want_map else "value only "}  kernel {k[0]:7.3f} ms ({k[1]:.3f} .. {k[2]:.3f})  '
                         f'{nbytes / 2 ** 20:6.1f} MiB to move, {rate / 1e12:.3f} TB/s = {rate / HBM_ACHIEVABLE:.1%} of achievable HBM   '
                         f'torch composition {t[0]:7.3f} ms ({t[1]:.3f} .. {t[2]:.3f}) = {t[0] / k[0]:.2f} x the kernel   '
                         f'largest difference of the values {float((tv - out).abs().max()):.1e}')
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
