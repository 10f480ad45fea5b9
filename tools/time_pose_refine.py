"""Times test-time pose refinement (poseprobe_amd/pose_refine.py) on one GPU and records one end-to-end recovery.

    python tools/time_pose_refine.py [--out profiles/pose_refine.txt] [--runs 5] [--skip-recovery]

Timing: 2048 rays x 128 samples per iteration on a 1200 x 1600 image, a seeded network.  Medians of `runs` timed calls with
min .. max, each between two events on the stream after a warm-up call, in one process; a call is 50 iterations and the figure is
per iteration.  Three variants of the same loop:
  (a) PoseRefiner.refine: pp_nerf_bwd_input, no parameter gradient;
  (b) the same loop with pp_nerf_bwd writing its parameter gradients into a discard block - the kernel work available before
      pp_nerf_bwd_input existed;
  (c) the autograd route: camera.current_pose_c2w -> bg_nerf.SceneRenderer.render -> F.mse_loss -> torch.optim.Adam, which forms
      the rays of all H x W pixels per iteration as the reference does and differentiates the network's parameters too.
Then the whole default call of (a): 500 iterations.

Recovery: a seeded 'teacher' network defines a consistent scene (the synthetic views of poseprobe_amd.synthetic are noise images:
nothing to register against); six views of it are rendered at synthetic.cameras, a fresh network is trained briefly on five of
them at their true poses (SceneEngine), the sixth view's pose is perturbed and refined against the frozen trained network.
Rotation (degrees) and translation (x 100) error of the held-out pose before and after, as evaluation.evaluate_camera_alignment
measures them.  A number for the record: no test threshold is derived from it."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from poseprobe_amd import bg_nerf, camera, evaluation, pose_refine           # noqa: E402
from poseprobe_amd import synthetic as syn                                    # noqa: E402


class FullBackwardRefiner(pose_refine.PoseRefiner):
    """Variant (b): the loop of PoseRefiner with the full backward, its parameter gradients thrown away."""

    def _backward(self, p, b, depth):
        if getattr(self, '_discard', None) is None:
            self._discard = torch.zeros_like(self.net.flat)
        return p.backward(b['ray'], depth, b['g_rgb'], None, self._discard)


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


def autograd_loop(sr, opt, base, K, image, H, W, N, depth_range, iters, gen):
    se3 = torch.zeros(1, 6, device='cuda', requires_grad=True)
    optim = torch.optim.Adam([se3], lr=5e-4)
    flat = image.view(-1, 3)
    for _ in range(iters):
        optim.zero_grad()
        w2c, _ = camera.current_pose_c2w(se3, base[None], fix_first=False)
        idx = torch.randperm(H * W, device='cuda', generator=gen)[:N]
        pred = sr.render(opt, w2c, H, W, K[None], ray_idx=idx, depth_range=depth_range, mode='train')
        torch.nn.functional.mse_loss(pred['rgb'][0], flat[idx]).backward()
        optim.step()
    return se3


def timing(runs):
    H, W, N, S, per_call = 1200, 1600, 2048, 128, 50
    depth_range = (0.5, 3.0)
    opt = bg_nerf.default_options(sample_intvs=S)
    torch.manual_seed(0)
    net = bg_nerf.NeRF(opt, device='cuda')
    net.progress.data.fill_(1.0)
    gen = torch.Generator(device='cuda').manual_seed(0)
    image = torch.rand(H, W, 3, device='cuda', generator=gen)
    K = torch.tensor([[2000., 0., W / 2], [0., 2000., H / 2], [0., 0., 1.]], device='cuda')
    base = torch.tensor(syn.cameras(3)[1], device='cuda')
    a = pose_refine.PoseRefiner(net, opt, H, W, K, depth_range, rand_rays=N)
    b = FullBackwardRefiner(net, opt, H, W, K, depth_range, rand_rays=N)
    sr = bg_nerf.SceneRenderer(opt, nerf=net)
    rows = []
    for name, fn in (('(a) refine: pp_nerf_bwd_input', lambda: a.refine(base, image, iters=per_call, generator=gen)),
                     ('(b) same loop, pp_nerf_bwd into a discard block', lambda: b.refine(base, image, iters=per_call, generator=gen)),
                     ('(c) autograd: SceneRenderer + torch.optim.Adam', lambda: autograd_loop(sr, opt, base, K, image, H, W, N, depth_range, per_call, gen))):
        rows.append((name, [t / per_call for t in timed(fn, runs)]))
    whole = timed(lambda: a.refine(base, image, iters=500, generator=gen), runs)
    lines = [f'Test-time pose refinement on {torch.cuda.get_device_name(0)}: {N} rays x {S} samples per iteration, {H} x {W} image; medians of '
             f'{runs} calls of {per_call} iterations (min .. max), each between two stream events after one warm-up call, one process', '']
    for name, (med, lo, hi) in rows:
        lines.append(f'{name:52s} {med:7.3f} ms per iteration ({lo:.3f} .. {hi:.3f})')
    (ma, _, _), (mb, _, _), (mc, _, _) = (r[1] for r in rows)
    lines += [f'(b) - (a) = {mb - ma:.3f} ms per iteration: the nine weight-gradient products and their launches = {(mb - ma) / mb:.1%} of (b); '
              f'(c) / (a) = {mc / ma:.2f}',
              f'refine(iters = 500), the whole default call of (a): {whole[0]:8.1f} ms ({whole[1]:.1f} .. {whole[2]:.1f})']
    return lines


def recovery():
    H = W = 100
    V, S, depth_range = 6, 128, (1.2, 3.2)
    opt = bg_nerf.default_options(barf_c2f=None, sample_intvs=S)
    torch.manual_seed(1)
    teacher = bg_nerf.NeRF(opt, device='cuda')
    with torch.no_grad():
        teacher.mlp_feat[7].weight[0] *= 3.                      # density and colour with some structure
        teacher.mlp_rgb[1].weight *= 2.
    w2c = torch.tensor(syn.cameras(V), device='cuda')
    K = torch.tensor(syn.intrinsics(1, H, W)[0], device='cuda')
    sr = bg_nerf.SceneRenderer(opt, nerf=teacher)
    images = torch.stack([sr.render_by_slices(opt, w2c[i:i + 1], H, W, K[None], depth_range, mode='val')['rgb'].view(H, W, 3)
                          for i in range(V)])
    held = V // 2
    train = [i for i in range(V) if i != held]
    torch.manual_seed(2)
    net = bg_nerf.NeRF(opt, device='cuda')
    eng = bg_nerf.SceneEngine(net, lr=1e-3)
    gen = torch.Generator(device='cuda').manual_seed(3)
    center, ray = bg_nerf.get_center_and_ray(w2c[train], H, W, K[None].expand(len(train), 3, 3))
    center, ray, target = center.reshape(-1, 3), ray.reshape(-1, 3), images[train].reshape(-1, 3)
    steps, R = 1500, 1024
    for _ in range(steps):
        idx = torch.randint(0, center.shape[0], (R,), device='cuda', generator=gen)
        depth = bg_nerf.sample_depth(opt, 1, R, S, depth_range, mode='train', device='cuda', generator=gen).view(R, S)
        loss, _, _ = eng.step(center[idx].contiguous(), ray[idx].contiguous(), depth.contiguous(), target[idx].contiguous())
    if not bool(torch.isfinite(net.flat).all()):
        return ['', 'Recovery: NOT MEASURED - the briefly trained network holds non-finite parameters (last training loss '
                f'{float(loss):.2e}); nothing was refined']
    se3 = torch.tensor([[0.02, -0.015, 0.01, 0.02, 0.015, -0.02]], device='cuda')
    eye = torch.eye(3, 4, device='cuda')[None]
    base = camera.pose.compose([camera.current_pose_c2w(se3, eye, fix_first=False)[0][0], w2c[held]])
    out = pose_refine.PoseRefiner(net, opt, H, W, K, depth_range, rand_rays=2048).refine(base, images[held], iters=500, generator=gen)
    e0 = evaluation.evaluate_camera_alignment(base[None], w2c[held][None])
    e1 = evaluation.evaluate_camera_alignment(out['pose_w2c'][None], w2c[held][None])
    l = out['losses']
    return ['', f'Recovery: teacher scene, {V} views {H} x {W} on synthetic.cameras, a fresh network trained {steps} steps x {R} rays on {V - 1} '
            f'of them (last training loss {float(loss):.2e}), view {held} held out, its pose perturbed by se3 = {[round(x, 4) for x in se3[0].tolist()]}, '
            f'500 iterations x 2048 rays x {S} samples',
            f'  rotation error {float(e0.R[0]):.3f} -> {float(e1.R[0]):.3f} degrees, translation error (x 100) {float(e0.t[0]):.3f} -> {float(e1.t[0]):.3f}; '
            f'refinement loss, mean of the first / last 50 iterations: {float(l[:50].mean()):.3e} -> {float(l[-50:].mean()):.3e}']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pose_refine.txt'))
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--skip-recovery', action='store_true')
    a = ap.parse_args()
    lines = timing(a.runs)
    if not a.skip_recovery:
        lines += recovery()
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main()
