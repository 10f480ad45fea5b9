"""Times forward-only scene rendering (pp_nerf_infer, SceneRenderer.render_view, gen_videos) on one GPU.

    python tools/time_scene_view.py [--out profiles/scene_view.txt] [--runs 5] [--skip-large]

Medians of `runs` timed calls with min .. max, each between two events on the stream after one warm-up call per path, in one
process; where two paths are compared their calls ALTERNATE (a, b, a, b, ...), so that drift of the device hits both alike.
  1. the sample stage alone: pp_nerf_infer against pp_nerf_fwd at 3072 rays x 128 samples and at 8192 x 256, a seeded network,
     with the bytes of per-sample workspace either one writes into (from pp_nerf_infer_workspace / pp_nerf_workspace);
  2. one whole view at 400 x 400 and at 1200 x 1600 (--skip-large leaves the second out), coarse 128 + fine 128 samples per ray,
     through render_by_slices (opt.nerf.rand_rays = 1024, the default) and through render_view (chunk_rays = 8192, the default);
  3. a 120-frame DTU novel-view sequence (gen_videos.render_novel_views, n_frames = 60) at 400 x 400: one timed call.
Every pp_nerf_infer / pp_nerf_fwd call re-forms the operand maxima and the packed weight stream of its network (four small
launches); at 8192-ray chunks that is below one per cent of a chunk and is not separated out here."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from poseprobe_amd import bg_nerf, gen_videos, ops      # noqa: E402
from poseprobe_amd import synthetic as syn              # noqa: E402

DEPTH_RANGE = (0.5, 3.0)


def _once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternated(fns, runs):
    """fns: [callable]; one warm-up call each, then `runs` rounds in which every path runs once -> [(median, min, max)]."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            ms[i].append(_once(fn))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def fmt(t):
    return f'{t[0]:10.3f} ms ({t[1]:.3f} .. {t[2]:.3f})'


def sample_stage(R, S, runs):
    opt = bg_nerf.default_options(sample_intvs=S)
    torch.manual_seed(0)
    net = bg_nerf.NeRF(opt, device='cuda')
    net.progress.data.fill_(1.0)
    g = torch.Generator(device='cuda').manual_seed(1)
    f = dict(dtype=torch.float32, device='cuda')
    center, ray = torch.randn(R, 3, generator=g, **f) * 0.2, torch.randn(R, 3, generator=g, **f)
    depth = ((torch.rand(R, S, generator=g, **f) + torch.arange(S, device='cuda')) / S * 2.5 + 0.5).contiguous()
    M = R * S
    acts_floats, _ = ops.nerf_workspace(M, R)
    work_floats = ops.nerf_infer_workspace(M, R)
    fixed = 2 * ops.nerf_infer_workspace(1, 1) - ops.nerf_infer_workspace(2, 1)
    acts, work = torch.empty(acts_floats, **f), torch.empty(work_floats, **f)
    count = torch.tensor([M], dtype=torch.int32, device='cuda')
    out = [(torch.empty(M, 3, **f), torch.empty(M, **f)) for _ in range(2)]
    bands = net.band_weights()
    fwd = lambda: ops.nerf_fwd(net.flat, center, ray, depth, bands, count, R, S, acts, out[0][0], out[0][1], net.ctx)
    inf = lambda: ops.nerf_infer(net.flat, center, ray, depth, bands, count, R, S, work, out[1][0], out[1][1], net.ctx)
    t_fwd, t_inf = alternated([fwd, inf], runs)
    same = torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    per_fwd, per_inf = 4 * acts_floats / M, 4 * (work_floats - fixed) / M
    return [f'{R} rays x {S} samples = {M} samples (outputs bit-identical: {same})',
            f'  pp_nerf_fwd    {fmt(t_fwd)}   workspace {4 * acts_floats / 2 ** 20:9.1f} MiB = {per_fwd:7.1f} bytes per sample',
            f'  pp_nerf_infer  {fmt(t_inf)}   workspace {4 * work_floats / 2 ** 20:9.1f} MiB = {per_inf:7.1f} bytes per sample + {4 * fixed} fixed',
            f'  infer median / fwd median = {t_inf[0] / t_fwd[0]:.3f}; infer median {"<=" if t_inf[0] <= t_fwd[1] else ">"} fwd minimum '
            f'({t_inf[0]:.3f} against {t_fwd[1]:.3f} ms)']


def renderer(S=128, Sf=128):
    opt = bg_nerf.default_options(sample_intvs=S)
    opt.nerf.fine_sampling, opt.nerf.sample_intvs_fine = True, Sf
    torch.manual_seed(2)
    sr = bg_nerf.SceneRenderer(opt, device='cuda')
    sr.nerf.progress.data.fill_(1.0)
    sr.nerf_fine.progress.data.fill_(1.0)
    return sr, opt


def whole_view(sr, opt, H, W, runs):
    views = syn.make_views(1, 8, 8, seed=5)
    pose = torch.tensor(views['w2c'][:1, :3, :4]).float().cuda()
    K = torch.tensor(syn.intrinsics(1, H, W)).float().cuda()
    res = {}
    slices = lambda: res.__setitem__('s', sr.render_by_slices(opt, pose, H, W, K, DEPTH_RANGE, mode='val'))
    view = lambda: res.__setitem__('v', sr.render_view(opt, pose, H, W, K, DEPTH_RANGE, mode='val'))
    t_s, t_v = alternated([slices, view], runs)
    d = float((res['s']['rgb_fine'] - res['v']['rgb_fine']).abs().max())
    n_s, n_v = -(-H * W // opt.nerf.rand_rays), -(-H * W // 8192)
    return [f'{H} x {W} view, coarse {opt.nerf.sample_intvs} + fine {opt.nerf.sample_intvs_fine} samples per ray '
            f'(largest |rgb_fine| difference between the two paths, whose chunks differ: {d:.2e})',
            f'  render_by_slices, rand_rays {opt.nerf.rand_rays} ({n_s} slices)  {fmt(t_s)}',
            f'  render_view, chunk_rays 8192 ({n_v} chunks)        {fmt(t_v)}',
            f'  render_by_slices / render_view = {t_s[0] / t_v[0]:.2f}']


def sequence(sr, opt, H, W):
    views = syn.make_views(3, 8, 8, seed=7)
    w2c = torch.tensor(views['w2c'][:, :3, :4]).float().cuda()
    K = torch.tensor(syn.intrinsics(1, H, W)).float().cuda()
    gen_videos.render_novel_views(sr, opt, w2c, K, H, W, DEPTH_RANGE, dataset='dtu', n_frames=1)       # warm-up: two frames
    torch.cuda.synchronize()
    out = {}
    t = _once(lambda: out.update(gen_videos.render_novel_views(sr, opt, w2c, K, H, W, DEPTH_RANGE, dataset='dtu', n_frames=60)))
    F = out['rgb'].shape[0]
    return [f'{F}-frame DTU novel-view sequence at {H} x {W} (render_novel_views, n_frames = 60): {t:.1f} ms = {t / F:.2f} ms per frame (one call)']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scene_view.txt'))
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--skip-large', action='store_true')
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    fh = open(a.out, 'w')

    def emit(lines):
        for l in lines:
            print(l, flush=True)
            fh.write(l + '\n')
        fh.flush()

    emit([f'Forward-only scene rendering on {torch.cuda.get_device_name(0)}: medians of {a.runs} calls (min .. max), each between two stream '
          'events after one warm-up call per path, paths alternated, one process', '',
          '1. sample stage: pp_nerf_infer against pp_nerf_fwd'])
    emit(sample_stage(3072, 128, a.runs))
    emit(sample_stage(8192, 256, a.runs))
    sr, opt = renderer()
    emit(['', '2. one whole view'])
    emit(whole_view(sr, opt, 400, 400, a.runs))
    if not a.skip_large:
        emit(whole_view(sr, opt, 1200, 1600, a.runs))
    emit(['', '3. novel views'])
    emit(sequence(sr, opt, 400, 400))
    fh.close()


if __name__ == '__main__':
    main()
