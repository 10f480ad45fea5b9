"""Times the two other branches of Voxurf.forward / Voxurf.inference on one GPU; one JSON line per measurement.

    python tools/time_forward_variants.py view [--root DIR] [--thres T] [--G 160] [--chunk 4096]
        one 400 x 400 view through Voxurf.inference_rays in chunks (the whole-view driver's path): a warm-up view, then ONE timed
        view.  --root: import poseprobe_amd from another checkout (the parent commit, which knows fast_color_thres = 0 only), so
        that a shell loop can alternate builds and thresholds process by process.  With a threshold the kept share of the samples
        is reported from a third, untimed view.
    python tools/time_forward_variants.py kernels [--G 160] [--rays 4096]
        on the samples of one chunk through the middle of the view: k_geometry_fwd (warp output in place) against
        k_geometry_plain_fwd, both backward kernels, and the three launches of the compaction; medians of 100 after 20 warm-ups."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

H = W = 400


def model_and_rays(G, thres):
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd import voxurf_coarse as Model
    rs = syn.range_shape()
    m = Model.Voxurf(syn.XYZ_MIN, syn.XYZ_MAX, num_voxels=G ** 3, num_voxels_base=G ** 3, alpha_init=1e-2, rgbnet_dim=12,
                     rgbnet_direct=True, rgbnet_depth=4, rgbnet_width=128, posbase_pe=5, viewbase_pe=1, geo_rgb_dim=3, s_ratio=50,
                     s_start=0.2, barf_c2f=[0.6, 1], i_train=np.arange(3), N_iters=10000, HW=np.array([[H, W]] * 3), range_shape=rs,
                     rect_size=rs.tolist(), camera_noise=0., fast_color_thres=thres).cuda()
    with torch.no_grad():
        m.k0.grid.normal_(0, 0.1, generator=torch.Generator(device='cuda').manual_seed(0))
    K = torch.tensor(syn.intrinsics(1, H, W)[0]).cuda()
    c2w = torch.eye(4)
    c2w[:3] = torch.tensor(syn.cameras(3)[1])
    c2w = torch.linalg.inv(c2w)[:3].cuda()
    ro, rd, vd = Model.get_rays_of_a_view(H, W, K, c2w, ndc=False, inverse_y=True, flip_x=False, flip_y=False)
    kw = dict(near=syn.NEAR, far=syn.FAR, bg=0, stepsize=1.5, inverse_y=True, flip_x=False, flip_y=False)
    return m, ro.reshape(-1, 3).contiguous(), rd.reshape(-1, 3).contiguous(), vd.reshape(-1, 3).contiguous(), kw


def view(a):
    m, ro, rd, vd, kw = model_and_rays(a.G, a.thres)

    def render(count=False):
        parts, kept, total = [], 0, 0
        with torch.no_grad():
            for b in range(0, H * W, a.chunk):
                parts.append(m.inference_rays(ro[b:b + a.chunk], rd[b:b + a.chunk], vd[b:b + a.chunk], global_step=None, **kw)['rgb_marched'])
                if count:
                    ws = m._ray_cache['ws']
                    total += int(ws.count)
                    kept += int(ws.kept.count) if a.thres > 0 else int(ws.count)
        return torch.cat(parts), kept, total

    render()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    img, _, _ = render()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    _, kept, total = render(count=True)
    print(json.dumps(dict(what='view', root=a.root or '.', G=a.G, chunk=a.chunk, thres=a.thres, ms=round(ms, 3), samples=total,
                          kept_share=round(kept / max(total, 1), 5), mean_rgb=round(float(img.mean()), 6))), flush=True)


def kernels(a):
    from poseprobe_amd import ops
    m, ro, rd, vd, kw = model_and_rays(a.G, 1e-4)
    b = (H // 2) * W - a.rays // 2                       # rows through the middle of the image
    with torch.no_grad():
        m.inference_rays(ro[b:b + a.rays], rd[b:b + a.rays], vd[b:b + a.rays], global_step=None, **kw)
    ws, core = m._ray_cache['ws'], m._core
    sc, cfg, s = core.cfg.pp, core.cfg, ws.kept
    flat = m._flat_params(ro.device)
    sdf, ab = m.sdf.grid[0, 0].contiguous(), flat.view('sdf_ab')
    _, inv_s = m._inv_s(None, False)
    ws.alloc_backward(False)
    s.alloc_backward()
    g_ab = torch.zeros(2, device=ro.device)
    runs = {
        'k_geometry_fwd': lambda: ops.geometry_fwd(sc, sdf, ab, ws.pts, ws.warp_out, ws.viewdirs, ws.ray_id, ws.count, ws.cap, inv_s,
                                                   ws.alpha, ws.gradient, ws.sdf_final, ws.sdf_deform, ws.grad_deform),
        'k_geometry_plain_fwd': lambda: ops.geometry_plain_fwd(sc, sdf, ab, ws.pts, ws.viewdirs, ws.ray_id, ws.count, ws.cap, inv_s,
                                                               ws.alpha, ws.gradient, ws.sdf_final),
        'k_geometry_bwd': lambda: ops.geometry_bwd(sc, sdf, ab, ws.pts, ws.warp_out, ws.viewdirs, ws.ray_id, ws.count, ws.cap, inv_s,
                                                   ws.g_alpha, ws.g_gradient, None, None, None, None, 0, ws.g_warp_out, ws.g_pts,
                                                   ws.g_view_s, g_ab),
        'k_geometry_plain_bwd': lambda: ops.geometry_plain_bwd(sc, sdf, ab, ws.pts, ws.viewdirs, ws.ray_id, ws.count, ws.cap, inv_s,
                                                               ws.g_alpha, ws.g_gradient, None, 0, ws.g_pts, ws.g_view_s, g_ab),
        'keep_compact (3 launches)': lambda: ops.keep_compact(s.weights_all, ws.ray_start, ws.N, ws.cap, 1e-4, ws.pts, ws.ray_id, ws.step,
                                                             ws.alpha, ws.gradient, s.idx, s.ray_start, s.count, s.pts, s.ray_id, s.step,
                                                             s.alpha, s.gradient),
        'keep_scatter_bwd (4 memsets + 1 launch)': lambda: ops.keep_scatter_bwd(s.idx, s.count, ws.cap, s.g_alpha, s.g_gradient, s.g_pts,
                                                                               s.g_view_s, ws.g_alpha, ws.g_gradient, ws.g_pts, ws.g_view_s),
    }
    for t in (ws.g_alpha, ws.g_gradient, s.g_alpha, s.g_gradient, s.g_pts, s.g_view_s):
        t.zero_()
    M, K = int(ws.count), int(s.count)
    for name, fn in runs.items():
        for _ in range(20):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
        for e0, e1 in ev:
            e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
        print(json.dumps(dict(what='kernel', name=name, G=a.G, rays=a.rays, samples=M, kept=K, us_median=round(statistics.median(us), 2),
                              us_min=round(us[0], 2), us_max=round(us[-1], 2))), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=('view', 'kernels'))
    ap.add_argument('--root', default=None)
    ap.add_argument('--thres', type=float, default=0.0)
    ap.add_argument('--G', type=int, default=160)
    ap.add_argument('--chunk', type=int, default=4096)
    ap.add_argument('--rays', type=int, default=4096)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root) if a.root else os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    {'view': view, 'kernels': kernels}[a.what](a)
