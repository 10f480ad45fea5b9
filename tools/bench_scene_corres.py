"""Times the dual-branch step (joint.DualBranchEngine.train_step) with and without SPARF's correspondence term at the bench's
setup (160^3 grid, 3 views of 400 x 400, 1024 object rays, rand_rays // 3 scene pixels per view x 128 samples) with M = 512
matched pixels of one view pair (rand_rays // 2, the reference's cap): coarse phase and hierarchical phase (coarse + fine
network on 128 + 128 samples).  HIP events around the two new kernels give their own times.  Prints one JSON line.

    python tools/bench_scene_corres.py [--steps 20] [--warmup 3] [--pairs 512]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--pairs', type=int, default=512)
    args = ap.parse_args()
    import numpy as np
    import torch
    from bench import init_engine_params
    from poseprobe_amd import bg_nerf, ops, synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    from poseprobe_amd.joint import DualBranchEngine
    dev = 'cuda:0'
    G, H, W, V, N, M = 160, 400, 400, 3, 1024, args.pairs
    rs = syn.range_shape()
    cfg = SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, out_range=float(rs.max()))
    views = syn.make_views(V, H, W)
    eng = TrainEngine(cfg, V, H, W, N, device=dev, pose_iters=3000)
    eng.set_views(views['images'], views['masks'], views['Ks'], views['w2c'])
    init_engine_params(eng, cfg, seed=3)
    eng.zero_grads()
    opt = bg_nerf.sparf_dtu_options(sample_intvs=128)
    opt.nerf.sample_intvs_fine = 128
    torch.manual_seed(0)
    nets = [bg_nerf.NeRF(opt, device=dev), bg_nerf.NeRF(opt, is_fine_network=True, device=dev)]
    for n in nets:
        n.progress.data.fill_(0.5)
    joint = DualBranchEngine(eng, nets[0], lr_scene=1e-3, depth_range=(0.5, 3.0), scene_net_fine=nets[1])
    g = torch.Generator().manual_seed(1)
    n_pix, total = opt.nerf.rand_rays // V, args.steps + args.warmup
    idx = [torch.randperm(V * H * W, generator=g)[:N].to(torch.int32).to(dev) for _ in range(total)]
    jit = [torch.rand(N, generator=g).to(dev) for _ in range(total)]
    px = [(torch.rand(n_pix, 2, generator=g) * torch.tensor([W - 1., H - 1.])).to(dev) for _ in range(total)]
    img = torch.rand(V, n_pix, 3, generator=g).to(dev)
    ps = (torch.rand(M, 2, generator=g) * torch.tensor([W - 1., H - 1.])).to(dev)
    corres = dict(i=1, j=0, pix_self=ps, pix_other=ps + torch.randn(M, 2, generator=g).to(dev) * 2,
                  conf=torch.rand(M, generator=g).to(dev), weight=1e-2)

    events = {}

    def timed(name, fn):
        def wrapper(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            events.setdefault(name, []).append((e0, e1))
            return r
        return wrapper

    out = {'workload': f'dual-branch step at {G}^3, {V} x {H} x {W}, {N} object rays, {V} x {n_pix} scene rays x 128 samples; '
                       f'+ correspondence term on {M} matched pixels of one pair (union pass of {V * n_pix} + {2 * M} rows)',
           'steps': args.steps}
    for phase, fine in (('coarse_phase', False), ('hierarchical_phase', True)):
        for label, c in (('photometric', None), ('photometric_corres', corres)):
            for s in range(args.warmup):
                joint.train_step(idx[s], jit[s], 100 + s, px[s], img, fine=fine, corres=c)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(args.warmup, total):
                joint.train_step(idx[s], jit[s], 100 + s, px[s], img, fine=fine, corres=c)
            torch.cuda.synchronize()
            out.setdefault(phase, {})[label + '_ms'] = (time.perf_counter() - t0) / args.steps * 1e3
        p = out[phase]
        p['added_ms'] = p['photometric_corres_ms'] - p['photometric_ms']
    # the two new kernels on their own (hierarchical phase: the loss kernel reads both passes)
    orig = ops.nerf_corres_loss, ops.nerf_pair_pose_bwd
    ops.nerf_corres_loss = timed('pp_nerf_corres_loss', ops.nerf_corres_loss)
    ops.nerf_pair_pose_bwd = timed('pp_nerf_pair_pose_bwd', ops.nerf_pair_pose_bwd)
    for s in range(args.warmup, total):
        joint.train_step(idx[s], jit[s], 100 + s, px[s], img, fine=True, corres=corres)
    torch.cuda.synchronize()
    ops.nerf_corres_loss, ops.nerf_pair_pose_bwd = orig
    out['kernels_us'] = {k: float(np.median([a.elapsed_time(b) for a, b in v])) * 1e3 for k, v in events.items()}
    out['corres_term'] = float(joint.last_scene_terms['corres'])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
