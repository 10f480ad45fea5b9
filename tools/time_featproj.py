"""Cost of the surface-projection feature term (lib/recon_scene.py:371-439, :610-619) at the bench workload (160^3 grid, 3 x 400 x 400
views, 1024 object rays; scene branch: rand_rays // 3 pixels per view x 128 samples, coarse phase) with 256 rays of view 0 per step
and one feature layer of 256 channels at H / 4 x W / 4 (a smooth random field plus noise).  Legs:

    none       joint.DualBranchEngine.train_step without the term (engine built without featproj_rows)
    native     train_step(featproj=...): TrainEngine.surface_projection_grads
    pass       surface_projection_grads alone, on the state a step left
    kernels    the new launches alone (pp_featproj_reproject + the three of pp_featproj_loss) on the buffers a pass left

All legs live in ONE process and are timed alternately, a block of steps each per round, device events around each block; the
median over the rounds is reported per leg with the minimum and maximum.  The kernels' must-move bytes: eight taps of C floats
per valid row and layer (the rays, flags and gradients are a few KB); achieved bytes / s = that over the kernels' time.

    python tools/time_featproj.py [--rounds 5] [--steps 20] [--warmup 5] [--out FILE]

Needs a GPU: there is no CPU timing path.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.time_deterministic import H, W, V, N, build, draws       # noqa: E402  (the bench workload's object engine)

ROWS, C_FEAT, S_SCENE = 256, 256, 128
NL, WEIGHT = 0.05, 1e-3                                              # configs/dtu_e2e: weight_surface_projection = 0.001
PAIRS = ((0, 1), (1, 2), (0, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from poseprobe_amd import bg_nerf, ops
    from poseprobe_amd.joint import DualBranchEngine
    dev = 'cuda'
    opt = bg_nerf.default_options(sample_intvs=S_SCENE)

    def joint_of(eng):
        torch.manual_seed(0)
        net = bg_nerf.NeRF(opt, device=dev)
        net.progress.data.fill_(0.5)
        return DualBranchEngine(eng, net, lr_scene=1e-3, depth_range=(0.5, 3.0))

    before = torch.cuda.memory_allocated()
    plain = build()
    one_engine = torch.cuda.memory_allocated() - before
    native = build(featproj_rows=ROWS)
    workspaces = torch.cuda.memory_allocated() - before - 2 * one_engine
    g = torch.Generator().manual_seed(1)
    feat = F.interpolate(torch.randn(V, C_FEAT, 8, 8, generator=g), size=(H // 4, W // 4), mode='bilinear', align_corners=True)
    feat = (feat + 0.05 * torch.randn(feat.shape, generator=g)).to(dev)
    native.set_feature_maps([feat])
    joints = {'plain': joint_of(plain), 'native': joint_of(native)}
    rays = draws(a.steps)
    n_pix = opt.nerf.rand_rays // V
    px = [(torch.rand(n_pix, 2, generator=g) * torch.tensor([W - 1., H - 1.])).to(dev) for _ in range(a.steps)]
    img = torch.rand(V, n_pix, 3, generator=g).to(dev)
    gs = 10
    rng = np.random.RandomState(0)
    gen = torch.Generator(device=dev).manual_seed(2)

    def rows():
        flat = torch.randperm(H * W, device=dev, generator=gen)[:ROWS]
        i, j = PAIRS[rng.randint(len(PAIRS))]
        pix = torch.stack([(flat % W).float() + 0.5, (flat // W).float() + 0.5], -1).contiguous()
        return dict(src=torch.zeros(ROWS, dtype=torch.int32, device=dev), pix=pix, own=i, other=j)

    def kernels():
        e, ws, wb, fp = native, native.ws_featproj, native.ws_featproj_ref, native._fp
        ops.featproj_reproject(ROWS, 1, ws.rays_o, ws.rays_d, ws.t_min, ws.depth_acc, e.intr, e.w2c, NL, fp['own_ref'], fp['pix_ref'])
        ops.featproj_loss(ROWS, 0, 1, ws.rays_o, ws.rays_d, ws.t_min, ws.depth_acc, wb.rays_o, wb.rays_d, wb.t_min, wb.depth_acc,
                          e.intr, e.w2c, NL, e.cfg.voxel_size, H, W, e.feature_maps, WEIGHT, e.loss_scale, fp['terms'], fp['valid'],
                          fp['cos'], fp['g_q'], fp['g_depth'], fp['g_o'], fp['g_d'], fp['g_w2c'])

    def step(which, s, **kw):
        idx, jit = rays[s]
        joints[which].train_step(idx, jit, gs, px[s], img, **kw)

    legs = {'none': lambda s: step('plain', s),
            'native': lambda s: step('native', s, featproj=dict(rows=rows(), weight=WEIGHT, nl=NL)),
            'pass': lambda s: native.surface_projection_grads(rows(), gs, WEIGHT, NL),
            'kernels': lambda s: kernels()}
    for leg, f in legs.items():
        for s in range(a.warmup):
            f(s)
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        native.zero_grads()                                          # the pass and kernels legs ran without an optimiser step
        for leg, f in legs.items():
            if leg == 'kernels':                                     # on a pass whose pair is the one the kernels are called with
                native.surface_projection_grads(dict(rows(), own=0, other=1), gs, WEIGHT, NL)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for s in range(a.steps):
                f(s)
            t1.record()
            t1.synchronize()
            ms[leg].append(t0.elapsed_time(t1) / a.steps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    n_valid = float(native._fp['terms'][1])
    must_move = n_valid * 8 * C_FEAT * 4
    res = {'workload': f'160^3 grid, {V} x {H} x {W} views, {N} object rays, scene branch {V} x {n_pix} rays x {S_SCENE} samples '
                       f'(coarse phase), {ROWS} rows, one layer of {C_FEAT} channels at {H // 4} x {W // 4}',
           'steps_per_block': a.steps, 'rounds': a.rounds, 'ms_median': med, 'ms_min_max': {k: [min(v), max(v)] for k, v in ms.items()},
           'term_cost_ms': {'native': med['native'] - med['none']},
           'kernels_share_of_the_pass': med['kernels'] / med['pass'], 'n_valid_at_the_kernels_leg': n_valid,
           'must_move_bytes': must_move, 'achieved_GB_per_s': must_move / (med['kernels'] * 1e-3) / 1e9,
           'workspaces_MB': workspaces / 2 ** 20, 'object_samples_per_ray': native.cfg.n_samples,
           'last_native_terms': {k: v.tolist() for k, v in native.last_featproj_terms.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
