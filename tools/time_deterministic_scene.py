"""Step time of bg_nerf.SceneEngine(deterministic=True) against the default engine at the reference's training size (3072 rays x
128 samples; coarse step and hierarchical step with 128 fine samples).  Both engines live in ONE process and are timed alternately,
a block of steps each per round, with device events around each block; the median over the rounds is reported per engine.

    python tools/time_deterministic_scene.py [--rounds 7] [--steps 20] [--warmup 5] [--out FILE]

With --evidence the tool instead runs two DEFAULT joint engines (joint.DualBranchEngine on a deterministic object engine: the object
branch alone would be bit-reproducible) for three steps on the same draws and prints how many entries of the scene network and of
the object engine's flat parameter block differ: the reason the mode exists.  Needs a GPU: there is no CPU timing path.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

R, S, NF = 3072, 128, 128


def build(**kw):
    from poseprobe_amd import bg_nerf
    opt = bg_nerf.default_options(sample_intvs=S)
    opt.nerf.fine_sampling, opt.nerf.sample_intvs_fine = True, NF
    torch.manual_seed(0)
    nets = [bg_nerf.NeRF(opt, is_fine_network=f, device='cuda') for f in (False, True)]
    for n in nets:
        n.progress.data.fill_(0.6)
    return bg_nerf.SceneEngine(nets[0], lr=1e-3, net_fine=nets[1], **kw)


def problem():
    g = torch.Generator().manual_seed(0)
    center = (torch.randn(R, 3, generator=g) * 0.3).cuda()
    ray = torch.randn(R, 3, generator=g).cuda()
    depth = ((torch.rand(R, S, generator=g) + torch.arange(S)) / S * 2.0 + 0.4).cuda().contiguous()
    image = torch.rand(R, 3, generator=g).cuda()
    return center, ray, depth, image, torch.rand(NF + 1, generator=g)


def evidence():
    from poseprobe_amd import bg_nerf
    from poseprobe_amd.joint import DualBranchEngine
    from tools.time_deterministic import H, W, V, build as build_obj, draws
    rays = draws(3, 40)
    g = torch.Generator().manual_seed(1)
    n_px = 1024
    pixels = (torch.rand(n_px, 2, generator=g) * torch.tensor([W - 1., H - 1.])).cuda()
    image = torch.rand(V, n_px, 3, generator=g).cuda()
    rand = [torch.rand(V, n_px, S, 1, generator=g).cuda() for _ in range(3)]
    data = []
    for _ in range(2):
        opt = bg_nerf.default_options(sample_intvs=S)
        torch.manual_seed(0)
        net = bg_nerf.NeRF(opt, device='cuda')
        net.progress.data.fill_(0.6)
        joint = DualBranchEngine(build_obj(deterministic=True), net)
        for s, (idx, jit) in enumerate(rays):
            joint.train_step(idx, jit, 10 + s, pixels, image, depth_rand=rand[s])
        torch.cuda.synchronize()
        data.append((net.flat.clone(), joint.obj.flat.data.clone(), joint.obj.se3.clone()))
        del joint
    (sa, fa, pa), (sb, fb, pb) = data
    print(json.dumps({'engines': 'default DualBranchEngine on TrainEngine(deterministic=True)', 'steps': 3,
                      'scene_flat_entries_differing': int((sa != sb).sum()), 'scene_flat_entries': sa.numel(),
                      'object_flat.data_entries_differing': int((fa != fb).sum()), 'object_flat.data_entries': fa.numel(),
                      'se3_entries_differing': int((pa != pb).sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--evidence', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    if a.evidence:
        return evidence()
    engines = {'default': build(), 'deterministic': build(deterministic=True)}
    center, ray, depth, image, grid = problem()
    res = {'workload': f'{R} rays x {S} samples (+ {NF} fine)', 'steps_per_block': a.steps, 'rounds': a.rounds,
           'ordered_workspace_MB': engines['deterministic']._ordered_work.numel() / 2 ** 20}
    for phase, kw in (('coarse', dict()), ('hierarchical', dict(fine=True, depth_range=(0.4, 2.4), fine_grid=grid))):
        for eng in engines.values():
            for _ in range(a.warmup):
                eng.step(center, ray, depth, image, **kw)
        torch.cuda.synchronize()
        ms = {k: [] for k in engines}
        for _ in range(a.rounds):
            for name, eng in engines.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.steps):
                    eng.step(center, ray, depth, image, **kw)
                t1.record()
                t1.synchronize()
                ms[name].append(t0.elapsed_time(t1) / a.steps)
        res[phase] = {'ms_per_step_median': {k: statistics.median(v) for k, v in ms.items()},
                      'ms_per_step_min_max': {k: [min(v), max(v)] for k, v in ms.items()}}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
