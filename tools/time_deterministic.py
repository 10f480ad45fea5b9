"""Step time of TrainEngine(deterministic=True) against the default engine and against deterministic_scatter=True alone, at the
bench workload (160^3 grid, 3 x 400 x 400 views, 1024 rays).  The engines live in ONE process and are timed alternately, a block
of steps each per round, with device events around each block; the median over the rounds is reported per engine.

    python tools/time_deterministic.py [--rounds 7] [--steps 40] [--warmup 10] [--out FILE]

With --evidence the tool instead runs the reproducibility experiment of tests/test_hip_deterministic.py with
deterministic_scatter=True alone (two engines, 3 steps, same draws) and prints whether the MLP weights still agree bit for bit.
Needs a GPU: there is no CPU timing path.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

G, H, W, V, N = 160, 400, 400, 3, 1024


def build(**kw):
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    from poseprobe_amd.params_init import reference_like_params
    cfg = SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, out_range=float(syn.range_shape().max()))
    views = syn.make_views(V, H, W)
    eng = TrainEngine(cfg, V, H, W, N, pose_iters=3000, **kw)
    eng.set_views(views['images'], views['masks'], views['Ks'], views['w2c'])
    P = reference_like_params(cfg, 3)
    eng.load_reference_params(P['k0'], P['sdf'], P['sdf_alpha'], P['sdf_beta'], P['rgbnet'], P['warp'],
                              se3=torch.tensor(syn.se3_perturbation(V)))
    eng.zero_grads()
    return eng


def draws(n, first_seed=2000):
    from poseprobe_amd import synthetic as syn
    out = []
    for s in range(n):
        idx, jit = syn.step_randomness(V * H * W, N, seed=first_seed + s)
        out.append((torch.tensor(idx, dtype=torch.int32, device='cuda'), torch.tensor(jit, device='cuda')))
    return out


def evidence():
    rays = draws(3, 40)
    data = []
    for _ in range(2):
        eng = build(deterministic_scatter=True)
        for s, (idx, jit) in enumerate(rays):
            eng.train_step(idx, jit, 10 + s)
        torch.cuda.synchronize()
        data.append((eng.flat.data.clone(), eng.k0_cl.clone()))
        del eng
    (fa, ka), (fb, kb) = data
    print(json.dumps({'engines': 'deterministic_scatter=True only', 'steps': 3, 'flat.data_bit_equal': bool(torch.equal(fa, fb)),
                      'flat.data_entries_differing': int((fa != fb).sum()), 'k0_bit_equal': bool(torch.equal(ka, kb)),
                      'k0_entries_differing': int((ka != kb).sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--evidence', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    if a.evidence:
        return evidence()
    engines = {'default': build(), 'deterministic_scatter': build(deterministic_scatter=True), 'deterministic': build(deterministic=True)}
    rays = draws(a.steps)
    gs = 10
    for eng in engines.values():
        for idx, jit in rays[:a.warmup]:
            eng.train_step(idx, jit, gs)
    torch.cuda.synchronize()
    ms = {k: [] for k in engines}
    for _ in range(a.rounds):
        for name, eng in engines.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for idx, jit in rays:
                eng.train_step(idx, jit, gs)
            t1.record()
            t1.synchronize()
            ms[name].append(t0.elapsed_time(t1) / a.steps)
    res = {'workload': f'{G}^3 grid, {V} x {H} x {W} views, {N} rays', 'steps_per_block': a.steps, 'rounds': a.rounds,
           'ms_per_step_median': {k: statistics.median(v) for k, v in ms.items()},
           'ms_per_step_min_max': {k: [min(v), max(v)] for k, v in ms.items()},
           'ordered_workspace_MB': engines['deterministic']._ordered_work.numel() / 2 ** 20}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
