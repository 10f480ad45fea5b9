"""Joint step time with the reprojection + near-surface terms (lib/recon_scene.py:621-637), at the bench workload (160^3 grid,
3 x 400 x 400 views, 1024 object rays; scene branch: rand_rays // 3 pixels per view x 128 samples, coarse phase) with 512
synthetic matches per view pair - surface voxels of the SDF template projected into both views of the pair.  Legs, every one a
joint.DualBranchEngine.train_step:

    none               no reprojection term (the default step; engine built without reproj_rows)
    native_crossing    train_step(reproj=dict(mode='crossing', ...)): TrainEngine.reprojection_grads
    native_render      train_step(reproj=dict(mode='render', ...))

All legs live in ONE process and are timed alternately, a block of steps each per round, device events around each block; the
median over the rounds is reported per leg, with the minimum and maximum (the run-to-run spread).  The native pass costs a
second render workspace; its size is reported.

    python tools/time_reprojection.py [--rounds 3] [--steps 20] [--warmup 5] [--out FILE]

Needs a GPU: there is no CPU timing path.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.time_deterministic import H, W, V, N, build, draws       # noqa: E402  (the bench workload's object engine)

MATCHES, S_SCENE = 512, 128
NL, W_PROJ, W_NEAR, THRE = 0.05, 1e-3, 1e-1, 200                     # configs/dtu_e2e/scan1.py:60-61


def surface_matches(eng, seed=0):
    """(i, j, coord_i, coord_j, conf) for the pairs (0, 1), (1, 2), (0, 2): MATCHES voxels where the template changes sign along
    x, projected with the engine's INITIAL poses and intrinsics (the refinement then moves the pose away from the matches)."""
    from poseprobe_amd import synthetic as syn
    sdf = eng.sdf.cpu().numpy()
    ix, iy, iz = np.nonzero(np.signbit(sdf[:-1]) != np.signbit(sdf[1:]))
    rng = np.random.RandomState(seed)
    lo, hi, size = syn.XYZ_MIN.astype(np.float64), syn.XYZ_MAX.astype(np.float64), np.array(sdf.shape) - 1
    K = eng.intr.cpu().numpy().astype(np.float64)
    w2c = eng.w2c_init.cpu().numpy().astype(np.float64)
    pairs = []
    for i, j in ((0, 1), (1, 2), (0, 2)):
        pick = rng.choice(ix.shape[0], 4 * MATCHES, replace=False)
        p = lo + (np.stack([ix[pick] + 0.5, iy[pick], iz[pick]], -1) / size) * (hi - lo)
        px = []
        for v in (i, j):
            q = p @ w2c[v, :, :3].T + w2c[v, :, 3]
            px.append(np.stack([K[v, 0] * q[:, 0] / q[:, 2] + K[v, 2], K[v, 1] * q[:, 1] / q[:, 2] + K[v, 3]], -1))
        ok = np.all([(c[:, 0] > 0) & (c[:, 0] < W - 1) & (c[:, 1] > 0) & (c[:, 1] < H - 1) for c in px], axis=0)
        sel = np.nonzero(ok)[0][:MATCHES]
        assert sel.shape[0] == MATCHES, 'too few surface voxels project into both views'
        t = lambda a: torch.tensor(a[sel], dtype=torch.float32)
        pairs.append((i, j, t(px[0]), t(px[1]), torch.tensor(rng.rand(MATCHES), dtype=torch.float32)))
    return pairs


def rows_of(pair, dev):
    i, j, ci, cj, conf = pair
    n = ci.shape[0]
    full = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)
    return dict(own=torch.cat([full(j), full(i)]), other=torch.cat([full(i), full(j)]), pix=torch.cat([cj, ci]).to(dev).contiguous(),
                match=torch.cat([ci, cj]).to(dev).contiguous(), conf=torch.cat([conf, conf]).to(dev).contiguous())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from poseprobe_amd import bg_nerf
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
    native = build(reproj_rows=2 * MATCHES)
    second_ws = torch.cuda.memory_allocated() - before - 2 * one_engine
    pairs = surface_matches(plain)
    joints = {'plain': joint_of(plain), 'native': joint_of(native)}
    rows = {(p[0], p[1]): rows_of(p, dev) for p in pairs}
    rng = np.random.RandomState(0)
    rays = draws(a.steps)
    g = torch.Generator().manual_seed(1)
    n_pix = opt.nerf.rand_rays // V
    px = [(torch.rand(n_pix, 2, generator=g) * torch.tensor([W - 1., H - 1.])).to(dev) for _ in range(a.steps)]
    img = torch.rand(V, n_pix, 3, generator=g).to(dev)
    gs = 10

    def native_kw(mode):
        live = [p for p in pairs if mode == 'render' or (p[0] < 2 and p[1] < 2)]
        p = live[rng.randint(len(live))]
        return dict(reproj=dict(rows=rows[(p[0], p[1])], mode=mode, weight_projection=W_PROJ, weight_near_surface=W_NEAR, nl=NL,
                                pixel_thre=THRE))

    legs = {'none': ('plain', lambda: {}),
            'native_crossing': ('native', lambda: native_kw('crossing')),
            'native_render': ('native', lambda: native_kw('render'))}

    def block(leg, n):
        which, kw = legs[leg]
        for s in range(n):
            idx, jit = rays[s]
            joints[which].train_step(idx, jit, gs, px[s], img, **kw())

    for leg in legs:
        block(leg, a.warmup)
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for leg in legs:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            block(leg, a.steps)
            t1.record()
            t1.synchronize()
            ms[leg].append(t0.elapsed_time(t1) / a.steps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    terms = {k: float(v) for k, v in native.last_reproj_terms.items()}
    res = {'workload': f'{160}^3 grid, {V} x {H} x {W} views, {N} object rays, scene branch {V} x {n_pix} rays x {S_SCENE} samples '
                       f'(coarse phase), {MATCHES} matches per pair = {2 * MATCHES} rows',
           'steps_per_block': a.steps, 'rounds': a.rounds, 'ms_per_step_median': med,
           'ms_per_step_min_max': {k: [min(v), max(v)] for k, v in ms.items()},
           'term_cost_ms': {k: med[k] - med['none'] for k in med if k != 'none'},
           'second_workspace_MB': second_ws / 2 ** 20, 'object_samples_per_ray': native.cfg.n_samples,
           'last_native_terms': terms}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
