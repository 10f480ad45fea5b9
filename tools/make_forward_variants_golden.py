"""Writes tests/golden/forward_variants_g24.npz: a recorded run of the reference's own Voxurf.forward / Voxurf.inference on the
two branches beside the default one.

    python tools/make_forward_variants_golden.py /path/to/reference --seed 7 --global-step 7000 --sdf-alpha 0.05    (the committed file)
    python tools/make_forward_variants_golden.py /path/to/reference --seed S --scan N ...      (conditions of seeds S .. S + N - 1)

The reference's Python is executed on the CPU under the stubs of oracle.ref_harness, on the `g24` scene of oracle.make_golden
(24^3 grid, 3 views of 32 x 32, seeded parameters, injected jitter), 192 rays.  Three cases (tests/forward_variants_reference.py
names them): use_deform=False | fast_color_thres=1e-3 with use_deform=True | both.  Stored, data only:
  seed, sdf_alpha, P.checksum         the parameters are regenerated from the seed by the tests (R.fixture_params); see setup()
  se3, ray_idx, jitter, images, masks, Ks, w2c_init, global_step, rays_o, ...     the inputs (as forward_g24_*.npz stores them)
  samples.pts / .ray_id / .step       the in-box samples of the reference's sampler (the restatement check starts from them)
  <case>.out.<key>                    the returned dict; <case>.keys its key list
  <case>.kept                         indices (into the in-box samples) of the samples that pass the threshold
  <case>.loss, <case>.loss.<term>, <case>.grad.<parameter>     the reference's object_losses and the gradients of 0.1 x its total
  inference.out.<key>                 Voxurf.inference on the same rays with fast_color_thres=1e-3, inference.kept likewise
The threshold decision is discontinuous: the tool REFUSES to write unless no reference weight lies within a relative 1e-3 of the
threshold (forward and inference), at least one ray keeps nothing, at least one keeps every sample and at least one misses the box.
--scan prints, for a range of seeds, which of these hold (to choose --seed)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from tests import forward_variants_reference as R      # noqa: E402

G, H, W, NV, N_RAND, THRES, MARGIN = 24, 32, 32, 3, 192, 1e-3, 1e-3


def setup(ref_root, seed, sdf_alpha):
    """sdf_alpha: the raw value of the mapping's amplitude parameter, in place of the seeded set's 10.  With 10 the mapped SDF
    saturates the NeuS sigmoid everywhere but in a thin band at the surface: every sample in front of the band has alpha = 1e-5, far
    below any threshold, and no ray of the scene can keep all its samples - whatever the seed.  A small amplitude leaves a soft
    density in front of the surface (weights of a few 1e-3: on both sides of the threshold) and rays that graze the box keep all."""
    from oracle import ref_harness
    ref_harness.REF_ROOT = ref_root
    from oracle import make_golden as MG
    from oracle import voxurf_oracle as O
    from poseprobe_amd import synthetic as syn
    V, _, C, L = ref_harness.import_reference()
    views = syn.make_views(NV, H, W, seed=777)
    ray_idx, jitter = syn.step_randomness(NV * H * W, N_RAND, seed=seed)
    se3 = syn.se3_perturbation(NV)
    P = O.init_params(MG.oracle_scene(G), seed=seed)
    P['sdf_alpha'] = torch.tensor([float(sdf_alpha)])
    return dict(MG=MG, V=V, C=C, L=L, views=views, ray_idx=ray_idx, jitter=jitter, se3=se3, P=P, seed=seed)


def run_case(S, use_deform, thres, global_step):
    """One forward + object_losses + backward of the reference -> (out, loss terms, loss, gradients, se3 gradient, extras)."""
    MG, V, C, L = S['MG'], S['V'], S['C'], S['L']
    m = MG.ref_model(V, G, NV, (H, W), S['seed'])
    MG.load_params_into_ref(m, S['P'])
    m.fast_color_thres = thres
    se3_t, w2c, c2w, ro, rd, vd, target, mask = MG.make_rays(V, C, S['views'], S['se3'], S['ray_idx'], H, W)
    jit = torch.tensor(S['jitter']).reshape(-1, 1)
    with MG.patched_rand_like(jit):
        out = m(ro, rd, vd, use_deform=use_deform, global_step=global_step, **R.RENDER_KWARGS)
    cfg = sys.modules['easydict'].EasyDict(weight_main=1., weight_tv_k0=.01, weight_mask=.1)
    terms, _, loss = L.object_losses(out, cfg, target, mask, global_step, 10000, use_deform)
    (loss * 0.1).backward()
    grads = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    # the first composite's weights and the in-box samples, from the reference's own sampler and a threshold-free second run
    m.fast_color_thres = 0
    with torch.no_grad(), MG.patched_rand_like(jit):
        pts, mask_out, step, _, _ = m.sample_ray_ori(rays_o=ro.detach(), rays_d=rd.detach(), is_train=True, **R.RENDER_KWARGS)
    keep = ~mask_out.flatten()
    ray_id = (torch.arange(step.numel()) // step.shape[1])[keep]
    with MG.patched_rand_like(jit):
        first = m(ro, rd, vd, use_deform=use_deform, global_step=global_step, **R.RENDER_KWARGS)   # (the warp branch differentiates its rays)
    extras = dict(pts=pts.reshape(-1, 3)[keep], ray_id=ray_id, step=step.flatten()[keep], first_weights=first['weights'].detach(),
                  rays=(ro, rd, vd, target, mask, w2c, c2w))
    return out, terms, loss, grads, se3_t.grad, extras


def ray_conditions(weights, ray_id, thres, n_rays):
    """-> (margin, rays keeping nothing, rays keeping everything, rays without a sample)."""
    w, r = MG_npy(weights), MG_npy(ray_id)
    n = np.bincount(r, minlength=n_rays)
    k = np.bincount(r[w > thres], minlength=n_rays)
    return R.margin_to_threshold(w, thres), int(((k == 0) & (n > 0)).sum()), int(((k == n) & (n > 0)).sum()), int((n == 0).sum())


def MG_npy(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def run_inference(S, thres):
    MG, V, C = S['MG'], S['V'], S['C']
    m = MG.ref_model(V, G, NV, (H, W), S['seed'])
    MG.load_params_into_ref(m, S['P'])
    _, _, _, ro, rd, vd, _, _ = MG.make_rays(V, C, S['views'], S['se3'], S['ray_idx'], H, W)
    ro, rd, vd = ro.detach(), rd.detach(), vd.detach()
    outs = []
    for t in (0, thres):
        m.fast_color_thres = t
        with torch.no_grad():
            outs.append(m.inference(ro, rd, vd, global_step=None, **R.RENDER_KWARGS))
    # the reference's dict names neither the ray nor the step of a sample: taken from its sampler, as inference takes them (:1104)
    with torch.no_grad():
        _, ray_id, step_id, *_ = m.sample_ray_cuda(rays_o=ro, rays_d=rd, is_train=False, **R.RENDER_KWARGS)
    assert ray_id.shape[0] == outs[0]['weights'].shape[0] > 1
    return outs[0], outs[1], ray_id, step_id     # threshold-free run (its weights decide the mask), thresholded run, the samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('reference_root')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'forward_variants_g24.npz'))
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--global-step', type=int, default=7000)
    ap.add_argument('--sdf-alpha', type=float, default=10.0, help='raw sdf_alpha of the parameter set (see setup)')
    ap.add_argument('--scan', type=int, default=0, help='try seeds [seed, seed + SCAN) and print the conditions; writes nothing')
    a = ap.parse_args()
    gs = a.global_step
    if a.scan:
        for seed in range(a.seed, a.seed + a.scan):
            S = setup(a.reference_root, seed, a.sdf_alpha)
            line = [f'seed {seed}:']
            for name in R.CASES:
                deform, _ = R.CASE_SWITCHES[name]
                *_, ex = run_case(S, deform, 0.0, gs)
                mg, none, every, miss = ray_conditions(ex['first_weights'], ex['ray_id'], THRES, N_RAND)
                line.append(f'{name}: margin {mg:.2e} none {none} all {every} miss {miss} |')
            first, _, ray_id, _ = run_inference(S, THRES)
            mg, none, every, miss = ray_conditions(first['weights'], ray_id, THRES, N_RAND)
            line.append(f'inference: margin {mg:.2e} none {none} all {every} miss {miss}')
            print(' '.join(line), flush=True)
        return
    S = setup(a.reference_root, a.seed, a.sdf_alpha)
    MG = S['MG']
    npy = MG.npy
    # the parameters are regenerated from the seed on the test side (R.fixture_params); their checksums travel
    d = {'P.checksum': np.array([float(v.double().abs().sum()) for v in R.flat_params(S['P'])])}
    views = S['views']
    d.update(G=G, H=H, W=W, n_rand=N_RAND, global_step=gs, seed=a.seed, sdf_alpha=np.float32(a.sdf_alpha), thres=np.float64(THRES), ray_idx=S['ray_idx'],
             jitter=S['jitter'], se3=S['se3'], images=views['images'], masks=views['masks'], Ks=views['Ks'], w2c_init=views['w2c'])
    for name in R.CASES:
        deform, thres = R.CASE_SWITCHES[name]
        out, terms, loss, grads, g_se3, ex = run_case(S, deform, thres, gs)
        M = ex['pts'].shape[0]
        assert M % 64 != 0 and M % 4096 != 0, f'{M} in-box samples: a multiple of the tile'
        if thres > 0:
            mg, none, every, miss = ray_conditions(ex['first_weights'], ex['ray_id'], thres, N_RAND)
            print(f'{name}: {M} samples, margin to the threshold {mg:.3e}; rays keeping nothing {none}, everything {every}, '
                  f'missing the box {miss}')
            assert mg > MARGIN, f'{name}: a reference weight lies within {MARGIN} (relative) of the threshold - choose another seed'
            assert none >= 1 and every >= 1 and miss >= 1, f'{name}: needs a ray of each kind - choose another seed'
            kept = np.nonzero(npy(ex['first_weights']) > thres)[0].astype(np.int32)
            assert np.array_equal(npy(out['mask']), npy(ex['first_weights']) > thres)
            assert out['weights'].shape[0] == kept.shape[0] == out['gradient'].shape[0]
            d[f'{name}.kept'] = kept
        if name == 'plain':
            ro, rd, vd, target, mask, w2c, c2w = ex['rays']
            d.update({'samples.pts': npy(ex['pts']), 'samples.ray_id': npy(ex['ray_id']).astype(np.int32), 'samples.step': npy(ex['step']),
                      'rays_o': npy(ro), 'rays_d': npy(rd), 'viewdirs': npy(vd), 'target': npy(target), 'mask_px': npy(mask),
                      'w2c': npy(w2c), 'c2w': npy(c2w)})
        d[f'{name}.keys'] = np.array(sorted(out.keys()))
        for k, v in out.items():
            if k == 's_val':
                d[f'{name}.out.s_val'] = np.float64(v)
            elif v is not None:
                d[f'{name}.out.{k}'] = npy(v)
        d[f'{name}.loss'] = npy(loss)
        for k, v in terms.items():
            d[f'{name}.loss.{k}'] = npy(v)
        d[f'{name}.grad.se3'] = npy(g_se3)
        # colour-grid gradient: at its 256 largest entries' voxels + 256 other touched voxels, + its sums (as forward_ref96.npz)
        gk = grads['k0.grid'][0]
        per_voxel = gk.abs().amax(0).flatten()
        touched = torch.nonzero(per_voxel > 0).flatten()
        other = touched[torch.tensor(np.random.RandomState(5).permutation(touched.numel())[:256])]
        vox = torch.unique(torch.cat([torch.topk(per_voxel, 256).indices, other]))
        d[f'{name}.k0g.voxels'], d[f'{name}.k0g.values'] = vox.numpy().astype(np.int32), npy(gk.reshape(12, -1)[:, vox].T.contiguous())
        d[f'{name}.k0g.n_touched'] = np.int32(touched.numel())
        d[f'{name}.k0g.sum'], d[f'{name}.k0g.abs_sum'] = np.float64(gk.double().sum()), np.float64(gk.double().abs().sum())
        d[f'{name}.grad.sdf_alpha'], d[f'{name}.grad.sdf_beta'] = npy(grads['sdf_alpha']), npy(grads['sdf_beta'])
        # MLP gradients: every R.GRAD_ROW_STEP-th row of a weight matrix (all of a matrix with fewer rows), every bias
        rows = lambda t: npy(t if t.shape[0] < R.GRAD_ROW_STEP else t[::R.GRAD_ROW_STEP])
        for li, key in enumerate(['rgbnet.0', 'rgbnet.2.0', 'rgbnet.3.0', 'rgbnet.4']):
            d[f'{name}.grad.rgbnet.{li}.weight'], d[f'{name}.grad.rgbnet.{li}.bias'] = rows(grads[key + '.weight']), npy(grads[key + '.bias'])
        warp = [k for k in grads if k.startswith('warp_network.deform_net')]
        assert bool(warp) == deform, 'the warp net receives a gradient exactly when it runs'
        for li in range(5 if deform else 0):
            pre = f'warp_network.deform_net.net.net.{li}.0'
            d[f'{name}.grad.warp.{li}.weight'], d[f'{name}.grad.warp.{li}.bias'] = rows(grads[pre + '.weight']), npy(grads[pre + '.bias'])
        print(f'{name}: loss {float(loss):.6f}, dict keys {len(out)}, kept {out["weights"].shape[0]} of {M}')
    first, out, ray_id, step_id = run_inference(S, THRES)
    mg, none, every, miss = ray_conditions(first['weights'], ray_id, THRES, N_RAND)
    Mi = first['weights'].shape[0]
    print(f'inference: {Mi} samples, margin {mg:.3e}; rays keeping nothing {none}, everything {every}, missing the box {miss}')
    assert mg > MARGIN, 'inference: a reference weight lies within the margin of the threshold - choose another seed'
    assert Mi % 64 != 0 and Mi % 4096 != 0
    kept = np.nonzero(npy(first['weights']) > THRES)[0]
    assert out['weights'].shape[0] == kept.shape[0]
    d['inference.kept'] = kept.astype(np.int32)
    d['inference.ray_id'], d['inference.step_id'] = npy(ray_id)[kept].astype(np.int32), npy(step_id)[kept].astype(np.int32)
    d['inference.n_samples'] = np.int32(Mi)
    for k, v in out.items():
        if k == 's_val':
            d['inference.out.s_val'] = np.float64(v)
        elif v is not None:
            d['inference.out.' + k] = npy(v)
    np.savez_compressed(a.out, **d)
    print(a.out, os.path.getsize(a.out) // 1024, 'KB')


if __name__ == '__main__':
    main()
