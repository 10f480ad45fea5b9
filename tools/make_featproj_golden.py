"""Writes tests/golden/featproj_g24.npz: a recorded run of the reference's own get_project_feature_loss.

    python tools/make_featproj_golden.py /path/to/reference [--seed S] [--scan N]

The body of get_project_feature_loss (lib/recon_scene.py:371-439) and of get_ray_dir (:93-113) is compiled from the reference's
source at run time under the stubs of oracle.ref_harness, as oracle/make_golden.py does for get_project_error; nothing of it is
stored.  It runs on the reference's Voxurf with the `g24` parameter set (24^3 grid, three views of 32 x 32, seed 23 - the set
reproj_g24.npz stores, regenerated from the seed by the tests), global_step 50, the view pair (1, 2), 96 rays of view 0 (the
reference always shoots from the first training view), two feature layers (256, 8, 8) and (20, 11, 7) that
tests/featproj_reference.py rebuilds from the case name.  torch.randperm and torch.rand_like are patched to recorded draws.
Stored, data only: the draws (pixel indices, the two jitter vectors), se3 / w2c_init / Ks, the loss, d loss / d se3, the per-row
flags (hit of both queries, valid), the rays, entry distances and weighted step sums of both queries (the float64 restatement starts from
them) and the parameter checksums.
The flags are discontinuous: the tool REFUSES to write if any row lies within a relative 1e-3 of a decision (|p - p_ref| against
2 voxels, max(|x|, |y|) against 1, q_z against nl, acc against 0) or if fewer than 16 rows are valid, and prints how many rows
each cause rejects.  --scan N tries the seeds [S, S + N) and prints these figures; it writes nothing."""
import argparse
import ast
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from tests import featproj_reference as R      # noqa: E402

CASE, PAIR, NL = 'featproj_g24', (1, 2), 0.05


class patched_draws:
    """torch.randperm returns the recorded pixel indices, successive torch.rand_like calls the recorded jitter vectors."""

    def __init__(self, perm, jitters):
        self.perm, self.jitters = perm, list(jitters)

    def __enter__(self):
        self.orig = torch.randperm, torch.rand_like
        torch.randperm = lambda n, **kw: self.perm.clone()

        def rand_like(x, *a, **k):
            j = self.jitters.pop(0)
            assert x.shape == j.shape, (x.shape, j.shape)
            return j.clone()
        torch.rand_like = rand_like

    def __exit__(self, *a):
        torch.randperm, torch.rand_like = self.orig


def run(ref_root, seed, draw=None):
    """draw: (pixel indices, jitter, jitter_ref) of the rows, at most 256 (the reference's own limit, :372)."""
    import einops
    import importlib
    from oracle import ref_harness
    ref_harness.REF_ROOT = ref_root
    from oracle import make_golden as MG
    from poseprobe_amd import synthetic as syn
    V, _, C, _ = ref_harness.import_reference()
    common = importlib.import_module('lib.common')
    path = os.path.join(ref_root, 'lib', 'recon_scene.py')
    nodes = MG._reference_functions(path, {'get_ray_dir': None, 'get_project_feature_loss': 'scene_rep_reconstruction'})
    ns = dict(torch=torch, np=np, einops=einops, camera=C, common=common)
    for node in nodes.values():
        exec(compile(ast.Module(body=[node], type_ignores=[]), path, 'exec'), ns)
    G, H, W, nv = R.G, R.H, R.W, R.NV
    views = syn.make_views(nv, H, W, seed=777)
    P = R.fixture_params()
    m = MG.ref_model(V, G, nv, (H, W), 0)
    MG.load_params_into_ref(m, P)
    perm, jitter, jitter_ref = draw
    n = perm.shape[0]
    se3 = syn.se3_perturbation(nv)
    feats = R.feature_maps(CASE, nv, R.LAYERS)
    se3_t = torch.tensor(se3, requires_grad=True)
    init = torch.tensor(views['w2c'])
    w2c = torch.cat([init[:1], C.pose.compose([C.lie.se3_to_SE3(se3_t), init])[1:]], 0)
    Ks = torch.tensor(views['Ks'])
    HW = np.array([[H, W]] * nv)
    target_tr, _, ro_tr, rd_tr, _, imsz = V.get_training_rays_flatten(
        rgb_tr_ori=torch.tensor(views['images']), mask_tr_ori=torch.tensor(views['masks']), train_poses=C.pose.invert(w2c), HW=HW,
        Ks=Ks, ndc=False, inverse_y=True, flip_x=False, flip_y=False)
    # what the two queries were given and what their sampler found, in call order
    calls = []
    query, sample = m.query_sdf_point_wocuda_render, m.sample_ray_ori

    def sample_rec(**kw):
        out = sample(**kw)
        calls.append(dict(o=kw['rays_o'].detach().clone(), d=kw['rays_d'].detach().clone(), t_min=out[3].detach().clone()))
        return out

    def segment_rec(**kw):                                    # the query's one call: n_step = sum of weight x step per ray (:905-909)
        out = segment(**kw)
        calls[-1]['n_step'] = out.detach().clone()
        return out

    def query_rec(rays_o, rays_d, **kw):
        pts, mask, depth = query(rays_o, rays_d, **kw)
        c = calls[-1]
        c.update(acc=c.pop('n_step') / c['d'].norm(dim=-1), hit=mask.detach().clone())
        assert torch.equal(c['t_min'] + c['acc'], depth.detach()[:, 0])
        return pts, mask, depth
    segment = V.segment_coo
    m.sample_ray_ori, m.query_sdf_point_wocuda_render, V.segment_coo = sample_rec, query_rec, segment_rec
    me = types.SimpleNamespace(model=m, Ks=Ks, HW=HW, nl=NL, render_kwargs=dict(R.RENDER_KWARGS), data_dict={'vgg_features': feats},
                               cfg=types.SimpleNamespace(data=types.SimpleNamespace(inverse_y=True, flip_x=False, flip_y=False)))
    # the reference's own count of valid rows: the length of what it hands to cosine_similarity, once per layer
    seen, cosine = [], torch.cosine_similarity

    def cosine_rec(x, y, **kw):
        seen.append(x.shape[0])
        return cosine(x, y, **kw)
    torch.cosine_similarity = cosine_rec
    try:
        with patched_draws(torch.tensor(perm), [torch.tensor(jitter).reshape(-1, 1), torch.tensor(jitter_ref).reshape(-1, 1)]):
            loss = ns['get_project_feature_loss'](me, R.GS, True, w2c, int(imsz[PAIR[0]]), target_tr, ro_tr, rd_tr, [PAIR[0]], [PAIR[1]])
    finally:
        torch.cosine_similarity, V.segment_coo = cosine, segment
    assert len(calls) == 2 and all(c['o'].shape == (n, 3) for c in calls) and len(seen) == len(R.LAYERS)
    qa, qb = ({k: c[k].double() for k in ('o', 'd', 't_min', 'acc')} for c in calls)
    assert all(torch.equal(q['acc'] > 0, c['hit']) for q, c in ((qa, calls[0]), (qb, calls[1]))), 'acc > 0 is not the hit flag'
    intr = R.intr_of(views['Ks'])
    voxel = float(m.voxel_size)
    dec = R.decisions(qa, qb, w2c.detach(), intr, PAIR[0], PAIR[1], NL, voxel, H, W)
    margin = R.decision_margin(dec, NL)
    rs = R.restate(qa, qb, w2c.detach(), intr, PAIR[0], PAIR[1], NL, voxel, H, W, feats)
    assert set(seen) == {rs['n_valid']}, f'the reference counted {seen} valid rows, the restatement {rs["n_valid"]}'
    counts = {k: int(v.sum()) for k, v in dec['reject'].items()}
    counts['behind'] = int((dec['qz'] < NL).any(-1).sum())
    return dict(loss=loss, se3_t=se3_t, qa=qa, qb=qb, calls=calls, margin=margin, counts=counts, rs=rs, perm=perm, jitter=jitter,
                row_margins=R.row_margins(dec, NL),
                jitter_ref=jitter_ref, se3=se3, views=views, P=P, voxel=voxel, w2c=w2c.detach())


def choose_draw(ref_root, seed):
    """The recorded draw: the first R.ROWS pixels of RandomState(seed)'s permutation of the image whose rows keep twice the margin
    from every decision when the whole image goes through the term (a row's fate depends on its own ray and jitter only), with
    the jitter drawn for them.  Rays that cross the box beside the surface are ties (tests/featproj_reference.row_margins) and
    common: a plain prefix of a permutation never passes."""
    rng = np.random.RandomState(seed)
    n = R.H * R.W
    full = rng.permutation(n).astype(np.int64), rng.rand(n).astype(np.float32), rng.rand(n).astype(np.float32)
    margins = torch.cat([run(ref_root, seed, tuple(t[at:at + 256] for t in full))['row_margins'] for at in range(0, n, 256)])
    keep = np.nonzero((margins > 2 * R.MARGIN).numpy())[0][:R.ROWS]
    if keep.shape[0] < R.ROWS:
        sys.exit(f'refused: only {keep.shape[0]} pixels of the image are clear of every decision')
    return tuple(t[keep] for t in full)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('reference_root')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'featproj_g24.npz'))
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--scan', type=int, default=0, help='try seeds [seed, seed + SCAN) and print the conditions; writes nothing')
    a = ap.parse_args()
    for seed in range(a.seed, a.seed + max(a.scan, 1)):
        S = run(a.reference_root, seed, choose_draw(a.reference_root, seed))
        n_valid = S['rs']['n_valid']
        print(f"seed {seed}: loss {float(S['loss']):.7f} (restated {float(S['rs']['loss']):.7f}), valid rows {n_valid} of {R.ROWS}, "
              f"margin to the nearest decision {S['margin']:.3e}; rows rejected by cause {S['counts']}", flush=True)
    if a.scan:
        return
    if S['margin'] <= R.MARGIN:
        sys.exit(f'refused: a row lies within {R.MARGIN} (relative) of a decision - choose another seed')
    if n_valid < 16:
        sys.exit(f'refused: {n_valid} valid rows, need at least 16 - choose another seed')
    S['loss'].backward()
    npy = lambda t: t.detach().cpu().numpy()
    views = S['views']
    d = dict(G=R.G, H=R.H, W=R.W, global_step=R.GS, seed=seed, pair=np.array(PAIR), nl=np.float32(NL), voxel_size=np.float64(S['voxel']),
             pix_index=S['perm'], jitter=S['jitter'], jitter_ref=S['jitter_ref'], se3=S['se3'], w2c_init=views['w2c'], Ks=views['Ks'],
             w2c=npy(S['w2c']), loss=npy(S['loss']), g_se3=npy(S['se3_t'].grad), valid=npy(S['rs']['valid']),
             hit=npy(S['calls'][0]['hit']), hit_ref=npy(S['calls'][1]['hit']), margin=np.float64(S['margin']))
    d['P.checksum'] = R.param_checksum(S['P'])
    for tag, q in (('a', S['qa']), ('b', S['qb'])):
        for k in ('o', 'd', 't_min', 'acc'):
            d[f'{tag}.{k}'] = npy(q[k]).astype(np.float32)
    np.savez_compressed(a.out, **d)
    print(a.out, os.path.getsize(a.out) // 1024, 'KB')


if __name__ == '__main__':
    main()
