"""Times of mesh extraction (poseprobe_amd.mesh) on a 160^3 Voxurf model with the synthetic scene's box and a perturbed warp net,
at lattice resolutions 128, 256 and 512: the device field fill (plain and deform), marching cubes (pp_mc_count, pp_mc_emit) and
the device-to-host copy of the mesh, the connected components of the mesh and the 'largest' filter (pp_cc_*, beside the host round
trip through scipy they replace), and the colour pass over the mesh's vertices (mesh.vertex_attributes: pp_warp_fwd,
pp_vertex_feat, pp_rgbnet_fwd per chunk of 262144 vertices), whole and launch by launch on its first chunk.  Everything runs in ONE process; each stage is warmed up, then timed `--runs` times with
device events (the copy with a host clock around a synchronising copy); medians are reported.

Beside each marching-cubes time: the bytes the stage has to move, from the shapes alone -
  count: the field once (4 N) + one flag byte per point (N)
  emit:  flags twice (2 N) + one vertex base per point written (4 N) + the output (12 Nv + 12 Nt)
(the field and the bases are read again near the surface only; that traffic is not counted)
  colour pass, per vertex: pp_warp_fwd 12 B in + 64 B out; pp_vertex_feat 12 + 64 B in, 256 + 12 B out (the k0 and template
         gathers are served by the caches: vertices arrive in lattice order); pp_rgbnet_fwd 256 B in + 12 B out
- and that figure over the time
as a fraction of the achievable HBM rate of MI355X_MICROARCH.md (6.3 TB/s).  It is a whole-stage rate (launch gaps and the
single-work-group tile scan included), not a kernel's share of peak.

    python tools/time_mesh.py [--resolutions 128 256 512] [--runs 5] [--out FILE]

Needs a GPU: there is no CPU timing path.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

G = 160
HBM_ACHIEVABLE = 6.3e12


def build_model():
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd import voxurf_coarse as Model
    from poseprobe_amd.engine import SceneConfig
    from poseprobe_amd.params_init import reference_like_params
    rs = syn.range_shape()
    m = Model.Voxurf(syn.XYZ_MIN, syn.XYZ_MAX, num_voxels=G ** 3, num_voxels_base=G ** 3, alpha_init=1e-2, rgbnet_dim=12,
                     rgbnet_direct=True, rgbnet_depth=4, rgbnet_width=128, posbase_pe=5, viewbase_pe=1, geo_rgb_dim=3, s_ratio=50,
                     s_start=0.2, barf_c2f=[0.6, 1], i_train=np.arange(3), N_iters=10000, HW=np.array([[400, 400]] * 3),
                     range_shape=rs, rect_size=rs.tolist(), camera_noise=0.)
    P = reference_like_params(SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, out_range=float(rs.max())), 3)
    with torch.no_grad():
        for lin, (Wt, b) in zip(m.warp_network.linears(), P['warp']):      # a non-trivial deformation, as after training
            lin.weight.copy_(Wt)
            lin.bias.copy_(b)
    return m.cuda()


def device_ms(fn, runs, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    return out


def fmt(ms):
    return f'{statistics.median(ms):10.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, {len(ms)} runs)'


def color_launches(m, vw, runs, chunk=262144):
    """The three launches of one chunk of mesh.vertex_attributes (use_deform=True, no activations kept), each timed on its own."""
    from poseprobe_amd import mesh, ops
    from poseprobe_amd.grid import channels_last_view
    cfg = mesh._color_stage_config(m)
    n = min(chunk, vw.shape[0])
    f = dict(dtype=torch.float32, device='cuda')
    pts = vw[:n].contiguous()
    flat, ctx = m._flat_params(pts.device), getattr(m, 'pp_ctx', None)
    m.k0.ensure_layout()
    k0_cl, sdf = channels_last_view(m.k0.grid.detach()), m.sdf.grid.detach()[0, 0].contiguous()
    pe_w = torch.from_numpy(cfg.pe_weights(1.0)).cuda()
    count = torch.full((1,), n, dtype=torch.int32, device='cuda')
    warp_out, normal, feat, rgb = torch.empty(n, 16, **f), torch.empty(n, 3, **f), torch.empty(n, ops.FEAT_LD, **f), torch.empty(n, 3, **f)
    stages = (('pp_warp_fwd', 76, lambda: ops.warp_fwd(flat.view('warp'), pts, count, n, cfg.out_range, None, warp_out, ctx)),
              ('pp_vertex_feat', 344, lambda: ops.vertex_feat(cfg.pp, sdf, flat.view('sdf_ab'), k0_cl, pts, warp_out, pe_w, n, normal, feat)),
              ('pp_vertex_feat, plain', 280, lambda: ops.vertex_feat(cfg.pp, sdf, flat.view('sdf_ab'), k0_cl, pts, None, pe_w, n, normal, feat)),
              ('pp_rgbnet_fwd', 268, lambda: ops.rgbnet_fwd(flat.view('rgbnet'), feat, count, n, None, rgb, ctx)))
    out = [f'one chunk of {n} vertices, launch by launch:']
    for name, per_vertex, fn in stages:
        ms = device_ms(fn, runs)
        rate = per_vertex * n / (statistics.median(ms) * 1e-3)
        out.append(f'{name:28s}  {fmt(ms)}  {per_vertex * n / 2 ** 20:9.1f} MiB to move, {rate / 1e12:.3f} TB/s = '
                   f'{rate / HBM_ACHIEVABLE:.1%} of achievable HBM')
    return out


def component_stage(vertices, triangles, runs):
    """Connected components and the 'largest' filter on the extracted mesh (mesh.connected_components / keep_components,
    csrc/pp_mesh_components.hip), stage by stage, and the host round trip through scipy.sparse.csgraph they replace."""
    from poseprobe_amd import mesh, ops
    nv, nt = vertices.shape[0], triangles.shape[0]
    i32 = dict(dtype=torch.int32, device='cuda')
    info = {}
    cc = mesh.connected_components(triangles, nv, info)
    rounds = info['rounds']
    batches = -(-rounds // mesh.CC_BATCH)
    labels, work = torch.empty(nv, **i32), torch.empty(ops.cc_workspace(nv), dtype=torch.uint8, device='cuda')
    changed = torch.empty(mesh.CC_BATCH, **i32)
    by_v, by_t = torch.empty(nv, **i32), torch.empty(nv, **i32)

    def label():
        for b in range(batches):
            ops.cc_rounds(triangles, nv, b * mesh.CC_BATCH, mesh.CC_BATCH, labels, work, changed)

    def one_round():                        # one more round at the fixpoint: a full pass over the mesh that changes nothing
        ops.cc_rounds(triangles, nv, batches * mesh.CC_BATCH, 1, labels, work, changed)

    tc = cc['triangle_counts']
    keep_c = tc == tc.max()
    keep_c &= torch.cumsum(keep_c, 0) == 1
    root_keep = torch.zeros(nv, dtype=torch.uint8, device='cuda')
    root_keep[cc['roots'][keep_c].long()] = 1
    vkeep, tkeep = torch.empty(nv, **i32), torch.empty(nt, **i32)
    ops.cc_keep_masks(cc['labels'], triangles, root_keep, vkeep, tkeep)
    n_kept_v, n_kept_t = int(vkeep.sum()), int(tkeep.sum())
    out_v, out_i, out_t = torch.empty(n_kept_v, 3, device='cuda'), torch.empty(n_kept_v, **i32), torch.empty(n_kept_t, 3, **i32)

    def compact():
        ops.cc_keep_masks(cc['labels'], triangles, root_keep, vkeep, tkeep)
        ops.cc_compact(vertices, triangles, torch.cumsum(vkeep, 0, dtype=torch.int32), torch.cumsum(tkeep, 0, dtype=torch.int32),
                       out_v, out_i, out_t)

    out = [f'components: {cc["n_components"]}, largest {int(tc.max())} of {nt} triangles, kept {n_kept_v} vertices; {rounds} rounds '
           f'({batches} batches of {mesh.CC_BATCH})']
    ms_label = device_ms(label, runs)
    out.append(f'labelling, {batches * mesh.CC_BATCH} rounds, no host read  {fmt(ms_label)}')
    assert torch.equal(labels, cc['labels'])
    per_round = [[] for _ in range(rounds)]                 # round by round (round 0 with the initialisation), one launch pair each
    for _ in range(runs):
        for r in range(rounds):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            ops.cc_rounds(triangles, nv, r, 1, labels, work, changed)
            t1.record()
            t1.synchronize()
            per_round[r].append(t0.elapsed_time(t1))
    out.append('round by round, medians (ms): ' + ' '.join(f'{statistics.median(x):.3f}' for x in per_round))
    out.append(f'one round (hook + jump) at the fixpoint  {fmt(device_ms(one_round, runs))}')
    out.append(f'pp_cc_count                          {fmt(device_ms(lambda: ops.cc_count(labels, triangles, by_v, by_t), runs))}')
    out.append(f'masks + two torch.cumsum + pp_cc_compact  {fmt(device_ms(compact, runs))}')
    out.append(f'mesh.connected_components (with its host reads)  {fmt(device_ms(lambda: mesh.connected_components(triangles, nv), runs))}')
    out.append(f"mesh.keep_components(keep='largest') (all of the above)  "
               f"{fmt(device_ms(lambda: mesh.keep_components(vertices, triangles, 'largest'), runs))}")
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return out + ['scipy is not installed: no host comparison']
    host = []
    for _ in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v, t = vertices.cpu().numpy(), triangles.cpu().numpy()
        rows, cols = np.concatenate([t[:, 0], t[:, 0]]), np.concatenate([t[:, 1], t[:, 2]])
        _, comp = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(nv, nv)), directed=False)
        big = np.argmax(np.bincount(comp[t[:, 0]]))
        vk = comp == big
        new = np.cumsum(vk, dtype=np.int32) - 1
        kv, kt = torch.from_numpy(v[vk]).cuda(), torch.from_numpy(new[t[vk[t[:, 0]]]]).cuda()
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(kv, out_v) and torch.equal(kt, out_t)
    return out + [f'host round trip: two copies + scipy.sparse.csgraph.connected_components + numpy compaction  {fmt(host[1:])}']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolutions', type=int, nargs='+', default=[128, 256, 512])
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    from poseprobe_amd import mesh, ops
    m = build_model()
    lo, hi = m.xyz_min, m.xyz_max
    lines = [f'mesh extraction, Voxurf {G}^3, box {lo.tolist()} .. {hi.tolist()}, {torch.cuda.get_device_name(0)}',
             f'medians of {a.runs} runs in one process after one warm-up run per stage; fractions against {HBM_ACHIEVABLE / 1e12} TB/s']
    for res in a.resolutions:
        n = res ** 3
        lines.append(f'\n== resolution {res} ({n} lattice points, field {4 * n / 2 ** 20:.0f} MiB, workspace '
                     f'{ops.mc_workspace(res, res, res) / 2 ** 20:.0f} MiB) ==')
        fields = {}
        for name, query in (('plain', mesh.voxurf_field(m)), ('deform', mesh.voxurf_deform_field(m))):
            ms = device_ms(lambda: fields.__setitem__(name, mesh.extract_fields_device(lo, hi, res, query, device='cuda')), a.runs)
            lines.append(f'field fill, {name:6s}            {fmt(ms)}')
        u = fields['deform']
        del fields
        work = torch.empty(ops.mc_workspace(res, res, res), dtype=torch.uint8, device='cuda')
        counts = torch.empty(2, dtype=torch.int32, device='cuda')
        ms_count = device_ms(lambda: ops.mc_count(u, 0.0, work, counts), a.runs)
        nv, nt = counts.tolist()
        vertices, triangles = torch.empty(nv, 3, device='cuda'), torch.empty(nt, 3, dtype=torch.int32, device='cuda')
        ms_emit = device_ms(lambda: ops.mc_emit(u, 0.0, work, vertices, nv, triangles, nt), a.runs)
        b_count, b_emit = 5 * n, 6 * n + 12 * (nv + nt)
        lines.append(f'deform field: {nv} vertices, {nt} triangles')
        for name, ms, b in (('pp_mc_count', ms_count, b_count), ('pp_mc_emit', ms_emit, b_emit)):
            rate = b / (statistics.median(ms) * 1e-3)
            lines.append(f'{name:28s}  {fmt(ms)}  {b / 2 ** 20:9.1f} MiB to move, {rate / 1e12:.3f} TB/s = '
                         f'{rate / HBM_ACHIEVABLE:.1%} of achievable HBM')
        ms_both = device_ms(lambda: mesh.marching_cubes(u, 0.0), a.runs)
        lines.append(f'mesh.marching_cubes (both + the host read of the counts + allocation)  {fmt(ms_both)}')
        host = []
        for _ in range(a.runs + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vertices.cpu(), triangles.cpu()
            host.append((time.perf_counter() - t0) * 1e3)
        lines.append(f'device-to-host copy of the mesh ({12 * (nv + nt) / 2 ** 20:.1f} MiB, pageable)  {fmt(host[1:])}')
        lines += component_stage(vertices, triangles, a.runs)
        # ---- colour pass over this mesh's vertices (model coordinates, on the device)
        vw = (vertices / (res - 1.0) * (hi - lo)[None] + lo[None]).contiguous()
        for name, deform, per_vertex in (('deform', True, 76 + 344 + 268), ('plain', False, 280 + 268)):
            ms = device_ms(lambda: mesh.vertex_attributes(m, vw, use_deform=deform), a.runs)
            rate = per_vertex * nv / (statistics.median(ms) * 1e-3)
            lines.append(f'vertex_attributes, {name:6s}     {fmt(ms)}  {per_vertex * nv / 2 ** 20:9.1f} MiB to move, {rate / 1e12:.3f} TB/s = '
                         f'{rate / HBM_ACHIEVABLE:.1%} of achievable HBM')
        lines += color_launches(m, vw, a.runs)
        del u, work, vertices, triangles, vw
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
