"""GPU tests of TrainEngine(deterministic=True): the ordered gradient flushes (include/poseprobe_hip.h, pp_ordered_attach) make the
whole object-branch train step bit-reproducible - not only the colour grid of the first step, which is all that
deterministic_scatter=True alone can promise (tests/test_hip_step.py)."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_close, load, params_from_npz
from tests.test_hip_step import build_engine

pytestmark = pytest.mark.gpu

STATE = ('k0', 'k0_m', 'k0_v', 'flat.data', 'flat.m', 'flat.v', 'se3', 'se3_m', 'se3_v')


def state(eng):
    return {'k0': eng.k0_cl, 'k0_m': eng.k0_m, 'k0_v': eng.k0_v, 'flat.data': eng.flat.data, 'flat.m': eng.flat.m,
            'flat.v': eng.flat.v, 'se3': eng.se3, 'se3_m': eng.se3_m, 'se3_v': eng.se3_v}


def snapshot(eng):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in state(eng).items()}


def assert_same_bits(a, b, what):
    for k in STATE:
        assert torch.equal(a[k], b[k]), f'{what}: {k} differs in {int((a[k] != b[k]).sum())} of {a[k].numel()} entries'


def run_small(n_steps, **kw):
    """-> per-step snapshots of a free-running trajectory from forward_g24_s10.npz."""
    from poseprobe_amd import synthetic as syn
    d = load('forward_g24_s10.npz')
    eng, _ = build_engine(d, pose_iters=1000, **kw)
    eng.zero_grads()
    V, H, W = d['images'].shape[:3]
    out = []
    for s in range(n_steps):
        idx, jit = syn.step_randomness(V * H * W, int(d['n_rand']), seed=40 + s)
        eng.train_step(torch.tensor(idx, dtype=torch.int32, device='cuda'), torch.tensor(jit, device='cuda'), 10 + s)
        out.append(snapshot(eng))
    return out


def test_small_trajectory_is_bit_reproducible():
    """Two separately built deterministic engines, 10 free-running steps on the same draws: all nine state tensors equal bit for
    bit after every step."""
    a, b = run_small(10, deterministic=True), run_small(10, deterministic=True)
    moved = a[-1]['flat.data'] != a[0]['flat.data']
    assert bool(moved.any())
    for s, (x, y) in enumerate(zip(a, b)):
        assert_same_bits(x, y, f'step {s + 1}')


def test_small_trajectory_is_bit_reproducible_with_fewer_work_groups():
    """Option mlp_wgs changes the persistent grids (and with them the order of the sums: no promise ACROSS values), the guarantee
    holds for each value."""
    a = run_small(3, deterministic=True, options={'mlp_wgs': 48})
    b = run_small(3, deterministic=True, options={'mlp_wgs': 48})
    for s, (x, y) in enumerate(zip(a, b)):
        assert_same_bits(x, y, f'mlp_wgs = 48, step {s + 1}')


def full_size_engine(**kw):
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    from poseprobe_amd.params_init import reference_like_params
    G, H, W, V, N = 160, 400, 400, 3, 1024
    cfg = SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, out_range=float(syn.range_shape().max()))
    views = syn.make_views(V, H, W)
    eng = TrainEngine(cfg, V, H, W, N, pose_iters=3000, **kw)
    eng.set_views(views['images'], views['masks'], views['Ks'], views['w2c'])
    P = reference_like_params(cfg, 3)
    eng.load_reference_params(P['k0'], P['sdf'], P['sdf_alpha'], P['sdf_beta'], P['rgbnet'], P['warp'],
                              se3=torch.tensor(syn.se3_perturbation(V)))
    eng.zero_grads()
    return eng


def full_size_trajectory(n_steps, check_first=False, **kw):
    from poseprobe_amd import synthetic as syn
    eng = full_size_engine(**kw)
    V, H, W, N = 3, 400, 400, 1024
    out = []
    for s in range(n_steps):
        idx, jit = syn.step_randomness(V * H * W, N, seed=40 + s)
        idx, jit = torch.tensor(idx, dtype=torch.int32, device='cuda'), torch.tensor(jit, device='cuda')
        if s == 0 and check_first:
            # train_step = render_and_grads + optimizer_step on one GPU; taken apart to look at the gradients in between
            eng.render_and_grads(idx, jit, 10 + s)
            torch.cuda.synchronize()
            M = int(eng.ws.count.item())
            cus = torch.cuda.get_device_properties(eng.dev).multi_processor_count
            # the weight-gradient chain shares 2 work-groups per CU out over its three layers: a third each for the warp net
            # (three 128-wide layers), 4/11 each for rgbnet's two 128-wide ones (pp_launch_wgrad_chain_s)
            assert 4 * M > 8 * 64 * ((2 * cus) // 3), f'warp net: {4 * M} rows: the weight-gradient launch halved its grid'
            assert (M + 63) // 64 < 8 * ((2 * cus * 4) // 11), f'rgbnet: {M} rows: the weight-gradient launch kept its whole grid'
            for seg in ('warp', 'rgbnet', 'sdf_ab'):
                assert float(eng.flat.view(seg, 'grad').abs().max()) > 0, f'gradient of {seg} is all zero'
            assert float(eng.se3_grad.abs().max()) > 0 and float(eng.k0_grad.abs().max()) > 0
            eng.optimizer_step(True, grad_scale=1.0)
        else:
            eng.train_step(idx, jit, 10 + s)
        out.append(snapshot(eng))
    del eng
    torch.cuda.empty_cache()
    return out


def test_bench_workload_trajectory_is_bit_reproducible():
    """160^3 grid, 1024 rays, ~55 k samples (the setup of tests/test_hip_fullsize.py), 3 steps, two engines: all nine state
    tensors equal bit for bit after every step.  Only here does every persistent work-group run.  This one test covers both
    branches of the weight-gradient kernel's grid rule: the warp net's launch (4 rows per sample, about 20 tiles per work-group)
    keeps its whole grid, rgbnet's (under 8 tiles per work-group) idles half of it on the device, and the reduction has to
    derive the same active count from the device-side sample count - both are asserted on the first step, as is that no
    segment's gradient is all zero."""
    a = full_size_trajectory(3, check_first=True, deterministic=True)
    b = full_size_trajectory(3, deterministic=True)
    for s, (x, y) in enumerate(zip(a, b)):
        assert_same_bits(x, y, f'step {s + 1}')


def one_step_grads(d, idx, jit, **kw):
    eng, _ = build_engine(d, pose_iters=1000, **kw)
    eng.zero_grads()
    eng.render_and_grads(idx, jit, 10)
    torch.cuda.synchronize()
    return eng, [t.detach().cpu().numpy().copy() for t in (eng.flat.grad, eng.se3_grad, eng.k0_grad)]


def small_inputs(seed=91):
    from poseprobe_amd import synthetic as syn
    d = load('forward_g24_s10.npz')
    V, H, W = d['images'].shape[:3]
    idx, jit = syn.step_randomness(V * H * W, int(d['n_rand']), seed=seed)
    return d, torch.tensor(idx, dtype=torch.int32, device='cuda'), torch.tensor(jit, device='cuda')


# "equal up to the order of the float atomics": the tolerances of
# tests/test_hip_step.py::test_step_gradients_do_not_depend_on_work_group_counts_or_the_auxiliary_stream
ORDER_TOL = dict(rtol=1e-4, scaled=2e-6)


def test_deterministic_step_computes_the_same_gradients_as_the_default_step():
    d, idx, jit = small_inputs()
    _, ref = one_step_grads(d, idx, jit)
    eng, got = one_step_grads(d, idx, jit, deterministic=True)
    assert eng.core.ordered and eng._ordered_work is not None
    for name, a, b in zip(('mlp / alpha / beta', 'se3', 'k0'), got, ref):
        assert float(np.abs(b).max()) > 0
        assert_close(a, b, name=f'deterministic vs default: grad {name}', **ORDER_TOL)


@pytest.mark.parametrize('n_steps', [3, 10])
def test_free_running_deterministic_trajectory_matches_the_oracle(n_steps):
    """The body of tests/test_hip_step.py::test_free_running_trajectory_with_deterministic_scatter_matches_the_oracle with
    deterministic=True: same thresholds."""
    from oracle import voxurf_oracle as O
    from poseprobe_amd import synthetic as syn
    from tests.helpers import assert_trajectory_close, engine_vs_oracle_tensors, scene_for
    d = load('forward_g24_s10.npz')
    eng, cfg = build_engine(d, pose_iters=1000, deterministic=True)
    P = params_from_npz(d)
    st = O.TrainState(P, scene_for(d['G']), torch.tensor(d['w2c_init']), torch.tensor(d['Ks']), torch.tensor(d['images']),
                      torch.tensor(d['masks']), se3_refine=torch.tensor(d['se3']), pose_iters=1000)
    eng.zero_grads()
    V, H, W = d['images'].shape[:3]
    start = engine_vs_oracle_tensors(eng, st, P)
    gmin, gmax = {}, {}
    names = {'k0': lambda: P['k0'].grad}
    for li in range(4):
        names[f'rgbnet{li}.W'] = (lambda li=li: P['rgbnet'][li][0].grad)
        names[f'rgbnet{li}.b'] = (lambda li=li: P['rgbnet'][li][1].grad)
    for li in range(5):
        names[f'warp{li}.W'] = (lambda li=li: P['warp'][li][0].grad)
        names[f'warp{li}.b'] = (lambda li=li: P['warp'][li][1].grad)
    for s in range(n_steps):
        idx, jit = syn.step_randomness(V * H * W, int(d['n_rand']), seed=40 + s)
        st.step(torch.tensor(idx), torch.tensor(jit), 10 + s)
        eng.train_step(torch.tensor(idx, dtype=torch.int32, device='cuda'), torch.tensor(jit, device='cuda'), 10 + s)
        for name, get in names.items():
            g = get().detach().abs().double().numpy()
            gmin[name] = g if name not in gmin else np.minimum(gmin[name], g)
            gmax[name] = g if name not in gmax else np.maximum(gmax[name], g)
    torch.cuda.synchronize()
    crossed = {name: gmin[name] / (gmax[name] + 1e-30) for name in names}
    assert_trajectory_close(engine_vs_oracle_tensors(eng, st, P), start, n_steps, rtol=1e-3, crossed=crossed, what=f'{n_steps} steps: ',
                            coupled=n_steps > 3)


def test_deterministic_step_stays_inside_its_buffers():
    """One deterministic step at a ragged size - the engine's capacity is cut to a count that is no multiple of 16 or 64 and lies
    below the fixture's sample count, so every kernel runs a partial last tile - with 64 KB of sentinels in front of and behind
    the ordered-flush workspace and the gradient buffers: the sentinels are intact, the gradients finite."""
    from poseprobe_amd import ops
    d = load('forward_g24_s10.npz')                 # the fixture's own rays: its sample count is known from the golden output
    idx, jit = torch.tensor(d['ray_idx'], dtype=torch.int32, device='cuda'), torch.tensor(d['jitter'], device='cuda')
    cap = (d['out.weights'].shape[0] // 64) * 64 - 27
    eng, _ = build_engine(d, pose_iters=1000, deterministic=True, capacity=cap)
    GUARD, MARK = 16384, -7.5          # floats, value
    guarded = {}

    def fenced(n, dtype=torch.float32):
        g = GUARD * (4 if dtype == torch.uint8 else 1)
        buf = torch.full((n + 2 * g,), MARK if dtype == torch.float32 else 0xA5, dtype=dtype, device='cuda')
        inner = buf[g:g + n]
        if dtype == torch.float32:
            inner.zero_()
        guarded[len(guarded)] = (buf, g, n)
        return inner

    mlp_wgs = eng.ctx.get('mlp_wgs')
    wgs = max(16, mlp_wgs) if mlp_wgs > 0 else torch.cuda.get_device_properties(eng.dev).multi_processor_count
    need = ops.ordered_workspace(wgs, eng.ws.cap, eng.N)
    work = fenced(need, torch.uint8)
    eng._ordered_work = work
    ops.ordered_attach(eng.ctx, work, wgs, eng.ws.cap, eng.N)
    eng.flat.grad = fenced(eng.flat.grad.numel())
    eng.se3_grad = fenced(eng.se3_grad.numel()).view(eng.V, 6)
    eng.c2w_grad = fenced(eng.c2w_grad.numel()).view(eng.V, 3, 4)
    eng.k0_grad = fenced(eng.k0_grad.numel()).view(eng.k0_grad.shape)
    eng.k0_touched.zero_()
    eng.train_step(idx, jit, 10)
    torch.cuda.synchronize()
    assert int(eng.ws.count.item()) == cap and cap % 16 != 0
    assert eng._ordered_work.data_ptr() == work.data_ptr()
    for buf, g, n in guarded.values():
        mark = MARK if buf.dtype == torch.float32 else 0xA5
        assert bool((buf[:g] == mark).all()) and bool((buf[g + n:] == mark).all()), 'a sentinel was overwritten'
    for t in state(eng).values():
        assert bool(torch.isfinite(t).all())


def test_options_without_an_ordered_flush_are_refused():
    d = load('forward_g24_s10.npz')
    for options in ({'mlp_split': 0}, {'mlp_fused': 0}, {'mlp_split': 15}):
        with pytest.raises(ValueError, match='deterministic=True'):
            build_engine(d, deterministic=True, options=options)


def test_the_library_refuses_calls_it_cannot_order():
    """A workspace attached to a context whose options select kernels without an ordered flush: the MLP backward refuses with a
    message instead of falling back to atomics; an undersized workspace is refused at attach time."""
    from poseprobe_amd import _lib, ops
    ctx = ops.Context(mlp_split=0)
    cap, n_rays = 256, 16
    work = torch.empty(ops.ordered_workspace(16, cap, n_rays), dtype=torch.uint8, device='cuda')
    with pytest.raises(_lib.PoseProbeError, match='smaller'):
        ops.ordered_attach(ctx, work[:-16], 16, cap, n_rays)
    ops.ordered_attach(ctx, work, 16, cap, n_rays)
    wsz = ops.mlp_workspaces(cap)
    z = lambda *s: torch.zeros(*s, device='cuda')
    count = torch.full((1,), cap, dtype=torch.int32, device='cuda')
    with pytest.raises(_lib.PoseProbeError, match='ordered'):
        ops.warp_bwd(z(ops.WARP_PARAMS), z(cap, 3), z(wsz['warp'][0]), z(cap, 16), count, cap, 1.0, z(wsz['warp'][1]),
                     z(ops.WARP_PARAMS), z(cap, 3), ctx)
    ops.ordered_attach(ctx, None, 0, 0, 0)          # detached: the same call runs, on atomics
    ops.warp_bwd(z(ops.WARP_PARAMS), z(cap, 3), z(wsz['warp'][0]), z(cap, 16), count, cap, 1.0, z(wsz['warp'][1]),
                 z(ops.WARP_PARAMS), z(cap, 3), ctx)
    torch.cuda.synchronize()


def test_flag_off_is_the_default_path():
    """deterministic=False is the default engine: no private context, no workspace, the atomic kernels - and one step of each
    agrees up to the order of the float atomics (they cannot be bit-equal: the atomics remain)."""
    d, idx, jit = small_inputs()
    a, ga = one_step_grads(d, idx, jit)
    b, gb = one_step_grads(d, idx, jit, deterministic=False)
    for eng in (a, b):
        assert eng.ctx is None and not eng.deterministic and not eng.deterministic_scatter and not eng.core.ordered
        assert eng._ordered_work is None
    for name, x, y in zip(('mlp / alpha / beta', 'se3', 'k0'), ga, gb):
        assert_close(x, y, name=f'deterministic=False vs default: grad {name}', **ORDER_TOL)
