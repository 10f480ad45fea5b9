"""pp_step_begin: the pose forward, the step's scalars, the zero block and the weight pack of a train step in one launch
of independent work-group roles, against the stand-alone entry points (pp_pose_fwd, pp_mlp_pack) on the same inputs.  Every role
runs the stand-alone kernel's body and nothing is summed across work-groups: every output has to be bit-identical.
"""
import numpy as np
import pytest
import torch

from tests.test_hip_mlp_pack import SENT, _fenced, _intact, _params

pytestmark = pytest.mark.gpu
NPE = 6                                        # posbase_pe + viewbase_pe of SceneConfig: TrainEngine.npe
ZERO = 16                                      # Workspace.zero_block


def _same(a, b, what):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: not the bits of the stand-alone launch'


def _pose_inputs(V, seed, refine_first=False):
    """refine_mask: only the last view is refined, and view 0 with refine_first (the single view of V = 1 both ways)."""
    g = torch.Generator().manual_seed(seed)
    rot = torch.linalg.qr(torch.randn(V, 3, 3, generator=g))[0]
    init = torch.cat([rot, torch.randn(V, 3, 1, generator=g)], -1).contiguous()
    se3 = torch.randn(V, 6, generator=g) * 0.05
    mask = torch.zeros(V, dtype=torch.int32)
    mask[V - 1] = 1
    mask[0] = int(refine_first)
    return se3.cuda(), init.cuda(), mask.cuda()


@pytest.mark.parametrize('V', [1, 3])
def test_step_begin_equals_the_separate_launches(V):
    """Two calls on the same buffers, the second with other parameters, other se3 and other scalars: the pack, the pose outputs and
    step_dev follow; zero_block is cleared from a sentinel both times; nothing is written outside the pack buffer."""
    from poseprobe_amd import ops
    dev = 'cuda'
    ctx = ops.Context(mlp_pack=1)
    n = ops.mlp_pack_workspace()
    arena, pack = _fenced(n)
    arena_ref, pack_ref = _fenced(n)
    z = lambda *s: torch.full(s, 4321.0, device=dev)
    out = dict(w2c=z(V, 3, 4), c2w=z(V, 3, 4), jac=z(V, 12, 6))
    ref = dict(w2c=z(V, 3, 4), c2w=z(V, 3, 4), jac=z(V, 12, 6))
    step_dev, zero_block = z(NPE + 4), z(ZERO)
    for call, scale in enumerate((0.09, 0.005)):
        warp, rgbp = _params(scale)
        se3, init, mask = _pose_inputs(V, 7 + call, refine_first=call == 0)
        g = torch.Generator().manual_seed(40 + call)
        scal = torch.cat([torch.rand(NPE, generator=g), torch.tensor([1e-2, 1e-3, 1e-3, 1e-3]) * 0.99 ** call]).numpy()
        zero_block.fill_(4321.0)
        ops.step_begin(se3, init, mask, out['w2c'], out['c2w'], out['jac'], scal, step_dev, zero_block, warp, rgbp, pack, ctx)
        assert ctx.get('mlp_pack') == 1
        ops.pose_fwd(se3, init, mask, ref['w2c'], ref['c2w'], ref['jac'])
        ops.mlp_pack(warp, rgbp, pack_ref, ops.Context(mlp_pack=1))
        torch.cuda.synchronize()
        for k in ref:
            _same(out[k], ref[k], f'call {call}: {k}')
        _same(pack, pack_ref, f'call {call}: weight pack')
        assert bool((pack.view(torch.int32) != SENT).any())
        assert np.array_equal(step_dev.cpu().numpy(), scal.astype(np.float32)), f'call {call}: step_dev'
        assert float(zero_block.abs().max()) == 0.0, f'call {call}: zero_block'
        _intact(arena, n, f'call {call}: weight pack')
        # views that are not refined keep their initial pose; the refined ones moved
        for v in range(V):
            assert torch.equal(out['w2c'][v], init[v]) == (int(mask[v]) == 0), f'call {call}: view {v}, refine_mask {int(mask[v])}'
    ops.mlp_pack_invalidate(ctx)


def test_step_begin_records_the_pack_as_mlp_pack_does():
    """A forward kernel called with the context of step_begin reads ITS pack: the same bits as with the record of pp_mlp_pack and as
    without any pack; with option mlp_pack = 0 the launch packs nothing and leaves the pack buffer alone."""
    from poseprobe_amd import ops
    from tests.test_hip_mlp_pack import _run_rgb
    warp, rgbp = _params(0.09)
    se3, init, mask = _pose_inputs(3, 3)
    V, dev = 3, 'cuda'
    z = lambda *s: torch.zeros(s, device=dev)
    n = ops.mlp_pack_workspace()
    results = []
    for opt in (1, 0):
        ctx = ops.Context(mlp_pack=opt)
        arena, pack = _fenced(n)
        ops.step_begin(se3, init, mask, z(V, 3, 4), z(V, 3, 4), z(V, 12, 6), np.zeros(NPE + 4, np.float32), z(NPE + 4), z(ZERO), warp,
                       rgbp, pack, ctx)
        results.append(_run_rgb(rgbp, 300, ctx))
        torch.cuda.synchronize()
        written = bool((pack.view(torch.int32) != SENT).any())
        assert written == bool(opt), f'mlp_pack = {opt}: pack buffer {"not " if opt else ""}written'
        ops.mlp_pack_invalidate(ctx)
    for k in ('out', 'acts', 'scratch', 'feat_grad'):
        _same(results[0][k], results[1][k], f'rgbnet {k} with the pack of step_begin')
