"""tests/generic_reference.py (the float64 yardstick of tests/test_hip_generic_kernels.py) pinned on the CPU: the feature builder to
stage_reference.color_feat, the MLP to the torch.nn.Sequential the DirectVoxGO twin builds, and the input selection of the
MLP tests to what it promises (few rows rejected, no ReLU of a kept row changes state between float32 and float64)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import generic_reference as GR
from tests import stage_reference as SR
from tests.test_hip_stage_kernels import XYZ_MAX, XYZ_MIN, color_inputs

# (width, in_ld, n_gemm) of the layered-MLP tests and the 64/3 shape of the diffuse-logit tests
MLP_SHAPES = [(7, 32, 1), (72, 96, 2), (128, 128, 4), (40, 64, 8), (61, 64, 3)]


def test_feat_generic_equals_the_specialised_colour_feature_reference():
    C, Lp, Lv, size, M = 12, 5, 1, (11, 6, 9), 300
    inp = color_inputs(M, C, Lp, Lv, size, seed=4)
    for dt, tol in ((torch.float64, 1e-15), (torch.float32, 1e-6)):
        a = SR.color_feat(inp['k0'], inp['p'], inp['vd'], inp['ray_id'], inp['g'], inp['pe_w'], Lp, Lv, XYZ_MIN, XYZ_MAX, dtype=dt,
                          feat_grad=inp['fg'])
        b = GR.feat_generic(inp['k0'], inp['p'], inp['vd'], inp['ray_id'], inp['g'], inp['pe_w'], None, 0, 64, Lp, Lv, XYZ_MIN,
                            XYZ_MAX, dtype=dt, feat_grad=inp['fg'])
        assert b['width'] == 57 and b['feat'].dtype == dt
        assert float((a['feat'] - b['feat']).abs().max()) <= tol
        assert float((a['k0_grad'] - b['k0_grad']).abs().max()) <= tol * float(a['k0_grad'].abs().max())
        assert float((b['k0_raw'] - b['feat'][:, :C]).abs().max()) == 0


def test_feat_generic_skip_selection_and_raw_gradient():
    """k0_skip drops the leading channels from the features only; sel == 0 rows are zero and carry no gradient; k0_raw_grad
    reaches every channel."""
    C, Lp, Lv, size, M = 8, 2, 1, (5, 6, 4), 40
    inp = color_inputs(M, C, Lp, Lv, size, seed=2)
    sel = (np.arange(M) % 3 != 0).astype(np.uint8)
    full = GR.feat_generic(inp['k0'], inp['p'], inp['vd'], inp['ray_id'], None, None, None, 0, 64, Lp, Lv, XYZ_MIN, XYZ_MAX)
    skip = GR.feat_generic(inp['k0'], inp['p'], inp['vd'], inp['ray_id'], None, None, sel, 3, 32, Lp, Lv, XYZ_MIN, XYZ_MAX)
    w = C - 3 + 3 + 6 * Lp + 3 + 6 * Lv
    assert skip['width'] == w and skip['feat'].shape == (M, 32)
    on = sel.astype(bool)
    assert torch.equal(skip['feat'][on, :w], full['feat'][on, 3:3 + w]) and torch.equal(skip['k0_raw'][on], full['feat'][on, :C])
    assert float(skip['feat'][~on].abs().max()) == 0 and float(skip['k0_raw'][~on].abs().max()) == 0
    assert float(skip['feat'][:, w:].abs().max()) == 0
    # un-weighted encodings: the sin block of the position starts right after x
    x = (torch.tensor(inp['p'], dtype=torch.float64) - torch.tensor(XYZ_MIN, dtype=torch.float64)) / torch.tensor(
        XYZ_MAX - XYZ_MIN.astype(np.float64))
    assert torch.allclose(full['feat'][:, C + 3 + 1 * Lp + 1], torch.sin(2 * x[:, 1]), rtol=0, atol=1e-15)
    fg = np.zeros((M, 32), np.float32)
    rg = np.random.RandomState(0).normal(size=(M, C)).astype(np.float32)
    g = GR.feat_generic(inp['k0'], inp['p'], inp['vd'], inp['ray_id'], None, None, sel, 3, 32, Lp, Lv, XYZ_MIN, XYZ_MAX,
                        feat_grad=fg, k0_raw_grad=rg)['k0_grad']
    ref = SR.grid_sample(inp['k0'], inp['p'], XYZ_MIN, XYZ_MAX, 0, out_grad=rg * sel[:, None])['grid_grad']
    assert float((g - ref).abs().max()) <= 1e-14 and float(g[:3].abs().max()) > 0


@pytest.mark.parametrize('width,depth', [(61, 4), (72, 3), (7, 2)])
def test_mlp_equals_the_sequential_of_the_twin(width, depth):
    torch.manual_seed(width)
    rgbnet = nn.Sequential(                                  # as DirectVoxGO.__init__ builds it
        nn.Linear(width, 128), nn.ReLU(inplace=True),
        *[nn.Sequential(nn.Linear(128, 128), nn.ReLU(inplace=True)) for _ in range(depth - 2)],
        nn.Linear(128, 3)).double()
    lins = [m for m in rgbnet.modules() if isinstance(m, nn.Linear)]
    layers = [(l.weight.detach(), l.bias.detach()) for l in lins]
    M = 50
    x = torch.randn(M, width + 3, dtype=torch.float64)       # trailing columns are ignored
    la = torch.randn(M, 4, dtype=torch.float64)
    og = torch.randn(M, 3, dtype=torch.float64)
    r = GR.mlp(layers, x, la, out_grad=og)
    xin = x[:, :width].clone().requires_grad_(True)
    lal = la.clone().requires_grad_(True)
    out = torch.sigmoid(rgbnet(xin) + lal[:, :3])
    (out * og).sum().backward()
    assert len(r['pre']) == depth - 1 and r['pre'][0].shape == (M, 128)
    assert torch.allclose(r['out'], out.detach(), rtol=0, atol=1e-15)
    assert torch.allclose(r['feat_grad'], xin.grad, rtol=1e-13, atol=1e-16)
    assert torch.allclose(r['logit_grad'], lal.grad[:, :3], rtol=1e-13, atol=1e-16) and float(lal.grad[:, 3].abs().max()) == 0
    for (gW, gb), l in zip(r['params_grad'], lins):
        assert torch.allclose(gW, l.weight.grad, rtol=1e-12, atol=1e-15) and torch.allclose(gb, l.bias.grad, rtol=1e-12, atol=1e-15)
    plain = GR.mlp(layers, x, None)
    assert torch.allclose(plain['out'], torch.sigmoid(rgbnet(x[:, :width])).detach(), rtol=0, atol=1e-15)


@pytest.mark.parametrize('width,in_ld,n_gemm', MLP_SHAPES)
def test_pick_rows_rejects_few_rows_and_keeps_none_that_flips(width, in_ld, n_gemm):
    """Under 5 % of standard-normal candidate rows have a pre-activation within 1e-5 (relative to its row) of zero, and on the
    kept rows a float32 evaluation takes every ReLU the way the float64 one does: the GPU tests need no allowance for rows
    whose ReLU state differs between two roundings."""
    layers = GR.mlp_params(width, n_gemm, seed=5)
    cand = torch.randn(4000, width, generator=torch.Generator().manual_seed(n_gemm))
    ok = GR.clear_rows(cand, layers)
    assert 1 - float(ok.float().mean()) < 0.05
    kept = GR.pick_rows(cand, layers, 3000)
    assert kept.shape == (3000, width) and torch.equal(kept, cand[ok][:3000])
    p64, p32 = GR.mlp(layers, kept)['pre'], GR.mlp(layers, kept, dtype=torch.float32)['pre']
    assert len(p64) == n_gemm
    for a, b in zip(p64, p32):
        assert torch.equal(a > 0, b > 0)
    with pytest.raises(AssertionError):
        GR.pick_rows(cand[:10], layers, 11)


def test_mlp_inputs_has_enough_candidates_at_every_size_the_gpu_tests_use():
    for width, in_ld, n_gemm in MLP_SHAPES:
        for M in (0, 1, 63, 64, 65, 1000, 2053):
            layers, feat = GR.mlp_inputs(width, n_gemm, M, seed=5)
            assert feat.shape == (M, width) and len(layers) == n_gemm + 1


def test_generic_k0_backward_checks_its_arguments_like_the_forward():
    """k0_skip outside 0..k0_dim, ld no multiple of 32 and a width beyond ld are refused by both entry points before anything is
    launched (the pointers below are never dereferenced)."""
    import ctypes
    from poseprobe_amd import _lib
    from tests.test_hip_stage_kernels import scene
    sc = scene((7, 5, 9), k0_dim=12, pos_pe=5, view_pe=4)               # width 72 - k0_skip
    fake = ctypes.c_void_p(4096)
    for skip, ld in ((13, 96), (-1, 96), (3, 80), (3, 64), (0, 64)):
        with pytest.raises(_lib.PoseProbeError, match='feature width does not fit ld'):
            _lib.call('pp_feat_generic_bwd_k0', ctypes.byref(sc), fake, None, skip, ld, fake, 16, fake, None, fake, None)
        with pytest.raises(_lib.PoseProbeError, match='feature width does not fit ld'):
            _lib.call('pp_feat_generic_fwd', ctypes.byref(sc), fake, fake, fake, fake, None, None, None, skip, ld, fake, 16, fake, None,
                      None)


def test_mlp_workspace_sizes():
    """ops.mlp_workspace: n_gemm activations; Ybar of max(n_gemm, 3) layers plus room for transposed weights; bad shapes refused."""
    from poseprobe_amd import _lib, ops
    for in_ld, n_gemm, cap in ((32, 1, 1), (96, 2, 130), (64, 3, 63), (128, 4, 1003), (64, 8, 65)):
        a, s = ops.mlp_workspace(in_ld, n_gemm, cap)
        assert a == n_gemm * cap * 128 and s == max(n_gemm, 3) * cap * 128 + 49152
    for in_ld, n_gemm, cap in ((48, 2, 10), (160, 2, 10), (64, 0, 10), (64, 9, 10), (64, 3, 0)):
        with pytest.raises(_lib.PoseProbeError):
            ops.mlp_workspace(in_ld, n_gemm, cap)
