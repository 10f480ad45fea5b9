"""Host-side logic of the scene branch's correspondence term (poseprobe_amd.trainer / bg_nerf): the loss_type parse, the 'exp'
loss weights, the weight decay gamma and the start iteration (corres_loss.py:78-90, :151), the per-view pair table with its
partner rule and conf > 0 mask, the subsample size, the DTU settings and the per-ray fine-sampling grid of the union pass.
No GPU needed."""
import pytest
import torch

from poseprobe_amd import bg_nerf
from poseprobe_amd.trainer import (corres_gamma, corres_sample_size, corres_started, loss_terms, loss_weight, pair_partner,
                                   pair_table)


def test_loss_type_parse():
    assert loss_terms(None) == {'photometric'}
    assert loss_terms('photometric') == {'photometric'}
    assert loss_terms('photometric_and_corres') == {'photometric', 'corres'}
    assert loss_terms('photometric_and_corres_and_depth_cons') == {'photometric', 'corres', 'depth_cons'}
    for bad in ('photometric_and_SparseCOLMAPDepthLoss', 'photometric_and_corres_and_fea_cons', 'corres'):
        with pytest.raises(NotImplementedError):
            loss_terms(bad)


def test_exp_loss_weights():
    opt = bg_nerf.sparf_dtu_options()
    assert loss_weight(opt, 'photometric') == 1.0
    assert loss_weight(opt, 'corres') == pytest.approx(1e-2, rel=1e-12)
    assert loss_weight(opt, 'depth_cons') == pytest.approx(1e-3, rel=1e-12)
    opt.loss_weight.parametrization = 'linear'
    assert loss_weight(opt, 'corres') == -2.0
    opt.loss_weight.corres = None
    assert loss_weight(opt, 'corres') is None
    assert loss_weight(bg_nerf.default_options(), 'photometric') == 1.0          # no loss_weight tree: the photometric term alone
    opt.loss_weight.equalize_losses = True
    with pytest.raises(NotImplementedError):
        loss_weight(opt, 'corres')


def test_corres_gamma_and_start_iteration():
    opt = bg_nerf.sparf_dtu_options()
    assert [corres_gamma(it, opt, 60000) for it in (0, 4999, 5000, 9999, 10000, 25000)] == [1, 1, 2, 2, 4, 32]
    opt.ratio_start_decrease_corres_weight = 0.1                      # decay from 0.1 * max_iter = 6000 on
    assert [corres_gamma(it, opt, 60000) for it in (5999, 6000, 10999, 11000)] == [1, 1, 1, 2]
    opt.ratio_start_decrease_corres_weight = None
    opt.iter_start_decrease_corres_weight = 100
    assert [corres_gamma(it, opt, 60000) for it in (99, 100, 5099, 5100)] == [1, 1, 1, 2]
    opt.gradually_decrease_corres_weight = False
    assert corres_gamma(10 ** 6, opt, 60000) == 1.0
    opt.start_iter.corres = 1000
    assert not corres_started(999, opt) and corres_started(1000, opt)
    assert corres_started(0, bg_nerf.default_options())


def test_pair_table_partner_rule_and_conf_mask():
    assert [pair_partner(i) for i in range(5)] == [1, 0, 1, 2, 3]
    g = torch.Generator().manual_seed(0)
    entries = []
    for i in range(4):
        conf = torch.rand(20, generator=g)
        conf[::3] = 0.0
        entries.append((torch.rand(20, 2, generator=g), torch.rand(20, 2, generator=g), conf))
    entries[3] = entries[3] + (0,)                                    # explicit partner
    entries.append(None)                                              # a view without matches
    table = pair_table(entries)
    assert [(t[0], t[1]) for t in table[:4]] == [(0, 1), (1, 0), (2, 1), (3, 0)] and table[4] is None
    for (ps, po, conf), (i, j, ps_k, po_k, conf_k) in zip([e[:3] for e in entries[:4]], table[:4]):
        keep = conf > 0
        assert int(keep.sum()) == 13 and conf_k.shape == (13,) and bool((conf_k > 0).all())
        assert torch.equal(ps_k, ps[keep]) and torch.equal(po_k, po[keep]) and torch.equal(conf_k, conf[keep])


def test_subsample_size():
    assert corres_sample_size(300, 1024) == 300
    assert corres_sample_size(512, 1024) == 512
    assert corres_sample_size(5000, 1024) == 512
    assert corres_sample_size(5000, 1023) == 511


def test_sparf_dtu_options_leave_the_defaults_alone():
    d0 = bg_nerf.default_options()
    opt = bg_nerf.sparf_dtu_options()
    assert 'loss_type' not in d0 and not d0.nerf.fine_sampling
    assert opt.loss_type == 'photometric_and_corres_and_depth_cons' and opt.nerf.fine_sampling
    assert opt.nerf.ratio_start_fine_sampling_at_x == 0.3 and opt.corres_weight_reduct_at_x_iter == 5000
    assert opt.renderrepro_pixel_reprojection_thresh == 10. and opt.renderrepro_depth_reprojection_thresh == 0.1
    assert not opt.renderrepro_do_pixel_reprojection_check and not opt.renderrepro_do_depth_reprojection_check
    assert opt.diff_loss_type == 'huber' and opt.barf_c2f == [0.4, 0.7]


def test_per_ray_fine_grid_equals_separate_sampler_calls():
    """The union pass samples the photometric rows and the matched rows in one call with one uniform grid per row; that
    equals two sampler calls (two render calls in the reference) with their own grids."""
    g = torch.Generator().manual_seed(3)
    w = torch.rand(1, 30, 16, generator=g) ** 3
    ga, gb = torch.rand(9, generator=g), torch.rand(9, generator=g)
    a = bg_nerf.sample_depth_from_pdf(w[:, :20], 16, 8, (0.5, 3.0), det=False, grid=ga)
    b = bg_nerf.sample_depth_from_pdf(w[:, 20:], 16, 8, (0.5, 3.0), det=False, grid=gb)
    both = bg_nerf.sample_depth_from_pdf(w, 16, 8, (0.5, 3.0), det=False,
                                         grid=torch.cat([ga.expand(20, 9), gb.expand(10, 9)]))
    assert torch.equal(both, torch.cat([a, b], dim=1))
