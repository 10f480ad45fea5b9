"""CPU-only checks of the scene branch's deterministic mode (include/poseprobe_hip.h, "ordered weight-gradient flush"): the
constructor refusals happen before the device is touched, the workspace query is a pure host function, the attach call
validates its arguments, and the ABI version stays."""
import ctypes
import types

import pytest

NEW = ('pp_nerf_ordered_workspace', 'pp_nerf_ordered_attach', 'pp_nerf_c2w_fold', 'pp_nerf_sample_pdf')


def _net(**kw):
    from poseprobe_amd import bg_nerf
    return bg_nerf.NeRF(bg_nerf.default_options(), device='cpu', **kw)


def test_new_entry_points_are_declared_and_the_abi_version_stays():
    from poseprobe_amd import _lib
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, f'{name} is not declared in the header'
        assert hasattr(_lib.lib(), name)
    assert _lib.header_abi_version() == 4 and _lib.lib().pp_abi_version() == 4
    assert [a for _, a in protos['pp_nerf_ordered_attach']] == ['ctx', 'work', 'work_bytes']
    assert set(_lib.Context().options()) == set(_lib.OPTION_NAMES)       # no new option: the workspace is a record, not a switch


def test_workspace_query_returns_the_documented_size():
    from poseprobe_amd import _lib, ops
    # 512 slots (128 row splits x 4 output blocks is the largest launch) of a 128 x 128 block + 128 bias sums, in floats
    assert ops.nerf_ordered_workspace() == 512 * (64 * 1024 + 512)
    assert ops.nerf_ordered_workspace() % 16 == 0
    assert _lib.lib().pp_nerf_ordered_workspace(None) == -1 and b'pp_nerf_ordered_workspace' in _lib.lib().pp_last_error()


def test_attach_rejects_bad_arguments_with_a_message():
    from poseprobe_amd import _lib, ops
    L = _lib.lib()
    need = ops.nerf_ordered_workspace()
    assert L.pp_nerf_ordered_attach(None, None, 0) == -1 and b'null context' in L.pp_last_error()
    ctx = _lib.Context()
    fake = ctypes.c_void_p(0x1008)                                          # never dereferenced: refused for its alignment
    assert L.pp_nerf_ordered_attach(ctx.handle, fake, need) == -1 and b'aligned' in L.pp_last_error()
    fake = ctypes.c_void_p(0x1000)
    assert L.pp_nerf_ordered_attach(ctx.handle, fake, need - 16) == -1 and b'smaller' in L.pp_last_error()
    assert L.pp_nerf_ordered_attach(ctx.handle, fake, need) == 0            # recorded only: nothing is touched at attach time
    assert L.pp_nerf_ordered_attach(ctx.handle, None, 0) == 0               # detaching is always possible
    with pytest.raises(ValueError, match='context of its own'):
        ops.nerf_ordered_attach(None, None)
    for name in ('pp_nerf_c2w_fold', 'pp_nerf_sample_pdf'):
        fn = getattr(L, name)
        null = [0.0 if t is ctypes.c_float else (0 if t is ctypes.c_int32 else None) for t in fn.argtypes]
        assert fn(*null) == -1 and name.encode() in L.pp_last_error()


def test_scene_engine_refuses_the_fp32_instruction_path_before_touching_the_device():
    from poseprobe_amd import bg_nerf
    with pytest.raises(ValueError, match='deterministic=True with nerf_split = 0'):
        bg_nerf.SceneEngine(_net(options={'nerf_split': 0}), deterministic=True)
    with pytest.raises(ValueError, match='deterministic=True with nerf_split = 0'):
        bg_nerf.SceneEngine(_net(), net_fine=_net(options={'nerf_split': 0}), deterministic=True)
    net = _net()
    eng = bg_nerf.SceneEngine(net)                                        # the default: no context, no workspace
    assert net.ctx is None and eng._ordered_work is None and not eng.deterministic


def test_joint_engine_refuses_object_engines_it_cannot_cover():
    from poseprobe_amd.joint import DualBranchEngine
    plain = types.SimpleNamespace(deterministic=False, dist=None)
    with pytest.raises(ValueError, match='deterministic=True with an object engine built without'):
        DualBranchEngine(plain, _net(), deterministic=True)
    sharded = types.SimpleNamespace(deterministic=True, dist=object())
    with pytest.raises(ValueError, match='deterministic=True with a multi-rank'):
        DualBranchEngine(sharded, _net(), deterministic=True)
    with pytest.raises(ValueError, match='deterministic=True with nerf_split = 0'):
        DualBranchEngine(types.SimpleNamespace(deterministic=True, dist=None), _net(options={'nerf_split': 0}), deterministic=True)


def test_torch_fp32_stays_inside_the_bounds_the_kernel_tests_allow():
    """The tolerances of the two kernel tests (tests/test_hip_scene_deterministic.py) are 4 x the error of torch's own fp32
    evaluation against float64 on the same inputs: that evaluation itself (whose summation order depends on the
    host's thread count) must lie inside the bound."""
    import torch
    from tests import test_hip_scene_deterministic as T
    a = T.fold_inputs()
    ref = T.fold_expression(*(t.double() for t in a))
    err = float((T.fold_expression(*a).double() - ref).abs().max() / ref.abs().max())
    assert 0 < err <= T.FOLD_TOL, err
    worst = 0.
    for per_ray in (False, True):
        for det in (True, False):
            w, d, g, rng = T.pdf_inputs(per_ray=per_ray, det=det)
            assert float(w.min()) > 1e-4                                   # no degenerate bin
            ref = T.pdf_expression(w.double(), d.double(), g.double(), rng, 128)
            worst = max(worst, float((T.pdf_expression(w, d, g, rng, 128).double() - ref).abs().max()))
    assert 0 < worst <= T.PDF_TOL, worst
