"""CPU-only checks of the ordered-flush boundary (include/poseprobe_hip.h): the workspace query is a pure host function, the new
entry points are declared (tests/test_abi.py then checks that the library exports them) and validate their arguments."""
import ctypes

import pytest

NEW = ('pp_ordered_workspace', 'pp_ordered_attach', 'pp_geometry_bwd_priors_ordered', 'pp_raygen_select_bwd_ordered')


def query(work_groups, capacity, n_rays):
    from poseprobe_amd import _lib
    b = ctypes.c_int64(-1)
    _lib.call('pp_ordered_workspace', work_groups, capacity, n_rays, ctypes.byref(b))
    return b.value


def test_new_entry_points_are_declared_and_the_abi_version_stays():
    from poseprobe_amd import _lib
    protos = _lib.parse_header()
    for name in NEW:
        assert name in protos, f'{name} is not declared in the header'
        assert hasattr(_lib.lib(), name)
    assert _lib.header_abi_version() == 4
    # the ordered variants take the arguments of the calls they stand in for, then the context in front of the stream
    for name in ('pp_geometry_bwd_priors', 'pp_raygen_select_bwd'):
        base, ordered = protos[name], protos[name + '_ordered']
        assert [a for _, a in ordered] == [a for _, a in base[:-1]] + ['ctx', 'stream']
    assert set(_lib.Context().options()) == set(_lib.OPTION_NAMES)       # no new option: the workspace is a record, not a switch


def test_workspace_query_is_positive_aligned_and_grows_with_the_work_group_count():
    sizes = [query(w, 55000, 1024) for w in (16, 64, 128, 256, 304)]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    # 2 nets x 2 work-groups per CU x 64.5 KB for the weight-gradient chains dominate: 66 MB at 256 CUs
    assert 2 * 2 * 256 * (128 * 128 + 128) * 4 <= sizes[3] < 72 * 2 ** 20
    assert query(8, 55000, 1024) == sizes[0]                               # the persistent kernels never run with fewer than 16
    assert query(256, 110000, 1024) > sizes[3] and query(256, 55000, 4096) > sizes[3]


def test_bad_arguments_are_refused_with_a_message():
    from poseprobe_amd import _lib
    L = _lib.lib()
    b = ctypes.c_int64()
    for args in ((0, 100, 10), (256, 0, 10), (256, 100, 0), (5000, 100, 10)):
        assert L.pp_ordered_workspace(*args, ctypes.byref(b)) == -1 and b'pp_ordered_workspace' in L.pp_last_error()
    assert L.pp_ordered_workspace(256, 100, 10, None) == -1
    assert L.pp_ordered_attach(None, None, 0, 16, 100, 10) == -1 and b'null context' in L.pp_last_error()
    ctx = _lib.Context()
    fake = ctypes.c_void_p(0x1008)                                          # never dereferenced: refused for its alignment
    assert L.pp_ordered_attach(ctx.handle, fake, 1 << 30, 16, 100, 10) == -1 and b'aligned' in L.pp_last_error()
    fake = ctypes.c_void_p(0x1000)
    assert L.pp_ordered_attach(ctx.handle, fake, 64, 16, 100, 10) == -1 and b'smaller' in L.pp_last_error()
    assert L.pp_ordered_attach(ctx.handle, None, 0, 0, 0, 0) == 0           # detaching is always possible
    for name in ('pp_geometry_bwd_priors_ordered', 'pp_raygen_select_bwd_ordered'):
        fn = getattr(L, name)
        null = [0.0 if t is ctypes.c_float else (0 if t is ctypes.c_int32 else None) for t in fn.argtypes]
        assert fn(*null) == -1 and name.encode() in L.pp_last_error()


def test_engine_refuses_options_without_an_ordered_flush_before_touching_the_device():
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    cfg = SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, 8 ** 3)
    for options in ({'mlp_split': 0}, {'mlp_fused': 0}):
        with pytest.raises(ValueError, match='deterministic=True'):
            TrainEngine(cfg, 3, 8, 8, 16, device='cpu', deterministic=True, options=options)
