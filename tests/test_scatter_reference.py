"""The references of tests/scatter_reference.py checked against each other on the CPU, before the GPU tests trust them.

Accuracy of the ordered float32 replay against the float64 grid_sample gradient, per voxel and channel:

    |replay32 - scatter64| <= (n_v + 8) eps32 A_v + 12 eps32 max(size) G_v

n_v contributions, A_v = sum |w g|, G_v = sum |g| (G_v also over the samples that reach v in float64 only, by a coordinate
within rounding distance of a cell face: their weight there, of the order eps * size, is all error).  First term: the standard bound of a sequential fp32 sum of n_v rounded
products (plus slack for the product and the final add).  Second term: the absolute error of a weight, three factors each
carrying the ~3-rounding error of the voxel coordinate u, which is of size eps * size.
"""
import numpy as np
import pytest

from tests import scatter_reference as R

CS = [12, 4, 16, 1]


def full_case(size, C):
    case = R.build_case(size)
    return case, [(case['pts'], R.build_gradients(R.N_CASE, C))]


@pytest.mark.parametrize('size', R.GRIDS)
@pytest.mark.parametrize('C', CS)
def test_replay32_is_as_accurate_as_an_fp32_sum_can_be(size, C):
    sc = R.GridScene(size)
    _, shards = full_case(size, C)
    r32 = R.replay32(shards, sc, C, np.zeros((sc.n_voxels, C), np.float32))
    r64 = R.scatter64(shards, sc, C)
    bound = (r32['n'][:, None] + 8) * R.EPS32 * r32['A'] + 12 * R.EPS32 * max(size) * r32['G']
    err = np.abs(r32['grad'].astype(np.float64) - r64)
    assert (err[bound == 0] == 0).all()
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f'grid {size} C {C}: worst |replay32 - scatter64| / bound = {ratio:.4f}')
    assert ratio <= 1
    assert np.abs(r64).max() > 1                                  # the comparison is not one of zeros
    # a voxel nobody reaches in either precision receives nothing
    assert (r64[(r32['G'] == 0).all(1)] == 0).all()


@pytest.mark.parametrize('size', R.GRIDS)
def test_cases_hold_what_the_gpu_tests_rely_on(size):
    """Asserted over the (count, capacity) pairs the GPU tests run, so that no case can go soft unnoticed."""
    C = 12
    sc = R.GridScene(size)
    case = R.build_case(size)
    g = R.build_gradients(R.N_CASE, C)
    pre = R.build_prefill(sc.n_voxels, C)
    assert set(case['kind']) == {'interior', 'node', 'face', 'band', 'far', 'huge', 'cell'} and case['kind'][0] == 'interior'
    assert np.isfinite(case['pts']).all() and (np.abs(case['pts']) == np.float32(1e30)).sum() == 20
    # the largest valid set (700 rows): every in/out pattern of the eight corners, samples with no corner inside, and a
    # weight of exactly zero on a corner inside the grid (exact faces: marked, zero contribution)
    big = max(min(c) for c in R.COUNTS)
    st = R.stencil32(case['pts'][:big], sc)
    pat = set(R.axis_patterns(st))
    assert set(R.CORNER_PATTERNS) <= pat, sorted(set(R.CORNER_PATTERNS) - pat)
    assert any('out' in p for p in pat)
    assert not st['ok'][np.isin(case['kind'][:big], ['far', 'huge'])].any()
    assert (np.abs(case['pts'][:big]) == np.float32(1e30)).any()
    assert ((st['w'] == 0) & st['ok']).any()
    seen = dict(one=False, crossing=False, long=False, marked_zero=False, unmarked=False)
    for count, cap in R.COUNTS:
        M = min(count, cap)
        r = R.replay32([(case['pts'][:M], g[:M])], sc, C, pre)
        n = r['n']
        seen['one'] |= bool((n == 1).any())                       # run lengths: 1, across a 16-position thread group, long
        seen['crossing'] |= bool((n >= 17).any())
        seen['long'] |= bool((n >= 64).any())
        seen['marked_zero'] |= bool((r['marks'] & (r['A'] == 0).all(1)).any())
        seen['unmarked'] |= bool((~r['marks']).any())
        assert R.bits(r['grad'][~r['marks']]).tobytes() == R.bits(pre[~r['marks']]).tobytes()
        if M >= R.CELL_AT + R.N_CELL:
            assert (n >= 64).sum() >= 8
        # what the tiny pre-fill of the atomic tests needs: no voxel sums terms anywhere near 2^-100
        multi = (n >= 2)[:, None] & (r['A'] > 0)
        assert not multi.any() or r['A'][multi].min() >= 2.0 ** -60
    if size == (2, 3, 2):                                         # 12 voxels: from 15 samples on every voxel gets real gradient
        seen['marked_zero'] = True
    assert all(seen.values()), seen
    # gradients: zero rows (-0 and +0), single -0.0 entries, junk beyond C
    assert (g[8::9, :C] == 0).all() and np.signbit(g[8::18, :C]).all() and not np.signbit(g[17::18, :C]).all(1).any()
    assert (g[0, :C] != 0).all()
    assert (np.signbit(g[:, :C]) & (g[:, :C] == 0)).any(1)[np.arange(4, R.N_CASE, 13)].all()
    assert (g[:, C:] != 0).all()


@pytest.mark.parametrize('size', R.GRIDS)
def test_the_one_cell_samples_make_the_order_visible(size):
    C = 12
    sc = R.GridScene(size)
    case = R.build_case(size)
    g = R.build_gradients(R.N_CASE, C)
    idx = case['cell']
    assert len(idx) == R.N_CELL and len(np.unique(R.stencil32(case['pts'][idx], sc)['i0'], axis=0)) == 1
    pre = R.build_prefill(sc.n_voxels, C)
    fwd = R.replay32([(case['pts'][idx], g[idx])], sc, C, pre)
    rev = R.replay32([(case['pts'][idx[::-1]], g[idx[::-1]])], sc, C, pre)
    assert fwd['marks'].sum() == 8 and (fwd['n'][fwd['marks']] == R.N_CELL).all()
    changed = (R.bits(fwd['grad']) != R.bits(rev['grad'])).any(1)
    print(f'grid {size}: reversed order changes {changed.sum()} of {fwd["marks"].sum()} marked voxels')
    assert changed.any() and not changed[~fwd['marks']].any()
    np.testing.assert_array_equal(fwd['A'], rev['A'])
    # two shards replay as their concatenation
    two = R.replay32([(case['pts'][idx[:30]], g[idx[:30]]), (case['pts'][idx[30:]], g[idx[30:]])], sc, C, pre)
    assert R.bits(two['grad']).tobytes() == R.bits(fwd['grad']).tobytes()


def test_stencil32_on_hand_computed_points():
    sc = R.GridScene((7, 4, 5))
    p = np.stack([R.XYZ_MIN, R.XYZ_MAX, R.XYZ_MIN - 1, np.array([np.nan, np.inf, -np.inf], np.float32)])
    st = R.stencil32(p, sc)
    assert st['i0'][0].tolist() == [0, 0, 0] and st['w'][0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert st['vox'][0].tolist() == [0, 1, 5, 6, 20, 21, 25, 26]          # z fastest, then y, then x
    assert st['i0'][1].tolist() == [6, 3, 4] and st['ok'][1].tolist() == [True] + [False] * 7
    assert st['vox'][1, 0] == 7 * 4 * 5 - 1 and st['w'][1, 0] == 1
    assert st['i0'][2].tolist() == [-2, -2, -2] and not st['ok'][2].any()
    assert st['i0'][3].tolist() == [-2, 4, -2] and not st['ok'][3].any() # NaN -> -2, +inf -> size, -inf -> -2
    # the centre of cell (3, 1, 2): eight equal weights
    st = R.stencil32(R.to_world(np.array([[3.5, 1.5, 2.5]]), sc.size), sc)
    assert st['ok'].all() and np.allclose(st['w'], 0.125, atol=1e-6)
    assert st['vox'][0, 0] == (3 * 4 + 1) * 5 + 2 and st['vox'][0, 7] == (4 * 4 + 2) * 5 + 3


def test_pack_image_on_a_three_row_example():
    nan = np.float32(np.nan)
    before = np.full((5, 16), 77.0, np.float32)
    before[3, 2] = nan
    pts = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]], np.float32)
    g = np.arange(4 * 64, dtype=np.float32).reshape(4, 64) + 100
    out = R.pack_image(pts, g, 3, 4, 2, before)
    i = lambda m: float(np.array([m], np.int32).view(np.float32)[0])
    want = np.array([[100, 101, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 2, 3, i(3)],
                     [164, 165, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 5, 6, 0],
                     [228, 229, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7, 8, 9, 0],
                     [77, 77, nan] + [77] * 13,
                     [77] * 16], np.float32)
    assert R.bits(out).tobytes() == R.bits(want).tobytes()
    assert out[0, 15:].view(np.int32)[0] == 3
    # the count clamps to the capacity; a count of 0 writes the count alone
    assert R.pack_image(pts, g, 9, 2, 2, before)[0, 15:].view(np.int32)[0] == 2
    assert (R.pack_image(pts, g, 9, 2, 2, before)[2:] == before[2:])[before[2:] == before[2:]].all()
    zero = R.pack_image(pts, g, 0, 4, 12, before)
    assert zero[0, 15:].view(np.int32)[0] == 0
    zero[0, 15] = 77.0
    assert R.bits(zero).tobytes() == R.bits(before).tobytes()
