"""The k0 gradient scatter family, one entry point at a time, against tests/scatter_reference.py (itself checked on the CPU by
tests/test_scatter_reference.py): pp_k0_scatter_samples, pp_k0_pack_samples, pp_k0_scatter_packed (pp_color.hip) and
pp_k0_scatter_samples_sorted, pp_k0_scatter_packed_sorted (pp_scatter_sorted.hip).

Sorted kernels: EQUAL, bit for bit, to replay32, the float32 accumulation in ascending (shard, sample, corner) order the kernels
document (the library is built with -ffp-contract=off and the stencil uses __f*_rn operations, so numpy float32 restates it
exactly).  Never a tolerance.

Atomic kernels, per voxel v and channel, with n_v contributions, A_v = sum |w g|, G_v = sum |g| and eps32 = 2^-23:

    |hip - replay32|  <= 2 n_v eps32 A_v                                  bit-equal where n_v <= 1
    |hip - scatter64| <= 2 (n_v + 8) eps32 A_v + 12 eps32 max(size) G_v

First line: both sides add the identical float32 terms w * g, only the order differs, and a sequential fp32 sum of n terms in any
order is within n eps32 / 2 sum |terms| of the exact sum.  Second line: the first plus the bound replay32 itself meets against
float64 (tests/test_scatter_reference.py: (n_v + 8) eps32 A_v for the sum, 12 eps32 max(size) G_v for the weights, whose three
factors each carry the rounding of the voxel coordinate).  These two lines do not budget for what is in k0_grad BEFORE the
scatter: the atomic kernel adds every term to the stored value, the replay adds their sum once, and each such addition rounds at
the size of the stored value.  They are therefore asserted as they stand on a pre-fill of magnitude 2^-100, far below every
term (tests/test_scatter_reference.py asserts A_v >= 2^-60 wherever n_v >= 2), and a second run on a pre-fill of magnitude 1
asserts the same two lines with A_v + |pre-fill_v| in place of A_v - the pre-fill counted as one more term of the sum - plus
everything that is exact: bit-equality where n_v <= 1, untouched voxels, the touched map.

Every run: rows past the count hold sentinels (in-grid points with large gradients, NaN, +-inf), feature-gradient rows have stride
64 with junk in columns C..63, k0_grad is pre-filled with seeded non-zero values and followed by guard rows, touched is pre-filled
with a 0/1/7 pattern and followed by guard bytes.  touched must come back 1 exactly on the reference's mark set (every in-range
corner of every valid sample, whatever its gradient) and unchanged elsewhere.
"""
import functools

import numpy as np
import pytest
import torch

from tests import scatter_reference as R
from tests.helpers import cu
from tests.test_hip_stage_kernels import XYZ_MAX, XYZ_MIN, scene

pytestmark = pytest.mark.gpu

CS = [1, 4, 12, 16]
PACK_CS = [1, 4, 12]
GUARD = 4096
GUARD_ROWS = 64
GRAD_CANARY = 4321.0
TINY = 2.0 ** -100
# packed tests: (shard counts, rows of each shard's own buffer, a smaller `rows` passed as capacity the way dist.py does)
SHARDS = [((0, 40, 37), 40, 38), ((257, 120), 300, 200)]


def test_bounds_are_those_of_the_stage_kernel_tests():
    assert np.array_equal(R.XYZ_MIN, XYZ_MIN) and np.array_equal(R.XYZ_MAX, XYZ_MAX)


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def case_of(size):
    return R.build_case(size)


@functools.lru_cache(maxsize=None)
def grads_of(C):
    return R.build_gradients(R.N_CASE, C)


def sample_buffers(size, C, count, capacity, lo=0):
    """Host pts [rows,3] and feat_grad [rows,64]: rows below `count` from the case (starting at its row `lo`, cyclic), the rest
    sentinels that would show in the result if a kernel read them."""
    rows = max(count, capacity) + 6
    centre = R.to_world((np.asarray(size) - 1)[None] / 2.0, size)[0]
    pts = np.empty((rows, 3), np.float32)
    g = np.empty((rows, R.FEAT_LD), np.float32)
    k = np.arange(rows) % 6
    pts[:] = centre
    pts[k == 1], pts[k == 2], pts[k == 3] = np.nan, np.inf, -np.inf
    g[:] = np.array([1e3, 5.0, np.nan, np.inf, -np.inf, -7e2], np.float32)[k][:, None]
    idx = (lo + np.arange(count)) % R.N_CASE
    pts[:count], g[:count] = case_of(size)['pts'][idx], grads_of(C)[idx]
    return pts, g


@functools.lru_cache(maxsize=None)
def reference(size, C, spec, scale):
    """replay32 (and scatter64 + pre-fill) of `spec` = ((lo, M), ...): one entry per shard, M valid samples from case row lo."""
    sc = R.GridScene(size)
    shards = []
    for lo, M in spec:
        idx = (lo + np.arange(M)) % R.N_CASE
        shards.append((case_of(size)['pts'][idx], grads_of(C)[idx]))
    pre = R.build_prefill(sc.n_voxels, C, scale=scale)
    r = R.replay32(shards, sc, C, pre)
    r['r64'] = R.scatter64(shards, sc, C) + pre.astype(np.float64)
    r['pre'] = pre
    return r


class Outputs:
    """k0_grad [V,C] pre-filled, with guard rows behind it; touched [V] pre-filled 0/1/7, with guard bytes behind it."""

    def __init__(self, size, C, scale=1.0, touched=True):
        self.V, self.C = int(np.prod(size)), C
        self.pre = R.build_prefill(self.V, C, scale=scale)
        self.grad_all = torch.cat([cu(self.pre), torch.full((GUARD_ROWS, C), GRAD_CANARY, device='cuda')]).contiguous()
        self.grad = self.grad_all[:self.V]
        self.touch_pre = np.array([0, 1, 7], np.uint8)[np.arange(self.V) % 3]
        self.touch_all = torch.cat([torch.from_numpy(self.touch_pre), torch.full((GUARD,), 0xA5, dtype=torch.uint8)]).cuda()
        self.touched = self.touch_all[:self.V] if touched else None

    def grad_host(self):
        assert (self.grad_all[self.V:] == GRAD_CANARY).all(), 'guard rows behind k0_grad were written'
        return self.grad.cpu().numpy()

    def check_touched(self, marks, what):
        t = self.touch_all.cpu().numpy()
        assert (t[self.V:] == 0xA5).all(), f'{what}: guard bytes behind touched were written'
        want = self.touch_pre if self.touched is None or marks is None else np.where(marks, 1, self.touch_pre).astype(np.uint8)
        bad = np.flatnonzero(t[:self.V] != want)
        assert len(bad) == 0, (f'{what}: touched differs at {len(bad)} voxels, first {bad[:5]}: got {t[bad[:5]]}, want '
                               f'{want[bad[:5]]} (marked: {None if marks is None else marks[bad[:5]]})')

    def check_unchanged(self, what):
        assert R.bits(self.grad_host()).tobytes() == R.bits(self.pre).tobytes(), f'{what}: k0_grad was written'
        self.check_touched(None, what)


def workspace(n_samples, short=0):
    """(work, arena): the sorted kernels' workspace inside an arena with GUARD bytes of 0xA5 behind it."""
    from poseprobe_amd import ops
    need = ops.k0_scatter_sorted_workspace(n_samples) - short
    arena = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    return arena[:need], arena


def check_arena(work, arena, what):
    assert (arena[work.numel():] == 0xA5).all(), f'{what}: bytes behind the workspace were written'


def assert_bits(hip, r, what):
    """hip [V,C] float32 == r['grad'] bit for bit; the message says where and how long the voxel's run is."""
    bad = (R.bits(hip) != R.bits(r['grad'])).any(1)
    if bad.any():
        v = int(np.flatnonzero(bad)[0])
        raise AssertionError(f'{what}: {bad.sum()} voxels differ in bits ({(bad & ~r["marks"]).sum()} of them unmarked); first '
                             f'voxel {v}: n_v {r["n"][v]}, hip {hip[v][:4]}, replay {r["grad"][v][:4]}, pre-fill {r["pre"][v][:4]}')


def assert_atomic(hip, r, size, what, prefilled):
    """The two bounds of the module docstring; returns the worst error-to-bound ratios (replay32, scatter64)."""
    n = r['n'][:, None]
    A = r['A'] + (np.abs(r['pre'].astype(np.float64)) if prefilled else 0.0)
    one = (r['n'] <= 1)
    assert_bits(np.where(one[:, None], hip, r['grad']), r, f'{what}, voxels with n_v <= 1')
    h = hip.astype(np.float64)
    e32, b32 = np.abs(h - r['grad']), 2 * n * R.EPS32 * A
    e64, b64 = np.abs(h - r['r64']), 2 * (n + 8) * R.EPS32 * A + 12 * R.EPS32 * max(size) * r['G']
    ratios = []
    for name, e, b in (('replay32', e32, b32), ('scatter64', e64, b64)):
        bad = ~(e <= b)
        q = np.where(b > 0, e / np.where(b > 0, b, 1), 0)
        if bad.any():
            v, c = np.argwhere(bad)[np.argmax(np.where(b[bad] > 0, q[bad], np.inf))]
            raise AssertionError(f'{what}: {bad.sum()} entries beyond the {name} bound; worst voxel {v} channel {c}: hip '
                                 f'{h[v, c]:.9g} ref {(r["grad"] if name == "replay32" else r["r64"])[v, c]:.9g} bound '
                                 f'{b[v, c]:.3g} n_v {r["n"][v]}')
        ratios.append(float(q.max()))
    return ratios


def device_case(size, C, count, capacity, lo=0):
    pts, g = sample_buffers(size, C, count, capacity, lo)
    return cu(pts), cu(g), torch.tensor([count], dtype=torch.int32, device='cuda')


def stale_packed(rows):
    """[rows,16] buffer of stale content: 77.0, with NaN rows in between."""
    p = torch.full((rows, R.PACK_LD), 77.0, device='cuda')
    p[1::3] = float('nan')
    return p


def pack_shards(size, C, counts, cap_buf, rows):
    """Pack every shard into its own stale buffer of cap_buf + 2 rows with capacity `rows`, gather the first `rows` rows as
    dist.py does.  Returns (gathered [n,rows,16], spec for reference(), list of (buffer after, expected image))."""
    from poseprobe_amd import ops
    gathered, spec, images = [], [], []
    for r, count in enumerate(counts):
        lo = 150 * r
        pts, g = sample_buffers(size, C, count, cap_buf, lo)
        buf = stale_packed(cap_buf + 2)
        before = buf.cpu().numpy()
        ops.k0_pack_samples(cu(pts), cu(g), torch.tensor([count], dtype=torch.int32, device='cuda'), rows, C, buf)
        images.append((buf.cpu().numpy(), R.pack_image(pts, g, count, rows, C, before)))
        gathered.append(buf[:rows])
        spec.append((lo, min(count, rows)))
    return torch.stack(gathered).contiguous(), tuple(spec), images


# ------------------------------------------------------------------------------------------------- (a) sorted == replay
@pytest.mark.parametrize('size', R.GRIDS)
@pytest.mark.parametrize('C', CS)
def test_sorted_scatter_is_the_ordered_fp32_replay_bit_for_bit(size, C):
    """pp_k0_scatter_samples_sorted == replay32 in every bit, for every (count, capacity) of R.COUNTS; touched exact; the same
    gradient without a touched map; the workspace's guard intact.  (1, 1) tests the weights alone; from 255 on the case holds 64
    samples in one cell, whose sum changes bits when the order is reversed (tests/test_scatter_reference.py)."""
    from poseprobe_amd import ops
    sc = scene(size, k0_dim=C)
    for count, cap in R.COUNTS:
        what = f'grid {size} C {C} count {count} capacity {cap}'
        r = reference(size, C, ((0, min(count, cap)),), 1.0)
        pts, g, cnt = device_case(size, C, count, cap)
        work, arena = workspace(cap)
        out, bare = Outputs(size, C), Outputs(size, C, touched=False)
        ops.k0_scatter_samples_sorted(sc, pts, cnt, cap, g, out.grad, work, out.touched)
        ops.k0_scatter_samples_sorted(sc, pts, cnt, cap, g, bare.grad, work, None)
        torch.cuda.synchronize()
        assert_bits(out.grad_host(), r, what)
        out.check_touched(r['marks'], what)
        assert_bits(bare.grad_host(), r, what + ', no touched map')
        bare.check_touched(None, what + ', no touched map')
        check_arena(work, arena, what)


@pytest.mark.parametrize('size', R.GRIDS)
@pytest.mark.parametrize('C', PACK_CS)
def test_packed_sorted_scatter_is_the_replay_in_shard_sample_corner_order(size, C):
    """pp_k0_pack_samples + pp_k0_scatter_packed_sorted over ragged shards (an empty one, a full one, stale 77.0 / NaN rows past
    each count) == replay32 over the shards' valid samples in shard order, bit for bit; with capacity = the buffers' row count
    and with a smaller `rows`, which clamps the larger counts."""
    from poseprobe_amd import ops
    sc = scene(size, k0_dim=C)
    for counts, cap_buf, fewer in SHARDS:
        for rows in (cap_buf, fewer):
            what = f'grid {size} C {C} shards {counts} rows {rows} of {cap_buf}'
            packed, spec, _ = pack_shards(size, C, counts, cap_buf, rows)
            r = reference(size, C, spec, 1.0)
            work, arena = workspace(len(counts) * rows)
            out, bare = Outputs(size, C), Outputs(size, C, touched=False)
            ops.k0_scatter_packed_sorted(sc, packed, len(counts), rows, out.grad, work, out.touched)
            ops.k0_scatter_packed_sorted(sc, packed, len(counts), rows, bare.grad, work, None)
            torch.cuda.synchronize()
            assert_bits(out.grad_host(), r, what)
            out.check_touched(r['marks'], what)
            assert_bits(bare.grad_host(), r, what + ', no touched map')
            check_arena(work, arena, what)


# ---------------------------------------------------------------------------------------------------- (b) atomic kernels
def run_atomic(kernel, sc, size, C, count, cap, scale):
    from poseprobe_amd import ops
    pts, g, cnt = device_case(size, C, count, cap)
    out = Outputs(size, C, scale=scale)
    if kernel == 'samples':
        ops.k0_scatter_samples(sc, pts, cnt, cap, g, out.grad, out.touched)
    else:
        packed = stale_packed(cap + 2)
        ops.k0_pack_samples(pts, g, cnt, cap, C, packed)
        ops.k0_scatter_packed(sc, packed, 1, cap, out.grad, out.touched)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('size', R.GRIDS)
@pytest.mark.parametrize('C', CS)
def test_atomic_scatter_is_within_the_reordering_bound_of_the_replay(size, C):
    """pp_k0_scatter_samples and (C <= 12) pp_k0_scatter_packed on the cases of the sorted test: the two bounds of the module
    docstring as they stand on a 2^-100 pre-fill, and with the pre-fill counted as a term on a pre-fill of magnitude 1; voxels
    with n_v <= 1 bit-equal, unmarked voxels bit-unchanged, touched exact.  Prints the worst error-to-bound ratios."""
    sc = scene(size, k0_dim=C)
    worst = {}
    for kernel in ('samples',) + (('packed',) if C <= 12 else ()):
        for count, cap in R.COUNTS:
            for scale in (TINY, 1.0):
                what = f'{kernel}: grid {size} C {C} count {count} capacity {cap} pre-fill {scale:.0e}'
                r = reference(size, C, ((0, min(count, cap)),), scale)
                out = run_atomic(kernel, sc, size, C, count, cap, scale)
                q = assert_atomic(out.grad_host(), r, size, what, prefilled=scale == 1.0)
                out.check_touched(r['marks'], what)
                key = (kernel, 'as stated' if scale == TINY else 'pre-fill as a term')
                worst[key] = np.maximum(worst.get(key, 0), q)
    for (kernel, how), q in worst.items():
        print(f'atomic {kernel}, grid {size} C {C}, bounds {how}: worst |hip - replay32| / bound {q[0]:.3f}, '
              f'worst |hip - scatter64| / bound {q[1]:.3f}')



@pytest.mark.parametrize('size', R.GRIDS)
@pytest.mark.parametrize('C', PACK_CS)
def test_packed_atomic_scatter_over_ragged_shards(size, C):
    """pp_k0_scatter_packed over the ragged shards of the packed sorted test (one block row per shard, shard stride = the
    `rows` passed as capacity): the same bounds and exact properties as the one-shard cases."""
    from poseprobe_amd import ops
    sc = scene(size, k0_dim=C)
    for counts, cap_buf, fewer in SHARDS:
        for rows in (cap_buf, fewer):
            packed, spec, _ = pack_shards(size, C, counts, cap_buf, rows)
            for scale in (TINY, 1.0):
                what = f'grid {size} C {C} shards {counts} rows {rows} of {cap_buf} pre-fill {scale:.0e}'
                r = reference(size, C, spec, scale)
                out = Outputs(size, C, scale=scale)
                ops.k0_scatter_packed(sc, packed, len(counts), rows, out.grad, out.touched)
                torch.cuda.synchronize()
                assert_atomic(out.grad_host(), r, size, what, prefilled=scale == 1.0)
                out.check_touched(r['marks'], what)


# -------------------------------------------------------------------------------------------------------- (c) pack image
@pytest.mark.parametrize('C', PACK_CS)
def test_pack_image_is_exact_in_every_byte(C):
    """pp_k0_pack_samples into a canary-filled buffer LARGER than `capacity` rows == pack_image in every bit: gradient columns,
    zero fill of columns C..11, points, pad, the count in row 0 slot 15 (also for count 0 and for a count above the capacity),
    rows past the count and rows past the capacity untouched."""
    from poseprobe_amd import ops
    size = (7, 4, 5)
    for count, cap in R.COUNTS:
        pts, g = sample_buffers(size, C, count, cap)
        buf = stale_packed(cap + 9)
        buf[-3:] = -123.0
        before = buf.cpu().numpy()
        ops.k0_pack_samples(cu(pts), cu(g), torch.tensor([count], dtype=torch.int32, device='cuda'), cap, C, buf)
        torch.cuda.synchronize()
        got, want = buf.cpu().numpy(), R.pack_image(pts, g, count, cap, C, before)
        bad = np.argwhere(R.bits(got) != R.bits(want))
        assert len(bad) == 0, f'C {C} count {count} capacity {cap}: {len(bad)} elements differ, first (row, column) {bad[:6].tolist()}'
        assert int(got[0, 15:].view(np.int32)[0]) == min(count, cap)
    # the images of the shard tests, packed with a capacity smaller than the buffer
    for counts, cap_buf, fewer in SHARDS:
        for got, want in pack_shards(size, C, counts, cap_buf, fewer)[2]:
            assert R.bits(got).tobytes() == R.bits(want).tobytes(), f'C {C} shards {counts} rows {fewer} of {cap_buf}'


# ----------------------------------------------------------------------------------------------- (d) buffers and refusals
def test_sorted_workspace_is_checked_to_the_byte():
    """One byte less than pp_k0_scatter_sorted_workspace asks for is refused ("workspace too small"), as is a workspace sized for
    fewer samples than the capacity, with k0_grad and touched bit-unchanged; 2^25 sample slots are refused outright."""
    from poseprobe_amd import _lib, ops
    size, C, count, cap = (7, 4, 5), 12, 257, 300
    sc = scene(size, k0_dim=C)
    pts, g, cnt = device_case(size, C, count, cap)
    packed, _, _ = pack_shards(size, C, (257, 120), cap, cap)
    for short, n in ((1, cap), (0, 100)):
        work, arena = workspace(n, short)
        out = Outputs(size, C)
        with pytest.raises(_lib.PoseProbeError, match='workspace too small'):
            ops.k0_scatter_samples_sorted(sc, pts, cnt, cap, g, out.grad, work, out.touched)
        work2, arena2 = workspace(2 * n, short)
        with pytest.raises(_lib.PoseProbeError, match='workspace too small'):
            ops.k0_scatter_packed_sorted(sc, packed, 2, cap, out.grad, work2, out.touched)
        torch.cuda.synchronize()
        out.check_unchanged(f'workspace {short} bytes short of {n} samples')
        check_arena(work, arena, 'refused call')
        check_arena(work2, arena2, 'refused call')
    with pytest.raises(_lib.PoseProbeError):
        ops.k0_scatter_sorted_workspace(2 ** 25)
    with pytest.raises(_lib.PoseProbeError):
        ops.k0_scatter_sorted_workspace(0)
    assert ops.k0_scatter_sorted_workspace(2 ** 25 - 1) > 0


def test_bad_sizes_are_refused_and_nothing_is_written():
    """k0_dim 13 and 16 for the pack and the two packed scatters, capacity 0 for all five entry points: PoseProbeError, outputs
    bit-unchanged."""
    from poseprobe_amd import _lib, ops
    size, count, cap = (7, 4, 5), 37, 40
    for C in (13, 16):
        sc = scene(size, k0_dim=C)
        pts, g, cnt = device_case(size, C, count, cap)
        buf = stale_packed(cap)
        before = buf.cpu().numpy()
        with pytest.raises(_lib.PoseProbeError):
            ops.k0_pack_samples(pts, g, cnt, cap, C, buf)
        packed, _, _ = pack_shards(size, 12, (count,), cap, cap)
        work, arena = workspace(cap)
        out = Outputs(size, C)
        with pytest.raises(_lib.PoseProbeError):
            ops.k0_scatter_packed(sc, packed, 1, cap, out.grad, out.touched)
        with pytest.raises(_lib.PoseProbeError):
            ops.k0_scatter_packed_sorted(sc, packed, 1, cap, out.grad, work, out.touched)
        torch.cuda.synchronize()
        assert R.bits(buf.cpu().numpy()).tobytes() == R.bits(before).tobytes()
        out.check_unchanged(f'k0_dim {C}')
        check_arena(work, arena, f'k0_dim {C}')
    C = 12
    sc = scene(size, k0_dim=C)
    pts, g, cnt = device_case(size, C, count, cap)
    packed, _, _ = pack_shards(size, C, (count,), cap, cap)
    buf = stale_packed(cap)
    before = buf.cpu().numpy()
    work, arena = workspace(cap)
    out = Outputs(size, C)
    calls = [lambda: ops.k0_pack_samples(pts, g, cnt, 0, C, buf),
             lambda: ops.k0_scatter_samples(sc, pts, cnt, 0, g, out.grad, out.touched),
             lambda: ops.k0_scatter_packed(sc, packed, 1, 0, out.grad, out.touched),
             lambda: ops.k0_scatter_samples_sorted(sc, pts, cnt, 0, g, out.grad, work, out.touched),
             lambda: ops.k0_scatter_packed_sorted(sc, packed, 1, 0, out.grad, work, out.touched)]
    for call in calls:
        with pytest.raises(_lib.PoseProbeError):
            call()
    torch.cuda.synchronize()
    assert R.bits(buf.cpu().numpy()).tobytes() == R.bits(before).tobytes()
    out.check_unchanged('capacity 0')
    check_arena(work, arena, 'capacity 0')


# ------------------------------------------------------------------------------------------ (e) non-finite valid samples
def test_valid_rows_with_non_finite_coordinates_contribute_and_mark_nothing():
    """k0_setup clamps floor(u) with fminf(fmaxf(f, -2), size) before the conversion to int: NaN and -inf give -2, +inf gives
    size, so a valid row with such a coordinate has no corner in range.  All four scatter kernels: the result is the replay with
    those rows removed (sorted: bit for bit; atomic: the bounds as stated, on the 2^-100 pre-fill), and they mark nothing."""
    from poseprobe_amd import ops
    size, C, count, cap = (7, 4, 5), 12, 300, 300
    sc, ref_sc = scene(size, k0_dim=C), R.GridScene(size)
    pts, g = sample_buffers(size, C, count, cap)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    bad = {3: (nan, None, None), 50: (None, inf, None), 120: (None, None, -inf), 121: (nan, nan, nan), 200: (inf, -inf, nan)}
    for row, xyz in bad.items():
        assert (g[row, :C] != 0).any()
        for a, v in enumerate(xyz):
            if v is not None:
                pts[row, a] = v
    keep = np.setdiff1d(np.arange(count), list(bad))
    assert R.stencil32(pts[keep], ref_sc)['ok'].any(1).sum() > 100 and not R.stencil32(pts[list(bad)], ref_sc)['ok'].any()
    refs = {}
    for scale in (1.0, TINY):
        pre = R.build_prefill(ref_sc.n_voxels, C, scale=scale)
        r = R.replay32([(pts[keep], g[keep])], ref_sc, C, pre)
        r['r64'], r['pre'] = R.scatter64([(pts[keep], g[keep])], ref_sc, C) + pre.astype(np.float64), pre
        refs[scale] = r
    d_pts, d_g, cnt = cu(pts), cu(g), torch.tensor([count], dtype=torch.int32, device='cuda')
    packed = stale_packed(cap)
    ops.k0_pack_samples(d_pts, d_g, cnt, cap, C, packed)
    work, arena = workspace(cap)
    for kernel in ('samples_sorted', 'packed_sorted', 'samples', 'packed'):
        scale = 1.0 if kernel.endswith('sorted') else TINY
        out = Outputs(size, C, scale=scale)
        if kernel == 'samples_sorted':
            ops.k0_scatter_samples_sorted(sc, d_pts, cnt, cap, d_g, out.grad, work, out.touched)
        elif kernel == 'packed_sorted':
            ops.k0_scatter_packed_sorted(sc, packed, 1, cap, out.grad, work, out.touched)
        elif kernel == 'samples':
            ops.k0_scatter_samples(sc, d_pts, cnt, cap, d_g, out.grad, out.touched)
        else:
            ops.k0_scatter_packed(sc, packed, 1, cap, out.grad, out.touched)
        torch.cuda.synchronize()
        if scale == 1.0:
            assert_bits(out.grad_host(), refs[scale], kernel)
        else:
            assert_atomic(out.grad_host(), refs[scale], size, kernel, prefilled=False)
        out.check_touched(refs[scale]['marks'], kernel)
    check_arena(work, arena, 'non-finite rows')
