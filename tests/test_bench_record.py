"""bench.py's plain run: the headline record, the per-step randomness it draws up front, and --dump-outputs."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests.conftest import ROOT


def test_step_randomness_does_not_depend_on_the_workers():
    sys.path.insert(0, ROOT)
    import bench
    from poseprobe_amd import synthetic as syn
    seeds = range(2000, 2070)
    forked = bench.all_step_randomness(3 * 40 * 40, 256, seeds, workers=2)
    assert len(forked) == len(seeds)
    for (idx, jit), s in zip(forked, seeds):
        ref_idx, ref_jit = syn.step_randomness(3 * 40 * 40, 256, seed=s)
        assert np.array_equal(idx, ref_idx) and np.array_equal(jit, ref_jit)


def test_write_outputs_names_dtypes_and_size(tmp_path):
    """A stand-in engine on the CPU with the real parameter block: every array is float32, the grid sample is the same on
    every call, and the files stay far below 64 MB at the benchmark's 160^3 x 12 colour grid."""
    sys.path.insert(0, ROOT)
    import bench
    from poseprobe_amd.engine import FlatParams
    X, Y, Z, C = 160, 160, 160, 12
    g = torch.Generator().manual_seed(0)
    k0 = torch.randn(X, Y, Z, C, generator=g)
    flat = FlatParams('cpu')
    flat.data.copy_(torch.randn(flat.n, generator=g))
    eng = types.SimpleNamespace(ws=types.SimpleNamespace(rgb_marched=torch.rand(1024, 3, generator=g), loss_out=torch.rand(8)),
                                se3=torch.randn(3, 6, generator=g), flat=flat,
                                k0_reference_layout=lambda: k0.permute(3, 0, 1, 2)[None])
    shapes = bench.write_outputs(eng, str(tmp_path / 'a'))
    bench.write_outputs(eng, str(tmp_path / 'b'))
    assert set(shapes) == {'rgb_marched', 'losses', 'se3', 'sdf_ab', 'rgbnet', 'warp', 'k0_sample'}
    total = 0
    for name in shapes:
        a, b = np.load(tmp_path / 'a' / f'{name}.npy'), np.load(tmp_path / 'b' / f'{name}.npy')
        assert a.dtype == np.float32 and list(a.shape) == shapes[name] and np.array_equal(a, b), name
        total += os.path.getsize(tmp_path / 'a' / f'{name}.npy')
    assert total <= 64 << 20
    sample = np.load(tmp_path / 'a' / 'k0_sample.npy')
    assert 0.9 * bench.DUMP_K0_SAMPLES <= sample.size <= bench.DUMP_K0_SAMPLES
    # the sample is drawn from the [C,X,Y,Z] reference layout: the first entries are channel-0 voxels
    pick = np.unique(np.random.default_rng(0).integers(0, k0.numel(), bench.DUMP_K0_SAMPLES))
    c, x, y, z = np.unravel_index(pick[:16], (C, X, Y, Z))
    assert np.array_equal(sample[:16], k0[x, y, z, c].numpy())
    assert np.array_equal(np.load(tmp_path / 'a' / 'rgbnet.npy'), flat.view('rgbnet').numpy())


def _plain_run(out_dir, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                        '--grid', '32', '--hw', '64', '--n-rand', '256', '--dump-outputs', str(out_dir)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_record_and_dumps_the_last_step(tmp_path):
    """Two small plain runs with the same arguments: the contract's fields only (the --full objects stay out), `steps` timed
    steps, and the dumped outputs of the last one - the same in both runs up to rounding (enough steps that free-running
    trajectories would already have drifted apart)."""
    runs = [_plain_run(tmp_path / name, 40, 2) for name in ('a', 'b')]
    for d in runs:
        assert d['metric'] == 'rays_per_sec_train_step' and d['unit'] == 'rays/s' and d['higher_is_better'] is True
        assert d['steps'] == 40 and d['warmup'] == 2 and d['n_gpus'] == 1 and d['dtype'].startswith('f32')
        assert abs(d['value'] - 256 / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
        assert not {'roofline', 'roofline_grid', 'roofline_mlp', 'dual_branch', 'cpu_baseline', 'psnr_parity'} & set(d)
    rgb = np.load(tmp_path / 'a' / 'rgb_marched.npy')
    assert rgb.shape == (256, 3) and rgb.dtype == np.float32 and np.isfinite(rgb).all()
    for name in ('rgb_marched', 'losses', 'se3', 'sdf_ab', 'rgbnet', 'warp', 'k0_sample'):
        a, b = np.load(tmp_path / 'a' / f'{name}.npy'), np.load(tmp_path / 'b' / f'{name}.npy')
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), name
        err = np.abs(a.astype(np.float64) - b).max()
        assert err <= 1e-5 * np.abs(a).max() + 1e-12, f'{name}: runs differ by {err:.3e} (max |a| {np.abs(a).max():.3e})'
