"""Writes tests/golden/dtu_eval_synth.npz: a recorded run of the reference's own lib/dtu_eval.py::eval on a small synthetic scene.

    python tools/make_dtu_eval_golden.py /path/to/reference [--seed 1]

The reference module runs unchanged (it needs numpy, scipy, sklearn and tqdm on the host) under three stubs:
  - a stub `trimesh` module: `load` returns the mesh (vertices, faces, remove_unreferenced_vertices) for the mesh path and the scan
    as a float64 array for the scan path; `PointCloud(x).export` records x, the thinned point set;
  - `np.random.default_rng` is replaced by an object whose `shuffle(x, axis)` applies a stored permutation, so that the fixture
    carries `perm` explicitly;
  - the module is registered in `sys.modules` under its import name, so that the multiprocessing pool can pickle its worker.
The two .mat inputs are written with scipy.io.savemat into a temporary directory.

Scene: a two-level icosphere (320 triangles) of radius 6 - coarse enough that runtime=True (thresh 0.5) samples triangle
interiors too -, 6000 scan points on a noisy shell, a 41^3 observation mask that cuts the sphere, a ground plane that cuts the scan.

Stored: the inputs (vertices, triangles, stl, obs_mask, bb, res, plane, perm_std / perm_rt) and, per mode, the reference's three
means, its thinned point set and the counts.  The tool refuses to write unless the float32 restatement
(tests/dtu_eval_reference.py) keeps exactly the reference's point set in both modes; it prints the relative difference of the
means, from which tests/test_dtu_eval_host.py takes its tolerance."""
import argparse
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from tests import dtu_eval_reference as R      # noqa: E402


def scene(seed):
    v, t = R.icosphere(2)
    verts = (v * 6.0 + 10.0).astype(np.float32)
    rs = np.random.RandomState(seed)
    d = rs.randn(6000, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    stl = (d * (6.15 + 0.05 * rs.randn(6000, 1)) + 10.0).astype(np.float32)
    obs = np.zeros((41, 41, 41), np.uint8)
    obs[:22] = 1
    return dict(vertices=verts, triangles=t, stl=stl, obs_mask=obs, bb=np.array([[0, 0, 0], [20, 20, 20]], np.float32),
                res=np.float32(0.5), plane=np.array([0, 0, 1, -8.0]))


def run_reference(ref_root, s, seed):
    import scipy.io
    box = {}

    class FakeMesh:
        def __init__(self):
            self.vertices, self.faces = s['vertices'].astype(np.float64), s['triangles']

        def remove_unreferenced_vertices(self):
            pass

    class PointCloud:
        def __init__(self, x):
            box['down'] = np.array(x)

        def export(self, *a):
            pass

    class Rng:
        def shuffle(self, x, axis=0):
            p = np.random.RandomState(seed + len(x)).permutation(len(x))
            box['perm'], box['n_sampled'] = p, len(x)
            x[:] = x[p]

    tm = types.ModuleType('trimesh')
    tm.load = lambda p: FakeMesh() if str(p).endswith('mesh.ply') else s['stl'].astype(np.float64)
    tm.PointCloud = PointCloud
    sys.modules['trimesh'] = tm
    spec = importlib.util.spec_from_file_location('ref_dtu_eval', os.path.join(ref_root, 'lib', 'dtu_eval.py'))
    m = importlib.util.module_from_spec(spec)
    sys.modules['ref_dtu_eval'] = m
    spec.loader.exec_module(m)
    real_rng = np.random.default_rng
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'ObsMask'))
        scipy.io.savemat(os.path.join(tmp, 'ObsMask', 'ObsMask1_10.mat'), dict(ObsMask=s['obs_mask'], BB=s['bb'], Res=s['res']))
        scipy.io.savemat(os.path.join(tmp, 'ObsMask', 'Plane1.mat'), dict(P=s['plane'].reshape(4, 1)))
        cwd = os.getcwd()
        os.chdir(tmp)
        np.random.default_rng = lambda: Rng()
        try:
            for tag, runtime in (('std', False), ('rt', True)):
                means = m.eval('mesh.ply', 1, tmp, dataset_dir=tmp, runtime=runtime)
                out[tag] = dict(means=np.array(means, np.float64), down=box['down'].astype(np.float32), perm=box['perm'],
                                n_sampled=box['n_sampled'])
        finally:
            np.random.default_rng = real_rng
            os.chdir(cwd)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('reference_root')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'dtu_eval_synth.npz'))
    a = ap.parse_args()
    s = scene(a.seed)
    ref = run_reference(a.reference_root, s, a.seed)
    store = dict(s)
    worst = 0.0
    for tag, runtime in (('std', False), ('rt', True)):
        r = ref[tag]
        mine = R.chamfer(s['vertices'], s['triangles'], s['stl'], s['obs_mask'], s['bb'], s['res'], s['plane'], runtime=runtime,
                         perm=r['perm'])
        same = mine['n_sampled'] == r['n_sampled'] and np.array_equal(mine['down'], r['down'])
        rel = np.abs(np.array([mine['mean_d2s'], mine['mean_s2d'], mine['over_all']]) - r['means']) / np.abs(r['means'])
        worst = max(worst, float(rel.max()))
        print(f'runtime={runtime}: reference means {r["means"].tolist()}  sampled {r["n_sampled"]} kept {len(r["down"])}  '
              f'in_obs {mine["n_in_obs"]} stl_above {mine["n_stl_above"]}  restatement keeps the same set: {same}  '
              f'relative difference of the means {rel.tolist()}')
        if not same:
            sys.exit('the float32 restatement does not keep the reference\'s point set: choose another --seed')
        store.update({f'perm_{tag}': r['perm'].astype(np.int32), f'means_{tag}': r['means'], f'down_{tag}': r['down'],
                      f'counts_{tag}': np.array([mine['n_sampled'], mine['n_down'], mine['n_in_obs'], mine['n_stl_above']], np.int64)})
    print(f'largest relative difference {worst:.3e}: tolerance of the tests = max(10 x this, 1e-6) = {max(10 * worst, 1e-6):.3e}')
    np.savez_compressed(a.out, **store)
    print(a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
