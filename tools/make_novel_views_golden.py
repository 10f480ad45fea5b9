"""Writes tests/golden/novel_view_poses.npz: a recorded run of the reference's own novel-view pose-path functions.

    python tools/make_novel_views_golden.py /path/to/reference

lib/camera.py (pose, get_novel_view_poses) is imported under the stubs of oracle.ref_harness.  lib/gen_videos.py does not
import as a module (tqdm, imageio, matplotlib are absent): its path functions (generate_spiral_path, generate_spiral_path_dtu and
the helpers they call) are compiled from its source at run time into a namespace that holds what they name; nothing of them is
stored.  The 'dtu' sequence is composed here from those functions exactly as the reference's renderer composes it
(lib/bg_nerf/source/models/renderer.py:1247-1264: the DTU spiral with one turn, inverted, followed by get_novel_view_poses
around the pose whose translation is nearest to the mean).

Stored (cases and inputs: tests/novel_views_reference.py; inputs are regenerated from the case name, not stored):
  spiral.<case>, spiral_dtu.<case>   the two generators on float64 camera-to-world arrays (they compute in numpy float64)
  oscil.<case>, dtu.<case>           get_novel_view_poses and the composed 'dtu' sequence on float32 tensors (the reference's
                                     camera.pose casts to float32)
  oscil.<case>.f64, dtu.<case>.f64   the same with every `.float()` of the run turned into `.double()`, float64 the default dtype
The tool prints, per quantity, the largest difference between the float32 and the float64 run; the tests' tolerance is 4 x that
(the rule of tools/make_eval_golden.py)."""
import argparse
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from tests import novel_views_reference as R      # noqa: E402

PATH_FUNCTIONS = ('pad_poses', 'unpad_poses', 'poses_avg', 'focus_pt_fn', 'normalize', 'viewmatrix', 'generate_spiral_path',
                  'generate_spiral_path_dtu')


def reference(ref_root):
    from oracle import ref_harness
    ref_harness.REF_ROOT = ref_root
    ref_harness.install()
    import importlib
    camera = importlib.import_module('lib.camera')
    path = os.path.join(ref_root, 'lib', 'gen_videos.py')
    nodes = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name in PATH_FUNCTIONS]
    assert len(nodes) == len(PATH_FUNCTIONS), [n.name for n in nodes]
    ns = dict(torch=torch, np=np, camera=camera)
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, 'exec'), ns)
    return camera, ns


def run_paths(camera, ns, poses_w2c, scale):
    """-> {quantity: array}: the oscillation around the centre-most pose and the composed 'dtu' sequence (tensors of the dtype given)."""
    n = R.N_PATH
    centre = (poses_w2c - poses_w2c.mean(dim=0, keepdim=True))[..., 3].norm(dim=-1).argmin()
    oscil = camera.get_novel_view_poses(None, poses_w2c[centre], N=n, scale=scale)
    c2w = ns['generate_spiral_path_dtu'](camera.pose.invert(poses_w2c), n_rots=1, n_frames=n)
    dtu = torch.cat((camera.pose.invert(c2w), camera.get_novel_view_poses(None, poses_w2c[centre], N=n, scale=1)), dim=0)
    return {k: np.asarray(v.detach().cpu().numpy(), np.float64) for k, v in (('oscil', oscil), ('dtu', dtu))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('reference_root')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'novel_view_poses.npz'))
    a = ap.parse_args()
    camera, ns = reference(a.reference_root)
    store, spread = {}, {}
    real_float = torch.Tensor.float
    for case in R.cases():
        name, w2c = case['name'], case['poses_w2c']
        c2w = R.invert(w2c)
        store[f'spiral.{name}'] = np.asarray(ns['generate_spiral_path'](c2w, case['bounds'], n_frames=R.N_SPIRAL), np.float64)[:, :3]
        store[f'spiral_dtu.{name}'] = np.asarray(ns['generate_spiral_path_dtu'](c2w, n_frames=R.N_SPIRAL), np.float64)[:, :3]
        f32 = run_paths(camera, ns, torch.tensor(w2c, dtype=torch.float32), case['scale'])
        torch.Tensor.float = lambda self, *a_, **k_: self.double()
        torch.set_default_dtype(torch.float64)
        try:
            f64 = run_paths(camera, ns, torch.tensor(w2c), case['scale'])
        finally:
            torch.Tensor.float = real_float
            torch.set_default_dtype(torch.float32)
        for k in f32:
            store[f'{k}.{name}'], store[f'{k}.{name}.f64'] = f32[k], f64[k]
            spread[k] = max(spread.get(k, 0.0), float(np.abs(f32[k] - f64[k]).max()))
        print(f'{name}: {w2c.shape[0]} views, spiral {store[f"spiral.{name}"].shape}, dtu spiral {store[f"spiral_dtu.{name}"].shape}, '
              f'oscillation {f32["oscil"].shape}, composed dtu sequence {f32["dtu"].shape}')
    for k, v in sorted(spread.items()):
        print(f'float32 against float64 run, {k}: {v:.3e}  (tolerance of the tests: 4 x = {4 * v:.3e})')
    np.savez_compressed(a.out, **store)
    print(a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
