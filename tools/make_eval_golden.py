"""Writes tests/golden/eval_metrics.npz: a recorded run of the reference's own score functions.

    python tools/make_eval_golden.py /path/to/reference

lib/utils.py (rgb_ssim), lib/camera.py (rotation_distance), lib/align_trajectories.py and external/ATE are imported under the
stubs of oracle.ref_harness.  eval.py does not import as a module (torchvision, mmcv, ... are absent): its four alignment
functions (evaluate_camera_alignment, prealign_w2c_large_camera_systems, prealign_w2c_small_camera_systems,
backtrack_from_aligning_the_trajectory) are compiled from its source at run time into a namespace that holds what they name;
nothing of them is stored.

Stored (cases and inputs: tests/evaluation_reference.py; inputs are regenerated from the case name, not stored):
  tile                        the tile edge T the SSIM shapes were derived from
  ssim.<case>.<i>.value/.map  rgb_ssim of pair i of the case on float64 arrays
  ssim.<case>.<i>.value32/.map32   the same function fed the arrays rounded to float32: the yardstick of tests/test_hip_ssim.py
  pose.<case>.<fn>.<field>    outputs of the pose functions on float32 tensors (the reference's camera.pose casts to float32)
  pose.<case>.<fn>.<field>.f64     the same with every `.float()` of the run turned into `.double()`, on float64 tensors
The tool prints, per pose quantity, the largest difference between the float32 and the float64 run (the tests' tolerance is
4 x that), and refuses to write unless tests/evaluation_reference.py's SSIM restatement agrees with the reference to 1e-12."""
import argparse
import ast
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from tests import evaluation_reference as R      # noqa: E402

EVAL_FUNCTIONS = ('evaluate_camera_alignment', 'prealign_w2c_large_camera_systems', 'prealign_w2c_small_camera_systems',
                  'backtrack_from_aligning_the_trajectory')


def reference(ref_root):
    from oracle import ref_harness
    ref_harness.REF_ROOT = ref_root
    ref_harness.install()
    import importlib
    utils = importlib.import_module('lib.utils')
    camera = importlib.import_module('lib.camera')
    align = importlib.import_module('lib.align_trajectories')
    from easydict import EasyDict as edict
    path = os.path.join(ref_root, 'eval.py')
    nodes = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name in EVAL_FUNCTIONS]
    assert len(nodes) == len(EVAL_FUNCTIONS), [n.name for n in nodes]
    ns = dict(torch=torch, np=np, camera=camera, edict=edict, align_ate_c2b_use_a2b=align.align_ate_c2b_use_a2b, device='cpu',
              logger=types.SimpleNamespace(info=lambda *a, **k: None))
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, 'exec'), ns)
    return utils, camera, ns


def run_poses(camera, ns, pose, GT):
    """-> {fn.field: array} of every pose function on one case (tensors of the dtype given)."""
    out = {}
    c2w, c2w_GT = camera.pose.invert(pose), camera.pose.invert(GT)
    out['rotation_distance.angle'] = camera.rotation_distance(c2w[..., :3], c2w_GT[..., :3])
    e = ns['evaluate_camera_alignment'](pose, GT)
    out['unaligned.R'], out['unaligned.t'] = e.R, e.t
    for tag, fn in (('small', 'prealign_w2c_small_camera_systems'), ('large', 'prealign_w2c_large_camera_systems')):
        aligned, sim3 = ns[fn](pose, GT)
        assert sim3.type == 'traj_align'
        e = ns['evaluate_camera_alignment'](aligned, GT)
        sim3.R, sim3.t = sim3.R.to(GT.dtype), sim3.t.to(GT.dtype)     # (the trajectory alignment returns float32 in either run)
        back = ns['backtrack_from_aligning_the_trajectory'](GT, sim3)
        out.update({f'{tag}.aligned': aligned, f'{tag}.sim3_R': sim3.R, f'{tag}.sim3_t': sim3.t, f'{tag}.sim3_s': torch.as_tensor(sim3.s),
                    f'{tag}.R': e.R, f'{tag}.t': e.t, f'{tag}.backtrack': back})
    return {k: np.asarray(v.detach().cpu().numpy(), np.float64) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('reference_root')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'eval_metrics.npz'))
    a = ap.parse_args()
    utils, camera, ns = reference(a.reference_root)
    store = {'tile': np.int32(R.GOLDEN_T)}
    worst = 0.0
    for case in R.ssim_cases(R.GOLDEN_T):
        for i, (x, y) in enumerate(case['pairs']):
            kw = dict(max_val=case['max_val'], filter_size=case['fs'])
            m = utils.rgb_ssim(x, y, return_map=True, **kw)
            v = utils.rgb_ssim(x, y, **kw)
            x32, y32 = x.astype(np.float32), y.astype(np.float32)
            m32 = np.asarray(utils.rgb_ssim(x32, y32, return_map=True, **kw), np.float64)
            v32 = np.float64(utils.rgb_ssim(x32, y32, **kw))
            mine = R.rgb_ssim(x, y, return_map=True, **kw)
            d = max(float(np.abs(mine - m).max()), abs(float(R.rgb_ssim(x, y, **kw)) - float(v)))
            worst = max(worst, d)
            key = f'ssim.{case["name"]}.{i}'
            store.update({key + '.value': np.float64(v), key + '.map': m, key + '.value32': v32, key + '.map32': m32})
            print(f'{key}: {x.shape} fs {case["fs"]}  value {float(v):.9g}  float32-input run: value off by {abs(v32 - v):.3e}, '
                  f'map by {np.abs(m32 - m).max():.3e}  restatement off by {d:.3e}')
    if worst > 1e-12:
        sys.exit(f'the SSIM restatement differs from the reference by {worst:.3e}')
    spread = {}
    real_float = torch.Tensor.float
    for case in R.pose_cases():
        f32 = run_poses(camera, ns, torch.tensor(case['pose'], dtype=torch.float32), torch.tensor(case['GT'], dtype=torch.float32))
        torch.Tensor.float = lambda self, *a_, **k_: self.double()
        try:
            f64 = run_poses(camera, ns, torch.tensor(case['pose']), torch.tensor(case['GT']))
        finally:
            torch.Tensor.float = real_float
        for k in f32:
            store[f'pose.{case["name"]}.{k}'] = f32[k]
            store[f'pose.{case["name"]}.{k}.f64'] = f64[k]
            q = k.split('.')[1]
            spread[q] = max(spread.get(q, 0.0), float(np.abs(f32[k] - f64[k]).max()))
        print(f'pose.{case["name"]}: mean R / t error  unaligned {f32["unaligned.R"].mean():.3f} / {f32["unaligned.t"].mean():.3f}  '
              f'small {f32["small.R"].mean():.4f} / {f32["small.t"].mean():.4f}  large {f32["large.R"].mean():.4f} / '
              f'{f32["large.t"].mean():.4f}')
    for q, v in sorted(spread.items()):
        print(f'float32 against float64 run, {q}: {v:.3e}  (tolerance of the tests: 4 x = {4 * v:.3e})')
    np.savez_compressed(a.out, **store)
    print(a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
