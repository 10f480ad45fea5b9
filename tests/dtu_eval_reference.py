"""Numpy restatement of the DTU mesh evaluation semantics of include/poseprobe_hip.h (pp_dtu_*) and poseprobe_amd/dtu_eval.py
(DESIGN.md §18): the reference the GPU tests compare with.  It follows lib/dtu_eval.py::eval step by step, with brute-force
neighbours (no scipy, no sklearn: GPU tests import it), points in float32 and squared float32 distances
d2 = (dx dx + dy dy) + dz dz; the thinning is the reference's sequential loop.  tests/test_dtu_eval_host.py checks it against a
recorded run of the reference itself (tests/golden/dtu_eval_synth.npz) and, where sklearn exists, against the reference's calls."""
import numpy as np

PATCH = 60


def icosphere(level):
    p = (1 + 5 ** 0.5) / 2
    V = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, float) / np.linalg.norm(v) for v in V]
    for _ in range(level):
        cache, F2 = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = V[a] + V[b]
                V.append(m / np.linalg.norm(m))
                cache[k] = len(V) - 1
            return cache[k]
        for a, b, c in F:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            F2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = F2
    return np.array(V), np.array(F, np.int32)


def _norm(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def sample_mesh_points(vertices, triangles, thresh, info=None):
    """lib/dtu_eval.py:62-89 -> float32 [N,3]: the referenced vertices in index order, then the sampled points triangle-major,
    i-major, j-minor.  info (a dict) receives the near-tie margins: `count_margin` = the smallest distance of an l / thr from an
    integer, `sum_margin` = the smallest |a + b - 1| over all candidates, and `n` = the (n1, n2) pairs."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3).astype(np.int64)
    tv = v[t]
    v1, v2, p0 = tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0], tv[:, 0]
    l1, l2 = _norm(v1), _norm(v2)
    cr = np.stack([v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1], v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2],
                   v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]], -1)
    area2 = _norm(cr)
    out, count_margin, sum_margin, ns = [], np.inf, np.inf, []
    for k in np.nonzero(area2 > 0)[0]:
        thr = float(thresh) * np.sqrt(l1[k] * l2[k] / area2[k])
        r1, r2 = l1[k] / thr, l2[k] / thr
        count_margin = min(count_margin, abs(r1 - np.round(r1)), abs(r2 - np.round(r2)))
        n1, n2 = np.floor(r1), np.floor(r2)
        ns.append((n1, n2))
        a = (np.arange(int(n1) + 1) + 0.5) / max(n1, 1e-7)
        b = (np.arange(int(n2) + 1) + 0.5) / max(n2, 1e-7)
        s = a[:, None] + b[None, :]
        sum_margin = min(sum_margin, float(np.abs(s - 1).min()))
        ii, jj = np.nonzero(s < 1)
        out.append((v1[k][None] * a[ii, None] + v2[k][None] * b[jj, None]) + p0[k][None])
    referenced = np.zeros(len(v), bool)
    referenced[t.reshape(-1)] = True
    if info is not None:
        info.update(count_margin=float(count_margin), sum_margin=float(sum_margin), n=ns)
    return np.concatenate([v[referenced]] + out, 0).astype(np.float32)


def _d2(points, q):
    d = points - q[None]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def thin_points(points, radius):
    """lib/dtu_eval.py:98-106 in the given order, as the sequential loop -> bool keep mask."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    r2 = np.float32(radius) * np.float32(radius)
    mask = np.ones(len(p), bool)
    for curr in range(len(p)):
        if mask[curr]:
            mask[_d2(p, p[curr]) <= r2] = False
            mask[curr] = True
    return mask


def thin_points_rounds(points, radius):
    """The same mask computed in rounds over (undecided 0, kept 1, removed 2) -> (mask, rounds)."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    r2 = np.float32(radius) * np.float32(radius)
    lower = [np.nonzero(_d2(p[:i], p[i]) <= r2)[0] for i in range(len(p))]
    state, rounds = np.zeros(len(p), np.int8), 0
    while (state == 0).any():
        rounds += 1
        new = state.copy()
        for i in np.nonzero(state == 0)[0]:
            s = state[lower[i]]
            if (s == 1).any():
                new[i] = 2
            elif (s == 2).all():
                new[i] = 1
        state = new
    return state == 1, rounds


def nearest(queries, points, max_dist, chunk=512):
    """-> (d2 float32 [Q], idx int32 [Q]): the exact nearest point by float32 d2, ties to the lowest index; (inf, -1) where no
    point has d2 < max_dist^2."""
    q = np.asarray(queries, np.float32).reshape(-1, 3)
    p = np.asarray(points, np.float32).reshape(-1, 3)
    d2 = np.full(len(q), np.inf, np.float32)
    idx = np.full(len(q), -1, np.int32)
    if len(p) == 0 or len(q) == 0:
        return d2, idx
    md2 = np.float32(max_dist) * np.float32(max_dist)
    for s in range(0, len(q), chunk):
        d = q[s:s + chunk, None, :] - p[None, :, :]
        m = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        i = m.argmin(1)                                 # (the first minimum: the lowest index)
        best = m[np.arange(len(i)), i]
        hit = best < md2
        d2[s:s + chunk] = np.where(hit, best, np.float32(np.inf))
        idx[s:s + chunk] = np.where(hit, i, -1)
    return d2, idx


def _mean(d2):
    d = np.sqrt(d2[np.isfinite(d2)].astype(np.float64))
    return float(d.mean()) if len(d) else float('nan')


def chamfer(vertices, triangles, stl, obs_mask, bb, res, plane, *, max_dist=20, runtime=False, perm=None, scale_mat=None):
    """lib/dtu_eval.py:37-160 on arrays -> dict(mean_d2s, mean_s2d, over_all, n_sampled, n_down, n_in_obs, n_stl_above, down)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    if scale_mat is not None:
        s = np.asarray(scale_mat, np.float64)
        v = v * s[0, 0] + s[:3, 3][None]
    thresh = 0.5 if runtime else 0.2
    pcd = sample_mesh_points(v, triangles, thresh)
    if perm is not None:
        pcd = pcd[np.asarray(perm)]
    down = pcd[thin_points(pcd, thresh)]
    bb = np.asarray(bb).astype(np.float32).reshape(2, 3)
    inbound = ((down >= bb[:1] - PATCH) & (down < bb[1:] + PATCH * 2)).sum(-1) == 3
    data_in = down[inbound]
    obs_mask = np.asarray(obs_mask)
    grid = np.around((data_in.astype(np.float64) - bb[:1].astype(np.float64)) / float(np.asarray(res).reshape(-1)[0])).astype(np.int64)
    grid_inbound = ((grid >= 0) & (grid < np.array(obs_mask.shape)[None])).sum(-1) == 3
    g = grid[grid_inbound]
    in_obs = obs_mask[g[:, 0], g[:, 1], g[:, 2]].astype(bool)
    data_in_obs = data_in[grid_inbound][in_obs]
    stl = np.asarray(stl, np.float32).reshape(-1, 3)
    if runtime:
        num_gt = len(data_in_obs) * 2
        stl = stl[::max(len(stl) // num_gt if num_gt else 1, 1)]
    d2s, _ = nearest(data_in_obs, stl, max_dist)
    P = np.asarray(plane, np.float64).reshape(4)
    s64 = stl.astype(np.float64)
    above = ((P[0] * s64[:, 0] + P[1] * s64[:, 1]) + P[2] * s64[:, 2]) + P[3] > 0
    stl_above = stl[above]
    s2d, _ = nearest(stl_above, data_in, max_dist)
    m1, m2 = _mean(d2s), _mean(s2d)
    return dict(mean_d2s=m1, mean_s2d=m2, over_all=(m1 + m2) / 2, n_sampled=len(pcd), n_down=len(down), n_in_obs=len(data_in_obs),
                n_stl_above=len(stl_above), down=down)
