"""Float64 numpy restatement of the PnP-RANSAC semantics of include/poseprobe_hip.h (pp_pnp_ransac): the reference
the GPU tests compare with, itself tested against mathematics in tests/test_pnp_host.py.

Deliberately NOT the kernel's algorithm where the semantics leave a choice: the quartic of Grunert's P3P is formed with numpy's
polynomial products and solved by `np.roots` (companion-matrix eigenvalues; the kernel iterates Durand-Kerner), and
`hypothesis(..., shift=1 or 2)` solves the same problem on a cyclic permutation of the three points - a different quartic with
the same solution set, i.e. a stand-in for a different closed-form solver."""
import numpy as np

REAL_TOL = 1e-6          # a root counts as real iff |Im z| <= REAL_TOL * max(1, |z|)


# ---- projection -------------------------------------------------------------------------------------------------------------------
def project(T, intr, world, pix):
    """T [3,4], intr (fx, fy, cx, cy), world [n,3], pix [n,2] -> (depth [n], squared pixel error [n])."""
    fx, fy, cx, cy = (float(v) for v in intr)
    c = world @ T[:, :3].T + T[:, 3]
    with np.errstate(divide='ignore', invalid='ignore'):
        du = fx * c[:, 0] / c[:, 2] + cx - pix[:, 0]
        dv = fy * c[:, 1] / c[:, 2] + cy - pix[:, 1]
    return c[:, 2], du * du + dv * dv


def bearings(pix, intr):
    fx, fy, cx, cy = (float(v) for v in intr)
    j = np.stack([(pix[:, 0] - cx) / fx, (pix[:, 1] - cy) / fy, np.ones(len(pix))], -1)
    return j / np.linalg.norm(j, axis=1, keepdims=True)


# ---- P3P ----------------------------------------------------------------------------------------------------------------------------
def frame(A0, A1, A2):
    """Rows: e1 along A1 - A0, e2 = e3 x e1, e3 along the triangle's normal."""
    e1 = (A1 - A0) / np.linalg.norm(A1 - A0)
    n = np.cross(e1, A2 - A0)
    e3 = n / np.linalg.norm(n)
    return np.stack([e1, np.cross(e3, e1), e3])


def cosine_law(s, cos, side2):
    (ca, cb, cg), (a2, b2, c2) = cos, side2
    return np.array([s[1] * s[1] + s[2] * s[2] - 2.0 * s[1] * s[2] * ca - a2, s[0] * s[0] + s[2] * s[2] - 2.0 * s[0] * s[2] * cb - b2,
                     s[0] * s[0] + s[1] * s[1] - 2.0 * s[0] * s[1] * cg - c2])


def polish(s, cos, side2):
    """Up to three Newton steps on the three cosine-law equations, each taken only if it lowers the residual: the elimination
    behind the quartic loses digits where D(v) is small, the equations themselves do not."""
    ca, cb, cg = cos
    f = cosine_law(s, cos, side2)
    for _ in range(3):
        J = 2.0 * np.array([[0.0, s[1] - s[2] * ca, s[2] - s[1] * ca], [s[0] - s[2] * cb, 0.0, s[2] - s[0] * cb],
                            [s[0] - s[1] * cg, s[1] - s[0] * cg, 0.0]])
        try:
            z = s - np.linalg.solve(J, f)
        except np.linalg.LinAlgError:
            break
        g = cosine_law(z, cos, side2)
        if not g @ g < f @ f:
            break
        s, f = z, g
    return s


def p3p(X, j):
    """X [3,3] world points, j [3,3] unit bearings -> list of poses T [3,4] with T X_i = s_i j_i, s_i > 0 (Grunert 1841, as in
    Haralick et al. 1994: s2 = u s1, s3 = v s1, u = N(v) / D(v), a quartic in v).  Exactly collinear triples: none."""
    d01, d02, d12 = X[1] - X[0], X[2] - X[0], X[2] - X[1]
    n = np.array([d01[1] * d02[2] - d01[2] * d02[1], d01[2] * d02[0] - d01[0] * d02[2], d01[0] * d02[1] - d01[1] * d02[0]])
    if not n[0] * n[0] + n[1] * n[1] + n[2] * n[2] > 0.0:
        return []
    a2, b2, c2 = d12 @ d12, d02 @ d02, d01 @ d01
    ca, cb, cg = j[1] @ j[2], j[0] @ j[2], j[0] @ j[1]
    q1, k = (a2 - c2) / b2, c2 / b2
    N = np.array([1.0 + q1, -2.0 * q1 * cb, q1 - 1.0])          # ascending powers of v
    D = np.array([2.0 * cg, -2.0 * ca])
    M = np.array([1.0 - k, 2.0 * k * cb, -k])                   # 1 - W
    Q = np.convolve(N, N) + np.convolve(np.convolve(D, D), M)
    Q[:4] -= 2.0 * cg * np.convolve(N, D)
    if Q[4] == 0.0 or not np.isfinite(Q).all():
        return []
    Fw = frame(X[0], X[1], X[2])
    out = []
    for z in np.roots(Q[::-1]):
        if abs(z.imag) > REAL_TOL * max(1.0, abs(z)):
            continue
        v = float(z.real)
        Dv = D[0] + D[1] * v
        if not v > 0.0 or Dv == 0.0:
            continue
        u = (N[0] + v * (N[1] + v * N[2])) / Dv
        den = 1.0 + v * v - 2.0 * v * cb
        if not (u > 0.0 and den > 0.0):
            continue
        s1 = np.sqrt(b2 / den)
        s = polish(np.array([s1, u * s1, v * s1]), (ca, cb, cg), (a2, b2, c2))
        if not (s > 0.0).all():
            continue
        C = s[:, None] * j
        with np.errstate(divide='ignore', invalid='ignore'):
            R = frame(C[0], C[1], C[2]).T @ Fw
        out.append(np.concatenate([R, (C[0] - R @ X[0])[:, None]], 1))
    return out


def hypothesis(world, pix, valid, intr, s, shift=0):
    """The pose of one sample s[4] or None (invalid).  shift: cyclic permutation of the three P3P points."""
    P = len(world)
    s = [int(v) for v in s]
    if any(v < 0 or v >= P for v in s) or len(set(s)) < 4 or not all(valid[v] for v in s):
        return None
    order = [s[(a + shift) % 3] for a in range(3)]
    best, best_e = None, np.inf
    for T in p3p(world[order], bearings(pix[order], intr)):
        depth, e2 = project(T, intr, world[s], pix[s])
        if (depth > 0).all() and e2[3] < best_e:
            best, best_e = T, e2[3]
    return best


# ---- refinement -------------------------------------------------------------------------------------------------------------------
def se3_exp(w, tau):
    th2 = float(w @ w)
    if th2 < 1e-12:
        A, B, C = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        th = np.sqrt(th2)
        A, B = np.sin(th) / th, (1.0 - np.cos(th)) / th2
        C = (1.0 - A) / th2
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    W2 = np.outer(w, w) - th2 * np.eye(3)
    return np.eye(3) + A * W + B * W2, (np.eye(3) + B * W + C * W2) @ tau


def gauss_newton(T, intr, world, pix, iters):
    """`iters` steps on sum |projection - pix|^2 with T <- exp(delta) T; stops at a non-positive Cholesky pivot."""
    fx, fy, cx, cy = (float(v) for v in intr)
    T = T.copy()
    for _ in range(iters):
        c = world @ T[:, :3].T + T[:, 3]
        x, y, iz = c[:, 0], c[:, 1], 1.0 / c[:, 2]
        ru, rv = fx * x * iz + cx - pix[:, 0], fy * y * iz + cy - pix[:, 1]
        a0, a2, b1, b2 = fx * iz, -fx * x * iz * iz, fy * iz, -fy * y * iz * iz
        o = np.zeros_like(x)
        Ju = np.stack([a2 * y, a0 * c[:, 2] - a2 * x, -a0 * y, a0, o, a2], 1)
        Jv = np.stack([b2 * y - b1 * c[:, 2], -b2 * x, b1 * x, o, b1, b2], 1)
        Hm, g = Ju.T @ Ju + Jv.T @ Jv, Ju.T @ ru + Jv.T @ rv
        try:
            L = np.linalg.cholesky(Hm)
        except np.linalg.LinAlgError:
            break
        d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        if not np.isfinite(d).all():
            break
        R, t = se3_exp(d[:3], d[3:])
        T = np.concatenate([R @ T[:, :3], (R @ T[:, 3] + t)[:, None]], 1)
    return T


# ---- RANSAC -------------------------------------------------------------------------------------------------------------------------
def ransac(world, pix, valid, intr, samples, reproj_error=8.0, refine_iters=10, min_inliers=6, fallback=None, shift=0,
           exact=False):
    """-> dict(w2c [3,4] float32, inliers [P] uint8, info [2] int32, flags [H] bool, counts [H] (-1 = invalid), poses [H,3,4],
    masks [H,P] bool, margin = the smallest | error - reproj_error | in pixels over the valid rows in front of the camera of every
    valid hypothesis, pose64 = the refined pose before rounding)."""
    inner = np.float64 if exact else np.float32             # exact: float64 inputs as they are (the checks against mathematics)
    world = np.asarray(world, inner).astype(np.float64)
    pix = np.asarray(pix, inner).astype(np.float64)
    intr = np.asarray(intr, inner).astype(np.float64)
    P, H = len(world), len(samples)
    valid = np.ones(P, bool) if valid is None else np.asarray(valid).astype(bool)
    thr2 = float(np.float32(reproj_error)) ** 2
    flags, counts = np.zeros(H, bool), np.full(H, -1, np.int64)
    poses, masks, margin = np.zeros((H, 3, 4)), np.zeros((H, P), bool), np.inf
    for h in range(H):
        T = hypothesis(world, pix, valid, intr, samples[h], shift)
        if T is None:
            continue
        depth, e2 = project(T, intr, world, pix)
        front = valid & (depth > 0)
        masks[h] = front & (e2 < thr2)
        flags[h], counts[h], poses[h] = True, masks[h].sum(), T
        if front.any():
            margin = min(margin, float(np.abs(np.sqrt(e2[front]) - np.sqrt(thr2)).min()))
    best = int(np.argmax(counts))                   # the first of the largest: ties go to the lowest index
    out = dict(flags=flags, counts=counts, poses=poses, masks=masks, margin=margin)
    if counts[best] < min_inliers:
        fb = np.eye(4)[:3] if fallback is None else np.asarray(fallback)
        out.update(w2c=fb.astype(np.float32), pose64=None, inliers=np.zeros(P, np.uint8), info=np.array([0, -1], np.int32))
        return out
    m = masks[best]
    T = gauss_newton(poses[best], intr, world[m], pix[m], refine_iters)
    out.update(w2c=T.astype(np.float32), pose64=T, inliers=m.astype(np.uint8), info=np.array([counts[best], best], np.int32))
    return out


# ---- synthetic cases ---------------------------------------------------------------------------------------------------------------
INTR = np.array([500.0, 500.0, 200.0, 200.0], np.float32)


def rotation(axis, angle):
    return se3_exp(np.asarray(axis, np.float64) / np.linalg.norm(axis) * angle, np.zeros(3))[0]


def synthetic(P, outliers=0.0, sigma=0.0, seed=0, invalid=0.1, round32=True, planar=False):
    """A random rotation of 0.4 rad, points 0.4 randn at distance about 3, intrinsics (500, 500, 200, 200), pixel noise sigma, a
    fraction of the matches replaced by uniform pixels, a fraction of the rows invalid; everything rounded to fp32 (round32=False
    keeps the pixels in float64: rounding them alone moves the pose by about 1e-7).
    -> dict(world, pix, valid uint8, intr, T [3,4] float64 = the generating pose, outlier [P] bool)."""
    rng = np.random.RandomState(seed)
    R = rotation(rng.randn(3), 0.4)
    t = np.array([0.0, 0.0, 3.0]) + 0.1 * rng.randn(3)
    world = (0.4 * rng.randn(P, 3)).astype(np.float32)
    if planar:
        world[:, 2] = 0.125
    c = world.astype(np.float64) @ R.T + t
    pix = np.stack([INTR[0] * c[:, 0] / c[:, 2] + INTR[2], INTR[1] * c[:, 1] / c[:, 2] + INTR[3]], -1)
    pix = pix + sigma * rng.randn(P, 2)
    outlier = rng.rand(P) < outliers
    pix[outlier] = rng.rand(int(outlier.sum()), 2) * 400.0
    valid = (rng.rand(P) >= invalid).astype(np.uint8)
    return dict(world=world, pix=pix.astype(np.float32) if round32 else pix, valid=valid, intr=INTR.copy(), T=np.concatenate([R, t[:, None]], 1),
                outlier=outlier)


def draw(valid, H, seed=0):
    """[H,4] int32: four distinct valid rows per hypothesis."""
    rng = np.random.RandomState(seed)
    rows = np.flatnonzero(np.asarray(valid))
    return np.stack([rng.choice(rows, 4, replace=False) for _ in range(H)]).astype(np.int32)


def pose_distance(T, T_ref):
    """(rotation angle in degrees, translation distance) between two poses."""
    R = T[:, :3] @ T_ref[:, :3].T
    return float(np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))), float(np.linalg.norm(T[:, 3] - T_ref[:, 3]))
