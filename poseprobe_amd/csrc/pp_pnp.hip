// PnP-RANSAC on device-resident matches (include/poseprobe_hip.h, pp_pnp_*; DESIGN.md "Pose initialisation"): the first pose of
// a view that joins the incremental schedule, where the reference calls cv2.solvePnPRansac (lib/recon_scene.py:276-310).
//
//   hypothesis h   = samples[h][0..3]: a P3P solve on the first three rows, disambiguated by the fourth
//   score          = rows with valid, depth > 0 and squared reprojection error < reproj_error^2
//   winner         = largest score, ties to the lowest h; it needs min_inliers rows
//   result         = the winner's pose after refine_iters Gauss-Newton steps on its inliers, or the fallback pose
//
// fp32 in and out, fp64 inside: in fp64 the inlier counts do not depend on which closed-form P3P is used (tests/pnp_reference.py
// solves the same quartic with another root finder and on permuted points).  Three launches, no atomics, no host read; every sum
// runs in a fixed order, so the outputs are bit-reproducible:
//   k_pnp_hypotheses  one lane per hypothesis: pose (12 doubles) + validity flag
//   k_pnp_score       one work-group per hypothesis: waves stride over the rows, ballot + popcount, partial counts through LDS
//   k_pnp_finish      one work-group: argmax (LDS tree), the winner's mask, the Gauss-Newton loop, the outputs
// The work is latency bound (a few hundred solves, a few hundred thousand reprojections); nothing here is tuned for throughput.
//
// The arithmetic lives in host + device functions so that it can be exercised without a GPU.
#include "pp_common.h"

#include <math.h>

namespace {

constexpr int PNP_THREADS = 256;
constexpr int PNP_WAVES = PNP_THREADS / 64;
constexpr int PNP_HYP_THREADS = 64;         // one wave per work-group: a few hundred lanes spread over as many CUs as possible
constexpr int PNP_MAX_P = 1 << 22;
constexpr int PNP_MAX_H = 1 << 16;
constexpr int PNP_MAX_REFINE = 1000;
constexpr int PNP_ROOT_ITERS = 96;          // cap of the root iteration (it leaves earlier once every root stands still)
constexpr double PNP_REAL_TOL = 1e-6;       // a root counts as real iff |Im z| <= PNP_REAL_TOL * max(1, |z|)
constexpr int PNP_ACC = 27;                 // 21 entries of the upper triangle of J^T J + 6 of J^T r

#define PNP_HD __host__ __device__ inline

struct PnpCam { double fx, fy, cx, cy; };

struct PnpWork {           // carved out of the caller's workspace (layout documented in the public header)
  double* poses;           // [H][12] row-major [R | t] of each hypothesis
  int32_t* flags;          // [H] 1 = valid
  int32_t* counts;         // [H] inliers, -1 for an invalid hypothesis
};

size_t pnp_align256(size_t x) { return (x + 255) & ~(size_t)255; }
int64_t pnp_work_bytes(int64_t H) {
  return (int64_t)(pnp_align256((size_t)H * 12 * sizeof(double)) + 2 * pnp_align256((size_t)H * sizeof(int32_t)));
}
PnpWork pnp_carve(void* work, int64_t H) {
  char* p = static_cast<char*>(work);
  PnpWork w;
  w.poses = reinterpret_cast<double*>(p); p += pnp_align256((size_t)H * 12 * sizeof(double));
  w.flags = reinterpret_cast<int32_t*>(p); p += pnp_align256((size_t)H * sizeof(int32_t));
  w.counts = reinterpret_cast<int32_t*>(p);
  return w;
}

// ---- projection ---------------------------------------------------------------------------------------------------------------
// camera coordinates under T = [R | t] (row-major 3 x 4); depth = zc; e2 = squared pixel distance to (px, py)
PNP_HD void pnp_project(const double* T, const PnpCam& k, double X, double Y, double Z, double px, double py, double& depth,
                        double& e2) {
  const double xc = T[0] * X + T[1] * Y + T[2] * Z + T[3];
  const double yc = T[4] * X + T[5] * Y + T[6] * Z + T[7];
  const double zc = T[8] * X + T[9] * Y + T[10] * Z + T[11];
  const double du = k.fx * xc / zc + k.cx - px;
  const double dv = k.fy * yc / zc + k.cy - py;
  depth = zc;
  e2 = du * du + dv * dv;
}

// the scoring predicate (NaN anywhere makes it false)
PNP_HD bool pnp_inlier(const double* T, const PnpCam& k, const float* __restrict__ world, const float* __restrict__ pix,
                       const uint8_t* __restrict__ valid, int i, double thr2) {
  if (valid && !valid[i]) return false;
  double depth, e2;
  pnp_project(T, k, world[3 * i], world[3 * i + 1], world[3 * i + 2], pix[2 * i], pix[2 * i + 1], depth, e2);
  return depth > 0.0 && e2 < thr2;
}

// ---- quartic ------------------------------------------------------------------------------------------------------------------
// real roots of q[0] + q[1] x + ... + q[4] x^4 (q[4] != 0) by the Durand-Kerner iteration on all four complex roots at once;
// returns how many were written to out[4].  A double root shows up twice, which is harmless to the caller.
PNP_HD int pnp_quartic_real_roots(const double* q, double* out) {
  if (!(q[4] != 0.0)) return 0;
  double c[4];
  double rho = 0.0;
  for (int i = 0; i < 4; ++i) {
    c[i] = q[i] / q[4];
    if (!(fabs(c[i]) < 1e150)) return 0;               // (also refuses NaN)
  }
  // starting radius: the largest of |c3|, |c2|^(1/2), |c1|^(1/3), |c0|^(1/4) (every root lies within twice that)
  rho = fmax(fmax(fabs(c[3]), sqrt(fabs(c[2]))), fmax(cbrt(fabs(c[1])), sqrt(sqrt(fabs(c[0])))));
  if (rho == 0.0) { out[0] = 0.0; return 1; }
  double zr[4], zi[4];
  {
    double pr = rho, pi = 0.0;                          // rho (0.4 + 0.9 i)^k
    for (int k = 0; k < 4; ++k) {
      zr[k] = pr; zi[k] = pi;
      const double nr = pr * 0.4 - pi * 0.9, ni = pr * 0.9 + pi * 0.4;
      pr = nr; pi = ni;
    }
  }
  for (int it = 0; it < PNP_ROOT_ITERS; ++it) {
    bool still = true;
    for (int k = 0; k < 4; ++k) {
      // p(z_k), Horner on the monic polynomial
      double pr = zr[k] + c[3], pi = zi[k];
      for (int d = 2; d >= 0; --d) {
        const double nr = pr * zr[k] - pi * zi[k] + c[d], ni = pr * zi[k] + pi * zr[k];
        pr = nr; pi = ni;
      }
      double dr = 1.0, di = 0.0;                        // prod over j != k of (z_k - z_j)
      for (int j = 0; j < 4; ++j) {
        if (j == k) continue;
        const double ar = zr[k] - zr[j], ai = zi[k] - zi[j];
        const double nr = dr * ar - di * ai, ni = dr * ai + di * ar;
        dr = nr; di = ni;
      }
      const double dd = dr * dr + di * di;
      if (!(dd > 0.0)) {                                // two iterates coincide: move this one aside and go on
        zr[k] += 1e-8 * rho; zi[k] += 1e-8 * rho;
        still = false;
        continue;
      }
      const double er = (pr * dr + pi * di) / dd, ei = (pi * dr - pr * di) / dd;
      zr[k] -= er; zi[k] -= ei;
      if (!(er * er + ei * ei <= 1e-31 * (zr[k] * zr[k] + zi[k] * zi[k]))) still = false;
    }
    if (still) break;
  }
  int n = 0;
  for (int k = 0; k < 4; ++k) {
    const double m = sqrt(zr[k] * zr[k] + zi[k] * zi[k]);
    if (fabs(zi[k]) <= PNP_REAL_TOL * fmax(1.0, m)) out[n++] = zr[k];
  }
  return n;
}

// ---- P3P ----------------------------------------------------------------------------------------------------------------------
PNP_HD void pnp_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
PNP_HD double pnp_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// orthonormal frame of a triangle: rows e1 along A1 - A0, e3 along the normal, e2 = e3 x e1
PNP_HD void pnp_frame(const double* A0, const double* A1, const double* A2, double (*F)[3]) {
  double d1[3], d2[3], n[3];
  for (int i = 0; i < 3; ++i) { d1[i] = A1[i] - A0[i]; d2[i] = A2[i] - A0[i]; }
  const double l1 = sqrt(pnp_dot(d1, d1));
  for (int i = 0; i < 3; ++i) F[0][i] = d1[i] / l1;
  pnp_cross(F[0], d2, n);
  const double ln = sqrt(pnp_dot(n, n));
  for (int i = 0; i < 3; ++i) F[2][i] = n[i] / ln;
  pnp_cross(F[2], F[0], F[1]);
}

// residuals of the three cosine-law equations at the distances s[3]; returns their squared norm
PNP_HD double pnp_cosine_law(double ca, double cb, double cg, double a2, double b2, double c2, const double* s, double* f) {
  f[0] = s[1] * s[1] + s[2] * s[2] - 2.0 * s[1] * s[2] * ca - a2;
  f[1] = s[0] * s[0] + s[2] * s[2] - 2.0 * s[0] * s[2] * cb - b2;
  f[2] = s[0] * s[0] + s[1] * s[1] - 2.0 * s[0] * s[1] * cg - c2;
  return f[0] * f[0] + f[1] * f[1] + f[2] * f[2];
}

// up to three Newton steps on the cosine-law equations: the elimination behind the quartic loses digits where D(v) is small, the
// equations themselves do not.  A step is taken only while it lowers the residual, so a solution never gets worse.
PNP_HD void pnp_polish(double ca, double cb, double cg, double a2, double b2, double c2, double* s) {
  double f[3];
  double n = pnp_cosine_law(ca, cb, cg, a2, b2, c2, s, f);
  for (int it = 0; it < 3; ++it) {
    // Jacobian [[0, p, q], [r, 0, t], [u, w, 0]]
    const double p = 2.0 * s[1] - 2.0 * s[2] * ca, q = 2.0 * s[2] - 2.0 * s[1] * ca;
    const double r = 2.0 * s[0] - 2.0 * s[2] * cb, t = 2.0 * s[2] - 2.0 * s[0] * cb;
    const double u = 2.0 * s[0] - 2.0 * s[1] * cg, w = 2.0 * s[1] - 2.0 * s[0] * cg;
    const double det = p * t * u + q * r * w;
    if (!(fabs(det) > 0.0)) break;
    double z[3], g[3];
    z[0] = s[0] - (-f[0] * t * w + p * t * f[2] + q * w * f[1]) / det;
    z[1] = s[1] - (f[0] * t * u + q * r * f[2] - q * u * f[1]) / det;
    z[2] = s[2] - (-p * r * f[2] + p * u * f[1] + f[0] * r * w) / det;
    const double m = pnp_cosine_law(ca, cb, cg, a2, b2, c2, z, g);
    if (!(m < n)) break;
    for (int i = 0; i < 3; ++i) { s[i] = z[i]; f[i] = g[i]; }
    n = m;
  }
}

// Grunert's P3P: world points X[3], unit bearings j[3] -> up to 4 poses T[.][12] with X_cam = s_i j_i, s_i > 0.
// With s2 = u s1, s3 = v s1 the three cosine-law equations give u = N(v) / D(v) (N quadratic, D linear) and the quartic
// N^2 + D^2 (1 - W) - 2 cos(gamma) N D = 0, W = (c^2 / b^2) (1 + v^2 - 2 v cos(beta)); its coefficients are formed by polynomial
// products.  Exactly collinear triples (zero normal, which includes zero side lengths) have no solution here.
PNP_HD int pnp_p3p(const double (*X)[3], const double (*j)[3], double (*T)[12]) {
  double d01[3], d02[3], d12[3], nrm[3];
  for (int i = 0; i < 3; ++i) { d01[i] = X[1][i] - X[0][i]; d02[i] = X[2][i] - X[0][i]; d12[i] = X[2][i] - X[1][i]; }
  pnp_cross(d01, d02, nrm);
  if (!(pnp_dot(nrm, nrm) > 0.0)) return 0;
  const double a2 = pnp_dot(d12, d12), b2 = pnp_dot(d02, d02), c2 = pnp_dot(d01, d01);
  if (!(a2 > 0.0 && b2 > 0.0 && c2 > 0.0)) return 0;
  const double ca = pnp_dot(j[1], j[2]), cb = pnp_dot(j[0], j[2]), cg = pnp_dot(j[0], j[1]);
  const double q1 = (a2 - c2) / b2, kk = c2 / b2;
  const double n0 = 1.0 + q1, n1 = -2.0 * q1 * cb, n2 = q1 - 1.0;
  const double d0 = 2.0 * cg, d1 = -2.0 * ca;
  const double m0 = 1.0 - kk, m1 = 2.0 * kk * cb, m2 = -kk;
  const double D0 = d0 * d0, D1 = 2.0 * d0 * d1, D2 = d1 * d1;
  double q[5];
  q[0] = n0 * n0 + D0 * m0 - 2.0 * cg * (n0 * d0);
  q[1] = 2.0 * n0 * n1 + (D0 * m1 + D1 * m0) - 2.0 * cg * (n0 * d1 + n1 * d0);
  q[2] = (n1 * n1 + 2.0 * n0 * n2) + (D0 * m2 + D1 * m1 + D2 * m0) - 2.0 * cg * (n1 * d1 + n2 * d0);
  q[3] = 2.0 * n1 * n2 + (D1 * m2 + D2 * m1) - 2.0 * cg * (n2 * d1);
  q[4] = n2 * n2 + D2 * m2;
  double roots[4];
  const int nr = pnp_quartic_real_roots(q, roots);
  double Fw[3][3];
  pnp_frame(X[0], X[1], X[2], Fw);
  int n = 0;
  for (int r = 0; r < nr; ++r) {
    const double v = roots[r];
    if (!(v > 0.0)) continue;
    const double Dv = d0 + d1 * v;
    if (!(Dv != 0.0)) continue;
    const double u = (n0 + v * (n1 + v * n2)) / Dv;
    if (!(u > 0.0)) continue;
    const double den = 1.0 + v * v - 2.0 * v * cb;
    if (!(den > 0.0)) continue;
    double s[3];
    s[0] = sqrt(b2 / den); s[1] = u * s[0]; s[2] = v * s[0];
    pnp_polish(ca, cb, cg, a2, b2, c2, s);
    if (!(s[0] > 0.0 && s[1] > 0.0 && s[2] > 0.0)) continue;
    double C[3][3], Fc[3][3];
    for (int i = 0; i < 3; ++i) { C[0][i] = s[0] * j[0][i]; C[1][i] = s[1] * j[1][i]; C[2][i] = s[2] * j[2][i]; }
    pnp_frame(C[0], C[1], C[2], Fc);
    double* t = T[n];
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) t[4 * a + b] = Fc[0][a] * Fw[0][b] + Fc[1][a] * Fw[1][b] + Fc[2][a] * Fw[2][b];
      t[4 * a + 3] = C[0][a] - (t[4 * a] * X[0][0] + t[4 * a + 1] * X[0][1] + t[4 * a + 2] * X[0][2]);
    }
    ++n;
  }
  return n;
}

// one hypothesis: false = invalid.  Nothing is read before the four indices are known to be in range.
PNP_HD bool pnp_hypothesis(const float* __restrict__ world, const float* __restrict__ pix, const uint8_t* __restrict__ valid, int P,
                           const PnpCam& k, const int32_t* __restrict__ s, double* Tbest) {
  for (int a = 0; a < 4; ++a) {
    if (s[a] < 0 || s[a] >= P) return false;
    for (int b = 0; b < a; ++b)
      if (s[a] == s[b]) return false;
  }
  if (valid)
    for (int a = 0; a < 4; ++a)
      if (!valid[s[a]]) return false;
  double X[4][3], px[4][2], j[3][3];
  for (int a = 0; a < 4; ++a) {
    for (int i = 0; i < 3; ++i) X[a][i] = world[3 * s[a] + i];
    px[a][0] = pix[2 * s[a]]; px[a][1] = pix[2 * s[a] + 1];
  }
  for (int a = 0; a < 3; ++a) {
    const double x = (px[a][0] - k.cx) / k.fx, y = (px[a][1] - k.cy) / k.fy;
    const double l = sqrt(x * x + y * y + 1.0);
    j[a][0] = x / l; j[a][1] = y / l; j[a][2] = 1.0 / l;
  }
  double T[4][12];
  const int n = pnp_p3p(X, j, T);
  double best = INFINITY;
  bool found = false;
  for (int r = 0; r < n; ++r) {
    bool front = true;
    double e4 = 0.0;
    for (int a = 0; a < 4; ++a) {
      double depth, e2;
      pnp_project(T[r], k, X[a][0], X[a][1], X[a][2], px[a][0], px[a][1], depth, e2);
      front = front && depth > 0.0;
      e4 = e2;
    }
    if (front && e4 < best) {
      best = e4;
      found = true;
      for (int i = 0; i < 12; ++i) Tbest[i] = T[r][i];
    }
  }
  return found;
}

// ---- Gauss-Newton -------------------------------------------------------------------------------------------------------------
// one row's share of J^T J (upper triangle, row by row) and J^T r; increment delta = (omega, tau), X_cam' = X_cam + omega x X_cam + tau
PNP_HD void pnp_gn_row(const double* T, const PnpCam& k, double X, double Y, double Z, double px, double py, double* acc) {
  const double xc = T[0] * X + T[1] * Y + T[2] * Z + T[3];
  const double yc = T[4] * X + T[5] * Y + T[6] * Z + T[7];
  const double zc = T[8] * X + T[9] * Y + T[10] * Z + T[11];
  const double iz = 1.0 / zc;
  const double ru = k.fx * xc * iz + k.cx - px, rv = k.fy * yc * iz + k.cy - py;
  const double a0 = k.fx * iz, a2 = -k.fx * xc * iz * iz, b1 = k.fy * iz, b2 = -k.fy * yc * iz * iz;
  const double Ju[6] = {a2 * yc, a0 * zc - a2 * xc, -a0 * yc, a0, 0.0, a2};
  const double Jv[6] = {b2 * yc - b1 * zc, -b2 * xc, b1 * xc, 0.0, b1, b2};
  int e = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) acc[e++] += Ju[a] * Ju[b] + Jv[a] * Jv[b];
  for (int a = 0; a < 6; ++a) acc[21 + a] += Ju[a] * ru + Jv[a] * rv;
}

// solves (J^T J) delta = -J^T r by Cholesky and left-multiplies exp(delta) onto T; false (T untouched) on a non-positive pivot
PNP_HD bool pnp_gn_update(const double* acc, double* T) {
  double L[6][6];
  int e = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) L[b][a] = acc[e++];          // lower triangle of the symmetric matrix
  for (int c = 0; c < 6; ++c) {
    double p = L[c][c];
    for (int m = 0; m < c; ++m) p -= L[c][m] * L[c][m];
    if (!(p > 0.0)) return false;
    const double d = sqrt(p);
    L[c][c] = d;
    for (int r = c + 1; r < 6; ++r) {
      double s = L[r][c];
      for (int m = 0; m < c; ++m) s -= L[r][m] * L[c][m];
      L[r][c] = s / d;
    }
  }
  double y[6], x[6];
  for (int r = 0; r < 6; ++r) {
    double s = -acc[21 + r];
    for (int m = 0; m < r; ++m) s -= L[r][m] * y[m];
    y[r] = s / L[r][r];
  }
  for (int r = 5; r >= 0; --r) {
    double s = y[r];
    for (int m = r + 1; m < 6; ++m) s -= L[m][r] * x[m];
    x[r] = s / L[r][r];
  }
  for (int r = 0; r < 6; ++r)
    if (!(fabs(x[r]) < 1e150)) return false;                 // (a NaN or an overflow: keep the pose reached so far)
  // exp of (omega, tau): R = I + A W + B W^2, V = I + B W + C W^2, W = [omega]x, W^2 = omega omega^T - theta^2 I
  const double* w = x;
  const double* tau = x + 3;
  const double th2 = pnp_dot(w, w);
  double A, B, C;
  if (th2 < 1e-12) {
    A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; C = 1.0 / 6.0 - th2 / 120.0;
  } else {
    const double th = sqrt(th2);
    A = sin(th) / th; B = (1.0 - cos(th)) / th2; C = (1.0 - A) / th2;
  }
  const double W[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
  double R[3][3], V[3][3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double w2 = w[a] * w[b] - (a == b ? th2 : 0.0), id = a == b ? 1.0 : 0.0;
      R[a][b] = id + A * W[a][b] + B * w2;
      V[a][b] = id + B * W[a][b] + C * w2;
    }
  double out[12];
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 4; ++b) out[4 * a + b] = R[a][0] * T[b] + R[a][1] * T[4 + b] + R[a][2] * T[8 + b];
    out[4 * a + 3] += V[a][0] * tau[0] + V[a][1] * tau[1] + V[a][2] * tau[2];
  }
  for (int i = 0; i < 12; ++i) T[i] = out[i];
  return true;
}

PNP_HD PnpCam pnp_cam(const float* __restrict__ intr) {
  PnpCam k;
  k.fx = intr[0]; k.fy = intr[1]; k.cx = intr[2]; k.cy = intr[3];
  return k;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PNP_HYP_THREADS) void k_pnp_hypotheses(const float* __restrict__ world, const float* __restrict__ pix,
                                                                    const uint8_t* __restrict__ valid, int P,
                                                                    const float* __restrict__ intr,
                                                                    const int32_t* __restrict__ samples, int H, PnpWork w) {
  const int h = blockIdx.x * PNP_HYP_THREADS + threadIdx.x;
  if (h >= H) return;
  const PnpCam k = pnp_cam(intr);
  int32_t s[4];
  for (int a = 0; a < 4; ++a) s[a] = samples[4 * h + a];
  double T[12];
  for (int i = 0; i < 12; ++i) T[i] = 0.0;
  const bool ok = pnp_hypothesis(world, pix, valid, P, k, s, T);
  for (int i = 0; i < 12; ++i) w.poses[(size_t)h * 12 + i] = ok ? T[i] : 0.0;
  w.flags[h] = ok ? 1 : 0;
}

__global__ __launch_bounds__(PNP_THREADS) void k_pnp_score(const float* __restrict__ world, const float* __restrict__ pix,
                                                           const uint8_t* __restrict__ valid, int P, const float* __restrict__ intr,
                                                           double thr2, PnpWork w) {
  __shared__ int s_part[PNP_WAVES];
  const int h = blockIdx.x;
  if (!w.flags[h]) {                                          // (uniform over the work-group)
    if (threadIdx.x == 0) w.counts[h] = -1;
    return;
  }
  const PnpCam k = pnp_cam(intr);
  double T[12];
  for (int i = 0; i < 12; ++i) T[i] = w.poses[(size_t)h * 12 + i];
  int count = 0;                                              // the same in every lane of a wave
  for (int base = 0; base < P; base += PNP_THREADS) {
    const int i = base + threadIdx.x;
    const bool in = i < P && pnp_inlier(T, k, world, pix, valid, i, thr2);
    count += __popcll(__ballot(in));
  }
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int v = 0; v < PNP_WAVES; ++v) total += s_part[v];
    w.counts[h] = total;
  }
}

__global__ __launch_bounds__(PNP_THREADS) void k_pnp_finish(const float* __restrict__ world, const float* __restrict__ pix,
                                                            const uint8_t* __restrict__ valid, int P, const float* __restrict__ intr,
                                                            int H, double thr2, int refine_iters, int min_inliers,
                                                            const float* __restrict__ fallback, PnpWork w, float* __restrict__ w2c,
                                                            uint8_t* __restrict__ inliers, int32_t* __restrict__ info) {
  __shared__ int s_cnt[PNP_THREADS], s_idx[PNP_THREADS];
  __shared__ double s_T[12];
  __shared__ double s_part[PNP_WAVES][PNP_ACC];
  __shared__ double s_acc[PNP_ACC];
  __shared__ int s_go;
  const int tid = threadIdx.x;
  // winner: largest count, ties to the lowest index (a thread meets its indices in ascending order)
  int bc = -1, bi = 0x7fffffff;
  for (int h = tid; h < H; h += PNP_THREADS) {
    const int c = w.counts[h];
    if (c > bc) { bc = c; bi = h; }
  }
  s_cnt[tid] = bc; s_idx[tid] = bi;
  __syncthreads();
  for (int s = PNP_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const int c = s_cnt[tid + s], i = s_idx[tid + s];
      if (c > s_cnt[tid] || (c == s_cnt[tid] && i < s_idx[tid])) { s_cnt[tid] = c; s_idx[tid] = i; }
    }
    __syncthreads();
  }
  bc = s_cnt[0]; bi = s_idx[0];
  if (bc < min_inliers) {                                     // failure (uniform): the fallback pose, an empty mask
    for (int i = tid; i < P; i += PNP_THREADS) inliers[i] = 0;
    if (tid < 12) w2c[tid] = fallback[tid];
    if (tid == 0) { info[0] = 0; info[1] = -1; }
    return;
  }
  if (tid < 12) s_T[tid] = w.poses[(size_t)bi * 12 + tid];
  __syncthreads();
  const PnpCam k = pnp_cam(intr);
  double T[12];
  for (int i = 0; i < 12; ++i) T[i] = s_T[i];
  for (int i = tid; i < P; i += PNP_THREADS) inliers[i] = pnp_inlier(T, k, world, pix, valid, i, thr2) ? 1 : 0;
  // Gauss-Newton on the winner's inliers; each thread re-reads the mask bytes it wrote itself
  for (int it = 0; it < refine_iters; ++it) {
    double acc[PNP_ACC];
    for (int e = 0; e < PNP_ACC; ++e) acc[e] = 0.0;
    for (int i = tid; i < P; i += PNP_THREADS)
      if (inliers[i]) pnp_gn_row(T, k, world[3 * i], world[3 * i + 1], world[3 * i + 2], pix[2 * i], pix[2 * i + 1], acc);
    for (int e = 0; e < PNP_ACC; ++e) {
      double v = acc[e];
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if ((tid & 63) == 0) s_part[tid >> 6][e] = v;
    }
    __syncthreads();
    if (tid < PNP_ACC) {
      double v = s_part[0][tid];
      for (int q = 1; q < PNP_WAVES; ++q) v += s_part[q][tid];
      s_acc[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
      double Tn[12];
      for (int i = 0; i < 12; ++i) Tn[i] = s_T[i];
      const bool ok = pnp_gn_update(s_acc, Tn);
      for (int i = 0; i < 12; ++i) s_T[i] = Tn[i];
      s_go = ok ? 1 : 0;
    }
    __syncthreads();
    if (!s_go) break;                                         // (uniform)
    for (int i = 0; i < 12; ++i) T[i] = s_T[i];
  }
  if (tid < 12) w2c[tid] = (float)s_T[tid];
  if (tid == 0) { info[0] = bc; info[1] = bi; }
}

// shared argument checks; run before any GPU call
int pnp_check(const char* fn, int32_t P, int32_t H) {
  if (P < 4) { pp_set_error("%s: at least 4 rows are needed (got P = %d)", fn, P); return PP_ERR_INVALID_ARG; }
  if (H < 1) { pp_set_error("%s: at least 1 hypothesis is needed (got H = %d)", fn, H); return PP_ERR_INVALID_ARG; }
  if (P > PNP_MAX_P || H > PNP_MAX_H) {
    pp_set_error("%s: P = %d, H = %d beyond the limits P <= %d, H <= %d", fn, P, H, PNP_MAX_P, PNP_MAX_H);
    return PP_ERR_UNSUPPORTED;
  }
  return PP_OK;
}

}  // namespace

extern "C" int pp_pnp_workspace(int32_t P, int32_t H, int64_t* bytes) {
  PP_REQUIRE(bytes, "null pointer");
  if (int rc = pnp_check(__func__, P, H)) return rc;
  *bytes = pnp_work_bytes(H);
  return PP_OK;
}

extern "C" int pp_pnp_ransac(const float* world, const float* pix, const uint8_t* valid, int32_t P, const float* intr,
                             const int32_t* samples, int32_t H, float reproj_error, int32_t refine_iters, int32_t min_inliers,
                             const float* fallback, void* work, int64_t work_bytes, float* w2c, uint8_t* inliers, int32_t* info,
                             void* stream) {
  PP_REQUIRE(world && pix && intr && samples && fallback && work && w2c && inliers && info, "null pointer");
  if (int rc = pnp_check(__func__, P, H)) return rc;
  PP_REQUIRE(reproj_error > 0.0f && reproj_error < 1e18f, "reproj_error must be positive and finite");
  PP_REQUIRE(refine_iters >= 0 && refine_iters <= PNP_MAX_REFINE, "refine_iters must lie in [0, 1000]");
  PP_REQUIRE(min_inliers >= 1, "min_inliers must be at least 1");
  PP_REQUIRE(work_bytes >= pnp_work_bytes(H), "workspace too small (pp_pnp_workspace)");
  PP_REQUIRE(reinterpret_cast<uintptr_t>(work) % 16 == 0, "workspace must be 16-byte aligned");
  const PnpWork w = pnp_carve(work, H);
  const double thr2 = (double)reproj_error * (double)reproj_error;
  hipStream_t st = pp_stream(stream);
  hipLaunchKernelGGL(k_pnp_hypotheses, dim3(pp_div_up(H, PNP_HYP_THREADS)), dim3(PNP_HYP_THREADS), 0, st, world, pix, valid, P,
                     intr, samples, H, w);
  hipLaunchKernelGGL(k_pnp_score, dim3(H), dim3(PNP_THREADS), 0, st, world, pix, valid, P, intr, thr2, w);
  hipLaunchKernelGGL(k_pnp_finish, dim3(1), dim3(PNP_THREADS), 0, st, world, pix, valid, P, intr, H, thr2, refine_iters,
                     min_inliers, fallback, w, w2c, inliers, info);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
