// Signed distance of a triangle mesh at the nodes of a grid (include/poseprobe_hip.h, pp_msdf_*): the inverse of
// pp_mesh.hip's marching cubes.
//
//   binning    every triangle is registered in the cells its padded bounding box overlaps (count / scan / emit: the scan and the
//              sort of the (cell key, triangle) pairs are the caller's).  One wavefront per triangle, the cells dealt to the lanes.
//   nearest    exact nearest point of the mesh by fp32 squared distance, expanding rings of cells around the query's cell - the
//              scheme of pp_dtu_eval.hip with triangles in the place of points.  A run of cells along z is one range of the
//              sorted keys, found by two binary searches.
//   crossings  parity sign: per node column the crossings of the line along x with the mesh, counted into the slot between two
//              nodes.  One wavefront per triangle, the columns of its (y, z) bounding box dealt to the lanes; coverage in fp64.
// fp32 distance everywhere: d2 = (dx dx + dy dy) + dz dz (the library is built with -ffp-contract=off).  Integer atomics only.
#include "pp_common.h"

namespace {

constexpr int MSDF_THREADS = 256;

struct MsdfGrid {
  float o[3], edge;
  int n[3];
};

// ---------------------------------------------------------------------------------------------------------------- cell grid
// cell coordinate along one axis, clamped into [lo, hi] (a NaN coordinate lands on lo: every index stays in range)
__device__ __forceinline__ int msdf_cell(float p, float o, float edge, int lo, int hi) {
  const float c = floorf(pp_div(pp_sub(p, o), edge));
  return (int)fminf(fmaxf(c, (float)lo), (float)hi);
}
__device__ __forceinline__ long long msdf_key(const MsdfGrid& g, int x, int y, int z) {
  return ((long long)x * g.n[1] + y) * g.n[2] + z;
}
// first position in the ascending keys[0, n) whose key is >= k
__device__ __forceinline__ int msdf_lower_bound(const int64_t* __restrict__ keys, int lo, int n, long long k) {
  int hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct MsdfTri {
  float a[3], b[3], c[3];
};
// false: an index outside [0, V) - the triangle takes part in nothing
__device__ __forceinline__ bool msdf_load(const float* __restrict__ vtx, int V, const int32_t* __restrict__ tri, int t, MsdfTri& s) {
  const int ia = tri[3 * (size_t)t], ib = tri[3 * (size_t)t + 1], ic = tri[3 * (size_t)t + 2];
  if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    s.a[k] = vtx[3 * (size_t)ia + k];
    s.b[k] = vtx[3 * (size_t)ib + k];
    s.c[k] = vtx[3 * (size_t)ic + k];
  }
  return true;
}

// the cells [c0, c1] (per axis) of the triangle's bounding box padded by edge / 64: the padding is larger than the rounding of a
// cell coordinate (below 2^-8 of a cell), so the range covers every cell the triangle really touches
__device__ __forceinline__ bool msdf_cells(const float* __restrict__ vtx, int V, const int32_t* __restrict__ tri, int t, const MsdfGrid& g,
                                           int* c0, int* c1) {
  MsdfTri s;
  if (!msdf_load(vtx, V, tri, t, s)) return false;
  const float pad = pp_mul(g.edge, 0.015625f);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float lo = fminf(fminf(s.a[k], s.b[k]), s.c[k]), hi = fmaxf(fmaxf(s.a[k], s.b[k]), s.c[k]);
    c0[k] = msdf_cell(pp_sub(lo, pad), g.o[k], g.edge, 0, g.n[k] - 1);
    c1[k] = msdf_cell(pp_add(hi, pad), g.o[k], g.edge, 0, g.n[k] - 1);
    if (c1[k] < c0[k]) c1[k] = c0[k];          // (NaN coordinates: one cell)
  }
  return true;
}

__global__ __launch_bounds__(MSDF_THREADS) void k_msdf_bin_count(const float* __restrict__ vtx, int V, const int32_t* __restrict__ tri,
                                                                 int T, MsdfGrid g, int64_t* __restrict__ counts) {
  const int t = blockIdx.x * MSDF_THREADS + threadIdx.x;
  if (t >= T) return;
  int c0[3], c1[3];
  long long n = 0;
  if (msdf_cells(vtx, V, tri, t, g, c0, c1)) n = (long long)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
  counts[t] = n;
}

__global__ __launch_bounds__(64) void k_msdf_bin_emit(const float* __restrict__ vtx, int V, const int32_t* __restrict__ tri, int T,
                                                      MsdfGrid g, const int64_t* __restrict__ offsets, int64_t* __restrict__ keys,
                                                      int32_t* __restrict__ tris, int64_t n_pairs) {
  const int t = blockIdx.x, lane = threadIdx.x;
  int c0[3], c1[3];
  if (!msdf_cells(vtx, V, tri, t, g, c0, c1)) return;
  const long long ny = c1[1] - c0[1] + 1, nz = c1[2] - c0[2] + 1, n = (long long)(c1[0] - c0[0] + 1) * ny * nz;
  const long long base = offsets[t];
  for (long long i = lane; i < n; i += 64) {
    const long long row = base + i;
    if (row < 0 || row >= n_pairs) continue;   // (offsets that do not belong to these counts write nothing out of bounds)
    const int z = c0[2] + (int)(i % nz), y = c0[1] + (int)((i / nz) % ny), x = c0[0] + (int)(i / (nz * ny));
    keys[row] = msdf_key(g, x, y, z);
    tris[row] = t;
  }
}

// ---------------------------------------------------------------------------------------------------------------- nearest
__device__ __forceinline__ float msdf_dot(const float* u, const float* v) {
  return pp_add(pp_add(pp_mul(u[0], v[0]), pp_mul(u[1], v[1])), pp_mul(u[2], v[2]));
}
__device__ __forceinline__ void msdf_cross(const float* u, const float* v, float* w) {
  w[0] = pp_sub(pp_mul(u[1], v[2]), pp_mul(u[2], v[1]));
  w[1] = pp_sub(pp_mul(u[2], v[0]), pp_mul(u[0], v[2]));
  w[2] = pp_sub(pp_mul(u[0], v[1]), pp_mul(u[1], v[0]));
}
__device__ __forceinline__ float msdf_d2(const float* p, const float* q) {
  const float dx = pp_sub(p[0], q[0]), dy = pp_sub(p[1], q[1]), dz = pp_sub(p[2], q[2]);
  return pp_add(pp_add(pp_mul(dx, dx), pp_mul(dy, dy)), pp_mul(dz, dz));
}

struct MsdfBest {
  float d2, c[3];
  int tri;
};

// candidate closest point c of triangle t: kept if nearer, or as near with a lower triangle index
__device__ __forceinline__ void msdf_offer(const float* q, const float* c, int t, MsdfBest& best) {
  const float d2 = msdf_d2(q, c);
  if (d2 < best.d2 || (d2 == best.d2 && t < best.tri)) { best.d2 = d2; best.c[0] = c[0]; best.c[1] = c[1]; best.c[2] = c[2]; best.tri = t; }
}
// the closest point of the segment u + s (v - u), 0 <= s <= 1; a segment of no length is the point u
__device__ __forceinline__ void msdf_segment(const float* q, const float* u, const float* v, int t, MsdfBest& best) {
  const float e[3] = {pp_sub(v[0], u[0]), pp_sub(v[1], u[1]), pp_sub(v[2], u[2])};
  const float uq[3] = {pp_sub(q[0], u[0]), pp_sub(q[1], u[1]), pp_sub(q[2], u[2])};
  const float num = msdf_dot(uq, e), den = msdf_dot(e, e);
  float c[3] = {u[0], u[1], u[2]};
  if (num >= den && den > 0.0f) {
    c[0] = v[0]; c[1] = v[1]; c[2] = v[2];
  } else if (num > 0.0f && den > 0.0f) {
    const float s = pp_div(num, den);
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = pp_add(u[k], pp_mul(s, e[k]));
  }
  msdf_offer(q, c, t, best);
}
// Every candidate is a point of the triangle (up to rounding), so a wrong decision of the inside test near a side costs no more
// than the rounding that caused it: there the foot of the perpendicular and the side's closest point nearly coincide.
__device__ __forceinline__ void msdf_triangle(const float* q, const MsdfTri& s, int t, MsdfBest& best) {
  const float ab[3] = {pp_sub(s.b[0], s.a[0]), pp_sub(s.b[1], s.a[1]), pp_sub(s.b[2], s.a[2])};
  const float ac[3] = {pp_sub(s.c[0], s.a[0]), pp_sub(s.c[1], s.a[1]), pp_sub(s.c[2], s.a[2])};
  const float ap[3] = {pp_sub(q[0], s.a[0]), pp_sub(q[1], s.a[1]), pp_sub(q[2], s.a[2])};
  float n[3], w1[3], w2[3];
  msdf_cross(ab, ac, n);
  const float nn = msdf_dot(n, n);
  if (nn > 0.0f) {
    msdf_cross(ap, ac, w1);
    msdf_cross(ab, ap, w2);
    const float v = pp_div(msdf_dot(n, w1), nn), w = pp_div(msdf_dot(n, w2), nn);
    if (v >= 0.0f && w >= 0.0f && pp_add(v, w) <= 1.0f) {
      float c[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = pp_add(pp_add(s.a[k], pp_mul(v, ab[k])), pp_mul(w, ac[k]));
      msdf_offer(q, c, t, best);
    }
  }
  msdf_segment(q, s.a, s.b, t, best);
  msdf_segment(q, s.b, s.c, t, best);
  msdf_segment(q, s.c, s.a, t, best);
}

__device__ __forceinline__ void msdf_scan_run(const float* __restrict__ vtx, int V, const int32_t* __restrict__ tri,
                                              const int64_t* __restrict__ keys, const int32_t* __restrict__ tris, int P, const MsdfGrid& g,
                                              int x, int y, int z0, int z1, const float* q, MsdfBest& best) {
  z0 = max(z0, 0); z1 = min(z1, g.n[2] - 1);
  if (z0 > z1) return;
  const int lo = msdf_lower_bound(keys, 0, P, msdf_key(g, x, y, z0));
  if (lo >= P || keys[lo] > msdf_key(g, x, y, z1)) return;
  const int hi = msdf_lower_bound(keys, lo, P, msdf_key(g, x, y, z1) + 1);
  for (int r = lo; r < hi; ++r) {
    const int t = tris[r];
    MsdfTri s;
    if (msdf_load(vtx, V, tri, t, s)) msdf_triangle(q, s, t, best);
  }
}

// Rings of cells at Chebyshev distance k around the query's cell (clamped to one cell outside the grid: a query out there is no
// nearer to any cell than that one is).  A triangle not met in the rings below k is registered in none of their cells; its padded
// box covers every cell it touches, so it lies at least k - 1 whole cells away along some axis: farther than lb = (k - 1.02) edge,
// where the 0.02 covers the rounding of the query's cell coordinate and of d2 (the host keeps the grid below 2^13 cells per axis,
// where that rounding stays below 2^-8 of a cell).  The search ends when the best d2 is at most lb^2 - no triangle still to come
// can match it, so ties are decided among triangles already met, by index - or when lb reaches max_dist.
__global__ __launch_bounds__(MSDF_THREADS) void k_msdf_nearest(const float* __restrict__ queries, int Q, const float* __restrict__ xs,
                                                               const float* __restrict__ ys, const float* __restrict__ zs, int Y, int Z,
                                                               const float* __restrict__ vtx, int V, const int32_t* __restrict__ tri,
                                                               const int64_t* __restrict__ keys, const int32_t* __restrict__ tris, int P,
                                                               MsdfGrid g, float max_dist, float* __restrict__ dist,
                                                               float* __restrict__ closest, int32_t* __restrict__ tri_out,
                                                               int32_t* __restrict__ rings) {
  const int i = blockIdx.x * MSDF_THREADS + threadIdx.x;
  if (i >= Q) return;
  float q[3];
  if (queries) {
    q[0] = queries[3 * (size_t)i]; q[1] = queries[3 * (size_t)i + 1]; q[2] = queries[3 * (size_t)i + 2];
  } else {
    q[0] = xs[i / (Y * Z)]; q[1] = ys[(i / Z) % Y]; q[2] = zs[i % Z];
  }
  const int cx = msdf_cell(q[0], g.o[0], g.edge, -1, g.n[0]), cy = msdf_cell(q[1], g.o[1], g.edge, -1, g.n[1]),
            cz = msdf_cell(q[2], g.o[2], g.edge, -1, g.n[2]);
  const int k_last = max(max(max(cx, g.n[0] - 1 - cx), max(cy, g.n[1] - 1 - cy)), max(cz, g.n[2] - 1 - cz));
  MsdfBest best = {INFINITY, {0.0f, 0.0f, 0.0f}, 0x7fffffff};
  int k = 0;
  for (; k <= k_last; ++k) {
    if (k >= 2) {
      const float lb = pp_mul((float)k - 1.02f, g.edge);
      if (lb >= max_dist || best.d2 <= pp_mul(lb, lb)) break;
    }
    for (int x = max(cx - k, 0); x <= min(cx + k, g.n[0] - 1); ++x)
      for (int y = max(cy - k, 0); y <= min(cy + k, g.n[1] - 1); ++y) {
        if (x - cx == k || cx - x == k || y - cy == k || cy - y == k) {
          msdf_scan_run(vtx, V, tri, keys, tris, P, g, x, y, cz - k, cz + k, q, best);
        } else {                           // (k >= 1 here: the two end cells of the column)
          msdf_scan_run(vtx, V, tri, keys, tris, P, g, x, y, cz - k, cz - k, q, best);
          msdf_scan_run(vtx, V, tri, keys, tris, P, g, x, y, cz + k, cz + k, q, best);
        }
      }
  }
  const bool hit = best.d2 < pp_mul(max_dist, max_dist);
  const float nan = __int_as_float(0x7fc00000);
  dist[i] = hit ? sqrtf(best.d2) : INFINITY;
  closest[3 * (size_t)i] = hit ? best.c[0] : nan;
  closest[3 * (size_t)i + 1] = hit ? best.c[1] : nan;
  closest[3 * (size_t)i + 2] = hit ? best.c[2] : nan;
  tri_out[i] = hit ? best.tri : -1;
  if (rings) rings[i] = k;
}

// ---------------------------------------------------------------------------------------------------------------- crossings
// number of entries of the ascending a[0, n) that are < v (v NaN: 0)
__device__ __forceinline__ int msdf_count_below(const float* __restrict__ a, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((double)a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Edge function of the directed edge u -> v at the column p, all in the (y, z) plane: positive to the left of the edge.  It is
// evaluated from the lexicographically smaller end point and negated for the other direction, so that the two triangles of an
// edge get the same number with opposite signs.  The differences of fp32 coordinates and their products are exact in fp64 unless
// the coordinates differ by more than 29 binary orders of magnitude, and the sign of the last subtraction is then exact too.
__device__ __forceinline__ double msdf_edge(const double* u, const double* v, const double* p) {
  const bool fwd = u[0] < v[0] || (u[0] == v[0] && u[1] <= v[1]);
  const double* lo = fwd ? u : v;
  const double* hi = fwd ? v : u;
  const double e = (hi[0] - lo[0]) * (p[1] - lo[1]) - (hi[1] - lo[1]) * (p[0] - lo[0]);
  return fwd ? e : -e;
}
// Weight of the vertex opposite the edge u -> v (sign: +1 or -1, which turns the triangle's interior to the positive side), or a
// negative number when the column is not the triangle's.  On the edge itself the column is the triangle's iff the shifted
// column p + (eps, eps^2) is: the edge function changes by dy eps^2 - dz eps there, (dy, dz) = the edge's direction with the interior
// on its positive side.
__device__ __forceinline__ double msdf_weight(const double* u, const double* v, const double* p, double sign) {
  const double e = sign * msdf_edge(u, v, p);
  if (e != 0.0) return e;
  const double dy = sign * (v[0] - u[0]), dz = sign * (v[1] - u[1]);
  return (dz < 0.0 || (dz == 0.0 && dy > 0.0)) ? 0.0 : -1.0;
}

__global__ __launch_bounds__(64) void k_msdf_crossings(const float* __restrict__ vtx, int V, const int32_t* __restrict__ tri, int T,
                                                       const float* __restrict__ xs, const float* __restrict__ ys,
                                                       const float* __restrict__ zs, int X, int Y, int Z, int32_t* __restrict__ counts) {
  const int t = blockIdx.x, lane = threadIdx.x;
  MsdfTri s;
  if (!msdf_load(vtx, V, tri, t, s)) return;           // (uniform over the work-group)
  const double a[2] = {s.a[1], s.a[2]}, b[2] = {s.b[1], s.b[2]}, c[2] = {s.c[1], s.c[2]};
  const double area = msdf_edge(a, b, c);
  if (!(area > 0.0 || area < 0.0)) return;             // no projected area (or NaN): no crossing
  const double sign = area > 0.0 ? 1.0 : -1.0;
  // columns inside the bounding box: first node >= the minimum, nodes <= the maximum
  const double y_lo = fmin(fmin(a[0], b[0]), c[0]), y_hi = fmax(fmax(a[0], b[0]), c[0]);
  const double z_lo = fmin(fmin(a[1], b[1]), c[1]), z_hi = fmax(fmax(a[1], b[1]), c[1]);
  const int j0 = msdf_count_below(ys, Y, y_lo), k0 = msdf_count_below(zs, Z, z_lo);
  int j1 = j0, k1 = k0;                                // one past the last
  while (j1 < Y && (double)ys[j1] <= y_hi) ++j1;
  while (k1 < Z && (double)zs[k1] <= z_hi) ++k1;
  const int nk = k1 - k0;
  const long long n = (long long)(j1 - j0) * nk;
  for (long long i = lane; i < n; i += 64) {
    const int j = j0 + (int)(i / nk), k = k0 + (int)(i % nk);
    const double p[2] = {ys[j], zs[k]};
    const double wa = msdf_weight(b, c, p, sign), wb = msdf_weight(c, a, p, sign), wc = msdf_weight(a, b, p, sign);
    if (wa < 0.0 || wb < 0.0 || wc < 0.0) continue;
    const double x = ((wa * s.a[0] + wb * s.b[0]) + wc * s.c[0]) / ((wa + wb) + wc);
    const int slot = msdf_count_below(xs, X, x);       // in [0, X]
    atomicAdd(&counts[((size_t)slot * Y + j) * Z + k], 1);
  }
}

// shared argument checks of the cell grid; runs before any GPU call
int msdf_grid(const char* fn, float ox, float oy, float oz, float edge, int32_t nx, int32_t ny, int32_t nz, MsdfGrid& g) {
  if (!(ox - ox == 0.0f && oy - oy == 0.0f && oz - oz == 0.0f) || !(edge > 0.0f) || !(edge - edge == 0.0f)) {
    pp_set_error("%s: the grid origin must be finite and the cell edge positive and finite", fn);
    return PP_ERR_INVALID_ARG;
  }
  if (nx < 1 || ny < 1 || nz < 1) { pp_set_error("%s: every grid dimension must be at least 1 (got %d x %d x %d)", fn, nx, ny, nz); return PP_ERR_INVALID_ARG; }
  if (nx > (1 << 13) || ny > (1 << 13) || nz > (1 << 13)) {
    pp_set_error("%s: grid %d x %d x %d too large: at most 2^13 cells per axis (the ring bound's rounding margin)", fn, nx, ny, nz);
    return PP_ERR_UNSUPPORTED;
  }
  g.o[0] = ox; g.o[1] = oy; g.o[2] = oz; g.edge = edge; g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
  return PP_OK;
}

int msdf_nodes(const char* fn, int32_t X, int32_t Y, int32_t Z, int64_t extra_x) {
  if (X < 1 || Y < 1 || Z < 1) { pp_set_error("%s: every node count must be at least 1 (got %d x %d x %d)", fn, X, Y, Z); return PP_ERR_INVALID_ARG; }
  if (((int64_t)X + extra_x) * Y > 0x7fffffffll || ((int64_t)X + extra_x) * Y * Z > 0x7fffffffll) {
    pp_set_error("%s: %d x %d x %d nodes: more than 2^31 - 1", fn, X, Y, Z);
    return PP_ERR_UNSUPPORTED;
  }
  return PP_OK;
}

}  // namespace

extern "C" int pp_msdf_bin_count(const float* vertices, int32_t V, const int32_t* triangles, int32_t T, float ox, float oy, float oz,
                                 float edge, int32_t nx, int32_t ny, int32_t nz, int64_t* counts, void* stream) {
  PP_REQUIRE(vertices && triangles && counts, "null pointer");
  PP_REQUIRE(V >= 1 && T >= 1, "at least one vertex and one triangle");
  MsdfGrid g;
  if (int rc = msdf_grid(__func__, ox, oy, oz, edge, nx, ny, nz, g)) return rc;
  hipLaunchKernelGGL(k_msdf_bin_count, dim3(pp_div_up(T, MSDF_THREADS)), dim3(MSDF_THREADS), 0, pp_stream(stream), vertices, V, triangles,
                     T, g, counts);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_msdf_bin_emit(const float* vertices, int32_t V, const int32_t* triangles, int32_t T, float ox, float oy, float oz,
                                float edge, int32_t nx, int32_t ny, int32_t nz, const int64_t* offsets, int64_t* keys, int32_t* tris,
                                int64_t n_pairs, void* stream) {
  PP_REQUIRE(vertices && triangles && offsets, "null pointer");
  PP_REQUIRE(V >= 1 && T >= 1, "at least one vertex and one triangle");
  MsdfGrid g;
  if (int rc = msdf_grid(__func__, ox, oy, oz, edge, nx, ny, nz, g)) return rc;
  PP_REQUIRE(n_pairs >= 0, "negative pair count");
  PP_REQUIRE((keys && tris) || n_pairs == 0, "null output with a non-zero pair count");
  if (n_pairs > 0x7fffffffll) { pp_set_error("%s: more than 2^31 - 1 (cell, triangle) pairs", __func__); return PP_ERR_UNSUPPORTED; }
  if (n_pairs == 0) return PP_OK;
  hipLaunchKernelGGL(k_msdf_bin_emit, dim3(T), dim3(64), 0, pp_stream(stream), vertices, V, triangles, T, g, offsets, keys, tris, n_pairs);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_msdf_nearest(const float* queries, int32_t Q, const float* xs, const float* ys, const float* zs, int32_t X, int32_t Y,
                               int32_t Z, const float* vertices, int32_t V, const int32_t* triangles, int32_t T, const int64_t* keys,
                               const int32_t* tris, int32_t n_pairs, float ox, float oy, float oz, float edge, int32_t nx, int32_t ny,
                               int32_t nz, float max_dist, float* dist, float* closest, int32_t* tri, int32_t* rings, void* stream) {
  PP_REQUIRE(vertices && triangles && keys && tris && dist && closest && tri, "null pointer");
  PP_REQUIRE(Q >= 1 && V >= 1 && T >= 1 && n_pairs >= 1, "at least one query, one vertex, one triangle and one pair");
  MsdfGrid g;
  if (int rc = msdf_grid(__func__, ox, oy, oz, edge, nx, ny, nz, g)) return rc;
  PP_REQUIRE(max_dist > 0.0f, "max_dist must be positive (inf: no cap)");
  if (!queries) {
    PP_REQUIRE(xs && ys && zs, "null pointer: without queries the node coordinates are needed");
    if (int rc = msdf_nodes(__func__, X, Y, Z, 0)) return rc;
    PP_REQUIRE((int64_t)X * Y * Z == (int64_t)Q, "without queries Q must be X Y Z");
  }
  hipLaunchKernelGGL(k_msdf_nearest, dim3(pp_div_up(Q, MSDF_THREADS)), dim3(MSDF_THREADS), 0, pp_stream(stream), queries, Q, xs, ys, zs, Y,
                     Z, vertices, V, triangles, keys, tris, n_pairs, g, max_dist, dist, closest, tri, rings);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_msdf_crossing_slots(int32_t X, int32_t Y, int32_t Z, int64_t* slots) {
  PP_REQUIRE(slots, "null pointer");
  if (int rc = msdf_nodes(__func__, X, Y, Z, 1)) return rc;
  *slots = ((int64_t)X + 1) * Y * Z;
  return PP_OK;
}

extern "C" int pp_msdf_crossings(const float* vertices, int32_t V, const int32_t* triangles, int32_t T, const float* xs, const float* ys,
                                 const float* zs, int32_t X, int32_t Y, int32_t Z, int32_t* counts, void* stream) {
  PP_REQUIRE(vertices && triangles && xs && ys && zs && counts, "null pointer");
  PP_REQUIRE(V >= 1 && T >= 1, "at least one vertex and one triangle");
  if (int rc = msdf_nodes(__func__, X, Y, Z, 1)) return rc;
  hipStream_t st = pp_stream(stream);
  if (hipMemsetAsync(counts, 0, sizeof(int32_t) * ((size_t)X + 1) * Y * Z, st) != hipSuccess) {
    pp_set_error("%s: clearing the counts failed", __func__);
    return PP_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(k_msdf_crossings, dim3(T), dim3(64), 0, st, vertices, V, triangles, T, xs, ys, zs, X, Y, Z, counts);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
