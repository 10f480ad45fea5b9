// DTU mesh evaluation on device-resident points (include/poseprobe_hip.h, pp_dtu_*; DESIGN.md "Mesh evaluation"): the three hot
// stages of lib/dtu_eval.py::eval.
//
//   sampling   points from triangles, decided in fp64 with the reference's own operation order (count / scan / emit: the scan
//              is the caller's).  One wavefront per triangle; the rows i of a triangle go to the lanes, and the points of 64 rows
//              are dealt to the lanes by rank, so that a large triangle is written by all 64 lanes, coalesced.
//   cell grid  int64 key (x ny + y) nz + z of floor((p - origin) / edge), clamped into the grid.  The caller sorts the points by
//              key; the kernels find a run of cells that is contiguous along z by two binary searches in the sorted keys.
//   thinning   the lexicographically first maximal independent set of the radius graph, in rounds over a three-valued state
//              (double-buffered: a round reads only the previous round's values).
//   nearest    exact nearest point by fp32 squared distance, expanding rings of cells around the query's cell.
// fp32 distance everywhere: d2 = (dx dx + dy dy) + dz dz (the library is built with -ffp-contract=off).
#include "pp_common.h"

namespace {

constexpr int DTU_THREADS = 256;
constexpr double DTU_N_MAX = 2147483648.0;          // a per-axis count at or above this cannot be emitted: reported as 2^31 points
constexpr uint8_t ST_UNDECIDED = 0, ST_KEPT = 1, ST_REMOVED = 2;

struct DtuGrid {
  float o[3], edge;
  int n[3];
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// ---------------------------------------------------------------------------------------------------------------- sampling
struct DtuTri {
  double p0[3], v1[3], v2[3], n1, n2;
};

__device__ __forceinline__ double dtu_norm(const double* v) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

// lib/dtu_eval.py:70-81 for one triangle; false: it contributes no sampled point (an index out of range, no area, a count of 0)
__device__ __forceinline__ bool dtu_tri(const double* __restrict__ vtx, int V, const int32_t* __restrict__ tri, int t, double thresh,
                                        DtuTri& s) {
  const int a = tri[3 * (size_t)t], b = tri[3 * (size_t)t + 1], c = tri[3 * (size_t)t + 2];
  if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    s.p0[k] = vtx[3 * (size_t)a + k];
    s.v1[k] = vtx[3 * (size_t)b + k] - s.p0[k];
    s.v2[k] = vtx[3 * (size_t)c + k] - s.p0[k];
  }
  const double l1 = dtu_norm(s.v1), l2 = dtu_norm(s.v2);
  const double cr[3] = {s.v1[1] * s.v2[2] - s.v1[2] * s.v2[1], s.v1[2] * s.v2[0] - s.v1[0] * s.v2[2],
                        s.v1[0] * s.v2[1] - s.v1[1] * s.v2[0]};
  const double area2 = dtu_norm(cr);
  if (!(area2 > 0.0)) return false;
  const double thr = thresh * sqrt(l1 * l2 / area2);
  s.n1 = floor(l1 / thr);
  s.n2 = floor(l2 / thr);
  return s.n1 >= 1.0 && s.n2 >= 1.0;       // (also false for NaN; with a count of 0 the reference's 0.5 / 1e-7 keeps nothing)
}

__device__ __forceinline__ bool dtu_kept(double a, long long j, double n2) { return a + ((double)j + 0.5) / n2 < 1.0; }

// number of j in [0, n2] with a + (j + 0.5) / n2 < 1: the predicate is monotone in j, so an estimate is stepped to the boundary
__device__ __forceinline__ long long dtu_row_count(double a, double n2) {
  if (!dtu_kept(a, 0, n2)) return 0;
  const long long last = (long long)n2;
  long long j = (long long)floor((1.0 - a) * n2 - 0.5) + 1;
  j = j < 1 ? 1 : j > last + 1 ? last + 1 : j;
  while (j > 1 && !dtu_kept(a, j - 1, n2)) --j;
  while (j <= last && dtu_kept(a, j, n2)) ++j;
  return j;
}

__global__ __launch_bounds__(64) void k_dtu_sample_count(const double* __restrict__ vtx, int V, const int32_t* __restrict__ tri, int T,
                                                         double thresh, int64_t* __restrict__ counts) {
  const int t = blockIdx.x, lane = threadIdx.x;
  DtuTri s;
  long long n = 0;
  if (dtu_tri(vtx, V, tri, t, thresh, s)) {
    if (s.n1 >= DTU_N_MAX || s.n2 >= DTU_N_MAX) {
      n = lane == 0 ? (1ll << 31) : 0;
    } else {
      const long long rows = (long long)s.n1;
      for (long long i = lane; i <= rows; i += 64) {
        const long long c = dtu_row_count(((double)i + 0.5) / s.n1, s.n2);
        if (c == 0) break;                 // (monotone in i as well: no later row keeps a point)
        n += c;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if (lane == 0) counts[t] = n > (1ll << 31) ? (1ll << 31) : n;
}

__global__ __launch_bounds__(64) void k_dtu_sample_emit(const double* __restrict__ vtx, int V, const int32_t* __restrict__ tri, int T,
                                                        double thresh, const int64_t* __restrict__ offsets, float* __restrict__ points,
                                                        int64_t n_points) {
  __shared__ long long off[64];
  const int t = blockIdx.x, lane = threadIdx.x;
  DtuTri s;
  if (!dtu_tri(vtx, V, tri, t, thresh, s) || s.n1 >= DTU_N_MAX || s.n2 >= DTU_N_MAX) return;     // (uniform over the work-group)
  long long base = offsets[t];
  const long long rows = (long long)s.n1;
  for (long long i0 = 0; i0 <= rows; i0 += 64) {
    const long long i = i0 + lane;
    const long long c = i <= rows ? dtu_row_count(((double)i + 0.5) / s.n1, s.n2) : 0;
    long long incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    const long long total = __shfl(incl, 63, 64);
    if (total == 0) break;                 // (uniform; no later row keeps a point)
    __syncthreads();                       // the previous tile's readers are done
    off[lane] = incl - c;
    __syncthreads();
    for (long long r = lane; r < total; r += 64) {
      int L = 0;                           // the largest row of the tile whose first rank is <= r
#pragma unroll
      for (int step = 32; step > 0; step >>= 1)
        if (off[L + step] <= r) L += step;
      const long long j = r - off[L];
      const double a = ((double)(i0 + L) + 0.5) / s.n1, b = ((double)j + 0.5) / s.n2;
      const long long row = base + r;
      if (row < n_points) {
        float* q = points + 3 * (size_t)row;
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = (float)((s.v1[k] * a + s.v2[k] * b) + s.p0[k]);
      }
    }
    base += total;
  }
}

// ---------------------------------------------------------------------------------------------------------------- cell grid
// cell coordinate along one axis, clamped into [lo, hi] (a NaN coordinate lands on lo: every index stays in range)
__device__ __forceinline__ int dtu_cell(float p, float o, float edge, int lo, int hi) {
  const float c = floorf(pp_div(pp_sub(p, o), edge));
  return (int)fminf(fmaxf(c, (float)lo), (float)hi);
}
__device__ __forceinline__ long long dtu_key(const DtuGrid& g, int x, int y, int z) {
  return ((long long)x * g.n[1] + y) * g.n[2] + z;
}
// first position in the ascending keys[0, n) whose key is >= k
__device__ __forceinline__ int dtu_lower_bound(const int64_t* __restrict__ keys, int lo, int n, long long k) {
  int hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ float dtu_d2(const float* __restrict__ p, float qx, float qy, float qz) {
  const float dx = pp_sub(p[0], qx), dy = pp_sub(p[1], qy), dz = pp_sub(p[2], qz);
  return pp_add(pp_add(pp_mul(dx, dx), pp_mul(dy, dy)), pp_mul(dz, dz));
}

__global__ __launch_bounds__(DTU_THREADS) void k_dtu_cell_keys(const float* __restrict__ pts, int N, DtuGrid g, int64_t* __restrict__ keys) {
  const int s = blockIdx.x * DTU_THREADS + threadIdx.x;
  if (s >= N) return;
  const float* p = pts + 3 * (size_t)s;
  keys[s] = dtu_key(g, dtu_cell(p[0], g.o[0], g.edge, 0, g.n[0] - 1), dtu_cell(p[1], g.o[1], g.edge, 0, g.n[1] - 1),
                    dtu_cell(p[2], g.o[2], g.edge, 0, g.n[2] - 1));
}

// ---------------------------------------------------------------------------------------------------------------- thinning
// One round on the points in key order (pts, keys, order [N]: order = the point's index in the caller's order).  An undecided
// point is removed if a neighbour with a lower index is kept, kept if every such neighbour is removed, and waits otherwise.
// Neighbours lie in the 27 cells around the point's own: edge >= radius (the host adds a margin for the rounding of the cell
// coordinate).  A cell run along z is one range of the sorted keys.
__global__ __launch_bounds__(DTU_THREADS) void k_dtu_thin_round(const float* __restrict__ pts, const int64_t* __restrict__ keys,
                                                                const int32_t* __restrict__ order, int N, DtuGrid g, float r2,
                                                                const uint8_t* __restrict__ sin, uint8_t* __restrict__ sout,
                                                                int32_t* __restrict__ undecided) {
  const int s = blockIdx.x * DTU_THREADS + threadIdx.x;
  if (s >= N) return;
  const uint8_t st = sin[s];
  if (st != ST_UNDECIDED) { sout[s] = st; return; }
  const float qx = pts[3 * (size_t)s], qy = pts[3 * (size_t)s + 1], qz = pts[3 * (size_t)s + 2];
  const int mine = order[s];
  long long key = keys[s];                 // the cell the point was sorted into: decoded, not recomputed
  const int cz = (int)(key % g.n[2]); key /= g.n[2];
  const int cy = (int)(key % g.n[1]);
  const int cx = (int)(key / g.n[1]);
  const int z0 = max(cz - 1, 0), z1 = min(cz + 1, g.n[2] - 1);
  bool removed = false, wait = false;
  for (int x = max(cx - 1, 0); x <= min(cx + 1, g.n[0] - 1) && !removed; ++x)
    for (int y = max(cy - 1, 0); y <= min(cy + 1, g.n[1] - 1) && !removed; ++y) {
      const int lo = dtu_lower_bound(keys, 0, N, dtu_key(g, x, y, z0));
      const int hi = dtu_lower_bound(keys, lo, N, dtu_key(g, x, y, z1) + 1);
      for (int t = lo; t < hi; ++t) {
        if (order[t] >= mine) continue;    // (the point itself included)
        if (dtu_d2(pts + 3 * (size_t)t, qx, qy, qz) <= r2) {
          const uint8_t o = sin[t];
          if (o == ST_KEPT) { removed = true; break; }
          if (o == ST_UNDECIDED) wait = true;
        }
      }
    }
  const uint8_t res = removed ? ST_REMOVED : wait ? ST_UNDECIDED : ST_KEPT;
  sout[s] = res;
  if (res == ST_UNDECIDED) *undecided = 1;
}

// ---------------------------------------------------------------------------------------------------------------- nearest
// Rings of cells at Chebyshev distance k around the query's cell (clamped to one cell outside the grid: a query out there is
// no nearer to any cell than that one is).  Before ring k is visited every unvisited point lies at least k - 1 whole cells
// away along some axis: farther than lb = (k - 1.02) edge, where the 0.02 covers the rounding of the cell coordinates and of
// d2 (the host keeps the grid below 2^13 cells per axis, where that rounding stays below 2^-8 of a cell).  The search ends when
// the best d2 is at most lb^2 - no unvisited point can match it, so ties are decided among visited points, by index - or
// when lb reaches max_dist.
struct DtuBest {
  float d2;
  int idx;
};
__device__ __forceinline__ void dtu_scan_run(const float* __restrict__ pts, const int64_t* __restrict__ keys,
                                             const int32_t* __restrict__ order, int P, const DtuGrid& g, int x, int y, int z0, int z1,
                                             float qx, float qy, float qz, DtuBest& best) {
  z0 = max(z0, 0); z1 = min(z1, g.n[2] - 1);
  if (z0 > z1) return;
  const int lo = dtu_lower_bound(keys, 0, P, dtu_key(g, x, y, z0));
  if (lo >= P || keys[lo] > dtu_key(g, x, y, z1)) return;
  const int hi = dtu_lower_bound(keys, lo, P, dtu_key(g, x, y, z1) + 1);
  for (int t = lo; t < hi; ++t) {
    const float d2 = dtu_d2(pts + 3 * (size_t)t, qx, qy, qz);
    const int i = order[t];
    if (d2 < best.d2 || (d2 == best.d2 && i < best.idx)) { best.d2 = d2; best.idx = i; }
  }
}

__global__ __launch_bounds__(DTU_THREADS) void k_dtu_nearest(const float* __restrict__ queries, int Q, const float* __restrict__ pts,
                                                             const int64_t* __restrict__ keys, const int32_t* __restrict__ order,
                                                             int P, DtuGrid g, float max_dist, float* __restrict__ d2_out,
                                                             int32_t* __restrict__ idx_out) {
  const int q = blockIdx.x * DTU_THREADS + threadIdx.x;
  if (q >= Q) return;
  const float qx = queries[3 * (size_t)q], qy = queries[3 * (size_t)q + 1], qz = queries[3 * (size_t)q + 2];
  const int cx = dtu_cell(qx, g.o[0], g.edge, -1, g.n[0]), cy = dtu_cell(qy, g.o[1], g.edge, -1, g.n[1]),
            cz = dtu_cell(qz, g.o[2], g.edge, -1, g.n[2]);
  const int k_last = max(max(max(cx, g.n[0] - 1 - cx), max(cy, g.n[1] - 1 - cy)), max(cz, g.n[2] - 1 - cz));
  DtuBest best = {INFINITY, 0x7fffffff};
  for (int k = 0; k <= k_last; ++k) {
    if (k >= 2) {
      const float lb = pp_mul((float)k - 1.02f, g.edge);
      if (lb >= max_dist || best.d2 <= pp_mul(lb, lb)) break;
    }
    for (int x = max(cx - k, 0); x <= min(cx + k, g.n[0] - 1); ++x)
      for (int y = max(cy - k, 0); y <= min(cy + k, g.n[1] - 1); ++y) {
        if (x - cx == k || cx - x == k || y - cy == k || cy - y == k) {
          dtu_scan_run(pts, keys, order, P, g, x, y, cz - k, cz + k, qx, qy, qz, best);
        } else {                           // (k >= 1 here: the two end cells of the column)
          dtu_scan_run(pts, keys, order, P, g, x, y, cz - k, cz - k, qx, qy, qz, best);
          dtu_scan_run(pts, keys, order, P, g, x, y, cz + k, cz + k, qx, qy, qz, best);
        }
      }
  }
  const bool hit = best.d2 < pp_mul(max_dist, max_dist);
  d2_out[q] = hit ? best.d2 : INFINITY;
  idx_out[q] = hit ? best.idx : -1;
}

// shared argument checks of the grid description; runs before any GPU call
int dtu_grid(const char* fn, float ox, float oy, float oz, float edge, int32_t nx, int32_t ny, int32_t nz, DtuGrid& g) {
  if (!(ox - ox == 0.0f && oy - oy == 0.0f && oz - oz == 0.0f) || !(edge > 0.0f) || !(edge - edge == 0.0f)) {
    pp_set_error("%s: the grid origin must be finite and the cell edge positive and finite", fn);
    return PP_ERR_INVALID_ARG;
  }
  if (nx < 1 || ny < 1 || nz < 1) { pp_set_error("%s: every grid dimension must be at least 1 (got %d x %d x %d)", fn, nx, ny, nz); return PP_ERR_INVALID_ARG; }
  if (nx > (1 << 20) || ny > (1 << 20) || nz > (1 << 20)) {
    pp_set_error("%s: grid %d x %d x %d too large: at most 2^20 cells per axis (int64 cell keys)", fn, nx, ny, nz);
    return PP_ERR_UNSUPPORTED;
  }
  g.o[0] = ox; g.o[1] = oy; g.o[2] = oz; g.edge = edge; g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
  return PP_OK;
}

}  // namespace

extern "C" int pp_dtu_sample_count(const double* vertices, int32_t V, const int32_t* triangles, int32_t T, double thresh,
                                   int64_t* counts, void* stream) {
  PP_REQUIRE(vertices && triangles && counts, "null pointer");
  PP_REQUIRE(V >= 1 && T >= 1, "at least one vertex and one triangle");
  PP_REQUIRE(thresh > 0.0 && thresh - thresh == 0.0, "thresh must be positive and finite");
  hipLaunchKernelGGL(k_dtu_sample_count, dim3(T), dim3(64), 0, pp_stream(stream), vertices, V, triangles, T, thresh, counts);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_dtu_sample_emit(const double* vertices, int32_t V, const int32_t* triangles, int32_t T, double thresh,
                                  const int64_t* offsets, float* points, int64_t n_points, void* stream) {
  PP_REQUIRE(vertices && triangles && offsets, "null pointer");
  PP_REQUIRE(V >= 1 && T >= 1, "at least one vertex and one triangle");
  PP_REQUIRE(thresh > 0.0 && thresh - thresh == 0.0, "thresh must be positive and finite");
  PP_REQUIRE(n_points >= 0, "negative row count");
  PP_REQUIRE(points || n_points == 0, "null output with a non-zero row count");
  if (n_points > 0x7fffffffll) { pp_set_error("%s: more than 2^31 - 1 points", __func__); return PP_ERR_UNSUPPORTED; }
  if (n_points == 0) return PP_OK;
  hipLaunchKernelGGL(k_dtu_sample_emit, dim3(T), dim3(64), 0, pp_stream(stream), vertices, V, triangles, T, thresh, offsets, points,
                     n_points);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_dtu_cell_keys(const float* points, int32_t N, float ox, float oy, float oz, float edge, int32_t nx, int32_t ny,
                                int32_t nz, int64_t* keys, void* stream) {
  PP_REQUIRE(points && keys, "null pointer");
  PP_REQUIRE(N >= 1, "at least one point");
  DtuGrid g;
  if (int rc = dtu_grid(__func__, ox, oy, oz, edge, nx, ny, nz, g)) return rc;
  hipLaunchKernelGGL(k_dtu_cell_keys, dim3(pp_div_up(N, DTU_THREADS)), dim3(DTU_THREADS), 0, pp_stream(stream), points, N, g, keys);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_dtu_thin_workspace(int32_t N, int64_t* bytes) {
  PP_REQUIRE(bytes, "null pointer");
  PP_REQUIRE(N >= 1, "at least one point");
  *bytes = (int64_t)(2 * align256((size_t)N));
  return PP_OK;
}

extern "C" int pp_dtu_thin_rounds(const float* points, const int64_t* keys, const int32_t* order, int32_t N, float ox, float oy,
                                  float oz, float edge, int32_t nx, int32_t ny, int32_t nz, float radius, int32_t first_round,
                                  int32_t n_rounds, void* work, int64_t work_bytes, int32_t* undecided, void* stream) {
  PP_REQUIRE(points && keys && order && work && undecided, "null pointer");
  PP_REQUIRE(N >= 1, "at least one point");
  DtuGrid g;
  if (int rc = dtu_grid(__func__, ox, oy, oz, edge, nx, ny, nz, g)) return rc;
  PP_REQUIRE(radius >= 0.0f && radius - radius == 0.0f, "radius must be non-negative and finite");
  PP_REQUIRE(edge >= radius, "the cell edge must be at least the radius");
  PP_REQUIRE(first_round >= 0 && n_rounds >= 1 && n_rounds <= 1024, "first_round >= 0 and 1 <= n_rounds <= 1024");
  PP_REQUIRE(work_bytes >= (int64_t)(2 * align256((size_t)N)), "workspace too small (pp_dtu_thin_workspace)");
  hipStream_t st = pp_stream(stream);
  uint8_t* state[2] = {static_cast<uint8_t*>(work), static_cast<uint8_t*>(work) + align256((size_t)N)};
  if (first_round == 0 && hipMemsetAsync(state[0], ST_UNDECIDED, (size_t)N, st) != hipSuccess) {
    pp_set_error("%s: clearing the state failed", __func__);
    return PP_ERR_LAUNCH;
  }
  if (hipMemsetAsync(undecided, 0, sizeof(int32_t) * (size_t)n_rounds, st) != hipSuccess) {
    pp_set_error("%s: clearing the flags failed", __func__);
    return PP_ERR_LAUNCH;
  }
  const float r2 = radius * radius;
  for (int k = 0; k < n_rounds; ++k) {
    const int r = first_round + k;
    hipLaunchKernelGGL(k_dtu_thin_round, dim3(pp_div_up(N, DTU_THREADS)), dim3(DTU_THREADS), 0, st, points, keys, order, N, g, r2,
                       state[r & 1], state[(r + 1) & 1], undecided + k);
  }
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_dtu_nearest(const float* queries, int32_t Q, const float* points, const int64_t* keys, const int32_t* order,
                              int32_t P, float ox, float oy, float oz, float edge, int32_t nx, int32_t ny, int32_t nz, float max_dist,
                              float* d2, int32_t* idx, void* stream) {
  PP_REQUIRE(queries && points && keys && order && d2 && idx, "null pointer");
  PP_REQUIRE(Q >= 1 && P >= 1, "at least one query and one point");
  DtuGrid g;
  if (int rc = dtu_grid(__func__, ox, oy, oz, edge, nx, ny, nz, g)) return rc;
  PP_REQUIRE(max_dist > 0.0f && max_dist - max_dist == 0.0f, "max_dist must be positive and finite");
  hipLaunchKernelGGL(k_dtu_nearest, dim3(pp_div_up(Q, DTU_THREADS)), dim3(DTU_THREADS), 0, pp_stream(stream), queries, Q, points, keys,
                     order, P, g, max_dist, d2, idx);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
