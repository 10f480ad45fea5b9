// Marching cubes on a device-resident fp32 lattice u[X,Y,Z] (C order): an indexed mesh with shared vertices in lattice
// coordinates, in a canonical order and without atomics (include/poseprobe_hip.h, pp_mc_*; DESIGN.md "Mesh extraction").
//
//   corner below    <=>  u < threshold
//   edge active     <=>  exactly one endpoint below; owned by its lower endpoint p0 and its axis a
//   vertex id        =   rank of its edge among the active edges in the order 3 * linear(p0) + a
//   triangle order   =   cells in C order, then the row order of the case table (pp_mc_table.h)
//
// Every kernel walks the lattice by linear point index, 4 consecutive points (or the cells they are the low corner of) per
// thread and MC_TILE = 1024 per work-group, so that the ranks are a work-group base plus a scan inside the work-group:
//   k_mc_classify   3 edge bits + the cell's triangle count per point (one byte), the tile's two sums
//   k_mc_scan_tiles exclusive scan of the tile sums by one work-group (integers: any order gives the same bits), the totals
//   k_mc_vertices   vertex base per point (kept for the triangle pass) and the vertices
//   k_mc_triangles  case index from the 8 corners again, table rows from LDS, vertex ids from the owners' bases
// Streaming kernels: the field is read once per pass from HBM (the stencil's re-reads come out of the caches; the classify pass
// reads a thread's 20 values as four 128-bit and four 32-bit loads), one flag byte and one base per point, no scratch memory.
#include "pp_common.h"
#include "pp_mc_table.h"

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_PER_THREAD = 4;
constexpr int MC_TILE = MC_THREADS * MC_PER_THREAD;

const int8_t h_mc_table[256][16] = PP_MC_TABLE_INIT;
__constant__ int8_t d_mc_table[256][16] __attribute__((aligned(16))) = PP_MC_TABLE_INIT;
__constant__ uint8_t d_mc_ntri[256] = PP_MC_NTRI_INIT;

struct McDims {
  int X, Y, Z;
  int YZ;      // stride of x
  int N;       // points
};

struct McWork {            // carved out of the caller's workspace; flags and vbase are padded to whole tiles
  uint8_t* flags;          // [tiles * MC_TILE]  bits 0-2: active edge along x, y, z owned by the point; bits 3-5: triangles of its cell
  int32_t* vbase;          // [tiles * MC_TILE]  vertex id of the point's first active edge
  unsigned long long* tsum;  // [tiles]  low word: vertices, high word: triangles of the tile; after the scan, of the tiles before it
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
int64_t mc_tiles(int64_t n) { return (n + MC_TILE - 1) / MC_TILE; }
int64_t mc_work_bytes(int64_t n) {
  const int64_t t = mc_tiles(n);
  return (int64_t)(align256((size_t)t * MC_TILE) + align256((size_t)t * MC_TILE * 4) + align256((size_t)t * 8));
}
McWork mc_carve(void* work, int64_t n) {
  const int64_t t = mc_tiles(n);
  char* p = static_cast<char*>(work);
  McWork w;
  w.flags = reinterpret_cast<uint8_t*>(p); p += align256((size_t)t * MC_TILE);
  w.vbase = reinterpret_cast<int32_t*>(p); p += align256((size_t)t * MC_TILE * 4);
  w.tsum = reinterpret_cast<unsigned long long*>(p);
  return w;
}

// exclusive scan of one value per thread over the work-group (NT threads, a multiple of 64); total = the work-group's sum
template <int NT, typename T>
__device__ __forceinline__ T mc_block_scan(T v, T* lds /*[NT / 64]*/, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  __syncthreads();                    // lds may still be read from the previous call
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  T base = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) {
    const T s = lds[k];
    if (k < wave) base += s;
    total += s;
  }
  return base + incl - v;
}

__device__ __forceinline__ void mc_coords(const McDims& d, int i, int& x, int& y, int& z) {
  x = i / d.YZ;
  const int r = i - x * d.YZ;
  y = r / d.Z;
  z = r - y * d.Z;
}
__device__ __forceinline__ void mc_next(const McDims& d, int& x, int& y, int& z) {
  if (++z == d.Z) { z = 0; if (++y == d.Y) { y = 0; ++x; } }
}

// case index of the cell whose low corner is point i (corner c at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1))
__device__ __forceinline__ int mc_case(const float* __restrict__ u, const McDims& d, int i, float thr) {
  const float* p = u + i;
  int c = 0;
  c |= (p[0] < thr) << 0;
  c |= (p[d.YZ] < thr) << 1;
  c |= (p[d.Z] < thr) << 2;
  c |= (p[d.YZ + d.Z] < thr) << 3;
  c |= (p[1] < thr) << 4;
  c |= (p[d.YZ + 1] < thr) << 5;
  c |= (p[d.Z + 1] < thr) << 6;
  c |= (p[d.YZ + d.Z + 1] < thr) << 7;
  return c;
}

// 5 consecutive lattice values from an address that is only 4-byte aligned (one 128-bit and one 32-bit load)
struct __attribute__((packed, aligned(4))) McRow4 { float v[4]; };
__device__ __forceinline__ void mc_load5(const float* __restrict__ p, float (&r)[5]) {
  const McRow4 q = *reinterpret_cast<const McRow4*>(p);
  r[0] = q.v[0]; r[1] = q.v[1]; r[2] = q.v[2]; r[3] = q.v[3];
  r[4] = p[4];
}

// A thread's 4 points and the 4 cells above them read 4 runs of 5 consecutive values: u[i0 + dx YZ + dy Z + 0..4].  That is plain
// linear addressing, also where the 4 points run over the end of a row: a value that belongs to no neighbour of a point is
// masked by that point's hx / hy / hz.  Only the end of the lattice needs care: there the indices are clamped.
__global__ __launch_bounds__(MC_THREADS) void k_mc_classify(const float* __restrict__ u, McDims d, float thr, McWork w) {
  __shared__ unsigned lds[MC_THREADS / 64];
  const int i0 = blockIdx.x * MC_TILE + threadIdx.x * MC_PER_THREAD;
  unsigned packed = 0, sums = 0;          // sums: vertices | triangles << 16 (at most 3072 and 5120 per tile)
  if (i0 < d.N) {
    float r[2][2][5];
    if (i0 + d.YZ + d.Z + 4 < d.N) {
#pragma unroll
      for (int dx = 0; dx < 2; ++dx)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) mc_load5(u + i0 + dx * d.YZ + dy * d.Z, r[dx][dy]);
    } else {
#pragma unroll
      for (int dx = 0; dx < 2; ++dx)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
          for (int k = 0; k < 5; ++k) r[dx][dy][k] = u[min(i0 + dx * d.YZ + dy * d.Z + k, d.N - 1)];
    }
    unsigned below[2][2];                 // bit k: value k of the run is below
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        below[dx][dy] = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) below[dx][dy] |= (unsigned)(r[dx][dy][k] < thr) << k;
      }
    int x, y, z;
    mc_coords(d, i0, x, y, z);
#pragma unroll
    for (int k = 0; k < MC_PER_THREAD; ++k) {
      if (i0 + k < d.N) {
        const bool hx = x + 1 < d.X, hy = y + 1 < d.Y, hz = z + 1 < d.Z;
        const unsigned c0 = below[0][0] >> k & 1u, c1 = below[1][0] >> k & 1u, c2 = below[0][1] >> k & 1u,
                       c3 = below[1][1] >> k & 1u, c4 = below[0][0] >> (k + 1) & 1u, c5 = below[1][0] >> (k + 1) & 1u,
                       c6 = below[0][1] >> (k + 1) & 1u, c7 = below[1][1] >> (k + 1) & 1u;
        unsigned bits = 0;
        if (hx) bits |= (c0 ^ c1) << 0;
        if (hy) bits |= (c0 ^ c2) << 1;
        if (hz) bits |= (c0 ^ c4) << 2;
        unsigned nt = 0;
        if (hx && hy && hz) nt = d_mc_ntri[c0 | c1 << 1 | c2 << 2 | c3 << 3 | c4 << 4 | c5 << 5 | c6 << 6 | c7 << 7];
        packed |= (bits | nt << 3) << (8 * k);
        sums += __popc(bits) + (nt << 16);
        mc_next(d, x, y, z);
      }
    }
  }
  reinterpret_cast<unsigned*>(w.flags)[i0 / MC_PER_THREAD] = packed;      // padded to whole tiles: no tail case
  unsigned total;
  mc_block_scan<MC_THREADS>(sums, lds, total);
  if (threadIdx.x == 0) w.tsum[blockIdx.x] = (unsigned long long)(total & 0xFFFFu) | (unsigned long long)(total >> 16) << 32;
}

// one work-group: tsum[t] <- sum of tsum[0..t), counts <- the totals.  The vertex total stays below 2^31 (3 N < 2^31) and so
// never carries into the triangle word; the triangle total may pass 2^31 - 1 (5 N): reported as -1.
constexpr int MC_SCAN_THREADS = 1024;
__global__ __launch_bounds__(MC_SCAN_THREADS) void k_mc_scan_tiles(unsigned long long* __restrict__ tsum, int tiles,
                                                                   int32_t* __restrict__ counts) {
  __shared__ unsigned long long lds[MC_SCAN_THREADS / 64];
  unsigned long long carry = 0;
  for (int t0 = 0; t0 < tiles; t0 += MC_SCAN_THREADS * 4) {
    const int e0 = t0 + threadIdx.x * 4;
    unsigned long long v[4], mine = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[k] = e0 + k < tiles ? tsum[e0 + k] : 0ull;
      mine += v[k];
    }
    unsigned long long total;
    unsigned long long run = carry + mc_block_scan<MC_SCAN_THREADS>(mine, lds, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (e0 + k < tiles) tsum[e0 + k] = run;
      run += v[k];
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    const unsigned long long nt = carry >> 32;
    counts[0] = (int32_t)(carry & 0xFFFFFFFFull);
    counts[1] = nt > 0x7FFFFFFFull ? -1 : (int32_t)nt;
  }
}

__global__ __launch_bounds__(MC_THREADS) void k_mc_vertices(const float* __restrict__ u, McDims d, float thr, McWork w,
                                                            float* __restrict__ vertices, int n_vertices) {
  __shared__ unsigned lds[MC_THREADS / 64];
  const int i0 = blockIdx.x * MC_TILE + threadIdx.x * MC_PER_THREAD;
  const unsigned packed = reinterpret_cast<const unsigned*>(w.flags)[i0 / MC_PER_THREAD];
  unsigned n[MC_PER_THREAD], mine = 0;
#pragma unroll
  for (int k = 0; k < MC_PER_THREAD; ++k) {
    n[k] = __popc((packed >> (8 * k)) & 7u);
    mine += n[k];
  }
  unsigned total;
  int id = (int)(unsigned)(w.tsum[blockIdx.x] & 0xFFFFFFFFull) + (int)mc_block_scan<MC_THREADS>(mine, lds, total);
  int4 base;
  base.x = id; base.y = base.x + (int)n[0]; base.z = base.y + (int)n[1]; base.w = base.z + (int)n[2];
  reinterpret_cast<int4*>(w.vbase)[i0 / MC_PER_THREAD] = base;
  if (mine == 0 || i0 >= d.N) return;
  int x, y, z;
  mc_coords(d, i0, x, y, z);
#pragma unroll
  for (int k = 0; k < MC_PER_THREAD; ++k) {
    const int i = i0 + k;
    const unsigned bits = (packed >> (8 * k)) & 7u;
    if (bits) {                      // (bits are zero at and beyond N)
      const float u0 = u[i];
      const float c[3] = {(float)x, (float)y, (float)z};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (bits >> a & 1u) {
          const float u1 = u[i + (a == 0 ? d.YZ : a == 1 ? d.Z : 1)];
          const float t = pp_div(pp_sub(thr, u0), pp_sub(u1, u0));
          if (id < n_vertices) {
            float* v = vertices + (size_t)id * 3;
            v[0] = a == 0 ? pp_add(c[0], t) : c[0];
            v[1] = a == 1 ? pp_add(c[1], t) : c[1];
            v[2] = a == 2 ? pp_add(c[2], t) : c[2];
          }
          ++id;
        }
      }
    }
    mc_next(d, x, y, z);
  }
}

__global__ __launch_bounds__(MC_THREADS) void k_mc_triangles(const float* __restrict__ u, McDims d, float thr, McWork w,
                                                             int32_t* __restrict__ triangles, int n_triangles) {
  __shared__ unsigned lds[MC_THREADS / 64];
  __shared__ int8_t table[256][16] __attribute__((aligned(16)));
  reinterpret_cast<uint4*>(&table[0][0])[threadIdx.x] = reinterpret_cast<const uint4*>(&d_mc_table[0][0])[threadIdx.x];
  const int i0 = blockIdx.x * MC_TILE + threadIdx.x * MC_PER_THREAD;
  const unsigned packed = reinterpret_cast<const unsigned*>(w.flags)[i0 / MC_PER_THREAD];
  unsigned mine = 0;
#pragma unroll
  for (int k = 0; k < MC_PER_THREAD; ++k) mine += (packed >> (8 * k + 3)) & 7u;
  unsigned total;
  // (the scan's barriers also publish the table)
  long long tri = (long long)(w.tsum[blockIdx.x] >> 32) + mc_block_scan<MC_THREADS>(mine, lds, total);
  if (mine == 0) return;
#pragma unroll
  for (int k = 0; k < MC_PER_THREAD; ++k) {
    const int i = i0 + k;
    const int nt = (packed >> (8 * k + 3)) & 7u;
    if (nt == 0) continue;           // (a non-zero count implies a whole cell inside the lattice)
    const int8_t* row = table[mc_case(u, d, i, thr)];
    for (int t = 0; t < nt; ++t, ++tri) {
      int ids[3];
      bool whole = true;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int e = row[3 * t + c];
        whole = whole && e >= 0;     // holds whenever the field and the threshold are those pp_mc_count saw
        const int a = (e & 15) >> 2, lo = e & 1, hi = (e >> 1) & 1;
        const int owner = i + lo * (a == 0 ? d.Z : d.YZ) + hi * (a == 2 ? d.Z : 1);
        ids[c] = w.vbase[owner] + __popc(w.flags[owner] & ((1u << a) - 1u));
      }
      if (whole && tri < n_triangles) {
        int32_t* o = triangles + (size_t)tri * 3;
        o[0] = ids[0]; o[1] = ids[1]; o[2] = ids[2];
      }
    }
  }
}

// shared argument checks; fills the dims.  Runs before any GPU call.
int mc_check(const char* fn, int32_t X, int32_t Y, int32_t Z, McDims& d) {
  if (X < 2 || Y < 2 || Z < 2) { pp_set_error("%s: every lattice dimension must be at least 2 (got %d x %d x %d)", fn, X, Y, Z); return PP_ERR_INVALID_ARG; }
  const int64_t n = (int64_t)X * Y * Z;
  if (3 * n >= (1ll << 31)) {
    pp_set_error("%s: lattice %d x %d x %d too large: 3 X Y Z must stay below 2^31 (32-bit vertex ids)", fn, X, Y, Z);
    return PP_ERR_UNSUPPORTED;
  }
  d.X = X; d.Y = Y; d.Z = Z; d.YZ = Y * Z; d.N = (int)n;
  return PP_OK;
}

}  // namespace

extern "C" int pp_mc_table(int32_t* table_host) {
  int32_t* table = table_host;
  PP_REQUIRE(table, "null pointer");
  for (int c = 0; c < 256; ++c)
    for (int k = 0; k < 16; ++k) table[c * 16 + k] = h_mc_table[c][k];
  return PP_OK;
}

extern "C" int pp_mc_workspace(int32_t X, int32_t Y, int32_t Z, int64_t* bytes) {
  PP_REQUIRE(bytes, "null pointer");
  McDims d;
  if (int rc = mc_check(__func__, X, Y, Z, d)) return rc;
  *bytes = mc_work_bytes(d.N);
  return PP_OK;
}

extern "C" int pp_mc_count(const float* u, int32_t X, int32_t Y, int32_t Z, float threshold, void* work, int64_t work_bytes,
                           int32_t* counts, void* stream) {
  PP_REQUIRE(u && work && counts, "null pointer");
  McDims d;
  if (int rc = mc_check(__func__, X, Y, Z, d)) return rc;
  PP_REQUIRE(work_bytes >= mc_work_bytes(d.N), "workspace too small (pp_mc_workspace)");
  PP_REQUIRE(reinterpret_cast<uintptr_t>(work) % 16 == 0, "workspace must be 16-byte aligned");
  const McWork w = mc_carve(work, d.N);
  const int tiles = (int)mc_tiles(d.N);
  hipStream_t st = pp_stream(stream);
  hipLaunchKernelGGL(k_mc_classify, dim3(tiles), dim3(MC_THREADS), 0, st, u, d, threshold, w);
  hipLaunchKernelGGL(k_mc_scan_tiles, dim3(1), dim3(MC_SCAN_THREADS), 0, st, w.tsum, tiles, counts);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_mc_emit(const float* u, int32_t X, int32_t Y, int32_t Z, float threshold, void* work, int64_t work_bytes,
                          float* vertices, int32_t n_vertices, int32_t* triangles, int32_t n_triangles, void* stream) {
  PP_REQUIRE(u && work, "null pointer");
  PP_REQUIRE(n_vertices >= 0 && n_triangles >= 0, "negative row count");
  PP_REQUIRE((vertices || n_vertices == 0) && (triangles || n_triangles == 0), "null output with a non-zero row count");
  McDims d;
  if (int rc = mc_check(__func__, X, Y, Z, d)) return rc;
  PP_REQUIRE(work_bytes >= mc_work_bytes(d.N), "workspace too small (pp_mc_workspace)");
  PP_REQUIRE(reinterpret_cast<uintptr_t>(work) % 16 == 0, "workspace must be 16-byte aligned");
  if (n_vertices == 0 && n_triangles == 0) return PP_OK;
  const McWork w = mc_carve(work, d.N);
  const int tiles = (int)mc_tiles(d.N);
  hipStream_t st = pp_stream(stream);
  hipLaunchKernelGGL(k_mc_vertices, dim3(tiles), dim3(MC_THREADS), 0, st, u, d, threshold, w, vertices, n_vertices);
  if (n_triangles > 0)
    hipLaunchKernelGGL(k_mc_triangles, dim3(tiles), dim3(MC_THREADS), 0, st, u, d, threshold, w, triangles, n_triangles);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
