// Connected components of an indexed triangle mesh on the device (include/poseprobe_hip.h, pp_cc_*): two vertices
// are connected when some triangle contains both.  labels[v] = the smallest vertex index of v's component, -1 for a vertex no
// triangle references.  Integers only; the only atomics are atomicMin (hook) and atomicAdd (counts).
//
// The labelling is the fixpoint of "hook to the smaller label, then shortcut", computed in ROUNDS of two launches on three label
// arrays: L (the caller's `labels`) and the two halves of `work`, P = half (round & 1) and Q = the other.  At the start of a
// round L == P on every referenced vertex.
//   k_cc_hook   one thread per triangle: reads the three labels from L (nobody writes L in this launch), m = their minimum, and
//               lowers P[label] to m with atomicMin for every label above m.  A minimum does not depend on the order of its
//               operands, so P after the launch is a pure function of L.
//   k_cc_jump   one thread per vertex: walks its own chain in P (nobody writes P in this launch) for at most CC_HOPS further
//               hops, writes the entry it reached to its OWN slots L[v] and Q[v], and raises the round's flag with a plain store
//               when that changed L[v].
// So every round is a pure function of the round before, whatever order the hardware retires lanes in: the labels AND the number
// of rounds are bit-reproducible.  Labels only decrease, stay inside their component and never pass below its smallest index.
// A round that changes nothing is the fixpoint: no jump moved, so every label is a root (P[l] == l); no hook moved, so a triangle
// with a label above its minimum m would have the root P[label] <= m < label - a contradiction; hence one label per component, and
// as labels[v] <= v it is the smallest index.
// No launch waits for another work-group: every thread does at most CC_HOPS + 1 dependent loads and ends.  The host decides
// convergence by reading the flags of a batch of rounds (poseprobe_amd/mesh.py).
//
// Memory: the hook reads a triangle's 12 bytes once (coalesced) and gathers three labels; marching cubes numbers the vertices in
// lattice order, so the labels a wavefront gathers sit in a few neighbouring rows of the lattice and come out of L2.  The jump
// reads and writes 4-byte entries in vertex order plus up to CC_HOPS + 1 gathers.
#include "pp_common.h"

namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_HOPS = 2;             // hops of a jump beyond the vertex's own entry: a chain's depth shrinks 3 x per round
constexpr int CC_MAX_ROUNDS = 1024;    // per call

size_t cc_half(int64_t nv) { return ((size_t)nv * 4 + 255) & ~(size_t)255; }

struct CcTri { int a, b, c; };
__device__ __forceinline__ CcTri cc_tri(const int32_t* __restrict__ triangles, int i) {
  const int32_t* t = triangles + (size_t)i * 3;
  return CcTri{t[0], t[1], t[2]};
}
__device__ __forceinline__ bool cc_inside(const CcTri& t, int nv) {
  return (unsigned)t.a < (unsigned)nv && (unsigned)t.b < (unsigned)nv && (unsigned)t.c < (unsigned)nv;
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_init_vertices(int nv, int32_t* __restrict__ L, int32_t* __restrict__ P,
                                                                 int32_t* __restrict__ Q) {
  const int v = blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= nv) return;
  L[v] = -1; P[v] = -1; Q[v] = -1;
}

// every writer of an entry writes the same value: plain stores.  A triangle with an index outside [0, nv) is skipped whole, here
// and in every other kernel (the Python host refuses such a mesh before it gets here).
__global__ __launch_bounds__(CC_THREADS) void k_cc_init_triangles(const int32_t* __restrict__ triangles, int nt, int nv,
                                                                  int32_t* __restrict__ L, int32_t* __restrict__ P,
                                                                  int32_t* __restrict__ Q) {
  const int i = blockIdx.x * CC_THREADS + threadIdx.x;
  if (i >= nt) return;
  const CcTri t = cc_tri(triangles, i);
  if (!cc_inside(t, nv)) return;
  L[t.a] = t.a; P[t.a] = t.a; Q[t.a] = t.a;
  L[t.b] = t.b; P[t.b] = t.b; Q[t.b] = t.b;
  L[t.c] = t.c; P[t.c] = t.c; Q[t.c] = t.c;
}

// The range tests on labels in hook and jump cannot fire on state pp_cc_rounds itself initialised; they keep a caller who hands
// first_round > 0 a foreign `labels` or `work` from indexing out of bounds.  A lane that takes one touches no label and RAISES the
// round's flag: such a run never reports a fixpoint, and the host's cap on the batches ends it with an error.
__global__ __launch_bounds__(CC_THREADS) void k_cc_hook(const int32_t* __restrict__ triangles, int nt, int nv,
                                                        const int32_t* __restrict__ L, int32_t* __restrict__ P,
                                                        int32_t* __restrict__ changed) {
  const int i = blockIdx.x * CC_THREADS + threadIdx.x;
  if (i >= nt) return;
  const CcTri t = cc_tri(triangles, i);
  if (!cc_inside(t, nv)) return;
  const int la = L[t.a], lb = L[t.b], lc = L[t.c];      // in [0, nv): referenced vertices carry a vertex index of their component
  const int m = min(la, min(lb, lc));
  if (m < 0 || max(la, max(lb, lc)) >= nv) { *changed = 1; return; }
  if (la > m) atomicMin(P + la, m);
  if (lb > m && lb != la) atomicMin(P + lb, m);
  if (lc > m && lc != la && lc != lb) atomicMin(P + lc, m);
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_jump(int nv, const int32_t* __restrict__ P, int32_t* __restrict__ L,
                                                        int32_t* __restrict__ Q, int32_t* __restrict__ changed) {
  const int v = blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= nv) return;
  int l = P[v];
  if (l < 0) return;                                    // unreferenced: -1 in all three arrays, for good
#pragma unroll
  for (int h = 0; h < CC_HOPS; ++h) {                   // (a root answers itself: no test for the end of the chain)
    if ((unsigned)l >= (unsigned)nv) { *changed = 1; return; }
    l = P[l];
  }
  if ((unsigned)l >= (unsigned)nv) { *changed = 1; return; }
  if (L[v] != l) {
    L[v] = l;
    *changed = 1;
  }
  Q[v] = l;
}

// counts by root: out[labels[key vertex]] += 1.  A thread takes CC_COUNT_ITEMS items a work-group's width apart (coalesced) and
// keeps the run of its current label in registers; a wavefront whose lanes all end on one label - the rule inside a large
// component, where every add would meet at ONE address - sums its runs by shuffles and adds once.
constexpr int CC_COUNT_ITEMS = 8;
template <bool TRI>
__global__ __launch_bounds__(CC_THREADS) void k_cc_count(const int32_t* __restrict__ labels, int nv,
                                                         const int32_t* __restrict__ triangles, int n, int32_t* __restrict__ out) {
  const long long base = (long long)blockIdx.x * (CC_THREADS * CC_COUNT_ITEMS) + threadIdx.x;
  int cur = -1, run = 0;
#pragma unroll
  for (int k = 0; k < CC_COUNT_ITEMS; ++k) {
    const long long i = base + k * CC_THREADS;
    int key = -1;
    if (i < n) {
      if (TRI) {
        const CcTri t = cc_tri(triangles, (int)i);
        if (cc_inside(t, nv)) key = labels[t.a];
      } else {
        key = labels[i];
      }
    }
    if (key < 0 || key >= nv) continue;
    if (key == cur) { ++run; continue; }
    if (run > 0) atomicAdd(out + cur, run);
    cur = key;
    run = 1;
  }
  // every lane arrives here (no early return above): the ballots and shuffles see the whole wavefront
  const bool live = run > 0;
  const unsigned long long lives = __ballot(live);
  if (lives == 0) return;                               // (wave-uniform)
  const int leader = __ffsll((long long)lives) - 1;
  const int first = __shfl(cur, leader, 64);
  if (__ballot(live && cur == first) == lives) {
    int sum = live ? run : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(out + first, sum);
  } else if (live) {
    atomicAdd(out + cur, run);
  }
}

// vkeep[v] = 1 iff v is referenced and its component's root is marked in root_keep; tkeep[i] likewise by the triangle's first vertex
__global__ __launch_bounds__(CC_THREADS) void k_cc_keep_masks(const int32_t* __restrict__ labels, int nv,
                                                              const int32_t* __restrict__ triangles, int nt,
                                                              const uint8_t* __restrict__ root_keep, int32_t* __restrict__ vkeep,
                                                              int32_t* __restrict__ tkeep) {
  const int i = blockIdx.x * CC_THREADS + threadIdx.x;
  if (i < nv) {
    const int l = labels[i];
    vkeep[i] = (l >= 0 && l < nv && root_keep[l]) ? 1 : 0;
  }
  if (i < nt) {
    const CcTri t = cc_tri(triangles, i);
    int keep = 0;
    if (cc_inside(t, nv)) {
      const int l = labels[t.a];
      keep = (l >= 0 && l < nv && root_keep[l]) ? 1 : 0;
    }
    tkeep[i] = keep;
  }
}

// vscan / tscan: INCLUSIVE prefix sums of the two masks.  A kept row's rank is its scan value - 1.
__global__ __launch_bounds__(CC_THREADS) void k_cc_compact(const float* __restrict__ vertices, const int32_t* __restrict__ triangles,
                                                           const int32_t* __restrict__ vscan, const int32_t* __restrict__ tscan,
                                                           int nv, int nt, float* __restrict__ out_vertices,
                                                           int32_t* __restrict__ out_index, int32_t* __restrict__ out_triangles,
                                                           int n_out_vertices, int n_out_triangles) {
  const int i = blockIdx.x * CC_THREADS + threadIdx.x;
  if (i < nv) {
    const int s = vscan[i], before = i > 0 ? vscan[i - 1] : 0;
    if (s == before + 1 && s >= 1 && s <= n_out_vertices) {
      const float* p = vertices + (size_t)i * 3;
      float* o = out_vertices + (size_t)(s - 1) * 3;
      o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
      out_index[s - 1] = i;
    }
  }
  if (i < nt) {
    const int s = tscan[i], before = i > 0 ? tscan[i - 1] : 0;
    if (s == before + 1 && s >= 1 && s <= n_out_triangles) {
      const CcTri t = cc_tri(triangles, i);
      if (cc_inside(t, nv)) {
        int32_t* o = out_triangles + (size_t)(s - 1) * 3;
        o[0] = vscan[t.a] - 1; o[1] = vscan[t.b] - 1; o[2] = vscan[t.c] - 1;
      }
    }
  }
}

int cc_check(const char* fn, int32_t nv, int32_t nt) {
  if (nv < 0 || nt < 0) { pp_set_error("%s: negative row count", fn); return PP_ERR_INVALID_ARG; }
  if (nv > (1 << 30) || nt > (1 << 29)) {
    pp_set_error("%s: at most 2^30 vertices and 2^29 triangles (32-bit element offsets)", fn);
    return PP_ERR_UNSUPPORTED;
  }
  return PP_OK;
}

}  // namespace

extern "C" int pp_cc_workspace(int32_t n_vertices, int64_t* bytes) {
  PP_REQUIRE(bytes, "null pointer");
  if (int rc = cc_check(__func__, n_vertices, 0)) return rc;
  *bytes = (int64_t)(2 * cc_half(n_vertices));
  return PP_OK;
}

extern "C" int pp_cc_rounds(const int32_t* triangles, int32_t n_triangles, int32_t n_vertices, int32_t first_round, int32_t n_rounds,
                            int32_t* labels, void* work, int64_t work_bytes, int32_t* changed, void* stream) {
  if (int rc = cc_check(__func__, n_vertices, n_triangles)) return rc;
  PP_REQUIRE(first_round >= 0 && n_rounds >= 1 && n_rounds <= CC_MAX_ROUNDS, "first_round >= 0 and 1 <= n_rounds <= 1024");
  PP_REQUIRE(first_round <= INT32_MAX - n_rounds, "round number overflow");
  PP_REQUIRE(changed, "null pointer");
  PP_REQUIRE(triangles || n_triangles == 0, "null triangles with a non-zero row count");
  PP_REQUIRE((labels && work) || n_vertices == 0, "null pointer");
  PP_REQUIRE(work_bytes >= (int64_t)(2 * cc_half(n_vertices)), "workspace too small (pp_cc_workspace)");
  PP_REQUIRE(n_vertices == 0 || reinterpret_cast<uintptr_t>(work) % 4 == 0, "workspace must be 4-byte aligned");
  hipStream_t st = pp_stream(stream);
  if (hipMemsetAsync(changed, 0, sizeof(int32_t) * (size_t)n_rounds, st) != hipSuccess) {
    pp_set_error("%s: hipMemsetAsync failed", __func__);
    return PP_ERR_LAUNCH;
  }
  if (n_vertices == 0) return PP_OK;
  int32_t* half[2] = {static_cast<int32_t*>(work),
                      reinterpret_cast<int32_t*>(static_cast<char*>(work) + cc_half(n_vertices))};
  const dim3 block(CC_THREADS), gv(pp_div_up(n_vertices, CC_THREADS)), gt(pp_div_up(n_triangles, CC_THREADS));
  if (first_round == 0) {
    hipLaunchKernelGGL(k_cc_init_vertices, gv, block, 0, st, n_vertices, labels, half[0], half[1]);
    if (n_triangles > 0)
      hipLaunchKernelGGL(k_cc_init_triangles, gt, block, 0, st, triangles, n_triangles, n_vertices, labels, half[0], half[1]);
  }
  if (n_triangles > 0) {                      // (no triangle: every label is -1 and no round can change that)
    for (int r = first_round; r < first_round + n_rounds; ++r) {
      int32_t* P = half[r & 1];
      int32_t* Q = half[(r & 1) ^ 1];
      hipLaunchKernelGGL(k_cc_hook, gt, block, 0, st, triangles, n_triangles, n_vertices, labels, P, changed + (r - first_round));
      hipLaunchKernelGGL(k_cc_jump, gv, block, 0, st, n_vertices, P, labels, Q, changed + (r - first_round));
    }
  }
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_cc_count(const int32_t* labels, int32_t n_vertices, const int32_t* triangles, int32_t n_triangles,
                           int32_t* vertex_counts, int32_t* triangle_counts, void* stream) {
  if (int rc = cc_check(__func__, n_vertices, n_triangles)) return rc;
  PP_REQUIRE(triangles || n_triangles == 0, "null triangles with a non-zero row count");
  if (n_vertices == 0) return PP_OK;
  PP_REQUIRE(labels && vertex_counts && triangle_counts, "null pointer");
  hipStream_t st = pp_stream(stream);
  if (hipMemsetAsync(vertex_counts, 0, sizeof(int32_t) * (size_t)n_vertices, st) != hipSuccess ||
      hipMemsetAsync(triangle_counts, 0, sizeof(int32_t) * (size_t)n_vertices, st) != hipSuccess) {
    pp_set_error("%s: hipMemsetAsync failed", __func__);
    return PP_ERR_LAUNCH;
  }
  const dim3 block(CC_THREADS);
  hipLaunchKernelGGL(k_cc_count<false>, dim3(pp_div_up(n_vertices, CC_THREADS * CC_COUNT_ITEMS)), block, 0, st, labels, n_vertices,
                     (const int32_t*)nullptr, n_vertices, vertex_counts);
  if (n_triangles > 0)
    hipLaunchKernelGGL(k_cc_count<true>, dim3(pp_div_up(n_triangles, CC_THREADS * CC_COUNT_ITEMS)), block, 0, st, labels, n_vertices, triangles,
                       n_triangles, triangle_counts);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_cc_keep_masks(const int32_t* labels, int32_t n_vertices, const int32_t* triangles, int32_t n_triangles,
                                const uint8_t* root_keep, int32_t* vertex_keep, int32_t* triangle_keep, void* stream) {
  if (int rc = cc_check(__func__, n_vertices, n_triangles)) return rc;
  PP_REQUIRE((triangles && triangle_keep) || n_triangles == 0, "null pointer with a non-zero triangle count");
  PP_REQUIRE((labels && root_keep && vertex_keep) || n_vertices == 0, "null pointer with a non-zero vertex count");
  const int n = n_vertices > n_triangles ? n_vertices : n_triangles;
  if (n == 0) return PP_OK;
  hipLaunchKernelGGL(k_cc_keep_masks, dim3(pp_div_up(n, CC_THREADS)), dim3(CC_THREADS), 0, pp_stream(stream), labels, n_vertices,
                     triangles, n_triangles, root_keep, vertex_keep, triangle_keep);
  PP_CHECK_LAUNCH();
  return PP_OK;
}

extern "C" int pp_cc_compact(const float* vertices, const int32_t* triangles, const int32_t* vertex_scan, const int32_t* triangle_scan,
                             int32_t n_vertices, int32_t n_triangles, float* out_vertices, int32_t* out_index, int32_t* out_triangles,
                             int32_t n_out_vertices, int32_t n_out_triangles, void* stream) {
  if (int rc = cc_check(__func__, n_vertices, n_triangles)) return rc;
  PP_REQUIRE(n_out_vertices >= 0 && n_out_vertices <= n_vertices && n_out_triangles >= 0 && n_out_triangles <= n_triangles,
             "kept row counts must lie in [0, rows]");
  PP_REQUIRE((vertices && vertex_scan) || n_vertices == 0, "null pointer with a non-zero vertex count");
  PP_REQUIRE((triangles && triangle_scan) || n_triangles == 0, "null pointer with a non-zero triangle count");
  PP_REQUIRE((out_vertices && out_index) || n_out_vertices == 0, "null output with a non-zero kept vertex count");
  PP_REQUIRE(out_triangles || n_out_triangles == 0, "null output with a non-zero kept triangle count");
  PP_REQUIRE(n_out_vertices > 0 || n_out_triangles == 0, "kept triangles need kept vertices");
  if (n_out_vertices == 0) return PP_OK;              // nothing kept: no launch
  const int n = n_vertices > n_triangles ? n_vertices : n_triangles;
  hipLaunchKernelGGL(k_cc_compact, dim3(pp_div_up(n, CC_THREADS)), dim3(CC_THREADS), 0, pp_stream(stream), vertices, triangles,
                     vertex_scan, triangle_scan, n_vertices, n_triangles, out_vertices, out_index, out_triangles, n_out_vertices,
                     n_out_triangles);
  PP_CHECK_LAUNCH();
  return PP_OK;
}
