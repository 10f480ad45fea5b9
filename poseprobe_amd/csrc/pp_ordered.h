// Ordered gradient flushes of the object-branch train step (pp_ordered_attach, include/poseprobe_hip.h).
// A kernel that would end in float atomics on shared addresses instead writes its work-group's partial sums with plain stores
// into a slot of a caller-owned workspace (row = work-group, or ray), and a reduction launched behind it on the same stream adds
// the rows of every entry in a fixed order and adds the result to the gradient buffer, one writer per address: the same inputs
// give the same bits, whatever order the work-groups finish in (the pattern of k_nerf_part_finish, pp_nerf.hip).
// Rows that do no work: a persistent kernel retires surplus work-groups on the device (row count from `count`); the reduction
// derives the SAME active row count from `count` and never reads their slots.  Work-groups inside the active count always write
// their whole slot (zeros where they had no rows).
#pragma once
#include "pp_common.h"

// slot sizes in floats
#define ORD_WGRAD_SLOT (128 * 128 + 128)      // weight-gradient chain: a 128 x KX block in accumulator order | 128 bias sums at 128 * 128
#define ORD_WGRAD_BIAS (128 * 128)
#define ORD_WARP_THIN 1152                    // warp net, thin layers: W4[4][128] | W0[128][3] | b0[128] | b4[4]
#define ORD_WARP_THIN_N 1028
#define ORD_RGB_THIN 512                      // rgbnet, output layer: W3[3][128] | b3[3]
#define ORD_RGB_THIN_N 387
#define ORD_GEO_ROW 4                         // geometry backward: d alpha, d beta of a work-group (2 used)
#define ORD_GEO_THREADS 512                   // = GEO_BWD_THREADS (pp_geometry.hip)
#define ORD_RAY_ROW 16                        // ray backward: the 12 c2w contributions of a ray | its view index (int bits)

// offsets (floats) of the regions of the workspace: every producer has its own, so launches on different streams never share one
struct OrdLayout {
  int64_t wgrad[2];       // [0] warp net, [1] rgbnet: 2 * work_groups slots of ORD_WGRAD_SLOT
  int64_t thin[2];        // work_groups slots of ORD_WARP_THIN / ORD_RGB_THIN
  int64_t geo, ray, total;
};
static inline OrdLayout pp_ord_layout(int work_groups, int capacity, int n_rays) {
  const int64_t w = work_groups < 16 ? 16 : work_groups;      // the persistent kernels never run with fewer than 16
  OrdLayout L;
  int64_t o = 0;
  L.wgrad[0] = o; o += 2 * w * ORD_WGRAD_SLOT;
  L.wgrad[1] = o; o += 2 * w * ORD_WGRAD_SLOT;
  L.thin[0] = o; o += w * ORD_WARP_THIN;
  L.thin[1] = o; o += w * ORD_RGB_THIN;
  L.geo = o; o += (int64_t)pp_div_up(capacity, ORD_GEO_THREADS) * ORD_GEO_ROW;
  L.ray = o; o += (int64_t)n_rays * ORD_RAY_ROW;
  L.total = o;
  return L;
}

// destination of the entries of a slot: up to four contiguous runs; run s covers the slot's floats [end[s - 1], end[s]) (from 0
// for s = 0) and lands at dst + off[s]
struct OrdSegs {
  int n;
  int end[4];
  int off[4];
};
// dst[...] += sum over the active rows of part[row][0 .. segs.end[n - 1]), rows added in a fixed order.  Active rows:
// rows_max, or (count != nullptr) min(rows_max, ceil(min(count[0], cap) / per)).  stride: floats per row, a multiple of 4.
int pp_launch_ordered_flush(const float* part, int stride, int rows_max, const int32_t* count, int cap, int per, const OrdSegs& segs,
                            float* dst, hipStream_t st);

#ifdef __HIPCC__
#define ORD_RED_THREADS 1024
#define ORD_RED_GROUPS (ORD_RED_THREADS / 64)
// Sum of entry e4 (a float4) over rows [row0, row0 + rows) of `part` (row stride stride4 float4s) by a 1024-thread work-group
// that handles 64 consecutive entries: wavefront g adds rows g, g + 16, ... in ascending order, the sixteen partial sums are then
// added in ascending g by the threads of wavefront 0, for which the function returns true with the total in `out`.  The order
// depends on `rows` only.  `valid`: this thread's entry exists (all threads must call: the function has a barrier).
__device__ __forceinline__ bool pp_ordered_rows_sum(const float4* __restrict__ part, size_t stride4, int row0, int rows, int e4, bool valid,
                                                    float4* __restrict__ lds /*[16][64]*/, float4& out) {
  const int g = threadIdx.x >> 6, el = threadIdx.x & 63;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid) {
    const float4* __restrict__ p = part + (size_t)row0 * stride4 + e4;
    int r = g;
    // eight rows in flight (a loop of single loads pays the memory latency once per row), added in ascending order
    for (; r + 7 * ORD_RED_GROUPS < rows; r += 8 * ORD_RED_GROUPS) {
      float4 v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = p[(size_t)(r + i * ORD_RED_GROUPS) * stride4];
#pragma unroll
      for (int i = 0; i < 8; ++i) { s.x += v[i].x; s.y += v[i].y; s.z += v[i].z; s.w += v[i].w; }
    }
    float4 v[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) v[i] = r + i * ORD_RED_GROUPS < rows ? p[(size_t)(r + i * ORD_RED_GROUPS) * stride4] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 7; ++i)
      if (r + i * ORD_RED_GROUPS < rows) { s.x += v[i].x; s.y += v[i].y; s.z += v[i].z; s.w += v[i].w; }
  }
  lds[g * 64 + el] = s;
  __syncthreads();
  if (g != 0) return false;
  out = lds[el];
#pragma unroll
  for (int i = 1; i < ORD_RED_GROUPS; ++i) {
    const float4 v = lds[i * 64 + el];
    out.x += v.x; out.y += v.y; out.z += v.z; out.w += v.w;
  }
  return valid;
}
#endif
