// Ordered gradient flushes: the workspace query, its record in a pp_context and the generic row reduction (pp_ordered.h).
#include "pp_ordered.h"

__global__ __launch_bounds__(ORD_RED_THREADS) void k_ordered_flush(const float* __restrict__ part, int stride, int rows_max,
                                                                   const int32_t* __restrict__ count, int cap, int per, OrdSegs segs,
                                                                   float* __restrict__ dst) {
  __shared__ float4 lds[ORD_RED_GROUPS * 64];
  const int n = segs.end[segs.n - 1];
  int rows = rows_max;
  if (count) rows = min(rows_max, (min(count[0], cap) + per - 1) / per);
  const int e4 = blockIdx.x * 64 + (threadIdx.x & 63);
  float4 s;
  if (!pp_ordered_rows_sum(reinterpret_cast<const float4*>(part), stride >> 2, 0, rows, e4, 4 * e4 < n, lds, s)) return;
  const float v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int i = 4 * e4 + c;
    if (i >= n) break;
    int seg = 0;
    while (i >= segs.end[seg]) ++seg;
    dst[segs.off[seg] + i - (seg ? segs.end[seg - 1] : 0)] += v[c];      // the only writer of this address in this launch
  }
}

int pp_launch_ordered_flush(const float* part, int stride, int rows_max, const int32_t* count, int cap, int per, const OrdSegs& segs,
                            float* dst, hipStream_t st) {
  const int n4 = pp_div_up(segs.end[segs.n - 1], 4);
  hipLaunchKernelGGL(k_ordered_flush, dim3(pp_div_up(n4, 64)), dim3(ORD_RED_THREADS), 0, st, part, stride, rows_max, count, cap, per,
                     segs, dst);
  return 0;
}

extern "C" int pp_ordered_workspace(int32_t work_groups, int32_t capacity, int32_t n_rays, int64_t* bytes) {
  PP_REQUIRE(bytes, "null pointer");
  PP_REQUIRE(work_groups > 0 && work_groups <= 4096 && capacity > 0 && n_rays > 0, "bad sizes (1 <= work_groups <= 4096, capacity > 0, n_rays > 0)");
  *bytes = pp_ord_layout(work_groups, capacity, n_rays).total * (int64_t)sizeof(float);
  return PP_OK;
}

extern "C" int pp_ordered_attach(void* ctx, void* work, int64_t work_bytes, int32_t work_groups, int32_t capacity, int32_t n_rays) {
  PP_REQUIRE(ctx, "null context (the workspace is recorded in a context: create one)");
  PPContext* c = static_cast<PPContext*>(ctx);
  if (!work) {                      // detach: back to the atomic flushes
    c->ord = nullptr;
    c->ord_wgs = c->ord_cap = c->ord_rays = 0;
    return PP_OK;
  }
  PP_REQUIRE(work_groups > 0 && work_groups <= 4096 && capacity > 0 && n_rays > 0, "bad sizes (1 <= work_groups <= 4096, capacity > 0, n_rays > 0)");
  PP_REQUIRE((reinterpret_cast<uintptr_t>(work) & 15) == 0, "work must be 16-byte aligned");
  PP_REQUIRE(work_bytes >= pp_ord_layout(work_groups, capacity, n_rays).total * (int64_t)sizeof(float),
             "work is smaller than pp_ordered_workspace(work_groups, capacity, n_rays)");
  c->ord = static_cast<float*>(work);
  c->ord_wgs = work_groups < 16 ? 16 : work_groups;
  c->ord_cap = capacity;
  c->ord_rays = n_rays;
  return PP_OK;
}
