// The per-row symmetric int8 quantiser (one copy of the formula for tt_quantize_rows_i8, the scan of topk_i8.hip and the
// list scan of ivf_i8.hip), the operand types of v_mfma_i32_32x32x32_i8, and the finish launch both int8 searches end with.
//   amax = max|x|, scale = amax / 127.0f (one IEEE f32 division), code = clamp(rintf(x / scale), -127, 127) (half to even);
//   a row with amax == 0 has scale 0 and all-zero codes.
#pragma once
#include "common.h"

namespace tt {
namespace i8 {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int kRing = 4;                 // tile buffers of a scan: one being scored, three in flight

__device__ __forceinline__ float row_scale(float amax) { return amax / 127.0f; }

__device__ __forceinline__ int quant1(float x, float scale) {
  if (scale == 0.f) return 0;
  float r = rintf(x / scale);
  r = fminf(fmaxf(r, -127.f), 127.f);
  return (int)r;
}

__device__ __forceinline__ int quant4(f32x4 v, float scale) {
  return (quant1(v[0], scale) & 255) | ((quant1(v[1], scale) & 255) << 8) | ((quant1(v[2], scale) & 255) << 16) |
         ((quant1(v[3], scale) & 255) << 24);
}

__device__ __forceinline__ float amax4(float m, f32x4 v) {
  return fmaxf(fmaxf(fmaxf(m, fabsf(v[0])), fmaxf(fabsf(v[1]), fabsf(v[2]))), fabsf(v[3]));
}

}  // namespace i8

// Stage 2 of an int8 search (topk_i8.hip), from the merged stage-1 candidates: cand_s / cand_i [nq][k1] (keys sorted, ids
// int64 into c, padding (-inf, -1) a suffix) and qscale [nq].  With c: i8_rerank_kernel (exact f32 scores of the candidates'
// rows c + id * dim, best k by counting); without (k1 == k): i8_scale_kernel.  One launch, arguments already validated.
int i8_finish_launch(const float* q, const float* c, const float* cand_s, const int64_t* cand_i, const float* qscale, int64_t nq,
                     int dim, int k, int k1, float* out_scores, int64_t* out_idx, hipStream_t stream);

}  // namespace tt
