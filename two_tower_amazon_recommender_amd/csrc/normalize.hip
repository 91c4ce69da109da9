// L2 normalisation of tower outputs (tf.math.l2_normalize) and its backward pass, for up to two towers per launch.
// HBM-bound: 4*dim bytes read + 4*dim written per row forward (8*rows*dim per tower), x and dy read + dx written
// backward (12*rows*dim).  A group of LPR lanes owns a row (LPR = the power of two >= dim/4, at most a wave: 8 lanes at
// dim 32, 16 at 64, 32 at 128, 64 from 256 on, where a lane holds NV = ceil(dim/256) float4 of the row), so a wave owns
// 64/LPR rows and every lane moves 16 bytes per load / store.  The row sums are a fixed-order butterfly inside the lane
// group (__shfl_xor, distances 1, 2, 4, ...: every lane ends with the same bits): no LDS, no barrier, no atomics, and the
// result of a row depends on neither the grid nor the number of problems.  Rows past the end load nothing, store
// nothing and still take part in the shuffles (a lane group is wholly inside or wholly outside).
#include "common.h"

namespace {

struct L2FwdArgs { const float* x[2]; float* y[2]; };
struct L2BwdArgs { const float* x[2]; const float* dy[2]; float* dx[2]; };

// sum over the lanes of a group of 1 << lpr_log2 lanes; identical bits in every lane of the group (a + b == b + a)
__device__ __forceinline__ float group_sum(float v, int lpr_log2) {
  for (int s = 0; s < lpr_log2; ++s) v = v + __shfl_xor(v, 1 << s, 64);
  return v;
}

__device__ __forceinline__ float sq4(float s, const tt::f32x4& a) {
  s = s + a.x * a.x; s = s + a.y * a.y; s = s + a.z * a.z; s = s + a.w * a.w;
  return s;
}
__device__ __forceinline__ float dot4(float s, const tt::f32x4& a, const tt::f32x4& b) {
  s = s + a.x * b.x; s = s + a.y * b.y; s = s + a.z * b.z; s = s + a.w * b.w;
  return s;
}

// R rows per lane group (independent loads in flight), NV float4 per lane and row
template <int R, int NV>
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(L2FwdArgs a, int64_t rows, int dim4, int lpr_log2, float eps) {
  const int p = blockIdx.y;
  const tt::f32x4* x = reinterpret_cast<const tt::f32x4*>(a.x[p]);
  tt::f32x4* y = reinterpret_cast<tt::f32x4*>(a.y[p]);
  const int lpr = 1 << lpr_log2;
  const int groups = 256 >> lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int64_t row0 = (int64_t)blockIdx.x * (R * groups) + (threadIdx.x >> lpr_log2);

  tt::f32x4 v[R][NV];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + (int64_t)r * groups;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = l + i * lpr;
      v[r][i] = tt::f32x4{0.f, 0.f, 0.f, 0.f};
      if (row < rows && c < dim4) v[r][i] = x[row * dim4 + c];
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + (int64_t)r * groups;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s = sq4(s, v[r][i]);
    s = group_sum(s, lpr_log2);
    const float inv = 1.0f / sqrtf(fmaxf(s, eps));        // correctly rounded division and square root (no v_rsq estimate)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = l + i * lpr;
      if (row < rows && c < dim4) y[row * dim4 + c] = v[r][i] * inv;
    }
  }
}

// dx may be dy: a lane loads every element it owns before it stores any, and no other lane touches them
template <int R, int NV>
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(L2BwdArgs a, int64_t rows, int dim4, int lpr_log2, float eps) {
  const int p = blockIdx.y;
  const tt::f32x4* x = reinterpret_cast<const tt::f32x4*>(a.x[p]);
  const tt::f32x4* dy = reinterpret_cast<const tt::f32x4*>(a.dy[p]);
  tt::f32x4* dx = reinterpret_cast<tt::f32x4*>(a.dx[p]);
  const int lpr = 1 << lpr_log2;
  const int groups = 256 >> lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int64_t row0 = (int64_t)blockIdx.x * (R * groups) + (threadIdx.x >> lpr_log2);

  tt::f32x4 v[R][NV], g[R][NV];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + (int64_t)r * groups;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = l + i * lpr;
      v[r][i] = tt::f32x4{0.f, 0.f, 0.f, 0.f};
      g[r][i] = tt::f32x4{0.f, 0.f, 0.f, 0.f};
      if (row < rows && c < dim4) {
        v[r][i] = x[row * dim4 + c];
        g[r][i] = dy[row * dim4 + c];
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + (int64_t)r * groups;
    float s = 0.f, t = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      s = sq4(s, v[r][i]);
      t = dot4(t, v[r][i], g[r][i]);
    }
    s = group_sum(s, lpr_log2);
    t = group_sum(t, lpr_log2);
    // s >= eps: y = x / sqrt(s), dx = inv * (dy - x * (t * inv * inv)); clamped: y = x / sqrt(eps) is linear in x
    const bool clamped = !(s >= eps);
    const float inv = 1.0f / sqrtf(clamped ? eps : s);
    const float k = clamped ? 0.f : (t * inv) * inv;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = l + i * lpr;
      if (row < rows && c < dim4) dx[row * dim4 + c] = (g[r][i] - v[r][i] * k) * inv;
    }
  }
}

int lanes_per_row_log2(int dim4) {
  int lg = 0;
  while ((1 << lg) < dim4 && lg < 6) ++lg;
  return lg;
}

template <typename Args, typename K1, typename K2, typename K3, typename K4>
int launch(const char* tag, const char* what, const Args& a, int32_t n_probs, int64_t rows, int32_t dim, float eps, hipStream_t stream,
           K1 k1, K2 k2, K3 k3, K4 k4) {
  const int dim4 = dim / 4;
  const int lg = lanes_per_row_log2(dim4);
  const int nv = (dim4 + (1 << lg) - 1) >> lg;            // 1 up to dim 256, then ceil(dim / 256) <= 4
  const int r = nv == 1 ? 2 : 1;
  const int64_t rows_per_block = (int64_t)(256 >> lg) * r;
  const int64_t blocks = (rows + rows_per_block - 1) / rows_per_block;
  TT_REQUIRE(blocks <= 0x7fffffff, "%s: too many rows", what);
  const dim3 grid((unsigned)blocks, (unsigned)n_probs), block(256);
  switch (nv) {
    case 1: tt::launch(tag, k1, grid, block, 0, stream, a, rows, dim4, lg, eps); break;
    case 2: tt::launch(tag, k2, grid, block, 0, stream, a, rows, dim4, lg, eps); break;
    case 3: tt::launch(tag, k3, grid, block, 0, stream, a, rows, dim4, lg, eps); break;
    default: tt::launch(tag, k4, grid, block, 0, stream, a, rows, dim4, lg, eps); break;
  }
  return tt::check_launch(what);
}

}  // namespace

#define TT_L2NORM_CHECKS(what)                                                                                        \
  TT_REQUIRE(probs != nullptr, what ": null pointer (probs)");                                                         \
  TT_REQUIRE(n_probs >= 1 && n_probs <= 2, what ": n_probs must be 1 or 2 (got %d)", n_probs);                         \
  TT_REQUIRE(rows >= 0, what ": rows must be >= 0");                                                                   \
  TT_REQUIRE(dim >= 4 && dim <= 1024 && dim % 4 == 0, what ": dim must be a multiple of 4 in 4..1024 (got %d)", dim); \
  TT_REQUIRE(eps > 0.0f, what ": eps must be > 0")

extern "C" int tt_l2_normalize_fwd_f32(const tt_l2norm_fwd_args* probs, int32_t n_probs, int64_t rows, int32_t dim, float eps,
                                       tt_stream_t stream) {
  TT_L2NORM_CHECKS("tt_l2_normalize_fwd_f32");
  if (rows == 0) return TT_OK;
  L2FwdArgs a{};
  for (int i = 0; i < n_probs; ++i) {
    TT_REQUIRE(probs[i].x && probs[i].y, "tt_l2_normalize_fwd_f32: null pointer (problem %d)", i);
    TT_REQUIRE(tt::aligned16(probs[i].x) && tt::aligned16(probs[i].y), "tt_l2_normalize_fwd_f32: x / y must be 16-byte aligned");
    a.x[i] = probs[i].x; a.y[i] = probs[i].y;
  }
  return launch("l2norm_fwd", "tt_l2_normalize_fwd_f32", a, n_probs, rows, dim, eps, tt::as_stream(stream),
                l2norm_fwd_kernel<2, 1>, l2norm_fwd_kernel<1, 2>, l2norm_fwd_kernel<1, 3>, l2norm_fwd_kernel<1, 4>);
}

extern "C" int tt_l2_normalize_bwd_f32(const tt_l2norm_bwd_args* probs, int32_t n_probs, int64_t rows, int32_t dim, float eps,
                                       tt_stream_t stream) {
  TT_L2NORM_CHECKS("tt_l2_normalize_bwd_f32");
  if (rows == 0) return TT_OK;
  L2BwdArgs a{};
  for (int i = 0; i < n_probs; ++i) {
    TT_REQUIRE(probs[i].x && probs[i].dy && probs[i].dx, "tt_l2_normalize_bwd_f32: null pointer (problem %d)", i);
    TT_REQUIRE(tt::aligned16(probs[i].x) && tt::aligned16(probs[i].dy) && tt::aligned16(probs[i].dx),
               "tt_l2_normalize_bwd_f32: x / dy / dx must be 16-byte aligned");
    a.x[i] = probs[i].x; a.dy[i] = probs[i].dy; a.dx[i] = probs[i].dx;
  }
  return launch("l2norm_bwd", "tt_l2_normalize_bwd_f32", a, n_probs, rows, dim, eps, tt::as_stream(stream),
                l2norm_bwd_kernel<2, 1>, l2norm_bwd_kernel<1, 2>, l2norm_bwd_kernel<1, 3>, l2norm_bwd_kernel<1, 4>);
}
