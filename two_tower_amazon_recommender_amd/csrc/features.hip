// Dense numeric side features (the Normalization -> concat -> Dense branch of a TFRS query / candidate model): a fixed
// [rows, F] f32 matrix per tower, F <= 32, whose row of the pair's id is normalised, projected by a trained [F, dim] kernel and
// ADDED to the tower's input - and the weight-gradient reduction of that kernel.  Up to two problems (both towers) per launch,
// every problem with its own row count (mixed negative sampling's item side is longer) and its own F.
// Forward: a group of LPR lanes owns a row (LPR = the power of two >= dim/4, at most a wave; a lane holds float4 columns
// l, l + LPR, ... - the shape of normalize.hip and bag.hip).  The row's F normalised values are computed ONCE, by the lanes of
// its group (lane l takes f = l, l + LPR, ...), written to z_out and handed to the others through LDS; then every lane runs
// the skinny product over f ascending for its columns.  The kernel rows come from the cache (F * dim * 4 bytes <= 16 KB at
// dim 128); HBM traffic is n * (8 + 4 F) bytes of ids and feature rows in and 4 * dim (+ 4 F) bytes per row out (twice
// the 4 * dim when accumulating): launch-floor territory at batch 8192.  Every product and sum is a separate correctly
// rounded f32 operation in a fixed order (no contraction): the bits of a row depend on neither the grid nor the other rows.
// Backward: dP[f, d] = sum_b z[b, f] * dy[b, d] as n_slabs partial sums over contiguous row blocks - the slab form the dense
// optimizer segments sum in ascending order.  A workgroup owns (slab, block of kFB features): its RG = 256 / LPR lane groups
// take the slab's rows round robin, every lane holds kFB * 4 accumulators (32 registers: no spill at any F, where one lane
// owning all of F = 32 would hold 128), and the groups' partial sums meet in LDS in ascending group order.  No atomics: a
// slab's bits depend on its rows alone; a slab without rows is written as zeros.
#include "common.h"

namespace {

constexpr int kMaxF = 32;
constexpr int kFB = 8;                      // features per workgroup of the backward launch

struct FeatFwdProb {
  const float* feat; int64_t feat_rows; const int64_t* ids; int64_t n;
  const float* mean; const float* inv_std; const float* proj; float* out; float* z_out;
  int F; int accumulate;
};
struct FeatFwdArgs { FeatFwdProb p[2]; };

struct FeatBwdProb { const float* z; const float* dy; float* dp; int64_t n; int64_t rows_per_slab; int F; int n_slabs; };
struct FeatBwdArgs { FeatBwdProb p[2]; };

__global__ __launch_bounds__(256) void features_fwd_kernel(FeatFwdArgs a, int dim4, int lpr_log2, float clip,
                                                           int32_t* __restrict__ oob_flag) {
  __shared__ float zs[256 * kMaxF];          // [row group of the block][f]; 256 groups only at dim 4
  const FeatFwdProb& p = a.p[blockIdx.y];
  const int lpr = 1 << lpr_log2;
  const int groups = 256 >> lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int g = threadIdx.x >> lpr_log2;
  const int64_t b = (int64_t)blockIdx.x * groups + g;
  if ((int64_t)blockIdx.x * groups >= p.n) return;       // (uniform over the block: the shorter problem's tail blocks)
  const bool live = b < p.n;
  const int F = p.F;

  int64_t id = -1;
  if (live) {
    id = p.ids[b];
    if (id < 0 || id >= p.feat_rows) {                   // (tt_embedding_gather's rule: a zero row; -1 sets no flag)
      if (id != -1 && l == 0 && oob_flag != nullptr) atomicOr(oob_flag, 1);
      id = -1;
    }
  }
  for (int f = l; f < F; f += lpr) {
    float z = 0.0f;
    if (id >= 0) {
      z = p.feat[id * F + f];
      if (p.mean != nullptr) z = __fmul_rn(__fsub_rn(z, p.mean[f]), p.inv_std[f]);
      if (clip > 0.0f) z = fminf(fmaxf(z, -clip), clip);
    }
    zs[g * F + f] = z;
    if (live && p.z_out != nullptr) p.z_out[b * F + f] = z;
  }
  __syncthreads();
  if (!live) return;

  const tt::f32x4* __restrict__ proj = reinterpret_cast<const tt::f32x4*>(p.proj);
  tt::f32x4* __restrict__ out = reinterpret_cast<tt::f32x4*>(p.out);
  for (int c = l; c < dim4; c += lpr) {
    tt::f32x4 o = tt::f32x4{0.f, 0.f, 0.f, 0.f};
    if (p.accumulate) o = out[b * dim4 + c];             // loaded ahead of the product, used after it
    tt::f32x4 acc = tt::f32x4{0.f, 0.f, 0.f, 0.f};
    for (int f = 0; f < F; ++f) {
      const float z = zs[g * F + f];
      const tt::f32x4 w = proj[(int64_t)f * dim4 + c];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = __fadd_rn(acc[q], __fmul_rn(z, w[q]));
    }
    if (p.accumulate) {
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = __fadd_rn(o[q], acc[q]);
    }
    out[b * dim4 + c] = acc;
  }
}

__global__ __launch_bounds__(256) void features_bwd_kernel(FeatBwdArgs a, int dim4, int lpr_log2) {
  __shared__ float red[256 * kFB * 4];       // [row group][j][column of the (padded) row]: 32 KB
  const FeatBwdProb& p = a.p[blockIdx.z];
  const int s = blockIdx.x;
  const int f0 = blockIdx.y * kFB;
  if (s >= p.n_slabs || f0 >= p.F) return;               // (uniform over the block)
  const int lpr = 1 << lpr_log2;
  const int rg_count = 256 >> lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int rg = threadIdx.x >> lpr_log2;
  const int F = p.F;
  const int64_t row0 = (int64_t)s * p.rows_per_slab;
  const int64_t row1 = row0 + p.rows_per_slab < p.n ? row0 + p.rows_per_slab : p.n;
  const tt::f32x4* __restrict__ dy = reinterpret_cast<const tt::f32x4*>(p.dy);
  const int width = lpr * 4;                             // columns of the padded row in `red`
  const int dim = dim4 * 4;

  for (int cb = 0; cb < dim4; cb += lpr) {               // one pass up to dim 256; every lane of the block makes every pass
    const int c = cb + l;
    const bool active = c < dim4;
    tt::f32x4 acc[kFB];
#pragma unroll
    for (int j = 0; j < kFB; ++j) acc[j] = tt::f32x4{0.f, 0.f, 0.f, 0.f};
    if (active) {
#pragma unroll 4
      for (int64_t r = row0 + rg; r < row1; r += rg_count) {
        const tt::f32x4 g = dy[r * dim4 + c];
#pragma unroll
        for (int j = 0; j < kFB; ++j) {
          const float z = f0 + j < F ? p.z[r * F + f0 + j] : 0.0f;
          acc[j] = acc[j] + g * z;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kFB; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[(rg * kFB + j) * width + l * 4 + q] = acc[j][q];
    __syncthreads();
    // element e = (j, column inside this pass): the groups' partial sums in ascending group order
    const int cols = (dim4 - cb < lpr ? dim4 - cb : lpr) * 4;                   // columns this pass covers
    for (int e = threadIdx.x; e < kFB * width; e += 256) {
      const int j = e / width, col = e - j * width;
      if (col >= cols || f0 + j >= F) continue;
      float t = red[j * width + col];
      for (int k = 1; k < rg_count; ++k) t = t + red[(k * kFB + j) * width + col];
      p.dp[((int64_t)s * F + f0 + j) * dim + cb * 4 + col] = t;
    }
    __syncthreads();
  }
}

int lanes_per_row_log2(int dim4) {
  int lg = 0;
  while ((1 << lg) < dim4 && lg < 6) ++lg;
  return lg;
}

}  // namespace

extern "C" int32_t tt_dense_features_num_slabs(int64_t n) {
  if (n <= 0) return 1;
  const int64_t s = (n + 127) / 128;                     // 128-row slabs, at most 64 of them (8192 rows: 64)
  return (int32_t)(s < 64 ? s : 64);
}

extern "C" int tt_dense_features_fwd_f32(const tt_dense_features_fwd_args* probs, int32_t n_probs, int32_t dim, float clip,
                                         int32_t* oob_flag, tt_stream_t stream) {
  const char* who = "tt_dense_features_fwd_f32";
  TT_REQUIRE(probs != nullptr, "%s: null pointer (probs)", who);
  TT_REQUIRE(n_probs >= 1 && n_probs <= 2, "%s: n_probs must be 1 or 2 (got %d)", who, n_probs);
  TT_REQUIRE(dim >= 4 && dim <= 1024 && dim % 4 == 0, "%s: dim must be a multiple of 4 in 4..1024 (got %d)", who, dim);
  TT_REQUIRE(clip >= 0.0f, "%s: clip must be >= 0 (0: no clipping)", who);
  FeatFwdArgs a{};
  int64_t n_max = 0;
  for (int i = 0; i < n_probs; ++i) {
    const tt_dense_features_fwd_args& q = probs[i];
    TT_REQUIRE(q.F >= 1 && q.F <= kMaxF, "%s: F must be in 1..%d (problem %d: %d)", who, kMaxF, i, q.F);
    TT_REQUIRE((q.mean == nullptr) == (q.inv_std == nullptr), "%s: mean and inv_std are given both or neither (problem %d)", who, i);
    TT_REQUIRE(q.n >= 0 && q.feat_rows >= 1, "%s: n must be >= 0 and feat_rows >= 1 (problem %d)", who, i);
    TT_REQUIRE(q.feat && q.proj && q.out && (q.ids || q.n == 0), "%s: null pointer (problem %d)", who, i);
    TT_REQUIRE(tt::aligned16(q.proj) && tt::aligned16(q.out), "%s: proj / out must be 16-byte aligned (problem %d)", who, i);
    a.p[i] = FeatFwdProb{q.feat, q.feat_rows, q.ids, q.n, q.mean, q.inv_std, q.proj, q.out, q.z_out, q.F, q.accumulate != 0};
    if (q.n > n_max) n_max = q.n;
  }
  if (n_max == 0) return TT_OK;
  const int dim4 = dim / 4;
  const int lg = lanes_per_row_log2(dim4);
  const int64_t groups = 256 >> lg;
  const int64_t blocks = (n_max + groups - 1) / groups;
  TT_REQUIRE(blocks <= 0x7fffffff, "%s: too many rows", who);
  tt::launch("features_fwd", features_fwd_kernel, dim3((unsigned)blocks, (unsigned)n_probs), dim3(256), 0, tt::as_stream(stream),
             a, dim4, lg, clip, oob_flag);
  return tt::check_launch(who);
}

extern "C" int tt_dense_features_bwd_f32(const tt_dense_features_bwd_args* probs, int32_t n_probs, int32_t dim, tt_stream_t stream) {
  const char* who = "tt_dense_features_bwd_f32";
  TT_REQUIRE(probs != nullptr, "%s: null pointer (probs)", who);
  TT_REQUIRE(n_probs >= 1 && n_probs <= 2, "%s: n_probs must be 1 or 2 (got %d)", who, n_probs);
  TT_REQUIRE(dim >= 4 && dim <= 1024 && dim % 4 == 0, "%s: dim must be a multiple of 4 in 4..1024 (got %d)", who, dim);
  FeatBwdArgs a{};
  int slabs_max = 0, f_max = 0;
  for (int i = 0; i < n_probs; ++i) {
    const tt_dense_features_bwd_args& q = probs[i];
    TT_REQUIRE(q.F >= 1 && q.F <= kMaxF, "%s: F must be in 1..%d (problem %d: %d)", who, kMaxF, i, q.F);
    TT_REQUIRE(q.n >= 0, "%s: n must be >= 0 (problem %d)", who, i);
    TT_REQUIRE(q.n_slabs >= 1 && q.n_slabs <= 65535, "%s: n_slabs must be in 1..65535 (problem %d: %d)", who, i, q.n_slabs);
    TT_REQUIRE(q.dp_slabs && ((q.z && q.dy) || q.n == 0), "%s: null pointer (problem %d)", who, i);
    TT_REQUIRE(tt::aligned16(q.dy), "%s: dy must be 16-byte aligned (problem %d)", who, i);
    const int64_t rps = (q.n + q.n_slabs - 1) / q.n_slabs;
    a.p[i] = FeatBwdProb{q.z, q.dy, q.dp_slabs, q.n, rps, q.F, q.n_slabs};
    if (q.n_slabs > slabs_max) slabs_max = q.n_slabs;
    if (q.F > f_max) f_max = q.F;
  }
  const int dim4 = dim / 4;
  const int lg = lanes_per_row_log2(dim4);
  tt::launch("features_bwd", features_bwd_kernel, dim3((unsigned)slabs_max, (unsigned)((f_max + kFB - 1) / kFB), (unsigned)n_probs),
             dim3(256), 0, tt::as_stream(stream), a, dim4, lg);
  return tt::check_launch(who);
}
