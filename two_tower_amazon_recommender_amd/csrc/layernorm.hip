// Layer normalisation of a tower's hidden layers (Keras LayerNormalization between a Dense layer and its activation) and its
// backward pass, for up to two towers per launch, every one with its own row count.  Per row of z [rows, dim]:
//   mu = mean(z)   var = mean((z - mu)^2)   r = 1 / sqrt(var + eps)   xhat = (z - mu) * r      (biased, two-pass)
//   y  = dropout(relu(xhat * gamma + beta))                                  product and sum rounded separately
// and, for dn = dL/d(xhat * gamma + beta) (the ReLU / dropout mask is applied by the dx epilogue of the layer above):
//   g = dn * gamma   dz = r * ((g - mean(g)) - xhat * mean(g * xhat))   dgamma = sum_rows dn * xhat   dbeta = sum_rows dn
// HBM-bound: z read + y written forward (8 * rows * dim bytes), z and dn read + dz written backward (12 * rows * dim).
// The lane layout is csrc/normalize.hip's: a group of LPR lanes owns a row (LPR = the power of two >= dim/4, at most a wave; a
// lane holds NV = ceil(dim / 256) float4 of it, float4 column c = lane + i * LPR), the row sums are a fixed-order butterfly
// inside the group and every lane ends with the same bits: no atomics, and row r of y / dz depends on row r alone - not on
// the grid, the number of problems or the number of rows.  dim % 32 == 0, so eight neighbouring lanes hold the 32 columns of
// one sign-bit word: they OR their nibbles together (three shuffles) and the first of them stores the word.
// Backward: ONE workgroup per (slab, problem) walks the slab's rows, R rows per lane group and trip; every lane keeps the
// dgamma / dbeta sums of its own columns in registers (rows ascending), the groups' sums are added through LDS in ascending
// group order and the slab is written in full - an empty one as zeros.  mu and r are recomputed from the z registers.
#include "common.h"

namespace {

using tt::f32x4;

struct LnFwdArgs {
  tt_layer_norm_fwd_args p[2];
  uint64_t drop_key[2];
  uint64_t drop_offset;
  unsigned blocks0;               // workgroups of problem 0 (the rest belong to problem 1)
  uint32_t drop_p24;
  float drop_scale;
  int relu;
};
struct LnBwdArgs {
  tt_layer_norm_bwd_args p[2];
  int64_t rows_per_slab[2];
  int64_t slab_stride;
};

// sum over the lanes of a group of 1 << lpr_log2 lanes; identical bits in every lane of the group (a + b == b + a)
__device__ __forceinline__ float group_sum(float v, int lpr_log2) {
  for (int s = 0; s < lpr_log2; ++s) v = v + __shfl_xor(v, 1 << s, 64);
  return v;
}
__device__ __forceinline__ float sum4(float s, const f32x4& a) {
  s = s + a.x; s = s + a.y; s = s + a.z; s = s + a.w;
  return s;
}
__device__ __forceinline__ float dot4(float s, const f32x4& a, const f32x4& b) {
  s = s + a.x * b.x; s = s + a.y * b.y; s = s + a.z * b.z; s = s + a.w * b.w;
  return s;
}

// mean and 1 / sqrt(var + eps) of the row whose float4 v[0 .. NV) this lane group holds (lanes past the row hold `live` =
// false and zeros); d = z - mu is left in v
template <int NV>
__device__ __forceinline__ float row_stats(f32x4 (&v)[NV], const bool (&live)[NV], int lpr_log2, float fdim, float eps) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) s = sum4(s, v[i]);
  const float mu = group_sum(s, lpr_log2) / fdim;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (live[i]) v[i] = v[i] - mu;
    q = dot4(q, v[i], v[i]);
  }
  const float var = group_sum(q, lpr_log2) / fdim;
  return 1.0f / sqrtf(var + eps);                          // correctly rounded division and square root (no v_rsq estimate)
}

template <int R, int NV, bool DROP>
__global__ __launch_bounds__(256) void layer_norm_fwd_kernel(LnFwdArgs a, int dim4, int lpr_log2, float fdim, float eps) {
  const bool second = blockIdx.x >= a.blocks0;
  const tt_layer_norm_fwd_args p = second ? a.p[1] : a.p[0];
  const f32x4* z = reinterpret_cast<const f32x4*>(p.z);
  const f32x4* gamma = reinterpret_cast<const f32x4*>(p.gamma);
  const f32x4* beta = reinterpret_cast<const f32x4*>(p.beta);
  f32x4* y = reinterpret_cast<f32x4*>(p.y);
  const int lpr = 1 << lpr_log2;
  const int groups = 256 >> lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int64_t row0 = (int64_t)(blockIdx.x - (second ? a.blocks0 : 0u)) * (R * groups) + (threadIdx.x >> lpr_log2);

  f32x4 v[R][NV], gm[NV], bt[NV];
  bool live[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = l + i * lpr;
    live[i] = c < dim4;
    gm[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    bt[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live[i]) { gm[i] = gamma[c]; bt[i] = beta[c]; }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + (int64_t)r * groups;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      v[r][i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (row < p.rows && live[i]) v[r][i] = z[row * dim4 + l + i * lpr];
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + (int64_t)r * groups;
    const float rs = row_stats<NV>(v[r], live, lpr_log2, fdim, eps);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = l + i * lpr;
      f32x4 o = (v[r][i] * rs) * gm[i] + bt[i];
      uint32_t nib = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float e = o[k];
        if (a.relu) e = fmaxf(e, 0.f);
        if constexpr (DROP) {      // the stream of the GEMM epilogue: element (row, col) uses counter offset + row * dim + col
          const uint64_t ctr = a.drop_offset + (uint64_t)row * (uint64_t)(4 * dim4) + (uint64_t)(4 * c + k);
          const uint64_t hsh = tt::splitmix((second ? a.drop_key[1] : a.drop_key[0]) + ctr);
          e = ((uint32_t)(hsh >> 40) < a.drop_p24) ? 0.f : e * a.drop_scale;
        }
        o[k] = e;
        nib |= (e > 0.f ? 1u : 0u) << k;
      }
      const bool mine = row < p.rows && live[i];
      if (mine) y[row * dim4 + c] = o;
      if (p.relu_bits != nullptr) {                        // (uniform per problem) the word of float4 columns 8w .. 8w + 7
        uint32_t word = mine ? nib << (4 * (c & 7)) : 0u;
        word |= __shfl_xor(word, 1, 64);
        word |= __shfl_xor(word, 2, 64);
        word |= __shfl_xor(word, 4, 64);
        if (mine && (c & 7) == 0) p.relu_bits[row * (dim4 >> 3) + (c >> 3)] = word;
      }
    }
  }
}

// dz may be dn: a lane loads every element it owns before it stores any, and no other lane touches them
template <int R, int NV>
__global__ __launch_bounds__(256) void layer_norm_bwd_kernel(LnBwdArgs a, int dim4, int lpr_log2, float fdim, float eps) {
  __shared__ f32x4 red[2 * NV * 256];                      // [group][dgamma | dbeta][float4 column]
  const int pi = blockIdx.y;
  const tt_layer_norm_bwd_args p = pi ? a.p[1] : a.p[0];
  const f32x4* z = reinterpret_cast<const f32x4*>(p.z);
  const f32x4* dn = reinterpret_cast<const f32x4*>(p.dn);
  const f32x4* gamma = reinterpret_cast<const f32x4*>(p.gamma);
  f32x4* dz = reinterpret_cast<f32x4*>(p.dz);
  const int lpr = 1 << lpr_log2;
  const int groups = 256 >> lpr_log2;
  const int l = threadIdx.x & (lpr - 1), grp = threadIdx.x >> lpr_log2;
  const int64_t rps = pi ? a.rows_per_slab[1] : a.rows_per_slab[0];
  const int64_t s0 = (int64_t)blockIdx.x * rps;
  const int64_t s1 = s0 + rps < p.rows ? s0 + rps : p.rows;                 // (s1 <= s0: a slab without rows)

  f32x4 gm[NV], dga[NV], dba[NV];
  bool live[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = l + i * lpr;
    live[i] = c < dim4;
    gm[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live[i]) gm[i] = gamma[c];
    dga[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    dba[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // (the trip count is uniform over the workgroup: lane groups past the slab's end load nothing, add zeros and store nothing)
  for (int64_t t0 = s0; t0 < s1; t0 += (int64_t)R * groups) {
    f32x4 v[R][NV], g[R][NV];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = t0 + grp + (int64_t)r * groups;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        v[r][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        g[r][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (row < s1 && live[i]) {
          v[r][i] = z[row * dim4 + l + i * lpr];
          g[r][i] = dn[row * dim4 + l + i * lpr];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = t0 + grp + (int64_t)r * groups;
      const float rs = row_stats<NV>(v[r], live, lpr_log2, fdim, eps);
      float sg = 0.f, sgx = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        v[r][i] = v[r][i] * rs;                            // xhat
        dba[i] = dba[i] + g[r][i];
        dga[i] = dga[i] + g[r][i] * v[r][i];
        g[r][i] = g[r][i] * gm[i];
        sg = sum4(sg, g[r][i]);
        sgx = dot4(sgx, g[r][i], v[r][i]);
      }
      const float m1 = group_sum(sg, lpr_log2) / fdim;
      const float m2 = group_sum(sgx, lpr_log2) / fdim;
#pragma unroll
      for (int i = 0; i < NV; ++i)
        if (row < s1 && live[i]) dz[row * dim4 + l + i * lpr] = ((g[r][i] - m1) - v[r][i] * m2) * rs;
    }
  }

  const int span = lpr * NV;                               // float4 columns a group's lanes cover (>= dim4)
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    red[(grp * 2 + 0) * span + l + i * lpr] = dga[i];
    red[(grp * 2 + 1) * span + l + i * lpr] = dba[i];
  }
  __syncthreads();
  float* dgs = p.dgamma_slabs + (int64_t)blockIdx.x * a.slab_stride;
  float* dbs = p.dbeta_slabs + (int64_t)blockIdx.x * a.slab_stride;
  for (int j = threadIdx.x; j < 2 * dim4; j += 256) {
    const int which = j >= dim4 ? 1 : 0, c = j - which * dim4;
    f32x4 t = red[which * span + c];
    for (int k = 1; k < groups; ++k) t = t + red[(k * 2 + which) * span + c];
    float* out = (which ? dbs : dgs) + 4 * c;              // (a slab is only 4-byte aligned in general: 4-byte stores)
    out[0] = t.x; out[1] = t.y; out[2] = t.z; out[3] = t.w;
  }
}

int lanes_per_row_log2(int dim4) {
  int lg = 0;
  while ((1 << lg) < dim4 && lg < 6) ++lg;
  return lg;
}

int check_common(const char* who, const void* probs, int32_t n_probs, int32_t dim, float eps) {
  TT_REQUIRE(probs != nullptr, "%s: probs is NULL", who);
  TT_REQUIRE(n_probs >= 1 && n_probs <= 2, "%s: n_probs must be 1 or 2 (got %d)", who, n_probs);
  TT_REQUIRE(dim >= 32 && dim <= 1024 && dim % 32 == 0, "%s: dim must be a multiple of 32 in 32..1024 (got %d)", who, dim);
  TT_REQUIRE(eps > 0.0f, "%s: eps must be > 0", who);
  return TT_OK;
}

template <bool DROP>
void launch_fwd(int nv, dim3 grid, hipStream_t stream, const LnFwdArgs& a, int dim4, int lg, float fdim, float eps) {
  const dim3 block(256);
  switch (nv) {
    case 1: tt::launch("layer_norm_fwd", layer_norm_fwd_kernel<2, 1, DROP>, grid, block, 0, stream, a, dim4, lg, fdim, eps); break;
    case 2: tt::launch("layer_norm_fwd", layer_norm_fwd_kernel<1, 2, DROP>, grid, block, 0, stream, a, dim4, lg, fdim, eps); break;
    case 3: tt::launch("layer_norm_fwd", layer_norm_fwd_kernel<1, 3, DROP>, grid, block, 0, stream, a, dim4, lg, fdim, eps); break;
    default: tt::launch("layer_norm_fwd", layer_norm_fwd_kernel<1, 4, DROP>, grid, block, 0, stream, a, dim4, lg, fdim, eps); break;
  }
}

}  // namespace

extern "C" int32_t tt_layer_norm_num_slabs(int64_t rows) {
  if (rows <= 0) return 1;
  const int64_t s = (rows + 31) / 32;                      // 32-row slabs, at most 256 of them (a workgroup per slab and tower)
  return (int32_t)(s < 256 ? s : 256);
}

extern "C" int tt_layer_norm_fwd_f32(const tt_layer_norm_fwd_args* probs, int32_t n_probs, int32_t dim, float eps, int32_t relu,
                                     float drop_rate, uint64_t seed, uint64_t counter_offset, tt_stream_t stream) {
  const char* who = "tt_layer_norm_fwd_f32";
  if (int rc = check_common(who, probs, n_probs, dim, eps)) return rc;
  TT_REQUIRE(drop_rate >= 0.f && drop_rate < 1.f, "%s: drop_rate must be in [0,1)", who);
  const int dim4 = dim / 4;
  const int lg = lanes_per_row_log2(dim4);
  const int nv = (dim4 + (1 << lg) - 1) >> lg;             // 1 up to dim 256, then ceil(dim / 256) <= 4
  const int64_t rows_per_block = (int64_t)(256 >> lg) * (nv == 1 ? 2 : 1);
  LnFwdArgs a{};
  int64_t blocks[2] = {0, 0};
  for (int i = 0; i < n_probs; ++i) {
    const tt_layer_norm_fwd_args& p = probs[i];
    TT_REQUIRE(p.rows >= 0, "%s: problem %d: rows must be >= 0", who, i);
    a.p[i] = p;
    if (p.rows == 0) continue;
    TT_REQUIRE(p.z && p.gamma && p.beta && p.y, "%s: problem %d: null pointer", who, i);
    TT_REQUIRE(tt::aligned16(p.z) && tt::aligned16(p.gamma) && tt::aligned16(p.beta) && tt::aligned16(p.y),
               "%s: problem %d: z, gamma, beta and y must be 16-byte aligned", who, i);
    TT_REQUIRE(p.y != p.z, "%s: problem %d: y must not alias z (the backward pass reads z)", who, i);
    blocks[i] = (p.rows + rows_per_block - 1) / rows_per_block;
    if (drop_rate > 0.f) a.drop_key[i] = tt::stream_key(seed, p.dropout_tensor_id);
  }
  TT_REQUIRE(blocks[0] + blocks[1] <= 0x7fffffff, "%s: too many rows", who);
  if (blocks[0] + blocks[1] == 0) return TT_OK;
  a.blocks0 = (unsigned)blocks[0];
  a.relu = relu != 0;
  a.drop_offset = counter_offset;
  const dim3 grid((unsigned)(blocks[0] + blocks[1]));
  const float fdim = (float)dim;
  if (drop_rate > 0.f) {
    a.drop_p24 = (uint32_t)((double)drop_rate * 16777216.0 + 0.5);
    a.drop_scale = 1.0f / (1.0f - drop_rate);
    launch_fwd<true>(nv, grid, tt::as_stream(stream), a, dim4, lg, fdim, eps);
  } else {
    launch_fwd<false>(nv, grid, tt::as_stream(stream), a, dim4, lg, fdim, eps);
  }
  return tt::check_launch(who);
}

extern "C" int tt_layer_norm_bwd_f32(const tt_layer_norm_bwd_args* probs, int32_t n_probs, int32_t dim, float eps, int32_t n_slabs,
                                     int64_t slab_stride, tt_stream_t stream) {
  const char* who = "tt_layer_norm_bwd_f32";
  if (int rc = check_common(who, probs, n_probs, dim, eps)) return rc;
  TT_REQUIRE(n_slabs >= 1 && n_slabs <= 65535, "%s: n_slabs must be in 1..65535 (got %d)", who, n_slabs);
  TT_REQUIRE(n_slabs == 1 || slab_stride >= 2 * (int64_t)dim, "%s: slab_stride must be >= 2 * dim", who);
  LnBwdArgs a{};
  a.slab_stride = slab_stride;
  bool any = false;
  for (int i = 0; i < n_probs; ++i) {
    TT_REQUIRE(probs[i].rows >= 0, "%s: problem %d: rows must be >= 0", who, i);
    any = any || probs[i].rows > 0;
  }
  if (!any) return TT_OK;
  for (int i = 0; i < n_probs; ++i) {
    const tt_layer_norm_bwd_args& p = probs[i];
    a.p[i] = p;
    TT_REQUIRE(p.gamma && p.dgamma_slabs && p.dbeta_slabs, "%s: problem %d: null pointer", who, i);
    TT_REQUIRE(tt::aligned16(p.gamma), "%s: problem %d: gamma must be 16-byte aligned", who, i);
    if (p.rows > 0) {
      TT_REQUIRE(p.z && p.dn && p.dz, "%s: problem %d: null pointer", who, i);
      TT_REQUIRE(tt::aligned16(p.z) && tt::aligned16(p.dn) && tt::aligned16(p.dz), "%s: problem %d: z, dn and dz must be 16-byte aligned", who, i);
      TT_REQUIRE(p.dz != p.z, "%s: problem %d: dz must not alias z", who, i);
    }
    a.rows_per_slab[i] = (p.rows + n_slabs - 1) / n_slabs;
  }
  const int dim4 = dim / 4;
  const int lg = lanes_per_row_log2(dim4);
  const int nv = (dim4 + (1 << lg) - 1) >> lg;
  const dim3 grid((unsigned)n_slabs, (unsigned)n_probs), block(256);
  const float fdim = (float)dim;
  hipStream_t st = tt::as_stream(stream);
  switch (nv) {
    case 1: tt::launch("layer_norm_bwd", layer_norm_bwd_kernel<2, 1>, grid, block, 0, st, a, dim4, lg, fdim, eps); break;
    case 2: tt::launch("layer_norm_bwd", layer_norm_bwd_kernel<1, 2>, grid, block, 0, st, a, dim4, lg, fdim, eps); break;
    case 3: tt::launch("layer_norm_bwd", layer_norm_bwd_kernel<1, 3>, grid, block, 0, st, a, dim4, lg, fdim, eps); break;
    default: tt::launch("layer_norm_bwd", layer_norm_bwd_kernel<1, 4>, grid, block, 0, st, a, dim4, lg, fdim, eps); break;
  }
  return tt::check_launch(who);
}
