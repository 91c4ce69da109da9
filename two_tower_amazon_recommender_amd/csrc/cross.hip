// DCN-v2 cross layer (tfrs.layers.dcn.Cross, Wang et al. 2021) between a tower's summed input rows x0 and its Dense stack:
//   u = x W + b,   y = x0 * u + x            W [D, D] row-major [in, out], b [D]; product and sum rounded separately
// and its backward pass for an upstream gradient g = dL/dy, with t = g * x0:
//   dx = g + t W^T,   dx0 (+)= g * u,   dW = x^T t,   db = sum over rows of t
// (layer 0, x = x0: dx = ((g + t W^T) + g * u) [+ dx0]).  Both launches run on the f32-input MFMA (v_mfma_f32_32x32x2_f32:
// exact f32 products, the k order of gemm.hip / rating.hip inside a group of 8: k = 8g + 4*lanehalf + s) and cover up to two
// problems - both towers, every one with its own row count.
//
// Forward: a 256-thread workgroup owns 32 rows.  Their x tile sits in LDS ([32][D + 4], 33 KB at D = 256), wave w owns the
// 32-column blocks w, w + 4 of u; W is streamed from global memory, every lane loading its own B fragment one round (four k
// groups, 16 loads) ahead of the MFMAs that use it - the structure of rating_fwd_kernel.  Epilogue: bias, u to HBM when the
// caller keeps it, y = x0 * u + x with x from the LDS tile.
//
// Backward: ONE launch whose grid holds two roles side by side, the dW workgroups (the long ones) first.
//   dx role: a workgroup per 32-row tile builds t = g * x0 in LDS and computes t W^T like the forward pass computes x W - the
//            B fragment of output column i is the contiguous row W[i, :], one 16-byte load per k group - then writes dx and
//            dx0 (upper layers) or the layer-0 sum.
//   dW role: workgroup (slab s, 32-row block y of W) accumulates dW[32y .. 32y + 32, :] += x block^T [32, 32 rows] . t [32 rows, D]
//            over the slab's 32-row tiles, wave w owning the column blocks w, w + 4 with accumulators that stay live across
//            the tiles; db is accumulated by the threads that build t (fixed column per thread) and reduced through LDS in
//            ascending thread-row order by the y = 0 workgroups.
// The dW role reads g while the dx role writes dx: dx must not alias g, x0, x or u.  No atomics: bits depend on
// (n, n_slabs, D) alone.
#include "common.h"

namespace {

using tt::f32x4;
using tt::f32x16;

constexpr int RB = 32;            // rows per tile
constexpr int XS = 36;            // row stride of the transposed x block in LDS

__device__ __forceinline__ f32x4 ldg4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

struct CrossFwdArgs {
  tt_cross_fwd_args p[2];
  unsigned blocks0;               // workgroups of problem 0 (the rest belong to problem 1)
  int D;
};

__global__ __launch_bounds__(256) void cross_fwd_kernel(CrossFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const bool second = blockIdx.x >= a.blocks0;
  const tt_cross_fwd_args p = second ? a.p[1] : a.p[0];
  const int D = a.D, LX = D + 4;
  float* XT = smem;                          // [32][D + 4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, ln = lane & 31;
  const int64_t m0 = (int64_t)(blockIdx.x - (second ? a.blocks0 : 0u)) * RB;

  const int c4n = D / 4;
  for (int f = tid; f < RB * c4n; f += 256) {
    const int row = f / c4n, c4 = f - row * c4n;
    const int64_t r = m0 + row;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (r < p.n) v = ldg4(p.x + r * D + 4 * c4);
    *reinterpret_cast<f32x4*>(XT + row * LX + 4 * c4) = v;
  }
  __syncthreads();

  for (int jb = wave; jb < D / 32; jb += 4) {
    const int col = jb * 32 + ln;
    f32x16 acc;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[reg] = 0.f;
    const float* __restrict__ wp = p.w + col;
    // four k groups (16 W loads per lane) are requested one round ahead of the MFMAs that use them (D / 8 is a multiple of 4;
    // the last round requests the first groups again: in bounds, never used)
    f32x4 bn[4];
    auto request = [&](int g0) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* bp = wp + (int64_t)(8 * (g0 + u) + 4 * hh) * D;
        bn[u] = f32x4{bp[0], bp[D], bp[2 * D], bp[3 * D]};
      }
    };
    request(0);
    for (int g0 = 0; g0 < D / 8; g0 += 4) {
      f32x4 a4[4], b4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        b4[u] = bn[u];
        a4[u] = *reinterpret_cast<const f32x4*>(XT + ln * LX + 8 * (g0 + u) + 4 * hh);
      }
      request(g0 + 4 < D / 8 ? g0 + 4 : 0);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u][s], b4[u][s], acc, 0, 0, 0);
    }
    const float bias = p.b[col];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = tt::acc_row(reg, hh);
      const int64_t r = m0 + row;
      if (r < p.n) {
        const float u = acc[reg] + bias;
        if (p.u_out != nullptr) p.u_out[r * D + col] = u;
        const float xu = p.x0[r * D + col] * u;
        p.y[r * D + col] = xu + XT[row * LX + col];
      }
    }
  }
}

struct CrossBwdArgs {
  tt_cross_bwd_args p[2];
  int64_t rows_per_slab[2];
  unsigned dw_blocks[2];          // n_slabs * D / 32 per problem; the grid: [dW 0 | dW 1 | dx 0 | dx 1]
  unsigned dx_blocks0;
  int D;
};

// dx role: the 32 rows from m0 on
__device__ __forceinline__ void cross_dx_role(const tt_cross_bwd_args& p, int D, int64_t m0, float* smem) {
  const int LX = D + 4;
  float* T = smem;                           // [32][D + 4]: t = g * x0
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, ln = lane & 31;
  const int c4n = D / 4;
  for (int f = tid; f < RB * c4n; f += 256) {
    const int row = f / c4n, c4 = f - row * c4n;
    const int64_t r = m0 + row;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (r < p.n) v = ldg4(p.g + r * D + 4 * c4) * ldg4(p.x0 + r * D + 4 * c4);
    *reinterpret_cast<f32x4*>(T + row * LX + 4 * c4) = v;
  }
  __syncthreads();

  for (int jb = wave; jb < D / 32; jb += 4) {
    const int col = jb * 32 + ln;            // the column i of dx: its B fragment is the row W[i, :]
    f32x16 acc;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[reg] = 0.f;
    const float* __restrict__ wp = p.w + (int64_t)col * D + 4 * hh;
    f32x4 bn[4];
    auto request = [&](int g0) {
#pragma unroll
      for (int u = 0; u < 4; ++u) bn[u] = ldg4(wp + 8 * (g0 + u));
    };
    request(0);
    for (int g0 = 0; g0 < D / 8; g0 += 4) {
      f32x4 a4[4], b4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        b4[u] = bn[u];
        a4[u] = *reinterpret_cast<const f32x4*>(T + ln * LX + 8 * (g0 + u) + 4 * hh);
      }
      request(g0 + 4 < D / 8 ? g0 + 4 : 0);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u][s], b4[u][s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int64_t r = m0 + tt::acc_row(reg, hh);
      if (r < p.n) {
        const int64_t idx = r * D + col;
        const float gv = p.g[idx];
        const float gu = gv * p.u[idx];
        float v = gv + acc[reg];
        if (p.x_is_x0) {                     // layer 0: x is x0, both gradients land in dx
          v = v + gu;
          if (p.dx0 != nullptr) v = v + p.dx0[idx];
        } else {
          p.dx0[idx] = p.accumulate_dx0 ? p.dx0[idx] + gu : gu;
        }
        p.dx[idx] = v;
      }
    }
  }
}

// dW role: slab s, rows 32y .. 32y + 31 of dW (the columns 32y .. of x)
__device__ __forceinline__ void cross_dw_role(const tt_cross_bwd_args& p, int D, int s, int y, int64_t rows_per_slab, float* smem) {
  const int LH = D + 4;
  float* T = smem;                           // [32 rows][D + 4]: t of the tile; the db reduction's scratch at the end
  float* XT = T + RB * LH;                   // [32 columns of x][36]: the x block of the tile, transposed
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, ln = lane & 31;
  const int i0 = RB * y;
  const int64_t row0 = (int64_t)s * rows_per_slab;
  const int64_t row1 = row0 + rows_per_slab < p.n ? row0 + rows_per_slab : p.n;      // (row1 <= row0: a slab without rows)

  const int c4n = D / 4;                     // float4 columns of t: 8 .. 64
  const int rpp = 256 / c4n;                 // rows of t the workgroup builds per pass (D = 96: 10, 240 threads at work)
  const int c4 = tid % c4n, rr = tid / c4n;
  const bool active = rr < rpp;
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 dba = zero4;
  f32x16 accw[2];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) accw[b][reg] = 0.f;
  const int xr = tid >> 3, xc4 = tid & 7;    // the x block: 32 rows x 8 float4, one per thread

  for (int64_t t0 = row0; t0 < row1; t0 += RB) {
    __syncthreads();                         // the previous tile's LDS reads are done
    if (active) {
      for (int r = rr; r < RB; r += rpp) {
        const int64_t row = t0 + r;
        f32x4 tv = zero4;
        if (row < row1) tv = ldg4(p.g + row * D + 4 * c4) * ldg4(p.x0 + row * D + 4 * c4);
        *reinterpret_cast<f32x4*>(T + r * LH + 4 * c4) = tv;
        dba = dba + tv;
      }
    }
    {
      const int64_t row = t0 + xr;
      const f32x4 v = row < row1 ? ldg4(p.x + row * D + i0 + 4 * xc4) : zero4;
#pragma unroll
      for (int k = 0; k < 4; ++k) XT[(4 * xc4 + k) * XS + xr] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int jb = wave + 4 * b;
      if (jb < D / 32) {
#pragma unroll
        for (int g = 0; g < RB / 8; ++g) {
          const int k = 8 * g + 4 * hh;
          const f32x4 a4 = *reinterpret_cast<const f32x4*>(XT + ln * XS + k);
          const float* bp = T + k * LH + jb * 32 + ln;
          const f32x4 b4 = f32x4{bp[0], bp[LH], bp[2 * LH], bp[3 * LH]};
#pragma unroll
          for (int q = 0; q < 4; ++q) accw[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[q], b4[q], accw[b], 0, 0, 0);
        }
      }
    }
  }

  float* wslab = p.dw_slabs + (int64_t)s * p.slab_stride;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int jb = wave + 4 * b;
    if (jb < D / 32) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) wslab[(int64_t)(i0 + tt::acc_row(reg, hh)) * D + jb * 32 + ln] = accw[b][reg];
    }
  }
  if (y != 0) return;                        // (uniform) db: the y = 0 workgroup of the slab
  __syncthreads();
  float* R = T;                              // [rpp][D] partial sums (<= 1024 floats)
  if (active) {
#pragma unroll
    for (int k = 0; k < 4; ++k) R[rr * D + 4 * c4 + k] = dba[k];
  }
  __syncthreads();
  for (int j = tid; j < D; j += 256) {
    float t = R[j];
    for (int k = 1; k < rpp; ++k) t = t + R[k * D + j];
    p.db_slabs[(int64_t)s * p.slab_stride + j] = t;
  }
}

__global__ __launch_bounds__(256) void cross_bwd_kernel(CrossBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int D = a.D;
  unsigned e = blockIdx.x;
  if (e < a.dw_blocks[0] + a.dw_blocks[1]) {
    const bool second = e >= a.dw_blocks[0];
    if (second) e -= a.dw_blocks[0];
    const tt_cross_bwd_args p = second ? a.p[1] : a.p[0];
    const unsigned nb = (unsigned)(D / RB);
    cross_dw_role(p, D, (int)(e / nb), (int)(e % nb), second ? a.rows_per_slab[1] : a.rows_per_slab[0], smem);
    return;
  }
  e -= a.dw_blocks[0] + a.dw_blocks[1];
  const bool second = e >= a.dx_blocks0;
  if (second) e -= a.dx_blocks0;
  const tt_cross_bwd_args p = second ? a.p[1] : a.p[0];
  cross_dx_role(p, D, (int64_t)e * RB, smem);
}

int check_common(const char* who, const void* probs, int32_t n_probs, int32_t D) {
  TT_REQUIRE(probs != nullptr, "%s: probs is NULL", who);
  TT_REQUIRE(n_probs >= 1 && n_probs <= 2, "%s: n_probs must be 1 or 2 (got %d)", who, n_probs);
  TT_REQUIRE(D >= 32 && D <= 256 && D % 32 == 0, "%s: D must be a multiple of 32 in 32..256 (got %d)", who, D);
  return TT_OK;
}

}  // namespace

extern "C" int32_t tt_cross_num_slabs(int64_t n) {
  if (n <= 0) return 1;
  const int64_t s = (n + 127) / 128;                     // 128-row slabs, at most 64 of them
  return (int32_t)(s < 64 ? s : 64);
}

extern "C" int tt_cross_fwd_f32(const tt_cross_fwd_args* probs, int32_t n_probs, int32_t D, tt_stream_t stream) {
  const char* who = "tt_cross_fwd_f32";
  if (int rc = check_common(who, probs, n_probs, D)) return rc;
  CrossFwdArgs a{};
  a.D = D;
  int64_t blocks[2] = {0, 0};
  for (int i = 0; i < n_probs; ++i) {
    const tt_cross_fwd_args& p = probs[i];
    TT_REQUIRE(p.n >= 0, "%s: problem %d: n must be >= 0", who, i);
    a.p[i] = p;
    if (p.n == 0) continue;
    TT_REQUIRE(p.x0 && p.x && p.w && p.b && p.y, "%s: problem %d: null pointer", who, i);
    TT_REQUIRE(tt::aligned16(p.x0) && tt::aligned16(p.x) && tt::aligned16(p.w) && tt::aligned16(p.b) && tt::aligned16(p.u_out) &&
               tt::aligned16(p.y), "%s: problem %d: x0, x, W, b, u_out and y must be 16-byte aligned", who, i);
    TT_REQUIRE(p.y != p.x && p.y != p.x0 && (p.u_out == nullptr || (p.u_out != p.x && p.u_out != p.x0 && p.u_out != p.y)),
               "%s: problem %d: y and u_out must not alias x, x0 or each other", who, i);
    blocks[i] = (p.n + RB - 1) / RB;
  }
  TT_REQUIRE(blocks[0] + blocks[1] <= 0x7fffffff, "%s: too many rows", who);
  if (blocks[0] + blocks[1] == 0) return TT_OK;
  a.blocks0 = (unsigned)blocks[0];
  const int lds = RB * (D + 4) * 4;
  tt::launch("cross_fwd", cross_fwd_kernel, dim3((unsigned)(blocks[0] + blocks[1])), dim3(256), (unsigned)lds, tt::as_stream(stream), a);
  return tt::check_launch(who);
}

extern "C" int tt_cross_bwd_f32(const tt_cross_bwd_args* probs, int32_t n_probs, int32_t D, tt_stream_t stream) {
  const char* who = "tt_cross_bwd_f32";
  if (int rc = check_common(who, probs, n_probs, D)) return rc;
  CrossBwdArgs a{};
  a.D = D;
  int64_t dxb[2] = {0, 0}, dwb[2] = {0, 0};
  bool any = false;
  for (int i = 0; i < n_probs; ++i) {
    const tt_cross_bwd_args& p = probs[i];
    TT_REQUIRE(p.n >= 0, "%s: problem %d: n must be >= 0", who, i);
    TT_REQUIRE(p.n_slabs >= 1 && p.n_slabs <= 65535, "%s: problem %d: n_slabs must be in 1..65535 (got %d)", who, i, p.n_slabs);
    a.p[i] = p;
    any = any || p.n > 0;
  }
  if (!any) return TT_OK;
  for (int i = 0; i < n_probs; ++i) {
    const tt_cross_bwd_args& p = probs[i];
    TT_REQUIRE(p.dw_slabs && p.db_slabs, "%s: problem %d: null pointer", who, i);
    TT_REQUIRE(p.n_slabs == 1 || p.slab_stride >= (int64_t)D * D, "%s: problem %d: slab_stride must be >= D * D", who, i);
    if (p.n > 0) {
      TT_REQUIRE(p.x0 && p.x && p.u && p.w && p.g && p.dx && (p.x_is_x0 || p.dx0), "%s: problem %d: null pointer", who, i);
      TT_REQUIRE(tt::aligned16(p.x0) && tt::aligned16(p.x) && tt::aligned16(p.u) && tt::aligned16(p.w) && tt::aligned16(p.g) &&
                 tt::aligned16(p.dx) && tt::aligned16(p.dx0), "%s: problem %d: x0, x, u, W, g, dx and dx0 must be 16-byte aligned", who, i);
      TT_REQUIRE(!p.x_is_x0 || p.x == p.x0, "%s: problem %d: x_is_x0 is set but x != x0", who, i);
      TT_REQUIRE(p.dx != p.g && p.dx != p.x0 && p.dx != p.x && p.dx != p.u,
                 "%s: problem %d: dx must not alias g, x0, x or u (the dW tiles read them while dx is written)", who, i);
      TT_REQUIRE(p.dx0 == nullptr || (p.dx0 != p.g && p.dx0 != p.x0 && p.dx0 != p.x && p.dx0 != p.u && p.dx0 != p.dx),
                 "%s: problem %d: dx0 must not alias g, x0, x, u or dx", who, i);
    }
    dxb[i] = (p.n + RB - 1) / RB;
    dwb[i] = (int64_t)p.n_slabs * (D / RB);
    a.rows_per_slab[i] = (p.n + p.n_slabs - 1) / p.n_slabs;
  }
  const int64_t total = dxb[0] + dxb[1] + dwb[0] + dwb[1];
  TT_REQUIRE(total <= 0x7fffffff, "%s: too many rows", who);
  a.dw_blocks[0] = (unsigned)dwb[0];
  a.dw_blocks[1] = (unsigned)dwb[1];
  a.dx_blocks0 = (unsigned)dxb[0];
  const int lds = (RB * (D + 4) + RB * XS) * 4;
  tt::launch("cross_bwd", cross_bwd_kernel, dim3((unsigned)total), dim3(256), (unsigned)lds, tt::as_stream(stream), a);
  return tt::check_launch(who);
}
