// Rating-prediction head (the tfrs.tasks.Ranking side of a joint retrieval + ranking model): one hidden ReLU layer over the
// pair's two tower outputs and a scalar output,
//   a = b1 + q W1[0:D] + c W1[D:2D],   h = max(a, 0),   pred = b2 + h . w2,
// and its backward pass for the MSE loss - two launches, both on the f32-input MFMA (v_mfma_f32_32x32x2_f32: exact f32
// products, the k order of gemm.hip / tower.hip inside a group of 8: k = 8g + 4*lanehalf + s).  x = [q ; c] is never
// materialised: the operand tiles are filled from q and c directly.
//
// Forward: a workgroup owns 32 pairs.  Their [32, 2D] operand tile sits in LDS (66 KB at D = 256), wave w owns the 32-column
// blocks w, w + 4, ... of h; W1 (512 KB at D = H = 256: no LDS home) is streamed from global memory, every lane loading its
// own B fragment (128-byte row segments per half wave, 16 loads in flight per lane).  Epilogue: bias, ReLU, h to HBM, and the
// lane's share of h . w2, reduced over the 32 columns by a fixed butterfly and over the waves through LDS in wave order.
//
// Backward: workgroup (s, y) owns slab s of the rows and the 32 columns [32y, 32y + 32) of x - a block of q or of c.  Per
// 32-row tile it rebuilds dh = g * w2 * (h > 0) in LDS while loading h (no [n, H] gradient in HBM), then
//   dx tile [32, 32] = dh [32, H] . W1[32y .. 32y+32, :]^T     the K = H products split over the four waves, their partial
//                                                               tiles summed through LDS in wave order;
//   dW1[32y .. 32y+32, :] += x block^T [32, 32 rows] . dh [32 rows, H]     wave w owns the column blocks w, w + 4 of H,
//                                                               accumulators live across the slab's tiles.
// The W1 block ([32, H], <= 33 KB) is staged in LDS once.  db1, dw2, db2 and the slab's sum of w e^2 are accumulated by
// the threads that load h (fixed column per thread) and reduced through LDS in ascending thread-row order by the y = 0
// workgroups.  Every dq / dc element belongs to one workgroup; no atomics anywhere: bits depend on (n, n_slabs, D, H) alone.
#include "common.h"

namespace {

using tt::f32x4;
using tt::f32x16;

constexpr int RB = 32;            // rows per tile
constexpr int XS = 36;            // row stride of the transposed x block in LDS
constexpr int PS = 33;            // row stride of a wave's partial dx tile in LDS

__device__ __forceinline__ f32x4 ldg4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct RatingFwdArgs {
  const float* q; const float* c; const float* w1; const float* b1; const float* w2; const float* b2;
  float* pred; float* h;
  int64_t n; int D, H;
};

__global__ __launch_bounds__(256) void rating_fwd_kernel(RatingFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int D = a.D, H = a.H, K = 2 * D, LX = K + 4;
  float* XT = smem;                          // [32][2D + 4]
  float* RED = smem + RB * LX;               // [4 waves][32 rows]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, ln = lane & 31;
  const int64_t m0 = (int64_t)blockIdx.x * RB;

  const int c4n = K / 4;
  for (int f = tid; f < RB * c4n; f += 256) {
    const int row = f / c4n, c4 = f - row * c4n;
    const int64_t r = m0 + row;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (r < a.n) v = 4 * c4 < D ? ldg4(a.q + r * D + 4 * c4) : ldg4(a.c + r * D + (4 * c4 - D));
    *reinterpret_cast<f32x4*>(XT + row * LX + 4 * c4) = v;
  }
  __syncthreads();

  float pp[16];
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) pp[reg] = 0.f;
  for (int jb = wave; jb < H / 32; jb += 4) {
    const int col = jb * 32 + ln;
    f32x16 acc;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[reg] = 0.f;
    const float* __restrict__ wp = a.w1 + col;
    // four k groups (16 W1 loads per lane) are requested one round ahead of the MFMAs that use them (K / 8 is a multiple of 8;
    // the last round requests the first groups again: in bounds, never used)
    f32x4 bn[4];
    auto request = [&](int g0) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float* bp = wp + (int64_t)(8 * (g0 + u) + 4 * hh) * H;
        bn[u] = f32x4{bp[0], bp[H], bp[2 * H], bp[3 * H]};
      }
    };
    request(0);
    for (int g0 = 0; g0 < K / 8; g0 += 4) {
      f32x4 a4[4], b4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        b4[u] = bn[u];
        a4[u] = *reinterpret_cast<const f32x4*>(XT + ln * LX + 8 * (g0 + u) + 4 * hh);
      }
      request(g0 + 4 < K / 8 ? g0 + 4 : 0);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u][s], b4[u][s], acc, 0, 0, 0);
    }
    const float bias = a.b1[col], w = a.w2[col];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int64_t r = m0 + tt::acc_row(reg, hh);
      const float v = fmaxf(acc[reg] + bias, 0.f);
      if (r < a.n) a.h[r * H + col] = v;
      pp[reg] = pp[reg] + v * w;
    }
  }
  // h . w2: the 32 columns of a half wave (xor butterfly: the same order in every lane), then the waves in order
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    float v = pp[reg];
    v = v + __shfl_xor(v, 16, 64);
    v = v + __shfl_xor(v, 8, 64);
    v = v + __shfl_xor(v, 4, 64);
    v = v + __shfl_xor(v, 2, 64);
    v = v + __shfl_xor(v, 1, 64);
    if (ln == 0) RED[wave * RB + tt::acc_row(reg, hh)] = v;
  }
  __syncthreads();
  if (tid < RB && m0 + tid < a.n)
    a.pred[m0 + tid] = (((RED[tid] + RED[RB + tid]) + RED[2 * RB + tid]) + RED[3 * RB + tid]) + a.b2[0];
}

struct RatingBwdArgs {
  const float* q; const float* c; const float* h; const float* pred; const float* rating; const float* sw;
  const float* w1; const float* w2;
  float* dq; float* dc; float* kslabs; float* bslabs; float* se;
  int64_t n, rows_per_slab;
  float grad_scale;
  int D, H, accumulate;
};

__global__ __launch_bounds__(256) void rating_bwd_kernel(RatingBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int D = a.D, H = a.H, LH = H + 4;
  float* WB = smem;                          // [32 columns of x][H + 4]: rows i0 .. i0 + 31 of W1
  float* DH = WB + RB * LH;                  // [32 rows][H + 4]: dh of the tile
  float* XT = DH + RB * LH;                  // [32 columns of x][36]: the x block of the tile, transposed
  float* PART = XT + RB * XS;                // [4 waves][32 rows][33]: partial dx tiles; the final reductions' scratch (4224 floats)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, ln = lane & 31;
  const int s = blockIdx.x, i0 = RB * blockIdx.y;
  const float* __restrict__ xsrc = i0 < D ? a.q + i0 : a.c + (i0 - D);
  float* __restrict__ dxdst = i0 < D ? a.dq + i0 : a.dc + (i0 - D);
  const int64_t row0 = (int64_t)s * a.rows_per_slab;
  const int64_t row1 = row0 + a.rows_per_slab < a.n ? row0 + a.rows_per_slab : a.n;      // (row1 <= row0: a slab without rows)
  const int64_t kstride = (int64_t)2 * D * H + H;

  const int c4n = H / 4;                     // float4 columns of h: 8 .. 64
  const int rpp = 256 / c4n;                 // rows of h the workgroup loads per pass (H = 96: 10, 240 threads at work)
  const int c4 = tid % c4n, rr = tid / c4n;
  const bool active = rr < rpp;
  for (int f = tid; f < RB * c4n; f += 256) {
    const int ii = f / c4n, cc = f - ii * c4n;
    *reinterpret_cast<f32x4*>(WB + ii * LH + 4 * cc) = ldg4(a.w1 + (int64_t)(i0 + ii) * H + 4 * cc);
  }
  const f32x4 w2v = active ? ldg4(a.w2 + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 db1a = zero4, dw2a = zero4;
  float db2a = 0.f, sea = 0.f;
  f32x16 accw[2];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) accw[b][reg] = 0.f;
  const int xr = tid >> 3, xc4 = tid & 7;    // the x block: 32 rows x 8 float4, one per thread

  for (int64_t t0 = row0; t0 < row1; t0 += RB) {
    __syncthreads();                         // the previous tile's LDS reads (and the W1 block's stores) are done
    if (active) {
      for (int r = rr; r < RB; r += rpp) {
        const int64_t row = t0 + r;
        float g = 0.f;
        f32x4 hv = zero4;
        if (row < row1) {
          const float rt = a.rating[row];
          if (finite_f32(rt)) {
            const float w = a.sw != nullptr ? a.sw[row] : 1.0f;
            const float e = a.pred[row] - rt;
            g = (a.grad_scale * w) * e;
            if (c4 == 0) { sea = sea + w * (e * e); db2a = db2a + g; }
          }
          hv = ldg4(a.h + row * H + 4 * c4);
        }
        f32x4 dh;
#pragma unroll
        for (int k = 0; k < 4; ++k) dh[k] = hv[k] > 0.f ? g * w2v[k] : 0.f;
        *reinterpret_cast<f32x4*>(DH + r * LH + 4 * c4) = dh;
        db1a = db1a + dh;
        dw2a = dw2a + hv * g;
      }
    }
    {
      const int64_t row = t0 + xr;
      const f32x4 v = row < row1 ? ldg4(xsrc + row * D + 4 * xc4) : zero4;
#pragma unroll
      for (int k = 0; k < 4; ++k) XT[(4 * xc4 + k) * XS + xr] = v[k];
    }
    __syncthreads();
    // dx tile: this wave's quarter of the K = H products
    {
      f32x16 accx;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) accx[reg] = 0.f;
      const int kq = wave * (H / 4);
      for (int g = 0; g < H / 32; ++g) {
        const int k = kq + 8 * g + 4 * hh;
        const f32x4 a4 = *reinterpret_cast<const f32x4*>(DH + ln * LH + k);
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(WB + ln * LH + k);
#pragma unroll
        for (int q = 0; q < 4; ++q) accx = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[q], b4[q], accx, 0, 0, 0);
      }
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) PART[(wave * RB + tt::acc_row(reg, hh)) * PS + ln] = accx[reg];
    }
    // dW1 rows i0 .. i0 + 31: += x block^T . dh over the tile's 32 rows, for the column blocks of H this wave owns
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int jb = wave + 4 * b;
      if (jb < H / 32) {
#pragma unroll
        for (int g = 0; g < RB / 8; ++g) {
          const int k = 8 * g + 4 * hh;
          const f32x4 a4 = *reinterpret_cast<const f32x4*>(XT + ln * XS + k);
          const float* bp = DH + k * LH + jb * 32 + ln;
          const f32x4 b4 = f32x4{bp[0], bp[LH], bp[2 * LH], bp[3 * LH]};
#pragma unroll
          for (int q = 0; q < 4; ++q) accw[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[q], b4[q], accw[b], 0, 0, 0);
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < RB * RB; e += 256) {
      const int r = e >> 5, ii = e & 31;
      const int64_t row = t0 + r;
      if (row < row1) {
        const float v = ((PART[r * PS + ii] + PART[(RB + r) * PS + ii]) + PART[(2 * RB + r) * PS + ii]) + PART[(3 * RB + r) * PS + ii];
        float* dst = dxdst + row * D + ii;
        *dst = a.accumulate ? *dst + v : v;
      }
    }
  }

  float* kslab = a.kslabs + (int64_t)s * kstride;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int jb = wave + 4 * b;
    if (jb < H / 32) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) kslab[(int64_t)(i0 + tt::acc_row(reg, hh)) * H + jb * 32 + ln] = accw[b][reg];
    }
  }
  if (blockIdx.y != 0) return;               // (uniform) db1, dw2, db2 and the squared error: the y = 0 workgroup of the slab
  __syncthreads();
  float* R1 = PART;                          // [rpp][H] db1 partials, then [rpp][H] dw2 partials (<= 2048 floats)
  float* R2 = PART + rpp * H;
  float* SC = PART + 4096;                   // [32] db2 partials, [32] squared-error partials
  if (active) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { R1[rr * H + 4 * c4 + k] = db1a[k]; R2[rr * H + 4 * c4 + k] = dw2a[k]; }
    if (c4 == 0) { SC[rr] = db2a; SC[32 + rr] = sea; }
  }
  __syncthreads();
  for (int j = tid; j < H; j += 256) {
    float t1 = R1[j], t2 = R2[j];
    for (int k = 1; k < rpp; ++k) { t1 = t1 + R1[k * H + j]; t2 = t2 + R2[k * H + j]; }
    a.bslabs[(int64_t)s * (H + 1) + j] = t1;
    kslab[(int64_t)2 * D * H + j] = t2;
  }
  if (tid == 0) {
    float t1 = SC[0], t2 = SC[32];
    for (int k = 1; k < rpp; ++k) { t1 = t1 + SC[k]; t2 = t2 + SC[32 + k]; }
    a.bslabs[(int64_t)s * (H + 1) + H] = t1;
    a.se[s] = t2;
  }
}

int check_shape(const char* who, int64_t n, int D, int H) {
  TT_REQUIRE(n >= 0, "%s: n must be >= 0", who);
  TT_REQUIRE(D == 32 || D == 64 || D == 128 || D == 256, "%s: D must be one of 32, 64, 128, 256 (got %d)", who, D);
  TT_REQUIRE(H >= 32 && H <= 256 && H % 32 == 0, "%s: H must be a multiple of 32 in 32..256 (got %d)", who, H);
  return TT_OK;
}

}  // namespace

extern "C" int32_t tt_rating_head_num_slabs(int64_t n) {
  if (n <= 0) return 1;
  const int64_t s = (n + 127) / 128;                     // 128-row slabs, at most 64 of them (8192 rows: 64 x 2D/32 workgroups)
  return (int32_t)(s < 64 ? s : 64);
}

extern "C" int tt_rating_head_fwd_f32(const float* q, const float* c, int64_t n, int32_t D, int32_t H, const float* w1,
                                      const float* b1, const float* w2, const float* b2, float* pred, float* h,
                                      tt_stream_t stream) {
  const char* who = "tt_rating_head_fwd_f32";
  if (int rc = check_shape(who, n, D, H)) return rc;
  if (n == 0) return TT_OK;
  TT_REQUIRE(q && c && w1 && b1 && w2 && b2 && pred && h, "%s: null pointer", who);
  TT_REQUIRE(tt::aligned16(q) && tt::aligned16(c) && tt::aligned16(w1) && tt::aligned16(w2) && tt::aligned16(h),
             "%s: q, c, W1, w2 and h must be 16-byte aligned", who);
  const int64_t blocks = (n + RB - 1) / RB;
  TT_REQUIRE(blocks <= 0x7fffffff, "%s: too many rows", who);
  const int lds = (RB * (2 * D + 4) + 4 * RB) * 4;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(rating_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
    return tt::fail(TT_ERR_LAUNCH, "%s: hipFuncSetAttribute(LDS %d) failed", who, lds);
  RatingFwdArgs a{q, c, w1, b1, w2, b2, pred, h, n, D, H};
  tt::launch("rating_fwd", rating_fwd_kernel, dim3((unsigned)blocks), dim3(256), (unsigned)lds, tt::as_stream(stream), a);
  return tt::check_launch(who);
}

extern "C" int tt_rating_head_bwd_f32(const float* q, const float* c, const float* h, const float* pred, const float* rating,
                                      const float* sample_weight, float grad_scale, int64_t n, int32_t D, int32_t H,
                                      const float* w1, const float* w2, float* dq, float* dc, int32_t accumulate,
                                      float* kslabs, float* bslabs, float* se_slabs, int32_t n_slabs, tt_stream_t stream) {
  const char* who = "tt_rating_head_bwd_f32";
  if (int rc = check_shape(who, n, D, H)) return rc;
  TT_REQUIRE(n_slabs >= 1 && n_slabs <= 65535, "%s: n_slabs must be in 1..65535 (got %d)", who, n_slabs);
  if (n == 0) return TT_OK;
  TT_REQUIRE(q && c && h && pred && rating && w1 && w2 && dq && dc && kslabs && bslabs && se_slabs, "%s: null pointer", who);
  TT_REQUIRE(tt::aligned16(q) && tt::aligned16(c) && tt::aligned16(h) && tt::aligned16(w1) && tt::aligned16(w2) &&
             tt::aligned16(dq) && tt::aligned16(dc), "%s: q, c, h, W1, w2, dq and dc must be 16-byte aligned", who);
  const int lds = (2 * RB * (H + 4) + RB * XS + 4 * RB * PS) * 4;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(rating_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
    return tt::fail(TT_ERR_LAUNCH, "%s: hipFuncSetAttribute(LDS %d) failed", who, lds);
  RatingBwdArgs a{q, c, h, pred, rating, sample_weight, w1, w2, dq, dc, kslabs, bslabs, se_slabs,
                  n, (n + n_slabs - 1) / n_slabs, grad_scale, D, H, accumulate != 0};
  tt::launch("rating_bwd", rating_bwd_kernel, dim3((unsigned)n_slabs, (unsigned)(2 * D / RB)), dim3(256), (unsigned)lds,
             tt::as_stream(stream), a);
  return tt::check_launch(who);
}
