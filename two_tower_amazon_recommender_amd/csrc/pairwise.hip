// Pairwise retrieval losses over in-batch negatives (BPR / pairwise logistic, and the pairwise hinge / triplet loss): the
// scorer's data flow with another epilogue.  Logits are the softmax scorer's (log2 domain inside the kernels, as in score.hip):
//   s2_ij = c1 <q_i, c_j> + bias2_j   (c1 = log2e / T, bias2 = -log2 clip(p_j)),   x_ij = ln2 (s2_{i,pos(i)} - s2_ij),
//   phi(x) = softplus(-x) | max(0, margin - x),   h_ij = -phi'(x_ij) on the valid pairs (not the positive, not an accidental
//   hit, not below the row's hard-negative threshold), 0 elsewhere.
// All matrix products are exact f32 on v_mfma_f32_32x32x2_f32, k order 8g + 4*lanehalf + s as in gemm.hip / rating.hip.
//
// One kernel body serves both passes.  A workgroup (4 waves) owns 128 rows of the STATIONARY matrix - wave w the 32 rows
// 32w .., every lane its row's fragment in registers (D/2 floats) - and one of `nsplit` slices of the STREAMED matrix, which
// passes through a double-buffered [32][D + 4] LDS tile (next tile's global loads in flight during the MFMAs, one barrier per
// tile).  Per tile and wave:
//   GEMM1   X[t][r] = <streamed row t, stationary row r>      A = the tile, B = the wave's fragment: the stationary row is the
//                                                             accumulator's COLUMN (lane), the streamed row its register
//   epilogue in that layout: bias, masks, phi, h              the lane's own row terms in registers, the tile's in LDS
//   GEMM2   G[r][:] += sum_t h[t][r] * streamed row t         the accumulator is the A operand as it stands (k = the register's
//                                                             row for this lane half), B = the tile's rows from LDS
// pass 1 (stationary q): row sums of phi, of h and the pair count per split, and the split's  sum_j h_ij c_j  slab;
// combine: splits in ascending order -> n_i, r_i, per_row, w_i r_i, H_i w_i r_i and dq;
// pass 2 (stationary c): the same products and masks again (the same fma chains: bit-identical logits, so both passes take
// the same side of every comparison), h scaled by w_i r_i, slabs of  sum_i h_ij q_i ;
// reduce: splits in ascending order, minus H_i q_i on row i + diag_offset, scaled -> dc.  The loss is summed in a fixed order.
// No atomics, no [nq, nc] array anywhere (pass 2 recomputes the products: 8 nq nc D executed FLOPs), nothing read back.
#include "common.h"
#include <cmath>

namespace {

using tt::f32x4;
using tt::f32x16;

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr int kWaves = 4;
constexpr int kRowsPerWg = 32 * kWaves;

enum { KIND_LOGISTIC = TT_PAIRWISE_LOGISTIC, KIND_HINGE = TT_PAIRWISE_HINGE };

__device__ __forceinline__ f32x4 ldg4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

struct PairArgs {
  const float* R; const float* K;        // stationary [n_r, D], streamed [n_k, D]
  int64_t n_r, n_k, nq, nc, diag;        // diag: the positive of query i is candidate i + diag
  const float* pos2;                     // [nq] the positive's logit (log2 domain)
  const int64_t* ids;                    // [nc] candidate ids (null: no accidental-hit removal)
  const float* thr;                      // [nq] hard-negative thresholds, log2 domain (null: none)
  const float* bias2;                    // [nc] -log2 clip(p) (null: none)
  const float* wr;                       // [nq] w_i r_i (pass 2)
  float c1, margin;
  int64_t k_per_split;                   // streamed rows per split (a multiple of 32)
  float* part_phi; float* part_h; int32_t* part_n;     // [nsplit][nq] (pass 1)
  float* slab;                           // [nsplit][n_r][D] (null: no gradient)
};

// phi and -phi' at x.
template <int KIND>
__device__ __forceinline__ void pair_terms(float margin, float x, float& phi, float& h) {
  if constexpr (KIND == KIND_HINGE) {
    phi = fmaxf(margin - x, 0.f);
    h = x < margin ? 1.f : 0.f;
  } else {
    const float e = __expf(-fabsf(x));                 // in (0, 1]
    const float u = 1.f + e;
    // log1p(e): log(u) (v_log_f32: u is in [1, 2], no denormal range to handle) corrected by e / (u - 1) (u - 1 is exact),
    // e itself where 1 + e rounds to 1.  Reciprocals by v_rcp_f32 (1 ulp): an IEEE division's expansion would be most of
    // this epilogue's instructions.
    const float l1p = u == 1.f ? e : (__builtin_amdgcn_logf(u) * kLn2) * (e * __builtin_amdgcn_rcpf(u - 1.f));
    phi = fmaxf(-x, 0.f) + l1p;
    h = (x >= 0.f ? e : 1.f) * __builtin_amdgcn_rcpf(u);        // sigmoid(-x)
  }
}

template <int D, bool STAT_Q, bool GRAD, int KIND>
__global__ __launch_bounds__(kWaves * 64) void pair_pass_kernel(PairArgs a) {
  constexpr int LD = D + 4, NT = kWaves * 64, C4 = D / 4, PF = 32 * C4 / NT;     // PF: float4 loads per thread and tile
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* KT = smem;                                    // [2][32][LD]
  float* TF = smem + 2 * 32 * LD;                      // [2][3][32] the tile rows' float terms
  int64_t* TID = reinterpret_cast<int64_t*>(TF + 2 * 3 * 32);      // [2][32] their ids
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, ln = lane & 31;
  const int split = blockIdx.y;
  const int64_t row = (int64_t)blockIdx.x * kRowsPerWg + 32 * wave + ln;         // this lane's stationary row
  const bool row_ok = row < a.n_r;
  const bool has_ids = a.ids != nullptr;

  // (loads from a clamped, valid row and a select: no branch around a load, here and in request())
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 rf[D / 8];
  {
    const float* rp = a.R + (row_ok ? row : 0) * D + 4 * hh;
#pragma unroll
    for (int g = 0; g < D / 8; ++g) rf[g] = ldg4(rp + 8 * g);
    if (!row_ok) {
#pragma unroll
      for (int g = 0; g < D / 8; ++g) rf[g] = zero4;
    }
  }
  // the tile row that is this lane's pair on the diagonal: row + diag - k0 (stationary q), row - diag - k0 (stationary c)
  const int64_t dbase = STAT_Q ? row + a.diag : row - a.diag;
  // the lane's own row terms
  float l_pos = 0.f, l_thr = -INFINITY, l_bias = 0.f;
  int64_t l_id = 0;
  if (row_ok) {
    if constexpr (STAT_Q) {
      l_pos = a.pos2[row];
      if (a.thr != nullptr) l_thr = a.thr[row];
      if (has_ids) l_id = a.ids[row + a.diag];
    } else {
      if (a.bias2 != nullptr) l_bias = a.bias2[row];
      if (has_ids) l_id = a.ids[row];
    }
  }

  const int64_t kbeg = (int64_t)split * a.k_per_split;
  const int64_t kend = kbeg + a.k_per_split < a.n_k ? kbeg + a.k_per_split : a.n_k;

  f32x4 pf[PF];
  float t0 = 0.f, t1 = 0.f, t2 = 0.f;
  int64_t tidv = 0;
  auto request = [&](int64_t k0) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int f = tid + u * NT, r = f / C4, c4 = f - r * C4;
      const bool ok = k0 + r < a.n_k;
      const f32x4 v = ldg4(a.K + (ok ? k0 + r : 0) * D + 4 * c4);
      pf[u] = ok ? v : zero4;
    }
    if (tid < 32) {
      const int64_t k = k0 + tid;
      t0 = 0.f; t1 = -INFINITY; t2 = 0.f; tidv = 0;
      if (k < a.n_k) {
        if constexpr (STAT_Q) {
          if (a.bias2 != nullptr) t0 = a.bias2[k];
          if (has_ids) tidv = a.ids[k];
        } else {
          t0 = a.pos2[k];
          if (a.thr != nullptr) t1 = a.thr[k];
          t2 = a.wr[k];
          if (has_ids) tidv = a.ids[k + a.diag];
        }
      }
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int f = tid + u * NT, r = f / C4, c4 = f - r * C4;
      *reinterpret_cast<f32x4*>(KT + (buf * 32 + r) * LD + 4 * c4) = pf[u];
    }
    if (tid < 32) {
      TF[(buf * 3 + 0) * 32 + tid] = t0;
      TF[(buf * 3 + 1) * 32 + tid] = t1;
      TF[(buf * 3 + 2) * 32 + tid] = t2;
      TID[buf * 32 + tid] = tidv;
    }
  };

  f32x16 dacc[GRAD ? D / 32 : 1];
#pragma unroll
  for (int b = 0; b < (GRAD ? D / 32 : 1); ++b)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) dacc[b][reg] = 0.f;
  float s_phi = 0.f, s_h = 0.f;
  int s_n = 0;

  if (kbeg < kend) { request(kbeg); stage(0); }
  int buf = 0;
  for (int64_t k0 = kbeg; k0 < kend; k0 += 32, buf ^= 1) {
    __syncthreads();                 // this tile is staged; every wave is done with the other buffer
    const bool more = k0 + 32 < kend;
    if (more) request(k0 + 32);
    const float* kt = KT + buf * 32 * LD;
    f32x16 acc;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) acc[reg] = 0.f;
    // the tile's A fragments four k groups at a time, one round ahead of the 16 MFMAs that use them (the scheduling fences
    // keep the compiler from hoisting the whole tile's LDS reads: D / 2 registers, spills at dim 256)
    {
      f32x4 an[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) an[u] = *reinterpret_cast<const f32x4*>(kt + ln * LD + 8 * u + 4 * hh);
#pragma unroll
      for (int g0 = 0; g0 < D / 8; g0 += 4) {
        f32x4 ac[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) ac[u] = an[u];
        if (g0 + 4 < D / 8) {
#pragma unroll
          for (int u = 0; u < 4; ++u) an[u] = *reinterpret_cast<const f32x4*>(kt + ln * LD + 8 * (g0 + 4 + u) + 4 * hh);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[u][s], rf[g0 + u][s], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    const float* tf = TF + buf * 3 * 32;
    const int krem = kend - k0 < 32 ? (int)(kend - k0) : 32;          // tile rows inside the streamed matrix
    const int64_t dd = dbase - k0;
    const int dloc = (dd >= 0 && dd < 32) ? (int)dd : -1;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int tr = tt::acc_row(reg, hh);
      float pos, thr, bias, wr;
      int64_t idq, idc;
      if constexpr (STAT_Q) {
        pos = l_pos; thr = l_thr; idq = l_id; wr = 1.f;
        bias = tf[tr]; idc = TID[buf * 32 + tr];
      } else {
        bias = l_bias; idc = l_id;
        pos = tf[tr]; thr = tf[32 + tr]; wr = tf[64 + tr]; idq = TID[buf * 32 + tr];
      }
      const float s2 = __builtin_fmaf(acc[reg], a.c1, bias);
      const bool valid = row_ok && tr < krem && tr != dloc && !(has_ids && idq == idc) && !(s2 < thr);
      float phi, h;
      pair_terms<KIND>(a.margin, (pos - s2) * kLn2, phi, h);
      if (!valid) { phi = 0.f; h = 0.f; }
      if constexpr (STAT_Q) { s_phi = s_phi + phi; s_h = s_h + h; s_n += valid ? 1 : 0; }
      acc[reg] = h * wr;
      if ((reg & 3) == 3) __builtin_amdgcn_sched_barrier(0);       // four elements at a time
    }
    if constexpr (GRAD) {
      // RS accumulator registers (k steps) per round, their B values requested one round ahead
      constexpr int RS = D >= 128 ? 1 : 128 / D, NB = D / 32;
      float bn[RS * NB];
#pragma unroll
      for (int u = 0; u < RS; ++u)
#pragma unroll
        for (int b = 0; b < NB; ++b) bn[u * NB + b] = kt[tt::acc_row(u, hh) * LD + ln + 32 * b];
#pragma unroll
      for (int r0 = 0; r0 < 16; r0 += RS) {
        float bc[RS * NB];
#pragma unroll
        for (int e = 0; e < RS * NB; ++e) bc[e] = bn[e];
        if (r0 + RS < 16) {
#pragma unroll
          for (int u = 0; u < RS; ++u)
#pragma unroll
            for (int b = 0; b < NB; ++b) bn[u * NB + b] = kt[tt::acc_row(r0 + RS + u, hh) * LD + ln + 32 * b];
        }
#pragma unroll
        for (int u = 0; u < RS; ++u)
#pragma unroll
          for (int b = 0; b < NB; ++b)
            dacc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[r0 + u], bc[u * NB + b], dacc[b], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (more) stage(buf ^ 1);
  }

  if constexpr (STAT_Q) {
    // the two lane halves hold the same row's sums over different tile rows: half 0 first
    s_phi = s_phi + __shfl_xor(s_phi, 32, 64);
    s_h = s_h + __shfl_xor(s_h, 32, 64);
    s_n = s_n + __shfl_xor(s_n, 32, 64);
    if (hh == 0 && row_ok) {
      a.part_phi[(int64_t)split * a.nq + row] = s_phi;
      a.part_h[(int64_t)split * a.nq + row] = s_h;
      a.part_n[(int64_t)split * a.nq + row] = s_n;
    }
  }
  if constexpr (GRAD) {
    const int64_t r0 = (int64_t)blockIdx.x * kRowsPerWg + 32 * wave;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int64_t r = r0 + tt::acc_row(reg, hh);
      if (r < a.n_r) {
        float* dst = a.slab + ((int64_t)split * a.n_r + r) * D + ln;
#pragma unroll
        for (int b = 0; b < D / 32; ++b) dst[32 * b] = dacc[b][reg];
      }
    }
  }
}

// blocks [0, ceil(nq / 8)): pos2[i] = c1 <q_i, c_{i+diag}> + bias2_{i+diag}, 32 lanes per row;
// the blocks behind them (only with cand_prob): bias2[j] = -log2 clip(p_j, 1e-6, 1).
__global__ __launch_bounds__(256) void pair_prep_kernel(const f32x4* __restrict__ q, const f32x4* __restrict__ c,
                                                        const float* __restrict__ prob, int64_t nq, int64_t nc, int d4,
                                                        int64_t diag, float c1, int64_t pos_blocks, float* __restrict__ pos2,
                                                        float* __restrict__ bias2) {
  if ((int64_t)blockIdx.x >= pos_blocks) {
    const int64_t j = ((int64_t)blockIdx.x - pos_blocks) * 256 + threadIdx.x;
    if (j < nc) bias2[j] = -__log2f(fminf(fmaxf(prob[j], 1e-6f), 1.0f));
    return;
  }
  const int64_t row = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int lane = threadIdx.x & 31;
  if (row >= nq) return;
  const int64_t pc = row + diag;
  float acc = 0.f;
  for (int k = lane; k < d4; k += 32) {
    const f32x4 x = q[row * d4 + k], y = c[pc * d4 + k];
    acc = acc + (((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]) + x[3] * y[3]);
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
  if (lane == 0)
    pos2[row] = __builtin_fmaf(acc, c1, prob != nullptr ? -__log2f(fminf(fmaxf(prob[pc], 1e-6f), 1.0f)) : 0.f);
}

// Pass 1's splits, ascending: n_i, r_i, per_row, w_i r_i, H_i w_i r_i and (dq != null)
//   dq_i = scale * w_i r_i * (sum_s slab_s[i] - H_i c_{i+diag}).  d4 lanes per row (a power of two, 8 .. 64).
__global__ __launch_bounds__(256) void pair_combine_kernel(const float* __restrict__ part_phi, const float* __restrict__ part_h,
                                                           const int32_t* __restrict__ part_n, const float* __restrict__ w,
                                                           const f32x4* __restrict__ slab, const f32x4* __restrict__ cpos,
                                                           int64_t nq, int d4, int nsplit, int mean, float scale,
                                                           float* __restrict__ per_row, float* __restrict__ wr_out,
                                                           float* __restrict__ hw_out, f32x4* __restrict__ dq) {
  const int rpb = 256 / d4;
  const int64_t row = (int64_t)blockIdx.x * rpb + threadIdx.x / d4;
  const int col = threadIdx.x % d4;
  if (row >= nq) return;
  float phi = 0.f, hs = 0.f;
  int n = 0;
  for (int s = 0; s < nsplit; ++s) {
    phi = phi + part_phi[(int64_t)s * nq + row];
    hs = hs + part_h[(int64_t)s * nq + row];
    n += part_n[(int64_t)s * nq + row];
  }
  const float r = mean ? 1.0f / (float)(n > 1 ? n : 1) : 1.0f;
  const float wr = (w != nullptr ? w[row] : 1.0f) * r;
  if (col == 0) {
    per_row[row] = wr * phi;
    wr_out[row] = wr;
    hw_out[row] = hs * wr;
  }
  if (dq != nullptr) {
    f32x4 g = slab[row * d4 + col];
    for (int s = 1; s < nsplit; ++s) g = g + slab[((int64_t)s * nq + row) * d4 + col];
    const f32x4 cp = cpos[row * d4 + col];
    const float k = scale * wr;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = k * __builtin_fmaf(-hs, cp[e], g[e]);
    dq[row * d4 + col] = o;
  }
}

// dc_j = scale * (sum_s slab_s[j] - [0 <= j - diag < nq] (H w r)_{j-diag} q_{j-diag}), splits ascending (float4 per thread)
__global__ __launch_bounds__(256) void pair_reduce_dc_kernel(const f32x4* __restrict__ slab, const f32x4* __restrict__ q,
                                                             const float* __restrict__ hw, int64_t nq, int64_t nc, int d4,
                                                             int64_t diag, int nsplit, float scale, f32x4* __restrict__ dc) {
  const int64_t n4 = nc * d4;
  const int64_t i4 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i4 >= n4) return;
  f32x4 g = slab[i4];
  for (int s = 1; s < nsplit; ++s) g = g + slab[(int64_t)s * n4 + i4];
  const int64_t j = i4 / d4, i = j - diag;
  if (i >= 0 && i < nq) {
    const float h = hw[i];
    const f32x4 qv = q[i * d4 + (i4 - j * d4)];
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = __builtin_fmaf(-h, qv[e], g[e]);
  }
  dc[i4] = g * scale;
}

// loss = sum_r per_row[r] in a fixed order (one workgroup: 1024 strided partial sums, then a binary tree)
__global__ __launch_bounds__(1024) void pair_sum_rows_kernel(const float* __restrict__ per_row, int64_t n, float* __restrict__ loss) {
  __shared__ float red[1024];
  float acc = 0.f;
  for (int64_t r = threadIdx.x; r < n; r += 1024) acc = acc + per_row[r];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = red[0];
}

// ---- host side --------------------------------------------------------------------------------

int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// Splits of the streamed side: enough workgroups for two per CU (one at dim 256, whose registers leave room for one), at most
// n_k / dim of them - so a pass's slabs never exceed the 4 nq nc bytes the scorer keeps for its dot products - and at most 64.
int choose_nsplit(int64_t n_r, int64_t n_k, int dim) {
  const int64_t nrb = (n_r + kRowsPerWg - 1) / kRowsPerWg;
  const int64_t target = dim == 256 ? 256 : 512;
  int64_t ns = (target + nrb - 1) / nrb;
  if (ns > n_k / dim) ns = n_k / dim;
  if (ns > 64) ns = 64;
  return (int)(ns < 1 ? 1 : ns);
}

struct PairLayout {
  int ns_q, ns_c;
  int64_t off_bias, off_pos, off_wr, off_hw, off_phi, off_h, off_n, off_slab, total;
};

PairLayout pair_layout(int64_t nq, int64_t nc, int32_t dim) {
  PairLayout w{};
  w.ns_q = choose_nsplit(nq, nc, dim);
  w.ns_c = choose_nsplit(nc, nq, dim);
  int64_t o = 0;
  w.off_bias = o; o = align_up(o + nc * 4, 256);
  w.off_pos = o;  o = align_up(o + nq * 4, 256);
  w.off_wr = o;   o = align_up(o + nq * 4, 256);
  w.off_hw = o;   o = align_up(o + nq * 4, 256);
  w.off_phi = o;  o = align_up(o + (int64_t)w.ns_q * nq * 4, 256);
  w.off_h = o;    o = align_up(o + (int64_t)w.ns_q * nq * 4, 256);
  w.off_n = o;    o = align_up(o + (int64_t)w.ns_q * nq * 4, 256);
  w.off_slab = o;
  const int64_t slab_q = (int64_t)w.ns_q * nq * dim * 4, slab_c = (int64_t)w.ns_c * nc * dim * 4;
  o = align_up(o + (slab_q > slab_c ? slab_q : slab_c), 256);
  w.total = o;
  return w;
}

template <int D, bool STAT_Q, bool GRAD, int KIND>
int launch_pass(const char* fn, const PairArgs& a, int nsplit, hipStream_t stream) {
  const int64_t nrb = (a.n_r + kRowsPerWg - 1) / kRowsPerWg;
  if (nrb > 0x7fffffff) return tt::fail(TT_ERR_INVALID_ARG, "%s: too many rows", fn);
  const int lds = (2 * 32 * (D + 4) + 2 * 3 * 32) * 4 + 2 * 32 * 8;
  auto kern = pair_pass_kernel<D, STAT_Q, GRAD, KIND>;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
    return tt::fail(TT_ERR_LAUNCH, "%s: hipFuncSetAttribute(LDS %d) failed", fn, lds);
  tt::launch(STAT_Q ? "pairwise_q" : "pairwise_c", kern, dim3((unsigned)nrb, (unsigned)nsplit), dim3(kWaves * 64), (unsigned)lds,
             stream, a);
  return tt::check_launch(fn);
}

template <bool STAT_Q, bool GRAD, int KIND>
int dispatch_dim(const char* fn, int32_t dim, const PairArgs& a, int nsplit, hipStream_t stream) {
  switch (dim) {
    case 32: return launch_pass<32, STAT_Q, GRAD, KIND>(fn, a, nsplit, stream);
    case 64: return launch_pass<64, STAT_Q, GRAD, KIND>(fn, a, nsplit, stream);
    case 128: return launch_pass<128, STAT_Q, GRAD, KIND>(fn, a, nsplit, stream);
    default: return launch_pass<256, STAT_Q, GRAD, KIND>(fn, a, nsplit, stream);
  }
}

template <bool STAT_Q, bool GRAD>
int dispatch_pass(const char* fn, int kind, int32_t dim, const PairArgs& a, int nsplit, hipStream_t stream) {
  return kind == KIND_HINGE ? dispatch_dim<STAT_Q, GRAD, KIND_HINGE>(fn, dim, a, nsplit, stream)
                            : dispatch_dim<STAT_Q, GRAD, KIND_LOGISTIC>(fn, dim, a, nsplit, stream);
}

// Both entries: validation, then the launches.  dq == dc == null: the forward-only form (no GEMM2, no second pass).
int pairwise_run(const char* fn, bool grad, const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                 int64_t diag_offset, float inv_temperature, const float* sample_weight, const float* cand_prob,
                 const int64_t* cand_ids, const float* hard_thr, float grad_scale, void* workspace, int64_t workspace_bytes,
                 float* per_row, float* loss, float* dq, float* dc, int32_t kind, float margin, int32_t reduction,
                 tt_stream_t stream_) {
  TT_REQUIRE(q && c && workspace, "%s: null pointer", fn);
  TT_REQUIRE(nq > 0 && nc > 0, "%s: nq and nc must be positive", fn);
  TT_REQUIRE(diag_offset >= 0 && nq + diag_offset <= nc, "%s: need 0 <= diag_offset and nq + diag_offset <= nc", fn);
  TT_REQUIRE(dim == 32 || dim == 64 || dim == 128 || dim == 256, "%s: dim %d not in {32,64,128,256}", fn, dim);
  TT_REQUIRE(tt::aligned16(q) && tt::aligned16(c), "%s: q/c must be 16-byte aligned", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "%s: workspace must be 256-byte aligned", fn);
  TT_REQUIRE(kind == KIND_LOGISTIC || kind == KIND_HINGE, "%s: kind %d not in {0 (logistic), 1 (hinge)}", fn, kind);
  TT_REQUIRE(std::isfinite(margin), "%s: margin must be finite", fn);
  TT_REQUIRE(reduction == TT_PAIRWISE_MEAN || reduction == TT_PAIRWISE_SUM, "%s: reduction %d not in {0 (mean), 1 (sum)}", fn,
             reduction);
  const PairLayout w = pair_layout(nq, nc, dim);
  if (workspace_bytes < w.total)
    return tt::fail(TT_ERR_WORKSPACE, "%s: workspace %lld < %lld bytes", fn, (long long)workspace_bytes, (long long)w.total);
  TT_REQUIRE(per_row && loss && (!grad || (dq && dc)), "%s: null output pointer", fn);
  TT_REQUIRE(!grad || (tt::aligned16(dq) && tt::aligned16(dc)), "%s: dq/dc must be 16-byte aligned", fn);

  hipStream_t stream = tt::as_stream(stream_);
  char* ws = static_cast<char*>(workspace);
  float* bias2 = cand_prob != nullptr ? reinterpret_cast<float*>(ws + w.off_bias) : nullptr;
  float* pos2 = reinterpret_cast<float*>(ws + w.off_pos);
  float* wr = reinterpret_cast<float*>(ws + w.off_wr);
  float* hw = reinterpret_cast<float*>(ws + w.off_hw);
  float* slab = reinterpret_cast<float*>(ws + w.off_slab);
  const float c1 = kLog2e * inv_temperature;
  const int d4 = dim / 4;
  const int64_t n4 = nc * d4;
  TT_REQUIRE((n4 + 255) / 256 <= 0x7fffffff, "%s: too many rows", fn);
  int rc;
  {
    const int64_t pos_blocks = (nq + 7) / 8, bias_blocks = cand_prob != nullptr ? (nc + 255) / 256 : 0;
    TT_REQUIRE(pos_blocks + bias_blocks <= 0x7fffffff, "%s: too many rows", fn);
    tt::launch("pairwise_aux", pair_prep_kernel, dim3((unsigned)(pos_blocks + bias_blocks)), dim3(256), 0, stream,
               reinterpret_cast<const f32x4*>(q), reinterpret_cast<const f32x4*>(c), cand_prob, nq, nc, d4, diag_offset, c1,
               pos_blocks, pos2, bias2);
    if ((rc = tt::check_launch(fn)) != TT_OK) return rc;
  }
  PairArgs a{};
  a.nq = nq; a.nc = nc; a.diag = diag_offset;
  a.pos2 = pos2; a.ids = cand_ids; a.thr = hard_thr; a.bias2 = bias2; a.wr = wr;
  a.c1 = c1; a.margin = margin;
  a.R = q; a.K = c; a.n_r = nq; a.n_k = nc;
  a.k_per_split = align_up((nc + w.ns_q - 1) / w.ns_q, 32);
  a.part_phi = reinterpret_cast<float*>(ws + w.off_phi);
  a.part_h = reinterpret_cast<float*>(ws + w.off_h);
  a.part_n = reinterpret_cast<int32_t*>(ws + w.off_n);
  a.slab = grad ? slab : nullptr;
  rc = grad ? dispatch_pass<true, true>(fn, kind, dim, a, w.ns_q, stream) : dispatch_pass<true, false>(fn, kind, dim, a, w.ns_q, stream);
  if (rc != TT_OK) return rc;
  {
    const int rpb = 256 / d4;
    tt::launch("pairwise_aux", pair_combine_kernel, dim3((unsigned)((nq + rpb - 1) / rpb)), dim3(256), 0, stream, a.part_phi,
               a.part_h, a.part_n, sample_weight, reinterpret_cast<const f32x4*>(slab),
               reinterpret_cast<const f32x4*>(c + diag_offset * dim), nq, d4, w.ns_q, reduction == TT_PAIRWISE_MEAN ? 1 : 0,
               inv_temperature * grad_scale, per_row, wr, hw, grad ? reinterpret_cast<f32x4*>(dq) : nullptr);
    if ((rc = tt::check_launch(fn)) != TT_OK) return rc;
  }
  tt::launch("pairwise_aux", pair_sum_rows_kernel, dim3(1), dim3(1024), 0, stream, per_row, nq, loss);
  if ((rc = tt::check_launch(fn)) != TT_OK) return rc;
  if (!grad) return TT_OK;
  a.R = c; a.K = q; a.n_r = nc; a.n_k = nq;
  a.k_per_split = align_up((nq + w.ns_c - 1) / w.ns_c, 32);
  if ((rc = dispatch_pass<false, true>(fn, kind, dim, a, w.ns_c, stream)) != TT_OK) return rc;
  tt::launch("pairwise_aux", pair_reduce_dc_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream,
             reinterpret_cast<const f32x4*>(slab), reinterpret_cast<const f32x4*>(q), hw, nq, nc, d4, diag_offset, w.ns_c,
             inv_temperature * grad_scale, reinterpret_cast<f32x4*>(dc));
  return tt::check_launch(fn);
}

}  // namespace

extern "C" int64_t tt_retrieval_pairwise_workspace_bytes(int64_t nq, int64_t nc, int32_t dim) {
  if (nq <= 0 || nc <= 0 || dim <= 0) return 0;
  return pair_layout(nq, nc, dim).total;
}

extern "C" int tt_retrieval_pairwise_fwd_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                             int64_t diag_offset, float inv_temperature, const float* sample_weight,
                                             const float* cand_prob, const int64_t* cand_ids, const float* hard_thr,
                                             void* workspace, int64_t workspace_bytes, float* per_row, float* loss,
                                             int32_t kind, float margin, int32_t reduction, tt_stream_t stream) {
  return pairwise_run("tt_retrieval_pairwise_fwd_f32", false, q, c, nq, nc, dim, diag_offset, inv_temperature, sample_weight,
                      cand_prob, cand_ids, hard_thr, 1.0f, workspace, workspace_bytes, per_row, loss, nullptr, nullptr, kind,
                      margin, reduction, stream);
}

extern "C" int tt_retrieval_pairwise_fwd_bwd_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                                 int64_t diag_offset, float inv_temperature, const float* sample_weight,
                                                 const float* cand_prob, const int64_t* cand_ids, const float* hard_thr,
                                                 float grad_scale, void* workspace, int64_t workspace_bytes, float* per_row,
                                                 float* loss, float* dq, float* dc, int32_t kind, float margin,
                                                 int32_t reduction, tt_stream_t stream) {
  return pairwise_run("tt_retrieval_pairwise_fwd_bwd_f32", true, q, c, nq, nc, dim, diag_offset, inv_temperature,
                      sample_weight, cand_prob, cand_ids, hard_thr, grad_scale, workspace, workspace_bytes, per_row, loss, dq,
                      dc, kind, margin, reduction, stream);
}
