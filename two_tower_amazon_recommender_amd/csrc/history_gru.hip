// GRU encoder of the user history (history_pooling = "gru"): Keras GRU(units = D, reset_after = True) with zero initial state
// and mask-aware stepping over the kept slots of a history bag, oldest slot first - the newest kept item is the last step.
//   a = x_t W + b_i            g = h U + b_r                          W, U [D, 3D] row-major, gate column blocks z | r | n
//   z = sigmoid(a_z + g_z)     r = sigmoid(a_r + g_r)     n = tanh(a_n + r * g_n)
//   h <- z * h + (1 - z) * n                                          a skipped slot leaves h untouched, bit for bit
// out[b] = base row + h_final (a bag without a kept slot: the base row itself).  Everything is f32; the products run on the
// f32-input MFMA (v_mfma_f32_32x32x2_f32, the k order of cross.hip); sigmoid is 1 / (1 + expf(-x)) and tanh is tanhf - the
// library's, which keep their relative accuracy at the small pre-activations of fresh tables.
//
// The launches of this file:
//   resolve   tokens, bag_rows, exclude -> batch_ids [n_bags * L] (-1: skipped) and the slot rows X [n_bags * L, D] (zeros
//             for a skipped slot); the rules and the out-of-range flag of the history bag launches.  A row gather: HBM-bound.
//   (A = X W + b_i over all slots is an ordinary GEMM: tt_dense_fwd_batched_f32.)
//   forward   a 256-thread workgroup owns 32 bags for all L steps.  The state tile sits in LDS ([32][D + 4], the A operand of the
//             MFMA) AND in registers in accumulator layout (lane = column, 16 rows per lane), wave w owning the 32-column blocks
//             w, w + 4 of every gate - so the gate math is lane-local: the three accumulators of a lane are the z, r and n
//             pre-activations of the same (row, column).  U is streamed from L2, every lane loading its own B fragment one round
//             ahead of the MFMAs (cross_fwd_kernel's structure).  A step in which no bag of the tile keeps its slot is skipped.
//             With the keep buffers it writes, per slot, h_{t-1} (hprev), the gate activations z | r | n (gates: may BE the A
//             buffer - every element is read and written by the same lane; a skipped slot keeps its projection there) and g_n
//             (gn; zero for a skipped slot): every kept buffer is written in full.
//   backward  the same tiling, slots in reverse from dh = dy.  Per kept slot
//               dn = dh (1 - z)   dz = dh (h_prev - n)   da_n = dn (1 - n^2)   da_z = dz z (1 - z)   da_r = da_n g_n r (1 - r)
//               dA = [da_z | da_r | da_n]     dG = [da_z | da_r | da_n r]     dh <- z dh + dG U^T
//             dh lives in registers in accumulator layout (z dh is the MFMA's starting accumulator); dG goes through a
//             [32][D + 4] LDS tile one gate at a time (three k passes over U's rows).  A skipped slot writes zero rows of dA and
//             dG and keeps dh.
//   (slot_grads = dA W^T, dW = X^T dA, db_i = sum dA, dU = hprev^T dG, db_r = sum dG are GEMMs: tt_dense_bwd_batched_f32.)
// No atomics (but the out-of-range flag), nothing read back, bits depend on the bag alone: not on the grid, not on its neighbours.
#include "common.h"

namespace {

using tt::f32x4;
using tt::f32x16;

constexpr int RB = 32;            // bags per workgroup
constexpr int MAXL = 64;

__device__ __forceinline__ f32x4 ldg4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

__device__ __forceinline__ float sigmoid_f32(float x) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-x))); }

// acc += T [32, K] (LDS, row stride LX) . B [K, 32 columns]: B row-major with leading dimension ldb, wp = &B[4 * hh][column]
__device__ __forceinline__ f32x16 tile_nn(const float* T, int LX, int K, const float* __restrict__ wp, int64_t ldb, int ln, int hh,
                                          f32x16 acc) {
  f32x4 bn[4];
  auto request = [&](int g0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float* bp = wp + (int64_t)(8 * (g0 + u)) * ldb;
      bn[u] = f32x4{bp[0], bp[ldb], bp[2 * ldb], bp[3 * ldb]};
    }
  };
  request(0);
  for (int g0 = 0; g0 < K / 8; g0 += 4) {    // (K / 8 is a multiple of 4; the last round requests the first groups again: unused)
    f32x4 a4[4], b4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      b4[u] = bn[u];
      a4[u] = *reinterpret_cast<const f32x4*>(T + ln * LX + 8 * (g0 + u) + 4 * hh);
    }
    request(g0 + 4 < K / 8 ? g0 + 4 : 0);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u][s], b4[u][s], acc, 0, 0, 0);
  }
  return acc;
}

// acc += T [32, K] . B^T: output column i takes the contiguous k run wp = &Bt[i][k0 + 4 * hh] (one 16-byte load per k group)
__device__ __forceinline__ f32x16 tile_nt(const float* T, int LX, int K, const float* __restrict__ wp, int ln, int hh, f32x16 acc) {
  f32x4 bn[4];
  auto request = [&](int g0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) bn[u] = ldg4(wp + 8 * (g0 + u));
  };
  request(0);
  for (int g0 = 0; g0 < K / 8; g0 += 4) {
    f32x4 a4[4], b4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      b4[u] = bn[u];
      a4[u] = *reinterpret_cast<const f32x4*>(T + ln * LX + 8 * (g0 + u) + 4 * hh);
    }
    request(g0 + 4 < K / 8 ? g0 + 4 : 0);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[u][s], b4[u][s], acc, 0, 0, 0);
  }
  return acc;
}

// the 16-row form of tile_nn on v_mfma_f32_16x16x4_f32: lane = (row or column ln = lane & 15, k quarter hh = lane >> 4), one MFMA
// takes k = k0 + 4 hh + s from its four quarters; wp = &B[4 * hh][column] as above
__device__ __forceinline__ f32x4 tile16_nn(const float* T, int LX, int K, const float* __restrict__ wp, int64_t ldb, int ln, int hh,
                                           f32x4 acc) {
  f32x4 bn;
  auto request = [&](int k0) {
    const float* bp = wp + (int64_t)k0 * ldb;
    bn = f32x4{bp[0], bp[ldb], bp[2 * ldb], bp[3 * ldb]};
  };
  request(0);
  for (int k0 = 0; k0 < K; k0 += 16) {
    const f32x4 b4 = bn;
    const f32x4 a4 = *reinterpret_cast<const f32x4*>(T + ln * LX + k0 + 4 * hh);
    request(k0 + 16 < K ? k0 + 16 : 0);
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[s], b4[s], acc, 0, 0, 0);
  }
  return acc;
}

template <int TR> struct TileAcc { using type = f32x16; };
template <> struct TileAcc<16> { using type = f32x4; };
// C/D row of accumulator register reg: the 32x32 layout of common.h, or 4 * (lane >> 4) + reg of the 16x16 one
template <int TR> __device__ __forceinline__ int tile_row(int reg, int hh) { return TR == 32 ? tt::acc_row(reg, hh) : 4 * hh + reg; }
template <int TR>
__device__ __forceinline__ typename TileAcc<TR>::type tile_nn_t(const float* T, int LX, int K, const float* __restrict__ wp, int64_t ldb,
                                                                int ln, int hh, typename TileAcc<TR>::type acc) {
  if constexpr (TR == 32) return tile_nn(T, LX, K, wp, ldb, ln, hh, acc);
  else return tile16_nn(T, LX, K, wp, ldb, ln, hh, acc);
}

#ifdef TT_GRU_TILE16
constexpr int kFwdTile = 16;
#else
constexpr int kFwdTile = 32;
#endif

// smask[t] bit r = bag b0 + r keeps slot t (threads 0 .. L-1 build it; the caller's barrier publishes it)
__device__ __forceinline__ void build_step_masks(uint32_t* smask, const int64_t* __restrict__ ids, int64_t b0, int64_t n_bags, int L,
                                                 int rows = RB) {
  const int t = threadIdx.x;
  if (t < L) {
    uint32_t m = 0;
    for (int r = 0; r < rows; ++r) {
      const int64_t b = b0 + r;
      if (b < n_bags && ids[b * L + t] >= 0) m |= 1u << r;
    }
    smask[t] = m;
  }
}

__global__ __launch_bounds__(256) void gru_resolve_kernel(const float* __restrict__ table_, int64_t table_rows, int dim4,
                                                          const int32_t* __restrict__ tokens, int64_t n_token_rows, int L,
                                                          const int64_t* __restrict__ bag_rows, int64_t n_bags,
                                                          const int64_t* __restrict__ exclude, float* __restrict__ X_,
                                                          int64_t* __restrict__ batch_ids, int32_t* __restrict__ oob_flag) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t s = idx / dim4;
  if (s >= n_bags * L) return;
  const int c = (int)(idx - s * dim4);
  const int64_t b = s / L;
  const int j = (int)(s - b * L);
  const bool first = c == 0;
  int64_t row = bag_rows != nullptr ? bag_rows[b] : b;
  if (row < 0 || row >= n_token_rows) {
    if (row != -1 && first && oob_flag != nullptr) atomicOr(oob_flag, 1);
    row = -1;
  }
  int32_t tok = -1;
  if (row >= 0) {
    tok = tokens[row * L + j];
    if (exclude != nullptr && (int64_t)tok == exclude[b]) tok = -1;    // the raw token, compared in int64: skipped like padding
    if (tok < 0 || (int64_t)tok >= table_rows) {
      if (tok != -1 && first && oob_flag != nullptr) atomicOr(oob_flag, 1);
      tok = -1;
    }
  }
  if (first && batch_ids != nullptr) batch_ids[s] = (int64_t)tok;
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (tok >= 0) v = reinterpret_cast<const f32x4*>(table_)[(int64_t)tok * dim4 + c];
  reinterpret_cast<f32x4*>(X_)[s * dim4 + c] = v;
}

// Dynamic LDS: the state tile [TR][D + 4] floats, then 64 step masks.  A and gates may be the same buffer (no __restrict__).
// TR = 32: v_mfma_f32_32x32x2_f32, 32-column blocks, wave w owns blocks w, w + 4 (the product).  TR = 16: v_mfma_f32_16x16x4_f32,
// 16-column blocks, wave w owns blocks w, w + 4, w + 8, w + 12 - twice the workgroups for the same bags (the -DTT_GRU_TILE16
// build: the A/B of profiles/history_gru.jsonl).
template <bool KEEP, int TR>
__global__ __launch_bounds__(256) void gru_fwd_kernel(const float* A, const int64_t* __restrict__ ids, int64_t n_bags, int L, int D,
                                                      const float* __restrict__ U, const float* __restrict__ br,
                                                      float* __restrict__ out, const float* __restrict__ base_table,
                                                      int64_t base_rows, const int64_t* __restrict__ base_ids,
                                                      int32_t* __restrict__ oob_flag, float* gates, float* __restrict__ gn,
                                                      float* __restrict__ hprev) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NREG = TR == 32 ? 16 : 4, NBI = TR == 32 ? 2 : 4, LB = TR == 32 ? 5 : 4;
  using acc_t = typename TileAcc<TR>::type;
  const int LX = D + 4, N3 = 3 * D, nb = D / TR;
  float* H = smem;
  uint32_t* smask = reinterpret_cast<uint32_t*>(smem + TR * LX);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> LB, ln = lane & (TR - 1);
  const int64_t b0 = (int64_t)blockIdx.x * TR;

  for (int f = tid; f < TR * LX; f += 256) H[f] = 0.0f;
  build_step_masks(smask, ids, b0, n_bags, L, TR);
  __syncthreads();

  float hreg[NBI][NREG];
#pragma unroll
  for (int bi = 0; bi < NBI; ++bi)
#pragma unroll
    for (int reg = 0; reg < NREG; ++reg) hreg[bi][reg] = 0.0f;
  uint32_t kept = 0;                                                 // bit r: bag b0 + r has a kept slot

  for (int t = 0; t < L; ++t) {
    const uint32_t m = smask[t];
    kept |= m;
    if constexpr (KEEP) {                                            // h_{t-1} of every slot, kept or not; g_n = 0 where skipped
#pragma unroll
      for (int bi = 0; bi < NBI; ++bi) {
        const int jb = wave + 4 * bi;
        if (jb < nb) {
#pragma unroll
          for (int reg = 0; reg < NREG; ++reg) {
            const int row = tile_row<TR>(reg, hh);
            const int64_t b = b0 + row;
            if (b < n_bags) {
              hprev[(b * L + t) * D + jb * TR + ln] = hreg[bi][reg];
              if (!((m >> row) & 1u)) gn[(b * L + t) * D + jb * TR + ln] = 0.0f;
            }
          }
        }
      }
    }
    if (m == 0) continue;                                            // (uniform) no bag of the tile keeps this slot
#pragma unroll
    for (int bi = 0; bi < NBI; ++bi) {
      const int jb = wave + 4 * bi;
      if (jb < nb) {
        const int col = jb * TR + ln;
        acc_t acc[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) {
#pragma unroll
          for (int reg = 0; reg < NREG; ++reg) acc[g][reg] = 0.f;
          acc[g] = tile_nn_t<TR>(H, LX, D, U + (int64_t)(4 * hh) * N3 + g * D + col, N3, ln, hh, acc[g]);
        }
        const float bz = br[col], brr = br[D + col], bnn = br[2 * D + col];
#pragma unroll
        for (int reg = 0; reg < NREG; ++reg) {
          const int row = tile_row<TR>(reg, hh);
          if ((m >> row) & 1u) {                                     // (a set bit implies b0 + row < n_bags)
            const int64_t s = (b0 + row) * L + t;
            const float az = A[s * N3 + col], ar = A[s * N3 + D + col], an = A[s * N3 + 2 * D + col];
            const float z = sigmoid_f32(__fadd_rn(az, __fadd_rn(acc[0][reg], bz)));
            const float r = sigmoid_f32(__fadd_rn(ar, __fadd_rn(acc[1][reg], brr)));
            const float g_n = __fadd_rn(acc[2][reg], bnn);
            const float n = tanhf(__fadd_rn(an, __fmul_rn(r, g_n)));
            const float h = hreg[bi][reg];
            hreg[bi][reg] = __fadd_rn(__fmul_rn(z, h), __fmul_rn(__fsub_rn(1.0f, z), n));
            if constexpr (KEEP) {
              gates[s * N3 + col] = z;
              gates[s * N3 + D + col] = r;
              gates[s * N3 + 2 * D + col] = n;
              gn[s * D + col] = g_n;
            }
          }
        }
      }
    }
    __syncthreads();                                                 // every wave has read the old state tile
#pragma unroll
    for (int bi = 0; bi < NBI; ++bi) {
      const int jb = wave + 4 * bi;
      if (jb < nb) {
#pragma unroll
        for (int reg = 0; reg < NREG; ++reg) H[tile_row<TR>(reg, hh) * LX + jb * TR + ln] = hreg[bi][reg];
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int bi = 0; bi < NBI; ++bi) {
    const int jb = wave + 4 * bi;
    if (jb < nb) {
      const int col = jb * TR + ln;
#pragma unroll
      for (int reg = 0; reg < NREG; ++reg) {
        const int row = tile_row<TR>(reg, hh);
        const int64_t b = b0 + row;
        if (b >= n_bags) continue;
        float v = hreg[bi][reg];                                     // no kept slot: +0
        if (base_table != nullptr) {
          const int64_t bid = base_ids[b];
          if (bid < 0 || bid >= base_rows) {
            if (bid != -1 && col == 0 && oob_flag != nullptr) atomicOr(oob_flag, 1);
          } else {
            const float o = base_table[bid * D + col];
            v = ((kept >> row) & 1u) ? __fadd_rn(o, v) : o;          // an emptied bag: the base row itself
          }
        }
        out[b * D + col] = v;
      }
    }
  }
}

// Dynamic LDS: one gate's dG tile [32][D + 4] floats, then 64 step masks.
__global__ __launch_bounds__(256) void gru_bwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ gates,
                                                      const float* __restrict__ gn, const float* __restrict__ hprev,
                                                      const float* __restrict__ dy, int64_t n_bags, int L, int D,
                                                      const float* __restrict__ U, float* __restrict__ dA, float* __restrict__ dG) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int LX = D + 4, N3 = 3 * D, nb = D / 32;
  float* T = smem;
  uint32_t* smask = reinterpret_cast<uint32_t*>(smem + RB * LX);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, ln = lane & 31;
  const int64_t b0 = (int64_t)blockIdx.x * RB;

  build_step_masks(smask, ids, b0, n_bags, L);
  float dh[2][16];
#pragma unroll
  for (int bi = 0; bi < 2; ++bi) {
    const int jb = wave + 4 * bi;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int64_t b = b0 + tt::acc_row(reg, hh);
      dh[bi][reg] = (jb < nb && b < n_bags) ? dy[b * D + jb * 32 + ln] : 0.0f;
    }
  }
  __syncthreads();

  for (int t = L - 1; t >= 0; --t) {
    const uint32_t m = smask[t];
    float dg[3][2][16];                                              // this slot's dG (dA's n gate goes straight to HBM)
    f32x16 acc[2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      const int jb = wave + 4 * bi;
      if (jb < nb) {
        const int col = jb * 32 + ln;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int row = tt::acc_row(reg, hh);
          const int64_t b = b0 + row;
          const int64_t s = b * L + t;
          float daz = 0.0f, dar = 0.0f, dan = 0.0f, dgn = 0.0f, a0 = dh[bi][reg];
          if ((m >> row) & 1u) {
            const float z = gates[s * N3 + col], r = gates[s * N3 + D + col], n = gates[s * N3 + 2 * D + col];
            const float g_n = gn[s * D + col], hp = hprev[s * D + col], d = dh[bi][reg];
            const float dn = __fmul_rn(d, __fsub_rn(1.0f, z));
            const float dz = __fmul_rn(d, __fsub_rn(hp, n));
            dan = __fmul_rn(dn, __fsub_rn(1.0f, __fmul_rn(n, n)));
            daz = __fmul_rn(dz, __fmul_rn(z, __fsub_rn(1.0f, z)));
            dar = __fmul_rn(__fmul_rn(dan, g_n), __fmul_rn(r, __fsub_rn(1.0f, r)));
            dgn = __fmul_rn(dan, r);
            a0 = __fmul_rn(z, d);
          }
          if (b < n_bags) {
            dA[s * N3 + col] = daz; dA[s * N3 + D + col] = dar; dA[s * N3 + 2 * D + col] = dan;
            dG[s * N3 + col] = daz; dG[s * N3 + D + col] = dar; dG[s * N3 + 2 * D + col] = dgn;
          }
          dg[0][bi][reg] = daz; dg[1][bi][reg] = dar; dg[2][bi][reg] = dgn;
          acc[bi][reg] = a0;
        }
      }
    }
    if (m == 0) continue;                                            // (uniform) zero rows written, dh carried
#pragma unroll
    for (int g = 0; g < 3; ++g) {
      __syncthreads();                                               // the previous pass's reads of the tile are done
#pragma unroll
      for (int bi = 0; bi < 2; ++bi) {
        const int jb = wave + 4 * bi;
        if (jb < nb) {
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) T[tt::acc_row(reg, hh) * LX + jb * 32 + ln] = dg[g][bi][reg];
        }
      }
      __syncthreads();
#pragma unroll
      for (int bi = 0; bi < 2; ++bi) {
        const int jb = wave + 4 * bi;
        if (jb < nb) acc[bi] = tile_nt(T, LX, D, U + (int64_t)(jb * 32 + ln) * N3 + g * D + 4 * hh, ln, hh, acc[bi]);
      }
    }
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      if (wave + 4 * bi < nb) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
          if ((m >> tt::acc_row(reg, hh)) & 1u) dh[bi][reg] = acc[bi][reg];      // a skipped slot: dh untouched
      }
    }
  }
}

int check_shape(const char* what, int32_t D, int32_t L, int64_t n_bags) {
  TT_REQUIRE(D >= 32 && D <= 256 && D % 32 == 0, "%s: D must be a multiple of 32 in 32..256 (got %d)", what, D);
  TT_REQUIRE(L >= 1 && L <= MAXL, "%s: L must be in 1..64 (got %d)", what, L);
  TT_REQUIRE(n_bags >= 0, "%s: n_bags must be >= 0", what);
  TT_REQUIRE(n_bags <= 0x7fffffff / (int64_t)L, "%s: n_bags * L must fit 31 bits (the sort plan's positions are int32)", what);
  return TT_OK;
}

unsigned tile_lds_bytes(int D) { return (unsigned)((RB * (D + 4) + MAXL) * sizeof(float)); }

}  // namespace

extern "C" int tt_history_gru_resolve_f32(const float* table, int64_t table_rows, int32_t dim, const int32_t* tokens,
                                          int64_t n_token_rows, int32_t L, const int64_t* bag_rows, int64_t n_bags,
                                          const int64_t* exclude, float* x, int64_t* batch_ids, int32_t* oob_flag,
                                          tt_stream_t stream) {
  const char* what = "tt_history_gru_resolve_f32";
  if (int rc = check_shape(what, dim, L, n_bags)) return rc;
  TT_REQUIRE(table_rows > 0 && n_token_rows >= 0, "%s: need table_rows > 0 and n_token_rows >= 0", what);
  TT_REQUIRE(bag_rows != nullptr || n_bags == n_token_rows,
             "%s: bag_rows is NULL (identity), so n_bags (%lld) must equal n_token_rows (%lld)", what, (long long)n_bags,
             (long long)n_token_rows);
  if (n_bags == 0) return TT_OK;
  TT_REQUIRE(table && x && (tokens || n_token_rows == 0), "%s: null pointer (table / x / tokens)", what);
  TT_REQUIRE(tt::aligned16(table) && tt::aligned16(x), "%s: table and x must be 16-byte aligned", what);
  const int dim4 = dim / 4;
  const int64_t blocks = (n_bags * L * dim4 + 255) / 256;
  TT_REQUIRE(blocks <= 0x7fffffff, "%s: too many slots", what);
  tt::launch("history_gru_resolve", gru_resolve_kernel, dim3((unsigned)blocks), dim3(256), 0, tt::as_stream(stream), table, table_rows,
             dim4, tokens, n_token_rows, (int)L, bag_rows, n_bags, exclude, x, batch_ids, oob_flag);
  return tt::check_launch(what);
}

extern "C" int tt_history_gru_fwd_f32(const float* a, const int64_t* batch_ids, int64_t n_bags, int32_t L, int32_t dim,
                                      const float* u, const float* b_r, float* out, const float* base_table, int64_t base_rows,
                                      const int64_t* base_ids, int32_t* oob_flag, float* gates, float* gn, float* hprev,
                                      tt_stream_t stream) {
  const char* what = "tt_history_gru_fwd_f32";
  if (int rc = check_shape(what, dim, L, n_bags)) return rc;
  TT_REQUIRE((base_table != nullptr) == (base_ids != nullptr), "%s: base_table and base_ids go together (both NULL or both given)", what);
  TT_REQUIRE(base_table == nullptr || base_rows > 0, "%s: need base_rows > 0 with a base", what);
  const bool keep = gates != nullptr;
  TT_REQUIRE((gn != nullptr) == keep && (hprev != nullptr) == keep, "%s: gates, gn and hprev go together (all NULL or all given)", what);
  if (n_bags == 0) return TT_OK;
  TT_REQUIRE(a && batch_ids && u && b_r && out, "%s: null pointer (a / batch_ids / u / b_r / out)", what);
  TT_REQUIRE(tt::aligned16(a) && tt::aligned16(u) && tt::aligned16(out), "%s: a, u and out must be 16-byte aligned", what);
  TT_REQUIRE(out != a && (!keep || (out != gates && out != gn && out != hprev && gn != a && hprev != a && gn != hprev && gates != gn &&
                                    gates != hprev)),
             "%s: out, gn and hprev must not alias a, gates or each other (gates alone may be a)", what);
  const int64_t blocks = (n_bags + kFwdTile - 1) / kFwdTile;
  const dim3 grid((unsigned)blocks), block(256);
  const unsigned lds = (unsigned)((kFwdTile * (dim + 4) + MAXL) * sizeof(float));
  hipStream_t s = tt::as_stream(stream);
  if (keep) {
    tt::launch("history_gru_fwd", gru_fwd_kernel<true, kFwdTile>, grid, block, lds, s, a, batch_ids, n_bags, (int)L, (int)dim, u, b_r, out,
               base_table, base_rows, base_ids, oob_flag, gates, gn, hprev);
  } else {
    tt::launch("history_gru_fwd", gru_fwd_kernel<false, kFwdTile>, grid, block, lds, s, a, batch_ids, n_bags, (int)L, (int)dim, u, b_r, out,
               base_table, base_rows, base_ids, oob_flag, gates, gn, hprev);
  }
  return tt::check_launch(what);
}

extern "C" int tt_history_gru_bwd_f32(const int64_t* batch_ids, const float* gates, const float* gn, const float* hprev,
                                      const float* dy, int64_t n_bags, int32_t L, int32_t dim, const float* u, float* da, float* dg,
                                      tt_stream_t stream) {
  const char* what = "tt_history_gru_bwd_f32";
  if (int rc = check_shape(what, dim, L, n_bags)) return rc;
  if (n_bags == 0) return TT_OK;
  TT_REQUIRE(batch_ids && gates && gn && hprev && dy && u && da && dg,
             "%s: null pointer (batch_ids / gates / gn / hprev / dy / u / da / dg)", what);
  TT_REQUIRE(tt::aligned16(u) && tt::aligned16(da) && tt::aligned16(dg), "%s: u, da and dg must be 16-byte aligned", what);
  TT_REQUIRE(da != dg && da != gates && dg != gates && da != gn && dg != gn && da != hprev && dg != hprev && da != dy && dg != dy,
             "%s: da and dg must not alias each other or an input", what);
  const int64_t blocks = (n_bags + RB - 1) / RB;
  tt::launch("history_gru_bwd", gru_bwd_kernel, dim3((unsigned)blocks), dim3(256), tile_lds_bytes(dim), tt::as_stream(stream), batch_ids,
             gates, gn, hprev, dy, n_bags, (int)L, (int)dim, u, da, dg);
  return tt::check_launch(what);
}
