// K4 / K5 — batched dot-product scorer fused with the in-batch sampled-softmax loss and its
// gradient (SURVEY.md §2.2 K4/K5, §8a a3+a4; tfrs.tasks.Retrieval semantics, Appendix A).
// Probabilities / coefficients never reach HBM.  The exact-f32 TRAINING entry keeps the raw dot products [nq][nc] in the
// workspace between its two passes (MODE_FUSED_S writes, MODE_BWD_S reads: pass 2 skips GEMM1); every other entry keeps nothing.
//
// One kernel serves the forward statistics pass and both gradient passes.  It sees a STATIONARY
// matrix R [n_r, D] (one 32-row fragment per wave, held in registers for the whole launch) and a
// STREAMED matrix K [n_c, D] (32-row tiles, double-buffered in LDS, shared by the 4 waves):
//
//   GEMM1   X[c][r]  = sum_d K[c][d] * R[r][d]          v_mfma_f32_32x32x2_f32, D/2 per tile
//           (c on accumulator registers, r on lanes: every softmax reduction over c is lane-local)
//   FWD     online (max, sum-exp2) over c per lane; positive logit captured in-tile
//   BWD     coef[c][r] = exp2(X*c1 + a_c + a_r) * s_c*s_r  - [c == r+diag] s_c*s_r
//   GEMM2   G^T[d][r] += sum_c K[c][d] * coef[c][r]      the accumulator IS the B operand (no LDS
//           transpose): lane half h of register `reg` holds row acc_row(reg,h) = k of that step.
//
//   pass        R        K        a_r          s_r        a_c          s_c        diag
//   FWD  (lse)  q        c        -            -          -log2 p_c    -          +off
//   BWD dq      q        c        -lse2        w/T*g      -log2 p_c    1          +off
//   BWD dc      c        q        -log2 p_r    1          -lse2        w/T*g      -off
//
// f32-input MFMA: exact f32 products (guide §3 'FP32-input MFMA'); peak 157.3 TF on MI355X.
// Per (32 r x 32 c) tile and wave: D/2 + D/2 MFMAs (BWD), 16 v_exp_f32 per lane, 16+16(+8) LDS reads.
// The c range is split over the grid (blockIdx % nsplit; blocks b and b+8 share an XCD, so one
// XCD's L2 keeps re-serving the same K range); partial results go to per-split slabs that a small
// kernel sums in split order (bitwise reproducible; no float atomics).
#include "common.h"

namespace {

using tt::f32x4;
using tt::f32x16;
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr float kLog2e = 1.44269504088896340736f;
constexpr float kLn2 = 0.69314718055994530942f;
constexpr float kNegBig = -1.0e30f;   // log2-domain stand-in for -inf (tfrs uses finfo.min/100)

// MODE_FUSED_S: MODE_FUSED that also writes the raw dot products X[q][c] to ScoreArgs::S; MODE_BWD_S: MODE_BWD that reads
// them back instead of recomputing GEMM1 (the training entry's pass 2: half the matrix-pipe work)
enum { MODE_FWD = 0, MODE_BWD = 1, MODE_FUSED = 2, MODE_RANK = 3, MODE_FUSED_S = 4, MODE_BWD_S = 5,
       // The plain train step's pair (no sampling probability, ids or hard negatives), chosen on the host in launch_score:
       // MODE_FUSED_S_NC = MODE_FUSED_S without a column bias (a_c == nullptr), MODE_BWD_S_NR = MODE_BWD_S without a row bias or row
       // scale (a_r == s_r == nullptr; a_c and s_c given).  Same passes, same arithmetic on every live value; see FAST in score_kernel.
       MODE_FUSED_S_NC = 6, MODE_BWD_S_NR = 7,
       // MODE_BWD_S_NR at D <= 128 keeps a_c / s_c of ALL the split's streamed rows in LDS, staged once per workgroup (kRowTermRows);
       // MODE_BWD_S_NR_T is the same kernel staging them per tile beside the tile, for splits longer than that array
       MODE_BWD_S_NR_T = 8,
       // MODE_FUSED_S_NC with the column splits INSIDE the workgroup (dim 128, 8 splits): all 8 waves hold the same 32-row fragment,
       // wave w runs split w on a private LDS tile, the 8 partial results meet in LDS and the kernel finishes lse, per-row loss, the
       // dc pass's row terms and dq itself - no slab, no part_m / part_l, no combine launch (score_rowfrag_kernel)
       MODE_FUSED_S_WG = 9,
       // MODE_BWD_S_NR_T with the query splits INSIDE the workgroup (dim 128, 8 splits of whole tiles): all 8 waves own the same
       // 32-candidate fragment, wave w runs split w on a private LDS tile, the 8 partial dc blocks are summed in LDS in split order
       // and one workgroup sums the per-row losses - no slab, no reduce_slabs_kernel launch (score_colfrag_kernel)
       MODE_BWD_S_WG = 10 };
constexpr int base_mode(int m) {
  return (m == MODE_FUSED_S_NC || m == MODE_FUSED_S_WG)
             ? (int)MODE_FUSED_S
             : ((m == MODE_BWD_S_NR || m == MODE_BWD_S_NR_T || m == MODE_BWD_S_WG) ? (int)MODE_BWD_S : m);
}
constexpr int kRowTermRows = 4096;        // streamed rows per split whose two row terms the LDS array holds (32 KB)
template <int D, int MODE_T> constexpr bool row_terms_in_lds() { return MODE_T == MODE_BWD_S_NR && D <= 128; }
template <bool B> struct BoolC { static constexpr bool value = B; };     // compile-time flag of a generic lambda
// FAST forms: a wave-uniform per-tile base pointer, pinned to an SGPR pair (an empty statement, no instruction).  The compiler
// may no longer fold the thread's loop-invariant offset into the base - that fold made every per-tile base a 64-bit VECTOR
// induction pointer (v_lshl_add_u64, v_add_co / v_addc per tile) - so the base advances on the scalar unit and the load takes it
// as `saddr` beside one loop-invariant 32-bit VGPR offset.  (The result is typed as a global-memory pointer: behind the statement the
// compiler no longer sees that the address came from a kernel argument, and a generic pointer would make the access a flat one.)
template <class T> using global_ptr = __attribute__((address_space(1))) T*;
template <class T> __device__ __forceinline__ global_ptr<T> uniform_base(T* p) {
  asm("" : "+s"(p));
  return (global_ptr<T>)p;
}
constexpr float kRescaleThr = 8.0f;   // FUSED: rescale the accumulators only when a row max grows by > 2^8 (p stays <= 256)

struct ScoreArgs {
  const float* R;
  const float* K;
  int64_t n_r, n_c;
  int64_t diag;             // positive pair: c == r + diag
  float c1;                 // log2(e) / temperature
  const float* a_r;         // [n_r] additive, log2 domain (nullable = 0)
  const float* s_r;         // [n_r] multiplicative (nullable = 1)
  const float* a_c;         // [n_c]
  const float* s_c;         // [n_c]
  const int64_t* id_r;      // accidental-hit ids (HAS_IDS only)
  const int64_t* id_c;
  int nsplit;
  int64_t c_per_split;      // multiple of 32
  float* part_m;            // FWD [nsplit][n_r]
  float* part_l;            // FWD [nsplit][n_r]
  float* pos2;              // FWD [n_r] positive logit (log2 domain)
  float* slab;              // BWD [nsplit][n_r][D]
  const float* h_r;         // optional [n_r]: hard-negative threshold per row   (element kept iff t >= h or positive)
  const float* h_c;         // optional [n_c]: hard-negative threshold per column (same domain as the masked value t)
  const int64_t* pos_idx;   // optional [n_r]: explicit positive column per row (else r + diag)
  int32_t* part_cnt;        // RANK [nsplit][n_r]: columns scoring strictly above the row's threshold a_r
  float* S;                 // FUSED_S (out) / BWD_S (in): raw dot products in 32 x 32 blocks (see store_S)
  int64_t ldS;              // number of query tiles = ceil(nq / 32)
  // MODE_FUSED_S_WG only: what fused_combine_kernel takes beside the per-split results, and its five outputs
  const float* w;           // optional [n_r] sample weight
  float scale;              // inv_temperature * grad_scale
  float* lse;               // [n_r]
  float* per_row;           // [n_r]
  float* aq;                // [n_r] -lse2: the dc pass's row bias
  float* sq;                // [n_r] w * scale: the dc pass's row scale
  float* dq;                // [n_r][D]
  // MODE_BWD_S_WG only: the gradient of the stationary side, and the scalar loss = sum(per_row[0 .. n_c)) its first workgroup writes
  float* dr;                // [n_r][D]
  float* loss;              // [1]
};

// The pass-1 combine for one (row, float4 column): the per-split (max, sum, G) of a row -> lse, per-row loss, the dc pass's row
// terms and dq[r] = (w_r/T*g) * ( sum_s G_s[r]*2^(m_s-M) / L  -  c[r+diag] ).  ONE body for fused_combine_kernel (the per-split
// results come from HBM) and for the epilogue of MODE_FUSED_S_WG (they come from LDS), so the two agree bit for bit by
// construction: M by fmaxf in split order, L += l_s * 2^(m_s - M) in split order, acc += G_s * 2^(m_s - M) in split order, 1 / L,
// (acc / L - c_pos) * s_r.  pm_of / pl_of / g_of(s): the statistics and the G float4 of split s, 0 <= s < nsplit.  Splits are taken
// 8 at a time, every chunk's reads issued together from clamped (valid) split indices; the G reads of the first 8 splits do not
// depend on the row statistics and are issued first, the (max, sum) passes run underneath them.
// row_lane0: this lane writes the row's four scalars; dq_out: this lane's float4 of dq (null: none).
template <class PM, class PL, class GS>
__device__ __forceinline__ void combine_row(int nsplit, PM pm_of, PL pl_of, GS g_of, f32x4 cp, float p2, float wr, float scale,
                                            bool row_lane0, float* lse, float* per_row, float* aq, float* sq, f32x4* dq_out) {
  constexpr int U = 8;
  const int last = nsplit - 1;
  f32x4 v0[U];
#pragma unroll
  for (int u = 0; u < U; ++u) v0[u] = g_of(u < last ? u : last);
  float pm0[U];                                      // the first chunk's maxima stay in registers for the sum below
  float M = kNegBig;
  for (int s0 = 0; s0 < nsplit; s0 += U) {
    float pm[U];
#pragma unroll
    for (int u = 0; u < U; ++u) pm[u] = pm_of(s0 + u < last ? s0 + u : last);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      M = fmaxf(M, pm[u]);                           // (a clamped duplicate of the last split changes no maximum)
      if (s0 == 0) pm0[u] = pm[u];
    }
  }
  float L = 0.f;
  for (int s0 = 0; s0 < nsplit; s0 += U) {
    float pm[U], pl[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int s = s0 + u < last ? s0 + u : last;
      pm[u] = pm_of(s);
      pl[u] = pl_of(s);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (s0 + u < nsplit) L += pl[u] * __builtin_amdgcn_exp2f(pm[u] - M);
  }
  const float lse2 = M + __log2f(L);
  const float sr = wr * scale;
  if (row_lane0) {
    *lse = lse2 * kLn2;
    *per_row = (lse2 - p2) * kLn2 * wr;
    *aq = -lse2;
    *sq = sr;
  }
  const float inv_l = 1.0f / L;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (u < nsplit) acc += v0[u] * __builtin_amdgcn_exp2f(pm0[u] - M);
  for (int s0 = U; s0 < nsplit; s0 += U) {           // splits beyond the first 8, in order, 8 reads at a time
    f32x4 v[U];
    float pm[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int s = s0 + u < last ? s0 + u : last;
      v[u] = g_of(s);
      pm[u] = pm_of(s);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (s0 + u < nsplit) acc += v[u] * __builtin_amdgcn_exp2f(pm[u] - M);
  }
  if (dq_out != nullptr) *dq_out = (acc * inv_l - cp) * sr;
}

// PREC = 0: exact f32 products (v_mfma_f32_32x32x2_f32).  PREC = 1: "bf16x3" — every f32 operand is split into three
// bf16 pieces (hi + mid + lo, the two residuals exact in f32) and the products run on v_mfma_f32_32x32x16_bf16 with f32
// accumulation: GEMM1 (the logits) keeps the 6 products down to 2^-24 relative (hi*hi, hi*mid, mid*hi, hi*lo, lo*hi,
// mid*mid), GEMM2 (the gradient sums, judged at 1e-4 of their maximum) the 3 down to 2^-16 (hi*hi, hi*mid, mid*hi).
// 72 bf16 MFMAs of 32 cycles per 32x32 tile and wave instead of 128 f32 MFMAs of 64: 0.28x the matrix-pipe time.
template <int D, int PREC>
struct Geo {
  static constexpr int LS = D + 4;             // f32: LDS row stride (floats): bank-conflict-free b128 reads
  static constexpr int NG = D / 8;             // f32 GEMM1 k-groups of 8 (4 per lane half)
  static constexpr int NB = D / 32;            // GEMM2 d-blocks (f32: d = NB*lane_row + b; bf16x3: d = 32*b + acc row)
  static constexpr int KS = D / 16;            // bf16x3 GEMM1 k-steps
  static constexpr int HALF_B = 32 * 256;      // bf16x3: bytes of one [32 rows][128 cols] bf16 sub-image
  static constexpr int PIECE_B = (D / 128) * HALF_B;
  static constexpr int TILE_F = PREC == 0 ? 32 * LS : 3 * PIECE_B / 4;
  static constexpr int BUF_F = TILE_F + 160;   // + a_c[32] + s_c[32] + id_c[32] (int64) + h_c[32]
  static constexpr int LDS_BYTES = 2 * BUF_F * 4;      // 4-wave schedule: 2 buffers
};

// x = hi + mid + lo, each a bf16 (round to nearest even); x - hi and (x - hi) - mid are exact in f32
struct Bf3 {
  __bf16 hi, mid, lo;
};
__device__ __forceinline__ Bf3 split3(float x) {
  Bf3 o;
  o.hi = (__bf16)x;
  const float r1 = x - (float)o.hi;
  o.mid = (__bf16)r1;
  o.lo = (__bf16)(r1 - (float)o.mid);
  return o;
}

// Byte offset of 16-byte chunk `ch` (8 bf16) of row `row` in a [32][128] bf16 sub-image with plain 256-byte rows and
// the chunk index XOR-swizzled by the row (cdna_hip_programming.md T10, image (b)): conflict-free both for the row
// reads (ds_read_b128, GEMM1's A operand) and for the transposing reads (ds_read_b64_tr_b16, GEMM2's A operand = K^T).
__device__ __forceinline__ int img_off(int row, int ch) { return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

constexpr int kBwdSWaves = 2;             // min waves per SIMD of the BWD_S pass at D <= 128 (3 = 170 VGPRs)
constexpr int kSPrefetch = 2;             // BWD_S: tiles of stored dot products in flight ahead of the one being worked on (1 or 2)
#ifndef TT_LOOP_LAMBDA
#define TT_LOOP_LAMBDA 0
#endif
constexpr int kTilesPerBarrier = 2;
constexpr int kTilesPerBarrierBwdS = kTilesPerBarrier;   // the dc pass (one 8-wave workgroup per CU: room for a ring of 8 buffers)
template <int D, int MODE, int PREC>
constexpr int tiles_per_barrier() {
  if (PREC == 0 && D <= 128 && MODE == MODE_BWD_S) return kTilesPerBarrierBwdS;
  return (PREC == 0 && D <= 128 && (MODE == MODE_BWD || MODE == MODE_FUSED || MODE == MODE_FUSED_S))
             ? kTilesPerBarrier : 1;
}

// bf16x3 at dim 256, passes with GEMM1 AND GEMM2: a PAIR of waves shares 32 stationary rows and splits the embedding
// dimension - each wave holds the three bf16 pieces of R[r][128 hw .. 128 hw + 127] (96 VGPRs instead of 192), multiplies
// the tile's matching k-half, the two partial dot-product blocks meet through LDS (4 KB per wave, one extra barrier), both
// waves run the (identical) softmax on the sum, and each accumulates its own 128 columns of the gradient block (64 AGPRs
// instead of 128).  r02's one-wave-per-32-rows form needed ~640 registers of the 512 and spilled 416-556 B per lane.
template <int D, int MODE, int PREC>
constexpr bool split_d() {
  return PREC == 1 && D == 256 && (MODE == MODE_BWD || MODE == MODE_FUSED || MODE == MODE_FUSED_S);
}
// exact f32 at dim 256, online-softmax passes WITH accidental-hit ids / hard negatives: the stationary fragment (128 VGPRs) +
// the gradient block (128) + the tile in flight (32) + the id / threshold state no longer fit 512 registers (r03: 40 / 56 /
// 132 B of scratch per lane).  The LAST k-groups of the fragment - 5 with ids, 8 with thresholds, 10 with both - live in LDS, one
// 16-byte slot per lane, written once and read back by the same lane (one ds_read_b128 per group and tile): 20 / 40 VGPRs less.
template <int D, int MODE, bool HAS_IDS, bool HAS_HN, int PREC>
constexpr int rf_lds_groups() {
  if (PREC == 0 && D == 256 && (MODE == MODE_FUSED || MODE == MODE_FUSED_S) && (HAS_IDS || HAS_HN))
    return (HAS_IDS && HAS_HN) ? 10 : (HAS_HN ? 8 : 5);
  if (PREC == 0 && D == 128 && MODE == MODE_BWD && HAS_IDS && HAS_HN) return 2;      // (20 B of scratch at 2 waves per SIMD)
  return 0;
}
template <int D, int MODE, int PREC, int WAVES>
constexpr int rows_per_wg() { return (split_d<D, MODE, PREC>() ? WAVES / 2 : WAVES) * 32; }

template <int D, int MODE_T, bool HAS_IDS, bool HAS_HN, int WAVES, int PREC>
__global__ __launch_bounds__(WAVES * 64, (WAVES == 8 ? 2 : (D <= 128 ? ((base_mode(MODE_T) == MODE_BWD_S && PREC == 0) ? kBwdSWaves : 2) : 1))) void score_kernel(ScoreArgs p) {   // (min waves per SIMD)
  static_assert(MODE_T != MODE_FUSED_S_WG, "the form without a barrier in its tile loops is score_rowfrag_kernel");
  static_assert(MODE_T != MODE_BWD_S_WG, "the form without a barrier in its tile loops is score_colfrag_kernel");
#include "score_kernel_body.h"
}

// Pass 1 of the plain train step with the column splits inside the workgroup (MODE_FUSED_S_WG): one 32-row fragment per
// workgroup, 8 waves = 8 splits, one workgroup per CU.  LDS: 8 private tile buffers + the row statistics.  The same body under a
// name of its own: its tile loops hold no workgroup barrier, and tests/isa_audit/audit_barriers.py expects one in the tile loop of
// everything called score_kernel.
constexpr int kRowfragWaves = 8;
template <int D> constexpr int rowfrag_lds_bytes() { return (kRowfragWaves * Geo<D, 0>::TILE_F + (2 * kRowfragWaves + 1) * 32) * 4; }
template <int D>
__global__ __launch_bounds__(kRowfragWaves * 64, 2) void score_rowfrag_kernel(ScoreArgs p) {
  constexpr int MODE_T = MODE_FUSED_S_WG, WAVES = kRowfragWaves, PREC = 0;
  constexpr bool HAS_IDS = false, HAS_HN = false;
#include "score_kernel_body.h"
}

// The dc pass of the plain train step with the query splits inside the workgroup (MODE_BWD_S_WG): one 32-candidate fragment per
// workgroup, 8 waves = 8 splits of whole tiles, one workgroup per CU.  LDS: 8 private buffers of a tile and its 64 row terms, and
// the 512 partial sums of the loss.  A name of its own for the reason score_rowfrag_kernel has one.
constexpr int kColfragWaves = 8;
template <int D> constexpr int colfrag_lds_bytes() { return (kColfragWaves * (Geo<D, 0>::TILE_F + 64) + kColfragWaves * 64) * 4; }
template <int D>
__global__ __launch_bounds__(kColfragWaves * 64, 2) void score_colfrag_kernel(ScoreArgs p) {
  constexpr int MODE_T = MODE_BWD_S_WG, WAVES = kColfragWaves, PREC = 0;
  constexpr bool HAS_IDS = false, HAS_HN = false;
#include "score_kernel_body.h"
}

// ---- small kernels around the main pass -------------------------------------------------------

// -log2(clip(p, 1e-6, 1))  (tfrs SamplingProbablityCorrection, log2 domain)
__global__ __launch_bounds__(256) void prob_bias_kernel(const float* __restrict__ prob, float* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = -__log2f(fminf(fmaxf(prob[i], 1e-6f), 1.0f));
}

// a = -lse*log2e ; s = w * inv_t * gscale
__global__ __launch_bounds__(256) void bwd_prep_kernel(const float* __restrict__ lse, const float* __restrict__ w,
                                                       float* __restrict__ a, float* __restrict__ s, int64_t n,
                                                       float scale) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    a[i] = -lse[i] * kLog2e;
    s[i] = (w != nullptr ? w[i] : 1.0f) * scale;
  }
}

// lse / per-row loss from the per-split (max, sum) pairs (the total is summed by sum_rows_kernel in a fixed order)
__global__ __launch_bounds__(256) void fwd_combine_kernel(const float* __restrict__ part_m, const float* __restrict__ part_l,
                                                          const float* __restrict__ pos2, const float* __restrict__ w,
                                                          int64_t n_r, int nsplit, float* __restrict__ lse,
                                                          float* __restrict__ per_row) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_r) return;
  float M = kNegBig;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, part_m[(int64_t)s * n_r + r]);
  float L = 0.f;
  for (int s = 0; s < nsplit; ++s)
    L += part_l[(int64_t)s * n_r + r] * __builtin_amdgcn_exp2f(part_m[(int64_t)s * n_r + r] - M);
  const float lse2 = M + __log2f(L);
  lse[r] = lse2 * kLn2;
  per_row[r] = (lse2 - pos2[r]) * kLn2 * (w != nullptr ? w[r] : 1.0f);
}

// FUSED pass 1 epilogue: per-split (max, sum, G) -> lse, per-row loss, the per-row terms of the dc pass, and
//   dq[r] = (w_r/T*g) * ( sum_s G_s[r]*2^(m_s-M) / L  -  c[r+diag] ).
// dim/4 lanes per row (8 .. 64: one float4 column each - no idle half rows at dim 64, no second column trip at dim 256),
// 256 >> lpr_log2 rows per block.  Splits are taken 8 at a time, every chunk's loads issued together from clamped (valid)
// split indices; additions in split order.  (Through r02: 32 lanes per row whatever the dim, and the splits past the 8th -
// B <= 4096 runs 16 or more - one dependent load after the other: 11.9 us at cfg2.)
__global__ __launch_bounds__(256) void fused_combine_kernel(const float* __restrict__ part_m, const float* __restrict__ part_l,
                                                            const float* __restrict__ pos2, const float* __restrict__ w,
                                                            const f32x4* __restrict__ slab, const f32x4* __restrict__ cpos,
                                                            int64_t n_r, int d4, int lpr_log2, int nsplit, float scale,
                                                            float* __restrict__ lse, float* __restrict__ per_row,
                                                            float* __restrict__ aq, float* __restrict__ sq,
                                                            f32x4* __restrict__ dq) {
  const int rpb = 256 >> lpr_log2;
  const int64_t row = (int64_t)blockIdx.x * rpb + (threadIdx.x >> lpr_log2);
  const int lane = threadIdx.x & ((1 << lpr_log2) - 1);
  if (row >= n_r) return;
  const int c = lane < d4 ? lane : d4 - 1;           // (lpr == d4 for the supported dims; clamped all the same)
  const f32x4 cp = cpos[row * d4 + c];
  const float p2 = pos2[row];
  const float wr = (w != nullptr ? w[row] : 1.0f);
  combine_row(nsplit, [&](int s) { return part_m[(int64_t)s * n_r + row]; }, [&](int s) { return part_l[(int64_t)s * n_r + row]; },
              [&](int s) { return slab[((int64_t)s * n_r + row) * d4 + c]; }, cp, p2, wr, scale, lane == 0, lse + row, per_row + row,
              aq + row, sq + row, lane < d4 ? dq + row * d4 + lane : nullptr);
}

// thr[r] = c1 * <q_r, c_pos(r)> + bias[pos(r)]  (log2 domain): the positive's logit, 32 lanes per row
__global__ __launch_bounds__(256) void pos_logit_kernel(const f32x4* __restrict__ q, const f32x4* __restrict__ c,
                                                        const int64_t* __restrict__ pos_idx, const float* __restrict__ bias,
                                                        int64_t nq, int64_t nc, int d4, float c1, float* __restrict__ thr,
                                                        int64_t diag) {
  const int64_t row = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int lane = threadIdx.x & 31;
  if (row >= nq) return;
  const int64_t pc = pos_idx != nullptr ? pos_idx[row] : row + diag;
  float acc = 0.f;
  if (pc >= 0 && pc < nc) {
    for (int k = lane; k < d4; k += 32) {
      const f32x4 a = q[row * d4 + k], b = c[pc * d4 + k];
      acc += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
    }
  }
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) thr[row] = (pc >= 0 && pc < nc) ? __builtin_fmaf(acc, c1, bias != nullptr ? bias[pc] : 0.f) : 3.0e38f;
}

__global__ __launch_bounds__(256) void rank_combine_kernel(const int32_t* __restrict__ part_cnt, int64_t n_r, int nsplit,
                                                           int32_t* __restrict__ rank) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_r) return;
  int tot = 0;
  for (int s = 0; s < nsplit; ++s) tot += part_cnt[(int64_t)s * n_r + r];
  rank[r] = tot;
}

// ---- hard-negative mining (tfrs.layers.loss.HardNegativeMining): per query keep the positive and the k highest-scoring
// negatives.  The kernels only need a per-row THRESHOLD; it is found on a materialised row of raw dot products
// (scratch [nq][nc], written by the tiled GEMM) with a 4-pass MSB-first radix select (8-bit digits, LDS histogram) of
// the k-th largest negative logit, then the largest value below it; thr = their midpoint, so the later comparisons
// inside the fused kernels cannot flip on rounding.  Ties AT the k-th value are all kept.  One workgroup per row.
__device__ __forceinline__ uint32_t f2key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);       // monotone: larger float -> larger key
}
__device__ __forceinline__ float key2f(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(256) void hardneg_select_kernel(const float* __restrict__ S, int64_t nc, float c1,
                                                            const float* __restrict__ bias2, const int64_t* __restrict__ ids,
                                                            int64_t diag, int k, float* __restrict__ thr) {
  __shared__ int hist[256];
  __shared__ uint32_t sh_prefix, sh_mask, sh_lower;
  __shared__ int sh_remaining, sh_valid;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t pos = row + diag;
  const float* srow = S + row * nc;
  const int64_t idpos = ids != nullptr ? ids[pos] : 0;
  auto valid = [&](int64_t j) { return j != pos && !(ids != nullptr && ids[j] == idpos); };
  auto keyof = [&](int64_t j) { return f2key(__builtin_fmaf(srow[j], c1, bias2 != nullptr ? bias2[j] : 0.f)); };
  if (tid == 0) { sh_prefix = 0; sh_mask = 0; sh_remaining = k; sh_valid = 0; sh_lower = 0; }
  __syncthreads();
  int nv = 0;
  for (int64_t j = tid; j < nc; j += 256) nv += valid(j) ? 1 : 0;
  atomicAdd(&sh_valid, nv);
  __syncthreads();
  if (k >= sh_valid) {                                       // fewer negatives than k: keep everything
    if (tid == 0) thr[row] = -3.0e38f;
    return;
  }
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hist[tid] = 0;
    __syncthreads();
    const uint32_t prefix = sh_prefix, mask = sh_mask;
    for (int64_t j = tid; j < nc; j += 256) {
      if (!valid(j)) continue;
      const uint32_t key = keyof(j);
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int cum = 0, rem = sh_remaining;
      for (int b = 255; b >= 0; --b) {
        if (cum + hist[b] >= rem) {
          sh_prefix = prefix | ((uint32_t)b << shift);
          sh_mask = mask | (255u << shift);
          sh_remaining = rem - cum;
          break;
        }
        cum += hist[b];
      }
    }
    __syncthreads();
  }
  const uint32_t key_k = sh_prefix;                          // exact key of the k-th largest negative
  uint32_t lower = 0;
  for (int64_t j = tid; j < nc; j += 256) {
    if (!valid(j)) continue;
    const uint32_t key = keyof(j);
    if (key < key_k && key > lower) lower = key;
  }
  atomicMax(&sh_lower, lower);
  __syncthreads();
  if (tid == 0) {
    const float vk = key2f(key_k);
    const float vn = sh_lower != 0 ? key2f(sh_lower) : vk - 1.0f;
    thr[row] = 0.5f * vk + 0.5f * vn;
  }
}

// hq = thr + aq : the threshold in the domain of the BWD passes (logit2 - lse2)
__global__ __launch_bounds__(256) void hn_shift_kernel(const float* __restrict__ thr, const float* __restrict__ aq,
                                                       float* __restrict__ hq, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) hq[i] = thr[i] + aq[i];
}

// loss = sum_r per_row[r], fixed order (one workgroup)
__global__ __launch_bounds__(1024) void sum_rows_kernel(const float* __restrict__ per_row, int64_t n, float* __restrict__ loss) {
  __shared__ float red[1024];
  float acc = 0.f;
  for (int64_t r = threadIdx.x; r < n; r += 1024) acc += per_row[r];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = red[0];
}

// out[i] = sum_s slab[s][i], s ascending (float4).  With per_row != NULL the launch has one EXTRA workgroup (the last)
// that computes loss = sum_r per_row[r] in exactly sum_rows_kernel's order (1024 strided partial sums, then the
// binary tree), so the fused training form needs no separate single-workgroup launch for the scalar.
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const f32x4* __restrict__ slab, f32x4* __restrict__ out,
                                                           int64_t n4, int nsplit, const float* __restrict__ per_row,
                                                           int64_t n_rows, float* __restrict__ loss) {
  if (per_row != nullptr && blockIdx.x == gridDim.x - 1) {
    __shared__ float red[256];
    const int t = threadIdx.x;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t r0 = t; r0 < n_rows; r0 += 8 * 1024) {        // 32 loads in flight per thread, adds in row order
      float v[8][4];
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t r = r0 + 1024 * i + 256 * j;
          v[i][j] = r < n_rows ? per_row[r] : 0.f;
        }
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (r0 + 1024 * i + 256 * j < n_rows) a[j] += v[i][j];
    }
    red[t] = (a[0] + a[2]) + (a[1] + a[3]);          // tree steps s = 512 and s = 256
    __syncthreads();
    for (int s2 = 128; s2 > 0; s2 >>= 1) {
      if (t < s2) red[t] += red[t + s2];
      __syncthreads();
    }
    if (t == 0) loss[0] = red[0];
    return;
  }
  const int64_t nblk = per_row != nullptr ? gridDim.x - 1 : gridDim.x;
  const int64_t stride = nblk * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    f32x4 a = slab[i];
    for (int s = 1; s < nsplit; ++s) a += slab[(int64_t)s * n4 + i];
    out[i] = a;
  }
}

// ---- host side --------------------------------------------------------------------------------

constexpr int kScoreWaves = 4;            // waves (32-row fragments) per workgroup of the exact-f32 passes
constexpr int kScoreWgs = 512;            // workgroups a pass aims for (two 4-wave workgroups per CU)
constexpr int kBwdSWgs = 512;             // workgroups the BWD_S pass (dc from the stored dot products) aims for
int choose_nsplit_pow2(int64_t n_r, int64_t n_c, int target_wgs = kScoreWgs) {
  const int64_t nrb = (n_r + 32 * kScoreWaves - 1) / (32 * kScoreWaves);
  int ns = 1;
  // 512 workgroups = two per CU measured best at B = 8192 (256: 291 us, 512: 272 us, 1024: 283 us, 2048: 294 us per launch)
  while (nrb * ns < target_wgs && (int64_t)ns * 2 * 64 <= n_c && ns < 64) ns *= 2;
  return ns;
}

// r04: the split count by a model of the launch instead of "double until 512 workgroups".  A scorer workgroup runs for the WHOLE
// launch (its row block against 1/ns of the columns), and `slots` of them are resident at once (two 4-wave or one 8-wave
// workgroup per CU): n_r = 8192 gives 64 row blocks x 8 splits = exactly 512 - and n_r = 8200 gave 65 x 8 = 520, eight workgroups
// that ran a second round alone: batch 8200 took 0.879 ms against 0.558 for 8192 (pass 1 289 -> 420 us, pass 2 173 -> 318;
// 4100 against 4096: 0.318 vs 0.214 ms).  cost(ns) = rounds(ns) / ns x (1 + 0.005 ns): the rounds the grid needs, each 1/ns of the
// columns long, plus the measured price of more, shorter workgroups (1024 instead of 512 at 8192: +4 %).  The minimum over ns =
// 1..64 is the old choice for every power-of-two shape (checked over n_r, n_c in 64 .. 262144: scratch/r04_nsplit_model.py) and e.g.
// 15 splits (975 workgroups, two nearly full rounds) for 8200.  Any ns is valid: the columns are cut at multiples of 32.
int choose_nsplit(int64_t n_r, int64_t n_c, int rows_per_wg = 32 * kScoreWaves, int slots = kScoreWgs) {
  const int64_t nrb = (n_r + rows_per_wg - 1) / rows_per_wg;
  int best = 1;
  double best_cost = 0.0;
  for (int ns = 1; ns <= 64; ++ns) {
    if (ns > 1 && (int64_t)ns * 64 > n_c) break;
    const int64_t rounds = (nrb * ns + slots - 1) / slots;
    const double cost = (double)rounds / ns * (1.0 + 0.005 * ns);
    if (ns == 1 || cost < best_cost - 1e-12) { best = ns; best_cost = cost; }
  }
  return best;
}

int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

struct WsLayout {
  int ns_q, ns_c;           // splits for the passes whose stationary side is q / c
  int ns_cs;                // ... for the dc pass that reads the stored dot products (BWD_S)
  int64_t off_bias, off_aq, off_sq, off_hq, off_pm, off_pl, off_pos, off_slab, off_S, total_no_S, total;
};

WsLayout ws_layout(int64_t nq, int64_t nc, int32_t dim) {
  WsLayout w{};
  if (dim <= 128) {
    w.ns_q = choose_nsplit(nq, nc);
    w.ns_c = choose_nsplit(nc, nq);
    w.ns_cs = choose_nsplit(nc, nq, 256, 256);     // the dc pass from the stored dot products: 8-wave workgroups, one per CU
  } else {                                         // (dim 256: other workgroup shapes per kernel form; not re-measured - r03's rule)
    w.ns_q = choose_nsplit_pow2(nq, nc);
    w.ns_c = choose_nsplit_pow2(nc, nq);
    w.ns_cs = choose_nsplit_pow2(nc, nq, kBwdSWgs);
  }
  int64_t o = 0;
  w.off_bias = o; o = align_up(o + nc * 4, 256);
  w.off_aq = o;   o = align_up(o + nq * 4, 256);
  w.off_sq = o;   o = align_up(o + nq * 4, 256);
  w.off_hq = o;   o = align_up(o + nq * 4, 256);
  w.off_pm = o;   o = align_up(o + (int64_t)w.ns_q * nq * 4, 256);
  w.off_pl = o;   o = align_up(o + (int64_t)w.ns_q * nq * 4, 256);
  w.off_pos = o;  o = align_up(o + nq * 4, 256);
  w.off_slab = o;
  const int64_t slab_q = (int64_t)w.ns_q * nq * dim * 4, slab_c = (int64_t)(w.ns_c > w.ns_cs ? w.ns_c : w.ns_cs) * nc * dim * 4;
  o = align_up(o + (slab_q > slab_c ? slab_q : slab_c), 256);
  w.total_no_S = o;
  // the training entry keeps the raw dot products [nq][nc] between its two passes (pass 2 reads them back instead of
  // recomputing them: half its matrix-pipe work for 8 bytes of hidden HBM traffic per logit)
  w.off_S = o;
  o = align_up(o + ((nq + 31) / 32) * ((nc + 31) / 32) * 4096, 256);
  w.total = o;
  return w;
}

// 4 waves (128 rows) per workgroup, two workgroups per CU.  An 8-wave variant whose two wave groups run one phase apart
// (GEMM1 | GEMM2, epilogue | GEMM1, GEMM2 | epilogue, a barrier per phase) was built and measured: no gain (277 vs 271 us).
// Ablation on MI355X (B = 8192, D = 128; us per launch): all 272 | no epilogue math 257 | no tile staging 270 |
// no GEMM1 171 | no GEMM2 171 | neither GEMM 58 | nothing but the loop skeleton 34.  So the two GEMMs together cost
// 220 us = 156 TF, the f32 MFMA peak; what is left is ~34 us of fixed cost (prologue, per-tile barriers, 33.5 MB of
// slab stores, drain) and ~20 us around the softmax epilogue that the partner wave's MFMAs do not hide (f32-input
// MFMA runs at the f32 vector rate; a 25 % cut of the epilogue's VALU instructions changed nothing measurable, so the
// cost is in the GEMM1 -> epilogue -> GEMM2 dependency hand-offs rather than in VALU throughput).
// waves per workgroup of the exact-f32 training passes at D <= 128 (r02 A/B at cfg3: the dc pass with 8 waves = 256 stationary
// rows per workgroup, one workgroup per CU, half the tile staging per MFMA: 169.0 -> 165.8 us; pass 1 with 8: 276.8 -> 277.6)
constexpr int kBwdSWgWaves = 8;
constexpr int kFusedSWgWaves = 4;
template <int D, int MODE_T, int PREC = 0>
constexpr int waves_for() {
  constexpr int MODE = base_mode(MODE_T);
  return (PREC == 1 && D == 128) ? 8 : (PREC == 1 ? 4 : ((MODE == MODE_BWD_S && D <= 128) ? kBwdSWgWaves
                                                         : ((MODE == MODE_FUSED_S && D <= 128) ? kFusedSWgWaves : kScoreWaves)));
}     // bf16x3 at dim 128: 256-row workgroups, one per CU

template <int D, int MODE, int PREC = 0>
int launch_score(const ScoreArgs& a_in, hipStream_t stream) {
  constexpr int W = waves_for<D, MODE, PREC>();
  constexpr int RPW = rows_per_wg<D, MODE, PREC, W>();
  const int64_t nrb = (a_in.n_r + RPW - 1) / RPW;
  const int64_t blocks = nrb * a_in.nsplit;
  // bf16x3 with 8 waves: + the R_lo fragments of the 8 waves
  const int lds_base = Geo<D, PREC>::LDS_BYTES * tiles_per_barrier<D, MODE, PREC>() +
                  ((PREC == 1 && W == 8) ? W * Geo<D, PREC>::KS * 64 * 16 : 0) +
                  (split_d<D, MODE, PREC>() ? W * 4096 : 0);          // + the pair's dot-product exchange
  const bool has_ids = a_in.id_c != nullptr;       // every pass sets the id pair together (pass_args)
  const bool has_hn = (a_in.h_r != nullptr) || (a_in.h_c != nullptr);
  const ScoreArgs& a = a_in;
  auto go_at = [&](auto kern, int64_t grid, int threads, int lds) -> int {
    if (lds > 64 * 1024) {   // above the 64 KiB default the limit must be raised (cheap, idempotent)
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return tt::fail(TT_ERR_LAUNCH, "hipFuncSetAttribute(LDS %d) failed", lds);
    }
    constexpr const char* tag = MODE == MODE_FWD ? "score_fwd" : ((MODE == MODE_BWD || MODE == MODE_BWD_S) ? "score_bwd"
                                : ((MODE == MODE_FUSED || MODE == MODE_FUSED_S) ? "score_fused" : "score_rank"));
    tt::launch(tag, kern, dim3((unsigned)grid), dim3(threads), (unsigned)lds, stream, a);
    return tt::check_launch(tag);
  };
  auto go = [&](auto kern, int rfl_groups = 0, int extra_lds = 0) -> int {
    // + the LDS-resident k-groups of the stationary fragment
    return go_at(kern, blocks, W * 64, lds_base + W * rfl_groups * 64 * 16 + extra_lds);
  };
  // the plain train step (exact f32): the instantiations without the arguments it never passes
  if constexpr (PREC == 0 && (MODE == MODE_FUSED_S || MODE == MODE_BWD_S)) {
    if (!has_ids && !has_hn && a.pos_idx == nullptr) {
      if constexpr (MODE == MODE_FUSED_S) {
        // (dim 256: the general kernel fills the register file - 512 with the accumulators - and a second loop body spilled 300 B;
        // dim 32: a thread stages ONE float4 per tile, and without the bias that is the only load of the loop - nothing for a
        // partial wait to keep in flight, and tests/test_isa_score_loads.py takes a loop with fewer than two loads for the wrong loop)
        if constexpr (D == 64 || D == 128) {
          if (a.a_c == nullptr) {
            // the splits inside the workgroup (the caller asks for it by passing the combine's outputs: pass1_in_workgroup)
            if constexpr (D == 128) {
              if (a.dq != nullptr && a.nsplit == kRowfragWaves)
                return go_at(score_rowfrag_kernel<D>, (a.n_r + 31) / 32, kRowfragWaves * 64, rowfrag_lds_bytes<D>());
            }
            if (a.dq == nullptr) return go(score_kernel<D, MODE_FUSED_S_NC, false, false, W, 0>);
          }
        }
      } else {
        if (a.a_r == nullptr && a.s_r == nullptr && a.a_c != nullptr && a.s_c != nullptr) {
          // the splits inside the workgroup (the caller asks for it by passing dc itself: dc_in_workgroup): wave w = split w, and
          // every split whole tiles of equal number - the kernel has no tail loop, no row mask and no clamp on a streamed row
          if constexpr (D == 128) {
            if (a.dr != nullptr && a.nsplit == kColfragWaves && a.n_c == kColfragWaves * a.c_per_split)
              return go_at(score_colfrag_kernel<D>, (a.n_r + 31) / 32, kColfragWaves * 64, colfrag_lds_bytes<D>());
          }
          if constexpr (row_terms_in_lds<D, MODE_BWD_S_NR>()) {
            // the row terms once per workgroup in LDS where a split's rows fit the array, else per tile as ever
            if (a.c_per_split > kRowTermRows) return go(score_kernel<D, MODE_BWD_S_NR_T, false, false, W, 0>);
            return go(score_kernel<D, MODE_BWD_S_NR, false, false, W, 0>, 0, 2 * kRowTermRows * 4);
          }
          return go(score_kernel<D, MODE_BWD_S_NR, false, false, W, 0>);
        }
      }
    }
  }
  if (a.dq != nullptr) return tt::fail(TT_ERR_UNSUPPORTED, "score pass 1: no in-workgroup combine for this call");   // (never silently without dq)
  if (a.dr != nullptr) return tt::fail(TT_ERR_UNSUPPORTED, "score pass 2: no in-workgroup split sum for this call"); // (... nor without dc)
  if (has_ids && has_hn) return go(score_kernel<D, MODE, true, true, W, PREC>, rf_lds_groups<D, MODE, true, true, PREC>());
  if (has_ids) return go(score_kernel<D, MODE, true, false, W, PREC>, rf_lds_groups<D, MODE, true, false, PREC>());
  if (has_hn) return go(score_kernel<D, MODE, false, true, W, PREC>, rf_lds_groups<D, MODE, false, true, PREC>());
  return go(score_kernel<D, MODE, false, false, W, PREC>);
}

// prec 0: exact f32 products; prec 1: bf16x3, at the dims whose tiles are whole [32][128] bf16 images.  MODE_BWD (the separate
// backward entry) is exact f32 only: no bf16x3 form of it is instantiated.
template <int MODE>
int dispatch_score(int prec, int32_t dim, const ScoreArgs& a, hipStream_t stream) {
  if (prec == 1) {
    if constexpr (MODE == MODE_BWD) return tt::fail(TT_ERR_UNSUPPORTED, "retrieval (bf16x3): no separate backward pass");
    else switch (dim) {
      case 128: return launch_score<128, MODE, 1>(a, stream);
      case 256: return launch_score<256, MODE, 1>(a, stream);
      default: return tt::fail(TT_ERR_UNSUPPORTED, "retrieval (bf16x3): dim %d not in {128,256}", dim);
    }
  }
  switch (dim) {
    case 32: return launch_score<32, MODE>(a, stream);
    case 64: return launch_score<64, MODE>(a, stream);
    case 128: return launch_score<128, MODE>(a, stream);
    case 256: return launch_score<256, MODE>(a, stream);
    default: return tt::fail(TT_ERR_UNSUPPORTED, "retrieval: dim %d not in {32,64,128,256}", dim);
  }
}

// How much of the workspace (ws_layout) an entry uses: the rank pass the regions in front of part_l, the forward-only and
// separate-backward entries everything in front of the stored dot products, the training entry all of it.
enum WsNeed { WS_RANK, WS_NO_S, WS_FULL };

// The requirements every launching entry shares, reported under the entry's own name `fn`.  has_diag = false: a rank pass with
// explicit positives has no diagonal, so nq > nc is fine.
int check_common(const char* fn, const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                 int64_t diag_offset, const void* ws, int64_t ws_bytes, WsNeed ws_need, bool has_diag = true) {
  TT_REQUIRE(q && c && ws, "%s: null pointer", fn);
  TT_REQUIRE(nq > 0 && nc > 0, "%s: nq and nc must be positive", fn);
  TT_REQUIRE(!has_diag || (diag_offset >= 0 && nq + diag_offset <= nc), "%s: need 0 <= diag_offset and nq + diag_offset <= nc", fn);
  TT_REQUIRE(dim == 32 || dim == 64 || dim == 128 || dim == 256, "%s: dim %d not in {32,64,128,256}", fn, dim);
  TT_REQUIRE(tt::aligned16(q) && tt::aligned16(c), "%s: q/c must be 16-byte aligned", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255u) == 0, "%s: workspace must be 256-byte aligned", fn);
  const WsLayout wl = ws_layout(nq, nc, dim);
  const int64_t need = ws_need == WS_FULL ? wl.total : (ws_need == WS_NO_S ? wl.total_no_S : wl.off_pl);
  if (ws_bytes < need)
    return tt::fail(TT_ERR_WORKSPACE, "%s: workspace %lld < %lld bytes", fn, (long long)ws_bytes, (long long)need);
  return TT_OK;
}

// The column bias -log2 p_c of the sampling-probability correction: written to the workspace's front when cand_prob is given.
// *bias = what the passes take as the candidates' additive term (null: none).
int column_bias(const float* cand_prob, int64_t nc, void* workspace, const WsLayout& w, hipStream_t stream, const float** bias) {
  *bias = nullptr;
  if (cand_prob == nullptr) return TT_OK;
  float* b = reinterpret_cast<float*>(static_cast<char*>(workspace) + w.off_bias);
  hipLaunchKernelGGL(prob_bias_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, stream, cand_prob, b, nc);
  *bias = b;
  return tt::check_launch("prob_bias");
}

// What every pass derives from the entry's arguments alone: which matrix is stationary (R) and which streamed (K), the diagonal
// as the stationary rows see it, the split of the streamed side, and the accidental-hit ids of rows and columns.  cand_ids is
// indexed by candidate, and query i's positive is candidate i + diag_offset: the query side reads it shifted by diag_offset.
// The caller adds what is particular to the pass: biases, scales, thresholds, outputs, S.
enum Stationary { STATIONARY_Q, STATIONARY_C };
ScoreArgs pass_args(Stationary side, const float* q, const float* c, int64_t nq, int64_t nc, int64_t diag_offset,
                    float inv_temperature, int nsplit, const int64_t* cand_ids) {
  const int64_t* ids_q = cand_ids != nullptr ? cand_ids + diag_offset : nullptr;
  ScoreArgs a{};
  if (side == STATIONARY_Q) {
    a.R = q; a.K = c; a.n_r = nq; a.n_c = nc; a.diag = diag_offset;
    a.id_r = ids_q; a.id_c = cand_ids;
  } else {
    a.R = c; a.K = q; a.n_r = nc; a.n_c = nq; a.diag = -diag_offset;
    a.id_r = cand_ids; a.id_c = ids_q;
  }
  a.c1 = kLog2e * inv_temperature;
  a.nsplit = nsplit;
  a.c_per_split = align_up((a.n_c + nsplit - 1) / nsplit, 32);
  return a;
}

// dc: stationary c, stream q.  Candidates beyond nq + diag_offset have no positive: diag never matches.
// smat: the dot products pass 1 stored (MODE_BWD_S); null: the pass recomputes them (MODE_BWD).
ScoreArgs dc_pass_args(const float* q, const float* c, int64_t nq, int64_t nc, int64_t diag_offset, float inv_temperature,
                       int nsplit, const int64_t* cand_ids, const float* bias, const float* aq, const float* sq,
                       const float* hq, float* slab, float* smat) {
  ScoreArgs a = pass_args(STATIONARY_C, q, c, nq, nc, diag_offset, inv_temperature, nsplit, cand_ids);
  a.a_r = bias; a.s_r = nullptr; a.a_c = aq; a.s_c = sq;
  a.h_c = hq;
  a.slab = slab;
  if (smat != nullptr) { a.S = smat; a.ldS = (nq + 31) / 32; }
  return a;
}

// out [n][dim] = the sum of a pass's nsplit slabs, in split order.  With per_row, one extra workgroup writes
// loss = sum(per_row[0 .. n_rows)).
int reduce_slabs(const char* what, const float* slab, float* out, int64_t n, int32_t dim, int nsplit, const float* per_row,
                 int64_t n_rows, float* loss, hipStream_t stream) {
  const int64_t n4 = n * dim / 4;
  const int64_t blocks = (n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048;
  tt::launch("score_aux", reduce_slabs_kernel, dim3((unsigned)blocks + (per_row != nullptr ? 1 : 0)), dim3(256), 0, stream,
             reinterpret_cast<const f32x4*>(slab), reinterpret_cast<f32x4*>(out), n4, nsplit, per_row, n_rows, loss);
  return tt::check_launch(what);
}

}  // namespace

// How many ways a pass of the scorer cuts its streamed side (a host query: what sizes the workspace, and what a test can pin):
// pass 0 = stationary q (loss + dq, forward, rank), 1 = stationary c (dc, recomputing the products), 2 = dc from the stored products.
extern "C" int32_t tt_retrieval_num_splits(int64_t nq, int64_t nc, int32_t dim, int32_t pass) {
  if (nq <= 0 || nc <= 0 || dim <= 0 || pass < 0 || pass > 2) return 0;
  const WsLayout w = ws_layout(nq, nc, dim);
  return pass == 0 ? w.ns_q : (pass == 1 ? w.ns_c : w.ns_cs);
}

extern "C" int64_t tt_retrieval_workspace_bytes(int64_t nq, int64_t nc, int32_t dim) {
  if (nq <= 0 || nc <= 0 || dim <= 0) return 0;
  return ws_layout(nq, nc, dim).total;
}

// the forward-only (validation) and separate-backward entries need no logit buffer: everything in front of it
extern "C" int64_t tt_retrieval_fwd_workspace_bytes(int64_t nq, int64_t nc, int32_t dim) {
  if (nq <= 0 || nc <= 0 || dim <= 0) return 0;
  return ws_layout(nq, nc, dim).total_no_S;
}

// the rank (metric) pass uses the regions in front of the gradient slabs only: bias, threshold, per-split counts
extern "C" int64_t tt_retrieval_rank_workspace_bytes(int64_t nq, int64_t nc, int32_t dim) {
  if (nq <= 0 || nc <= 0 || dim <= 0) return 0;
  return ws_layout(nq, nc, dim).off_pl;
}

// (`fn`, here and in the other shared bodies: the entry's own name, for its messages)
static int retrieval_fwd(const char* fn, int prec, const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                         int64_t diag_offset, float inv_temperature, const float* sample_weight,
                         const float* cand_prob, const int64_t* cand_ids, const float* hard_thr,
                         void* workspace, int64_t workspace_bytes, float* lse, float* per_row, float* loss,
                         tt_stream_t stream_) {
  int rc = check_common(fn, q, c, nq, nc, dim, diag_offset, workspace, workspace_bytes, WS_NO_S);
  if (rc != TT_OK) return rc;
  TT_REQUIRE(lse && per_row && loss, "%s: null output pointer", fn);
  hipStream_t stream = tt::as_stream(stream_);
  const WsLayout w = ws_layout(nq, nc, dim);
  char* ws = static_cast<char*>(workspace);
  const float* bias;
  if ((rc = column_bias(cand_prob, nc, workspace, w, stream, &bias)) != TT_OK) return rc;
  ScoreArgs a = pass_args(STATIONARY_Q, q, c, nq, nc, diag_offset, inv_temperature, w.ns_q, cand_ids);
  a.a_c = bias;
  a.h_r = hard_thr;
  a.part_m = reinterpret_cast<float*>(ws + w.off_pm);
  a.part_l = reinterpret_cast<float*>(ws + w.off_pl);
  a.pos2 = reinterpret_cast<float*>(ws + w.off_pos);
  if ((rc = dispatch_score<MODE_FWD>(prec, dim, a, stream)) != TT_OK) return rc;
  tt::ProfScope prof("score_aux", stream);
  hipLaunchKernelGGL(fwd_combine_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, a.part_m, a.part_l, a.pos2,
                     sample_weight, nq, a.nsplit, lse, per_row);
  if ((rc = tt::check_launch("fwd_combine")) != TT_OK) return rc;
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(1024), 0, stream, per_row, nq, loss);
  return tt::check_launch("sum_rows");
}

extern "C" int tt_retrieval_fwd_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                    int64_t diag_offset, float inv_temperature, const float* sample_weight,
                                    const float* cand_prob, const int64_t* cand_ids, const float* hard_thr,
                                    void* workspace, int64_t workspace_bytes, float* lse, float* per_row, float* loss,
                                    tt_stream_t stream) {
  return retrieval_fwd("tt_retrieval_fwd_f32", 0, q, c, nq, nc, dim, diag_offset, inv_temperature, sample_weight, cand_prob, cand_ids,
                       hard_thr, workspace, workspace_bytes, lse, per_row, loss, stream);
}

// The validation pass with the logits' products on the bf16 matrix cores (the 6-product split of GEMM1: 2^-24 relative,
// f32 accumulation, f32 softmax): the forward pass is pure GEMM1, so the 6-product form is the whole kernel.  dim in {128, 256}.
extern "C" int tt_retrieval_fwd_bf16x3_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                           int64_t diag_offset, float inv_temperature, const float* sample_weight,
                                           const float* cand_prob, const int64_t* cand_ids, const float* hard_thr,
                                           void* workspace, int64_t workspace_bytes, float* lse, float* per_row, float* loss,
                                           tt_stream_t stream) {
  if (dim != 128 && dim != 256) return tt::fail(TT_ERR_UNSUPPORTED, "tt_retrieval_fwd_bf16x3_f32: dim %d not in {128,256}", dim);
  return retrieval_fwd("tt_retrieval_fwd_bf16x3_f32", 1, q, c, nq, nc, dim, diag_offset, inv_temperature, sample_weight, cand_prob,
                       cand_ids, hard_thr, workspace, workspace_bytes, lse, per_row, loss, stream);
}

extern "C" int tt_retrieval_bwd_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                    int64_t diag_offset, float inv_temperature, const float* sample_weight,
                                    const float* cand_prob, const int64_t* cand_ids, const float* hard_thr,
                                    const float* lse, float grad_scale, void* workspace, int64_t workspace_bytes,
                                    float* dq, float* dc, tt_stream_t stream_) {
  int rc = check_common("tt_retrieval_bwd_f32", q, c, nq, nc, dim, diag_offset, workspace, workspace_bytes, WS_NO_S);
  if (rc != TT_OK) return rc;
  TT_REQUIRE(lse && dq && dc, "tt_retrieval_bwd_f32: null lse/dq/dc");
  TT_REQUIRE(tt::aligned16(dq) && tt::aligned16(dc), "tt_retrieval_bwd_f32: dq/dc must be 16-byte aligned");
  hipStream_t stream = tt::as_stream(stream_);
  const WsLayout w = ws_layout(nq, nc, dim);
  char* ws = static_cast<char*>(workspace);
  float* aq = reinterpret_cast<float*>(ws + w.off_aq);
  float* sq = reinterpret_cast<float*>(ws + w.off_sq);
  float* slab = reinterpret_cast<float*>(ws + w.off_slab);
  const float* bias;
  if ((rc = column_bias(cand_prob, nc, workspace, w, stream, &bias)) != TT_OK) return rc;
  hipLaunchKernelGGL(bwd_prep_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, lse, sample_weight, aq,
                     sq, nq, inv_temperature * grad_scale);
  if ((rc = tt::check_launch("bwd_prep")) != TT_OK) return rc;
  float* hq = nullptr;
  if (hard_thr != nullptr) {
    hq = reinterpret_cast<float*>(ws + w.off_hq);
    hipLaunchKernelGGL(hn_shift_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, hard_thr, aq, hq, nq);
    if ((rc = tt::check_launch("hn_shift")) != TT_OK) return rc;
  }

  // dq: stationary q, stream c
  {
    ScoreArgs a = pass_args(STATIONARY_Q, q, c, nq, nc, diag_offset, inv_temperature, w.ns_q, cand_ids);
    a.a_r = aq; a.s_r = sq; a.a_c = bias; a.s_c = nullptr;
    a.h_r = hq;
    a.slab = slab;
    if ((rc = dispatch_score<MODE_BWD>(0, dim, a, stream)) != TT_OK) return rc;
    if ((rc = reduce_slabs("reduce_slabs(dq)", slab, dq, nq, dim, a.nsplit, nullptr, 0, nullptr, stream)) != TT_OK) return rc;
  }
  const ScoreArgs a = dc_pass_args(q, c, nq, nc, diag_offset, inv_temperature, w.ns_c, cand_ids, bias, aq, sq, hq, slab, nullptr);
  if ((rc = dispatch_score<MODE_BWD>(0, dim, a, stream)) != TT_OK) return rc;
  return reduce_slabs("reduce_slabs(dc)", slab, dc, nc, dim, a.nsplit, nullptr, 0, nullptr, stream);
}

// Fused training entry: loss AND both gradients in two passes (8*B^2*D executed FLOPs instead of 10):
//   pass 1 (R = q, K = c, MODE_FUSED_S): online softmax + sum_c p*c  -> lse, per-row loss, dq; stores the dot products
//   pass 2 (R = c, K = q, MODE_BWD_S)  : reads them back with the final lse -> dc
static int retrieval_fwd_bwd(const char* fn, int prec, const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                             int64_t diag_offset, float inv_temperature, const float* sample_weight,
                             const float* cand_prob, const int64_t* cand_ids, const float* hard_thr,
                             float grad_scale, void* workspace, int64_t workspace_bytes, float* lse,
                             float* per_row, float* loss, float* dq, float* dc, tt_stream_t stream_) {
  // Both precisions keep pass 1's dot products for pass 2 (the workspace includes the buffer).  bf16x3 at dim 256 recomputed them
  // until r03: with the wave-pair kernels, B 32768: pass 1 / pass 2 = 6.10 / 5.87 ms recomputing, 6.45 / 3.51 ms keeping them
  // (exact f32: 8.77 / 5.17 ms) - profiles/r03_score_f32_vs_bf16x3.jsonl.
  int rc = check_common(fn, q, c, nq, nc, dim, diag_offset, workspace, workspace_bytes, WS_FULL);
  if (rc != TT_OK) return rc;
  TT_REQUIRE(lse && per_row && loss && dq && dc, "%s: null output pointer", fn);
  TT_REQUIRE(tt::aligned16(dq) && tt::aligned16(dc), "%s: dq/dc must be 16-byte aligned", fn);
  hipStream_t stream = tt::as_stream(stream_);
  const WsLayout w = ws_layout(nq, nc, dim);
  char* ws = static_cast<char*>(workspace);
  float* aq = reinterpret_cast<float*>(ws + w.off_aq);
  float* sq = reinterpret_cast<float*>(ws + w.off_sq);
  float* slab = reinterpret_cast<float*>(ws + w.off_slab);
  float* smat = reinterpret_cast<float*>(ws + w.off_S);       // [nq][nc] raw dot products, pass 1 -> pass 2
  const float* bias;
  if ((rc = column_bias(cand_prob, nc, workspace, w, stream, &bias)) != TT_OK) return rc;
  {
    ScoreArgs a = pass_args(STATIONARY_Q, q, c, nq, nc, diag_offset, inv_temperature, w.ns_q, cand_ids);
    a.a_c = bias;
    a.h_r = hard_thr;
    a.S = smat; a.ldS = (nq + 31) / 32;
    a.part_m = reinterpret_cast<float*>(ws + w.off_pm);
    a.part_l = reinterpret_cast<float*>(ws + w.off_pl);
    a.pos2 = reinterpret_cast<float*>(ws + w.off_pos);
    a.slab = slab;
    // The plain step (exact f32, no probability, ids or hard negatives) at dim 128 with 8 column splits: one row fragment per
    // workgroup, the splits combined in LDS by the pass itself (MODE_FUSED_S_WG) - no slab, no part_m / part_l, no combine launch.
    const bool in_workgroup = prec == 0 && dim == 128 && w.ns_q == kRowfragWaves && bias == nullptr && cand_ids == nullptr &&
                              hard_thr == nullptr;
    if (in_workgroup) {
      a.w = sample_weight; a.scale = inv_temperature * grad_scale;
      a.lse = lse; a.per_row = per_row; a.aq = aq; a.sq = sq; a.dq = dq;
    }
    // (bf16x3 at dim 128 keeps the dot products too: 134 + 89 us against 123 + 124 us recomputing - with the row-major buffer
    // it had been 200 + 127 us, the blocked layout is what makes it pay.)
    if ((rc = dispatch_score<MODE_FUSED_S>(prec, dim, a, stream)) != TT_OK) return rc;
    if (!in_workgroup) {
      int lpr_log2 = 3;                              // dim/4 lanes per row: 8 (dim 32) .. 64 (dim 256)
      while ((1 << lpr_log2) < dim / 4) ++lpr_log2;
      const int rpb = 256 >> lpr_log2;
      tt::launch("score_aux", fused_combine_kernel, dim3((unsigned)((nq + rpb - 1) / rpb)), dim3(256), 0, stream, a.part_m, a.part_l, a.pos2,
                         sample_weight, reinterpret_cast<const f32x4*>(slab),
                         reinterpret_cast<const f32x4*>(c + diag_offset * dim), nq, dim / 4, lpr_log2, a.nsplit,
                         inv_temperature * grad_scale, lse, per_row, aq, sq, reinterpret_cast<f32x4*>(dq));
      if ((rc = tt::check_launch("fused_combine")) != TT_OK) return rc;
    }
    // loss = sum(per_row): by one extra workgroup of the dc slab reduction below
  }
  float* hq = nullptr;
  if (hard_thr != nullptr) {
    hq = reinterpret_cast<float*>(ws + w.off_hq);
    hipLaunchKernelGGL(hn_shift_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, hard_thr, aq, hq, nq);
    if ((rc = tt::check_launch("hn_shift")) != TT_OK) return rc;
  }
  ScoreArgs a = dc_pass_args(q, c, nq, nc, diag_offset, inv_temperature, w.ns_cs, cand_ids, bias, aq, sq, hq, slab, smat);
  // The plain step at dim 128 with 8 query splits of whole tiles (nq = 8 * c_per_split, so nq % 256 == 0): one candidate fragment
  // per workgroup, the splits summed in LDS and the loss summed by the pass itself (MODE_BWD_S_WG) - the slab region stays
  // untouched and there is no reduction launch.  Independent of pass 1's form.
  const bool dc_in_workgroup = prec == 0 && dim == 128 && w.ns_cs == kColfragWaves && bias == nullptr && cand_ids == nullptr &&
                               hard_thr == nullptr && nq == kColfragWaves * a.c_per_split;
  if (dc_in_workgroup) { a.dr = dc; a.per_row = per_row; a.loss = loss; }
  if ((rc = dispatch_score<MODE_BWD_S>(prec, dim, a, stream)) != TT_OK) return rc;
  if (dc_in_workgroup) return TT_OK;
  return reduce_slabs("reduce_slabs(dc)", slab, dc, nc, dim, a.nsplit, per_row, nq, loss, stream);
}

extern "C" int tt_retrieval_fwd_bwd_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                        int64_t diag_offset, float inv_temperature, const float* sample_weight,
                                        const float* cand_prob, const int64_t* cand_ids, const float* hard_thr,
                                        float grad_scale, void* workspace, int64_t workspace_bytes, float* lse,
                                        float* per_row, float* loss, float* dq, float* dc, tt_stream_t stream) {
  return retrieval_fwd_bwd("tt_retrieval_fwd_bwd_f32", 0, q, c, nq, nc, dim, diag_offset, inv_temperature, sample_weight, cand_prob,
                           cand_ids, hard_thr, grad_scale, workspace, workspace_bytes, lse, per_row, loss, dq, dc, stream);
}

// The same two passes with every matrix product on bf16 MFMA through the hi/mid/lo split of the f32 operands
// (f32-emulated: 6 products for the logits, 3 for the gradient sums; f32 accumulation, f32 softmax).  dim in {128, 256}.
extern "C" int tt_retrieval_fwd_bwd_bf16x3_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                               int64_t diag_offset, float inv_temperature, const float* sample_weight,
                                               const float* cand_prob, const int64_t* cand_ids, const float* hard_thr,
                                               float grad_scale, void* workspace, int64_t workspace_bytes, float* lse,
                                               float* per_row, float* loss, float* dq, float* dc, tt_stream_t stream) {
  if (dim != 128 && dim != 256) return tt::fail(TT_ERR_UNSUPPORTED, "tt_retrieval_fwd_bwd_bf16x3_f32: dim %d not in {128,256}", dim);
  return retrieval_fwd_bwd("tt_retrieval_fwd_bwd_bf16x3_f32", 1, q, c, nq, nc, dim, diag_offset, inv_temperature, sample_weight,
                           cand_prob, cand_ids, hard_thr, grad_scale, workspace, workspace_bytes, lse, per_row, loss, dq, dc, stream);
}

// Retrieval metric support (configs/data_config.yaml:71 top_k_eval): rank of each query's true
// candidate among ALL nc candidates = number of other candidates with a strictly larger logit.  One fused pass over
// the [nq, nc] logits (never materialised); Recall@K / NDCG@K follow from rank < K on the host side.
// The positive of query i: candidate pos_index[i], or with pos_index == nullptr (the in-batch form) candidate i + diag_offset.
static int retrieval_rank(const char* fn, int prec, const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                          int64_t diag_offset, float inv_temperature, const float* cand_prob, const int64_t* pos_index,
                          const int64_t* cand_ids, void* workspace, int64_t workspace_bytes, int32_t* rank, tt_stream_t stream_) {
  // (a rank pass with explicit positives has no diagonal, so nq > nc is fine; either form needs only the front of the workspace)
  int rc = check_common(fn, q, c, nq, nc, dim, diag_offset, workspace, workspace_bytes, WS_RANK, pos_index == nullptr);
  if (rc != TT_OK) return rc;
  hipStream_t stream = tt::as_stream(stream_);
  const WsLayout w = ws_layout(nq, nc, dim);
  char* ws = static_cast<char*>(workspace);
  float* thr = reinterpret_cast<float*>(ws + w.off_aq);
  const float* bias;
  if ((rc = column_bias(cand_prob, nc, workspace, w, stream, &bias)) != TT_OK) return rc;
  ScoreArgs a = pass_args(STATIONARY_Q, q, c, nq, nc, diag_offset, inv_temperature, w.ns_q, cand_ids);
  hipLaunchKernelGGL(pos_logit_kernel, dim3((unsigned)((nq + 7) / 8)), dim3(256), 0, stream, reinterpret_cast<const f32x4*>(q),
                     reinterpret_cast<const f32x4*>(c), pos_index, bias, nq, nc, dim / 4, a.c1, thr, diag_offset);
  if ((rc = tt::check_launch("pos_logit")) != TT_OK) return rc;
  a.a_r = thr; a.a_c = bias;
  a.pos_idx = pos_index;
  a.part_cnt = reinterpret_cast<int32_t*>(ws + w.off_pm);
  if ((rc = dispatch_score<MODE_RANK>(prec, dim, a, stream)) != TT_OK) return rc;
  hipLaunchKernelGGL(rank_combine_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, a.part_cnt, nq, a.nsplit, rank);
  return tt::check_launch("rank_combine");
}

extern "C" int tt_retrieval_rank_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                     float inv_temperature, const float* cand_prob, const int64_t* pos_index,
                                     void* workspace, int64_t workspace_bytes, int32_t* rank, tt_stream_t stream) {
  TT_REQUIRE(pos_index && rank, "tt_retrieval_rank_f32: null pointer");
  return retrieval_rank("tt_retrieval_rank_f32", 0, q, c, nq, nc, dim, 0, inv_temperature, cand_prob, pos_index, nullptr, workspace,
                        workspace_bytes, rank, stream);
}

// Top-K over a 10M-100M-row corpus is pure GEMM1 as well: the same rank pass with the 6-product bf16 split.  The positive's
// threshold logit stays an exact f32 dot product (pos_logit_kernel); a competitor within ~2^-22 relative of it may fall on
// either side, exactly as between two exact-f32 evaluation orders (the tests pin ranks between f64 +-1e-5 bounds).
extern "C" int tt_retrieval_rank_bf16x3_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                            float inv_temperature, const float* cand_prob, const int64_t* pos_index,
                                            void* workspace, int64_t workspace_bytes, int32_t* rank, tt_stream_t stream) {
  if (dim != 128 && dim != 256) return tt::fail(TT_ERR_UNSUPPORTED, "tt_retrieval_rank_bf16x3_f32: dim %d not in {128,256}", dim);
  TT_REQUIRE(pos_index && rank, "tt_retrieval_rank_bf16x3_f32: null pointer");
  return retrieval_rank("tt_retrieval_rank_bf16x3_f32", 1, q, c, nq, nc, dim, 0, inv_temperature, cand_prob, pos_index, nullptr,
                        workspace, workspace_bytes, rank, stream);
}

// In-batch rank (tfrs.tasks.Retrieval(batch_metrics=...): Keras top-k categorical accuracy over the IN-BATCH score matrix):
// rank[i] = number of in-batch candidates j != i + diag_offset whose logit - after temperature, sampling-probability
// correction and accidental-hit removal, exactly the scores the loss sees - is strictly above the positive's.  Top-k
// accuracy = mean(rank < k): no [nq, nc] score matrix is materialised, it is the metric pass above run on the batch.
extern "C" int tt_retrieval_batch_rank_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim, int64_t diag_offset,
                                           float inv_temperature, const float* cand_prob, const int64_t* cand_ids,
                                           void* workspace, int64_t workspace_bytes, int32_t* rank, tt_stream_t stream) {
  TT_REQUIRE(rank, "tt_retrieval_batch_rank_f32: null pointer");
  return retrieval_rank("tt_retrieval_batch_rank_f32", 0, q, c, nq, nc, dim, diag_offset, inv_temperature, cand_prob, nullptr, cand_ids,
                        workspace, workspace_bytes, rank, stream);
}

// Hard-negative thresholds (tfrs.tasks.Retrieval(num_hard_negatives=k)): thr[i] separates the k highest-scoring negatives
// of query i (after temperature, sampling-probability correction and accidental-hit removal) from the rest; pass it as
// `hard_thr` to tt_retrieval_{fwd,bwd,fwd_bwd}_f32.  scratch: nq*nc floats (the only place logits are materialised).
extern "C" int tt_retrieval_hard_negative_thresholds_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                                         int64_t diag_offset, float inv_temperature, const float* cand_prob,
                                                         const int64_t* cand_ids, int32_t num_hard_negatives, void* workspace,
                                                         int64_t workspace_bytes, float* scratch, int64_t scratch_bytes,
                                                         float* thr, tt_stream_t stream_) {
  int rc = check_common("tt_retrieval_hard_negative_thresholds_f32", q, c, nq, nc, dim, diag_offset, workspace, workspace_bytes, WS_NO_S);
  if (rc != TT_OK) return rc;
  TT_REQUIRE(num_hard_negatives >= 1, "tt_retrieval_hard_negative_thresholds_f32: num_hard_negatives must be >= 1");
  TT_REQUIRE(scratch && thr, "tt_retrieval_hard_negative_thresholds_f32: null scratch/thr");
  if (scratch_bytes < nq * nc * 4)
    return tt::fail(TT_ERR_WORKSPACE, "tt_retrieval_hard_negative_thresholds_f32: scratch %lld < %lld bytes",
                    (long long)scratch_bytes, (long long)(nq * nc * 4));
  hipStream_t stream = tt::as_stream(stream_);
  const float* bias;
  if ((rc = column_bias(cand_prob, nc, workspace, ws_layout(nq, nc, dim), stream, &bias)) != TT_OK) return rc;
  if ((rc = tt::gemm_nt(q, c, scratch, nq, nc, dim, stream)) != TT_OK) return rc;
  tt::launch("score_aux", hardneg_select_kernel, dim3((unsigned)nq), dim3(256), 0, stream, scratch, nc, kLog2e * inv_temperature,
                     bias, cand_ids, diag_offset, num_hard_negatives, thr);
  return tt::check_launch("hardneg_select");
}
