// Int8-quantised top-K retrieval with an exact f32 re-rank: tt_quantize_rows_i8 and tt_retrieval_topk_i8_f32.
//
// Quantiser (per row, the same code for corpus rows and for the queries inside the scan): amax = max|x|,
// scale = amax / 127.0f (one IEEE f32 division), code = clamp(rintf(x / scale), -127, 127) (half to even); a row with
// amax == 0 has scale 0 and all-zero codes.  A corpus row of D codes is D bytes: one 128-byte line at D = 128.
//
// Contract (include/twotower_hip.h):
//   Stage 1, scan: qc / qscale = the quantised query; iscore[i][j] = sum_d qc[i][d] * codes[j][d] in int32 (|iscore| <=
//   256 * 127^2 < 2^24: its f32 conversion is exact); key = float(iscore) * scales[j] (one f32 multiply).  The k1 candidates
//   of a query are its best by (key descending, index ascending), also at the cut; excluded ids never take a slot.
//   Stage 2, finish: with c, every candidate is scored with topk_select_kernel's f32 MFMA chain (same operands, same
//   k-order: bit-identical to tt_retrieval_topk_f32's score of that pair) and the best k by (score descending, index
//   ascending) are written; without c (k1 == k) the stage-1 order is written with scores key * qscale.  Fewer than k
//   candidates: the tail is (-inf, -1).  Integer sums are order-free and the f32 chain is per pair, so a query's row does
//   not depend on the batch, the split count or the run.
//
// Launches (no synchronisation, no copy to the host):
//   1. i8_scan_kernel: one wave per (32-query row block x corpus split), as topk_select_kernel.  The wave quantises its 32
//      query rows into the B operand of v_mfma_i32_32x32x32_i8 (D / 32 x 4 VGPRs) and streams 32-candidate tiles straight
//      from global memory into the A operand: lane (ln, h) loads the 16 bytes at byte 32 s + 16 h of row c0 + ln for k-step
//      s, A and B hold the same bytes of their rows in the same lane half, so the pairing is consistent whatever the
//      instruction's k <-> element map.  D / 32 MFMAs per tile (4 at D = 128; the f32 kernel issues 64).  Lane ln also
//      loads its row's scale; the scales move to the accumulator rows by shuffles with every lane active (before the
//      divergent selection code).  A tile is D / 8 VGPRs (16 at D = 128, where the f32 kernel needs 64): the room goes to
//      a ring of four tile buffers, three tiles in flight behind the one being scored.
//      Selection is the scheme of topk.hip over the f32 keys with list length k1: sorted LDS list, 48-slot survivor queue,
//      register threshold, rank-based flush.  Each (query, split) writes its sorted list of k1.
//   2. topk_merge_kernel rounds (topk_select.h) over the splits' lists into the [nq][k1] candidate buffer.
//   3. i8_rerank_kernel (with c) or i8_scale_kernel (without): one wave per query.  The re-rank gathers the candidates'
//      f32 rows, 32 at a time, into the A operand in topk_select's tile form with the query in every column of B, reads
//      column 0, and ranks the <= 256 scores by counting.
//
// Split rule (i8_plan; no environment variable): enough waves for the chip (kTargetWaves) but at least kMinColsPerSplit
// candidates per split - about k1 (1 + ln(len / k1)) candidates survive per (query, split), and each split's list of k1
// goes through the merge rounds, so splits are longer than the exact kernel's 512-row minimum.
// LDS: scan min(nq, 32) x (k1 + 48) x 8 B; re-rank 2 KB.
// The quantiser's inline helpers live in quant_i8.h; the finish launch is tt::i8_finish_launch, which ivf_i8.hip ends with too.
#include "topk_select.h"
#include "quant_i8.h"

namespace {

using tt::f32x4;
using tt::f32x16;
using tt::topk::beats;
using tt::topk::kMaxEntries;
using tt::topk::kQueue;

using tt::i8::amax4;
using tt::i8::i32x16;
using tt::i8::i32x4;
using tt::i8::kRing;
using tt::i8::quant4;
using tt::i8::row_scale;

constexpr int kTargetWaves = 2048;       // 256 CUs x 8
constexpr int kMinColsPerSplit = 2048;
constexpr int kMaxSplits = 4096;
constexpr int kQuantThreads = 256;

using tt::align256;

// ---------------------------------------------------------------------------------------------------- quantiser
struct QuantArgs {
  const float* x;
  int64_t n;
  int8_t* codes;
  float* scales;
};

// D / 4 adjacent lanes per row, four elements each
template <int D>
__global__ __launch_bounds__(kQuantThreads) void i8_quantize_kernel(QuantArgs p) {
  constexpr int L = D / 4;
  constexpr int ROWS = kQuantThreads / L;
  const int sub = threadIdx.x % L;
  const int64_t row = (int64_t)blockIdx.x * ROWS + threadIdx.x / L;
  const bool ok = row < p.n;
  const f32x4 v = reinterpret_cast<const f32x4*>(p.x + (ok ? row : 0) * D)[sub];
  float amax = amax4(0.f, v);
#pragma unroll
  for (int off = 1; off < L; off <<= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
  const float scale = row_scale(amax);
  if (ok) {
    reinterpret_cast<int*>(p.codes + row * D)[sub] = quant4(v, scale);
    if (sub == 0) p.scales[row] = scale;
  }
}

// ---------------------------------------------------------------------------------------------------- plan
struct I8Plan {
  int64_t rblocks;
  int nsplit;
  int64_t c_per_split;          // multiple of 32
  int64_t bytes_a, bytes_b;     // one array of the merge buffers
  int64_t off_b, off_cs, off_ci, off_qs;
  int64_t total;
};

I8Plan i8_plan(int64_t nq, int64_t nc, int k1) {
  I8Plan p{};
  p.rblocks = (nq + 31) / 32;
  int64_t ns = (kTargetWaves + p.rblocks - 1) / p.rblocks;
  const int64_t by_cols = (nc + kMinColsPerSplit - 1) / kMinColsPerSplit;
  if (ns > by_cols) ns = by_cols;
  if (ns > kMaxSplits) ns = kMaxSplits;
  if (ns < 1) ns = 1;
  int64_t cps = (nc + ns - 1) / ns;
  cps = (cps + 31) & ~(int64_t)31;
  p.c_per_split = cps;
  p.nsplit = (int)((nc + cps - 1) / cps);
  p.bytes_a = align256(nq * p.nsplit * (int64_t)k1 * 4);
  p.bytes_b = tt::topk_merge_b_bytes(nq, p.nsplit, k1);
  int64_t o = 2 * p.bytes_a;
  p.off_b = o; o += 2 * p.bytes_b;
  p.off_cs = o; o += align256(nq * (int64_t)k1 * 4);     // candidate keys [nq][k1]
  p.off_ci = o; o += align256(nq * (int64_t)k1 * 8);     // candidate indices int64 [nq][k1]
  p.off_qs = o; o += align256(nq * 4);                   // query scales [nq]
  p.total = o;
  return p;
}

bool shape_ok(int64_t nq, int64_t nc, int32_t dim, int32_t k, int32_t k1) {
  return nq > 0 && nc > 0 && nc <= INT32_MAX && (dim == 32 || dim == 64 || dim == 128 || dim == 256) && k >= 1 && k <= k1 &&
         k1 <= TT_TOPK_MAX_K && k1 <= nc;
}

// ---------------------------------------------------------------------------------------------------- stage 1
struct ScanArgs {
  const float* q;
  const int8_t* codes;
  const float* scales;
  int64_t nq, nc;
  int k;                        // list length (k1)
  int nsplit;
  int64_t c_per_split;
  int rows_lds;                 // query rows with LDS state: min(nq, 32)
  const int64_t* excl_off;      // nullable
  const int64_t* excl_idx;
  float* ws_s;                  // [nq][nsplit][k]
  int32_t* ws_i;
  float* qscale;                // [nq]
};

template <int D>
__global__ __launch_bounds__(64) void i8_scan_kernel(ScanArgs p) {
  constexpr int NS = D / 32;                        // k-steps of 32 codes (16 per lane half)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x;
  const int h = lane >> 5;
  const int ln = lane & 31;
  const int k = p.k;
  const int RS = 2 * (k + kQueue);                  // LDS words per query row: list scores, list indices, queue scores, queue indices

  // every quantity that steers a loop with a barrier in it is wave-uniform by construction (readfirstlane)
  const int split = __builtin_amdgcn_readfirstlane((int)(blockIdx.x % (unsigned)p.nsplit));
  const int rblk = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / (unsigned)p.nsplit));
  const int rows_lds = __builtin_amdgcn_readfirstlane(p.rows_lds);
  const int64_t r0 = (int64_t)rblk * 32;
  const int64_t r = r0 + ln;
  const bool r_ok = r < p.nq;
  const int64_t c_begin = (int64_t)split * p.c_per_split;
  int64_t c_end = c_begin + p.c_per_split;
  if (c_end > p.nc) c_end = p.nc;
  const int ntiles = __builtin_amdgcn_readfirstlane((int)((c_end - c_begin + 31) >> 5));

  // stationary fragment: qb[s] = the codes of q[r][32 s + 16 h .. + 15] (two passes over the row: amax, then the codes)
  i32x4 qb[NS];
  {
    const f32x4* R4 = reinterpret_cast<const f32x4*>(p.q + (r_ok ? r : 0) * D) + 4 * h;
    float amax = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) amax = amax4(amax, R4[8 * s + j]);
    amax = fmaxf(amax, __shfl_xor(amax, 32));
    const float qscale = row_scale(amax);
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) qb[s][j] = r_ok ? quant4(R4[8 * s + j], qscale) : 0;
    if (split == 0 && h == 0 && r_ok) p.qscale[r] = qscale;
  }
  int64_t ex_lo = 0, ex_hi = 0;
  if (p.excl_off != nullptr && r_ok) {
    ex_lo = p.excl_off[r];
    ex_hi = p.excl_off[r + 1];
  }
  auto excluded = [&](int64_t cand) -> bool {
    int64_t lo = ex_lo, hi = ex_hi;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (p.excl_idx[mid] < cand) lo = mid + 1; else hi = mid;
    }
    return lo < ex_hi && p.excl_idx[lo] == cand;
  };

  // per-row selection state (lanes ln and ln + 32 hold the same copy)
  int m = 0;                    // list length
  int qn = 0;                   // queue length
  bool full = false;
  float thr_s = 0.f;
  int thr_i = 0;
  float* row = smem + (r_ok ? ln : 0) * RS;
  float* qs = row + 2 * k;
  int* qi = reinterpret_cast<int*>(row + 2 * k + kQueue);

  // a tile: lane (ln, h) loads half h of every 32-byte k-step of row c0 + ln, and the row's scale.  Rows past c_end read
  // the split's first row instead (unconditional loads; their scores are masked by cand < c_end below).
  auto load_tile = [&](i32x4 (&a)[NS], float& sc, int t) {
    const int64_t cand = c_begin + 32 * (int64_t)t + ln;
    const int64_t src_row = cand < c_end ? cand : c_begin;
    const i32x4* src = reinterpret_cast<const i32x4*>(p.codes + src_row * D) + h;
#pragma unroll
    for (int s = 0; s < NS; ++s) a[s] = src[2 * s];
    sc = p.scales[src_row];
  };

  // merge every non-empty queue into its row's list (wave-cooperative; called on wave-uniform control only)
  auto flush = [&]() {
    for (int rr = 0; rr < rows_lds; ++rr) {
      const int qn_r = __builtin_amdgcn_readlane(qn, rr);
      const int m_r = __builtin_amdgcn_readlane(m, rr);
      if (qn_r == 0) continue;
      float* Ls = smem + rr * RS;
      int* Li = reinterpret_cast<int*>(Ls + k);
      const float* Qs = Ls + 2 * k;
      const int* Qi = reinterpret_cast<const int*>(Ls + 2 * k + kQueue);
      const int tot = m_r + qn_r;
      float es[kMaxEntries];
      int ei[kMaxEntries], er[kMaxEntries];
#pragma unroll
      for (int j = 0; j < kMaxEntries; ++j) {
        const int e = lane + 64 * j;
        er[j] = INT_MAX;
        es[j] = 0.f;
        ei[j] = 0;
        if (e < tot) {
          float s;
          int i, rank;
          if (e < m_r) {
            s = Ls[e]; i = Li[e]; rank = e;
          } else {
            s = Qs[e - m_r]; i = Qi[e - m_r];
            int lo = 0, hi = m_r;                    // list entries that beat it: a prefix of the sorted list
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (beats(Ls[mid], Li[mid], s, i)) lo = mid + 1; else hi = mid;
            }
            rank = lo;
          }
          for (int t = 0; t < qn_r; ++t) rank += beats(Qs[t], Qi[t], s, i) ? 1 : 0;
          es[j] = s; ei[j] = i; er[j] = rank;
        }
      }
      __syncthreads();                               // every read of the old list is done (one wave: orders the LDS ops)
#pragma unroll
      for (int j = 0; j < kMaxEntries; ++j)
        if (er[j] < k) { Ls[er[j]] = es[j]; Li[er[j]] = ei[j]; }
      __syncthreads();
      if (ln == rr) {
        m = tot < k ? tot : k;
        qn = 0;
        if (m == k) { full = true; thr_s = Ls[k - 1]; thr_i = Li[k - 1]; }
      }
    }
  };

  auto process = [&](int t, const i32x4 (&a)[NS], float sc) {
    i32x16 X;
#pragma unroll
    for (int i = 0; i < 16; ++i) X[i] = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) X = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], qb[s], X, 0, 0, 0);
    // X[reg] = iscore(query r, candidate c0 + acc_row(reg, h)); the scale of row acc_row(reg, h) comes from the lane that
    // loaded it: the shuffles run here, with every lane active
    const int64_t c0 = c_begin + 32 * (int64_t)t;
    float key[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) key[reg] = (float)X[reg] * __shfl(sc, tt::acc_row(reg, h));
    uint32_t mask = 0;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int64_t cand = c0 + tt::acc_row(reg, h);
      const bool ok = r_ok && cand < c_end && (!full || beats(key[reg], (int)cand, thr_s, thr_i));
      mask |= ok ? (1u << reg) : 0u;
    }
    if (ex_hi > ex_lo && mask != 0u) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
        if (((mask >> reg) & 1u) && excluded(c0 + tt::acc_row(reg, h))) mask &= ~(1u << reg);
    }
    const int n = __builtin_popcount(mask);
    const int n_other = __shfl_xor(n, 32);
    int pos = qn + (h ? n_other : 0);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
      if ((mask >> reg) & 1u) {
        qs[pos] = key[reg];
        qi[pos] = (int)(c0 + tt::acc_row(reg, h));
        ++pos;
      }
    qn += n + n_other;
    if (__ballot(qn > kQueue - 32) != 0ull) flush();
  };

  i32x4 a[kRing][NS];
  float sc[kRing];
#pragma unroll
  for (int j = 0; j < kRing; ++j) {
    sc[j] = 0.f;
    if (j < ntiles) load_tile(a[j], sc[j], j);
  }
  for (int t = 0; t < ntiles; t += kRing) {
#pragma unroll
    for (int j = 0; j < kRing; ++j) {
      if (t + j < ntiles) {
        process(t + j, a[j], sc[j]);
        if (t + j + kRing < ntiles) load_tile(a[j], sc[j], t + j + kRing);
      }
    }
  }
  if (__ballot(qn > 0) != 0ull) flush();

  // this (query, split)'s sorted list, padded with (-inf, -1)
  for (int rr = 0; rr < rows_lds; ++rr) {
    if (r0 + rr >= p.nq) break;
    const int m_r = __builtin_amdgcn_readlane(m, rr);
    const float* Ls = smem + rr * RS;
    const int* Li = reinterpret_cast<const int*>(Ls + k);
    const int64_t o = ((r0 + rr) * p.nsplit + split) * (int64_t)k;
    for (int e = lane; e < k; e += 64) {
      p.ws_s[o + e] = e < m_r ? Ls[e] : -__builtin_inff();
      p.ws_i[o + e] = e < m_r ? Li[e] : -1;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- stage 2
struct FinArgs {
  const float* q;
  const float* c;               // re-rank only
  const float* cand_s;          // [nq][k1] keys, sorted; padding (-inf, -1) is a suffix
  const int64_t* cand_i;
  const float* qscale;          // [nq]
  int k, k1;
  float* out_s;                 // [nq][k]
  int64_t* out_i;
};

// without c (k1 == k): the stage-1 order, scores key * qscale
__global__ __launch_bounds__(64) void i8_scale_kernel(FinArgs p) {
  const int64_t qrow = blockIdx.x;
  const float qscale = p.qscale[qrow];
  for (int e = threadIdx.x; e < p.k; e += 64) {
    const int64_t i = p.cand_i[qrow * p.k1 + e];
    p.out_s[qrow * p.k + e] = i >= 0 ? p.cand_s[qrow * p.k1 + e] * qscale : -__builtin_inff();
    p.out_i[qrow * p.k + e] = i >= 0 ? i : -1;
  }
}

// with c: exact f32 scores of the k1 candidates (topk_select_kernel's MFMA chain per pair), best k by counting
template <int D>
__global__ __launch_bounds__(64) void i8_rerank_kernel(FinArgs p) {
  constexpr int NG = D / 8;
  __shared__ float S[TT_TOPK_MAX_K];
  __shared__ int I[TT_TOPK_MAX_K];
  const int lane = threadIdx.x;
  const int h = lane >> 5;
  const int ln = lane & 31;
  const int64_t qrow = blockIdx.x;
  const int k = p.k, k1 = p.k1;
  const int64_t* ci = p.cand_i + qrow * k1;
  const int ntiles = __builtin_amdgcn_readfirstlane((k1 + 31) >> 5);

  // the query in every column of B: rf[g] = q[qrow][8g + 4h .. +3]
  f32x4 rf[NG];
  {
    const f32x4* R4 = reinterpret_cast<const f32x4*>(p.q + qrow * D) + h;
#pragma unroll
    for (int g = 0; g < NG; ++g) rf[g] = R4[2 * g];
  }
  for (int t = 0; t < ntiles; ++t) {
    const int e = 32 * t + ln;
    const int id = e < k1 ? (int)ci[e] : -1;
    const f32x4* src = reinterpret_cast<const f32x4*>(p.c + (int64_t)(id >= 0 ? id : 0) * D) + h;
    f32x4 a[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) a[g] = src[2 * g];
    f32x16 X;
#pragma unroll
    for (int i = 0; i < 16; ++i) X[i] = 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      X = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g][0], rf[g][0], X, 0, 0, 0);
      X = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g][1], rf[g][1], X, 0, 0, 0);
      X = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g][2], rf[g][2], X, 0, 0, 0);
      X = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g][3], rf[g][3], X, 0, 0, 0);
    }
    // column 0 (lanes 0 and 32) holds score(query, candidate 32 t + acc_row(reg, h))
    if (ln == 0) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) S[32 * t + tt::acc_row(reg, h)] = X[reg];
    }
    if (h == 0) I[e] = id;
  }
  __syncthreads();
  int nv = 0;                                                // valid candidates: padding (index -1) is a suffix
  {
    int lo = 0, hi = k1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (I[mid] >= 0) lo = mid + 1; else hi = mid;
    }
    nv = lo;
  }
  for (int e = lane; e < nv; e += 64) {
    const float s = S[e];
    const int i = I[e];
    int rank = 0;
    for (int j = 0; j < nv; ++j) rank += beats(S[j], I[j], s, i) ? 1 : 0;
    if (rank < k) {
      p.out_s[qrow * k + rank] = s;
      p.out_i[qrow * k + rank] = i;
    }
  }
  for (int pos = nv + lane; pos < k; pos += 64) {
    p.out_s[qrow * k + pos] = -__builtin_inff();
    p.out_i[qrow * k + pos] = -1;
  }
}

template <int D>
int launch_scan(const ScanArgs& a, int64_t blocks, hipStream_t stream) {
  return tt::topk::launch_select("topk_i8_scan", i8_scan_kernel<D>, tt::topk::select_lds_bytes(a.rows_lds, a.k), blocks, stream, a,
                                 "tt_retrieval_topk_i8_f32");
}

template <int D>
int launch_quantize(const QuantArgs& a, hipStream_t stream) {
  constexpr int rows = kQuantThreads / (D / 4);
  tt::launch("quantize_i8", i8_quantize_kernel<D>, dim3((unsigned)((a.n + rows - 1) / rows)), dim3(kQuantThreads), 0u, stream, a);
  return tt::check_launch("quantize_i8");
}

}  // namespace

int tt::i8_finish_launch(const float* q, const float* c, const float* cand_s, const int64_t* cand_i, const float* qscale, int64_t nq,
                         int dim, int k, int k1, float* out_scores, int64_t* out_idx, hipStream_t stream) {
  FinArgs f{};
  f.q = q; f.c = c; f.cand_s = cand_s; f.cand_i = cand_i; f.qscale = qscale; f.k = k; f.k1 = k1;
  f.out_s = out_scores; f.out_i = out_idx;
  if (c == nullptr) {
    tt::launch("topk_i8_scale", i8_scale_kernel, dim3((unsigned)nq), dim3(64), 0u, stream, f);
    return tt::check_launch("topk_i8_scale");
  }
  switch (dim) {
    case 32: tt::launch("topk_i8_rerank", i8_rerank_kernel<32>, dim3((unsigned)nq), dim3(64), 0u, stream, f); break;
    case 64: tt::launch("topk_i8_rerank", i8_rerank_kernel<64>, dim3((unsigned)nq), dim3(64), 0u, stream, f); break;
    case 128: tt::launch("topk_i8_rerank", i8_rerank_kernel<128>, dim3((unsigned)nq), dim3(64), 0u, stream, f); break;
    default: tt::launch("topk_i8_rerank", i8_rerank_kernel<256>, dim3((unsigned)nq), dim3(64), 0u, stream, f); break;
  }
  return tt::check_launch("topk_i8_rerank");
}

extern "C" int tt_quantize_rows_i8(const float* x, int64_t n, int32_t dim, int8_t* codes, float* scales, tt_stream_t stream_) {
  const char* fn = "tt_quantize_rows_i8";
  TT_REQUIRE(x && codes && scales, "%s: null pointer", fn);
  TT_REQUIRE(n > 0 && n <= INT32_MAX, "%s: n %lld not in [1, 2^31 - 1]", fn, (long long)n);
  TT_REQUIRE(dim == 32 || dim == 64 || dim == 128 || dim == 256, "%s: dim %d not in {32,64,128,256}", fn, dim);
  TT_REQUIRE(tt::aligned16(x) && tt::aligned16(codes), "%s: x / codes must be 16-byte aligned", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(scales) & 3u) == 0, "%s: scales must be 4-byte aligned", fn);
  hipStream_t stream = tt::as_stream(stream_);
  QuantArgs a{x, n, codes, scales};
  switch (dim) {
    case 32: return launch_quantize<32>(a, stream);
    case 64: return launch_quantize<64>(a, stream);
    case 128: return launch_quantize<128>(a, stream);
    default: return launch_quantize<256>(a, stream);
  }
}

extern "C" int64_t tt_retrieval_topk_i8_workspace_bytes(int64_t nq, int64_t nc, int32_t dim, int32_t k, int32_t k1) {
  if (!shape_ok(nq, nc, dim, k, k1)) return 0;
  return i8_plan(nq, nc, k1).total;
}

extern "C" int tt_retrieval_topk_i8_f32(const float* q, const int8_t* codes, const float* scales, const float* c, int64_t nq,
                                        int64_t nc, int32_t dim, int32_t k, int32_t k1, const int64_t* excl_offsets,
                                        const int64_t* excl_idx, void* workspace, int64_t workspace_bytes, float* out_scores,
                                        int64_t* out_idx, tt_stream_t stream_) {
  const char* fn = "tt_retrieval_topk_i8_f32";
  TT_REQUIRE(q && codes && scales && workspace && out_scores && out_idx, "%s: null pointer", fn);
  TT_REQUIRE((excl_offsets == nullptr) == (excl_idx == nullptr), "%s: excl_offsets and excl_idx must be given together", fn);
  TT_REQUIRE(nq > 0 && nc > 0, "%s: nq and nc must be positive", fn);
  TT_REQUIRE(nc <= INT32_MAX, "%s: nc %lld exceeds 2^31 - 1 candidates", fn, (long long)nc);
  TT_REQUIRE(dim == 32 || dim == 64 || dim == 128 || dim == 256, "%s: dim %d not in {32,64,128,256}", fn, dim);
  TT_REQUIRE(k >= 1, "%s: k %d must be positive", fn, k);
  TT_REQUIRE(k <= k1, "%s: k %d exceeds k1 %d", fn, k, k1);
  TT_REQUIRE(k1 <= TT_TOPK_MAX_K, "%s: k1 %d exceeds %d", fn, k1, TT_TOPK_MAX_K);
  TT_REQUIRE(k1 <= nc, "%s: k1 %d exceeds nc %lld", fn, k1, (long long)nc);
  TT_REQUIRE(c != nullptr || k1 == k, "%s: without c there is no re-rank: k1 %d must equal k %d", fn, k1, k);
  TT_REQUIRE(tt::aligned16(q) && tt::aligned16(codes) && tt::aligned16(c), "%s: q / codes / c must be 16-byte aligned", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(scales) & 3u) == 0, "%s: scales must be 4-byte aligned", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "%s: workspace must be 256-byte aligned", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(out_scores) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out_idx) & 7u) == 0,
             "%s: out_scores / out_idx must be aligned to their element size", fn);
  TT_REQUIRE(excl_offsets == nullptr || ((reinterpret_cast<uintptr_t>(excl_offsets) & 7u) == 0 &&
                                         (reinterpret_cast<uintptr_t>(excl_idx) & 7u) == 0),
             "%s: excl_offsets / excl_idx must be 8-byte aligned", fn);
  const I8Plan pl = i8_plan(nq, nc, k1);
  TT_REQUIRE(workspace_bytes >= pl.total, "%s: workspace %lld < %lld bytes", fn, (long long)workspace_bytes, (long long)pl.total);
  hipStream_t stream = tt::as_stream(stream_);
  tt::ProfScope scope("topk_i8", stream);
  char* ws = static_cast<char*>(workspace);
  float* a_s = reinterpret_cast<float*>(ws);
  int32_t* a_i = reinterpret_cast<int32_t*>(ws + pl.bytes_a);
  float* b_s = reinterpret_cast<float*>(ws + pl.off_b);
  int32_t* b_i = reinterpret_cast<int32_t*>(ws + pl.off_b + pl.bytes_b);
  float* cand_s = reinterpret_cast<float*>(ws + pl.off_cs);
  int64_t* cand_i = reinterpret_cast<int64_t*>(ws + pl.off_ci);
  float* qscale = reinterpret_cast<float*>(ws + pl.off_qs);

  ScanArgs a{};
  a.q = q; a.codes = codes; a.scales = scales; a.nq = nq; a.nc = nc; a.k = k1;
  a.nsplit = pl.nsplit; a.c_per_split = pl.c_per_split;
  a.rows_lds = nq < 32 ? (int)nq : 32;
  a.excl_off = excl_offsets; a.excl_idx = excl_idx;
  a.ws_s = a_s; a.ws_i = a_i; a.qscale = qscale;
  const int64_t blocks = pl.rblocks * pl.nsplit;
  int rc;
  switch (dim) {
    case 32: rc = launch_scan<32>(a, blocks, stream); break;
    case 64: rc = launch_scan<64>(a, blocks, stream); break;
    case 128: rc = launch_scan<128>(a, blocks, stream); break;
    default: rc = launch_scan<256>(a, blocks, stream); break;
  }
  if (rc != TT_OK) return rc;
  rc = tt::topk_merge_launch(nq, pl.nsplit, k1, a_s, a_i, b_s, b_i, cand_s, cand_i, stream);
  if (rc != TT_OK) return rc;

  return tt::i8_finish_launch(q, c, cand_s, cand_i, qscale, nq, dim, k, k1, out_scores, out_idx, stream);
}
