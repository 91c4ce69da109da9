// The score-and-select scheme of topk.hip (exact top-K over the corpus) as a template with an id hook, for ivf.hip
// (top-K over inverted lists), plus the pieces both files share: constants, the tie rule, the merge launcher and the
// top-K launch path.  One wave streams candidate rows [c_begin, c_end) of c against up to 32 query rows held in registers
// and leaves, for every query row, its sorted list of the k best candidates (score descending, ties to the lower candidate
// id) in the workspace.  The scheme (LDS list / survivor queue / register threshold, rank-based merges) is described in
// topk.hip, whose topk_select_kernel keeps its own copy of this body: compiled from this template it allocated registers
// differently and ran 2-4 % slower in a same-box A/B.
// Candidate ids: the row index itself (IDS = false) or ids[row] (IDS = true: the ids of a chunk must be distinct).
#pragma once
#include "common.h"
#include <climits>

namespace tt {
namespace topk {

constexpr int kQueue = 48;               // survivor slots per query row (a tile adds at most 32)
constexpr int kMaxEntries = (TT_TOPK_MAX_K + kQueue + 63) / 64;   // (list + queue) entries per lane in a merge
constexpr int kMergeFan = 16;
constexpr int kMergeThreads = 256;

__device__ __forceinline__ bool beats(float as, int ai, float bs, int bi) { return as > bs || (as == bs && ai < bi); }

// LDS bytes of the selection state for `rows` query rows
inline int select_lds_bytes(int rows, int k) { return rows * 2 * (k + kQueue) * 4; }

struct Stream {
  const float* qrow;            // this lane's query row (read where r_ok)
  bool r_ok;                    // lane ln holds query row ln of the wave (lanes ln and ln + 32 agree)
  int rows_lds;                 // wave-uniform: rows with LDS state (the valid rows are a prefix)
  int k;
  int64_t ex_lo, ex_hi;         // this row's exclusion segment of excl_idx (sorted ascending; candidate ids)
  const int64_t* excl_idx;
  const float* c;               // candidate rows
  const int32_t* ids;           // IDS: original id of every row
  int64_t c_begin, c_end;       // wave-uniform row range
  float* ws_s;                  // outputs: row rr's sorted list of k at ws_*[out_off(rr)]
  int32_t* ws_i;
};

// out_off(rr): element offset of query row rr's output list, or < 0 past the last valid row (wave-uniform)
template <int D, bool IDS, class OutOff>
__device__ __forceinline__ void select_run(const Stream& p, OutOff out_off) {
  constexpr int NG = D / 8;                         // k-groups of 8 (4 per lane half), as score_kernel's GEMM1
  constexpr bool PREFETCH = D <= 128;               // dim 256: the rows (128 VGPRs) and one tile (128) fill the budget
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x;
  const int h = lane >> 5;
  const int ln = lane & 31;
  const int k = p.k;
  const int RS = 2 * (k + kQueue);                  // LDS words per query row: list scores, list indices, queue scores, queue indices
  const int rows_lds = __builtin_amdgcn_readfirstlane(p.rows_lds);
  const bool r_ok = p.r_ok;
  const int64_t c_begin = p.c_begin;
  const int64_t c_end = p.c_end;
  const int ntiles = __builtin_amdgcn_readfirstlane((int)((c_end - c_begin + 31) >> 5));

  // stationary fragment: rf[g] = q[r][8g + 4h .. +3]
  f32x4 rf[NG];
  {
    const f32x4* R4 = reinterpret_cast<const f32x4*>(p.qrow) + h;
#pragma unroll
    for (int g = 0; g < NG; ++g) rf[g] = r_ok ? R4[2 * g] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int64_t ex_lo = p.ex_lo, ex_hi = p.ex_hi;
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

  // a tile: lane (ln, h) loads half h of candidate row c0 + ln (and, IDS, that row's id)
  auto load_tile = [&](f32x4 (&a)[NG], int& id, int t) {
    const int64_t cand = c_begin + 32 * (int64_t)t + ln;
    const bool ok = cand < c_end;
    const f32x4* src = reinterpret_cast<const f32x4*>(p.c + (ok ? cand : 0) * D) + h;
#pragma unroll
    for (int g = 0; g < NG; ++g) a[g] = ok ? src[2 * g] : f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (IDS) id = ok ? p.ids[cand] : 0;
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

  auto process = [&](int t, const f32x4 (&a)[NG], int id) {
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
    // X[reg] = score(query r, candidate row c0 + acc_row(reg, h))
    const int64_t c0 = c_begin + 32 * (int64_t)t;
    // IDS: the id of row acc_row(reg, h) comes from the lane that loaded it; the shuffles run here, with every lane active
    // (a shuffle inside the divergent code below would read inactive source lanes as 0)
    int idr[IDS ? 16 : 1];
    if constexpr (IDS) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) idr[reg] = __shfl(id, tt::acc_row(reg, h));
    }
    auto cand_id = [&](int reg) -> int64_t {
      if constexpr (IDS) return idr[reg];
      else return c0 + tt::acc_row(reg, h);
    };
    uint32_t mask = 0;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int64_t cand = c0 + tt::acc_row(reg, h);
      const bool ok = r_ok && cand < c_end && (!full || beats(X[reg], (int)cand_id(reg), thr_s, thr_i));
      mask |= ok ? (1u << reg) : 0u;
    }
    if (ex_hi > ex_lo && mask != 0u) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
        if (((mask >> reg) & 1u) && excluded(cand_id(reg))) mask &= ~(1u << reg);
    }
    const int n = __builtin_popcount(mask);
    const int n_other = __shfl_xor(n, 32);
    int pos = qn + (h ? n_other : 0);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
      if ((mask >> reg) & 1u) {
        qs[pos] = X[reg];
        qi[pos] = (int)cand_id(reg);
        ++pos;
      }
    qn += n + n_other;
    if (__ballot(qn > kQueue - 32) != 0ull) flush();
  };

  f32x4 a0[NG];
  int id0 = 0;
  if (ntiles > 0) load_tile(a0, id0, 0);
  if constexpr (PREFETCH) {
    f32x4 a1[NG];
    int id1 = 0;
    for (int t = 0; t < ntiles; t += 2) {
      if (t + 1 < ntiles) load_tile(a1, id1, t + 1);
      process(t, a0, id0);
      if (t + 1 < ntiles) {
        if (t + 2 < ntiles) load_tile(a0, id0, t + 2);
        process(t + 1, a1, id1);
      }
    }
  } else {
    for (int t = 0; t < ntiles; ++t) {
      if (t > 0) load_tile(a0, id0, t);
      process(t, a0, id0);
    }
  }
  if (__ballot(qn > 0) != 0ull) flush();

  // every valid row's sorted list, padded with (-inf, -1)
  for (int rr = 0; rr < rows_lds; ++rr) {
    const int64_t o = out_off(rr);
    if (o < 0) break;
    const int m_r = __builtin_amdgcn_readlane(m, rr);
    const float* Ls = smem + rr * RS;
    const int* Li = reinterpret_cast<const int*>(Ls + k);
    for (int e = lane; e < k; e += 64) {
      p.ws_s[o + e] = e < m_r ? Ls[e] : -__builtin_inff();
      p.ws_i[o + e] = e < m_r ? Li[e] : -1;
    }
  }
}

}  // namespace topk

// The merge rounds of topk.hip (topk_merge_kernel) over nl sorted lists of k per query, disjoint in candidates, padding a
// suffix: buffer a ([nq][nl][k] scores / indices) holds the input, buffer b the intermediate rounds (merge_b_bytes), the
// last round writes out_s / out_i [nq][k].  Launches only.
int topk_merge_rounds_count(int64_t nl);
int64_t topk_merge_b_bytes(int64_t nq, int64_t nl, int k);           // one array of buffer b (256-byte multiple)
int topk_merge_launch(int64_t nq, int nl, int k, float* a_s, int32_t* a_i, float* b_s, int32_t* b_i, float* out_s,
                      int64_t* out_i, hipStream_t stream);

// tt_retrieval_topk_f32's launches (arguments already validated) with at least min_cols candidates per corpus split instead
// of the entry point's 512; the answer does not depend on the split.  Workspace: topk_workspace_bytes_split.
int64_t topk_workspace_bytes_split(int64_t nq, int64_t nc, int k, int min_cols);
int topk_run(const float* q, const float* c, int64_t nq, int64_t nc, int dim, int k, const int64_t* excl_offsets,
             const int64_t* excl_idx, void* workspace, float* out_scores, int64_t* out_idx, hipStream_t stream, int min_cols);


// tt_ivf_search_f32's first two launches (ivf.hip), shared with ivf_i8.hip: the coarse probe over the centroids and
// ivf_bucket_kernel, into the leading `bytes` of the workspace.  The plan holds the chunk rule too (S chunks per list, chosen
// for lists of list_k entries per (query, probe, chunk)), so both searches cut lists alike.
struct IvfProbePlan {
  int S;                        // chunks per list
  int nl;                       // lists per query entering the merge: nprobe * S
  int64_t grid;                 // upper bound of the (list, chunk, query tile) work items
  int64_t off_probe_s, off_probe_i, off_cnt, off_pstart, off_tstart, off_pairs;   // byte offsets (the coarse top-k's own
  int64_t bytes;                                                                  // workspace leads); 256-byte multiple
};
IvfProbePlan ivf_probe_plan(int64_t nq, int64_t nlist, int64_t n, int list_k, int nprobe);
int ivf_probe_bucket(const float* q, const float* centroids, int64_t nq, int64_t nlist, int dim, int nprobe,
                     const IvfProbePlan& pl, void* workspace, hipStream_t stream);

}  // namespace tt
