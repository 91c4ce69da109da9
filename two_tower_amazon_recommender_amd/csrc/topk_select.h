// What the four serving searches share: exact f32 top-K (topk.hip), IVF (ivf.hip), int8 top-K (topk_i8.hip) and int8 IVF
// (ivf_i8.hip).  One wave streams candidate rows [c_begin, c_end) against up to 32 query rows held in registers and leaves,
// for every query row, its sorted list of the k best candidates (key descending, ties to the lower candidate id) in the
// workspace.
//   * topk::Select, the selection core: per-row state, push (range check, threshold, exclusions, enqueue), flush (the
//     rank-based merge) and write_out.  The tie rule, the queue-overflow trigger and the threshold update exist here only.
//   * topk::select_run, the f32 tile stream on top of it (load, MFMA, two-buffer prefetch) with the row index as the
//     candidate id: the whole body of topk_select_kernel.
//   * topk::select_run_ids, ivf_select_kernel's body: the scheme as a template of its own, not yet on Select (see there;
//     neither are the int8 scans of topk_i8.hip and ivf_i8.hip, which carry their own bodies).
//   * the corpus-split work-item decode, align256, the select launcher (all four select kernels), the merge launcher and
//     the top-K launch path.
// The scheme (LDS list / survivor queue / register threshold, rank-based merges) is described in topk.hip.
#pragma once
#include "common.h"
#include <climits>

namespace tt {

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

namespace topk {

constexpr int kQueue = 48;               // survivor slots per query row (a tile adds at most 32)
constexpr int kMaxEntries = (TT_TOPK_MAX_K + kQueue + 63) / 64;   // (list + queue) entries per lane in a merge
constexpr int kMergeFan = 16;
constexpr int kMergeThreads = 256;

__device__ __forceinline__ bool beats(float as, int ai, float bs, int bi) { return as > bs || (as == bs && ai < bi); }
// the same rule without short-circuit evaluation, for the per-tile test of 16 candidates per lane: three compares cost
// less there than the branches that would skip two of them
__device__ __forceinline__ bool beats_flat(float as, int ai, float bs, int bi) {
  return ((int)(as > bs) | ((int)(as == bs) & (int)(ai < bi))) != 0;
}

// LDS bytes of the selection state for `rows` query rows
inline int select_lds_bytes(int rows, int k) { return rows * 2 * (k + kQueue) * 4; }

// The selection state of one wave: lane (ln, h) serves query row ln (lanes ln and ln + 32 hold the same copy of the row's
// state), and a tile is one 32x32 MFMA accumulator, lane (ln, h) holding the keys of query ln against candidate rows
// c0 + acc_row(reg, h), reg < 16.  LDS per query row: list keys [k], list ids [k], queue keys [kQueue], queue ids [kQueue].
struct Select {
  float* lds;
  int k, RS;                    // RS: LDS words per query row
  int rows_lds;                 // wave-uniform: rows with LDS state (the valid rows are a prefix)
  int lane, h, ln;
  bool r_ok;                    // this lane's query row exists
  int64_t ex_lo, ex_hi;         // this row's exclusion segment of excl_idx (sorted ascending; candidate ids)
  const int64_t* excl_idx;
  int m, qn;                    // list length, queue length
  bool full;
  float thr_s;                  // the list's k-th entry once it is full
  int thr_i;
  float* qs;                    // this row's queue
  int* qi;

  // excl_off / excl_idx: the exclusion CSR (both null: none); qid: this lane's query (read where r_ok)
  __device__ __forceinline__ void init(float* lds_base, int k_, int rows_lds_, bool r_ok_, int lane_, const int64_t* excl_off,
                                       const int64_t* excl_idx_, int64_t qid) {
    lds = lds_base; k = k_; RS = 2 * (k_ + kQueue);
    rows_lds = __builtin_amdgcn_readfirstlane(rows_lds_);
    lane = lane_; h = lane_ >> 5; ln = lane_ & 31; r_ok = r_ok_;
    ex_lo = 0; ex_hi = 0; excl_idx = excl_idx_;
    if (excl_off != nullptr && r_ok) {
      ex_lo = excl_off[qid];
      ex_hi = excl_off[qid + 1];
    }
    m = 0; qn = 0; full = false; thr_s = 0.f; thr_i = 0;
    float* row = lds + (r_ok ? ln : 0) * RS;
    qs = row + 2 * k;
    qi = reinterpret_cast<int*>(row + 2 * k + kQueue);
  }

  __device__ __forceinline__ bool excluded(int64_t cand) const {
    int64_t lo = ex_lo, hi = ex_hi;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (excl_idx[mid] < cand) lo = mid + 1; else hi = mid;
    }
    return lo < ex_hi && excl_idx[lo] == cand;
  }

  // the candidate ids of a tile whose ids are its row indices
  struct RowIds {
    int64_t c0;
    int h;
    __device__ __forceinline__ int operator[](int reg) const { return (int)(c0 + tt::acc_row(reg, h)); }
  };
  __device__ __forceinline__ RowIds row_ids(int64_t c0) const { return RowIds{c0, h}; }

  // One tile: key[reg] / id[reg] belong to candidate row c0 + acc_row(reg, h); rows at or past c_end are ignored.  The
  // caller fetches ids (and scales) that live in other lanes BEFORE the call, with every lane active: a shuffle inside the
  // divergent code below would read inactive source lanes as 0.  Called by the whole wave.
  template <class Keys, class Ids>
  __device__ __forceinline__ void push(const Keys& key, const Ids& id, int64_t c0, int64_t c_end) {
    // rows of the tile inside the range: wave-uniform, below 32 only on a range's last tile
    const int nrows = c_end - c0 < 32 ? (int)(c_end - c0) : 32;
    uint32_t mask = 0;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {           // branch-free: 32-bit compares and mask logic only
      const int ok = (int)r_ok & (int)(tt::acc_row(reg, h) < nrows) &
                     ((int)!full | (int)beats_flat(key[reg], id[reg], thr_s, thr_i));
      mask |= ok ? (1u << reg) : 0u;
    }
    if (ex_hi > ex_lo && mask != 0u) {             // survivors only, so long exclusion lists cost almost nothing
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
        if (((mask >> reg) & 1u) && excluded(id[reg])) mask &= ~(1u << reg);
    }
    const int n = __builtin_popcount(mask);
    const int n_other = __shfl_xor(n, 32);
    int pos = qn + (h ? n_other : 0);              // half 0's survivors first, then half 1's
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
      if ((mask >> reg) & 1u) {
        qs[pos] = key[reg];
        qi[pos] = id[reg];
        ++pos;
      }
    qn += n + n_other;
    if (__ballot(qn > kQueue - 32) != 0ull) flush();   // some row's queue could overflow on the next tile
  }

  // merge every non-empty queue into its row's list (wave-cooperative; called on wave-uniform control only): an entry's new
  // position is its rank in (list + queue) under the total order
  __device__ __forceinline__ void flush() {
    for (int rr = 0; rr < rows_lds; ++rr) {
      const int qn_r = __builtin_amdgcn_readlane(qn, rr);
      const int m_r = __builtin_amdgcn_readlane(m, rr);
      if (qn_r == 0) continue;
      float* Ls = lds + rr * RS;
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
  }

  // The last flush, then every valid row's sorted list padded with (-inf, -1): row rr's at ws_*[out_off(rr)].
  // out_off(rr): element offset, or < 0 past the last valid row (wave-uniform)
  template <class OutOff>
  __device__ __forceinline__ void write_out(float* ws_s, int32_t* ws_i, OutOff out_off) {
    if (__ballot(qn > 0) != 0ull) flush();
    for (int rr = 0; rr < rows_lds; ++rr) {
      const int64_t o = out_off(rr);
      if (o < 0) break;
      const int m_r = __builtin_amdgcn_readlane(m, rr);
      const float* Ls = lds + rr * RS;
      const int* Li = reinterpret_cast<const int*>(Ls + k);
      for (int e = lane; e < k; e += 64) {
        ws_s[o + e] = e < m_r ? Ls[e] : -__builtin_inff();
        ws_i[o + e] = e < m_r ? Li[e] : -1;
      }
    }
  }
};

// What a select kernel hands to select_run
struct Stream {
  const float* qrow;            // this lane's query row (read where r_ok)
  int64_t qid;                  // its query index (the row of excl_off; read where r_ok)
  bool r_ok;                    // lane ln holds query row ln of the wave (lanes ln and ln + 32 agree)
  int rows_lds;                 // wave-uniform: rows with LDS state (the valid rows are a prefix)
  int k;
  const int64_t* excl_off;      // nullable, with excl_idx
  const int64_t* excl_idx;
  const int32_t* ids;           // IDS: original id of every candidate row
  int64_t c_begin, c_end;       // wave-uniform row range
  float* ws_s;                  // outputs: row rr's sorted list of k at ws_*[out_off(rr)]
  int32_t* ws_i;
};

// The f32 stream over candidate rows c [.., D]: out_off as Select::write_out.  Candidate ids: the row index (IDS = false,
// topk_select_kernel) or p.ids[row] (IDS = true: the form ivf_select_kernel takes once it meets the speed rule on Select;
// no kernel instantiates it yet)
template <int D, bool IDS, class OutOff>
__device__ __forceinline__ void select_run(const Stream& p, const float* c, OutOff out_off) {
  constexpr int NG = D / 8;                         // k-groups of 8 (4 per lane half), as score_kernel's GEMM1
  constexpr bool PREFETCH = D <= 128;               // dim 256: the rows (128 VGPRs) and one tile (128) fill the budget
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x;
  const int h = lane >> 5;
  const int ln = lane & 31;
  const bool r_ok = p.r_ok;
  const int64_t c_begin = p.c_begin;
  const int64_t c_end = p.c_end;
  // every quantity that steers a loop with a barrier in it is wave-uniform by construction (readfirstlane)
  const int ntiles = __builtin_amdgcn_readfirstlane((int)((c_end - c_begin + 31) >> 5));

  // stationary fragment: rf[g] = q[r][8g + 4h .. +3]
  f32x4 rf[NG];
  {
    const f32x4* R4 = reinterpret_cast<const f32x4*>(p.qrow) + h;
#pragma unroll
    for (int g = 0; g < NG; ++g) rf[g] = r_ok ? R4[2 * g] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  Select sel;
  sel.init(smem, p.k, p.rows_lds, r_ok, lane, p.excl_off, p.excl_idx, p.qid);

  // a tile: lane (ln, h) loads half h of candidate row c0 + ln (and, IDS, that row's id)
  auto load_tile = [&](f32x4 (&a)[NG], int& id, int t) {
    const int64_t cand = c_begin + 32 * (int64_t)t + ln;
    const bool ok = cand < c_end;
    const f32x4* src = reinterpret_cast<const f32x4*>(c + (ok ? cand : 0) * D) + h;
#pragma unroll
    for (int g = 0; g < NG; ++g) a[g] = ok ? src[2 * g] : f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (IDS) id = ok ? p.ids[cand] : 0;
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
    // X[reg] = score(query r, candidate row c0 + acc_row(reg, h)); IDS: the id of that row comes from the lane that loaded it
    const int64_t c0 = c_begin + 32 * (int64_t)t;
    if constexpr (IDS) {
      int idr[16];
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) idr[reg] = __shfl(id, tt::acc_row(reg, h));
      sel.push(X, idr, c0, c_end);
    } else {
      sel.push(X, sel.row_ids(c0), c0, c_end);
    }
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
  sel.write_out(p.ws_s, p.ws_i, out_off);
}

// The work item of a corpus-split select kernel: grid = (32-query row block) x (corpus split)
struct SplitWork {
  int split;
  int64_t r0;                   // first query row of the block
  int64_t c_begin, c_end;
};
__device__ __forceinline__ SplitWork split_work(int nsplit, int64_t c_per_split, int64_t nc) {
  SplitWork w;
  w.split = __builtin_amdgcn_readfirstlane((int)(blockIdx.x % (unsigned)nsplit));
  w.r0 = (int64_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x / (unsigned)nsplit)) * 32;
  w.c_begin = (int64_t)w.split * c_per_split;
  w.c_end = w.c_begin + c_per_split;
  if (w.c_end > nc) w.c_end = nc;
  return w;
}

// ivf_select_kernel's body: the same scheme as a template of its own, as it was before Select existed (IDS = true: the
// candidate id is ids[row]; the ids of a chunk must be distinct).  It is not yet on Select: there the kernel measured
// 0.4-1.5 % slower on the large-batch shapes of bench_ivf.py (profiles/retrieval_select_core_ab.jsonl), and so did the two
// int8 scans on some of theirs, which keep their own bodies in topk_i8.hip and ivf_i8.hip.  A fix to the tie rule, the
// overflow trigger or the threshold update goes into Select AND into these three.
struct ListStream {
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
__device__ __forceinline__ void select_run_ids(const ListStream& p, OutOff out_off) {
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

// Launch a one-wave-per-workgroup select kernel with lds_bytes of dynamic LDS; above the 64 KiB default the limit must be
// raised first (cheap, idempotent).  entry: the calling entry point, for the error message.
template <class Kern, class Args>
int launch_select(const char* name, Kern kernel, int lds_bytes, int64_t blocks, hipStream_t stream, const Args& args,
                  const char* entry) {
  if (lds_bytes > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess)
    return tt::fail(TT_ERR_LAUNCH, "%s: hipFuncSetAttribute(LDS %d) failed", entry, lds_bytes);
  tt::launch(name, kernel, dim3((unsigned)blocks), dim3(64), (unsigned)lds_bytes, stream, args);
  return tt::check_launch(name);
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
