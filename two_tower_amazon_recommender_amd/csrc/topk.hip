// Exact top-K retrieval: the K best candidates of every query over the whole corpus, fused onto the scorer's f32 MFMA
// tile loop (tfrs.layers.factorized_top_k.BruteForce semantics).  The [nq x nc] score matrix never reaches HBM.
//
// Contract (tt_retrieval_topk_f32, include/twotower_hip.h):
//   q [nq, D], c [nc, D] f32, 16-byte aligned; nq >= 1, 1 <= nc < 2^31, D in {32, 64, 128, 256}, 1 <= k <= TT_TOPK_MAX_K,
//   k <= nc.  score[i][j] = q_i . c_j (plain dot product: no temperature, no bias).
//   out_scores f32 [nq, k], out_idx int64 [nq, k]: score descending, EQUAL SCORES GO TO THE LOWER CANDIDATE INDEX FIRST
//   (also at the cut at position k), so the answer is unique.
//   Exclusions (optional, both pointers or neither): CSR excl_offsets int64 [nq + 1], excl_idx int64, each query's segment
//   sorted ascending; duplicates and values outside [0, nc) are allowed and match nothing.  An excluded candidate never
//   enters a list: the result is the exact top-K of the remaining candidates, and when fewer than k remain the tail is
//   padded with (-inf, -1).
//   Determinism: the f32 score of a pair is the same MFMA chain (k-order fixed per output element) whatever nq, the pair's
//   position in the batch, the split count or k - a query's answer is bit-identical alone or in a batch, run to run.
//
// Launch 1, score-and-select (topk_select_kernel): one wave per workgroup, grid = (32-query row block) x (corpus split).
//   The wave holds its 32 queries' rows in registers (the B operand of v_mfma_f32_32x32x2_f32, as score_kernel's GEMM1)
//   and streams its split's candidates 32 at a time straight from global memory into the A operand (one tile prefetched in
//   registers ahead of the MFMAs at D <= 128; no LDS tile, so LDS holds only the selection state).  Lane (ln, h) ends a
//   tile with the scores of query ln against candidates c0 + acc_row(reg, h), reg < 16.
//   Selection per query row, in LDS: a sorted list of the best m <= k so far and a queue of kQueue survivors.  A candidate
//   survives when the list is not yet full or it beats the list's k-th entry (the threshold, held in registers), and is not
//   excluded (binary search over the query's segment - survivors only, so long exclusion lists cost almost nothing).
//   Survivors append to the row's queue; when any row's queue could overflow on the next tile (a ballot: wave-uniform), the
//   wave merges every non-empty queue into its list: each entry's new position = its rank in (list + queue) under the total
//   order (score desc, index asc) - list entries count the queue entries that beat them, queue entries binary-search the
//   list and count the queue - and entries of rank < k are written to that position.  After the first k candidates the
//   threshold rises quickly, survivors are ~k ln(n/k) of a split's n candidates, and the merges become rare.
//   Each (query, split) writes its sorted list of k (padded with (-inf, -1)) to the workspace.
//   The code is in topk_select.h: the selection is topk::Select (state, push, flush, write_out) and the kernel below is
//   its work-item decode around topk::select_run, the f32 tile stream on that core.  Select's per-tile test is branch-free
//   and does no 64-bit arithmetic; on it the kernel measured 0.8-8 % faster than its former hand-written body on every
//   shape of bench_topk.py (profiles/retrieval_select_core_ab.jsonl).  The IVF and int8 select kernels still carry bodies
//   of their own (topk::select_run_ids, topk_i8.hip, ivf_i8.hip): on Select they were slower on some shapes.
// Launch 2.., merge (topk_merge_kernel): one 256-thread workgroup per (query, group of kMergeFan lists) loads the group into
//   LDS; every entry's rank in the merged order = its position + the number of entries of each other list that beat it
//   (binary search); ranks < k are written.  Lists come from disjoint candidate ranges, so the ranks are unique and dense.
//   ceil(log16(nsplit)) launches: 1 for nsplit <= 16, 3 for the 2048 splits of a serving call.  The last writes the outputs.
//
// LDS: launch 1 keeps min(nq, 32) rows x (k + kQueue) x (f32 score + int32 index): 38 KB at k = 100 (4 waves per CU), 78 KB
// at k = 256.  Launch 2: kMergeFan x k x 8 B <= 32 KB.  Split rule (topk_plan): enough (row block x split) waves for the
// whole chip (kTargetWaves) - past the scorer's 64-split cap when nq is small - but at least kMinColsPerSplit candidates per
// split.  It reads no environment variable.
#include "topk_select.h"

namespace {

using tt::align256;
using tt::topk::beats;
using tt::topk::kMergeFan;
using tt::topk::kMergeThreads;

constexpr int kTargetWaves = 2048;       // 256 CUs x 8
constexpr int kMinColsPerSplit = 512;
constexpr int kMaxSplits = 4096;

struct TopkPlan {
  int64_t rblocks;        // 32-query row blocks
  int nsplit;
  int64_t c_per_split;    // multiple of 32
  int rounds;             // merge launches
  int64_t off_b;          // workspace: buffer A at 0 ([nq][nsplit][k] scores, then indices), buffer B here
  int64_t total;
};

TopkPlan topk_plan(int64_t nq, int64_t nc, int k, int min_cols = kMinColsPerSplit) {
  TopkPlan p{};
  p.rblocks = (nq + 31) / 32;
  int64_t ns = (kTargetWaves + p.rblocks - 1) / p.rblocks;
  const int64_t by_cols = (nc + min_cols - 1) / min_cols;
  if (ns > by_cols) ns = by_cols;
  if (ns > kMaxSplits) ns = kMaxSplits;
  if (ns < 1) ns = 1;
  int64_t cps = (nc + ns - 1) / ns;
  cps = (cps + 31) & ~(int64_t)31;
  p.c_per_split = cps;
  p.nsplit = (int)((nc + cps - 1) / cps);
  p.rounds = tt::topk_merge_rounds_count(p.nsplit);
  const int64_t bytes_a = align256(nq * p.nsplit * (int64_t)k * 4);         // one array (scores or indices)
  const int64_t bytes_b = tt::topk_merge_b_bytes(nq, p.nsplit, k);
  p.off_b = 2 * bytes_a;
  p.total = 2 * bytes_a + 2 * bytes_b;
  return p;
}

struct SelArgs {
  const float* q;
  const float* c;
  int64_t nq, nc;
  int k;
  int nsplit;
  int64_t c_per_split;
  int rows_lds;                 // query rows with LDS state: min(nq, 32)
  const int64_t* excl_off;      // nullable
  const int64_t* excl_idx;
  float* ws_s;                  // [nq][nsplit][k]
  int32_t* ws_i;
};

template <int D>
__global__ __launch_bounds__(64) void topk_select_kernel(SelArgs p) {
  const tt::topk::SplitWork w = tt::topk::split_work(p.nsplit, p.c_per_split, p.nc);
  const int64_t r = w.r0 + (threadIdx.x & 31);
  tt::topk::Stream s;
  s.r_ok = r < p.nq;
  s.qid = s.r_ok ? r : 0;
  s.qrow = p.q + s.qid * D;
  s.rows_lds = p.rows_lds;
  s.k = p.k;
  s.excl_off = p.excl_off;
  s.excl_idx = p.excl_idx;
  s.ids = nullptr;
  s.c_begin = w.c_begin;
  s.c_end = w.c_end;
  s.ws_s = p.ws_s;
  s.ws_i = p.ws_i;
  tt::topk::select_run<D, false>(s, p.c, [&](int rr) -> int64_t {
    // this (query, split)'s list of the [nq][nsplit][k] workspace
    return w.r0 + rr >= p.nq ? -1 : ((w.r0 + rr) * p.nsplit + w.split) * (int64_t)p.k;
  });
}

struct MergeArgs {
  int64_t nq;
  int k;
  int nl;                       // input lists per query
  int groups;                   // output lists per query (ceil(nl / kMergeFan))
  const float* in_s;            // [nq][nl][k]
  const int32_t* in_i;
  float* out_s;                 // [nq][groups][k]
  int32_t* out_i;               // (intermediate rounds)
  int64_t* out_i64;             // (last round: [nq][k])
};

__global__ __launch_bounds__(kMergeThreads) void topk_merge_kernel(MergeArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int k = p.k;
  float* Ls = smem;                                          // [kMergeFan][k]
  int* Li = reinterpret_cast<int*>(smem + kMergeFan * k);
  int* cnt = Li + kMergeFan * k;                             // real (non-padding) entries per list
  const int g = (int)(blockIdx.x % (unsigned)p.groups);
  const int64_t qrow = blockIdx.x / (unsigned)p.groups;
  const int j0 = g * kMergeFan;
  const int nj = p.nl - j0 < kMergeFan ? p.nl - j0 : kMergeFan;
  const int64_t src = (qrow * p.nl + j0) * (int64_t)k;       // the group's lists are contiguous
  for (int e = threadIdx.x; e < nj * k; e += kMergeThreads) {
    Ls[e] = p.in_s[src + e];
    Li[e] = p.in_i[src + e];
  }
  __syncthreads();
  if ((int)threadIdx.x < nj) {
    const int* L = Li + threadIdx.x * k;
    int lo = 0, hi = k;                                      // padding (index -1) is a suffix
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (L[mid] >= 0) lo = mid + 1; else hi = mid;
    }
    cnt[threadIdx.x] = lo;
  }
  __syncthreads();
  int total = 0;
  for (int j = 0; j < nj; ++j) total += cnt[j];
  const bool last = p.out_i64 != nullptr;
  const int64_t dst = (qrow * p.groups + g) * (int64_t)k;
  for (int e = threadIdx.x; e < nj * k; e += kMergeThreads) {
    const int j = e / k, pos = e - j * k;
    if (pos >= cnt[j]) continue;
    const float s = Ls[e];
    const int i = Li[e];
    int rank = pos;
    for (int jj = 0; jj < nj; ++jj) {
      if (jj == j) continue;
      const float* S = Ls + jj * k;
      const int* I = Li + jj * k;
      int lo = 0, hi = cnt[jj];
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (beats(S[mid], I[mid], s, i)) lo = mid + 1; else hi = mid;
      }
      rank += lo;
      if (rank >= k) break;
    }
    if (rank < k) {
      p.out_s[dst + rank] = s;
      if (last) p.out_i64[dst + rank] = i; else p.out_i[dst + rank] = i;
    }
  }
  for (int pos = total + threadIdx.x; pos < k; pos += kMergeThreads) {
    p.out_s[dst + pos] = -__builtin_inff();
    if (last) p.out_i64[dst + pos] = -1; else p.out_i[dst + pos] = -1;
  }
}

template <int D>
int launch_select(const SelArgs& a, int64_t blocks, hipStream_t stream) {
  return tt::topk::launch_select("topk_select", topk_select_kernel<D>, tt::topk::select_lds_bytes(a.rows_lds, a.k), blocks, stream, a,
                                 "tt_retrieval_topk_f32");
}

}  // namespace

namespace tt {

int topk_merge_rounds_count(int64_t nl) {
  int rounds = 0;
  do {
    nl = (nl + kMergeFan - 1) / kMergeFan;
    ++rounds;
  } while (nl > 1);
  return rounds;
}

int64_t topk_merge_b_bytes(int64_t nq, int64_t nl, int k) {
  const int64_t groups1 = (nl + kMergeFan - 1) / kMergeFan;
  return topk_merge_rounds_count(nl) > 1 ? align256(nq * groups1 * (int64_t)k * 4) : 0;
}

int topk_merge_launch(int64_t nq, int nl, int k, float* a_s, int32_t* a_i, float* b_s, int32_t* b_i, float* out_s,
                      int64_t* out_i, hipStream_t stream) {
  float* buf_s[2] = {a_s, b_s};
  int32_t* buf_i[2] = {a_i, b_i};
  const int rounds = topk_merge_rounds_count(nl);
  for (int round = 0; round < rounds; ++round) {
    const int groups = (nl + kMergeFan - 1) / kMergeFan;
    const bool last = round == rounds - 1;
    MergeArgs m{};
    m.nq = nq; m.k = k; m.nl = nl; m.groups = groups;
    m.in_s = buf_s[round & 1]; m.in_i = buf_i[round & 1];
    if (last) {
      m.out_s = out_s; m.out_i = nullptr; m.out_i64 = out_i;
    } else {
      m.out_s = buf_s[(round + 1) & 1]; m.out_i = buf_i[(round + 1) & 1]; m.out_i64 = nullptr;
    }
    const int lds = kMergeFan * k * 8 + kMergeFan * 4;
    tt::launch("topk_merge", topk_merge_kernel, dim3((unsigned)(nq * groups)), dim3(kMergeThreads), (unsigned)lds, stream, m);
    const int rc = tt::check_launch("topk_merge");
    if (rc != TT_OK) return rc;
    nl = groups;
  }
  return TT_OK;
}

}  // namespace tt

namespace tt {

int64_t topk_workspace_bytes_split(int64_t nq, int64_t nc, int k, int min_cols) { return topk_plan(nq, nc, k, min_cols).total; }

int topk_run(const float* q, const float* c, int64_t nq, int64_t nc, int dim, int k, const int64_t* excl_offsets,
             const int64_t* excl_idx, void* workspace, float* out_scores, int64_t* out_idx, hipStream_t stream, int min_cols) {
  const TopkPlan pl = topk_plan(nq, nc, k, min_cols);
  char* ws = static_cast<char*>(workspace);
  const int64_t bytes_a = pl.off_b / 2;
  const int64_t bytes_b = (pl.total - pl.off_b) / 2;
  float* buf_s[2] = {reinterpret_cast<float*>(ws), reinterpret_cast<float*>(ws + pl.off_b)};
  int32_t* buf_i[2] = {reinterpret_cast<int32_t*>(ws + bytes_a), reinterpret_cast<int32_t*>(ws + pl.off_b + bytes_b)};

  SelArgs a{};
  a.q = q; a.c = c; a.nq = nq; a.nc = nc; a.k = k;
  a.nsplit = pl.nsplit; a.c_per_split = pl.c_per_split;
  a.rows_lds = nq < 32 ? (int)nq : 32;
  a.excl_off = excl_offsets; a.excl_idx = excl_idx;
  a.ws_s = buf_s[0]; a.ws_i = buf_i[0];
  const int64_t blocks = pl.rblocks * pl.nsplit;
  int rc;
  switch (dim) {
    case 32: rc = launch_select<32>(a, blocks, stream); break;
    case 64: rc = launch_select<64>(a, blocks, stream); break;
    case 128: rc = launch_select<128>(a, blocks, stream); break;
    default: rc = launch_select<256>(a, blocks, stream); break;
  }
  if (rc != TT_OK) return rc;

  return tt::topk_merge_launch(nq, pl.nsplit, k, buf_s[0], buf_i[0], buf_s[1], buf_i[1], out_scores, out_idx, stream);
}

}  // namespace tt

extern "C" int64_t tt_retrieval_topk_workspace_bytes(int64_t nq, int64_t nc, int32_t dim, int32_t k) {
  if (nq <= 0 || nc <= 0 || nc > INT32_MAX || k < 1 || k > TT_TOPK_MAX_K || k > nc || dim <= 0) return 0;
  return topk_plan(nq, nc, k).total;
}

extern "C" int tt_retrieval_topk_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim, int32_t k,
                                     const int64_t* excl_offsets, const int64_t* excl_idx, void* workspace,
                                     int64_t workspace_bytes, float* out_scores, int64_t* out_idx, tt_stream_t stream_) {
  const char* fn = "tt_retrieval_topk_f32";
  TT_REQUIRE(q && c && workspace && out_scores && out_idx, "%s: null pointer", fn);
  TT_REQUIRE((excl_offsets == nullptr) == (excl_idx == nullptr), "%s: excl_offsets and excl_idx must be given together", fn);
  TT_REQUIRE(nq > 0 && nc > 0, "%s: nq and nc must be positive", fn);
  TT_REQUIRE(nc <= INT32_MAX, "%s: nc %lld exceeds 2^31 - 1 candidates", fn, (long long)nc);
  TT_REQUIRE(dim == 32 || dim == 64 || dim == 128 || dim == 256, "%s: dim %d not in {32,64,128,256}", fn, dim);
  TT_REQUIRE(k >= 1 && k <= TT_TOPK_MAX_K, "%s: k %d not in [1, %d]", fn, k, TT_TOPK_MAX_K);
  TT_REQUIRE(k <= nc, "%s: k %d exceeds nc %lld", fn, k, (long long)nc);
  TT_REQUIRE(tt::aligned16(q) && tt::aligned16(c), "%s: q/c must be 16-byte aligned", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "%s: workspace must be 256-byte aligned", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(out_scores) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out_idx) & 7u) == 0,
             "%s: out_scores / out_idx must be aligned to their element size", fn);
  TT_REQUIRE(excl_offsets == nullptr || ((reinterpret_cast<uintptr_t>(excl_offsets) & 7u) == 0 &&
                                         (reinterpret_cast<uintptr_t>(excl_idx) & 7u) == 0),
             "%s: excl_offsets / excl_idx must be 8-byte aligned", fn);
  const TopkPlan pl = topk_plan(nq, nc, k);
  if (workspace_bytes < pl.total)
    return tt::fail(TT_ERR_WORKSPACE, "%s: workspace %lld < %lld bytes", fn, (long long)workspace_bytes, (long long)pl.total);
  hipStream_t stream = tt::as_stream(stream_);
  tt::ProfScope scope("topk", stream);
  return tt::topk_run(q, c, nq, nc, dim, k, excl_offsets, excl_idx, workspace, out_scores, out_idx, stream, kMinColsPerSplit);
}
