// IVF (inverted-file) approximate top-K retrieval: the exact top-K of every query over the items of the nprobe lists
// whose centroids score highest, with tt_retrieval_topk_f32's scores, order and tie rule.
//
// Index (built by serving.IVF): centroids [nlist, D]; list_offsets int64 [nlist + 1]; list_vectors [n, D], the items
// reordered so that list l is rows list_offsets[l] .. list_offsets[l + 1]; list_ids int32 [n], the original item id of
// every reordered row (ascending within a list).  Ties and exclusions are keyed on the ORIGINAL id.
//
// Contract (tt_ivf_search_f32, include/twotower_hip.h): BruteForce restricted to the probed lists.  Score descending, equal
// scores to the lower original id (also at the cut); exclusions as tt_retrieval_topk_f32 (original ids); fewer than k
// candidates left: the tail is (-inf, -1).  The probed lists are exactly tt_retrieval_topk_f32(q, centroids, nprobe).
// A pair's f32 score is the MFMA chain of topk_select_kernel (same operands, same k-order), so it is bit-identical to the
// score BruteForce computes, and a query's answer does not depend on the batch.
//
// Launches (no host synchronisation, no device-to-host copy):
//   1. coarse probe: tt_retrieval_topk_f32's launches over the centroids with k = nprobe, into the workspace (select + merge
//      launches), split finer than the entry point's (32 centroids per wave): at nq = 1 the 512-candidate splits would leave
//      8 waves of 16 tiles each on the chip.
//   2. ivf_bucket_kernel (one 1024-thread workgroup; list counters in LDS up to nlist 8192): the [nq, nprobe] pairs become
//      a list-major CSR of pair slots (q * nprobe + p) per list, plus per-list work counts ceil(queries / 32) * S and their exclusive scan.
//      The order of the slots within a list is not fixed (atomics), and does not matter: each query row's selection is
//      independent of its tile mates, and every result is written to its slot.
//   3. ivf_select_kernel: one wave per (list, chunk, tile of <= 32 queries probing that list).  The wave gathers its
//      queries' rows into the B operand and streams the chunk's rows of list_vectors through the A operand, selecting
//      with topk::select_run_ids (topk_select.h) keyed on list_ids[row].  It writes the sorted list of k of every
//      (query, probe, chunk) to a [nq][nprobe * S][k] workspace; empty chunks write padding.  The grid is a host-side upper
//      bound; surplus waves exit after reading the scanned work count.
//   4. topk_merge_kernel rounds over the nprobe * S lists of each query (they cover disjoint candidates; padding is a
//      suffix).  The last round writes the outputs.
// Chunks: every list is cut into S chunks of equal length (a multiple of 32 rows).  S is chosen on the host from nq * nprobe
// so that a small batch still puts enough waves on the chip (kTargetWaves, as topk_plan), but no more chunks than the
// average list has 64-row pieces and no more than keep the [nq][nprobe * S][k] lists within 1 GiB.  Large batches get
// S = 1: shorter chunks would let more candidates survive into the selection queues (k of every chunk) for no gain in
// parallelism.
// Launches 1 and 2 and the chunk rule are host functions of namespace tt (ivf_probe_plan, ivf_probe_bucket; declared in
// topk_select.h): ivf_i8.hip's int8 search starts with the same two launches into the same workspace layout.
#include "topk_select.h"

namespace {

constexpr int kTargetWaves = 2048;
constexpr int kMaxChunks = 64;
constexpr int kMinRowsPerChunk = 64;
constexpr int64_t kChunkWsCap = int64_t(1) << 30;   // per-chunk lists of all queries: at most 1 GiB of workspace
constexpr int kCoarseMinCols = 32;          // the coarse probe's split: one 32-centroid tile per wave at small nq
constexpr int kBucketThreads = 1024;
constexpr int kBucketLdsLists = 8192;       // list counters in LDS (32 KiB) up to this nlist, in the workspace above it

using tt::align256;

struct IvfPlan {
  int S;                        // chunks per list
  int nl;                       // lists per query entering the merge: nprobe * S
  int64_t grid;                 // upper bound of the (list, chunk, query tile) work items
  tt::IvfProbePlan probe;       // the probe + bucket regions (shared with ivf_i8.hip)
  int64_t off_as, off_ai, off_bs, off_bi;
  int64_t total;
};

IvfPlan ivf_plan(int64_t nq, int64_t nlist, int64_t n, int dim, int k, int nprobe) {
  IvfPlan p{};
  p.probe = tt::ivf_probe_plan(nq, nlist, n, k, nprobe);
  p.S = p.probe.S;
  p.nl = p.probe.nl;
  p.grid = p.probe.grid;
  int64_t o = p.probe.bytes;
  const int64_t bytes_a = align256(nq * (int64_t)p.nl * k * 4);
  const int64_t bytes_b = tt::topk_merge_b_bytes(nq, p.nl, k);
  p.off_as = o; o += bytes_a;
  p.off_ai = o; o += bytes_a;
  p.off_bs = o; o += bytes_b;
  p.off_bi = o; o += bytes_b;
  p.total = o;
  return p;
}

struct BucketArgs {
  const int64_t* probe;         // [P] list of pair i = q * nprobe + p
  int64_t P;
  int64_t nlist;
  int S;
  int32_t* cnt;                 // [nlist]: counts, then the fill cursors
  int32_t* pstart;              // [nlist + 1]
  int32_t* tstart;              // [nlist + 1]
  int32_t* pairs;               // [P]
};

__device__ __forceinline__ int32_t load_agent(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBucketThreads) void ivf_bucket_kernel(BucketArgs p) {
  __shared__ int32_t sp[kBucketThreads], st[kBucketThreads];
  extern __shared__ int32_t cnt_lds[];
  const int t = threadIdx.x;
  // the counters: in LDS (dynamic, nlist words) when they fit, else the workspace's; flat atomics serve both
  int32_t* cnt = p.nlist <= kBucketLdsLists ? cnt_lds : p.cnt;
  for (int64_t l = t; l < p.nlist; l += kBucketThreads) __hip_atomic_store(cnt + l, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence();
  __syncthreads();
  for (int64_t i = t; i < p.P; i += kBucketThreads) {
    const int64_t l = p.probe[i];
    if (l >= 0 && l < p.nlist) atomicAdd(cnt + l, 1);
  }
  __threadfence();
  __syncthreads();
  // exclusive scans of the pair counts and the work counts: thread t owns lists [t * per, (t + 1) * per)
  const int64_t per = (p.nlist + kBucketThreads - 1) / kBucketThreads;
  const int64_t l0 = t * per < p.nlist ? t * per : p.nlist;
  const int64_t l1 = l0 + per < p.nlist ? l0 + per : p.nlist;
  int32_t sum_p = 0, sum_t = 0;
  for (int64_t l = l0; l < l1; ++l) {
    const int32_t c = load_agent(cnt + l);
    sum_p += c;
    sum_t += (c + 31) / 32 * p.S;
  }
  sp[t] = sum_p;
  st[t] = sum_t;
  __syncthreads();
  for (int off = 1; off < kBucketThreads; off <<= 1) {           // Hillis-Steele inclusive scan
    const int32_t ap = t >= off ? sp[t - off] : 0;
    const int32_t at = t >= off ? st[t - off] : 0;
    __syncthreads();
    sp[t] += ap;
    st[t] += at;
    __syncthreads();
  }
  int32_t run_p = sp[t] - sum_p, run_t = st[t] - sum_t;
  for (int64_t l = l0; l < l1; ++l) {
    const int32_t c = load_agent(cnt + l);
    p.pstart[l] = run_p;
    p.tstart[l] = run_t;
    __hip_atomic_store(cnt + l, run_p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    run_p += c;
    run_t += (c + 31) / 32 * p.S;
  }
  if (t == kBucketThreads - 1) {
    p.pstart[p.nlist] = sp[t];
    p.tstart[p.nlist] = st[t];
  }
  __threadfence();
  __syncthreads();
  for (int64_t i = t; i < p.P; i += kBucketThreads) {
    const int64_t l = p.probe[i];
    if (l >= 0 && l < p.nlist) {
      const int32_t pos = atomicAdd(cnt + l, 1);
      if (pos >= 0 && pos < p.P) p.pairs[pos] = (int32_t)i;
    }
  }
}

struct IvfSelArgs {
  const float* q;
  const float* lv;              // list_vectors
  const int32_t* lids;          // list_ids
  const int64_t* loff;          // list_offsets
  int64_t nlist;
  int k;
  int nprobe;
  int S;
  const int32_t* pstart;
  const int32_t* tstart;
  const int32_t* pairs;
  const int64_t* excl_off;      // nullable
  const int64_t* excl_idx;
  float* ws_s;                  // [nq][nprobe * S][k]
  int32_t* ws_i;
};

template <int D>
__global__ __launch_bounds__(64) void ivf_select_kernel(IvfSelArgs p) {
  const int ln = threadIdx.x & 31;
  const int w = (int)blockIdx.x;
  if (w >= __builtin_amdgcn_readfirstlane(p.tstart[p.nlist])) return;     // surplus wave of the host's upper bound
  // the list: tstart[l] <= w < tstart[l + 1] (lists without work have tstart[l] == tstart[l + 1])
  int64_t lo = 0, hi = p.nlist;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (__builtin_amdgcn_readfirstlane(p.tstart[mid]) <= w) lo = mid; else hi = mid;
  }
  const int64_t l = lo;
  const int S = p.S;
  const int local = w - __builtin_amdgcn_readfirstlane(p.tstart[l]);
  const int qt = local / S;
  const int chunk = local - qt * S;
  const int p0 = __builtin_amdgcn_readfirstlane(p.pstart[l]) + 32 * qt;
  int tn = __builtin_amdgcn_readfirstlane(p.pstart[l + 1]) - p0;
  if (tn > 32) tn = 32;
  const int64_t L0 = p.loff[l], L1 = p.loff[l + 1];
  const int64_t cps = ((L1 - L0 + S - 1) / S + 31) & ~(int64_t)31;
  int64_t c_begin = L0 + chunk * cps;
  if (c_begin > L1) c_begin = L1;
  int64_t c_end = c_begin + cps;
  if (c_end > L1) c_end = L1;

  tt::topk::ListStream s;
  s.r_ok = ln < tn;
  const int64_t qid = s.r_ok ? p.pairs[p0 + ln] / p.nprobe : 0;
  s.qrow = p.q + qid * D;
  s.rows_lds = tn;
  s.k = p.k;
  s.ex_lo = 0;
  s.ex_hi = 0;
  if (p.excl_off != nullptr && s.r_ok) {
    s.ex_lo = p.excl_off[qid];
    s.ex_hi = p.excl_off[qid + 1];
  }
  s.excl_idx = p.excl_idx;
  s.c = p.lv;
  s.ids = p.lids;
  s.c_begin = c_begin;
  s.c_end = c_end;
  s.ws_s = p.ws_s;
  s.ws_i = p.ws_i;
  const int32_t* pairs = p.pairs;
  const int64_t k = p.k;
  tt::topk::select_run_ids<D, true>(s, [&](int rr) -> int64_t {
    // slot q * nprobe + probe: list (q, probe, chunk) of the [nq][nprobe * S][k] workspace
    return rr >= tn ? -1 : ((int64_t)__builtin_amdgcn_readfirstlane(pairs[p0 + rr]) * S + chunk) * k;
  });
}

template <int D>
int launch_ivf_select(const IvfSelArgs& a, int rows, int64_t blocks, hipStream_t stream) {
  return tt::topk::launch_select("ivf_select", ivf_select_kernel<D>, tt::topk::select_lds_bytes(rows, a.k), blocks, stream, a,
                                 "tt_ivf_search_f32");
}

bool shape_ok(int64_t nq, int64_t nlist, int64_t n, int32_t dim, int32_t k, int32_t nprobe) {
  return nq > 0 && nlist > 0 && n > 0 && n <= INT32_MAX && nlist <= INT32_MAX &&
         (dim == 32 || dim == 64 || dim == 128 || dim == 256) && k >= 1 && k <= TT_TOPK_MAX_K && nprobe >= 1 &&
         nprobe <= TT_TOPK_MAX_K && nprobe <= nlist && nq * nprobe <= INT32_MAX;
}

}  // namespace

// The chunk rule and the probe + bucket workspace regions, for lists of list_k entries per (query, probe, chunk).
tt::IvfProbePlan tt::ivf_probe_plan(int64_t nq, int64_t nlist, int64_t n, int list_k, int nprobe) {
  IvfProbePlan p{};
  const int64_t P = nq * nprobe;
  int64_t est = P < nlist ? P : nlist;                       // work items before chunking, roughly
  if (est < (P + 31) / 32) est = (P + 31) / 32;
  int64_t S = (kTargetWaves + est - 1) / est;
  const int64_t by_rows = (n / nlist + kMinRowsPerChunk - 1) / kMinRowsPerChunk;
  if (S > by_rows) S = by_rows;
  if (S > kMaxChunks) S = kMaxChunks;
  const int64_t by_ws = kChunkWsCap / (P * (int64_t)list_k * 8);
  if (S > by_ws) S = by_ws;
  if (S < 1) S = 1;
  p.S = (int)S;
  p.nl = nprobe * p.S;
  p.grid = ((P + 31) / 32 + (P < nlist ? P : nlist)) * S;    // sum over lists of ceil(c_l / 32) <= ceil(P / 32) + #lists
  int64_t o = align256(tt::topk_workspace_bytes_split(nq, nlist, nprobe, kCoarseMinCols));
  p.off_probe_s = o; o += align256(P * 4);
  p.off_probe_i = o; o += align256(P * 8);
  p.off_cnt = o; o += align256(nlist * 4);
  p.off_pstart = o; o += align256((nlist + 1) * 4);
  p.off_tstart = o; o += align256((nlist + 1) * 4);
  p.off_pairs = o; o += align256(P * 4);
  p.bytes = o;
  return p;
}

// Launches 1 and 2: the coarse probe into the workspace, then the bucket kernel (arguments already validated).
int tt::ivf_probe_bucket(const float* q, const float* centroids, int64_t nq, int64_t nlist, int dim, int nprobe,
                         const IvfProbePlan& pl, void* workspace, hipStream_t stream) {
  char* ws = static_cast<char*>(workspace);
  float* probe_s = reinterpret_cast<float*>(ws + pl.off_probe_s);
  int64_t* probe_i = reinterpret_cast<int64_t*>(ws + pl.off_probe_i);
  int rc = tt::topk_run(q, centroids, nq, nlist, dim, nprobe, nullptr, nullptr, ws, probe_s, probe_i, stream, kCoarseMinCols);
  if (rc != TT_OK) return rc;
  BucketArgs b{};
  b.probe = probe_i; b.P = nq * nprobe; b.nlist = nlist; b.S = pl.S;
  b.cnt = reinterpret_cast<int32_t*>(ws + pl.off_cnt);
  b.pstart = reinterpret_cast<int32_t*>(ws + pl.off_pstart);
  b.tstart = reinterpret_cast<int32_t*>(ws + pl.off_tstart);
  b.pairs = reinterpret_cast<int32_t*>(ws + pl.off_pairs);
  const unsigned bucket_lds = nlist <= kBucketLdsLists ? (unsigned)(nlist * 4) : 0u;
  tt::launch("ivf_bucket", ivf_bucket_kernel, dim3(1), dim3(kBucketThreads), bucket_lds, stream, b);
  return tt::check_launch("ivf_bucket");
}

extern "C" int64_t tt_ivf_search_workspace_bytes(int64_t nq, int64_t nlist, int64_t n, int32_t dim, int32_t k, int32_t nprobe) {
  if (!shape_ok(nq, nlist, n, dim, k, nprobe)) return 0;
  const IvfPlan pl = ivf_plan(nq, nlist, n, dim, k, nprobe);
  return pl.grid <= INT32_MAX ? pl.total : 0;
}

extern "C" int tt_ivf_search_f32(const float* q, int64_t nq, const float* centroids, int64_t nlist, const int64_t* list_offsets,
                                 const float* list_vectors, const int32_t* list_ids, int64_t n, int32_t dim, int32_t k,
                                 int32_t nprobe, const int64_t* excl_offsets, const int64_t* excl_idx, void* workspace,
                                 int64_t workspace_bytes, float* out_scores, int64_t* out_idx, tt_stream_t stream_) {
  const char* fn = "tt_ivf_search_f32";
  TT_REQUIRE(q && centroids && list_offsets && list_vectors && list_ids && workspace && out_scores && out_idx,
             "%s: null pointer", fn);
  TT_REQUIRE((excl_offsets == nullptr) == (excl_idx == nullptr), "%s: excl_offsets and excl_idx must be given together", fn);
  TT_REQUIRE(nq > 0 && nlist > 0 && n > 0, "%s: nq, nlist and n must be positive", fn);
  TT_REQUIRE(n <= INT32_MAX && nlist <= INT32_MAX, "%s: n %lld / nlist %lld exceed 2^31 - 1", fn, (long long)n,
             (long long)nlist);
  TT_REQUIRE(dim == 32 || dim == 64 || dim == 128 || dim == 256, "%s: dim %d not in {32,64,128,256}", fn, dim);
  TT_REQUIRE(k >= 1 && k <= TT_TOPK_MAX_K, "%s: k %d not in [1, %d]", fn, k, TT_TOPK_MAX_K);
  TT_REQUIRE(nprobe >= 1 && nprobe <= TT_TOPK_MAX_K && nprobe <= nlist, "%s: nprobe %d not in [1, min(nlist %lld, %d)]", fn,
             nprobe, (long long)nlist, TT_TOPK_MAX_K);
  TT_REQUIRE(nq * nprobe <= INT32_MAX, "%s: nq * nprobe exceeds 2^31 - 1", fn);
  TT_REQUIRE(tt::aligned16(q) && tt::aligned16(centroids) && tt::aligned16(list_vectors),
             "%s: q / centroids / list_vectors must be 16-byte aligned", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(list_offsets) & 7u) == 0 && (reinterpret_cast<uintptr_t>(list_ids) & 3u) == 0,
             "%s: list_offsets / list_ids must be aligned to their element size", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "%s: workspace must be 256-byte aligned", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(out_scores) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out_idx) & 7u) == 0,
             "%s: out_scores / out_idx must be aligned to their element size", fn);
  TT_REQUIRE(excl_offsets == nullptr || ((reinterpret_cast<uintptr_t>(excl_offsets) & 7u) == 0 &&
                                         (reinterpret_cast<uintptr_t>(excl_idx) & 7u) == 0),
             "%s: excl_offsets / excl_idx must be 8-byte aligned", fn);
  const IvfPlan pl = ivf_plan(nq, nlist, n, dim, k, nprobe);
  TT_REQUIRE(pl.grid <= INT32_MAX, "%s: nq * nprobe too large for one call", fn);
  if (workspace_bytes < pl.total)
    return tt::fail(TT_ERR_WORKSPACE, "%s: workspace %lld < %lld bytes", fn, (long long)workspace_bytes, (long long)pl.total);
  hipStream_t stream = tt::as_stream(stream_);
  tt::ProfScope scope("ivf", stream);
  char* ws = static_cast<char*>(workspace);
  int rc = tt::ivf_probe_bucket(q, centroids, nq, nlist, dim, nprobe, pl.probe, workspace, stream);
  if (rc != TT_OK) return rc;

  IvfSelArgs a{};
  a.q = q; a.lv = list_vectors; a.lids = list_ids; a.loff = list_offsets; a.nlist = nlist; a.k = k; a.nprobe = nprobe;
  a.S = pl.S;
  a.pstart = reinterpret_cast<const int32_t*>(ws + pl.probe.off_pstart);
  a.tstart = reinterpret_cast<const int32_t*>(ws + pl.probe.off_tstart);
  a.pairs = reinterpret_cast<const int32_t*>(ws + pl.probe.off_pairs);
  a.excl_off = excl_offsets; a.excl_idx = excl_idx;
  a.ws_s = reinterpret_cast<float*>(ws + pl.off_as); a.ws_i = reinterpret_cast<int32_t*>(ws + pl.off_ai);
  const int rows = nq < 32 ? (int)nq : 32;                   // a list holds each query at most once
  switch (dim) {
    case 32: rc = launch_ivf_select<32>(a, rows, pl.grid, stream); break;
    case 64: rc = launch_ivf_select<64>(a, rows, pl.grid, stream); break;
    case 128: rc = launch_ivf_select<128>(a, rows, pl.grid, stream); break;
    default: rc = launch_ivf_select<256>(a, rows, pl.grid, stream); break;
  }
  if (rc != TT_OK) return rc;
  return tt::topk_merge_launch(nq, pl.nl, k, a.ws_s, a.ws_i, reinterpret_cast<float*>(ws + pl.off_bs),
                               reinterpret_cast<int32_t*>(ws + pl.off_bi), out_scores, out_idx, stream);
}
