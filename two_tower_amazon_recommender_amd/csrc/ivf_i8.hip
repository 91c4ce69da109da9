// Int8 IVF: tt_ivf_search_i8_f32, the int8 scan of topk_i8.hip restricted to the probed inverted lists of ivf.hip, with the
// same exact f32 re-rank.
//
// Index (built by serving.Int8IVF): centroids, list_offsets and list_ids as tt_ivf_search_f32; list_codes int8 [n, D] and
// list_scales f32 [n], the tt_quantize_rows_i8 output of the items in list order; optionally c f32 [n, D] in ORIGINAL id
// order (the re-rank gathers by the ids stage 1 produced, so no reordered f32 copy exists).
//
// Contract (include/twotower_hip.h): the probed lists are tt_retrieval_topk_f32(q, centroids, nprobe); stage 1 is
// tt_retrieval_topk_i8_f32's over the rows of those lists (same query quantiser, key = float(int32 dot) * list_scales[row],
// the k1 best by (key descending, ORIGINAL id ascending), also at the cut; excluded original ids never take a slot); stage 2
// is tt_retrieval_topk_i8_f32's.  Integer sums are order-free, keys and re-rank scores are per pair and ids are unique, so a
// query's row is identical alone, in any batch, for any chunk count and on any run; with nprobe == nlist the output is
// tt_retrieval_topk_i8_f32's over the whole corpus, bit for bit.
//
// Launches (no synchronisation, no copy to the host):
//   1. the coarse probe and 2. ivf_bucket_kernel: tt::ivf_probe_bucket (ivf.hip), unchanged.
//   3. ivf_i8_select_kernel: one wave per (list, chunk, tile of <= 32 queries probing that list), ivf_select_kernel's
//      decomposition.  The wave gathers its queries' rows by pair slot and quantises them into the B operand of
//      v_mfma_i32_32x32x32_i8 (D / 32 x 4 VGPRs; amax, then the codes; lanes without a query hold zeros), and streams the
//      chunk's rows of list_codes through the A operand with i8_scan_kernel's lane-half byte pairing and its ring of four
//      tile buffers; lane ln also loads its row's scale and original id.  The loads are unconditional: rows past the chunk's
//      end read the chunk's first row and are masked by the range check.  Selection is the sorted-list / 48-slot-queue /
//      register-threshold scheme with list length k1, keyed on list_ids[row].  Every (query, probe, chunk) writes its sorted
//      list of k1 to the [nq][nprobe * S][k1] workspace; empty chunks write padding.
//      Query scales: ONE designated wave per query writes qscale[query] - the wave that holds the query's probe slot 0 in
//      chunk 0 (every pair slot lies in exactly one list's bucket, and a bucket has work items whatever the list's length).
//   4. topk_merge_kernel rounds over the nprobe * S lists of each query into the [nq][k1] candidate buffer.
//   5. tt::i8_finish_launch (topk_i8.hip): i8_rerank_kernel with c, i8_scale_kernel without.
// Chunks: tt::ivf_probe_plan's rule (ivf.hip) with lists of k1 entries: S from nq * nprobe so that a small batch fills the
// chip, at most one chunk per 64 rows of the average list, at most 64, and the [nq][nprobe * S][k1] lists within 1 GiB.
// LDS: min(nq, 32) x (k1 + 48) x 8 B (78 KB at k1 = 256: topk::launch_select raises the dynamic limit).
#include "topk_select.h"
#include "quant_i8.h"

namespace {

using tt::f32x4;
using tt::i8::amax4;
using tt::i8::i32x16;
using tt::i8::i32x4;
using tt::i8::kRing;
using tt::i8::quant4;
using tt::i8::row_scale;
using tt::topk::beats;
using tt::topk::kMaxEntries;
using tt::topk::kQueue;

using tt::align256;

struct IvfI8Plan {
  tt::IvfProbePlan probe;
  int64_t bytes_a, bytes_b;     // one array of the merge buffers
  int64_t off_as, off_ai, off_bs, off_bi, off_cs, off_ci, off_qs;
  int64_t total;
};

IvfI8Plan ivf_i8_plan(int64_t nq, int64_t nlist, int64_t n, int k1, int nprobe) {
  IvfI8Plan p{};
  p.probe = tt::ivf_probe_plan(nq, nlist, n, k1, nprobe);
  p.bytes_a = align256(nq * (int64_t)p.probe.nl * k1 * 4);
  p.bytes_b = tt::topk_merge_b_bytes(nq, p.probe.nl, k1);
  int64_t o = p.probe.bytes;
  p.off_as = o; o += p.bytes_a;
  p.off_ai = o; o += p.bytes_a;
  p.off_bs = o; o += p.bytes_b;
  p.off_bi = o; o += p.bytes_b;
  p.off_cs = o; o += align256(nq * (int64_t)k1 * 4);     // candidate keys [nq][k1]
  p.off_ci = o; o += align256(nq * (int64_t)k1 * 8);     // candidate ids int64 [nq][k1]
  p.off_qs = o; o += align256(nq * 4);                   // query scales [nq]
  p.total = o;
  return p;
}

struct IvfI8SelArgs {
  const float* q;
  const int8_t* codes;          // list_codes
  const float* scales;          // list_scales
  const int32_t* lids;          // list_ids
  const int64_t* loff;          // list_offsets
  int64_t nlist;
  int k;                        // list length (k1)
  int nprobe;
  int S;
  const int32_t* pstart;
  const int32_t* tstart;
  const int32_t* pairs;
  const int64_t* excl_off;      // nullable
  const int64_t* excl_idx;
  float* ws_s;                  // [nq][nprobe * S][k]
  int32_t* ws_i;
  float* qscale;                // [nq]
};

template <int D>
__global__ __launch_bounds__(64) void ivf_i8_select_kernel(IvfI8SelArgs p) {
  constexpr int NS = D / 32;                        // k-steps of 32 codes (16 per lane half)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x;
  const int h = lane >> 5;
  const int ln = lane & 31;
  const int k = p.k;
  const int RS = 2 * (k + kQueue);                  // LDS words per query row: list scores, list ids, queue scores, queue ids

  // the work item: every quantity that steers a loop with a barrier in it is wave-uniform by construction (readfirstlane)
  const int w = (int)blockIdx.x;
  if (w >= __builtin_amdgcn_readfirstlane(p.tstart[p.nlist])) return;     // surplus wave of the host's upper bound
  int64_t lo = 0, hi = p.nlist;                     // the list: tstart[l] <= w < tstart[l + 1]
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
  const int rows_lds = tn;
  const int64_t L0 = p.loff[l], L1 = p.loff[l + 1];
  const int64_t cps = ((L1 - L0 + S - 1) / S + 31) & ~(int64_t)31;
  int64_t c_begin = L0 + chunk * cps;
  if (c_begin > L1) c_begin = L1;
  int64_t c_end = c_begin + cps;
  if (c_end > L1) c_end = L1;
  const int ntiles = __builtin_amdgcn_readfirstlane((int)((c_end - c_begin + 31) >> 5));

  const bool r_ok = ln < tn;
  const int pair = r_ok ? p.pairs[p0 + ln] : 0;     // slot q * nprobe + probe
  const int64_t qid = pair / p.nprobe;

  // stationary fragment: qb[s] = the codes of q[qid][32 s + 16 h .. + 15] (two passes over the row: amax, then the codes)
  i32x4 qb[NS];
  {
    const f32x4* R4 = reinterpret_cast<const f32x4*>(p.q + qid * D) + 4 * h;
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
    // the designated writer of a query's scale: the wave holding its probe slot 0, in chunk 0
    if (r_ok && h == 0 && chunk == 0 && pair - (int)qid * p.nprobe == 0) p.qscale[qid] = qscale;
  }
  int64_t ex_lo = 0, ex_hi = 0;
  if (p.excl_off != nullptr && r_ok) {
    ex_lo = p.excl_off[qid];
    ex_hi = p.excl_off[qid + 1];
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

  // a tile: lane (ln, h) loads half h of every 32-byte k-step of row c0 + ln, and the row's scale and original id.  Rows
  // past c_end read the chunk's first row instead (unconditional loads; their scores are masked by cand < c_end below).
  auto load_tile = [&](i32x4 (&a)[NS], float& sc, int& id, int t) {
    const int64_t cand = c_begin + 32 * (int64_t)t + ln;
    const int64_t src_row = cand < c_end ? cand : c_begin;
    const i32x4* src = reinterpret_cast<const i32x4*>(p.codes + src_row * D) + h;
#pragma unroll
    for (int s = 0; s < NS; ++s) a[s] = src[2 * s];
    sc = p.scales[src_row];
    id = p.lids[src_row];
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

  auto process = [&](int t, const i32x4 (&a)[NS], float sc, int id) {
    i32x16 X;
#pragma unroll
    for (int i = 0; i < 16; ++i) X[i] = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) X = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], qb[s], X, 0, 0, 0);
    // X[reg] = iscore(query, row c0 + acc_row(reg, h)); the scale and the id of row acc_row(reg, h) come from the lane that
    // loaded it: the shuffles run here, with every lane active (inside the divergent code below they would read inactive
    // source lanes as 0)
    const int64_t c0 = c_begin + 32 * (int64_t)t;
    float key[16];
    int idr[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      key[reg] = (float)X[reg] * __shfl(sc, tt::acc_row(reg, h));
      idr[reg] = __shfl(id, tt::acc_row(reg, h));
    }
    uint32_t mask = 0;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int64_t cand = c0 + tt::acc_row(reg, h);
      const bool ok = r_ok && cand < c_end && (!full || beats(key[reg], idr[reg], thr_s, thr_i));
      mask |= ok ? (1u << reg) : 0u;
    }
    if (ex_hi > ex_lo && mask != 0u) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
        if (((mask >> reg) & 1u) && excluded(idr[reg])) mask &= ~(1u << reg);
    }
    const int n = __builtin_popcount(mask);
    const int n_other = __shfl_xor(n, 32);
    int pos = qn + (h ? n_other : 0);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
      if ((mask >> reg) & 1u) {
        qs[pos] = key[reg];
        qi[pos] = idr[reg];
        ++pos;
      }
    qn += n + n_other;
    if (__ballot(qn > kQueue - 32) != 0ull) flush();
  };

  i32x4 a[kRing][NS];
  float sc[kRing];
  int id[kRing];
#pragma unroll
  for (int j = 0; j < kRing; ++j) {
    sc[j] = 0.f;
    id[j] = 0;
    if (j < ntiles) load_tile(a[j], sc[j], id[j], j);
  }
  for (int t = 0; t < ntiles; t += kRing) {
#pragma unroll
    for (int j = 0; j < kRing; ++j) {
      if (t + j < ntiles) {
        process(t + j, a[j], sc[j], id[j]);
        if (t + j + kRing < ntiles) load_tile(a[j], sc[j], id[j], t + j + kRing);
      }
    }
  }
  if (__ballot(qn > 0) != 0ull) flush();

  // every (query, probe, chunk)'s sorted list, padded with (-inf, -1): list pair * S + chunk of the [nq][nprobe * S][k] workspace
  for (int rr = 0; rr < rows_lds; ++rr) {
    const int m_r = __builtin_amdgcn_readlane(m, rr);
    const float* Ls = smem + rr * RS;
    const int* Li = reinterpret_cast<const int*>(Ls + k);
    const int64_t o = ((int64_t)__builtin_amdgcn_readfirstlane(p.pairs[p0 + rr]) * S + chunk) * (int64_t)k;
    for (int e = lane; e < k; e += 64) {
      p.ws_s[o + e] = e < m_r ? Ls[e] : -__builtin_inff();
      p.ws_i[o + e] = e < m_r ? Li[e] : -1;
    }
  }
}

template <int D>
int launch_ivf_i8_select(const IvfI8SelArgs& a, int rows, int64_t blocks, hipStream_t stream) {
  return tt::topk::launch_select("ivf_i8_select", ivf_i8_select_kernel<D>, tt::topk::select_lds_bytes(rows, a.k), blocks, stream, a,
                                 "tt_ivf_search_i8_f32");
}

bool shape_ok(int64_t nq, int64_t nlist, int64_t n, int32_t dim, int32_t k, int32_t k1, int32_t nprobe) {
  return nq > 0 && nlist > 0 && n > 0 && n <= INT32_MAX && nlist <= INT32_MAX &&
         (dim == 32 || dim == 64 || dim == 128 || dim == 256) && k >= 1 && k <= k1 && k1 <= TT_TOPK_MAX_K && k1 <= n &&
         nprobe >= 1 && nprobe <= TT_TOPK_MAX_K && nprobe <= nlist && nq <= INT32_MAX && nq * nprobe <= INT32_MAX;
}

}  // namespace

extern "C" int64_t tt_ivf_search_i8_workspace_bytes(int64_t nq, int64_t nlist, int64_t n, int32_t dim, int32_t k, int32_t k1,
                                                    int32_t nprobe) {
  if (!shape_ok(nq, nlist, n, dim, k, k1, nprobe)) return 0;
  const IvfI8Plan pl = ivf_i8_plan(nq, nlist, n, k1, nprobe);
  return pl.probe.grid <= INT32_MAX ? pl.total : 0;
}

extern "C" int tt_ivf_search_i8_f32(const float* q, int64_t nq, const float* centroids, int64_t nlist, const int64_t* list_offsets,
                                    const int8_t* list_codes, const float* list_scales, const int32_t* list_ids, const float* c,
                                    int64_t n, int32_t dim, int32_t k, int32_t k1, int32_t nprobe, const int64_t* excl_offsets,
                                    const int64_t* excl_idx, void* workspace, int64_t workspace_bytes, float* out_scores,
                                    int64_t* out_idx, tt_stream_t stream_) {
  const char* fn = "tt_ivf_search_i8_f32";
  TT_REQUIRE(q && centroids && list_offsets && list_codes && list_scales && list_ids && workspace && out_scores && out_idx,
             "%s: null pointer", fn);
  TT_REQUIRE((excl_offsets == nullptr) == (excl_idx == nullptr), "%s: excl_offsets and excl_idx must be given together", fn);
  TT_REQUIRE(nq > 0 && nlist > 0 && n > 0, "%s: nq, nlist and n must be positive", fn);
  TT_REQUIRE(n <= INT32_MAX && nlist <= INT32_MAX, "%s: n %lld / nlist %lld exceed 2^31 - 1", fn, (long long)n,
             (long long)nlist);
  TT_REQUIRE(dim == 32 || dim == 64 || dim == 128 || dim == 256, "%s: dim %d not in {32,64,128,256}", fn, dim);
  TT_REQUIRE(k >= 1, "%s: k %d must be positive", fn, k);
  TT_REQUIRE(k <= k1, "%s: k %d exceeds k1 %d", fn, k, k1);
  TT_REQUIRE(k1 <= TT_TOPK_MAX_K, "%s: k1 %d exceeds %d", fn, k1, TT_TOPK_MAX_K);
  TT_REQUIRE(k1 <= n, "%s: k1 %d exceeds n %lld", fn, k1, (long long)n);
  TT_REQUIRE(c != nullptr || k1 == k, "%s: without c there is no re-rank: k1 %d must equal k %d", fn, k1, k);
  TT_REQUIRE(nprobe >= 1 && nprobe <= TT_TOPK_MAX_K && nprobe <= nlist, "%s: nprobe %d not in [1, min(nlist %lld, %d)]", fn,
             nprobe, (long long)nlist, TT_TOPK_MAX_K);
  TT_REQUIRE(nq <= INT32_MAX && nq * nprobe <= INT32_MAX, "%s: nq * nprobe exceeds 2^31 - 1", fn);
  TT_REQUIRE(tt::aligned16(q) && tt::aligned16(centroids) && tt::aligned16(list_codes) && tt::aligned16(c),
             "%s: q / centroids / list_codes / c must be 16-byte aligned", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(list_offsets) & 7u) == 0 && (reinterpret_cast<uintptr_t>(list_ids) & 3u) == 0 &&
                 (reinterpret_cast<uintptr_t>(list_scales) & 3u) == 0,
             "%s: list_offsets / list_scales / list_ids must be aligned to their element size", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "%s: workspace must be 256-byte aligned", fn);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(out_scores) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out_idx) & 7u) == 0,
             "%s: out_scores / out_idx must be aligned to their element size", fn);
  TT_REQUIRE(excl_offsets == nullptr || ((reinterpret_cast<uintptr_t>(excl_offsets) & 7u) == 0 &&
                                         (reinterpret_cast<uintptr_t>(excl_idx) & 7u) == 0),
             "%s: excl_offsets / excl_idx must be 8-byte aligned", fn);
  const IvfI8Plan pl = ivf_i8_plan(nq, nlist, n, k1, nprobe);
  TT_REQUIRE(pl.probe.grid <= INT32_MAX, "%s: nq * nprobe too large for one call", fn);
  if (workspace_bytes < pl.total)
    return tt::fail(TT_ERR_WORKSPACE, "%s: workspace %lld < %lld bytes", fn, (long long)workspace_bytes, (long long)pl.total);
  hipStream_t stream = tt::as_stream(stream_);
  tt::ProfScope scope("ivf_i8", stream);
  char* ws = static_cast<char*>(workspace);
  int rc = tt::ivf_probe_bucket(q, centroids, nq, nlist, dim, nprobe, pl.probe, workspace, stream);
  if (rc != TT_OK) return rc;

  IvfI8SelArgs a{};
  a.q = q; a.codes = list_codes; a.scales = list_scales; a.lids = list_ids; a.loff = list_offsets; a.nlist = nlist;
  a.k = k1; a.nprobe = nprobe; a.S = pl.probe.S;
  a.pstart = reinterpret_cast<const int32_t*>(ws + pl.probe.off_pstart);
  a.tstart = reinterpret_cast<const int32_t*>(ws + pl.probe.off_tstart);
  a.pairs = reinterpret_cast<const int32_t*>(ws + pl.probe.off_pairs);
  a.excl_off = excl_offsets; a.excl_idx = excl_idx;
  a.ws_s = reinterpret_cast<float*>(ws + pl.off_as); a.ws_i = reinterpret_cast<int32_t*>(ws + pl.off_ai);
  a.qscale = reinterpret_cast<float*>(ws + pl.off_qs);
  const int rows = nq < 32 ? (int)nq : 32;                   // a list holds each query at most once
  switch (dim) {
    case 32: rc = launch_ivf_i8_select<32>(a, rows, pl.probe.grid, stream); break;
    case 64: rc = launch_ivf_i8_select<64>(a, rows, pl.probe.grid, stream); break;
    case 128: rc = launch_ivf_i8_select<128>(a, rows, pl.probe.grid, stream); break;
    default: rc = launch_ivf_i8_select<256>(a, rows, pl.probe.grid, stream); break;
  }
  if (rc != TT_OK) return rc;
  float* cand_s = reinterpret_cast<float*>(ws + pl.off_cs);
  int64_t* cand_i = reinterpret_cast<int64_t*>(ws + pl.off_ci);
  rc = tt::topk_merge_launch(nq, pl.probe.nl, k1, a.ws_s, a.ws_i, reinterpret_cast<float*>(ws + pl.off_bs),
                             reinterpret_cast<int32_t*>(ws + pl.off_bi), cand_s, cand_i, stream);
  if (rc != TT_OK) return rc;
  return tt::i8_finish_launch(q, c, cand_s, cand_i, a.qscale, nq, dim, k, k1, out_scores, out_idx, stream);
}
