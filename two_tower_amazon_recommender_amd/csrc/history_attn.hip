// Attention pooling of the user history: a learned query a [dim] and a recency bias p [L] decide how much every kept slot of a
// history bag weighs (history_pooling = "attention"), where bag.hip's poolings weigh them all alike.  For the valid slots j of bag b
// (padding, out-of-range tokens and the excluded item skipped exactly as in tt_history_bag_fwd_f32):
//   r_j = number of valid slots behind j (0: the newest kept item), e_j = <h_j, a> / sqrt(dim) + p[r_j], w = softmax(e),
//   out[b] = base row + sum_j w_j h_j.
// Both launches are HBM-bound row gathers and keep bag.hip's structure: a group of LPR lanes (the power of two >= dim/4, at most a
// wave; NV = ceil(dim/256) float4 per lane) owns a bag, its slots are read once per group, LPR at a time, the valid ones found
// with a ballot and handed round by shuffle, kInFlight independent row loads leave before the first wait.  A dot product is a
// fixed fmaf chain inside the lane followed by a fixed xor butterfly over the group's lanes, so every lane holds the same sum.
//
// Forward: 4*dim*(sum(cnt) + 3*n_bags) bytes (the rows, the base row, out, pooled).  One pass over the token row counts the valid
// slots (the ranks count from the END of the bag) and writes batch_ids; the second gathers the rows in ascending slot order into an
// online softmax (running max, running sum, rescaled accumulator - branch-free: both exponentials are taken for every slot).
// The logits are parked in ``weights`` and turned into the normalised weights by the lane that wrote them, once the bag's max and
// sum are known.  No LDS, no atomics (but the out-of-range flag): a bag's bits depend on that bag alone.
//
// Backward: 4*dim*(2*sum(cnt) + 2*n_bags) bytes (the rows and their slot gradient rows, dy, pooled).  One pass over the rows per
// bag, newest slot first (the rank is then a running count): G = <g, pooled>, t_j = <g, h_j>, de_j = w_j (t_j - G),
// dh_j = w_j g + de_j a / sqrt(dim) written to row b*L + j of slot_grads (a skipped slot's row is left untouched: its batch id
// is -1, the sort plan never reads it).  Workgroup s owns the contiguous bags of slab s: every lane group sums de_j h_j (registers)
// and de_j by rank (LDS, its own line) over its bags in a fixed order, the groups' sums are added in ascending group order and
// written to dattn_slabs[s] = [da (dim) | dp (L)] - every slab in full, no atomics, no pre-zeroing: the form the dense optimizer
// segments sum.
#include "common.h"

namespace {

constexpr int kInFlight = 4;

// sum of v over the lanes of a group (a fixed xor butterfly: every lane ends with the same bits)
__device__ __forceinline__ float group_sum(float v, int lpr) {
  for (int off = lpr >> 1; off > 0; off >>= 1) v = __fadd_rn(v, __shfl_xor(v, off, 64));
  return v;
}

template <int NV>
__device__ __forceinline__ float row_dot(const tt::f32x4 (&r)[NV], const tt::f32x4 (&a)[NV]) {
  float d = 0.0f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) d = __fmaf_rn(r[i][q], a[i][q], d);
  return d;
}

template <int NV, bool EXCL, bool BASE>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ table_, int64_t table_rows, int dim4, int lpr_log2,
                                                       const int32_t* __restrict__ tokens, int64_t n_token_rows, int L,
                                                       const int64_t* __restrict__ bag_rows, int64_t n_bags,
                                                       const float* __restrict__ attn, float scale, float* __restrict__ out_,
                                                       int64_t* __restrict__ batch_ids, float* weights, float* __restrict__ pooled_,
                                                       int32_t* __restrict__ oob_flag, const int64_t* __restrict__ exclude,
                                                       const float* __restrict__ base_table_, int64_t base_rows,
                                                       const int64_t* __restrict__ base_ids) {
  const tt::f32x4* __restrict__ table = reinterpret_cast<const tt::f32x4*>(table_);
  tt::f32x4* __restrict__ out = reinterpret_cast<tt::f32x4*>(out_);
  const float* __restrict__ bias = attn + (int64_t)dim4 * 4;         // p[0..L)
  const int lpr = 1 << lpr_log2;
  const int groups = 256 >> lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int gbase = (threadIdx.x & 63) & ~(lpr - 1);                 // first lane of this group inside its wave
  const uint64_t gmask = lpr == 64 ? ~0ull : ((1ull << lpr) - 1);
  const int64_t b = (int64_t)blockIdx.x * groups + (threadIdx.x >> lpr_log2);
  const bool live = b < n_bags;

  int64_t row = -1;                                                  // token row of the bag; -1: empty bag
  int64_t ex = -1;                                                   // EXCL: the token this bag leaves out
  int64_t bid = -1;                                                  // BASE: the base row of this bag; -1: a zero row
  if (live) {
    row = bag_rows != nullptr ? bag_rows[b] : b;
    if constexpr (EXCL) ex = exclude[b];
    if constexpr (BASE) {
      bid = base_ids[b];
      if (bid < 0 || bid >= base_rows) {
        if (bid != -1 && l == 0 && oob_flag != nullptr) atomicOr(oob_flag, 1);
        bid = -1;
      }
    }
    if (row < 0 || row >= n_token_rows) {
      if (row != -1 && l == 0 && oob_flag != nullptr) atomicOr(oob_flag, 1);
      row = -1;
    }
  }
  // the base row and the query: loaded ahead of the gather (a lane past the row's end holds a zero query: its re-read float4s
  // add nothing to a dot product)
  tt::f32x4 o[NV], a[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = l + i * lpr;
    o[i] = tt::f32x4{0.f, 0.f, 0.f, 0.f};
    a[i] = tt::f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < dim4) a[i] = reinterpret_cast<const tt::f32x4*>(attn)[c];
    if constexpr (BASE) {
      if (bid >= 0 && c < dim4) o[i] = reinterpret_cast<const tt::f32x4*>(base_table_)[bid * dim4 + c];
    }
  }

  // this lane's slot of a chunk: its token after padding, exclusion and the range check (-1: skipped)
  auto slot_token = [&](int slot, bool first_pass) -> int32_t {
    int32_t tok = -1;
    if (row >= 0 && slot < L) {
      tok = tokens[row * L + slot];
      if constexpr (EXCL) {                                          // the raw token, compared in int64: skipped like padding
        if ((int64_t)tok == ex) tok = -1;
      }
      if (tok < 0 || (int64_t)tok >= table_rows) {
        if (first_pass && tok != -1 && oob_flag != nullptr) atomicOr(oob_flag, 1);
        tok = -1;
      }
    }
    return tok;
  };

  // pass 1: batch_ids, the flag and the number of valid slots (the ranks count from the bag's end)
  int total = 0;
  for (int base = 0; base < L; base += lpr) {                        // (L is uniform: every lane of the wave reaches the ballot)
    const int slot = base + l;
    const int32_t tok = slot_token(slot, true);
    if (live && slot < L && batch_ids != nullptr) batch_ids[b * L + slot] = (int64_t)tok;
    total += __popcll((__ballot(tok >= 0) >> gbase) & gmask);
  }

  // pass 2: the rows, in ascending slot order, into the online softmax
  tt::f32x4 s[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) s[i] = tt::f32x4{0.f, 0.f, 0.f, 0.f};
  float mx = 0.0f, den = 0.0f;                                       // running max and sum of exp(e - mx) (set by the first slot)
  int cnt = 0;
  for (int base = 0; base < L; base += lpr) {
    const int slot = base + l;
    const int32_t tok = slot_token(slot, false);
    float my_e = -INFINITY;                                          // this lane's slot: its logit; -inf: skipped
    uint64_t m = (__ballot(tok >= 0) >> gbase) & gmask;              // valid slots of this group's chunk, bit k = slot base + k
    while (m != 0) {                                                 // (m is uniform inside a group: its lanes stay together)
      // the next (up to) kInFlight valid slots; a batch shorter than that repeats its first row and rank (loads that hit the
      // cache, never used) and a lane past the row's end its last float4: the loads carry no branch and all leave before the wait
      int64_t id[kInFlight];
      int kk[kInFlight], rk[kInFlight];
      int nk = 0;
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        const bool has = m != 0;
        const int k = has ? __ffsll((unsigned long long)m) - 1 : 0;
        m &= m - 1;
        const int t = __shfl(tok, gbase + k, 64);
        id[u] = (has || u == 0) ? (int64_t)t : id[0];
        kk[u] = has ? k : -1;
        rk[u] = has ? total - 1 - (cnt + u) : rk[0];                 // 0 <= rank < L: cnt + u < total <= L
        nk += has ? 1 : 0;
      }
      tt::f32x4 r[kInFlight][NV];
      float pb[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const int c = l + i * lpr;
          r[u][i] = table[id[u] * dim4 + (c < dim4 ? c : dim4 - 1)];
        }
        pb[u] = bias[rk[u]];
      }
      float e[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) e[u] = row_dot<NV>(r[u], a);
      for (int off = lpr >> 1; off > 0; off >>= 1) {                 // the four butterflies side by side
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) e[u] = __fadd_rn(e[u], __shfl_xor(e[u], off, 64));
      }
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        if (u < nk) {
          const float eu = __fmaf_rn(e[u], scale, pb[u]);
          if (kk[u] == l) my_e = eu;
          if (cnt == 0) {                                            // the first valid slot: weight exp(0) = 1, s starts AT its row
            mx = eu;
            den = 1.0f;
#pragma unroll
            for (int i = 0; i < NV; ++i) s[i] = r[u][i];
          } else {
            const float mn = fmaxf(mx, eu);
            const float alpha = __expf(__fsub_rn(mx, mn));           // one of the two is exp(0) = 1
            const float pw = __expf(__fsub_rn(eu, mn));
            den = __fmaf_rn(den, alpha, pw);
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
              for (int q = 0; q < 4; ++q) s[i][q] = __fmaf_rn(pw, r[u][i][q], __fmul_rn(s[i][q], alpha));
            mx = mn;
          }
          ++cnt;
        }
      }
    }
    if (live && slot < L && weights != nullptr) weights[b * L + slot] = my_e;   // parked: normalised below
  }
  if (!live) return;

  const float inv = cnt > 0 ? __fdiv_rn(1.0f, den) : 0.0f;          // a bag with one valid slot: exactly 1
  if (weights != nullptr) {                                          // every lane turns the logits IT parked into weights
    for (int base = 0; base < L; base += lpr) {
      const int slot = base + l;
      if (slot < L) {
        const float ev = weights[b * L + slot];
        weights[b * L + slot] = ev == -INFINITY ? 0.0f : __fmul_rn(__expf(__fsub_rn(ev, mx)), inv);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = l + i * lpr;
    if (c >= dim4) continue;
    tt::f32x4 p = s[i];                                              // cnt == 0: +0
    if (cnt > 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) p[q] = __fmul_rn(p[q], inv);
    }
    if (pooled_ != nullptr) reinterpret_cast<tt::f32x4*>(pooled_)[b * dim4 + c] = p;
    if constexpr (BASE) {
      if (cnt == 0) {                                                // empty bag: the base row itself
        p = o[i];
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) p[q] = __fadd_rn(o[i][q], p[q]);
      }
    }
    out[b * dim4 + c] = p;
  }
}

// Dynamic LDS: [groups][dim4 * 4] floats (the groups' da sums) followed by [groups][L] floats (their dp sums).
// KF rows in flight per lane: kInFlight up to dim 512, 2 beyond (3 or 4 float4 per row and lane: as many bytes, half the registers).
template <int NV, int KF>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const float* __restrict__ table_, int64_t table_rows, int dim4, int lpr_log2,
                                                       int L, const int64_t* __restrict__ batch_ids,
                                                       const float* __restrict__ weights, const float* __restrict__ pooled_,
                                                       const float* __restrict__ dy_, int64_t n_bags, const float* __restrict__ attn,
                                                       float scale, float* __restrict__ slot_grads_, float* __restrict__ slabs,
                                                       int64_t bags_per_slab) {
  extern __shared__ float lds[];
  const tt::f32x4* __restrict__ table = reinterpret_cast<const tt::f32x4*>(table_);
  tt::f32x4* __restrict__ slot_grads = reinterpret_cast<tt::f32x4*>(slot_grads_);
  const int dim = dim4 * 4;
  const int lpr = 1 << lpr_log2;
  const int groups = (int)blockDim.x >> lpr_log2;
  const int gi = threadIdx.x >> lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int gbase = (threadIdx.x & 63) & ~(lpr - 1);
  const uint64_t gmask = lpr == 64 ? ~0ull : ((1ull << lpr) - 1);
  float* __restrict__ lds_da = lds;
  float* __restrict__ lds_dp = lds + (int64_t)groups * dim + (int64_t)gi * L;   // this group's line
  for (int j = l; j < L; j += lpr) lds_dp[j] = 0.0f;                 // (written and read by this group's lanes only until the barrier)

  tt::f32x4 as[NV], da[NV];                                          // a / sqrt(dim); this group's sum of de_j h_j
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = l + i * lpr;
    as[i] = tt::f32x4{0.f, 0.f, 0.f, 0.f};
    da[i] = tt::f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < dim4) {
      const tt::f32x4 v = reinterpret_cast<const tt::f32x4*>(attn)[c];
#pragma unroll
      for (int q = 0; q < 4; ++q) as[i][q] = __fmul_rn(v[q], scale);
    }
  }

  const int64_t lo = (int64_t)blockIdx.x * bags_per_slab;
  const int64_t hi = lo + bags_per_slab < n_bags ? lo + bags_per_slab : n_bags;
  const int last_chunk = ((L - 1) >> lpr_log2) << lpr_log2;
  for (int64_t b0 = lo; b0 < hi; b0 += groups) {                     // (uniform over the workgroup: every lane reaches the ballots)
    const int64_t b = b0 + gi;
    const bool live = b < hi;
    tt::f32x4 g[NV];
    float gp = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = l + i * lpr;
      g[i] = tt::f32x4{0.f, 0.f, 0.f, 0.f};                          // (a lane past the row's end: zeros, nothing in a dot product)
      if (live && c < dim4) {
        g[i] = reinterpret_cast<const tt::f32x4*>(dy_)[b * dim4 + c];
        const tt::f32x4 pl = reinterpret_cast<const tt::f32x4*>(pooled_)[b * dim4 + c];
#pragma unroll
        for (int q = 0; q < 4; ++q) gp = __fmaf_rn(g[i][q], pl[q], gp);
      }
    }
    const float G = group_sum(gp, lpr);
    int rank = 0;                                                    // valid slots seen so far, from the bag's end
    for (int base = last_chunk; base >= 0; base -= lpr) {
      const int slot = base + l;
      int32_t tok = -1;
      float w = 0.0f;
      if (live && slot < L) {
        const int64_t id = batch_ids[b * L + slot];
        if (id >= 0 && id < table_rows) {                            // (the forward's ids; anything else is skipped, never read)
          tok = (int32_t)id;
          w = weights[b * L + slot];
        }
      }
      uint64_t m = (__ballot(tok >= 0) >> gbase) & gmask;
      while (m != 0) {
        int64_t id[KF];
        int kk[KF];
        float wk[KF];
        int nk = 0;
#pragma unroll
        for (int u = 0; u < KF; ++u) {                        // newest first: the highest set bit
          const bool has = m != 0;
          const int k = has ? 63 - __clzll((unsigned long long)m) : 0;
          m &= ~(1ull << k);
          const int t = __shfl(tok, gbase + k, 64);
          const float wt = __shfl(w, gbase + k, 64);
          id[u] = (has || u == 0) ? (int64_t)t : id[0];
          kk[u] = k;
          wk[u] = wt;
          nk += has ? 1 : 0;
        }
        tt::f32x4 r[KF][NV];
#pragma unroll
        for (int u = 0; u < KF; ++u)
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            const int c = l + i * lpr;
            r[u][i] = table[id[u] * dim4 + (c < dim4 ? c : dim4 - 1)];
          }
        float t[KF];
#pragma unroll
        for (int u = 0; u < KF; ++u) t[u] = row_dot<NV>(r[u], g);
        for (int off = lpr >> 1; off > 0; off >>= 1) {
#pragma unroll
          for (int u = 0; u < KF; ++u) t[u] = __fadd_rn(t[u], __shfl_xor(t[u], off, 64));
        }
#pragma unroll
        for (int u = 0; u < KF; ++u) {
          if (u < nk) {
            const float de = __fmul_rn(wk[u], __fsub_rn(t[u], G));
            const int64_t grow = (b * L + base + kk[u]) * dim4;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
              const int c = l + i * lpr;
              if (c < dim4) {
                tt::f32x4 dh;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  dh[q] = __fmaf_rn(de, as[i][q], __fmul_rn(wk[u], g[i][q]));
                  da[i][q] = __fmaf_rn(de, r[u][i][q], da[i][q]);
                }
                slot_grads[grow + c] = dh;
              }
            }
            if (l == 0) lds_dp[rank] = __fadd_rn(lds_dp[rank], de);  // rank < L: at most L valid slots
            ++rank;
          }
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = l + i * lpr;
    if (c < dim4) {
#pragma unroll
      for (int q = 0; q < 4; ++q) lds_da[(int64_t)gi * dim + c * 4 + q] = da[i][q];
    }
  }
  __syncthreads();
  float* __restrict__ slab = slabs + (int64_t)blockIdx.x * (dim + L);
  const float* __restrict__ all_dp = lds + (int64_t)groups * dim;
  for (int j = threadIdx.x; j < dim + L; j += blockDim.x) {          // the groups' sums, in ascending group order
    float v = 0.0f;
    if (j < dim) {
      for (int gq = 0; gq < groups; ++gq) v = __fadd_rn(v, lds_da[(int64_t)gq * dim + j]);
      v = __fmul_rn(v, scale);
    } else {
      for (int gq = 0; gq < groups; ++gq) v = __fadd_rn(v, all_dp[(int64_t)gq * L + (j - dim)]);
    }
    slab[j] = v;
  }
}

int lane_group(int dim4, int* nv) {
  int lg = 0;
  while ((1 << lg) < dim4 && lg < 6) ++lg;
  *nv = (dim4 + (1 << lg) - 1) >> lg;                                // 1 up to dim 256, then ceil(dim / 256) <= 4
  return lg;
}

}  // namespace

extern "C" int tt_history_attention_fwd_f32(const float* table, int64_t table_rows, int32_t dim, const int32_t* tokens,
                                            int64_t n_token_rows, int32_t L, const int64_t* bag_rows, int64_t n_bags,
                                            const float* attn, float* out, int64_t* batch_ids, float* weights, float* pooled,
                                            int32_t* oob_flag, const int64_t* exclude, const float* base_table, int64_t base_rows,
                                            const int64_t* base_ids, tt_stream_t stream) {
  const char* what = "tt_history_attention_fwd_f32";
  TT_REQUIRE(dim >= 4 && dim <= 1024 && dim % 4 == 0, "%s: dim must be a multiple of 4 in 4..1024 (got %d)", what, dim);
  TT_REQUIRE(L >= 1 && L <= 64, "%s: L must be in 1..64 (got %d)", what, L);
  TT_REQUIRE(table_rows > 0 && n_token_rows >= 0 && n_bags >= 0, "%s: need table_rows > 0, n_token_rows >= 0, n_bags >= 0", what);
  TT_REQUIRE(bag_rows != nullptr || n_bags == n_token_rows,
             "%s: bag_rows is NULL (identity), so n_bags (%lld) must equal n_token_rows (%lld)", what, (long long)n_bags,
             (long long)n_token_rows);
  TT_REQUIRE(n_bags <= 0x7fffffff / (int64_t)L, "%s: n_bags * L must fit 31 bits (the sort plan's positions are int32)", what);
  TT_REQUIRE((base_table != nullptr) == (base_ids != nullptr), "%s: base_table and base_ids go together (both NULL or both given)", what);
  TT_REQUIRE(base_table == nullptr || base_rows > 0, "%s: need base_rows > 0 with a base", what);
  if (n_bags == 0) return TT_OK;
  TT_REQUIRE(table && out && attn && (tokens || n_token_rows == 0), "%s: null pointer (table / out / attn / tokens)", what);
  TT_REQUIRE(tt::aligned16(table) && tt::aligned16(out) && tt::aligned16(attn), "%s: table / out / attn must be 16-byte aligned", what);
  TT_REQUIRE(pooled == nullptr || tt::aligned16(pooled), "%s: pooled must be 16-byte aligned", what);
  TT_REQUIRE(base_table == nullptr || tt::aligned16(base_table), "%s: base_table must be 16-byte aligned", what);
  const int dim4 = dim / 4;
  int nv = 1;
  const int lg = lane_group(dim4, &nv);
  const int64_t groups = 256 >> lg;
  const int64_t blocks = (n_bags + groups - 1) / groups;
  TT_REQUIRE(blocks <= 0x7fffffff, "%s: too many bags", what);
  const dim3 grid((unsigned)blocks), block(256);
  const float scale = 1.0f / sqrtf((float)dim);
  hipStream_t s = tt::as_stream(stream);
#define TT_ATTN_LAUNCH(NV, EXCL, BASE)                                                                                         \
  tt::launch("history_attn_fwd", attn_fwd_kernel<NV, EXCL, BASE>, grid, block, 0, s, table, table_rows, dim4, lg, tokens,      \
             n_token_rows, (int)L, bag_rows, n_bags, attn, scale, out, batch_ids, weights, pooled, oob_flag, exclude,           \
             base_table, base_rows, base_ids)
#define TT_ATTN_LAUNCH_NV(EXCL, BASE)                                                                                          \
  switch (nv) {                                                                                                                \
    case 1: TT_ATTN_LAUNCH(1, EXCL, BASE); break;                                                                              \
    case 2: TT_ATTN_LAUNCH(2, EXCL, BASE); break;                                                                              \
    case 3: TT_ATTN_LAUNCH(3, EXCL, BASE); break;                                                                              \
    default: TT_ATTN_LAUNCH(4, EXCL, BASE); break;                                                                             \
  }
  if (exclude != nullptr && base_table != nullptr) {
    TT_ATTN_LAUNCH_NV(true, true);
  } else if (exclude != nullptr) {
    TT_ATTN_LAUNCH_NV(true, false);
  } else if (base_table != nullptr) {
    TT_ATTN_LAUNCH_NV(false, true);
  } else {
    TT_ATTN_LAUNCH_NV(false, false);
  }
#undef TT_ATTN_LAUNCH_NV
#undef TT_ATTN_LAUNCH
  return tt::check_launch(what);
}

// 8 bags per slab (one per lane group of a workgroup at dim 128: every group gathers at once), at most 1024 slabs.
extern "C" int32_t tt_history_attention_num_slabs(int64_t n_bags) {
  if (n_bags <= 0) return 1;
  const int64_t n = (n_bags + 7) / 8;
  return (int32_t)(n < 1024 ? n : 1024);
}

extern "C" int tt_history_attention_bwd_f32(const float* table, int64_t table_rows, int32_t dim, int32_t L, const int64_t* batch_ids,
                                            const float* weights, const float* pooled, const float* dy, int64_t n_bags,
                                            const float* attn, float* slot_grads, float* dattn_slabs, int32_t n_slabs,
                                            tt_stream_t stream) {
  const char* what = "tt_history_attention_bwd_f32";
  TT_REQUIRE(dim >= 4 && dim <= 1024 && dim % 4 == 0, "%s: dim must be a multiple of 4 in 4..1024 (got %d)", what, dim);
  TT_REQUIRE(L >= 1 && L <= 64, "%s: L must be in 1..64 (got %d)", what, L);
  TT_REQUIRE(table_rows > 0 && n_bags >= 0, "%s: need table_rows > 0 and n_bags >= 0", what);
  TT_REQUIRE(n_bags <= 0x7fffffff / (int64_t)L, "%s: n_bags * L must fit 31 bits (the sort plan's positions are int32)", what);
  TT_REQUIRE(n_slabs >= 1 && n_slabs <= 65536, "%s: n_slabs must be in 1..65536 (got %d)", what, n_slabs);
  if (n_bags == 0) return TT_OK;
  TT_REQUIRE(table && batch_ids && weights && pooled && dy && attn && slot_grads && dattn_slabs,
             "%s: null pointer (table / batch_ids / weights / pooled / dy / attn / slot_grads / dattn_slabs)", what);
  TT_REQUIRE(tt::aligned16(table) && tt::aligned16(pooled) && tt::aligned16(dy) && tt::aligned16(attn) && tt::aligned16(slot_grads),
             "%s: table / pooled / dy / attn / slot_grads must be 16-byte aligned", what);
  const int dim4 = dim / 4;
  int nv = 1;
  const int lg = lane_group(dim4, &nv);
  // the workgroup: 256 threads, halved while its groups' LDS lines (dim + L floats each) exceed 48 KiB (dim 4..16 at a long L)
  int threads = 256;
  while (threads > 64 && (size_t)(threads >> lg) * (dim + L) * sizeof(float) > 48 * 1024) threads >>= 1;
  const unsigned lds = (unsigned)((size_t)(threads >> lg) * (dim + L) * sizeof(float));
  const int64_t per = (n_bags + n_slabs - 1) / n_slabs;
  const dim3 grid((unsigned)n_slabs), block((unsigned)threads);
  hipStream_t s = tt::as_stream(stream);
#define TT_ATTN_BWD(NV)                                                                                                        \
  tt::launch("history_attn_bwd", attn_bwd_kernel<NV, (NV >= 3 ? 2 : kInFlight)>, grid, block, lds, s, table, table_rows, dim4, lg, (int)L, batch_ids,     \
             weights, pooled, dy, n_bags, attn, 1.0f / sqrtf((float)dim), slot_grads, dattn_slabs, per)
  switch (nv) {
    case 1: TT_ATTN_BWD(1); break;
    case 2: TT_ATTN_BWD(2); break;
    case 3: TT_ATTN_BWD(3); break;
    default: TT_ATTN_BWD(4); break;
  }
#undef TT_ATTN_BWD
  return tt::check_launch(what);
}
