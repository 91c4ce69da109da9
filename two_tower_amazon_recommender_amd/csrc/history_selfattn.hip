// Multi-head self-attention encoder of the user history (history_pooling = "self_attention"): one SASRec-style causal attention
// block read at the LAST position only, so the one query of a bag is its newest kept item.  With the kept slots j of bag b
// (padding, out-of-range tokens and the excluded item skipped exactly as in tt_history_attention_fwd_f32), r_j = kept slots
// behind j and n the kept slot with r = 0:
//   x_j = table[token_j]      T = x_n Wqk  [H D]      e_hj = <x_j, T_h> / sqrt(D) + p[h, r_j]      w_h = softmax_j(e_h)
//   P_h = sum_j w_hj x_j      O = concat_h(P_h) Wvo   out[b] = base row + O
// Wqk's head block is Wq_h Wk_h^T kept as one D x D form and Wvo's is Wv_h Wo_h, so both GEMMs run over n_bags rows (the tower
// entry points, tt_dense_fwd_batched_f32 / tt_dense_bwd_batched_f32) and never over n_bags * L.  The launches of this file:
//   resolve     tokens, bag_rows, exclude -> batch_ids [n_bags * L] (-1: skipped), newest [n_bags] (the slot of n; -1: no kept
//               slot) and xn [n_bags, D] (the newest kept row; +0 for an emptied bag); the out-of-range flag of the history launches
//               (token, bag row, base id; -1 is silent).
//   pool fwd    history_attn.hip's forward with H queries per bag: a group of LPR lanes (the power of two >= D / 4, one float4 per
//               lane) owns a bag, a slot's row is loaded ONCE and dotted with all H query rows (a fixed fmaf chain in the lane, a
//               fixed xor butterfly over the group), one online softmax per head, kInFlight row loads leave before the first wait.
//               The logits are parked in ``weights`` [n_bags, H, L] and normalised by the lane that wrote them.
//               4 D (sum(cnt) + 2 H n_bags) bytes (the rows, T, P); 4 H D VALU FLOP per kept slot.
//   combine     out[b] = base row + out[b] in place behind the O GEMM (an emptied bag: the base row's bits).
//   pool bwd    one pass over the rows per bag, newest first (the rank is a running count): G_h = <dP_h, P_h>, t_hj = <dP_h, x_j>,
//               de_hj = w_hj (t_hj - G_h), dx_j = sum_h (w_hj dP_h + de_hj T_h / sqrt(D)) -> slot_grads[b L + j] (a skipped slot's
//               row is left untouched), dT_h = sum_j de_hj x_j / sqrt(D) -> dT [n_bags, H D] (every row written), and dp[h, r_j] +=
//               de_hj per lane group in LDS, the groups of workgroup s (the contiguous bags of slab s) added in ascending order ->
//               dp_slabs[s] [H L]: every slab in full, no atomics, no pre-zeroing.
//   query grad  slot_grads[b L + newest[b]] += dxn[b]: the newest row's share through T = x_n Wqk.
// No atomics (but the flag), no workspace to zero, nothing read back: a bag's bits depend on that bag alone.
#include "common.h"

namespace {

using tt::f32x4;

constexpr int kInFlight = 4;
constexpr int MAXL = 64;

__device__ __forceinline__ float group_sum(float v, int lpr) {
  for (int off = lpr >> 1; off > 0; off >>= 1) v = __fadd_rn(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ float row_dot(const f32x4& r, const f32x4& a) {
  float d = 0.0f;
#pragma unroll
  for (int q = 0; q < 4; ++q) d = __fmaf_rn(r[q], a[q], d);
  return d;
}

__global__ __launch_bounds__(256) void sa_resolve_kernel(const float* __restrict__ table_, int64_t table_rows, int dim4, int lpr_log2,
                                                         const int32_t* __restrict__ tokens, int64_t n_token_rows, int L,
                                                         const int64_t* __restrict__ bag_rows, int64_t n_bags,
                                                         const int64_t* __restrict__ exclude, const int64_t* __restrict__ base_ids,
                                                         int64_t base_rows, int64_t* __restrict__ batch_ids,
                                                         int32_t* __restrict__ newest, float* __restrict__ xn_,
                                                         int32_t* __restrict__ oob_flag) {
  const f32x4* __restrict__ table = reinterpret_cast<const f32x4*>(table_);
  const int lpr = 1 << lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int gbase = (threadIdx.x & 63) & ~(lpr - 1);
  const uint64_t gmask = lpr == 64 ? ~0ull : ((1ull << lpr) - 1);
  const int64_t b = (int64_t)blockIdx.x * (256 >> lpr_log2) + (threadIdx.x >> lpr_log2);
  const bool live = b < n_bags;

  int64_t row = -1, ex = -1;
  if (live) {
    row = bag_rows != nullptr ? bag_rows[b] : b;
    if (exclude != nullptr) ex = exclude[b];
    if (base_ids != nullptr) {
      const int64_t bid = base_ids[b];
      if ((bid < 0 || bid >= base_rows) && bid != -1 && l == 0 && oob_flag != nullptr) atomicOr(oob_flag, 1);
    }
    if (row < 0 || row >= n_token_rows) {
      if (row != -1 && l == 0 && oob_flag != nullptr) atomicOr(oob_flag, 1);
      row = -1;
    }
  }
  int nw = -1;                                                       // the newest kept slot and its token
  int32_t nw_tok = 0;
  for (int base = 0; base < L; base += lpr) {                        // (L is uniform: every lane of the wave reaches the ballot)
    const int slot = base + l;
    int32_t tok = -1;
    if (row >= 0 && slot < L) {
      tok = tokens[row * L + slot];
      if (exclude != nullptr && (int64_t)tok == ex) tok = -1;        // the raw token, compared in int64: skipped like padding
      if (tok < 0 || (int64_t)tok >= table_rows) {
        if (tok != -1 && oob_flag != nullptr) atomicOr(oob_flag, 1);
        tok = -1;
      }
    }
    if (live && slot < L) batch_ids[b * L + slot] = (int64_t)tok;
    const uint64_t m = (__ballot(tok >= 0) >> gbase) & gmask;
    const int k = m != 0 ? 63 - __clzll((unsigned long long)m) : 0;
    const int32_t t = __shfl(tok, gbase + k, 64);
    if (m != 0) {
      nw = base + k;
      nw_tok = t;
    }
  }
  if (!live) return;
  if (l == 0) newest[b] = nw;
  if (l < dim4) {
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (nw >= 0) v = table[(int64_t)nw_tok * dim4 + l];
    reinterpret_cast<f32x4*>(xn_)[b * dim4 + l] = v;
  }
}

template <int H, int KF>
__global__ __launch_bounds__(256) void sa_pool_fwd_kernel(const float* __restrict__ table_, int64_t table_rows, int dim4, int lpr_log2,
                                                          int L, const int64_t* __restrict__ batch_ids, int64_t n_bags,
                                                          const float* __restrict__ T_, const float* __restrict__ p, float scale,
                                                          float* __restrict__ P_, float* weights) {
  const f32x4* __restrict__ table = reinterpret_cast<const f32x4*>(table_);
  const int lpr = 1 << lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int gbase = (threadIdx.x & 63) & ~(lpr - 1);
  const uint64_t gmask = lpr == 64 ? ~0ull : ((1ull << lpr) - 1);
  const int64_t b = (int64_t)blockIdx.x * (256 >> lpr_log2) + (threadIdx.x >> lpr_log2);
  const bool live = b < n_bags;
  const int cl = l < dim4 ? l : dim4 - 1;                            // a lane past the row's end re-reads the last float4 ...

  f32x4 th[H];                                                       // ... against a zero query: nothing in a dot product
#pragma unroll
  for (int h = 0; h < H; ++h) {
    th[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live && l < dim4) th[h] = reinterpret_cast<const f32x4*>(T_)[(b * H + h) * dim4 + l];
  }

  auto slot_token = [&](int slot) -> int32_t {                       // the resolve launch's ids; anything else is skipped, never read
    int32_t tok = -1;
    if (live && slot < L) {
      const int64_t id = batch_ids[b * L + slot];
      if (id >= 0 && id < table_rows) tok = (int32_t)id;
    }
    return tok;
  };

  int total = 0;                                                     // pass 1: the kept slots (the ranks count from the bag's end)
  for (int base = 0; base < L; base += lpr) total += __popcll((__ballot(slot_token(base + l) >= 0) >> gbase) & gmask);

  f32x4 s[H];
  float mx[H], den[H];
#pragma unroll
  for (int h = 0; h < H; ++h) {
    s[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    mx[h] = 0.0f;
    den[h] = 0.0f;
  }
  int cnt = 0;
  for (int base = 0; base < L; base += lpr) {                        // pass 2: the rows, in ascending slot order
    const int slot = base + l;
    const int32_t tok = slot_token(slot);
    float my_e[H];
#pragma unroll
    for (int h = 0; h < H; ++h) my_e[h] = -INFINITY;
    uint64_t m = (__ballot(tok >= 0) >> gbase) & gmask;
    while (m != 0) {                                                 // (m is uniform inside a group: its lanes stay together)
      int64_t id[KF];
      int kk[KF], rk[KF];
      int nk = 0;
#pragma unroll
      for (int u = 0; u < KF; ++u) {                                 // a short batch repeats its first row and rank: never used
        const bool has = m != 0;
        const int k = has ? __ffsll((unsigned long long)m) - 1 : 0;
        m &= m - 1;
        const int t = __shfl(tok, gbase + k, 64);
        id[u] = (has || u == 0) ? (int64_t)t : id[0];
        kk[u] = has ? k : -1;
        rk[u] = has ? total - 1 - (cnt + u) : rk[0];                 // 0 <= rank < L: cnt + u < total <= L
        nk += has ? 1 : 0;
      }
      f32x4 r[KF];
      float e[KF][H], pb[KF][H];
#pragma unroll
      for (int u = 0; u < KF; ++u) {
        r[u] = table[id[u] * dim4 + cl];
#pragma unroll
        for (int h = 0; h < H; ++h) pb[u][h] = p[h * L + rk[u]];
      }
#pragma unroll
      for (int u = 0; u < KF; ++u)
#pragma unroll
        for (int h = 0; h < H; ++h) e[u][h] = row_dot(r[u], th[h]);
      for (int off = lpr >> 1; off > 0; off >>= 1) {                 // the butterflies side by side
#pragma unroll
        for (int u = 0; u < KF; ++u)
#pragma unroll
          for (int h = 0; h < H; ++h) e[u][h] = __fadd_rn(e[u][h], __shfl_xor(e[u][h], off, 64));
      }
#pragma unroll
      for (int u = 0; u < KF; ++u) {
        if (u < nk) {
#pragma unroll
          for (int h = 0; h < H; ++h) {
            const float eu = __fmaf_rn(e[u][h], scale, pb[u][h]);
            if (kk[u] == l) my_e[h] = eu;
            if (cnt == 0) {                                          // the first kept slot: weight exp(0) = 1, s starts AT its row
              mx[h] = eu;
              den[h] = 1.0f;
              s[h] = r[u];
            } else {
              const float mn = fmaxf(mx[h], eu);
              const float alpha = __expf(__fsub_rn(mx[h], mn));      // one of the two is exp(0) = 1
              const float pw = __expf(__fsub_rn(eu, mn));
              den[h] = __fmaf_rn(den[h], alpha, pw);
#pragma unroll
              for (int q = 0; q < 4; ++q) s[h][q] = __fmaf_rn(pw, r[u][q], __fmul_rn(s[h][q], alpha));
              mx[h] = mn;
            }
          }
          ++cnt;
        }
      }
    }
    if (live && slot < L) {                                          // parked: normalised below
#pragma unroll
      for (int h = 0; h < H; ++h) weights[(b * H + h) * L + slot] = my_e[h];
    }
  }
  if (!live) return;

#pragma unroll
  for (int h = 0; h < H; ++h) {
    const float inv = cnt > 0 ? __fdiv_rn(1.0f, den[h]) : 0.0f;      // a bag with one kept slot: exactly 1
    for (int base = 0; base < L; base += lpr) {                      // every lane turns the logits IT parked into weights
      const int slot = base + l;
      if (slot < L) {
        const float ev = weights[(b * H + h) * L + slot];
        weights[(b * H + h) * L + slot] = ev == -INFINITY ? 0.0f : __fmul_rn(__expf(__fsub_rn(ev, mx[h])), inv);
      }
    }
    if (l < dim4) {
      f32x4 v = s[h];                                                // cnt == 0: +0
      if (cnt > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = __fmul_rn(v[q], inv);
      }
      reinterpret_cast<f32x4*>(P_)[(b * H + h) * dim4 + l] = v;
    }
  }
}

__global__ __launch_bounds__(256) void sa_combine_kernel(float* __restrict__ out_, const int32_t* __restrict__ newest, int64_t n_bags,
                                                         int dim4, const float* __restrict__ base_table_, int64_t base_rows,
                                                         const int64_t* __restrict__ base_ids) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_bags * dim4) return;
  const int64_t b = i / dim4;
  const int c = (int)(i - b * dim4);
  const int64_t bid = base_ids[b];
  f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};                               // a base id out of range: a zero row
  if (bid >= 0 && bid < base_rows) o = reinterpret_cast<const f32x4*>(base_table_)[bid * dim4 + c];
  if (newest[b] >= 0) {                                              // (an emptied bag: the base row itself)
    const f32x4 v = reinterpret_cast<const f32x4*>(out_)[i];
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = __fadd_rn(o[q], v[q]);
  }
  reinterpret_cast<f32x4*>(out_)[i] = o;
}

// Dynamic LDS: [groups][H * L] floats, the groups' dp sums.
template <int H, int KF>
__global__ __launch_bounds__(256) void sa_pool_bwd_kernel(const float* __restrict__ table_, int64_t table_rows, int dim4, int lpr_log2,
                                                          int L, const int64_t* __restrict__ batch_ids,
                                                          const float* __restrict__ weights, const float* __restrict__ P_,
                                                          const float* __restrict__ dP_, const float* __restrict__ T_, int64_t n_bags,
                                                          float scale, float* __restrict__ slot_grads_, float* __restrict__ dT_,
                                                          float* __restrict__ slabs, int64_t bags_per_slab) {
  extern __shared__ float lds[];
  const f32x4* __restrict__ table = reinterpret_cast<const f32x4*>(table_);
  f32x4* __restrict__ slot_grads = reinterpret_cast<f32x4*>(slot_grads_);
  const int lpr = 1 << lpr_log2;
  const int groups = (int)blockDim.x >> lpr_log2;
  const int gi = threadIdx.x >> lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int gbase = (threadIdx.x & 63) & ~(lpr - 1);
  const uint64_t gmask = lpr == 64 ? ~0ull : ((1ull << lpr) - 1);
  const int cl = l < dim4 ? l : dim4 - 1;
  const int HL = H * L;
  float* __restrict__ lds_dp = lds + (int64_t)gi * HL;               // this group's line
  for (int j = l; j < HL; j += lpr) lds_dp[j] = 0.0f;                // (written and read by this group's lanes only until the barrier)

  const int64_t lo = (int64_t)blockIdx.x * bags_per_slab;
  const int64_t hi = lo + bags_per_slab < n_bags ? lo + bags_per_slab : n_bags;
  const int last_chunk = ((L - 1) >> lpr_log2) << lpr_log2;
  for (int64_t b0 = lo; b0 < hi; b0 += groups) {                     // (uniform over the workgroup: every lane reaches the ballots)
    const int64_t b = b0 + gi;
    const bool live = b < hi;
    f32x4 g[H], ts[H], dT[H];                                        // dP_h, T_h / sqrt(D), sum_j de_hj x_j
    float G[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
      g[h] = f32x4{0.f, 0.f, 0.f, 0.f};                              // (a lane past the row's end: zeros, nothing in a dot product)
      ts[h] = f32x4{0.f, 0.f, 0.f, 0.f};
      dT[h] = f32x4{0.f, 0.f, 0.f, 0.f};
      float gp = 0.0f;
      if (live && l < dim4) {
        const int64_t at = (b * H + h) * dim4 + l;
        g[h] = reinterpret_cast<const f32x4*>(dP_)[at];
        const f32x4 pl = reinterpret_cast<const f32x4*>(P_)[at];
        const f32x4 tv = reinterpret_cast<const f32x4*>(T_)[at];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          gp = __fmaf_rn(g[h][q], pl[q], gp);
          ts[h][q] = __fmul_rn(tv[q], scale);
        }
      }
      G[h] = group_sum(gp, lpr);
    }
    int rank = 0;                                                    // kept slots seen so far, from the bag's end
    for (int base = last_chunk; base >= 0; base -= lpr) {
      const int slot = base + l;
      int32_t tok = -1;
      float w[H];
#pragma unroll
      for (int h = 0; h < H; ++h) w[h] = 0.0f;
      if (live && slot < L) {
        const int64_t id = batch_ids[b * L + slot];
        if (id >= 0 && id < table_rows) {                            // (the forward's ids; anything else is skipped, never read)
          tok = (int32_t)id;
#pragma unroll
          for (int h = 0; h < H; ++h) w[h] = weights[(b * H + h) * L + slot];
        }
      }
      uint64_t m = (__ballot(tok >= 0) >> gbase) & gmask;
      while (m != 0) {
        int64_t id[KF];
        int kk[KF];
        float wk[KF][H];
        int nk = 0;
#pragma unroll
        for (int u = 0; u < KF; ++u) {                               // newest first: the highest set bit
          const bool has = m != 0;
          const int k = has ? 63 - __clzll((unsigned long long)m) : 0;
          m &= ~(1ull << k);
          const int t = __shfl(tok, gbase + k, 64);
#pragma unroll
          for (int h = 0; h < H; ++h) wk[u][h] = __shfl(w[h], gbase + k, 64);
          id[u] = (has || u == 0) ? (int64_t)t : id[0];
          kk[u] = k;
          nk += has ? 1 : 0;
        }
        f32x4 r[KF];
#pragma unroll
        for (int u = 0; u < KF; ++u) r[u] = table[id[u] * dim4 + cl];
        float t[KF][H];
#pragma unroll
        for (int u = 0; u < KF; ++u)
#pragma unroll
          for (int h = 0; h < H; ++h) t[u][h] = row_dot(r[u], g[h]);
        for (int off = lpr >> 1; off > 0; off >>= 1) {
#pragma unroll
          for (int u = 0; u < KF; ++u)
#pragma unroll
            for (int h = 0; h < H; ++h) t[u][h] = __fadd_rn(t[u][h], __shfl_xor(t[u][h], off, 64));
        }
#pragma unroll
        for (int u = 0; u < KF; ++u) {
          if (u < nk) {
            f32x4 dh = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int h = 0; h < H; ++h) {
              const float de = __fmul_rn(wk[u][h], __fsub_rn(t[u][h], G[h]));
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                dh[q] = __fmaf_rn(de, ts[h][q], __fmaf_rn(wk[u][h], g[h][q], dh[q]));
                dT[h][q] = __fmaf_rn(de, r[u][q], dT[h][q]);
              }
              if (l == 0) lds_dp[h * L + rank] = __fadd_rn(lds_dp[h * L + rank], de);   // rank < L: at most L kept slots
            }
            if (l < dim4) slot_grads[(b * L + base + kk[u]) * dim4 + l] = dh;
            ++rank;
          }
        }
      }
    }
    if (live && l < dim4) {
#pragma unroll
      for (int h = 0; h < H; ++h) {
        f32x4 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = __fmul_rn(dT[h][q], scale);
        reinterpret_cast<f32x4*>(dT_)[(b * H + h) * dim4 + l] = v;
      }
    }
  }
  __syncthreads();
  float* __restrict__ slab = slabs + (int64_t)blockIdx.x * HL;
  for (int j = threadIdx.x; j < HL; j += blockDim.x) {               // the groups' sums, in ascending group order
    float v = 0.0f;
    for (int gq = 0; gq < groups; ++gq) v = __fadd_rn(v, lds[(int64_t)gq * HL + j]);
    slab[j] = v;
  }
}

__global__ __launch_bounds__(256) void sa_query_grad_kernel(const int32_t* __restrict__ newest, const float* __restrict__ dxn_,
                                                            int64_t n_bags, int L, int dim4, float* __restrict__ slot_grads_) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_bags * dim4) return;
  const int64_t b = i / dim4;
  const int c = (int)(i - b * dim4);
  const int nw = newest[b];
  if (nw < 0 || nw >= L) return;
  f32x4* dst = reinterpret_cast<f32x4*>(slot_grads_) + (b * L + nw) * dim4 + c;
  const f32x4 d = reinterpret_cast<const f32x4*>(dxn_)[i];
  f32x4 v = *dst;
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = __fadd_rn(v[q], d[q]);
  *dst = v;
}

int check_shape(const char* what, int32_t D, int32_t L, int64_t n_bags) {
  TT_REQUIRE(D >= 32 && D <= 256 && D % 32 == 0, "%s: dim must be a multiple of 32 in 32..256 (got %d)", what, D);
  TT_REQUIRE(L >= 1 && L <= MAXL, "%s: L must be in 1..64 (got %d)", what, L);
  TT_REQUIRE(n_bags >= 0, "%s: n_bags must be >= 0", what);
  TT_REQUIRE(n_bags <= 0x7fffffff / (int64_t)L, "%s: n_bags * L must fit 31 bits (the sort plan's positions are int32)", what);
  return TT_OK;
}

int check_heads(const char* what, int32_t H) {
  TT_REQUIRE(H == 1 || H == 2 || H == 4 || H == 8, "%s: heads must be 1, 2, 4 or 8 (got %d)", what, H);
  return TT_OK;
}

int lane_group_log2(int dim4) {                                      // dim4 in 8..64: one float4 per lane
  int lg = 3;
  while ((1 << lg) < dim4) ++lg;
  return lg;
}

}  // namespace

extern "C" int tt_history_self_attention_resolve_f32(const float* table, int64_t table_rows, int32_t dim, const int32_t* tokens,
                                                     int64_t n_token_rows, int32_t L, const int64_t* bag_rows, int64_t n_bags,
                                                     const int64_t* exclude, const int64_t* base_ids, int64_t base_rows,
                                                     int64_t* batch_ids, int32_t* newest, float* xn, int32_t* oob_flag,
                                                     tt_stream_t stream) {
  const char* what = "tt_history_self_attention_resolve_f32";
  if (int rc = check_shape(what, dim, L, n_bags)) return rc;
  TT_REQUIRE(table_rows > 0 && n_token_rows >= 0, "%s: need table_rows > 0 and n_token_rows >= 0", what);
  TT_REQUIRE(bag_rows != nullptr || n_bags == n_token_rows,
             "%s: bag_rows is NULL (identity), so n_bags (%lld) must equal n_token_rows (%lld)", what, (long long)n_bags,
             (long long)n_token_rows);
  TT_REQUIRE(base_ids == nullptr || base_rows > 0, "%s: need base_rows > 0 with base_ids", what);
  if (n_bags == 0) return TT_OK;
  TT_REQUIRE(table && batch_ids && newest && xn && (tokens || n_token_rows == 0),
             "%s: null pointer (table / batch_ids / newest / xn / tokens)", what);
  TT_REQUIRE(tt::aligned16(table) && tt::aligned16(xn), "%s: table and xn must be 16-byte aligned", what);
  const int dim4 = dim / 4;
  const int lg = lane_group_log2(dim4);
  const int64_t groups = 256 >> lg;
  const int64_t blocks = (n_bags + groups - 1) / groups;
  tt::launch("history_selfattn_resolve", sa_resolve_kernel, dim3((unsigned)blocks), dim3(256), 0, tt::as_stream(stream), table,
             table_rows, dim4, lg, tokens, n_token_rows, (int)L, bag_rows, n_bags, exclude, base_ids, base_rows, batch_ids, newest, xn,
             oob_flag);
  return tt::check_launch(what);
}

extern "C" int tt_history_self_attention_pool_fwd_f32(const float* table, int64_t table_rows, int32_t dim, int32_t L, int32_t heads,
                                                      const int64_t* batch_ids, int64_t n_bags, const float* t, const float* p,
                                                      float* pooled, float* weights, tt_stream_t stream) {
  const char* what = "tt_history_self_attention_pool_fwd_f32";
  if (int rc = check_shape(what, dim, L, n_bags)) return rc;
  if (int rc = check_heads(what, heads)) return rc;
  TT_REQUIRE(table_rows > 0, "%s: need table_rows > 0", what);
  if (n_bags == 0) return TT_OK;
  TT_REQUIRE(table && batch_ids && t && p && pooled && weights, "%s: null pointer (table / batch_ids / t / p / pooled / weights)", what);
  TT_REQUIRE(tt::aligned16(table) && tt::aligned16(t) && tt::aligned16(pooled), "%s: table, t and pooled must be 16-byte aligned", what);
  const int dim4 = dim / 4;
  const int lg = lane_group_log2(dim4);
  const int64_t groups = 256 >> lg;
  const int64_t blocks = (n_bags + groups - 1) / groups;
  const dim3 grid((unsigned)blocks), block(256);
  const float scale = 1.0f / sqrtf((float)dim);
  hipStream_t s = tt::as_stream(stream);
#define TT_SA_FWD(H, KF)                                                                                                       \
  tt::launch("history_selfattn_pool_fwd", sa_pool_fwd_kernel<H, KF>, grid, block, 0, s, table, table_rows, dim4, lg, (int)L,   \
             batch_ids, n_bags, t, p, scale, pooled, weights)
  switch (heads) {
    case 1: TT_SA_FWD(1, kInFlight); break;
    case 2: TT_SA_FWD(2, kInFlight); break;
    case 4: TT_SA_FWD(4, kInFlight); break;
    default: TT_SA_FWD(8, 2); break;                                 // 8 heads: half the rows in flight, as many registers
  }
#undef TT_SA_FWD
  return tt::check_launch(what);
}

extern "C" int tt_history_self_attention_combine_f32(float* out, const int32_t* newest, int64_t n_bags, int32_t dim,
                                                     const float* base_table, int64_t base_rows, const int64_t* base_ids,
                                                     tt_stream_t stream) {
  const char* what = "tt_history_self_attention_combine_f32";
  if (int rc = check_shape(what, dim, 1, n_bags)) return rc;
  TT_REQUIRE(base_rows > 0, "%s: need base_rows > 0", what);
  if (n_bags == 0) return TT_OK;
  TT_REQUIRE(out && newest && base_table && base_ids, "%s: null pointer (out / newest / base_table / base_ids)", what);
  TT_REQUIRE(tt::aligned16(out) && tt::aligned16(base_table), "%s: out and base_table must be 16-byte aligned", what);
  const int dim4 = dim / 4;
  const int64_t blocks = (n_bags * dim4 + 255) / 256;
  tt::launch("history_selfattn_combine", sa_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, tt::as_stream(stream), out, newest,
             n_bags, dim4, base_table, base_rows, base_ids);
  return tt::check_launch(what);
}

// 8 bags per slab (one per lane group of a workgroup at dim 128: every group gathers at once), at most 1024 slabs.
extern "C" int32_t tt_history_self_attention_num_slabs(int64_t n_bags) {
  if (n_bags <= 0) return 1;
  const int64_t n = (n_bags + 7) / 8;
  return (int32_t)(n < 1024 ? n : 1024);
}

extern "C" int tt_history_self_attention_pool_bwd_f32(const float* table, int64_t table_rows, int32_t dim, int32_t L, int32_t heads,
                                                      const int64_t* batch_ids, const float* weights, const float* pooled,
                                                      const float* dpooled, const float* t, int64_t n_bags, float* slot_grads,
                                                      float* dt, float* dp_slabs, int32_t n_slabs, tt_stream_t stream) {
  const char* what = "tt_history_self_attention_pool_bwd_f32";
  if (int rc = check_shape(what, dim, L, n_bags)) return rc;
  if (int rc = check_heads(what, heads)) return rc;
  TT_REQUIRE(table_rows > 0, "%s: need table_rows > 0", what);
  TT_REQUIRE(n_slabs >= 1 && n_slabs <= 65536, "%s: n_slabs must be in 1..65536 (got %d)", what, n_slabs);
  if (n_bags == 0) return TT_OK;
  TT_REQUIRE(table && batch_ids && weights && pooled && dpooled && t && slot_grads && dt && dp_slabs,
             "%s: null pointer (table / batch_ids / weights / pooled / dpooled / t / slot_grads / dt / dp_slabs)", what);
  TT_REQUIRE(tt::aligned16(table) && tt::aligned16(pooled) && tt::aligned16(dpooled) && tt::aligned16(t) && tt::aligned16(slot_grads) &&
                 tt::aligned16(dt),
             "%s: table / pooled / dpooled / t / slot_grads / dt must be 16-byte aligned", what);
  const int dim4 = dim / 4;
  const int lg = lane_group_log2(dim4);
  // the workgroup: 256 threads, halved while its groups' LDS lines (heads * L floats each) exceed 48 KiB (dim 32 at 8 heads, L 64)
  int threads = 256;
  while (threads > 64 && (size_t)(threads >> lg) * heads * L * sizeof(float) > 48 * 1024) threads >>= 1;
  const unsigned lds = (unsigned)((size_t)(threads >> lg) * heads * L * sizeof(float));
  const int64_t per = (n_bags + n_slabs - 1) / n_slabs;
  const dim3 grid((unsigned)n_slabs), block((unsigned)threads);
  const float scale = 1.0f / sqrtf((float)dim);
  hipStream_t s = tt::as_stream(stream);
#define TT_SA_BWD(H, KF)                                                                                                       \
  tt::launch("history_selfattn_pool_bwd", sa_pool_bwd_kernel<H, KF>, grid, block, lds, s, table, table_rows, dim4, lg, (int)L, \
             batch_ids, weights, pooled, dpooled, t, n_bags, scale, slot_grads, dt, dp_slabs, per)
  switch (heads) {
    case 1: TT_SA_BWD(1, kInFlight); break;
    case 2: TT_SA_BWD(2, kInFlight); break;
    case 4: TT_SA_BWD(4, 2); break;
    default: TT_SA_BWD(8, 2); break;
  }
#undef TT_SA_BWD
  return tt::check_launch(what);
}

extern "C" int tt_history_self_attention_query_grad_f32(const int32_t* newest, const float* dxn, int64_t n_bags, int32_t L, int32_t dim,
                                                        float* slot_grads, tt_stream_t stream) {
  const char* what = "tt_history_self_attention_query_grad_f32";
  if (int rc = check_shape(what, dim, L, n_bags)) return rc;
  if (n_bags == 0) return TT_OK;
  TT_REQUIRE(newest && dxn && slot_grads, "%s: null pointer (newest / dxn / slot_grads)", what);
  TT_REQUIRE(tt::aligned16(dxn) && tt::aligned16(slot_grads), "%s: dxn and slot_grads must be 16-byte aligned", what);
  const int dim4 = dim / 4;
  const int64_t blocks = (n_bags * dim4 + 255) / 256;
  tt::launch("history_selfattn_query_grad", sa_query_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, tt::as_stream(stream), newest,
             dxn, n_bags, (int)L, dim4, slot_grads);
  return tt::check_launch(what);
}
