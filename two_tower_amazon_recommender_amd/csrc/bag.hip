// Embedding bag: a bag of hashed token rows pooled into one vector (TFRS TextVectorization -> Embedding -> GlobalAveragePooling1D;
// the pooled item-title feature summed into the item tower's input), and the one launch its backward pass needs.
// HBM-bound, the regime of K1 (gather.hip): sum(cnt) random 4*dim-byte row reads, one 4*dim-byte row written (and read, when
// accumulating) per bag: 4*dim*(sum(cnt) + 2*n_bags) bytes.  A group of LPR lanes owns a bag (LPR = the power of two >= dim/4,
// at most a wave: 8 lanes at dim 32, 32 at 128, 64 from 256 on, where a lane holds NV = ceil(dim/256) float4 of the row - the
// shape of normalize.hip), so a wave owns 64/LPR bags.  The bag's token slots are read ONCE per group, LPR at a time (lane l
// holds slot base + l; the same lane writes batch_ids), the valid ones are found with a ballot and handed round by shuffle in
// ascending slot order; every lane keeps kInFlight independent row loads outstanding (sparse_apply_body's four).  The sum is a
// fixed sequence of f32 adds in ascending slot order inside one lane: no LDS, no atomics (but the out-of-range flag), and the
// bits of a bag depend on neither the grid nor the other bags.  Lane groups past the last bag load nothing, store nothing and
// still take part in the ballots and shuffles (a group is wholly inside or wholly outside).
// The pooled user-history feature (tt_history_bag_fwd_f32) is the same body under two template flags.  EXCL: the bag skips
// every slot whose token equals exclude[b] (leave-one-out: the pair's own positive must not be pooled into the query it is
// scored against) - one more 8-byte load per bag, issued with bag_rows[b], one compare per slot, and the slot is written to
// batch_ids as -1 like any skipped slot, so the sort plan and the update never see it.  BASE: the row the sum is added to is
// base_table[base_ids[b]] instead of out[b] - the tower input user_table[u] + pool(history rows) in ONE launch, without the
// gather launch's [n_bags, dim] round trip.  <NV, false, false> is the kernel of tt_embedding_bag_fwd_f32 as it was.
#include "common.h"

namespace {

constexpr int kInFlight = 4;
enum { kPoolSum = 0, kPoolMean = 1, kPoolSqrtN = 2 };

template <int NV, bool EXCL, bool BASE>
__global__ __launch_bounds__(256) void bag_fwd_kernel(const float* __restrict__ table_, int64_t table_rows, int dim4, int lpr_log2,
                                                      const int32_t* __restrict__ tokens, int64_t n_token_rows, int L,
                                                      const int64_t* __restrict__ bag_rows, int64_t n_bags, int pooling,
                                                      int accumulate, float* __restrict__ out_, int64_t* __restrict__ batch_ids,
                                                      float* __restrict__ inv_out, int32_t* __restrict__ oob_flag,
                                                      const int64_t* __restrict__ exclude, const float* __restrict__ base_table_,
                                                      int64_t base_rows, const int64_t* __restrict__ base_ids) {
  const tt::f32x4* __restrict__ table = reinterpret_cast<const tt::f32x4*>(table_);
  tt::f32x4* __restrict__ out = reinterpret_cast<tt::f32x4*>(out_);
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
      if (bid < 0 || bid >= base_rows) {                             // (tt_embedding_gather's rule: zero row; -1 sets no flag)
        if (bid != -1 && l == 0 && oob_flag != nullptr) atomicOr(oob_flag, 1);
        bid = -1;
      }
    }
    if (row < 0 || row >= n_token_rows) {
      if (row != -1 && l == 0 && oob_flag != nullptr) atomicOr(oob_flag, 1);
      row = -1;
    }
  }
  // the row the sum is added to: loaded ahead of the gather, used after it
  tt::f32x4 o[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = l + i * lpr;
    o[i] = tt::f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (BASE) {
      if (bid >= 0 && c < dim4) o[i] = reinterpret_cast<const tt::f32x4*>(base_table_)[bid * dim4 + c];
    } else {
      if (live && accumulate && c < dim4) o[i] = out[b * dim4 + c];
    }
  }

  tt::f32x4 s[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) s[i] = tt::f32x4{0.f, 0.f, 0.f, 0.f};
  int cnt = 0;
  for (int base = 0; base < L; base += lpr) {                        // (L is uniform: every lane of the wave reaches the ballot)
    const int slot = base + l;
    int32_t tok = -1;
    if (row >= 0 && slot < L) {
      tok = tokens[row * L + slot];
      if constexpr (EXCL) {                                          // the raw token, compared in int64: skipped like padding
        if ((int64_t)tok == ex) tok = -1;
      }
      if (tok < 0 || (int64_t)tok >= table_rows) {
        if (tok != -1 && oob_flag != nullptr) atomicOr(oob_flag, 1);
        tok = -1;
      }
    }
    if (live && slot < L && batch_ids != nullptr) batch_ids[b * L + slot] = (int64_t)tok;
    uint64_t m = (__ballot(tok >= 0) >> gbase) & gmask;              // valid slots of this group's chunk, bit k = slot base + k
    while (m != 0) {                                                 // (m is uniform inside a group: its lanes stay together)
      // the next (up to) kInFlight valid slots' tokens; a batch shorter than that repeats its first row (a load that hits the
      // cache, never added) and a lane past the row's end its last float4, so that the loads below carry no branch of their own
      // and all leave before the first wait
      int64_t id[kInFlight];
      int nk = 0;
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        const bool has = m != 0;
        const int k = has ? __ffsll((unsigned long long)m) - 1 : 0;
        m &= m - 1;
        const int t = __shfl(tok, gbase + k, 64);
        id[u] = (has || u == 0) ? (int64_t)t : id[0];
        nk += has ? 1 : 0;
      }
      tt::f32x4 r[kInFlight][NV];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u)
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const int c = l + i * lpr;
          r[u][i] = table[id[u] * dim4 + (c < dim4 ? c : dim4 - 1)];   // (a lane past the row's end re-reads its last float4)
        }
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        if (u < nk) {
          if (cnt == 0) {                                            // s starts AT the first valid row (not at +0 + row)
#pragma unroll
            for (int i = 0; i < NV; ++i) s[i] = r[u][i];
          } else {
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
              for (int q = 0; q < 4; ++q) s[i][q] = __fadd_rn(s[i][q], r[u][i][q]);
          }
          ++cnt;
        }
      }
    }
  }
  if (!live) return;

  float inv = 0.0f;                                                  // empty bag: 0
  if (cnt > 0) {
    inv = 1.0f;
    if (pooling == kPoolMean) inv = __fdiv_rn(1.0f, (float)cnt);
    // sqrtf is the correctly rounded square root (as in normalize.hip); __fsqrt_rn compiles to the bare v_sqrt_f32 estimate
    else if (pooling == kPoolSqrtN) inv = __fdiv_rn(1.0f, sqrtf((float)cnt));
  }
  if (l == 0 && inv_out != nullptr) inv_out[b] = inv;
  if (cnt == 0 && accumulate) return;                                // nothing to add: the row is not written
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = l + i * lpr;
    if (c >= dim4) continue;
    tt::f32x4 p = s[i];                                              // cnt == 0 (and not accumulating): +0
    if (pooling != kPoolSum && cnt > 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) p[q] = __fmul_rn(p[q], inv);
    }
    if constexpr (BASE) {
      if (cnt == 0) {                                                // empty bag: the base row itself
        p = o[i];
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) p[q] = __fadd_rn(o[i][q], p[q]);
      }
    } else if (accumulate) {
#pragma unroll
      for (int q = 0; q < 4; ++q) p[q] = __fadd_rn(o[i][q], p[q]);
    }
    out[b * dim4 + c] = p;
  }
}

// gs[b, :] = dy[b, :] * inv[b] (element i of the launch: one float4) and order_bags[j] = order[j] / L (element j): one launch.
__global__ __launch_bounds__(256) void bag_bwd_kernel(const float* __restrict__ dy_, const float* __restrict__ inv, int64_t n_vec,
                                                      int dim4, int L, const int32_t* __restrict__ order, int64_t n_ids,
                                                      float* __restrict__ gs_, int32_t* __restrict__ order_bags) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gs_ != nullptr && i < n_vec) {
    const tt::f32x4 g = reinterpret_cast<const tt::f32x4*>(dy_)[i];
    const float k = inv[i / dim4];
    tt::f32x4 r;
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = __fmul_rn(g[q], k);
    reinterpret_cast<tt::f32x4*>(gs_)[i] = r;
  }
  if (i < n_ids) order_bags[i] = order[i] / L;
}

// The argument checks and the launch of both forward entries (``what`` names the entry in the messages).
int bag_fwd_launch(const char* what, const float* table, int64_t table_rows, int32_t dim, const int32_t* tokens,
                   int64_t n_token_rows, int32_t L, const int64_t* bag_rows, int64_t n_bags, int32_t pooling, int32_t accumulate,
                   float* out, int64_t* batch_ids, float* inv, int32_t* oob_flag, const int64_t* exclude, const float* base_table,
                   int64_t base_rows, const int64_t* base_ids, tt_stream_t stream) {
  TT_REQUIRE(dim >= 4 && dim <= 1024 && dim % 4 == 0, "%s: dim must be a multiple of 4 in 4..1024 (got %d)", what, dim);
  TT_REQUIRE(L >= 1, "%s: L must be >= 1 (got %d)", what, L);
  TT_REQUIRE(pooling >= kPoolSum && pooling <= kPoolSqrtN, "%s: pooling must be 0 (sum), 1 (mean) or 2 (sqrtn) (got %d)", what, pooling);
  TT_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate must be 0 or 1 (got %d)", what, accumulate);
  TT_REQUIRE(table_rows > 0 && n_token_rows >= 0 && n_bags >= 0, "%s: need table_rows > 0, n_token_rows >= 0, n_bags >= 0", what);
  TT_REQUIRE(bag_rows != nullptr || n_bags == n_token_rows,
             "%s: bag_rows is NULL (identity), so n_bags (%lld) must equal n_token_rows (%lld)", what, (long long)n_bags,
             (long long)n_token_rows);
  TT_REQUIRE(n_bags <= 0x7fffffff / (int64_t)L, "%s: n_bags * L must fit 31 bits (the sort plan's positions are int32)", what);
  TT_REQUIRE((base_table != nullptr) == (base_ids != nullptr), "%s: base_table and base_ids go together (both NULL or both given)", what);
  TT_REQUIRE(base_table == nullptr || accumulate == 0, "%s: a base row takes the place of out's: accumulate must be 0 with a base", what);
  TT_REQUIRE(base_table == nullptr || base_rows > 0, "%s: need base_rows > 0 with a base", what);
  if (n_bags == 0) return TT_OK;
  TT_REQUIRE(table && out && (tokens || n_token_rows == 0), "%s: null pointer", what);
  TT_REQUIRE(tt::aligned16(table) && tt::aligned16(out), "%s: table / out must be 16-byte aligned", what);
  TT_REQUIRE(base_table == nullptr || tt::aligned16(base_table), "%s: base_table must be 16-byte aligned", what);
  const int dim4 = dim / 4;
  int lg = 0;
  while ((1 << lg) < dim4 && lg < 6) ++lg;
  const int nv = (dim4 + (1 << lg) - 1) >> lg;                       // 1 up to dim 256, then ceil(dim / 256) <= 4
  const int64_t groups = 256 >> lg;
  const int64_t blocks = (n_bags + groups - 1) / groups;
  TT_REQUIRE(blocks <= 0x7fffffff, "%s: too many bags", what);
  const dim3 grid((unsigned)blocks), block(256);
  hipStream_t s = tt::as_stream(stream);
#define TT_BAG_LAUNCH(NV, EXCL, BASE)                                                                                          \
  tt::launch("bag_fwd", bag_fwd_kernel<NV, EXCL, BASE>, grid, block, 0, s, table, table_rows, dim4, lg, tokens, n_token_rows,   \
             (int)L, bag_rows, n_bags, (int)pooling, (int)accumulate, out, batch_ids, inv, oob_flag, exclude, base_table,       \
             base_rows, base_ids)
#define TT_BAG_LAUNCH_NV(EXCL, BASE)                                                                                           \
  switch (nv) {                                                                                                                \
    case 1: TT_BAG_LAUNCH(1, EXCL, BASE); break;                                                                               \
    case 2: TT_BAG_LAUNCH(2, EXCL, BASE); break;                                                                               \
    case 3: TT_BAG_LAUNCH(3, EXCL, BASE); break;                                                                               \
    default: TT_BAG_LAUNCH(4, EXCL, BASE); break;                                                                              \
  }
  if (exclude != nullptr && base_table != nullptr) {
    TT_BAG_LAUNCH_NV(true, true);
  } else if (exclude != nullptr) {
    TT_BAG_LAUNCH_NV(true, false);
  } else if (base_table != nullptr) {
    TT_BAG_LAUNCH_NV(false, true);
  } else {
    TT_BAG_LAUNCH_NV(false, false);
  }
#undef TT_BAG_LAUNCH_NV
#undef TT_BAG_LAUNCH
  return tt::check_launch(what);
}

}  // namespace

extern "C" int tt_embedding_bag_fwd_f32(const float* table, int64_t table_rows, int32_t dim, const int32_t* tokens,
                                        int64_t n_token_rows, int32_t L, const int64_t* bag_rows, int64_t n_bags, int32_t pooling,
                                        int32_t accumulate, float* out, int64_t* batch_ids, float* inv, int32_t* oob_flag,
                                        tt_stream_t stream) {
  return bag_fwd_launch("tt_embedding_bag_fwd_f32", table, table_rows, dim, tokens, n_token_rows, L, bag_rows, n_bags, pooling,
                        accumulate, out, batch_ids, inv, oob_flag, nullptr, nullptr, 0, nullptr, stream);
}

extern "C" int tt_history_bag_fwd_f32(const float* table, int64_t table_rows, int32_t dim, const int32_t* tokens,
                                      int64_t n_token_rows, int32_t L, const int64_t* bag_rows, int64_t n_bags, int32_t pooling,
                                      int32_t accumulate, float* out, int64_t* batch_ids, float* inv, int32_t* oob_flag,
                                      const int64_t* exclude, const float* base_table, int64_t base_rows, const int64_t* base_ids,
                                      tt_stream_t stream) {
  return bag_fwd_launch("tt_history_bag_fwd_f32", table, table_rows, dim, tokens, n_token_rows, L, bag_rows, n_bags, pooling,
                        accumulate, out, batch_ids, inv, oob_flag, exclude, base_table, base_rows, base_ids, stream);
}

extern "C" int tt_embedding_bag_bwd_f32(const float* dy, const float* inv, int64_t n_bags, int32_t dim, int32_t L,
                                        const int32_t* order, int64_t n_ids, float* gs, int32_t* order_bags, tt_stream_t stream) {
  const char* what = "tt_embedding_bag_bwd_f32";
  TT_REQUIRE(dim >= 4 && dim <= 1024 && dim % 4 == 0, "%s: dim must be a multiple of 4 in 4..1024 (got %d)", what, dim);
  TT_REQUIRE(L >= 1, "%s: L must be >= 1 (got %d)", what, L);
  TT_REQUIRE(n_bags >= 0 && n_bags <= 0x7fffffff / (int64_t)L, "%s: need 0 <= n_bags and n_bags * L within 31 bits", what);
  TT_REQUIRE(n_ids == n_bags * L, "%s: n_ids (%lld) must be n_bags * L (%lld)", what, (long long)n_ids, (long long)(n_bags * L));
  if (n_bags == 0) return TT_OK;
  TT_REQUIRE(order && order_bags, "%s: null pointer (order / order_bags)", what);
  TT_REQUIRE(gs == nullptr || (dy && inv), "%s: gs needs dy and inv", what);
  TT_REQUIRE(gs == nullptr || (tt::aligned16(dy) && tt::aligned16(gs)), "%s: dy / gs must be 16-byte aligned", what);
  const int dim4 = dim / 4;
  const int64_t n_vec = gs != nullptr ? n_bags * dim4 : 0;
  const int64_t n = n_vec > n_ids ? n_vec : n_ids;
  const int64_t blocks = (n + 255) / 256;
  TT_REQUIRE(blocks <= 0x7fffffff, "%s: too many elements", what);
  tt::launch("bag_bwd", bag_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, tt::as_stream(stream), dy, inv, n_vec, dim4, (int)L,
             order, n_ids, gs, order_bags);
  return tt::check_launch(what);
}
