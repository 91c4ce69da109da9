// Lazy Adam (TF-Addons LazyAdam / torch.optim.SparseAdam) on embedding rows and on the dense tower parameters.
//
// Only the rows of this batch's ids are touched; duplicates are summed first, in the run / piece order of csrc/sparse_runs.h,
// so g is bit-identical to what SGD and Adagrad see.  Per element, every operation rounded once, no contraction:
//   m' = m + (g - m) * omb1          v' = v + (g*g - v) * omb2          w' = w - (alpha_t * m') / (sqrt(v') + eps)
// with omb1 = 1 - beta1, omb2 = 1 - beta2, alpha_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) computed on the host in f64 and
// rounded once to f32.
//
// TWO stream-ordered launches, no communication inside a launch (no arrival tickets, no in-kernel wait between workgroups):
//   A  adam_sparse_kernel   one lane group per sorted slot; only piece heads work.  A run inside its 64-slot block - the
//                           common case - is summed and updated on the spot (g, w, m, v rows requested together).  A piece of
//                           a run that crosses a block boundary stores its sum (P / S of its block) with plain stores.
//   B  adam_finish_kernel   one lane group per 64-slot block: if a run crosses the block's end with its head in the block, it
//                           adds the run's pieces and applies the update.  The dense segments ride in this launch as extra
//                           workgroups (blockIdx.y >= n_tables).
// B reads only what A wrote in the same call (the launch boundary is the synchronisation), so the workspace needs no
// initialisation.
// HBM-bound.  Algorithmic bytes per distinct row: 4*dim (grad) + 3 * 8*dim (w, m, v read + write) = 28*dim, + 12 (sorted id +
// position); Adagrad moves 20*dim + 12.
#include "common.h"
#include "sparse_runs.h"
#include <cmath>

namespace {

using tt::f32x4;

constexpr int kMaxAdamTables = 3;     // user, item, hashed category

struct AdamTab {
  float* table; float* m; float* v;
  const float* grads;
  const int64_t* sorted_ids;
  const int32_t* order;
  int64_t rows;
  float* p_sum;       // [nblk][dim]  first piece of a run that continues past its block (head in block j)
  float* s_sum;       // [nblk][dim]  piece starting exactly at slot 64*j
};
struct AdamArgs {     // (an array of structs: a workgroup picks its table with ONE dynamic offset into the kernel arguments)
  AdamTab tab[kMaxAdamTables];
};
struct AdamSegTable {
  tt_adam_seg seg[TT_MAX_DENSE_SEGS];
};
struct AdamCoef {
  float omb1, omb2, alpha, eps;
};

__device__ __forceinline__ void adam_one(float& w, float& m, float& v, const float g, const AdamCoef h) {
  m = __fadd_rn(m, __fmul_rn(__fsub_rn(g, m), h.omb1));
  v = __fadd_rn(v, __fmul_rn(__fsub_rn(__fmul_rn(g, g), v), h.omb2));
  w = __fsub_rn(w, __fdiv_rn(__fmul_rn(h.alpha, m), __fadd_rn(sqrtf(v), h.eps)));
}

__device__ __forceinline__ void adam_store(f32x4* __restrict__ table, f32x4* __restrict__ mom, f32x4* __restrict__ var, int64_t off,
                                           f32x4 w, f32x4 m, f32x4 v, const f32x4& g, const AdamCoef h) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float we = w[e], me = m[e], ve = v[e];
    adam_one(we, me, ve, g[e], h);
    w[e] = we; m[e] = me; v[e] = ve;
  }
  mom[off] = m;
  var[off] = v;
  table[off] = w;
}

// ---- launch A: every piece is summed; whole runs are updated at once ------------------------------------------------------
__global__ __launch_bounds__(256) void adam_sparse_kernel(AdamArgs a, int dim4, int lpr_log2, int64_t n_ids, AdamCoef h) {
  const int t = blockIdx.y;
  f32x4* __restrict__ table = reinterpret_cast<f32x4*>(a.tab[t].table);
  f32x4* __restrict__ mom = reinterpret_cast<f32x4*>(a.tab[t].m);
  f32x4* __restrict__ var = reinterpret_cast<f32x4*>(a.tab[t].v);
  const f32x4* __restrict__ grads = reinterpret_cast<const f32x4*>(a.tab[t].grads);
  const int64_t* __restrict__ sid = a.tab[t].sorted_ids;
  const int32_t* __restrict__ order = a.tab[t].order;
  const int64_t rows = a.tab[t].rows;

  const int lpr = 1 << lpr_log2;
  const int groups = 256 >> lpr_log2;
  const int64_t k = (int64_t)blockIdx.x * groups + (threadIdx.x >> lpr_log2);   // sorted slot
  const int l = threadIdx.x & (lpr - 1);
  if (k >= n_ids) return;
  tt::PieceHead hd;
  if (!tt::piece_head(sid, order, k, n_ids, rows, hd)) return;   // inside a piece, or an out-of-range / padding id
  // ... then ONE more round trip for the gradient row together with the table row and both moment rows (a piece that is not
  // a whole run - rare - does not use the three: its id is valid, so the loads are in bounds)
  const int lc = l < dim4 ? l : dim4 - 1;
  const int64_t row = hd.id * dim4;
  const f32x4 g_first = grads[(int64_t)hd.ord0 * dim4 + lc];
  const f32x4 w_first = table[row + lc];
  const f32x4 m_first = mom[row + lc];
  const f32x4 v_first = var[row + lc];
  const tt::PieceExtent x = tt::piece_extent(sid, k, n_ids, hd);   // (behind the row requests: they fly during the search)
  f32x4* __restrict__ piece_out = reinterpret_cast<f32x4*>(hd.run_head ? a.tab[t].p_sum : a.tab[t].s_sum) + x.blk * dim4;

  for (int c = l; c < dim4; c += lpr) {
    f32x4 g = c == l ? g_first : grads[(int64_t)hd.ord0 * dim4 + c];
    tt::piece_walk<1, 4>(grads, order, dim4, &c, k + 1, x.e, &g);
    if (x.whole) {                                // whole run summed: fused update
      if (c == l) adam_store(table, mom, var, row + c, w_first, m_first, v_first, g, h);
      else adam_store(table, mom, var, row + c, table[row + c], mom[row + c], var[row + c], g, h);
    } else {
      piece_out[c] = g;                           // plain store: launch B reads it behind the launch boundary
    }
  }
}

// ---- launch B, sparse half: the runs that cross a 64-slot boundary --------------------------------------------------------
__device__ __forceinline__ void adam_finish_body(const AdamArgs& a, const int t, const int64_t bx, int dim4, int lpr_log2,
                                                 int64_t n_ids, const AdamCoef h) {
  f32x4* __restrict__ table = reinterpret_cast<f32x4*>(a.tab[t].table);
  f32x4* __restrict__ mom = reinterpret_cast<f32x4*>(a.tab[t].m);
  f32x4* __restrict__ var = reinterpret_cast<f32x4*>(a.tab[t].v);
  const int64_t* __restrict__ sid = a.tab[t].sorted_ids;
  const f32x4* __restrict__ P = reinterpret_cast<const f32x4*>(a.tab[t].p_sum);
  const f32x4* __restrict__ S = reinterpret_cast<const f32x4*>(a.tab[t].s_sum);
  const int lpr = 1 << lpr_log2;
  const int groups = 256 >> lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int64_t jh = bx * groups + (threadIdx.x >> lpr_log2);   // 64-slot block
  int64_t id, jl;                                               // the run that crosses this block's end, its last piece's block
  if (!tt::crossing_run(sid, jh, n_ids, a.tab[t].rows, id, jl)) return;
  const int64_t row = id * dim4;
  for (int c = l; c < dim4; c += lpr) {
    const f32x4 w = table[row + c], m = mom[row + c], v = var[row + c];
    f32x4 g;
    tt::add_pieces<1, 4>(P, S, dim4, &c, jh, jl, &g);
    adam_store(table, mom, var, row + c, w, m, v, g, h);
  }
}

// ---- launch B, dense half: one thread owns 4 consecutive elements (float4 when the segment allows it); parameter and both
// moments are requested first, U slab loads in flight, the additions in slab order starting AT slab 0 ------------------------
__device__ __forceinline__ bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int U>
__device__ __forceinline__ void adam_dense_body(const tt_adam_seg& s, const int bx, const int nbx, const AdamCoef h) {
  const int64_t stride = (int64_t)nbx * 256;
  const float l2x2 = 2.0f * s.l2;
  const bool vec = (s.count % 4 == 0) && (s.slab_stride % 4 == 0) && al16(s.grad_slabs) && al16(s.param) && al16(s.m) && al16(s.v);
  if (vec) {
    const int64_t n4 = s.count / 4, st4 = s.slab_stride / 4;
    const f32x4* __restrict__ gs = reinterpret_cast<const f32x4*>(s.grad_slabs);
    const int ns = s.n_slabs;
    f32x4* param4 = reinterpret_cast<f32x4*>(s.param);
    f32x4* m4 = reinterpret_cast<f32x4*>(s.m);
    f32x4* v4 = reinterpret_cast<f32x4*>(s.v);
    for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < n4; i += stride) {
      f32x4 w = param4[i], m = m4[i], v = v4[i];
      const f32x4* __restrict__ gp = gs + i;
      f32x4 g = gp[0];                                    // the sum STARTS at slab 0 (0 + x would turn -0 into +0)
      int k = 1;
      if (ns >= U) {                                      // (uniform) slab 0 heads a full group: 32 slabs are four round trips
        f32x4 r[U];
#pragma unroll
        for (int u = 1; u < U; ++u) r[u] = gp[(int64_t)u * st4];
#pragma unroll
        for (int u = 1; u < U; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) g[e] = __fadd_rn(g[e], r[u][e]);
        k = U;
      }
      for (; k + U <= ns; k += U) {                       // U slab loads in flight, added in slab order
        f32x4 r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = gp[(int64_t)(k + u) * st4];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) g[e] = __fadd_rn(g[e], r[u][e]);
      }
      for (; k < ns; ++k) {
        const f32x4 r = gp[(int64_t)k * st4];
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] = __fadd_rn(g[e], r[e]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float we = w[e], me = m[e], ve = v[e];
        adam_one(we, me, ve, __fadd_rn(g[e], __fmul_rn(l2x2, we)), h);
        w[e] = we; m[e] = me; v[e] = ve;
      }
      m4[i] = m;
      v4[i] = v;
      param4[i] = w;
    }
    return;
  }
  for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < s.count; i += stride) {
    float g = s.grad_slabs[i];
    for (int k = 1; k < s.n_slabs; ++k) g = __fadd_rn(g, s.grad_slabs[(int64_t)k * s.slab_stride + i]);
    float w = s.param[i], m = s.m[i], v = s.v[i];
    adam_one(w, m, v, __fadd_rn(g, __fmul_rn(l2x2, w)), h);
    s.m[i] = m;
    s.v[i] = v;
    s.param[i] = w;
  }
}

// blockIdx.y < n_tables: the boundary-crossing runs of table y; else dense segment y - n_tables
__global__ __launch_bounds__(256) void adam_finish_kernel(AdamArgs a, int n_tables, int dim4, int lpr_log2, int64_t n_ids,
                                                          int64_t sparse_blocks, AdamSegTable tbl, int dense_blocks, AdamCoef h) {
  if ((int)blockIdx.y < n_tables) {
    if ((int64_t)blockIdx.x < sparse_blocks) adam_finish_body(a, blockIdx.y, blockIdx.x, dim4, lpr_log2, n_ids, h);
  } else if ((int)blockIdx.x < dense_blocks) {
    adam_dense_body<8>(tbl.seg[blockIdx.y - n_tables], blockIdx.x, dense_blocks, h);
  }
}

}  // namespace

extern "C" int64_t tt_adam_workspace_bytes(int64_t n_ids, int32_t dim) {
  if (n_ids <= 0 || dim <= 0) return 0;
  return 2 * tt::piece_array_bytes(n_ids, dim);
}

extern "C" int tt_adam_step_f32(const tt_adam_table* tables, int32_t n_tables, int32_t dim, int64_t n_ids, const tt_adam_seg* segs,
                                int32_t n_segs, const tt_adam_hyper* hp, tt_stream_t stream_) {
  const char* const who = "tt_adam_step_f32";
  TT_REQUIRE(n_tables >= 0 && n_tables <= kMaxAdamTables, "%s: n_tables must be in 0..%d", who, kMaxAdamTables);
  TT_REQUIRE(n_segs >= 0 && n_segs <= TT_MAX_DENSE_SEGS, "%s: n_segs must be in 0..%d", who, TT_MAX_DENSE_SEGS);
  TT_REQUIRE(hp != nullptr && (n_tables == 0 || tables != nullptr) && (n_segs == 0 || segs != nullptr), "%s: null pointer", who);
  TT_REQUIRE(n_ids >= 0, "%s: n_ids must be >= 0", who);
  TT_REQUIRE(n_tables == 0 || (dim > 0 && dim % 4 == 0), "%s: dim must be a positive multiple of 4", who);
  TT_REQUIRE(hp->step >= 1, "%s: step must be >= 1 (the 1-based global step)", who);
  TT_REQUIRE(hp->beta1 >= 0.f && hp->beta1 < 1.f, "%s: beta1 must be in [0, 1)", who);
  TT_REQUIRE(hp->beta2 >= 0.f && hp->beta2 < 1.f, "%s: beta2 must be in [0, 1)", who);
  TT_REQUIRE(hp->eps > 0.f, "%s: eps must be > 0", who);
  TT_REQUIRE(std::isfinite(hp->lr), "%s: lr must be finite", who);
  const bool sparse = n_tables > 0 && n_ids > 0;
  AdamArgs a{};
  for (int t = 0; t < n_tables; ++t) {
    const tt_adam_table& s = tables[t];
    TT_REQUIRE(s.rows > 0, "%s: table %d: rows must be positive", who, t);
    TT_REQUIRE(s.m != nullptr && s.v != nullptr, "%s: table %d: Adam needs both moment arrays m and v", who, t);
    TT_REQUIRE(s.table != nullptr, "%s: table %d: null pointer", who, t);
    TT_REQUIRE(!sparse || (s.grads && s.sorted_ids && s.order), "%s: table %d: null pointer", who, t);
    TT_REQUIRE(tt::aligned16(s.table) && tt::aligned16(s.m) && tt::aligned16(s.v) && tt::aligned16(s.grads),
               "%s: table %d: table, m, v and grads must be 16-byte aligned", who, t);
    if (sparse) {
      const int rc = tt::split_piece_ws(who, t, s.workspace, n_ids, dim, a.tab[t].p_sum, a.tab[t].s_sum);
      if (rc != TT_OK) return rc;
    }
    a.tab[t].table = s.table; a.tab[t].m = s.m; a.tab[t].v = s.v; a.tab[t].grads = s.grads; a.tab[t].sorted_ids = s.sorted_ids; a.tab[t].order = s.order;
    a.tab[t].rows = s.rows;
  }
  AdamSegTable tbl{};
  int64_t max_count = 0;
  for (int i = 0; i < n_segs; ++i) {
    const int rc = tt::check_dense_seg(who, i, segs[i], segs[i].m != nullptr && segs[i].v != nullptr,
                                       "Adam needs both moment arrays m and v", max_count);
    if (rc != TT_OK) return rc;
    tbl.seg[i] = segs[i];
  }
  if (!sparse && n_segs == 0) return TT_OK;
  // the step's three scalars: f64 on the host, each rounded once to f32
  const double b1 = (double)hp->beta1, b2 = (double)hp->beta2, st = (double)hp->step;
  AdamCoef h;
  h.omb1 = (float)(1.0 - b1);
  h.omb2 = (float)(1.0 - b2);
  h.alpha = (float)((double)hp->lr * std::sqrt(1.0 - std::pow(b2, st)) / (1.0 - std::pow(b1, st)));
  h.eps = hp->eps;

  hipStream_t stream = tt::as_stream(stream_);
  const int dim4 = sparse ? dim / 4 : 1;
  const int lpr_log2 = tt::lanes_per_row_log2(dim4, 5);           // min(dim / 4, 32) lanes per row
  const int groups = 256 >> lpr_log2;
  const int nt = sparse ? n_tables : 0;
  if (sparse) {
    const int64_t blocks = (n_ids + groups - 1) / groups;
    TT_REQUIRE(blocks <= 0x7fffffff, "%s: n_ids too large", who);
    tt::launch("adam_sparse", adam_sparse_kernel, dim3((unsigned)blocks, (unsigned)nt), dim3(256), 0, stream, a, dim4, lpr_log2, n_ids, h);
    const int rc = tt::check_launch(who);
    if (rc != TT_OK) return rc;
  }
  const tt::FinishGrid f = tt::finish_grid(sparse, n_ids, groups, max_count, n_segs);
  tt::launch("adam_finish", adam_finish_kernel, dim3((unsigned)f.gx, (unsigned)(nt + n_segs)), dim3(256), 0, stream, a, nt, dim4, lpr_log2,
             n_ids, f.finish_blocks, tbl, (int)f.dense_blocks, h);
  return tt::check_launch(who);
}
