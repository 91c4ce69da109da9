// Row-wise ("exact row-wise") Adagrad on embedding rows - FBGEMM / TorchRec's default for embedding tables, with this project's
// Keras epsilon placement - and the existing element-wise Adagrad on the dense tower parameters.
//
// ONE accumulator float per table row, fed with the mean of the row's squared gradient.  Only the rows of this batch's ids are
// touched (their accumulator included); duplicates are summed first, in the run / piece order of csrc/sparse_runs.h, so g is
// bit-identical to what SGD, Adagrad and lazy Adam see.  Every operation rounded once:
//   q_j = g_j * g_j      S = sum_j q_j (fixed order, below)      a' = a + S * inv_dim      w' = w - (lr * g) / sqrt(a' + eps)
// Order of S (a function of dim alone, the same in both launches): a lane group of lpr = min(32, dim/4 rounded up to a power of
// two) lanes owns the row; lane l holds the float4 chunks c = l, l + lpr, ...; it adds its q values one after the other (chunks
// ascending, elements ascending, starting AT the first; a lane without a chunk holds +0); then a butterfly
// p_l = p_l + p_{l xor off}, off = 1, 2, 4, ... < lpr, after which every lane of the group holds the same bits.
//
// TWO stream-ordered launches shaped like csrc/adam.hip's, no communication inside either (no tickets, no wait, no atomics):
//   A  rowwise_sparse_kernel   one lane group per sorted slot; only piece heads work.  A run inside its 64-slot block is summed,
//                              reduced to S and applied on the spot (gradient row, table row and the accumulator scalar are
//                              requested together).  A piece of a run that crosses a block boundary stores its sum (P / S of
//                              its block) with plain stores.
//   B  rowwise_finish_kernel   one lane group per 64-slot block finishes the run that crosses its end: the pieces added, then
//                              the same reduction and update (rowwise_update, shared with A).  The dense segments ride as
//                              extra workgroups (blockIdx.y >= n_tables) in the dense Adagrad body.
// A lane keeps its CPL = ceil(dim / (4 lpr)) chunks of g and w in registers (the kernels are instantiated for CPL 1, 2, 4:
// dim <= 512); nothing spills.  The butterfly sits behind the chunk loops, and a lane group leaves or stays as a whole, so a
// cross-lane read never leaves the active lanes.
// HBM-bound.  Algorithmic bytes per distinct row: 4*dim (grad) + 8*dim (w read + write) + 8 (accumulator) + 12 (sorted id +
// position) = 12*dim + 20; Adagrad moves 20*dim + 12.
#include "common.h"
#include "dense_update_body.h"
#include "sparse_runs.h"
#include <cmath>

namespace {

using tt::f32x4;

constexpr int kMaxRowwiseTables = 3;    // user, item, hashed category
constexpr int kMaxChunksPerLane = 4;    // 32 lanes x 4 float4 chunks: dim <= 512

struct RowTab {
  float* table; float* accum;
  const float* grads;
  const int64_t* sorted_ids;
  const int32_t* order;
  int64_t rows;
  float* p_sum;       // [nblk][dim]  first piece of a run that continues past its block (head in block j)
  float* s_sum;       // [nblk][dim]  piece starting exactly at slot 64*j
};
struct RowArgs {      // (an array of structs: a workgroup picks its table with ONE dynamic offset into the kernel arguments)
  RowTab tab[kMaxRowwiseTables];
};
struct RowCoef {
  float lr, eps, inv_dim;
};

// The reduction and the update of one row, shared by both launches.  Every lane of the row's group calls it together (g: the
// row's summed gradient, w: its parameters, acc: its accumulator, the lane's chunks c = l + i * lpr < dim4 only).
template <int CPL>
__device__ __forceinline__ void rowwise_update(f32x4* __restrict__ table, float* __restrict__ accum, const int64_t id, const int dim4,
                                               const int l, const int lpr, const f32x4 (&g)[CPL], f32x4 (&w)[CPL], const float acc,
                                               const RowCoef h) {
  float p = 0.f;
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    if (l + i * lpr < dim4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float q = __fmul_rn(g[i][e], g[i][e]);
        p = (i == 0 && e == 0) ? q : __fadd_rn(p, q);       // the lane's sum STARTS at its first value
      }
    }
  }
  for (int off = 1; off < lpr; off <<= 1) p = __fadd_rn(p, __shfl_xor(p, off, lpr));   // behind the chunk loop: all lanes of the group
  const float a2 = __fadd_rn(acc, __fmul_rn(p, h.inv_dim));
  if (l == 0) accum[id] = a2;
  const float den = sqrtf(__fadd_rn(a2, h.eps));
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int c = l + i * lpr;
    if (c < dim4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) w[i][e] = __fsub_rn(w[i][e], __fdiv_rn(__fmul_rn(h.lr, g[i][e]), den));
      table[id * dim4 + c] = w[i];
    }
  }
}

// ---- launch A: every piece is summed; whole runs are reduced and updated at once ------------------------------------------
template <int CPL>
__global__ __launch_bounds__(256) void rowwise_sparse_kernel(RowArgs a, int dim4, int lpr_log2, int64_t n_ids, RowCoef h) {
  const int t = blockIdx.y;
  f32x4* __restrict__ table = reinterpret_cast<f32x4*>(a.tab[t].table);
  float* __restrict__ accum = a.tab[t].accum;
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
  const int64_t id = hd.id;
  // ... then ONE more round trip for the gradient row together with the table row and the accumulator (a piece that is not a
  // whole run - rare - does not use the two: its id is valid, so the loads are in bounds).  A chunk past the row re-reads the last.
  int cc[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) cc[i] = l + i * lpr < dim4 ? l + i * lpr : dim4 - 1;
  const int64_t row = id * dim4;
  f32x4 g[CPL], w[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) g[i] = grads[(int64_t)hd.ord0 * dim4 + cc[i]];
#pragma unroll
  for (int i = 0; i < CPL; ++i) w[i] = table[row + cc[i]];
  const float acc = accum[id];
  const tt::PieceExtent x = tt::piece_extent(sid, k, n_ids, hd);   // (behind the row requests: they fly during the search)
  tt::piece_walk<CPL, (CPL <= 2 ? 4 : 2)>(grads, order, dim4, cc, k + 1, x.e, g);
  if (x.whole) {                                  // (the same for every lane of the group) whole run summed: fused update
    rowwise_update<CPL>(table, accum, id, dim4, l, lpr, g, w, acc, h);
  } else {                                        // plain stores: launch B reads them behind the launch boundary
    f32x4* __restrict__ piece_out = reinterpret_cast<f32x4*>(hd.run_head ? a.tab[t].p_sum : a.tab[t].s_sum) + x.blk * dim4;
#pragma unroll
    for (int i = 0; i < CPL; ++i)
      if (l + i * lpr < dim4) piece_out[l + i * lpr] = g[i];
  }
}

// ---- launch B, sparse half: the runs that cross a 64-slot boundary --------------------------------------------------------
template <int CPL>
__device__ __forceinline__ void rowwise_finish_body(const RowArgs& a, const int t, const int64_t bx, int dim4, int lpr_log2,
                                                    int64_t n_ids, const RowCoef h) {
  f32x4* __restrict__ table = reinterpret_cast<f32x4*>(a.tab[t].table);
  float* __restrict__ accum = a.tab[t].accum;
  const int64_t* __restrict__ sid = a.tab[t].sorted_ids;
  const f32x4* __restrict__ P = reinterpret_cast<const f32x4*>(a.tab[t].p_sum);
  const f32x4* __restrict__ S = reinterpret_cast<const f32x4*>(a.tab[t].s_sum);
  const int lpr = 1 << lpr_log2;
  const int groups = 256 >> lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int64_t jh = bx * groups + (threadIdx.x >> lpr_log2);   // 64-slot block
  int64_t id, jl;                                               // the run that crosses this block's end, its last piece's block
  if (!tt::crossing_run(sid, jh, n_ids, a.tab[t].rows, id, jl)) return;
  int cc[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) cc[i] = l + i * lpr < dim4 ? l + i * lpr : dim4 - 1;
  f32x4 g[CPL], w[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) w[i] = table[id * dim4 + cc[i]];
  const float acc = accum[id];
  tt::add_pieces<CPL, (CPL <= 2 ? 4 : 1)>(P, S, dim4, cc, jh, jl, g);   // (4 chunks per lane: the registers go to g and w)
  rowwise_update<CPL>(table, accum, id, dim4, l, lpr, g, w, acc, h);
}

// blockIdx.y < n_tables: the boundary-crossing runs of table y; else dense segment y - n_tables (element-wise Adagrad)
template <int CPL>
__global__ __launch_bounds__(256) void rowwise_finish_kernel(RowArgs a, int n_tables, int dim4, int lpr_log2, int64_t n_ids,
                                                             int64_t sparse_blocks, tt::SegTable tbl, int dense_blocks, RowCoef h) {
  if ((int)blockIdx.y < n_tables) {
    if ((int64_t)blockIdx.x < sparse_blocks) rowwise_finish_body<CPL>(a, blockIdx.y, blockIdx.x, dim4, lpr_log2, n_ids, h);
  } else if ((int)blockIdx.x < dense_blocks) {
    tt::dense_update_body<TT_OPT_ADAGRAD, 256, 8>(tbl.seg[blockIdx.y - n_tables], blockIdx.x, dense_blocks, 1, h.lr, h.eps);
  }
}

template <int CPL>
int launch_rowwise(const char* who, const RowArgs& a, int nt, bool sparse, int dim4, int lpr_log2, int64_t n_ids, const tt::SegTable& tbl,
                   int n_segs, int64_t max_count, RowCoef h, hipStream_t stream) {
  const int groups = 256 >> lpr_log2;
  if (sparse) {
    const int64_t blocks = (n_ids + groups - 1) / groups;
    TT_REQUIRE(blocks <= 0x7fffffff, "%s: n_ids too large", who);
    tt::launch("rowwise_sparse", rowwise_sparse_kernel<CPL>, dim3((unsigned)blocks, (unsigned)nt), dim3(256), 0, stream, a, dim4, lpr_log2,
               n_ids, h);
    const int rc = tt::check_launch(who);
    if (rc != TT_OK) return rc;
  }
  const tt::FinishGrid f = tt::finish_grid(sparse, n_ids, groups, max_count, n_segs);
  tt::launch("rowwise_finish", rowwise_finish_kernel<CPL>, dim3((unsigned)f.gx, (unsigned)(nt + n_segs)), dim3(256), 0, stream, a, nt, dim4,
             lpr_log2, n_ids, f.finish_blocks, tbl, (int)f.dense_blocks, h);
  return tt::check_launch(who);
}

}  // namespace

extern "C" int64_t tt_rowwise_adagrad_workspace_bytes(int64_t n_ids, int32_t dim) {
  if (n_ids <= 0 || dim <= 0) return 0;
  return 2 * tt::piece_array_bytes(n_ids, dim);
}

extern "C" int tt_rowwise_adagrad_step_f32(const tt_rowwise_table* tables, int32_t n_tables, int32_t dim, int64_t n_ids,
                                           const tt_dense_seg* segs, int32_t n_segs, float lr, float eps, tt_stream_t stream_) {
  const char* const who = "tt_rowwise_adagrad_step_f32";
  TT_REQUIRE(n_tables >= 0 && n_tables <= kMaxRowwiseTables, "%s: n_tables must be in 0..%d", who, kMaxRowwiseTables);
  TT_REQUIRE(n_segs >= 0 && n_segs <= TT_MAX_DENSE_SEGS, "%s: n_segs must be in 0..%d", who, TT_MAX_DENSE_SEGS);
  TT_REQUIRE((n_tables == 0 || tables != nullptr) && (n_segs == 0 || segs != nullptr), "%s: null pointer", who);
  TT_REQUIRE(n_ids >= 0, "%s: n_ids must be >= 0", who);
  TT_REQUIRE(n_tables == 0 || (dim > 0 && dim % 4 == 0), "%s: dim must be a positive multiple of 4", who);
  TT_REQUIRE(eps > 0.f, "%s: eps must be > 0", who);
  TT_REQUIRE(std::isfinite(lr), "%s: lr must be finite", who);
  const bool sparse = n_tables > 0 && n_ids > 0;
  RowArgs a{};
  for (int t = 0; t < n_tables; ++t) {
    const tt_rowwise_table& s = tables[t];
    TT_REQUIRE(s.rows > 0, "%s: table %d: rows must be positive", who, t);
    TT_REQUIRE(s.table != nullptr && s.row_accum != nullptr, "%s: table %d: null pointer (table, row_accum)", who, t);
    TT_REQUIRE(!sparse || (s.grads && s.sorted_ids && s.order), "%s: table %d: null pointer", who, t);
    TT_REQUIRE(tt::aligned16(s.table) && tt::aligned16(s.grads), "%s: table %d: table and grads must be 16-byte aligned", who, t);
    TT_REQUIRE((reinterpret_cast<uintptr_t>(s.row_accum) & 3u) == 0, "%s: table %d: row_accum must be 4-byte aligned", who, t);
    if (sparse) {
      const int rc = tt::split_piece_ws(who, t, s.workspace, n_ids, dim, a.tab[t].p_sum, a.tab[t].s_sum);
      if (rc != TT_OK) return rc;
    }
    a.tab[t].table = s.table; a.tab[t].accum = s.row_accum; a.tab[t].grads = s.grads; a.tab[t].sorted_ids = s.sorted_ids;
    a.tab[t].order = s.order;
    a.tab[t].rows = s.rows;
  }
  tt::SegTable tbl{};
  int64_t max_count = 0;
  for (int i = 0; i < n_segs; ++i) {
    const int rc = tt::check_dense_seg(who, i, segs[i], segs[i].accum != nullptr, "Adagrad needs accum", max_count);
    if (rc != TT_OK) return rc;
    tbl.seg[i] = segs[i];
  }
  if (!sparse && n_segs == 0) return TT_OK;

  const int dim4 = sparse ? dim / 4 : 1;
  const int lpr_log2 = tt::lanes_per_row_log2(dim4, 5);           // min(32, dim / 4 rounded up to a power of two) lanes per row
  const int cpl = (dim4 + (1 << lpr_log2) - 1) >> lpr_log2;       // float4 chunks per lane
  if (cpl > kMaxChunksPerLane)
    return tt::fail(TT_ERR_UNSUPPORTED, "%s: dim %d: rows of more than %d floats are not built", who, dim, 128 * kMaxChunksPerLane);
  RowCoef h;
  h.lr = lr;
  h.eps = eps;
  h.inv_dim = sparse ? 1.0f / (float)dim : 1.0f;                  // formed once, here
  hipStream_t stream = tt::as_stream(stream_);
  const int nt = sparse ? n_tables : 0;
  if (cpl == 1) return launch_rowwise<1>(who, a, nt, sparse, dim4, lpr_log2, n_ids, tbl, n_segs, max_count, h, stream);
  if (cpl == 2) return launch_rowwise<2>(who, a, nt, sparse, dim4, lpr_log2, n_ids, tbl, n_segs, max_count, h, stream);
  return launch_rowwise<4>(who, a, nt, sparse, dim4, lpr_log2, n_ids, tbl, n_segs, max_count, h, stream);
}
