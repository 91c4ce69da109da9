// The run / piece scheme of the sparse optimizers (csrc/sparse.hip, adam.hip, rowwise.hip): the ONE statement of the order in
// which duplicate gradient rows are summed.  oracle.two_tower.dedup_sum restates it; every bit-exactness test depends on it.
//
// A run of equal ids occupies consecutive slots of the sorted id list.  It is cut into PIECES at global multiples of kPiece
// slots; every piece is summed sequentially in slot (= ascending batch position) order, then the pieces are added in index
// order: P[jh] (the head piece, in block jh) + S[jh + 1] + ... + S[jl] (the pieces that start on a boundary).  A run inside one
// block - the common case - is a plain sequential sum, bit-equal to np.add.at.  Out-of-range ids (negative padding, the plan's
// sentinel id == rows) are skipped: they write no piece and no row.
// A kernel calls piece_head, requests its gradient / table / state rows, and only then calls piece_extent, so that the rows
// are in flight during the extent search; one helper doing both would push the row loads behind the search.
#pragma once
#include "common.h"

namespace tt {

constexpr int kPiece = 64;   // sorted slots per piece (oracle.two_tower.PIECE)

struct PieceHead {
  int64_t id, id_right;      // the slot's id and its right neighbour's
  int32_t ord0;              // the slot's batch position
  bool run_head;             // the slot starts a run (else it starts a piece on a block boundary)
};
struct PieceExtent {
  int64_t e, pend, blk;      // the piece is [k, e); its block ends at pend (clamped to n_ids); blk = k / kPiece
  bool continues, whole;     // the run goes on past e; the piece is the whole run
};

// One round trip for everything slot k's position gives: its id, both neighbours, its batch position.  False: the slot has
// nothing to do (inside a piece, or a skipped id).  k < n_ids.
__device__ __forceinline__ bool piece_head(const int64_t* __restrict__ sid, const int32_t* __restrict__ order, const int64_t k,
                                           const int64_t n_ids, const int64_t rows, PieceHead& h) {
  h.id = sid[k];
  const int64_t id_left = sid[k > 0 ? k - 1 : 0];
  h.id_right = sid[k + 1 < n_ids ? k + 1 : n_ids - 1];
  h.ord0 = order[k];
  h.run_head = (k == 0) || (id_left != h.id);
  if (!h.run_head && (k % kPiece) != 0) return false;
  return h.id >= 0 && h.id < rows;
}

// The end of the piece: known from the right neighbour for the usual run of length 1, else a binary search (sorted ids):
// <= 6 dependent loads per piece.
__device__ __forceinline__ PieceExtent piece_extent(const int64_t* __restrict__ sid, const int64_t k, const int64_t n_ids,
                                                    const PieceHead& h) {
  PieceExtent x;
  x.blk = k / kPiece;
  x.pend = (x.blk + 1) * kPiece;
  if (x.pend > n_ids) x.pend = n_ids;
  x.e = k + 1;
  if (x.e < x.pend && h.id_right == h.id) {
    int64_t lo = x.e + 1, hi = x.pend;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (sid[mid] == h.id) lo = mid + 1; else hi = mid;
    }
    x.e = lo;
  }
  x.continues = (x.e == x.pend) && (x.pend < n_ids) && (sid[x.pend] == h.id);
  x.whole = h.run_head && !x.continues;
  return x;
}

// First slot of id's run, given sid[k] == id (lower bound in [0, k]).
__device__ __forceinline__ int64_t run_begin(const int64_t* __restrict__ sid, const int64_t k, const int64_t id) {
  int64_t lo = 0, hi = k;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sid[mid] < id) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// One past the last slot of id's run, given that every slot before lo holds id or less (sentinel / valid ids ascend,
// nothing sorts below 0).
__device__ __forceinline__ int64_t run_end(const int64_t* __restrict__ sid, int64_t lo, const int64_t n_ids, const int64_t id) {
  int64_t hi = n_ids;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sid[mid] <= id) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The finish launch's view: does a run with a valid id cross the end of block jh, with its head IN block jh?  Then id is the
// run's id and jl (> jh) the block of its last piece.
__device__ __forceinline__ bool crossing_run(const int64_t* __restrict__ sid, const int64_t jh, const int64_t n_ids, const int64_t rows,
                                             int64_t& id, int64_t& jl) {
  const int64_t nxt = (jh + 1) * kPiece;                        // first slot of the next block
  if (nxt >= n_ids) return false;                               // nothing lies past the last block
  id = sid[nxt - 1];
  const int64_t id_next = sid[nxt];
  const int64_t id_before = sid[jh > 0 ? jh * kPiece - 1 : 0];
  if (id_next != id) return false;                              // no run crosses this block's end
  if (id < 0 || id >= rows) return false;                       // skipped ids wrote no pieces
  if (jh > 0 && id_before == id) return false;                  // the run's head lies in an earlier block, which finishes it
  jl = (run_end(sid, nxt + 1, n_ids, id) - 1) / kPiece;
  return true;
}

// g[i] += the gradient rows of slots [j, e), chunk cc[i] of each, in slot order; U rows' loads in flight (the adds stay in
// slot order, the loads do not depend on them).
template <int CPL, int U>
__device__ __forceinline__ void piece_walk(const f32x4* __restrict__ grads, const int32_t* __restrict__ order, const int dim4,
                                           const int* cc, int64_t j, const int64_t e, f32x4* g) {
  while (j + U - 1 < e) {
    f32x4 r[U][CPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t base = (int64_t)order[j + u] * dim4;
#pragma unroll
      for (int i = 0; i < CPL; ++i) r[u][i] = grads[base + cc[i]];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) g[i][q] = __fadd_rn(g[i][q], r[u][i][q]);
    j += U;
  }
  for (; j < e; ++j) {
    const int64_t base = (int64_t)order[j] * dim4;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const f32x4 g1 = grads[base + cc[i]];
#pragma unroll
      for (int q = 0; q < 4; ++q) g[i][q] = __fadd_rn(g[i][q], g1[q]);
    }
  }
}

struct PlainLoad {
  __device__ __forceinline__ f32x4 operator()(const f32x4* p) const { return *p; }
};

// g[i] = P[jh] + S[jh + 1] + ... + S[jl], chunk cc[i] of each, in index order (never arrival order); U piece sums in flight.
template <int CPL, int U, class Load = PlainLoad>
__device__ __forceinline__ void add_pieces(const f32x4* P, const f32x4* S, const int dim4, const int* cc, const int64_t jh,
                                           const int64_t jl, f32x4* g, const Load load = Load{}) {
#pragma unroll
  for (int i = 0; i < CPL; ++i) g[i] = load(P + jh * dim4 + cc[i]);
  int64_t b = jh + 1;
  if constexpr (U > 1) while (b + U - 1 <= jl) {      // (U == 1: the loop below is the whole add)
    f32x4 s[U][CPL];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < CPL; ++i) s[u][i] = load(S + (b + u) * dim4 + cc[i]);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) g[i][q] = __fadd_rn(g[i][q], s[u][i][q]);
    b += U;
  }
  for (; b <= jl; ++b) {
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const f32x4 s = load(S + b * dim4 + cc[i]);
#pragma unroll
      for (int q = 0; q < 4; ++q) g[i][q] = __fadd_rn(g[i][q], s[q]);
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
inline int64_t piece_blocks(int64_t n_ids) { return (n_ids + kPiece - 1) / kPiece; }
inline int64_t piece_array_bytes(int64_t n_ids, int32_t dim) { return (piece_blocks(n_ids) * dim * 4 + 255) / 256 * 256; }   // p_sum or s_sum

// min(dim / 4 rounded up to a power of two, 2^max_log2) lanes per row
inline int lanes_per_row_log2(int dim4, int max_log2) {
  int l = 0;
  while ((1 << l) < dim4 && l < max_log2) ++l;
  return l;
}

// The second launch of a two-launch optimizer: one lane group per 64-slot block beside the dense segments' workgroups.
struct FinishGrid {
  int64_t finish_blocks, dense_blocks, gx;
};
inline FinishGrid finish_grid(bool sparse, int64_t n_ids, int groups, int64_t max_count, int n_segs) {
  FinishGrid f{};
  if (sparse) f.finish_blocks = (piece_blocks(n_ids) + groups - 1) / groups;
  f.dense_blocks = (max_count / 4 + 255) / 256;
  if (f.dense_blocks < 1) f.dense_blocks = 1;
  if (f.dense_blocks > 512) f.dense_blocks = 512;
  if (n_segs == 0) f.dense_blocks = 0;
  f.gx = f.finish_blocks > f.dense_blocks ? f.finish_blocks : f.dense_blocks;
  return f;
}

// What a dense segment (tt_dense_seg, tt_adam_seg) must satisfy; has_state / state_what: the optimizer's own state arrays.
// max_count: the longest segment so far.
template <class Seg>
inline int check_dense_seg(const char* who, int i, const Seg& s, bool has_state, const char* state_what, int64_t& max_count) {
  TT_REQUIRE(s.count > 0 && s.n_slabs >= 1 && s.grad_slabs != nullptr && s.param != nullptr, "%s: segment %d: bad count/slabs/param", who, i);
  TT_REQUIRE(has_state, "%s: segment %d: %s", who, i, state_what);
  TT_REQUIRE(s.n_slabs == 1 || s.slab_stride >= s.count, "%s: segment %d: slab_stride must be >= count", who, i);
  if (s.count > max_count) max_count = s.count;
  return TT_OK;
}

// A table's piece workspace of the two-launch optimizers: p_sum, then s_sum (2 * piece_array_bytes).
inline int split_piece_ws(const char* who, int t, void* ws, int64_t n_ids, int32_t dim, float*& p_sum, float*& s_sum) {
  TT_REQUIRE(ws != nullptr && (reinterpret_cast<uintptr_t>(ws) & 255u) == 0, "%s: table %d: workspace must be non-null, 256-byte aligned", who, t);
  p_sum = static_cast<float*>(ws);
  s_sum = reinterpret_cast<float*>(static_cast<char*>(ws) + piece_array_bytes(n_ids, dim));
  return TT_OK;
}

}  // namespace tt
