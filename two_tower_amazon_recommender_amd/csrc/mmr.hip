// MMR diversified re-ranking (Carbonell & Goldstein 1998) of the candidate pool an index returns, with an optional cap on
// the items of one group: tt_mmr_rerank_f32 (include/twotower_hip.h states the arithmetic; tests/mmr_check.py restates it).
//
// One launch, no workspace, no atomics, nothing read back: one workgroup per query, thread j owns candidate j of the pool
// (k1 <= TT_TOPK_MAX_K = 256), the workgroup is 64, 128 or 256 threads by k1 (a pool of <= 64 candidates is one wave: the
// compiler drops the s_barrier of a one-wave workgroup).
//   Set-up: thread j checks its candidate, loads its corpus row once with 16-byte loads (summing the row's squared norm on
//   the way) and, on the LDS path, stores it interleaved by groups of four dimensions - rows[d / 4][j] is one 16-byte slot,
//   row stride = the workgroup size - so that the walk of thread j over d is one ds_read_b128 per four dimensions whose 16
//   lanes of a lane group cover 16 consecutive slots = all 64 banks (no conflict), and the picked row rows[d / 4][p] is one
//   broadcast address.  (A fully transposed rows[d][j] image is conflict-free too, but needs four ds_read_b32 where this
//   needs one read; measured 2.65 against 2.58 us per pick at k = 100 of 256, D = 128.)  The pool's min / max score is one wave
//   reduction + one LDS round.
//   Pick t: every thread forms val = lambda rel - (1 - lambda) pen; arg-max (val, then the lower position): inside the wave
//   the maximum by four DPP steps and four readlanes, its lowest lane by a ballot (no LDS traffic: the ds_bpermute butterfly
//   this replaced measured 2.5 us per pick against 2.0 us), then one LDS round across waves
//   (double-buffered by the parity of t: one barrier per pick);
//   thread p writes the output pair; every valid thread then walks d once more: dot(c_j, c_p), cosine, pen = max(pen, sim),
//   and counts the pick against its group.
//   Rows that do not fit (workgroup size x D x 4 > 128 KB: the 256-candidate pool at D = 256) stay in global memory: the
//   picked row is copied to LDS (prow, read back as broadcast ds_read_b128) and thread j re-reads its own row with 16-byte
//   loads from L2.  The arithmetic - four partial sums by d mod 4, products and sums rounded one by one - is the same on both
//   paths, so the answer is too.
// LDS: 16 words of reduction scratch + inv[NT] + group[NT] + row[NT] + prow[D] + rows[D][NT]: 134,720 B at k1 = 256, D = 128 (one
// workgroup per CU), 34.1 KB at k1 <= 64, D = 128 (4 per CU).
#include "common.h"

namespace {

using tt::f32x4;

constexpr int kRowsLdsMax = 128 * 1024;          // rows[D][NT] up to here; beyond it the rows stay in global memory
constexpr int kNone = 0x7fffffff;                // "no eligible candidate" position

struct MmrArgs {
  const float* scores;      // [nq, k1]
  const int64_t* idx;       // [nq, k1]
  const float* c;           // [nc, dim]
  const int32_t* groups;    // [nc] or null
  float* out_s;             // [nq, k]
  int64_t* out_i;           // [nq, k]
  int64_t nc;
  int k1, k, dim, cap;
  float lam;
  int rows_lds;             // 1: rows staged (transposed) in LDS
};

// max(v, v of the lane the DPP control names): quad_perm / row_ror move data inside a row of 16 lanes without the LDS
template <int CTRL>
__device__ __forceinline__ float dpp_max(float v) {
  return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false)));
}

// The wave's largest v (no NaN; every lane active) and the lowest lane that holds it with ok set (-1: none), wave-uniform:
// four DPP steps give every row of 16 its maximum, four readlanes join the rows, a ballot picks the lowest lane.
__device__ __forceinline__ void wave_argmax(float& v, int& lane, bool ok) {
  float m = dpp_max<0xB1>(v);           // quad_perm [1, 0, 3, 2]
  m = dpp_max<0x4E>(m);                 // quad_perm [2, 3, 0, 1]
  m = dpp_max<0x124>(m);                // row_ror 4
  m = dpp_max<0x128>(m);                // row_ror 8
  const int mi = __builtin_bit_cast(int, m);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(mi, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(mi, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(mi, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(mi, 48));
  m = fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
  const unsigned long long hit = __ballot(ok && v == m);
  lane = hit ? __ffsll((long long)hit) - 1 : -1;
  v = m;
}

template <int NT>
__global__ __launch_bounds__(NT) void mmr_kernel(MmrArgs p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int NW = NT / 64;
  float* red_v = smem;                                   // [2][4]
  int* red_i = reinterpret_cast<int*>(smem + 8);         // [2][4]
  float* s_inv = smem + 16;                              // [NT]
  int* s_grp = reinterpret_cast<int*>(smem + 16 + NT);   // [NT]
  int* s_row = reinterpret_cast<int*>(smem + 16 + 2 * NT);   // [NT] corpus row of every candidate (global path)
  float* prow = smem + 16 + 3 * NT;                      // [dim] the picked row (global path)
  f32x4* rows = reinterpret_cast<f32x4*>(prow + p.dim);  // [dim / 4][NT] x 4 consecutive d (LDS path)

  const int j = threadIdx.x, w = j >> 6;
  const int dim = p.dim, d4n = dim >> 2;
  const int64_t q = blockIdx.x;

  // ---- set-up: validity, own row, norm
  float s = 0.f;
  int64_t id = -1;
  if (j < p.k1) {
    s = p.scores[q * p.k1 + j];
    id = p.idx[q * p.k1 + j];
  }
  const bool valid = j < p.k1 && id >= 0 && id < p.nc && __builtin_isfinite(s);
  const int grp = (valid && p.cap > 0) ? p.groups[id] : -1;
  const f32x4* crow = reinterpret_cast<const f32x4*>(p.c + (valid ? id : 0) * (int64_t)dim);
  float inv = 0.f;
  if (valid) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (p.rows_lds) {
#pragma unroll 4
      for (int d4 = 0; d4 < d4n; ++d4) {
        const f32x4 v = crow[d4];
        rows[d4 * NT + j] = v;
        a0 = __fadd_rn(a0, __fmul_rn(v.x, v.x));
        a1 = __fadd_rn(a1, __fmul_rn(v.y, v.y));
        a2 = __fadd_rn(a2, __fmul_rn(v.z, v.z));
        a3 = __fadd_rn(a3, __fmul_rn(v.w, v.w));
      }
    } else {
#pragma unroll 4
      for (int d4 = 0; d4 < d4n; ++d4) {
        const f32x4 v = crow[d4];
        a0 = __fadd_rn(a0, __fmul_rn(v.x, v.x));
        a1 = __fadd_rn(a1, __fmul_rn(v.y, v.y));
        a2 = __fadd_rn(a2, __fmul_rn(v.z, v.z));
        a3 = __fadd_rn(a3, __fmul_rn(v.w, v.w));
      }
    }
    const float n2 = __fadd_rn(__fadd_rn(a0, a1), __fadd_rn(a2, a3));
    inv = n2 > 0.f ? __fdiv_rn(1.0f, __fsqrt_rn(n2)) : 0.f;
  }
  s_inv[j] = inv;
  s_grp[j] = grp;
  s_row[j] = valid ? (int)id : 0;

  // ---- relevance: min / max of the valid scores
  float lo = valid ? s : __builtin_inff(), hi = valid ? s : -__builtin_inff();
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off));
    hi = fmaxf(hi, __shfl_xor(hi, off));
  }
  if (NW > 1) {
    if ((j & 63) == 0) { red_v[w] = lo; red_v[4 + w] = hi; }
    __syncthreads();
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) { lo = fminf(lo, red_v[ww]); hi = fmaxf(hi, red_v[4 + ww]); }
  }
  __syncthreads();          // set-up stores (and the reads of red_v above) are done before the first pick
  const float rel = (valid && hi > lo) ? __fdiv_rn(__fsub_rn(s, lo), __fsub_rn(hi, lo)) : 0.f;
  const float lam = p.lam, om = __fsub_rn(1.0f, lam);
  const float lrel = __fmul_rn(lam, rel);

  float pen = 0.f;
  int cnt = 0;
  bool picked = false;
  int t = 0;
  for (; t < p.k; ++t) {
    const bool eligible = valid && !picked && !(grp >= 0 && cnt >= p.cap);      // grp >= 0 only with cap > 0
    float bv = eligible ? __fsub_rn(lrel, __fmul_rn(om, pen)) : -__builtin_inff();
    int bi;
    wave_argmax(bv, bi, eligible);
    bi = bi < 0 ? kNone : w * 64 + bi;
    if (NW > 1) {
      const int buf = (t & 1) * 4;
      if ((j & 63) == 0) { red_v[buf + w] = bv; red_i[buf + w] = bi; }
      __syncthreads();
      bv = red_v[buf]; bi = red_i[buf];
#pragma unroll
      for (int ww = 1; ww < NW; ++ww) {                    // waves in position order: a later one wins only when larger
        const float ov = red_v[buf + ww];
        const int oi = red_i[buf + ww];
        const bool better = oi != kNone && (bi == kNone || ov > bv);
        bv = better ? ov : bv;
        bi = better ? oi : bi;
      }
    }
    const int pk = __builtin_amdgcn_readfirstlane(bi);
    if (pk == kNone) break;
    if (j == pk) {
      picked = true;
      p.out_s[q * p.k + t] = s;
      p.out_i[q * p.k + t] = id;
    }
    if (t + 1 == p.k) { ++t; break; }                    // the last pick changes nothing anyone reads
    if (!p.rows_lds) {
      const f32x4* src = reinterpret_cast<const f32x4*>(p.c + (int64_t)s_row[pk] * dim);
      for (int d4 = j; d4 < d4n; d4 += NT) reinterpret_cast<f32x4*>(prow)[d4] = src[d4];
      __syncthreads();
    }
    if (valid) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      if (p.rows_lds) {
        const f32x4* rj = rows + j;
        const f32x4* rp = rows + pk;
#pragma unroll 8
        for (int d4 = 0; d4 < d4n; ++d4) {
          const f32x4 x = rj[d4 * NT], y = rp[d4 * NT];
          a0 = __fadd_rn(a0, __fmul_rn(x.x, y.x));
          a1 = __fadd_rn(a1, __fmul_rn(x.y, y.y));
          a2 = __fadd_rn(a2, __fmul_rn(x.z, y.z));
          a3 = __fadd_rn(a3, __fmul_rn(x.w, y.w));
        }
      } else {
        const f32x4* pr = reinterpret_cast<const f32x4*>(prow);
#pragma unroll 4
        for (int d4 = 0; d4 < d4n; ++d4) {
          const f32x4 x = crow[d4], y = pr[d4];
          a0 = __fadd_rn(a0, __fmul_rn(x.x, y.x));
          a1 = __fadd_rn(a1, __fmul_rn(x.y, y.y));
          a2 = __fadd_rn(a2, __fmul_rn(x.z, y.z));
          a3 = __fadd_rn(a3, __fmul_rn(x.w, y.w));
        }
      }
      const float dot = __fadd_rn(__fadd_rn(a0, a1), __fadd_rn(a2, a3));
      const float sim = __fmul_rn(__fmul_rn(dot, inv), s_inv[pk]);
      pen = sim > pen ? sim : pen;
      if (grp >= 0 && grp == s_grp[pk]) ++cnt;
    }
  }
  for (int u = t + j; u < p.k; u += NT) {               // t is uniform: the unfilled tail
    p.out_s[q * p.k + u] = -__builtin_inff();
    p.out_i[q * p.k + u] = -1;
  }
}

template <int NT>
int launch_mmr(const MmrArgs& a, int64_t nq, hipStream_t stream) {
  const int lds = (16 + 3 * NT + a.dim + (a.rows_lds ? a.dim * NT : 0)) * 4;
  auto kern = mmr_kernel<NT>;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
    return tt::fail(TT_ERR_LAUNCH, "tt_mmr_rerank_f32: hipFuncSetAttribute(LDS %d) failed", lds);
  tt::launch("mmr", kern, dim3((unsigned)nq), dim3(NT), (unsigned)lds, stream, a);
  return tt::check_launch("mmr");
}

}  // namespace

extern "C" int tt_mmr_rerank_f32(const float* scores, const int64_t* idx, int64_t nq, int32_t k1, const float* c, int64_t nc,
                                 int32_t dim, const int32_t* groups, int32_t max_per_group, float lambda, int32_t k,
                                 float* out_scores, int64_t* out_idx, tt_stream_t stream_) {
  const char* fn = "tt_mmr_rerank_f32";
  TT_REQUIRE(scores && idx && c && out_scores && out_idx, "%s: null pointer (scores, idx, c, out_scores, out_idx)", fn);
  TT_REQUIRE(nq >= 0 && nq <= INT32_MAX, "%s: nq %lld not in [0, 2^31 - 1]", fn, (long long)nq);
  TT_REQUIRE(k1 >= 1 && k1 <= TT_TOPK_MAX_K, "%s: k1 %d not in [1, %d]", fn, k1, TT_TOPK_MAX_K);
  TT_REQUIRE(k >= 1 && k <= k1, "%s: k %d not in [1, k1 = %d]", fn, k, k1);
  TT_REQUIRE(dim >= 4 && dim <= 1024 && dim % 4 == 0, "%s: dim %d must be a multiple of 4 in [4, 1024]", fn, dim);
  TT_REQUIRE(nc >= 1 && nc <= INT32_MAX, "%s: nc %lld not in [1, 2^31 - 1]", fn, (long long)nc);
  TT_REQUIRE(lambda >= 0.f && lambda <= 1.f, "%s: lambda %g not in [0, 1]", fn, (double)lambda);
  TT_REQUIRE(max_per_group >= 0, "%s: max_per_group %d is negative", fn, max_per_group);
  TT_REQUIRE(max_per_group == 0 || groups != nullptr, "%s: max_per_group %d needs groups", fn, max_per_group);
  TT_REQUIRE(tt::aligned16(c), "%s: c must be 16-byte aligned", fn);
  if (nq == 0) return TT_OK;
  MmrArgs a{};
  a.scores = scores; a.idx = idx; a.c = c; a.groups = groups; a.out_s = out_scores; a.out_i = out_idx;
  a.nc = nc; a.k1 = k1; a.k = k; a.dim = dim; a.cap = max_per_group; a.lam = lambda;
  const int nt = k1 <= 64 ? 64 : (k1 <= 128 ? 128 : 256);
  a.rows_lds = (int64_t)nt * dim * 4 <= kRowsLdsMax;
  hipStream_t stream = tt::as_stream(stream_);
  switch (nt) {
    case 64: return launch_mmr<64>(a, nq, stream);
    case 128: return launch_mmr<128>(a, nq, stream);
    default: return launch_mmr<256>(a, nq, stream);
  }
}
