// Time-of-interaction context features (the TFRS context-feature recipe: timestamp -> Discretization -> Embedding plus the
// calendar fields, in the query model): ONE small table [R, dim] whose rows are the enabled fields' blocks - hour (24),
// day of week (7), month (12), period (N buckets of the training range) - in that order.  A pair's int64 timestamp (whole
// seconds since the Unix epoch, UTC; INT64_MIN = no timestamp) picks one row per field; the rows are summed in field order
// and added to the user tower's input.
//
// Forward: an HBM/L2-bound row kernel in the shape of gather.hip - a group of LPR lanes owns a pair (LPR = the power of two
// >= dim/4, at most a wave; 16-byte loads and stores), derives the indices from the timestamp in integer arithmetic
// (floor division, civil-from-days for the month), loads the F rows (all in flight together; the table is cache resident)
// and writes  s = ((row_0 + row_1) + row_2) + row_3  as  out = s | out + s | base_table[base_ids] + s.
//
// Backward: grad[r] = sum of dy[p] over the pairs that picked row r, EVERY row written in full, no atomics.  The tables are
// tiny and a full batch hits them: at 8192 pairs a day-of-week row has ~1170 adders, which float atomics serialise at the
// memory side and which the sparse optimizer's row ranges cannot spread.  Instead a workgroup owns (a row of a field - or 8
// consecutive rows of a field with more than 256 of them -, a tile of 32 columns) and reads the field's index column itself
// (4 n F bytes, cache resident): its 32 lane groups of 8 lanes (a float4 each) take the batch positions round robin - group
// g the positions g, g + 32, g + 64, ... in ascending order, four in flight - and add the dy rows that match into a sub-sum of their own,
// which starts at +0 (one row: registers; 8 rows: an LDS cell only that lane ever touches).  The 32 sub-sums then meet in
// LDS and are added in ascending g, starting from sub-sum 0:
//     grad[r][c] = (((s_0 + s_1) + s_2) + ... + s_31),    s_g = sum over t ascending of dy[g + 32 t][c] where idx matches
// - a fixed function of (n, idx): bit-identical across runs, grids and dims (tests/time_check.py restates it).  A row
// nobody hit is thirty-two zeros added up.  No sort plan either: the plan's sorted runs would again put ~1170 gradient rows
// behind one table row, and the position-interleaved sub-sums spread a hot row over 256 lanes without knowing the counts.
#include "common.h"

namespace {

constexpr int kFields = 4;
constexpr int kCard[kFields] = {24, 7, 12, 0};       // hour, day of week, month, period (time_buckets rows)
constexpr int kSub = 32;                             // sub-sums (lane groups) per workgroup of the backward launch
constexpr int kWideRows = 8;                         // rows per workgroup of a field with more than kWideCard rows
constexpr int kWideCard = 256;
constexpr int64_t kMissing = INT64_MIN;

struct Layout {
  int F;                       // enabled fields
  int field[kFields];          // which field column k of idx is (0 hour, 1 day of week, 2 month, 3 period)
  int card[kFields];           // its rows
  int off[kFields];            // its first row of the table
  int R;
};

// the enabled fields in their fixed order; false: a bad mask / bucket count
bool make_layout(int32_t field_mask, int32_t buckets, Layout* lay) {
  if (field_mask <= 0 || field_mask >= (1 << kFields)) return false;
  const bool period = (field_mask >> 3) & 1;
  if (period ? (buckets < 1 || buckets > 4096) : buckets != 0) return false;
  lay->F = lay->R = 0;
  for (int f = 0; f < kFields; ++f) {
    if (!((field_mask >> f) & 1)) continue;
    const int k = lay->F++;
    lay->field[k] = f;
    lay->card[k] = f == 3 ? buckets : kCard[f];
    lay->off[k] = lay->R;
    lay->R += lay->card[k];
  }
  return true;
}

struct FwdArgs {
  const int64_t* ts; const float* table; float* out; const float* base_table; const int64_t* base_ids; int32_t* idx_out;
  int64_t n, base_rows, time_min, time_max;
  int F, field[kFields], off[kFields], buckets, dim4, lpr_log2, accumulate;
};

// the row of field `f` (0 hour, 1 day of week, 2 month, 3 period) a timestamp picks; all integer, floor-divided
__device__ __forceinline__ int field_index(int f, int64_t t, int64_t days, int32_t sec, const FwdArgs& a) {
  if (f == 0) return sec / 3600;
  if (f == 1) {
    const int64_t q = (days + 3) / 7;
    int r = (int)((days + 3) - q * 7);
    return r < 0 ? r + 7 : r;                       // 1970-01-01 is a Thursday; Monday = 0
  }
  if (f == 2) {                                     // civil-from-days (the month of the proleptic Gregorian calendar)
    const int64_t z = days + 719468;
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const int32_t doe = (int32_t)(z - era * 146097);
    const int32_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    const int32_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const int32_t mp = (5 * doy + 2) / 153;
    return (mp < 10 ? mp + 3 : mp - 9) - 1;
  }
  const uint64_t span = (uint64_t)(a.time_max - a.time_min);               // < 2^40 (checked by the entry)
  const uint64_t x = t <= a.time_min ? 0 : t >= a.time_max ? span : (uint64_t)(t - a.time_min);
  return (int)(x * (uint64_t)a.buckets / (span + 1));                      // the product stays below 2^52
}

__global__ __launch_bounds__(256) void time_fwd_kernel(FwdArgs a, int32_t* __restrict__ oob_flag) {
  const int lpr = 1 << a.lpr_log2;
  const int groups = 256 >> a.lpr_log2;
  const int g = threadIdx.x >> a.lpr_log2;
  const int l = threadIdx.x & (lpr - 1);
  const int64_t p = (int64_t)blockIdx.x * groups + g;
  if (p >= a.n) return;
  const tt::f32x4* __restrict__ table = reinterpret_cast<const tt::f32x4*>(a.table);
  tt::f32x4* __restrict__ out = reinterpret_cast<tt::f32x4*>(a.out);

  const int64_t t = a.ts[p];
  int idx[kFields];
  if (t == kMissing) {
#pragma unroll
    for (int k = 0; k < kFields; ++k) idx[k] = -1;
  } else {
    int64_t days = t / 86400;
    int32_t sec = (int32_t)(t - days * 86400);
    if (sec < 0) { sec += 86400; days -= 1; }
#pragma unroll
    for (int k = 0; k < kFields; ++k) idx[k] = k < a.F ? field_index(a.field[k], t, days, sec, a) : -1;
  }
  if (a.idx_out != nullptr && l == 0) {
#pragma unroll
    for (int k = 0; k < kFields; ++k)
      if (k < a.F) a.idx_out[p * a.F + k] = idx[k];
  }
  int64_t bid = -1;
  if (a.base_table != nullptr) {
    bid = a.base_ids[p];
    if (bid < 0 || bid >= a.base_rows) {            // (tt_embedding_gather_f32's rule: a zero row; -1 sets no flag)
      if (bid != -1 && l == 0 && oob_flag != nullptr) atomicOr(oob_flag, 1);
      bid = -1;
    }
  }
  const tt::f32x4 zero{0.f, 0.f, 0.f, 0.f};
  for (int c = l; c < a.dim4; c += lpr) {           // one trip unless dim > 256
    tt::f32x4 v[kFields];
#pragma unroll
    for (int k = 0; k < kFields; ++k)
      v[k] = (k < a.F && idx[k] >= 0) ? table[(int64_t)(a.off[k] + idx[k]) * a.dim4 + c] : zero;
    tt::f32x4 b = zero;
    if (a.base_table != nullptr) {
      if (bid >= 0) b = reinterpret_cast<const tt::f32x4*>(a.base_table)[bid * a.dim4 + c];
    } else if (a.accumulate) {
      b = out[p * a.dim4 + c];
    }
    tt::f32x4 s = v[0];                             // (a missing timestamp: s = +0)
#pragma unroll
    for (int k = 1; k < kFields; ++k)
      if (k < a.F) s = s + v[k];
    out[p * a.dim4 + c] = (a.base_table != nullptr || a.accumulate) ? b + s : s;
  }
}

struct BwdArgs {
  const int32_t* idx; const float* dy; float* grad;
  int64_t n;
  int F, card[kFields], off[kFields], wide[kFields], first_item[kFields + 1];   // items of field k: [first_item[k], first_item[k + 1])
  int dim, tiles;
};

__global__ __launch_bounds__(256) void time_bwd_kernel(BwdArgs a) {
  __shared__ tt::f32x4 part[kWideRows * kSub * 8];          // [row of the range][sub-sum][8 lanes x float4]: 32 KB
  int k = 0;
  while (k + 1 < a.F && (int)blockIdx.x >= a.first_item[k + 1]) ++k;
  const int item = (int)blockIdx.x - a.first_item[k];
  const int ct = item % a.tiles;                            // the tile of 32 columns
  const int w = a.wide[k] ? kWideRows : 1;
  const int r0 = (item / a.tiles) * w;                      // first row of the range, within the field
  const int rows = min(w, a.card[k] - r0);
  const int F = a.F, dim4 = a.dim >> 2;
  const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
  const int c4 = ct * 8 + l;                                // this lane's float4 column
  const bool col_ok = c4 < dim4;
  const int32_t* __restrict__ idx = a.idx + k;
  const tt::f32x4* __restrict__ dy = reinterpret_cast<const tt::f32x4*>(a.dy);
  const tt::f32x4 zero{0.f, 0.f, 0.f, 0.f};
  constexpr int U = 4;                                      // positions a group has in flight

  if (w == 1) {
    tt::f32x4 acc = zero;
    for (int64_t p0 = g; p0 < a.n; p0 += (int64_t)kSub * U) {
      int id[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t p = p0 + (int64_t)u * kSub;
        id[u] = p < a.n ? idx[p * F] : -1;
      }
      tt::f32x4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t p = p0 + (int64_t)u * kSub;
        v[u] = (p < a.n && id[u] == r0 && col_ok) ? dy[p * dim4 + c4] : zero;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)                           // ascending positions; + 0 where nothing matched (exact)
        acc = acc + v[u];
    }
    part[g * 8 + l] = acc;
  } else {
    for (int i = threadIdx.x; i < kWideRows * kSub * 8; i += 256) part[i] = zero;
    __syncthreads();
    for (int64_t p0 = g; p0 < a.n; p0 += (int64_t)kSub * U) {
      int rl[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t p = p0 + (int64_t)u * kSub;
        const int id = p < a.n ? idx[p * F] : -1;
        rl[u] = (id >= r0 && id < r0 + rows) ? id - r0 : -1;
      }
      tt::f32x4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t p = p0 + (int64_t)u * kSub;
        v[u] = (rl[u] >= 0 && col_ok) ? dy[p * dim4 + c4] : zero;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (rl[u] >= 0) {                                   // a cell only this lane reads and writes: program order suffices
          const int cell = (rl[u] * kSub + g) * 8 + l;
          part[cell] = part[cell] + v[u];
        }
    }
  }
  __syncthreads();
  const float* __restrict__ pf = reinterpret_cast<const float*>(part);
  for (int o = threadIdx.x; o < rows * 32; o += 256) {      // one thread per (row, column): the sub-sums in ascending order
    const int r = o >> 5, c = o & 31;
    float s = pf[(r * kSub) * 32 + c];
#pragma unroll 8
    for (int q = 1; q < kSub; ++q) s = s + pf[(r * kSub + q) * 32 + c];
    const int col = ct * 32 + c;
    if (col < a.dim) a.grad[(int64_t)(a.off[k] + r0 + r) * a.dim + col] = s;
  }
}

}  // namespace

extern "C" int tt_time_context_fwd_f32(const int64_t* timestamps, int64_t n, const float* table, int64_t table_rows, int32_t dim,
                                       int32_t field_mask, int32_t buckets, int64_t time_min, int64_t time_max,
                                       float* out, int32_t accumulate, const float* base_table, int64_t base_rows,
                                       const int64_t* base_ids, int32_t* idx_out, int32_t* oob_flag, tt_stream_t stream) {
  Layout lay;
  TT_REQUIRE(make_layout(field_mask, buckets, &lay),
             "tt_time_context_fwd_f32: field_mask must be in 1..15 and buckets in 1..4096 exactly when the period field (bit 3) is on "
             "(got mask %d, buckets %d)", field_mask, buckets);
  TT_REQUIRE(n >= 0 && n <= 0x7fffffff, "tt_time_context_fwd_f32: n must be in 0..2^31-1");
  TT_REQUIRE(dim > 0 && dim % 4 == 0 && dim <= 512, "tt_time_context_fwd_f32: dim must be a multiple of 4 in 4..512 (got %d)", dim);
  TT_REQUIRE(table_rows == lay.R, "tt_time_context_fwd_f32: the table must have %d rows for these fields (got %lld)", lay.R,
             (long long)table_rows);
  TT_REQUIRE(time_min <= time_max && (uint64_t)time_max - (uint64_t)time_min < (1ull << 40),
             "tt_time_context_fwd_f32: need time_min <= time_max and time_max - time_min < 2^40");
  TT_REQUIRE((base_table == nullptr) == (base_ids == nullptr), "tt_time_context_fwd_f32: base_table and base_ids are given both or neither");
  TT_REQUIRE(base_table == nullptr || (!accumulate && base_rows > 0),
             "tt_time_context_fwd_f32: a base needs accumulate 0 and base_rows > 0");
  if (n == 0) return TT_OK;
  TT_REQUIRE(timestamps && table && out, "tt_time_context_fwd_f32: null pointer");
  TT_REQUIRE(tt::aligned16(table) && tt::aligned16(out) && tt::aligned16(base_table),
             "tt_time_context_fwd_f32: table, out and base_table must be 16-byte aligned");
  FwdArgs a{};
  a.ts = timestamps; a.table = table; a.out = out; a.base_table = base_table; a.base_ids = base_ids; a.idx_out = idx_out;
  a.n = n; a.base_rows = base_rows; a.time_min = time_min; a.time_max = time_max;
  a.F = lay.F; a.buckets = buckets; a.dim4 = dim / 4; a.accumulate = accumulate ? 1 : 0;
  for (int k = 0; k < lay.F; ++k) { a.field[k] = lay.field[k]; a.off[k] = lay.off[k]; }
  while ((1 << a.lpr_log2) < a.dim4 && a.lpr_log2 < 6) ++a.lpr_log2;
  const int groups = 256 >> a.lpr_log2;
  const int64_t blocks = (n + groups - 1) / groups;
  tt::launch("time_context_fwd", time_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, tt::as_stream(stream), a, oob_flag);
  return tt::check_launch("tt_time_context_fwd_f32");
}

extern "C" int tt_time_context_bwd_f32(const int32_t* idx, const float* dy, int64_t n, int32_t dim, int32_t field_mask,
                                       int32_t buckets, int64_t table_rows, float* grad, tt_stream_t stream) {
  Layout lay;
  TT_REQUIRE(make_layout(field_mask, buckets, &lay),
             "tt_time_context_bwd_f32: field_mask must be in 1..15 and buckets in 1..4096 exactly when the period field (bit 3) is on "
             "(got mask %d, buckets %d)", field_mask, buckets);
  TT_REQUIRE(n >= 0 && n <= 0x7fffffff, "tt_time_context_bwd_f32: n must be in 0..2^31-1");
  TT_REQUIRE(dim > 0 && dim % 4 == 0 && dim <= 512, "tt_time_context_bwd_f32: dim must be a multiple of 4 in 4..512 (got %d)", dim);
  TT_REQUIRE(table_rows == lay.R, "tt_time_context_bwd_f32: grad must have %d rows for these fields (got %lld)", lay.R,
             (long long)table_rows);
  TT_REQUIRE(grad && (n == 0 || (idx && dy)), "tt_time_context_bwd_f32: null pointer");
  TT_REQUIRE(tt::aligned16(dy) && tt::aligned16(grad), "tt_time_context_bwd_f32: dy and grad must be 16-byte aligned");
  BwdArgs a{};
  a.idx = idx; a.dy = dy; a.grad = grad; a.n = n; a.F = lay.F; a.dim = dim; a.tiles = (dim + 31) / 32;
  for (int k = 0; k < lay.F; ++k) {
    a.card[k] = lay.card[k]; a.off[k] = lay.off[k]; a.wide[k] = lay.card[k] > kWideCard;
    const int w = a.wide[k] ? kWideRows : 1;
    a.first_item[k + 1] = a.first_item[k] + (lay.card[k] + w - 1) / w * a.tiles;
  }
  tt::launch("time_context_bwd", time_bwd_kernel, dim3((unsigned)a.first_item[lay.F]), dim3(256), 0, tt::as_stream(stream), a);
  return tt::check_launch("tt_time_context_bwd_f32");
}
