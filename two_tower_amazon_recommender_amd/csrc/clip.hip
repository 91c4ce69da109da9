// Global-norm gradient clipping (tf.clip_by_global_norm) over every gradient buffer of a step, in two launches however many
// buffers there are.  A step's gradient is not one tensor: up to a handful of [rows, dim] gradient-row buffers (the towers' input
// gradients, the attention pool's slot rows) and, per dense optimizer segment, n_slabs gradient slabs that the optimizer
// launches sum themselves.  Both kinds are cut into CHUNKS - a function of the shapes alone - and the list of buffers with the
// first chunk of each rides in the kernel arguments (TT_CLIP_MAX_BUFFERS descriptors: 1.7 KB, read with scalar loads).
//   launch 1  workgroup w walks the chunks w, w + grid, ...; every thread adds its squares into one f32 register in that order,
//             the workgroup reduces through a wave butterfly and LDS and writes ONE partial.  A dense chunk is 1024 elements:
//             a thread owns 4 consecutive ones, adds their slabs in slab order (8 loads in flight, the optimizer's order and
//             its bits) and squares the sums.  A row chunk is 4 rows per lane group: a group of G lanes (the power of two >=
//             dim / 4, at most a wave) owns a row, derives its factor from the slot ids (a butterfly over the group's counts)
//             and skips a row whose factor is 0 - such a row may hold stale or non-finite data.
//   launch 2  every workgroup adds the partials in the same fixed order (f64), forms norm and scale, workgroup 0 stores them,
//             and - unless scale is exactly 1 - all of them multiply their chunks in place: a dense chunk is 4096 elements of
//             ONE slab, a row chunk 1024 float4 of the flat buffer - four float4 per thread, all loaded before the first store.
// No atomics anywhere; the bits depend on the inputs and the shapes only.  HBM-bound: every gradient byte is read once by
// launch 1 and, where something is clipped, read and written once by launch 2 (3 x the gradient bytes).
#include "common.h"
#include <math.h>
#include <string.h>

namespace {

using tt::f32x4;

constexpr int kThreads = 256;
constexpr int kDenseChunk = 1024;            // elements of a dense chunk (a float4 per thread)
constexpr int kRowsPerGroup = 4;             // rows a lane group takes per chunk
constexpr int kFlatChunk4 = 1024;            // float4 of a row buffer's chunk in launch 2
constexpr int kScaleChunk = 4096;            // elements of ONE slab in a dense chunk of launch 2 (4 float4 per thread in flight)
constexpr int kMaxGrid = 1024;               // workgroups of launch 1 = partials (256 CUs x 4)
constexpr int kMaxScaleGrid = 2048;          // workgroups of launch 2 (256 CUs x 8: every one resident)
constexpr int kSlabsInFlight = 8;

struct ClipArgs {
  tt_clip_buffer b[TT_CLIP_MAX_BUFFERS];
  uint32_t sum0[TT_CLIP_MAX_BUFFERS + 1];    // first chunk of buffer i in launch 1 (sum0[n]: their number)
  uint32_t scale0[TT_CLIP_MAX_BUFFERS + 1];  // likewise in launch 2
  uint8_t glog2[TT_CLIP_MAX_BUFFERS];        // row buffers: log2 of the lanes per row
  uint8_t vec[TT_CLIP_MAX_BUFFERS];          // dense buffers: 16-byte loads allowed (data aligned, slab_stride % 4 == 0)
  int32_t n;
};

__device__ __forceinline__ float sq4(float s, const f32x4& v) {
  s = s + v.x * v.x; s = s + v.y * v.y; s = s + v.z * v.z; s = s + v.w * v.w;
  return s;
}

// sum of squares of the slab sums of elements [1024 k, 1024 k + 1024) of a dense buffer, added to acc
__device__ __forceinline__ float dense_sumsq(float acc, const tt_clip_buffer& B, uint32_t k, bool vec) {
  const int64_t e0 = (int64_t)k * kDenseChunk;
  const int ns = B.n_slabs;
  if (vec) {
    const int64_t e = e0 + 4 * (int64_t)threadIdx.x;
    if (e + 3 < B.count) {
      const f32x4* __restrict__ gs = reinterpret_cast<const f32x4*>(B.data + e);
      const int64_t st4 = B.slab_stride / 4;
      f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int s0 = 0; s0 < ns; s0 += kSlabsInFlight) {
        f32x4 v[kSlabsInFlight];
#pragma unroll
        for (int u = 0; u < kSlabsInFlight; ++u) v[u] = gs[(int64_t)(s0 + u < ns ? s0 + u : ns - 1) * st4];   // (past the end: an L1 hit)
#pragma unroll
        for (int u = 0; u < kSlabsInFlight; ++u)
          if (s0 + u < ns) g = (s0 + u == 0) ? v[u] : g + v[u];
      }
      return sq4(acc, g);
    }
    for (int j = 0; j < 4; ++j)                // the tail of a count that is no multiple of 4
      if (e + j < B.count) {
        float g = B.data[e + j];
        for (int s = 1; s < ns; ++s) g = g + B.data[(int64_t)s * B.slab_stride + e + j];
        acc = acc + g * g;
      }
    return acc;
  }
#pragma unroll
  for (int u = 0; u < kDenseChunk / kThreads; ++u) {
    const int64_t e = e0 + threadIdx.x + u * kThreads;
    if (e < B.count) {
      float g = B.data[e];
      for (int s = 1; s < ns; ++s) g = g + B.data[(int64_t)s * B.slab_stride + e];
      acc = acc + g * g;
    }
  }
  return acc;
}

// f_r * |row r|^2 of the rows of chunk k of a row buffer, added to acc
__device__ __forceinline__ float rows_sumsq(float acc, const tt_clip_buffer& B, uint32_t k, int glog2) {
  const int G = 1 << glog2, groups = kThreads >> glog2;
  const int l = threadIdx.x & (G - 1), grp = threadIdx.x >> glog2;
  const int dim4 = B.dim / 4;
  const f32x4* __restrict__ data = reinterpret_cast<const f32x4*>(B.data);
#pragma unroll
  for (int r = 0; r < kRowsPerGroup; ++r) {
    const int64_t row = ((int64_t)k * kRowsPerGroup + r) * groups + grp;
    const bool live = row < B.rows;
    float f = B.weight;
    if (B.mode == TT_CLIP_SLOT_MASK) {         // (the mode is uniform over the launch's chunk)
      if (live && B.slot_ids[row] >= 0) f = f + 1.0f;
    } else if (B.mode != TT_CLIP_ROWS) {
      int n = 0;
      if (live)
        for (int j = l; j < B.L; j += G) n += B.slot_ids[row * B.L + j] >= 0 ? 1 : 0;
      for (int s = 0; s < glog2; ++s) n += __shfl_xor(n, 1 << s, 64);      // every lane of the group: the bag's kept slots
      if (n > 0) f = f + (B.mode == TT_CLIP_BAG_SUM ? (float)n : B.mode == TT_CLIP_BAG_MEAN ? 1.0f / (float)n : 1.0f);
    }
    if (live && f != 0.f) {
      float p = 0.f;
      for (int c = l; c < dim4; c += G) p = sq4(p, data[row * dim4 + c]);
      acc = acc + f * p;
    }
  }
  return acc;
}

__global__ __launch_bounds__(kThreads) void clip_sumsq_kernel(ClipArgs a, float* __restrict__ partials) {
  __shared__ float red[kThreads / 64];
  const uint32_t total = a.sum0[a.n];
  float acc = 0.f;
  for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
    int i = 0;
    while (a.sum0[i + 1] <= c) ++i;
    const tt_clip_buffer& B = a.b[i];
    if (B.mode == TT_CLIP_DENSE) acc = dense_sumsq(acc, B, c - a.sum0[i], a.vec[i] != 0);
    else acc = rows_sumsq(acc, B, c - a.sum0[i], a.glog2[i]);
  }
  for (int s = 1; s < 64; s <<= 1) acc = acc + __shfl_xor(acc, s, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(kThreads) void clip_scale_kernel(ClipArgs a, const float* __restrict__ partials, int n_partials, float clip,
                                                              float* __restrict__ stats) {
  __shared__ double red[kThreads];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += kThreads) s += (double)partials[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  const float norm = sqrtf((float)red[0]);
  const float scale = isfinite(norm) ? clip / fmaxf(norm, clip) : __builtin_nanf("");
  if (blockIdx.x == 0 && threadIdx.x == 0) { stats[0] = norm; stats[1] = scale; }
  if (scale == 1.0f) return;                   // nothing is clipped: the buffers stay as they are, unread
  const uint32_t total = a.scale0[a.n];
  for (uint32_t c = blockIdx.x; c < total; c += gridDim.x) {
    int i = 0;
    while (a.scale0[i + 1] <= c) ++i;
    const tt_clip_buffer& B = a.b[i];
    const uint32_t k = c - a.scale0[i];
    if (B.mode == TT_CLIP_DENSE) {
      const uint32_t per = (uint32_t)((B.count + kScaleChunk - 1) / kScaleChunk);
      float* slab = B.data + (int64_t)(k / per) * B.slab_stride;
      const int64_t e0 = (int64_t)(k % per) * kScaleChunk;
      constexpr int U = kScaleChunk / (4 * kThreads);        // float4 per thread, all loaded before the first store
      if (a.vec[i]) {
        f32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t e = e0 + 4 * (int64_t)(threadIdx.x + u * kThreads);
          if (e + 3 < B.count) v[u] = *reinterpret_cast<const f32x4*>(slab + e);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int64_t e = e0 + 4 * (int64_t)(threadIdx.x + u * kThreads);
          if (e + 3 < B.count) {
            *reinterpret_cast<f32x4*>(slab + e) = v[u] * scale;
          } else {
            for (int j = 0; j < 4; ++j)
              if (e + j < B.count) slab[e + j] = slab[e + j] * scale;
          }
        }
      } else {
#pragma unroll 4
        for (int u = 0; u < kScaleChunk / kThreads; ++u) {
          const int64_t e = e0 + threadIdx.x + u * kThreads;
          if (e < B.count) slab[e] = slab[e] * scale;
        }
      }
    } else {
      f32x4* data = reinterpret_cast<f32x4*>(B.data);
      const int64_t n4 = B.rows * (B.dim / 4);
      f32x4 v[kFlatChunk4 / kThreads];
#pragma unroll
      for (int u = 0; u < kFlatChunk4 / kThreads; ++u) {
        const int64_t i4 = (int64_t)k * kFlatChunk4 + threadIdx.x + u * kThreads;
        if (i4 < n4) v[u] = data[i4];
      }
#pragma unroll
      for (int u = 0; u < kFlatChunk4 / kThreads; ++u) {
        const int64_t i4 = (int64_t)k * kFlatChunk4 + threadIdx.x + u * kThreads;
        if (i4 < n4) data[i4] = v[u] * scale;
      }
    }
  }
}

// validates the list and cuts it into chunks; `a` may be NULL (the workspace query)
int plan(const char* who, const tt_clip_buffer* bufs, int32_t n_bufs, ClipArgs* a, int64_t* sum_chunks, int64_t* scale_chunks) {
  TT_REQUIRE(n_bufs >= 0 && n_bufs <= TT_CLIP_MAX_BUFFERS, "%s: n_bufs must be in 0..%d (got %d)", who, TT_CLIP_MAX_BUFFERS, n_bufs);
  TT_REQUIRE(bufs != nullptr || n_bufs == 0, "%s: bufs is NULL", who);
  int64_t sum = 0, scale = 0;
  for (int i = 0; i < n_bufs; ++i) {
    const tt_clip_buffer& b = bufs[i];
    int64_t c1 = 0, c2 = 0;
    int glog2 = 0;
    bool vec = false;
    TT_REQUIRE(b.mode >= TT_CLIP_DENSE && b.mode <= TT_CLIP_SLOT_MASK, "%s: buffer %d: unknown mode %d", who, i, b.mode);
    if (b.mode == TT_CLIP_DENSE) {
      TT_REQUIRE(b.n_slabs >= 1, "%s: buffer %d: n_slabs must be >= 1 (got %d)", who, i, b.n_slabs);
      TT_REQUIRE(b.count >= 0, "%s: buffer %d: count must be >= 0", who, i);
      TT_REQUIRE(b.n_slabs == 1 || b.slab_stride >= b.count, "%s: buffer %d: slab_stride must be >= count", who, i);
      if (b.count > 0) {
        TT_REQUIRE(b.data != nullptr, "%s: buffer %d: null pointer (data)", who, i);
        TT_REQUIRE((reinterpret_cast<uintptr_t>(b.data) & 3u) == 0, "%s: buffer %d: data must be 4-byte aligned", who, i);
        c1 = (b.count + kDenseChunk - 1) / kDenseChunk;
        c2 = (b.count + kScaleChunk - 1) / kScaleChunk * b.n_slabs;
        vec = tt::aligned16(b.data) && (b.n_slabs == 1 || b.slab_stride % 4 == 0);
      }
    } else {
      TT_REQUIRE(b.rows >= 0, "%s: buffer %d: rows must be >= 0", who, i);
      TT_REQUIRE(b.dim >= 4 && b.dim % 4 == 0, "%s: buffer %d: dim must be a multiple of 4 (got %d)", who, i, b.dim);
      TT_REQUIRE(b.weight >= 0.0f && isfinite(b.weight), "%s: buffer %d: weight must be finite and >= 0", who, i);
      const bool bag = b.mode >= TT_CLIP_BAG_SUM && b.mode <= TT_CLIP_BAG_SQRTN;
      TT_REQUIRE(!bag || b.L >= 1, "%s: buffer %d: L must be >= 1 in a bag mode (got %d)", who, i, b.L);
      if (b.rows > 0) {
        TT_REQUIRE(b.data != nullptr, "%s: buffer %d: null pointer (data)", who, i);
        TT_REQUIRE(b.mode == TT_CLIP_ROWS || b.slot_ids != nullptr, "%s: buffer %d: null pointer (slot_ids)", who, i);
        TT_REQUIRE(tt::aligned16(b.data), "%s: buffer %d: a row buffer must be 16-byte aligned", who, i);
        while ((1 << glog2) < b.dim / 4 && glog2 < 6) ++glog2;
        const int64_t rows_per_chunk = (int64_t)(kThreads >> glog2) * kRowsPerGroup;
        c1 = (b.rows + rows_per_chunk - 1) / rows_per_chunk;
        c2 = (b.rows * (b.dim / 4) + kFlatChunk4 - 1) / kFlatChunk4;
      }
    }
    if (a != nullptr) {
      a->b[i] = b;
      a->sum0[i] = (uint32_t)sum;
      a->scale0[i] = (uint32_t)scale;
      a->glog2[i] = (uint8_t)glog2;
      a->vec[i] = vec ? 1 : 0;
    }
    sum += c1;
    scale += c2;
    TT_REQUIRE(sum <= 0x7fffffff && scale <= 0x7fffffff, "%s: too many elements", who);
  }
  if (a != nullptr) {
    a->n = n_bufs;
    a->sum0[n_bufs] = (uint32_t)sum;
    a->scale0[n_bufs] = (uint32_t)scale;
  }
  *sum_chunks = sum;
  *scale_chunks = scale;
  return TT_OK;
}

int64_t grid_of(int64_t chunks) { return chunks < kMaxGrid ? chunks : kMaxGrid; }

}  // namespace

extern "C" int64_t tt_clip_workspace_bytes(const tt_clip_buffer* bufs, int32_t n_bufs) {
  int64_t sum = 0, scale = 0;
  if (plan("tt_clip_workspace_bytes", bufs, n_bufs, nullptr, &sum, &scale) != TT_OK) return -1;
  const int64_t bytes = grid_of(sum) * (int64_t)sizeof(float);
  return bytes < 256 ? 256 : (bytes + 255) / 256 * 256;
}

extern "C" int tt_clip_global_norm_f32(const tt_clip_buffer* bufs, int32_t n_bufs, float clip_norm, void* workspace,
                                       int64_t workspace_bytes, float* stats, tt_stream_t stream) {
  const char* who = "tt_clip_global_norm_f32";
  TT_REQUIRE(clip_norm > 0.0f && isfinite(clip_norm), "%s: clip_norm must be finite and > 0", who);
  TT_REQUIRE(stats != nullptr, "%s: null pointer (stats)", who);
  ClipArgs a{};
  int64_t sum = 0, scale = 0;
  if (int rc = plan(who, bufs, n_bufs, &a, &sum, &scale)) return rc;
  hipStream_t st = tt::as_stream(stream);
  if (sum == 0) {                              // nothing to add up: norm 0, scale 1, by two 4-byte fills (no kernel)
    const float one = 1.0f;
    uint32_t one_bits;
    memcpy(&one_bits, &one, sizeof(one_bits));
    if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(stats), 0, 1, st) != hipSuccess ||
        hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(stats + 1), (int)one_bits, 1, st) != hipSuccess)
      return tt::fail(TT_ERR_LAUNCH, "%s: hipMemsetD32Async failed", who);
    return TT_OK;
  }
  TT_REQUIRE(workspace != nullptr, "%s: null pointer (workspace)", who);
  TT_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, "%s: workspace must be 4-byte aligned", who);
  const int64_t g1 = grid_of(sum), g2 = scale < kMaxScaleGrid ? scale : kMaxScaleGrid;
  if (workspace_bytes < g1 * (int64_t)sizeof(float))
    return tt::fail(TT_ERR_WORKSPACE, "%s: workspace of %lld bytes, need %lld (tt_clip_workspace_bytes)", who, (long long)workspace_bytes,
                    (long long)(g1 * (int64_t)sizeof(float)));
  float* partials = static_cast<float*>(workspace);
  tt::launch("clip_sumsq", clip_sumsq_kernel, dim3((unsigned)g1), dim3(kThreads), 0, st, a, partials);
  tt::launch("clip_scale", clip_scale_kernel, dim3((unsigned)g2), dim3(kThreads), 0, st, a, (const float*)partials, (int)g1, clip_norm, stats);
  return tt::check_launch(who);
}
