// Streaming item-frequency estimation (Yi et al. 2019, "Sampling-bias-corrected neural modeling", Algorithms 2 and 3): a hashed
// sketch of "steps since this item was last a positive", updated by every batch, whose reciprocal is the probability the scorer's
// logQ correction takes.  `hashes` rows of `slots` slots; a slot is ONE 64-bit word - low half `last` (int32, the 1-based step of
// the last hit, 0 = never), high half the bits of `delta` (f32, the moving average of the gap in steps).
// Latency-bound: `hashes` random 8-byte reads and at most as many 8-byte writes per id, a few hundred KB per step.  The shape of
// sample.hip: 256-thread blocks, grid-stride, no LDS, no atomic read-modify-write but the flag.
//
// Why the result does not depend on how workgroups interleave: a slot is read with one 64-bit atomic load and written with one
// 64-bit atomic store (relaxed, agent scope: single-copy atomic by the memory model), so a thread sees either the pair from
// before the step or the finished pair of this step.  From the first it computes the same new pair as every other thread that
// hits the slot - the new pair is a function of the old pair, the step and alpha alone - and stores it (identical stores); in the
// second `last == step` and it leaves the slot alone.  Either way it knows the slot's final delta.  Duplicates and collisions
// inside a batch need no sort and no lock.  Ids at or beyond n_update (sampled negatives) never write and must read the slots
// after ALL updates: they run in a second stream-ordered launch.
//
// One deviation from the paper: on a slot's FIRST sighting delta is set to the gap itself (the step number), not to
// alpha * gap.  The paper's zero start biases every estimate by (1 - alpha)^k, which never decays for the tail items the
// correction exists for.  (A slot that was never hit estimates a gap of `step`: the item has not been seen in `step` steps.)
// A property of the estimator: a gap cannot be below one step, so 1 / D saturates at 1 for items that occur several times a batch.
#include "common.h"

namespace {

struct FreqKeys {
  uint64_t key[4];                       // stream_key(seed, tensor_id + h)
};

__device__ __forceinline__ uint64_t slot_load(const uint64_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void slot_store(uint64_t* p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// candidates j0 <= j < j1; those with j < n_update feed the sketch
__global__ __launch_bounds__(256) void frequency_estimate_kernel(
    const int64_t* __restrict__ ids, int64_t j0, int64_t j1, int64_t n_update, uint64_t n_items, uint64_t* sketch, int hashes,
    uint64_t slots, FreqKeys keys, int32_t step, float alpha, float one_minus_alpha, const float* __restrict__ sampler_prob,
    int mix, float uniform_prob, float f_neg, float f_all, float* __restrict__ prob, int32_t* __restrict__ oob_flag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float f_step = (float)step;
  for (int64_t j = j0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < j1; j += stride) {
    const int64_t id = ids[j];
    const bool ok = id >= 0 && (uint64_t)id < n_items;
    float p = 1.0f;
    if (!ok) {
      if (oob_flag != nullptr) atomicOr(oob_flag, 1);
    } else {
      const bool update = j < n_update;
      float big = 0.0f;                                                        // every d_h is >= 1
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        if (h < hashes) {
          const uint64_t x = tt::splitmix(keys.key[h] + (uint64_t)id);
          const uint64_t s = ((x >> 32) * slots) >> 32;                        // fill_ids_kernel's bucket rule, s < slots
          uint64_t* cell = sketch + (uint64_t)h * slots + s;
          const uint64_t w = slot_load(cell);
          const int32_t last = (int32_t)(uint32_t)w;
          float delta = __uint_as_float((uint32_t)(w >> 32));
          if (update && last != step) {
            const float gap = (float)(step - last);
            delta = last == 0 ? gap : __fadd_rn(__fmul_rn(one_minus_alpha, delta), __fmul_rn(alpha, gap));
            slot_store(cell, ((uint64_t)__float_as_uint(delta) << 32) | (uint64_t)(uint32_t)step);
          } else if (last == 0) {
            delta = f_step;
          }
          big = fmaxf(big, delta);
        }
      }
      p = __fdiv_rn(1.0f, big);
      if (mix) {
        const float u = sampler_prob != nullptr ? sampler_prob[id] : uniform_prob;
        p = __fdiv_rn(__fadd_rn(p, __fmul_rn(f_neg, u)), f_all);
      }
    }
    prob[j] = p;
  }
}

}  // namespace

extern "C" int tt_frequency_estimate_i64(const int64_t* ids, int64_t n, int64_t n_update, int64_t n_items, int64_t* sketch,
                                         int32_t hashes, int64_t slots, int64_t step, float alpha, uint64_t seed,
                                         uint64_t tensor_id, const float* sampler_prob, int32_t mix, float* prob,
                                         int32_t* oob_flag, tt_stream_t stream) {
  const char* what = "tt_frequency_estimate_i64";
  TT_REQUIRE(hashes >= 1 && hashes <= 4, "%s: hashes must be in 1..4 (got %d)", what, hashes);
  TT_REQUIRE(slots >= 1 && slots <= (int64_t)1 << 32, "%s: slots must be in 1..2^32 (got %lld)", what, (long long)slots);
  TT_REQUIRE(n_items >= 1 && n_items <= (int64_t)1 << 32, "%s: n_items must be in 1..2^32 (got %lld)", what, (long long)n_items);
  TT_REQUIRE(step >= 1 && step <= 0x7fffffff, "%s: step is 1-based and fits 31 bits: must be in 1..2^31-1 (got %lld)", what,
             (long long)step);
  TT_REQUIRE(alpha > 0.0f && alpha <= 1.0f, "%s: alpha must be in (0, 1] (got %g)", what, (double)alpha);
  TT_REQUIRE(n >= 0 && n <= 0x7fffffff, "%s: n must be in 0..2^31-1 (got %lld)", what, (long long)n);
  TT_REQUIRE(n_update >= 0 && n_update <= n, "%s: n_update must be in 0..n (got %lld, n = %lld)", what, (long long)n_update,
             (long long)n);
  TT_REQUIRE(mix == 0 || mix == 1, "%s: mix must be 0 or 1 (got %d)", what, mix);
  TT_REQUIRE(!mix || (n_update >= 1 && n_update < n), "%s: mix needs 1 <= n_update < n (got n_update %lld, n %lld)", what,
             (long long)n_update, (long long)n);
  TT_REQUIRE(sampler_prob == nullptr || mix, "%s: sampler_prob without mix", what);
  if (n == 0) return TT_OK;
  TT_REQUIRE(ids != nullptr && sketch != nullptr && prob != nullptr, "%s: null pointer (ids / sketch / prob)", what);
  FreqKeys keys;
  for (int h = 0; h < 4; ++h) keys.key[h] = tt::stream_key(seed, tensor_id + (uint64_t)h);
  const float one_minus_alpha = 1.0f - alpha;
  const float uniform_prob = 1.0f / (float)n_items;
  const int64_t bounds[3] = {0, n_update, n};
  const char* tags[2] = {"freq_update", "freq_estimate"};
  for (int part = 0; part < 2; ++part) {         // the updating candidates, then - stream-ordered behind them - the others
    const int64_t j0 = bounds[part], j1 = bounds[part + 1];
    if (j1 == j0) continue;
    int64_t blocks = (j1 - j0 + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;                                    // 8 blocks per CU, grid-stride the rest
    tt::launch(tags[part], frequency_estimate_kernel, dim3((unsigned)blocks), dim3(256), 0, tt::as_stream(stream), ids, j0, j1,
               n_update, (uint64_t)n_items, reinterpret_cast<uint64_t*>(sketch), (int)hashes, (uint64_t)slots, keys, (int32_t)step,
               alpha, one_minus_alpha, sampler_prob, (int)mix, uniform_prob, (float)(n - n_update), (float)n, prob, oob_flag);
  }
  return tt::check_launch(what);
}
