// Mixed negative sampling (Yang et al. 2020): one launch writes a step's whole candidate list - the batch's positives followed
// by n_neg items drawn from the corpus with the counter-based generator of fill.hip - and, when the item frequencies are given,
// every candidate's probability under the mixture of the in-batch and the sampled stream (what the scorer's logQ correction
// takes).  Latency-bound: 8 bytes read and 8 (+4) written per candidate plus two or three random 4-byte reads, tens of KB in
// all.  The shape of fill.hip: 256-thread blocks, grid-stride, plain loads and stores, no LDS, no atomics but the flag.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void sample_candidates_kernel(
    const int64_t* __restrict__ pos_ids, int64_t n_pos, int64_t n_neg, uint64_t n_items, int sampler,
    const float* __restrict__ alias_thr, const int32_t* __restrict__ alias_idx, const float* __restrict__ item_freq,
    const float* __restrict__ sampler_prob, float uniform_prob, float f_pos, float f_neg, float f_all, uint64_t key_start,
    int64_t* __restrict__ cand_ids, float* __restrict__ cand_prob, int32_t* __restrict__ oob_flag) {
  const int64_t n = n_pos + n_neg;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
    int64_t id;
    if (j < n_pos) {
      id = pos_ids[j];
    } else {
      const uint64_t x = tt::splitmix(key_start + (uint64_t)(j - n_pos));
      const uint64_t b = ((x >> 32) * n_items) >> 32;                          // fill_ids_kernel's uniform id
      id = (int64_t)b;
      if (sampler == TT_SAMPLER_ALIAS) {
        const float u = __fmul_rn((float)(uint32_t)(x & 0xFFFFFFull), 5.9604644775390625e-08f);   // * 2^-24, exact
        if (!(u < alias_thr[b])) id = (int64_t)alias_idx[b];
      }
    }
    // a bad positive id is copied through (the lookups report it too); a bad alias entry is caught the same way, so that the
    // probability vectors are never read out of range
    const bool ok = id >= 0 && (uint64_t)id < n_items;
    if (!ok && oob_flag != nullptr) atomicOr(oob_flag, 1);
    cand_ids[j] = id;
    if (item_freq != nullptr) {
      float p = 1.0f;
      if (ok) {
        const float u_id = sampler_prob != nullptr ? sampler_prob[id] : uniform_prob;
        p = __fdiv_rn(__fadd_rn(__fmul_rn(f_pos, item_freq[id]), __fmul_rn(f_neg, u_id)), f_all);
      }
      cand_prob[j] = p;
    }
  }
}

}  // namespace

extern "C" int tt_sample_candidates_i64(const int64_t* pos_ids, int64_t n_pos, int64_t n_items, int64_t n_neg, int32_t sampler,
                                        const float* alias_thr, const int32_t* alias_idx, const float* item_freq,
                                        const float* sampler_prob, uint64_t seed, uint64_t tensor_id, uint64_t start,
                                        int64_t* cand_ids, float* cand_prob, int32_t* oob_flag, tt_stream_t stream) {
  const char* what = "tt_sample_candidates_i64";
  TT_REQUIRE(n_items >= 1 && n_items <= (int64_t)1 << 32, "%s: n_items must be in 1..2^32 (got %lld)", what, (long long)n_items);
  TT_REQUIRE(n_pos >= 0 && n_neg >= 0, "%s: n_pos and n_neg must be >= 0 (got %lld, %lld)", what, (long long)n_pos,
             (long long)n_neg);
  TT_REQUIRE(n_pos <= 0x7fffffff && n_neg <= 0x7fffffff && n_pos + n_neg >= 1,
             "%s: n_pos + n_neg must be >= 1 and each fit 31 bits (got %lld, %lld)", what, (long long)n_pos, (long long)n_neg);
  TT_REQUIRE(sampler == TT_SAMPLER_UNIFORM || sampler == TT_SAMPLER_ALIAS, "%s: unknown sampler %d", what, sampler);
  if (sampler == TT_SAMPLER_ALIAS) {
    TT_REQUIRE(alias_thr != nullptr && alias_idx != nullptr, "%s: the alias sampler needs alias_thr and alias_idx", what);
    TT_REQUIRE(n_items < (int64_t)1 << 31, "%s: the alias sampler needs n_items < 2^31 (alias_idx is int32)", what);
  }
  TT_REQUIRE(sampler_prob == nullptr || item_freq != nullptr, "%s: sampler_prob without item_freq", what);
  TT_REQUIRE(cand_ids != nullptr && (pos_ids != nullptr || n_pos == 0), "%s: null pointer (pos_ids / cand_ids)", what);
  TT_REQUIRE(item_freq == nullptr || cand_prob != nullptr, "%s: item_freq needs cand_prob", what);
  const int64_t n = n_pos + n_neg;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 256 * 8) blocks = 256 * 8;                                      // 8 blocks per CU, grid-stride the rest
  const float uniform_prob = 1.0f / (float)n_items;
  tt::launch("sample", sample_candidates_kernel, dim3((unsigned)blocks), dim3(256), 0, tt::as_stream(stream), pos_ids, n_pos, n_neg,
             (uint64_t)n_items, (int)sampler, alias_thr, alias_idx, item_freq, sampler_prob, uniform_prob, (float)n_pos, (float)n_neg,
             (float)n, tt::stream_key(seed, tensor_id) + start, cand_ids, cand_prob, oob_flag);
  return tt::check_launch(what);
}
