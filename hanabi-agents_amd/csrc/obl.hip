// obl.hip — off-belief learning (hanabi_hip/obl.py): whole replay transitions from a fictitious branch.
//
// hb_obl_insert: row g of the batch -> ring slot (start + g) mod capacity. The branch was played for n_steps = P moves (the
// learner's own, then every partner's); e = the first step whose terminal flag is set, or P:
//   ring_obs_tm1 <- obs_tm1, ring_act <- actions, ring_rew <- rewards[0] + ... + rewards[min(e, P - 1)] (fp32, ascending),
//   ring_term <- (e < P), ring_obs_t / ring_lms <- obs_t / legal_t where e == P, zeros otherwise.
// One launch, grid-stride: a lane takes one 16-byte chunk of one row (the chunks of a row sit on neighbouring lanes, rows follow
// each other: coalesced; rows are row_bytes apart, so no side is more than byte-aligned: unaligned dwordx4 accesses, one
// instruction on gfx950, as in replay_insert_kernel of policy.hip), the row_bytes % 16 tail goes bytewise. The lanes of a row
// each read its <= 5 terminal flags (one byte per step, the same address across the row's lanes). No LDS, no atomics, no barrier.
#include <hip/hip_runtime.h>

#include "../../include/hanabi_hip.h"
#include "common.hpp"

using hb::fail;

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));  // byte-aligned 16-byte access: one dwordx4 instruction on gfx950

constexpr int MAX_STEPS = 5;

struct OblArgs {
  const int8_t* obs_tm1;    // [n, L]
  const int32_t* actions;   // [n]
  const float* rewards;     // [S, n]
  const int8_t* terminal;   // [S, n]
  const int8_t* obs_t;      // [n, L]
  const int8_t* legal_t;    // [n, A]
  int8_t* ring_obs_tm1;     // [cap, L]
  int8_t* ring_obs_t;       // [cap, L]
  int8_t* ring_act;         // [cap]
  int8_t* ring_lms;         // [cap, A]
  float* ring_rew;          // [cap]
  uint8_t* ring_term;       // [cap] (bool)
  long long n, cap, start;
  int L, A, S;
};

// first step with a terminal flag, S when there is none
__device__ __forceinline__ int end_step(const OblArgs& a, long long g) {
  int e = a.S;
#pragma unroll
  for (int k = MAX_STEPS - 1; k >= 0; --k)
    if (k < a.S && a.terminal[k * a.n + g] != 0) e = k;
  return e;
}

__device__ __forceinline__ long long slot_of(const OblArgs& a, long long g) {
  const long long s = a.start + g;
  return s >= a.cap ? s - a.cap : s;
}

// chunk c of [n, bytes]-rows: (row, 16-byte piece); `live` false writes zeros. d0 may be null (nothing to copy unconditionally).
__device__ __forceinline__ void row_chunk(const OblArgs& a, long long c, int cpr, int bytes, const int8_t* __restrict__ src0,
                                          int8_t* __restrict__ d0, const int8_t* __restrict__ src1, int8_t* __restrict__ d1) {
  const long long g = c / cpr;
  const int off = static_cast<int>(c - g * cpr) << 4;
  const long long slot = slot_of(a, g);
  const bool live = end_step(a, g) == a.S;
  const long long in = g * bytes + off, out = slot * bytes + off;
  if (off + 16 <= bytes) {
    if (d0) *reinterpret_cast<u32x4_u*>(d0 + out) = *reinterpret_cast<const u32x4_u*>(src0 + in);
    u32x4 v = {0u, 0u, 0u, 0u};
    if (live) v = *reinterpret_cast<const u32x4_u*>(src1 + in);
    *reinterpret_cast<u32x4_u*>(d1 + out) = v;
  } else {
    for (int b = 0; off + b < bytes; ++b) {
      if (d0) d0[out + b] = src0[in + b];
      d1[out + b] = live ? src1[in + b] : static_cast<int8_t>(0);
    }
  }
}

__global__ __launch_bounds__(256) void obl_insert_kernel(const OblArgs a) {
  const long long tid = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const long long nthreads = static_cast<long long>(gridDim.x) * blockDim.x;
  const int cpr = (a.L + 15) >> 4, cpl = (a.A + 15) >> 4;
  for (long long c = tid; c < a.n * cpr; c += nthreads) row_chunk(a, c, cpr, a.L, a.obs_tm1, a.ring_obs_tm1, a.obs_t, a.ring_obs_t);
  for (long long c = tid; c < a.n * cpl; c += nthreads) row_chunk(a, c, cpl, a.A, nullptr, nullptr, a.legal_t, a.ring_lms);
  for (long long g = tid; g < a.n; g += nthreads) {
    const int e = end_step(a, g);
    const int last = e < a.S - 1 ? e : a.S - 1;
    float r = a.rewards[g];
    for (int k = 1; k <= last; ++k) r += a.rewards[k * a.n + g];
    const long long slot = slot_of(a, g);
    a.ring_act[slot] = static_cast<int8_t>(a.actions[g]);
    a.ring_rew[slot] = r;
    a.ring_term[slot] = e < a.S;
  }
}

}  // namespace

extern "C" {

int hb_obl_insert(const int8_t* obs_tm1_dev, const int32_t* actions_dev, const float* rewards_dev, const int8_t* terminal_dev,
                  const int8_t* obs_t_dev, const int8_t* legal_t_dev, int8_t* ring_obs_tm1_dev, int8_t* ring_obs_t_dev,
                  int8_t* ring_act_dev, int8_t* ring_lms_dev, float* ring_rew_dev, uint8_t* ring_term_dev, int64_t n,
                  int32_t n_steps, int32_t row_bytes, int32_t n_actions, int64_t capacity, int64_t start, void* stream) {
  if (!obs_tm1_dev || !actions_dev || !rewards_dev || !terminal_dev || !obs_t_dev || !legal_t_dev || !ring_obs_tm1_dev ||
      !ring_obs_t_dev || !ring_act_dev || !ring_lms_dev || !ring_rew_dev || !ring_term_dev)
    return fail(HB_ERR_INVALID, "null argument");
  if (n < 0) return fail(HB_ERR_INVALID, "n must be >= 0");
  if (n_steps < 1 || n_steps > MAX_STEPS) return fail(HB_ERR_INVALID, "n_steps must be 1..5 (one per player)");
  if (capacity <= 0) return fail(HB_ERR_INVALID, "capacity must be positive");
  if (row_bytes <= 0) return fail(HB_ERR_INVALID, "row_bytes must be positive");
  if (n_actions <= 0) return fail(HB_ERR_INVALID, "n_actions must be positive");
  if (n == 0) return HB_OK;
  if (n > capacity || start < 0 || start >= capacity) return fail(HB_ERR_INVALID, "bad ring range");
  OblArgs a{obs_tm1_dev, actions_dev, rewards_dev, terminal_dev, obs_t_dev, legal_t_dev, ring_obs_tm1_dev, ring_obs_t_dev,
            ring_act_dev, ring_lms_dev, ring_rew_dev, ring_term_dev, n, capacity, start, row_bytes, n_actions, n_steps};
  const long long chunks = n * ((row_bytes + 15) >> 4);
  long long blocks = (chunks + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(obl_insert_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

}  // extern "C"
