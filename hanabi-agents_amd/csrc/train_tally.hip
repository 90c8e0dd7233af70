// train_tally.hip — per-partner statistics of a training run against a partner pool (hb_train_tally): issued once per env step,
// after the step, on the same stream. The env auto-resets, so unlike hb_eval_tally (eval.hip) every terminal counts and a
// game's tally state (lives lost, moves played) restarts at each deal. Row g of the env belongs to the pool member that owns its
// 128-game tile (tile_member_dev[g / 128]), and the counters of that member get what the row did.
//
// One lane per game; a 64-lane wave lies inside one 128-row tile, so its member is wave-uniform. Every counter is reduced
// inside the wave first (__ballot), then inside the workgroup (LDS, one row of counters per member), and added to HBM with
// ONE integer atomic per workgroup, member and counter from at most 128 workgroups (as eval.hip: thousands of atomics on one
// address cost ~12 ns each). Integer adds keep every count exact and independent of the order of the atomics.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/hanabi_hip.h"
#include "common.hpp"

namespace {

constexpr int kTile = 128;                                        // rows per pool tile
constexpr int kMaxBlocks = 128;                                   // at most this many global atomics per counter and step
constexpr uint8_t kUnarmed = 0x80;                                // lost byte: the game's deal was not seen, lengths / lives unknown

struct TrainTallyArgs {
  long long n;
  int P, H, C, A, max_life, seat, bins, nc, n_members;
  const int32_t* actions;
  const float* reward;
  const int8_t* terminal;
  const int8_t* score;
  const int32_t* tile_member;
  uint8_t* lost;
  int16_t* length;
  unsigned long long* counters;
};

__device__ __forceinline__ void wave_add(unsigned int* c, unsigned long long mask, int lane) {
  if (mask && lane == 0) atomicAdd(c, static_cast<unsigned int>(__popcll(mask)));
}

// Counter row of one member (hb_train_counters): [0] episodes, [1] score sum, [2] score^2 sum, [3, 3 + B) histogram,
// [3 + B] bomb-outs, [4 + B] length sum, [5 + B] episodes whose deal was seen, [6 + B + 4 p + k] moves, [6 + B + 4 P + p] misplays.
__global__ void __launch_bounds__(256) train_tally_kernel(TrainTallyArgs a) {
  extern __shared__ unsigned int lc[];   // [n_members][nc]
  const int lane = threadIdx.x & 63;
  const int B = a.bins, nc = a.nc, total = a.n_members * nc;
  for (int i = threadIdx.x; i < total; i += 256) lc[i] = 0;
  __syncthreads();
  for (long long base = static_cast<long long>(blockIdx.x) * 256; base < a.n; base += static_cast<long long>(gridDim.x) * 256) {
    const long long g = base + threadIdx.x;
    // (n is a multiple of 128: a wave is either wholly inside the rows or wholly past them)
    if (base + (threadIdx.x & ~63) >= a.n) continue;
    const int member = a.tile_member[g / kTile];
    if (member < 0 || member >= a.n_members) continue;   // (wave-uniform: one tile)
    unsigned int* m = lc + member * nc;
    const int u = a.actions[g];
    const int kind = (u >= 0 && u < a.A) ? (u < a.H ? 0 : u < 2 * a.H ? 1 : u < 2 * a.H + (a.P - 1) * a.C ? 2 : 3) : -1;   // App. A.2
    const bool misplay = kind == 1 && a.reward[g] <= 0.f;   // a successful play always scores +1; a misplay 0, or -score at a bomb-out
    const bool ended = a.terminal[g] != 0;
    const uint8_t st = a.lost[g];
    const bool armed = !(st & kUnarmed);
    const int lost = (st & 0x7f) + (misplay ? 1 : 0);
    const int len = a.length[g] + 1;
    int bin = 0;
    bool bomb = false, tracked = false;
    if (ended) {
      const int sc = a.score[g];   // 0 after a bomb-out (hb_env_step), as the env's own episode statistics count it
      bin = sc < 0 ? 0 : sc > B - 1 ? B - 1 : sc;
      tracked = armed;
      bomb = armed && lost >= a.max_life;
      a.lost[g] = 0;      // the next deal is already in the row (auto-reset): tracked from its first move on
      a.length[g] = 0;
    } else if (armed) {
      a.lost[g] = static_cast<uint8_t>(lost);
      a.length[g] = static_cast<int16_t>(len);
    }
    unsigned long long em = __ballot(ended);
    if (em) {
      wave_add(m, em, lane);
      wave_add(m + 3 + B, __ballot(bomb), lane);
      wave_add(m + 5 + B, __ballot(tracked), lane);
      // length sum: the wave's sum of the tracked games' lengths (<= 64 * 32767, fits 32 bits)
      int ls = tracked ? len : 0;
      for (int o = 32; o > 0; o >>= 1) ls += __shfl_xor(ls, o);
      if (lane == 0 && ls) atomicAdd(m + 4 + B, static_cast<unsigned int>(ls));
      while (em) {   // histogram, score and score^2 sums: one ballot per score that occurs in this wave (wave-uniform loop)
        const int b = __shfl(bin, __ffsll(static_cast<unsigned long long>(em)) - 1);
        const unsigned long long mb = __ballot(ended && bin == b);
        if (lane == 0) {
          const unsigned int c = static_cast<unsigned int>(__popcll(mb));
          atomicAdd(m + 3 + b, c);
          if (b) {
            atomicAdd(m + 1, c * static_cast<unsigned int>(b));
            atomicAdd(m + 2, c * static_cast<unsigned int>(b * b));
          }
        }
        em &= ~mb;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) wave_add(m + 6 + B + 4 * a.seat + k, __ballot(kind == k), lane);
    wave_add(m + 6 + B + 4 * a.P + a.seat, __ballot(misplay), lane);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += 256) {
    const unsigned int v = lc[i];
    if (v) atomicAdd(a.counters + i, static_cast<unsigned long long>(v));
  }
}

// hb_train_tally_init: a game is armed (lost = 0, length = 0) when its state row is at the first move of its deal, else unarmed.
// A fresh deal has every information token, no firework, an empty discard pile and the deck less the hands; every first move
// changes one of them (a hint spends a token, a play or discard draws a card).
__global__ void __launch_bounds__(256) train_tally_init_kernel(const uint32_t* rows, long long n, int SW, int INFO, int deck0,
                                                                uint8_t* lost, int16_t* length) {
  const long long g = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (g >= n) return;
  const uint32_t* row = rows + g * SW;
  const uint32_t w0 = row[0], w1 = row[1];
  const bool dealt = static_cast<int>(w0 & 63) == deck0 && static_cast<int>((w0 >> 6) & 15) == INFO && (w1 & 0x7FFFu) == 0 &&
                     row[8] == 0 && row[9] == 0;
  lost[g] = dealt ? 0 : kUnarmed;
  length[g] = 0;
}

int have_device() {
  static const int ndev = [] {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
  }();
  return ndev > 0 ? HB_OK : hb::fail(HB_ERR_NO_DEVICE, "no HIP device available");
}

}  // namespace

extern "C" int hb_train_counters(const hb_config* cfg) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  return 6 + cfg->colors * cfg->ranks + 1 + 5 * cfg->players;
}

extern "C" int hb_train_tally_init(const hb_config* cfg, const uint32_t* state_rows_dev, int64_t n_games, uint8_t* lost_dev,
                                   int16_t* length_dev, void* stream) {
  if (!cfg || !state_rows_dev || !lost_dev || !length_dev) return hb::fail(HB_ERR_INVALID, "null argument");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (n_games < 0) return hb::fail(HB_ERR_INVALID, "n_games must be >= 0");
  if (n_games == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  const unsigned blocks = static_cast<unsigned>((n_games + 255) / 256);
  hipLaunchKernelGGL(train_tally_init_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), state_rows_dev,
                     static_cast<long long>(n_games), hb_state_words(cfg), cfg->max_info, hb_deck_size(cfg) - cfg->players * cfg->hand_size,
                     lost_dev, length_dev);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

extern "C" int hb_train_tally(const hb_config* cfg, int64_t n_games, int32_t seat, const int32_t* actions_dev, const float* reward_dev,
                              const int8_t* terminal_dev, const int8_t* score_dev, const int32_t* tile_member_dev, int32_t n_members,
                              uint8_t* lost_dev, int16_t* length_dev, int64_t* counters_dev, void* stream) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (n_games < 0 || n_games % kTile != 0) return hb::fail(HB_ERR_INVALID, "n_games must be a non-negative multiple of %d", kTile);
  if (seat < 0 || seat >= cfg->players) return hb::fail(HB_ERR_INVALID, "seat %d out of range for %d players", seat, cfg->players);
  if (n_members < 1 || n_members > HB_TRAIN_MAX_MEMBERS)
    return hb::fail(HB_ERR_INVALID, "n_members must be 1..%d", HB_TRAIN_MAX_MEMBERS);
  if (!actions_dev || !reward_dev || !terminal_dev || !score_dev || !tile_member_dev || !lost_dev || !length_dev || !counters_dev)
    return hb::fail(HB_ERR_INVALID, "null argument");
  if (n_games == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  TrainTallyArgs a{};
  a.n = n_games;
  a.P = cfg->players; a.H = cfg->hand_size; a.C = cfg->colors;
  a.A = hb_num_actions(cfg);
  a.max_life = cfg->max_life;
  a.seat = seat;
  a.bins = cfg->colors * cfg->ranks + 1;
  a.nc = hb_train_counters(cfg);
  a.n_members = n_members;
  a.actions = actions_dev; a.reward = reward_dev; a.terminal = terminal_dev; a.score = score_dev;
  a.tile_member = tile_member_dev;
  a.lost = lost_dev; a.length = length_dev;
  a.counters = reinterpret_cast<unsigned long long*>(counters_dev);
  const unsigned blocks = static_cast<unsigned>(std::min<int64_t>((n_games + 255) / 256, kMaxBlocks));
  const size_t lds = sizeof(unsigned int) * static_cast<size_t>(n_members) * a.nc;
  hipLaunchKernelGGL(train_tally_kernel, dim3(blocks), dim3(256), lds, static_cast<hipStream_t>(stream), a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}
