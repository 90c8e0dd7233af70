// eval.hip — the evaluation tally (hb_eval_tally): issued once per turn after the env step of a fixed set of evaluation
// games (auto-reset off), it records each game's final score and length on the turn it ends and keeps one small block
// of int64 counters — games still live, the score histogram, bomb-outs, per-seat move kinds and misplays — on the
// device, so the host only has to read the live count now and then.
//
// One lane per game. Every counter is reduced inside the wavefront first (__ballot over the 64 lanes), then inside the
// workgroup (LDS), and added to HBM with ONE atomic per workgroup and counter from at most 128 workgroups: thousands of
// atomics on one address cost ~12 ns each (env_kernel.hpp, the episode statistics). Measured: one atomic per wave and
// counter cost 22-25 us per turn at 32 768 games (512 waves on the same few addresses) against 7 us at 4 096.
//
// hb_eval_tally_grouped runs the same kernel over blocks of games, one grid row and one row of counters per block; hb_eval_tally
// is that launch with one grid row. The partner-response counts (hb_eval_response_tally, issued between the env step and the
// tally; grouped in the same way) are at the end of the file.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/hanabi_hip.h"
#include "common.hpp"
#include "eval_tally.hpp"

namespace {

struct TallyArgs {
  long long n;
  int P, C, R, H, A, max_life, seat, turn, bins;
  const int32_t* actions;
  const float* reward;
  const int8_t* terminal;
  const int8_t* score;
  uint8_t* done;
  int8_t* final_score;
  int16_t* length;
  unsigned long long* counters;
};

constexpr int kMaxCounters = 2 + 5 * 5 + 1 + 5 * 5;   // hb_eval_counters() at its largest (5 colours, 5 ranks, 5 players)
constexpr int kMaxBlocks = 128;                        // at most this many global atomics per counter and turn

// what hb_eval_tally does on the turn game g ends, and after a misplay that does not end it (HB_TALLY_GAME, eval_tally.hpp)
#define TALLY_FINISH(SC, LEN, ST) \
  a.final_score[g] = (SC);        \
  a.length[g] = (LEN);            \
  a.done[g] = (ST)
#define TALLY_SET_DONE(ST) a.done[g] = (ST)

// blockIdx.y selects a block of a0.n games and its own row of counters (hb_eval_tally: the one block). Grid-stride over the
// block's games (the loop bound is uniform across the workgroup, so every lane takes part in every ballot). Each wave adds its
// ballot counts into the workgroup's LDS copy of the counters; the workgroup then issues one global atomic per nonzero counter.
__global__ void __launch_bounds__(256) eval_tally_grouped_kernel(TallyArgs a0) {
  const long long off = static_cast<long long>(blockIdx.y) * a0.n;
  TallyArgs a = a0;
  a.actions += off; a.reward += off; a.terminal += off; a.score += off;
  a.done += off; a.final_score += off; a.length += off;
  a.counters += static_cast<long long>(blockIdx.y) * (2 + a0.bins + 5 * a0.P);
  __shared__ unsigned int lc[kMaxCounters];
  const int lane = threadIdx.x & 63;
  const int B = a.bins, nc = 2 + B + 5 * a.P;
  for (int i = threadIdx.x; i < nc; i += 256) lc[i] = 0;
  __syncthreads();
  for (long long base = static_cast<long long>(blockIdx.x) * 256; base < a.n; base += static_cast<long long>(gridDim.x) * 256) {
    const long long g = base + threadIdx.x;
    HB_TALLY_VARS
    if (g < a.n) {
      HB_TALLY_GAME(a.A, a.H, a.P, a.C, B, a.max_life, a.turn, a.done[g], a.actions[g], a.reward[g], a.terminal[g], a.score[g],
                    TALLY_FINISH, TALLY_SET_DONE)
    }
    HB_TALLY_WAVE(lc, B, a.P, a.seat, lane)
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nc; i += 256) {
    const unsigned int v = lc[i];
    if (v) atomicAdd(a.counters + i, i == 0 ? static_cast<unsigned long long>(-static_cast<long long>(v)) : static_cast<unsigned long long>(v));
  }
}

}  // namespace

extern "C" int hb_eval_counters(const hb_config* cfg) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  return 2 + cfg->colors * cfg->ranks + 1 + 5 * cfg->players;
}

namespace {

int check_tally(const hb_config* cfg, int64_t n_games, int32_t seat, int32_t turn, const int32_t* actions_dev, const float* reward_dev,
                const int8_t* terminal_dev, const int8_t* score_dev, uint8_t* done_dev, int8_t* final_score_dev, int16_t* length_dev,
                int64_t* counters_dev) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (n_games < 0) return hb::fail(HB_ERR_INVALID, "n_games must be >= 0");
  if (seat < 0 || seat >= cfg->players) return hb::fail(HB_ERR_INVALID, "seat %d out of range for %d players", seat, cfg->players);
  if (turn < 0 || turn >= 32767) return hb::fail(HB_ERR_INVALID, "turn %d out of range 0..32766 (lengths are int16)", turn);
  if (!actions_dev || !reward_dev || !terminal_dev || !score_dev || !done_dev || !final_score_dev || !length_dev || !counters_dev)
    return hb::fail(HB_ERR_INVALID, "null argument");
  return HB_OK;
}

int have_device() {
  static const int ndev = [] {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
  }();
  return ndev > 0 ? HB_OK : hb::fail(HB_ERR_NO_DEVICE, "no HIP device available");
}

TallyArgs tally_args(const hb_config* cfg, int64_t n_games, int32_t seat, int32_t turn, const int32_t* actions_dev, const float* reward_dev,
                     const int8_t* terminal_dev, const int8_t* score_dev, uint8_t* done_dev, int8_t* final_score_dev, int16_t* length_dev,
                     int64_t* counters_dev) {
  TallyArgs a{};
  a.n = n_games;
  a.P = cfg->players; a.C = cfg->colors; a.R = cfg->ranks; a.H = cfg->hand_size;
  a.A = hb_num_actions(cfg);
  a.max_life = cfg->max_life;
  a.seat = seat;
  a.turn = turn;
  a.bins = cfg->colors * cfg->ranks + 1;
  a.actions = actions_dev; a.reward = reward_dev; a.terminal = terminal_dev; a.score = score_dev;
  a.done = done_dev; a.final_score = final_score_dev; a.length = length_dev;
  a.counters = reinterpret_cast<unsigned long long*>(counters_dev);
  return a;
}

// n_blocks grid rows of at most kMaxBlocks workgroups each over the a.n games of a block
int launch_tally(const TallyArgs& a, int64_t n_blocks, void* stream) {
  const dim3 grid(static_cast<unsigned>(std::min<int64_t>((a.n + 255) / 256, kMaxBlocks)), static_cast<unsigned>(n_blocks));
  hipLaunchKernelGGL(eval_tally_grouped_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

}  // namespace

extern "C" int hb_eval_tally(const hb_config* cfg, int64_t n_games, int32_t seat, int32_t turn, const int32_t* actions_dev,
                             const float* reward_dev, const int8_t* terminal_dev, const int8_t* score_dev, uint8_t* done_dev,
                             int8_t* final_score_dev, int16_t* length_dev, int64_t* counters_dev, void* stream) {
  if (int rc = check_tally(cfg, n_games, seat, turn, actions_dev, reward_dev, terminal_dev, score_dev, done_dev, final_score_dev,
                           length_dev, counters_dev))
    return rc;
  if (n_games == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  return launch_tally(tally_args(cfg, n_games, seat, turn, actions_dev, reward_dev, terminal_dev, score_dev, done_dev, final_score_dev,
                                 length_dev, counters_dev), 1, stream);
}

extern "C" int hb_eval_tally_grouped(const hb_config* cfg, int64_t n_blocks, int64_t block_games, int32_t seat, int32_t turn,
                                     const int32_t* actions_dev, const float* reward_dev, const int8_t* terminal_dev,
                                     const int8_t* score_dev, uint8_t* done_dev, int8_t* final_score_dev, int16_t* length_dev,
                                     int64_t* counters_dev, void* stream) {
  if (int rc = check_tally(cfg, block_games, seat, turn, actions_dev, reward_dev, terminal_dev, score_dev, done_dev, final_score_dev,
                           length_dev, counters_dev))
    return rc;
  if (n_blocks < 0 || n_blocks > 65535) return hb::fail(HB_ERR_INVALID, "n_blocks must be 0..65535 (one grid row per block)");
  if (n_blocks == 0 || block_games == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  return launch_tally(tally_args(cfg, block_games, seat, turn, actions_dev, reward_dev, terminal_dev, score_dev, done_dev,
                                 final_score_dev, length_dev, counters_dev), n_blocks, stream);
}

// ---- partner-response counts (hb_eval_response_tally) -------------------------------------------------------------------------
// Issued once per turn between the env step and that turn's hb_eval_tally: resp[seat][prev + 1][uid] += 1 for every game still live
// (bit 7 of done clear: the tally of this turn has not run yet, so a game's last move is counted), then prev[g] = uid.
//
// One lane per game, grid-stride, at most 128 workgroups per block of games. Each workgroup keeps the (A + 1) * A bins of its seat's
// slab as int32 in LDS (420 bins at 2 players, 2 352 at 5 players; 2 550 = 10.2 KB at the largest valid configuration): zeroed,
// barrier, one LDS add per counted game, barrier, then one 64-bit global atomic per non-zero bin and workgroup. Only the [seat] slab
// is touched. Every sum is an integer sum, so the result does not depend on the order of the adds: it is bit-reproducible.
namespace {

constexpr int kMaxRespBins = 51 * 50;   // (A + 1) * A at A = 2 * 5 + 4 * (5 + 5), the largest hb_num_actions of a valid config

struct RespArgs {
  long long n;
  int P, A, seat;
  const int32_t* actions;
  const uint8_t* done;
  int32_t* prev;
  unsigned long long* resp;
};

// blockIdx.y selects a block of a0.n games and its own [P][A + 1][A] counts (hb_eval_response_tally: the one block)
__global__ void __launch_bounds__(256) eval_response_grouped_kernel(RespArgs a0) {
  const long long off = static_cast<long long>(blockIdx.y) * a0.n;
  RespArgs a = a0;
  a.actions += off; a.done += off; a.prev += off;
  a.resp += static_cast<long long>(blockIdx.y) * a0.P * ((a0.A + 1) * a0.A);
  __shared__ unsigned int hist[kMaxRespBins];
  const int bins = (a.A + 1) * a.A;   // <= kMaxRespBins (checked on the host)
  for (int i = threadIdx.x; i < bins; i += 256) hist[i] = 0;
  __syncthreads();
  for (long long g = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x; g < a.n; g += static_cast<long long>(gridDim.x) * 256) {
    if (a.done[g] & 0x80u) continue;   // finished before this turn: not counted, not written
    const int u = a.actions[g];
    if (u < 0 || u >= a.A) continue;   // not a move: not counted, prev stays
    const int p = a.prev[g];
    if (p >= -1 && p < a.A) atomicAdd(&hist[(p + 1) * a.A + u], 1u);   // (a prev outside -1 .. A-1 is the caller's error: no bin)
    a.prev[g] = u;
  }
  __syncthreads();
  unsigned long long* out = a.resp + static_cast<long long>(a.seat) * bins;
  for (int i = threadIdx.x; i < bins; i += 256) {
    const unsigned int v = hist[i];
    if (v) atomicAdd(out + i, static_cast<unsigned long long>(v));
  }
}

int check_response(const hb_config* cfg, int64_t n_games, int32_t seat, const int32_t* actions_dev, const uint8_t* done_dev,
                   int32_t* prev_dev, int64_t* resp_dev) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (n_games < 0) return hb::fail(HB_ERR_INVALID, "n_games must be >= 0");
  if (seat < 0 || seat >= cfg->players) return hb::fail(HB_ERR_INVALID, "seat %d out of range for %d players", seat, cfg->players);
  if (!actions_dev || !done_dev || !prev_dev || !resp_dev) return hb::fail(HB_ERR_INVALID, "null argument");
  const int A = hb_num_actions(cfg);
  if ((A + 1) * A > kMaxRespBins) return hb::fail(HB_ERR_INVALID, "internal: %d response bins exceed the kernel's %d", (A + 1) * A, kMaxRespBins);
  return HB_OK;
}

RespArgs response_args(const hb_config* cfg, int64_t n_games, int32_t seat, const int32_t* actions_dev, const uint8_t* done_dev,
                       int32_t* prev_dev, int64_t* resp_dev) {
  RespArgs a{};
  a.n = n_games;
  a.P = cfg->players;
  a.A = hb_num_actions(cfg);
  a.seat = seat;
  a.actions = actions_dev; a.done = done_dev; a.prev = prev_dev;
  a.resp = reinterpret_cast<unsigned long long*>(resp_dev);
  return a;
}

// n_blocks grid rows of at most kMaxBlocks workgroups each over the a.n games of a block
int launch_response(const RespArgs& a, int64_t n_blocks, void* stream) {
  const dim3 grid(static_cast<unsigned>(std::min<int64_t>((a.n + 255) / 256, kMaxBlocks)), static_cast<unsigned>(n_blocks));
  hipLaunchKernelGGL(eval_response_grouped_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

}  // namespace

extern "C" int hb_eval_response_bins(const hb_config* cfg) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  const int A = hb_num_actions(cfg);
  return (A + 1) * A;
}

extern "C" int hb_eval_response_tally(const hb_config* cfg, int64_t n_games, int32_t seat, const int32_t* actions_dev,
                                      const uint8_t* done_dev, int32_t* prev_dev, int64_t* resp_dev, void* stream) {
  if (int rc = check_response(cfg, n_games, seat, actions_dev, done_dev, prev_dev, resp_dev)) return rc;
  if (n_games == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  return launch_response(response_args(cfg, n_games, seat, actions_dev, done_dev, prev_dev, resp_dev), 1, stream);
}

extern "C" int hb_eval_response_tally_grouped(const hb_config* cfg, int64_t n_blocks, int64_t block_games, int32_t seat,
                                              const int32_t* actions_dev, const uint8_t* done_dev, int32_t* prev_dev, int64_t* resp_dev,
                                              void* stream) {
  if (int rc = check_response(cfg, block_games, seat, actions_dev, done_dev, prev_dev, resp_dev)) return rc;
  if (n_blocks < 0 || n_blocks > 65535) return hb::fail(HB_ERR_INVALID, "n_blocks must be 0..65535 (one grid row per block)");
  if (block_games >= (int64_t{1} << 31) || n_blocks * block_games >= (int64_t{1} << 31))
    return hb::fail(HB_ERR_INVALID, "n_blocks * block_games must be < 2^31");
  if (n_blocks == 0 || block_games == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  return launch_response(response_args(cfg, block_games, seat, actions_dev, done_dev, prev_dev, resp_dev), n_blocks, stream);
}
