// playout.hip — hb_rule_playout (include/hanabi_hip_playout.h): games of rule-list teams played from their state rows to the end
// in one launch. It replaces the per-turn loop hb_rule_act -> hb_env_step_packed -> hb_eval_tally for teams that read no
// observation, and computes what that loop computes, bit for bit.
//
// One lane per game: a 64-lane wavefront copies its 64 rows HBM -> LDS once (16-byte coalesced loads, row stride SW + 1 words so
// that lane-per-game accesses are bank-conflict free), every lane then plays its game on its own LDS row, and the wavefront copies
// the rows back. A turn is the rule walk (rule_walk.hpp: the code of hb_rule_act), the rules phase of the env step
// (env_kernel.hpp: env_wave_step with RULES, phases 2a and the scalar words of 2c, nothing encoded) and the tally of one game
// (eval_tally.hpp: the code of hb_eval_tally) on registers. The counters follow hb_eval_tally's pattern — ballots per wavefront
// into the workgroup's LDS copy every turn — but reach HBM once, at the end: one atomic per non-zero counter and workgroup.
//
// The turn loop is a plain for bounded by the caller's max_turns (checked on the host); a wavefront leaves it when none of its
// games is running. Wavefronts share nothing but the LDS counters, whose two workgroup barriers every wavefront reaches; nothing
// waits on another workgroup. Lanes of a wavefront diverge (different rules fire, games end on different turns): that is the price
// of the design, measured in DESIGN.md.
#include <hip/hip_runtime.h>

#include "../../include/hanabi_hip_playout.h"
#include "common.hpp"
#include "env_kernel.hpp"
#include "eval_tally.hpp"
#include "rule_walk.hpp"

namespace {

constexpr int kMaxPlayers = 5;

struct PlayArgs {
  uint32_t* rows;
  long long n, first_gid;
  unsigned long long seed;
  int first_seat, max_turns;
  const int32_t* first_moves;
  uint8_t* done;
  int8_t* final_score;
  int16_t* length;
  unsigned long long* counters;
  int32_t* log;
  unsigned long long* illegal;
  int32_t* max_len;
  int n_rules[kMaxPlayers];
  hb_rule rules[kMaxPlayers][HB_MAX_RULES];
};

// what HB_RULE_WALK reads of its argument block: the game's dimensions (compile-time here) and the Philox key of this turn
template <class K>
struct WalkArgs {
  static constexpr int P = K::P, C = K::C, R = K::R, H = K::H, INFO = K::INFO, CPC = K::CPC;
  unsigned long long seed, draw;
};

// what the tally does on the turn a game ends, and after a misplay that does not end it (HB_TALLY_GAME): the lane's registers
#define PLAY_FINISH(SC, LEN, ST) \
  fs = (SC);                     \
  len = (LEN);                   \
  status = (ST)
#define PLAY_SET_DONE(ST) status = (ST)

constexpr int GW = 64;   // games per wavefront: one per lane

template <class K>
__global__ __launch_bounds__(256) void playout_kernel(const PlayArgs a) {
  constexpr int B = K::C * K::R + 1, NC = 2 + B + 5 * K::P;   // hb_eval_counters(cfg)
  constexpr int Q = K::SW / 4;                                // 16-byte pieces of a row
  __shared__ uint32_t lds[4 * GW * K::SWP];
  __shared__ unsigned int lc[NC + 2];   // hb_eval_tally's counters, then: illegal moves, longest game
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long long g0 = (static_cast<long long>(blockIdx.x) * 4 + wave) * GW;
  uint32_t* const srow = lds + wave * (GW * K::SWP);
  for (int i = threadIdx.x; i < NC + 2; i += 256) lc[i] = 0;
  __syncthreads();

  const long long left = a.n - g0;
  const int nvalid = left <= 0 ? 0 : (left < GW ? static_cast<int>(left) : GW);
  if (nvalid > 0) {   // (wave-uniform)
    {  // rows HBM -> LDS: every 16-byte piece requested before the first is written (env_wave_step, phase 1)
      const uint4* src = reinterpret_cast<const uint4*>(a.rows + g0 * K::SW);
      uint4 v[Q];
#pragma unroll
      for (int r = 0; r < Q; ++r) {
        const int e = lane + 64 * r;
        v[r] = e < nvalid * Q ? src[e] : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int r = 0; r < Q; ++r) {
        const int e = lane + 64 * r;
        if (e < nvalid * Q) {
          const int g = e / Q, q = e - g * Q;
          uint32_t* d = srow + g * K::SWP + 4 * q;
          d[0] = v[r].x; d[1] = v[r].y; d[2] = v[r].z; d[3] = v[r].w;
        }
      }
    }
    const bool mine = lane < nvalid;
    const long long gi = g0 + lane;
    uint8_t status = mine ? a.done[gi] : static_cast<uint8_t>(0x80);
    const bool played = !(status & 0x80u);   // bit 7 at entry: a slot that is not played (its row stays as it is)
    const int first = (played && a.first_moves) ? a.first_moves[gi] : 0;
    int8_t fs = 0;
    int16_t len = 0;
    int n_illegal = 0;
    hb::EnvArgs ea{};
    ea.n = a.n;
    ea.mode = hb::MODE_STEP;
    ea.flags = 0;   // auto-reset off, no leniency
    hb::wave_sync();

    int t = 0;
    for (; t < a.max_turns; ++t) {
      const bool live = !(status & 0x80u);
      if (!__ballot(live)) break;   // (wave-uniform) every game of this wavefront is finished
      int seat = a.first_seat + t % K::P;
      if (seat >= K::P) seat -= K::P;
      int uid = first;
      if (t > 0 || !a.first_moves) {
        if (live) {
          const WalkArgs<K> wa{a.seed, static_cast<unsigned long long>(t) + 1ull};
          HB_RULE_WALK(wa, srow + lane * K::SWP, a.first_gid + gi, a.n_rules[seat], a.rules[seat])
          (void)fired;
          uid = act;
        }
      }
      hb::StepResult sr;
      sr.play = live;
      hb::env_wave_step<K, GW, false, true>(ea, g0, lane, srow, uid, 0, &sr);
      HB_TALLY_VARS
      if (live) {
        HB_TALLY_GAME(K::A, K::H, K::P, K::C, B, K::LIFE, t, status, uid, sr.reward, sr.terminal, sr.score, PLAY_FINISH, PLAY_SET_DONE)
        n_illegal += sr.illegal ? 1 : 0;
      }
      HB_TALLY_WAVE(lc, B, K::P, seat, lane)
      if (a.log && mine) a.log[static_cast<long long>(t) * a.n + gi] = live ? uid : -1;
    }
    if (a.log && mine)
      for (; t < a.max_turns; ++t) a.log[static_cast<long long>(t) * a.n + gi] = -1;

    // per-game results: only of the games played here (the others' bytes are the caller's)
    if (mine && played) {
      a.done[gi] = status;
      if (status & 0x80u) {
        a.final_score[gi] = fs;
        a.length[gi] = len;
      }
    }
    int longest = len, bad = n_illegal;
    for (int o = 32; o > 0; o >>= 1) {
      longest = max(longest, __shfl_xor(longest, o));
      bad += __shfl_xor(bad, o);
    }
    if (lane == 0) {
      if (bad) atomicAdd(lc + NC, static_cast<unsigned int>(bad));
      if (longest) atomicMax(lc + NC + 1, static_cast<unsigned int>(longest));
    }
    hb::wave_sync();
    {  // rows LDS -> HBM, full-width coalesced stores (env_wave_step, phase 3); a row that was not played is unchanged
      uint4* dst = reinterpret_cast<uint4*>(a.rows + g0 * K::SW);
      for (int e = lane; e < nvalid * Q; e += 64) {
        const int g = e / Q, q = e - g * Q;
        const uint32_t* s = srow + g * K::SWP + 4 * q;
        uint4 v;
        v.x = s[0]; v.y = s[1]; v.z = s[2]; v.w = s[3];
        dst[e] = v;
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NC + 2; i += 256) {
    const unsigned int v = lc[i];
    if (!v) continue;
    if (i < NC)
      atomicAdd(a.counters + i, i == 0 ? static_cast<unsigned long long>(-static_cast<long long>(v)) : static_cast<unsigned long long>(v));
    else if (i == NC)
      atomicAdd(a.illegal, static_cast<unsigned long long>(v));
    else
      atomicMax(a.max_len, static_cast<int32_t>(v));
  }
}

template <class K>
void launch_playout(const PlayArgs& a, hipStream_t stream) {
  const unsigned blocks = static_cast<unsigned>((a.n + 4 * GW - 1) / (4 * GW));
  hipLaunchKernelGGL((playout_kernel<K>), dim3(blocks), dim3(256), 0, stream, a);
}

struct PlayVariant {
  int P, C, R, H, INFO, LIFE, D;
  void (*launch)(const PlayArgs&, hipStream_t);
};
template <class K>
constexpr PlayVariant variant() {
  return PlayVariant{K::P, K::C, K::R, K::H, K::INFO, K::LIFE, K::D, &launch_playout<K>};
}
using hb::Cfg;
// the configurations the env is compiled for (env_full / env_small / env_vsmall.hip)
const PlayVariant k_variants[] = {
    variant<Cfg<2, 5, 5, 5, 8, 3>>(), variant<Cfg<3, 5, 5, 5, 8, 3>>(), variant<Cfg<4, 5, 5, 4, 8, 3>>(), variant<Cfg<5, 5, 5, 4, 8, 3>>(),
    variant<Cfg<2, 2, 5, 2, 3, 1>>(), variant<Cfg<3, 2, 5, 2, 3, 1>>(), variant<Cfg<4, 2, 5, 2, 3, 1>>(), variant<Cfg<5, 2, 5, 2, 3, 1>>(),
    variant<Cfg<2, 1, 5, 2, 3, 1>>(), variant<Cfg<3, 1, 5, 2, 3, 1>>(), variant<Cfg<4, 1, 5, 2, 3, 1>>(), variant<Cfg<5, 1, 5, 2, 3, 1>>(),
};

int have_device() {
  static const int ndev = [] {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
  }();
  return ndev > 0 ? HB_OK : hb::fail(HB_ERR_NO_DEVICE, "no HIP device available");
}

}  // namespace

extern "C" int hb_rule_playout(const hb_config* cfg, uint32_t* rows_dev, int64_t n, int64_t first_game_id, const hb_rule* const* rules,
                               const int32_t* n_rules, uint64_t seed, int32_t first_seat, const int32_t* first_moves_dev,
                               int32_t max_turns, uint8_t* done_dev, int8_t* final_score_dev, int16_t* length_dev,
                               int64_t* counters_dev, int32_t* actions_log_dev, int64_t* illegal_dev, int32_t* max_len_dev,
                               void* stream) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  const PlayVariant* var = nullptr;
  for (const PlayVariant& v : k_variants)
    if (v.P == cfg->players && v.C == cfg->colors && v.R == cfg->ranks && v.H == cfg->hand_size && v.INFO == cfg->max_info &&
        v.LIFE == cfg->max_life)
      var = &v;
  if (!var)
    return hb::fail(HB_ERR_INVALID,
                    "no compiled kernel for players=%d colors=%d ranks=%d hand=%d info=%d life=%d "
                    "(built: Hanabi-Full / -Small / -Very-Small, 2..5 players)",
                    cfg->players, cfg->colors, cfg->ranks, cfg->hand_size, cfg->max_info, cfg->max_life);
  if (!rows_dev) return hb::fail(HB_ERR_INVALID, "null rows_dev");
  if (!counters_dev) return hb::fail(HB_ERR_INVALID, "null counters_dev");
  if (!done_dev || !final_score_dev || !length_dev || !illegal_dev || !max_len_dev)
    return hb::fail(HB_ERR_INVALID, "null argument: done_dev, final_score_dev, length_dev, illegal_dev and max_len_dev are required");
  if (!rules || !n_rules) return hb::fail(HB_ERR_INVALID, "null rules: one rule list and its length per seat");
  if (n < 0 || n > (int64_t{1} << 31)) return hb::fail(HB_ERR_INVALID, "n must be 0..2^31: split the call");
  const int P = cfg->players;
  for (int p = 0; p < P; ++p) {
    if (n_rules[p] < 0 || n_rules[p] > HB_MAX_RULES) return hb::fail(HB_ERR_INVALID, "seat %d: n_rules must be 0..%d", p, HB_MAX_RULES);
    if (n_rules[p] > 0 && !rules[p]) return hb::fail(HB_ERR_INVALID, "seat %d: null rules", p);
    for (int i = 0; i < n_rules[p]; ++i)
      if (rules[p][i].kind < 0 || rules[p][i].kind >= HB_RULE_KINDS)
        return hb::fail(HB_ERR_INVALID, "seat %d, rule %d: unknown kind %d", p, i, rules[p][i].kind);
  }
  if (first_seat < 0 || first_seat >= P) return hb::fail(HB_ERR_INVALID, "first_seat %d out of range for %d players", first_seat, P);
  // no game is longer (hanabi_hip.evaluate.max_turns): draws discards / plays, INFO + draws + C hints, P turns after the last card
  const int draws = var->D - P * var->H;
  const int bound = draws + (var->INFO + draws + var->C) + P;
  if (max_turns < 1 || max_turns > bound) return hb::fail(HB_ERR_INVALID, "max_turns %d out of range 1..%d", max_turns, bound);
  if (reinterpret_cast<uintptr_t>(rows_dev) & 15) return hb::fail(HB_ERR_ALIGN, "rows_dev must be 16-byte aligned");
  if (n == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  PlayArgs a{};
  a.rows = rows_dev;
  a.n = n;
  a.first_gid = first_game_id;
  a.seed = seed;
  a.first_seat = first_seat;
  a.max_turns = max_turns;
  a.first_moves = first_moves_dev;
  a.done = done_dev;
  a.final_score = final_score_dev;
  a.length = length_dev;
  a.counters = reinterpret_cast<unsigned long long*>(counters_dev);
  a.log = actions_log_dev;
  a.illegal = reinterpret_cast<unsigned long long*>(illegal_dev);
  a.max_len = max_len_dev;
  for (int p = 0; p < P; ++p) {
    a.n_rules[p] = n_rules[p];
    for (int i = 0; i < n_rules[p]; ++i) a.rules[p][i] = rules[p][i];
  }
  var->launch(a, static_cast<hipStream_t>(stream));
  HB_HIP(hipGetLastError());
  return HB_OK;
}
