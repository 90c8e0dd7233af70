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
//
// hb_rule_playout_grouped is the same for blocks of games with one team per block (playout_grouped_kernel): the rule lists come
// from device tables through an LDS copy per workgroup, the counters go to the block's own row.
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

// One wavefront's games from the copy in to the copy out, and the workgroup's counters to HBM: the bodies of playout_kernel and
// playout_grouped_kernel. Macros for the reason HB_RULE_WALK is one: playout_kernel expands to exactly the code it was written as.
// They read the enclosing kernel's a (rows, n, seed, first_seat, max_turns, first_moves, done, final_score, length, log,
// illegal), g0 (the wavefront's first game in those arrays), nvalid, lane, srow and lc. GID: the Philox game id of the lane's
// game (may name gi = g0 + lane); N_RULES / RULES: the list of `seat`, read uniformly.
#define PLAY_WAVE(GID, N_RULES, RULES)                                                                                                 \
  {  /* rows HBM -> LDS: every 16-byte piece requested before the first is written (env_wave_step, phase 1) */                         \
    const uint4* src = reinterpret_cast<const uint4*>(a.rows + g0 * K::SW);                                                            \
    uint4 v[Q];                                                                                                                        \
    _Pragma("unroll")                                                                                                                  \
    for (int r = 0; r < Q; ++r) {                                                                                                      \
      const int e = lane + 64 * r;                                                                                                     \
      v[r] = e < nvalid * Q ? src[e] : make_uint4(0u, 0u, 0u, 0u);                                                                     \
    }                                                                                                                                  \
    _Pragma("unroll")                                                                                                                  \
    for (int r = 0; r < Q; ++r) {                                                                                                      \
      const int e = lane + 64 * r;                                                                                                     \
      if (e < nvalid * Q) {                                                                                                            \
        const int g = e / Q, q = e - g * Q;                                                                                            \
        uint32_t* d = srow + g * K::SWP + 4 * q;                                                                                       \
        d[0] = v[r].x; d[1] = v[r].y; d[2] = v[r].z; d[3] = v[r].w;                                                                    \
      }                                                                                                                                \
    }                                                                                                                                  \
  }                                                                                                                                    \
  const bool mine = lane < nvalid;                                                                                                     \
  const long long gi = g0 + lane;                                                                                                      \
  uint8_t status = mine ? a.done[gi] : static_cast<uint8_t>(0x80);                                                                     \
  const bool played = !(status & 0x80u);  /* bit 7 at entry: a slot that is not played (its row stays as it is) */                     \
  const int first = (played && a.first_moves) ? a.first_moves[gi] : 0;                                                                 \
  int8_t fs = 0;                                                                                                                       \
  int16_t len = 0;                                                                                                                     \
  int n_illegal = 0;                                                                                                                   \
  hb::EnvArgs ea{};                                                                                                                    \
  ea.n = a.n;                                                                                                                          \
  ea.mode = hb::MODE_STEP;                                                                                                             \
  ea.flags = 0;  /* auto-reset off, no leniency */                                                                                     \
  hb::wave_sync();                                                                                                                     \
                                                                                                                                       \
  int t = 0;                                                                                                                           \
  for (; t < a.max_turns; ++t) {                                                                                                       \
    const bool live = !(status & 0x80u);                                                                                               \
    if (!__ballot(live)) break;  /* (wave-uniform) every game of this wavefront is finished */                                         \
    int seat = a.first_seat + t % K::P;                                                                                                \
    if (seat >= K::P) seat -= K::P;                                                                                                    \
    int uid = first;                                                                                                                   \
    if (t > 0 || !a.first_moves) {                                                                                                     \
      if (live) {                                                                                                                      \
        const WalkArgs<K> wa{a.seed, static_cast<unsigned long long>(t) + 1ull};                                                       \
        HB_RULE_WALK(wa, srow + lane * K::SWP, GID, N_RULES, RULES)                                                                    \
        (void)fired;                                                                                                                   \
        uid = act;                                                                                                                     \
      }                                                                                                                                \
    }                                                                                                                                  \
    hb::StepResult sr;                                                                                                                 \
    sr.play = live;                                                                                                                    \
    hb::env_wave_step<K, GW, false, true>(ea, g0, lane, srow, uid, 0, &sr);                                                            \
    HB_TALLY_VARS                                                                                                                      \
    if (live) {                                                                                                                        \
      HB_TALLY_GAME(K::A, K::H, K::P, K::C, B, K::LIFE, t, status, uid, sr.reward, sr.terminal, sr.score, PLAY_FINISH, PLAY_SET_DONE)  \
      n_illegal += sr.illegal ? 1 : 0;                                                                                                 \
    }                                                                                                                                  \
    HB_TALLY_WAVE(lc, B, K::P, seat, lane)                                                                                             \
    if (a.log && mine) a.log[static_cast<long long>(t) * a.n + gi] = live ? uid : -1;                                                  \
  }                                                                                                                                    \
  if (a.log && mine)                                                                                                                   \
    for (; t < a.max_turns; ++t) a.log[static_cast<long long>(t) * a.n + gi] = -1;                                                     \
                                                                                                                                       \
  /* per-game results: only of the games played here (the others' bytes are the caller's) */                                           \
  if (mine && played) {                                                                                                                \
    a.done[gi] = status;                                                                                                               \
    if (status & 0x80u) {                                                                                                              \
      a.final_score[gi] = fs;                                                                                                          \
      a.length[gi] = len;                                                                                                              \
    }                                                                                                                                  \
  }                                                                                                                                    \
  int longest = len, bad = n_illegal;                                                                                                  \
  for (int o = 32; o > 0; o >>= 1) {                                                                                                   \
    longest = max(longest, __shfl_xor(longest, o));                                                                                    \
    bad += __shfl_xor(bad, o);                                                                                                         \
  }                                                                                                                                    \
  if (lane == 0) {                                                                                                                     \
    if (bad) atomicAdd(lc + NC, static_cast<unsigned int>(bad));                                                                       \
    if (longest) atomicMax(lc + NC + 1, static_cast<unsigned int>(longest));                                                           \
  }                                                                                                                                    \
  hb::wave_sync();                                                                                                                     \
  {  /* rows LDS -> HBM, full-width coalesced stores (env_wave_step, phase 3); a row that was not played is unchanged */               \
    uint4* dst = reinterpret_cast<uint4*>(a.rows + g0 * K::SW);                                                                        \
    for (int e = lane; e < nvalid * Q; e += 64) {                                                                                      \
      const int g = e / Q, q = e - g * Q;                                                                                              \
      const uint32_t* s = srow + g * K::SWP + 4 * q;                                                                                   \
      uint4 v;                                                                                                                         \
      v.x = s[0]; v.y = s[1]; v.z = s[2]; v.w = s[3];                                                                                  \
      dst[e] = v;                                                                                                                      \
    }                                                                                                                                  \
  }

#define PLAY_FLUSH(COUNTERS, MAX_LEN)                                                                                                        \
  for (int i = threadIdx.x; i < NC + 2; i += 256) {                                                                                          \
    const unsigned int v = lc[i];                                                                                                            \
    if (!v) continue;                                                                                                                        \
    if (i < NC)                                                                                                                              \
      atomicAdd((COUNTERS) + i, i == 0 ? static_cast<unsigned long long>(-static_cast<long long>(v)) : static_cast<unsigned long long>(v));  \
    else if (i == NC)                                                                                                                        \
      atomicAdd(a.illegal, static_cast<unsigned long long>(v));                                                                              \
    else                                                                                                                                     \
      atomicMax((MAX_LEN), static_cast<int32_t>(v));                                                                                         \
  }

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
    PLAY_WAVE(a.first_gid + gi, a.n_rules[seat], a.rules[seat])
  }
  __syncthreads();
  PLAY_FLUSH(a.counters, a.max_len)
}

// hb_rule_playout_grouped: n_blocks blocks of block_games games, one team per block. The per-game fields are PlayArgs' under
// PlayArgs' names (PLAY_WAVE reads them; n = n_blocks * block_games); the rule lists are device tables, as hb_rule_act_grouped's.
struct GroupArgs {
  uint32_t* rows;
  long long n, first_gid;
  unsigned long long seed;
  int first_seat, max_turns;
  const int32_t* first_moves;
  uint8_t* done;
  int8_t* final_score;
  int16_t* length;
  unsigned long long* counters;   // [n_blocks][NC]
  int32_t* log;
  unsigned long long* illegal;
  int32_t* max_len;               // [n_blocks]
  const int32_t* team_of_block;   // [n_blocks][P]
  const hb_rule* rules;           // [n_sets][HB_MAX_RULES]
  const int32_t* n_rules;         // [n_sets]
  long long block_games, id_stride;
  int n_sets;
  unsigned wgs_per_block;         // ceil(block_games / 256)
};

// a rule list in LDS, read at a uniform address; the fields are made scalar, so that the walk branches on them as it does on
// hb_rule_playout's kernel arguments
struct UniformRules {
  const hb_rule* list;
  __device__ hb_rule operator[](int q) const {
    hb_rule r;
    r.kind = __builtin_amdgcn_readfirstlane(list[q].kind);
    r.arg = __builtin_amdgcn_readfirstlane(list[q].arg);
    r.threshold = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(list[q].threshold)));
    return r;
  }
};

// Workgroup blockIdx.x plays games [w * 256, w * 256 + 256) of block b = blockIdx.x / wgs_per_block, w the remainder: no wavefront
// holds games of two blocks, the last wavefront of a block may be partial. The block's P rule lists are copied to LDS once (at
// most 960 bytes) and every turn's walk reads its seat's list from there at a uniform address; the LDS counters go to the block's
// own counter row and max_len. A block with a seat whose set index is out of range is not played: only its log entries (-1)
// are written.
template <class K>
__global__ __launch_bounds__(256) void playout_grouped_kernel(const GroupArgs a) {
  constexpr int B = K::C * K::R + 1, NC = 2 + B + 5 * K::P;   // hb_eval_counters(cfg)
  constexpr int Q = K::SW / 4;                                // 16-byte pieces of a row
  __shared__ uint32_t lds[4 * GW * K::SWP];
  __shared__ unsigned int lc[NC + 2];   // hb_eval_tally's counters, then: illegal moves, longest game
  __shared__ hb_rule team_rules[K::P][HB_MAX_RULES];
  __shared__ int team_n_rules[K::P];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (provably uniform: g0, nvalid and srow stay scalar)
  const long long b = blockIdx.x / a.wgs_per_block;
  const long long r0 = (static_cast<long long>(blockIdx.x - b * a.wgs_per_block) * 4 + wave) * GW;   // the wavefront's first row of b
  const long long g0 = b * a.block_games + r0;
  const long long left = a.block_games - r0;
  const int nvalid = left <= 0 ? 0 : (left < GW ? static_cast<int>(left) : GW);
  const int32_t* const team = a.team_of_block + b * K::P;   // (workgroup-uniform: scalar loads)
  bool skip = false;
#pragma unroll
  for (int p = 0; p < K::P; ++p) skip = skip || team[p] < 0 || team[p] >= a.n_sets;
  if (skip) {   // (workgroup-uniform)
    if (a.log && lane < nvalid)
      for (int t = 0; t < a.max_turns; ++t) a.log[static_cast<long long>(t) * a.n + g0 + lane] = -1;
    return;
  }
  uint32_t* const srow = lds + wave * (GW * K::SWP);
  for (int i = threadIdx.x; i < NC + 2; i += 256) lc[i] = 0;
  if (threadIdx.x < K::P * HB_MAX_RULES) {
    const int p = threadIdx.x / HB_MAX_RULES, q = threadIdx.x % HB_MAX_RULES;
    team_rules[p][q] = a.rules[static_cast<long long>(team[p]) * HB_MAX_RULES + q];
  }
  if (threadIdx.x < K::P) team_n_rules[threadIdx.x] = min(max(a.n_rules[team[threadIdx.x]], 0), HB_MAX_RULES);
  __syncthreads();

  if (nvalid > 0) {   // (wave-uniform)
    const long long gid0 = a.first_gid + b * (a.id_stride - a.block_games);   // game id of row r of b: gid0 + its index gi
    PLAY_WAVE(gid0 + gi, __builtin_amdgcn_readfirstlane(team_n_rules[seat]), UniformRules{team_rules[seat]})
  }
  __syncthreads();
  PLAY_FLUSH(a.counters + b * NC, a.max_len + b)
}

template <class K>
void launch_playout(const PlayArgs& a, hipStream_t stream) {
  const unsigned blocks = static_cast<unsigned>((a.n + 4 * GW - 1) / (4 * GW));
  hipLaunchKernelGGL((playout_kernel<K>), dim3(blocks), dim3(256), 0, stream, a);
}
template <class K>
void launch_grouped(const GroupArgs& a, hipStream_t stream) {
  const unsigned blocks = static_cast<unsigned>(a.n / a.block_games * a.wgs_per_block);   // n_blocks * wgs_per_block <= n < 2^31
  hipLaunchKernelGGL((playout_grouped_kernel<K>), dim3(blocks), dim3(256), 0, stream, a);
}

struct PlayVariant {
  int P, C, R, H, INFO, LIFE, D;
  void (*launch)(const PlayArgs&, hipStream_t);
  void (*launch_grouped)(const GroupArgs&, hipStream_t);
};
template <class K>
constexpr PlayVariant variant() {
  return PlayVariant{K::P, K::C, K::R, K::H, K::INFO, K::LIFE, K::D, &launch_playout<K>, &launch_grouped<K>};
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

// the checks hb_rule_playout and hb_rule_playout_grouped share: the configuration and its kernel, the buffers every call needs ...
int check_buffers(const hb_config* cfg, const uint32_t* rows_dev, const uint8_t* done_dev, const int8_t* final_score_dev,
                  const int16_t* length_dev, const int64_t* counters_dev, const int64_t* illegal_dev, const int32_t* max_len_dev,
                  const PlayVariant** out) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  const PlayVariant*& var = *out;
  var = nullptr;
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
  return HB_OK;
}

// ... and, after the call's own arguments, the seat, the turn bound and the rows' alignment
int check_turns(const hb_config* cfg, const PlayVariant* var, int32_t first_seat, int32_t max_turns, const uint32_t* rows_dev) {
  const int P = cfg->players;
  if (first_seat < 0 || first_seat >= P) return hb::fail(HB_ERR_INVALID, "first_seat %d out of range for %d players", first_seat, P);
  // no game is longer (hanabi_hip.evaluate.max_turns): draws discards / plays, INFO + draws + C hints, P turns after the last card
  const int draws = var->D - P * var->H;
  const int bound = draws + (var->INFO + draws + var->C) + P;
  if (max_turns < 1 || max_turns > bound) return hb::fail(HB_ERR_INVALID, "max_turns %d out of range 1..%d", max_turns, bound);
  if (reinterpret_cast<uintptr_t>(rows_dev) & 15) return hb::fail(HB_ERR_ALIGN, "rows_dev must be 16-byte aligned");
  return HB_OK;
}

}  // namespace

extern "C" int hb_rule_playout(const hb_config* cfg, uint32_t* rows_dev, int64_t n, int64_t first_game_id, const hb_rule* const* rules,
                               const int32_t* n_rules, uint64_t seed, int32_t first_seat, const int32_t* first_moves_dev,
                               int32_t max_turns, uint8_t* done_dev, int8_t* final_score_dev, int16_t* length_dev,
                               int64_t* counters_dev, int32_t* actions_log_dev, int64_t* illegal_dev, int32_t* max_len_dev,
                               void* stream) {
  const PlayVariant* var = nullptr;
  if (int rc = check_buffers(cfg, rows_dev, done_dev, final_score_dev, length_dev, counters_dev, illegal_dev, max_len_dev, &var)) return rc;
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
  if (int rc = check_turns(cfg, var, first_seat, max_turns, rows_dev)) return rc;
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

extern "C" int hb_rule_playout_grouped(const hb_config* cfg, uint32_t* rows_dev, int64_t n_blocks, int64_t block_games,
                                       int64_t first_game_id, int64_t id_stride, const int32_t* team_of_block_dev,
                                       const hb_rule* rules_dev, const int32_t* n_rules_dev, int32_t n_sets, uint64_t seed,
                                       int32_t first_seat, const int32_t* first_moves_dev, int32_t max_turns, uint8_t* done_dev,
                                       int8_t* final_score_dev, int16_t* length_dev, int64_t* counters_dev, int32_t* actions_log_dev,
                                       int64_t* illegal_dev, int32_t* max_len_dev, void* stream) {
  const PlayVariant* var = nullptr;
  if (int rc = check_buffers(cfg, rows_dev, done_dev, final_score_dev, length_dev, counters_dev, illegal_dev, max_len_dev, &var)) return rc;
  if (!team_of_block_dev) return hb::fail(HB_ERR_INVALID, "null team_of_block_dev: one rule-set index per block and seat");
  if (!rules_dev) return hb::fail(HB_ERR_INVALID, "null rules_dev");
  if (!n_rules_dev) return hb::fail(HB_ERR_INVALID, "null n_rules_dev");
  if (n_sets < 1) return hb::fail(HB_ERR_INVALID, "n_sets must be >= 1, got %d", n_sets);
  if (n_blocks < 0) return hb::fail(HB_ERR_INVALID, "n_blocks must be >= 0");
  if (block_games < 1) return hb::fail(HB_ERR_INVALID, "block_games must be >= 1");
  if (id_stride != 0 && id_stride != block_games)
    return hb::fail(HB_ERR_INVALID, "id_stride must be 0 (repeated deals) or block_games (distinct games)");
  constexpr int64_t kMaxGames = (int64_t{1} << 31) - 1;
  if (n_blocks > 0 && block_games > kMaxGames / n_blocks)
    return hb::fail(HB_ERR_INVALID, "n_blocks * block_games must be below 2^31: split the call");
  if (int rc = check_turns(cfg, var, first_seat, max_turns, rows_dev)) return rc;
  if (n_blocks == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  GroupArgs a{};
  a.rows = rows_dev;
  a.n = n_blocks * block_games;
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
  a.team_of_block = team_of_block_dev;
  a.rules = rules_dev;
  a.n_rules = n_rules_dev;
  a.block_games = block_games;
  a.id_stride = id_stride;
  a.n_sets = n_sets;
  a.wgs_per_block = static_cast<unsigned>((block_games + 4 * GW - 1) / (4 * GW));
  var->launch_grouped(a, static_cast<hipStream_t>(stream));
  HB_HIP(hipGetLastError());
  return HB_OK;
}
