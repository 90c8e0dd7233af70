// rule_agent.hip — the reference's rule-based partners (hanabi_agents/rule_based/ruleset.py, rule_based.py) for all
// games at once: one lane per game walks the caller's priority list of rules over the game's packed state row
//  and emits the first move a rule produces, or a random legal move (rule_based.py:13-25).
//
// A rule only reads what the player to act may see — its OWN cards enter only through their knowledge bits
// (plausible colours / ranks, hinted flags); the other hands, fireworks, discard pile, tokens and deck size are
// public. Everything is integer / bit work on ~130 bytes per game; the two probability rules divide two small
// integers in double precision so that thresholds compare exactly as the Python code (and the CPU oracle) does.
#include <hip/hip_runtime.h>

#include "../../include/hanabi_hip.h"
#include "common.hpp"
#include "env_kernel.hpp"
#include "rule_walk.hpp"

namespace {

struct RuleArgs {
  const uint32_t* rows;
  long long n, first_gid;
  int P, C, R, H, INFO, SW, CPC;
  int n_rules;
  hb_rule rules[HB_MAX_RULES];
  unsigned long long seed, draw;
  int32_t* actions;
  int32_t* fired;
};

// The walk over one game (rule_walk.hpp): state row and outputs g (the enclosing kernel's), Philox game id a.first_gid + LID, rules
// RULES[0 .. N_RULES). A macro, so that rule_kernel expands to exactly the code it was written as (its code object is unchanged)
// and the grouped kernel shares it.
#define HB_RULE_GAME(LID, N_RULES, RULES)                                        \
  HB_RULE_WALK(a, a.rows + g * a.SW, a.first_gid + (LID), N_RULES, RULES)        \
  a.actions[g] = act;                                                            \
  if (a.fired) a.fired[g] = fired;

__global__ void __launch_bounds__(128) rule_kernel(RuleArgs a) {
  const long long g = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (g >= a.n) return;
  HB_RULE_GAME(g, a.n_rules, a.rules)
}

// hb_rule_act_grouped / hb_rule_act_blocks: blockIdx.y = block b of a.n games, blockIdx.x * 128 + lane = its row r. The block's rule
// set (and with it the rule walked at each step) is uniform over the workgroup. The Philox game id of the row is
// a.first_gid + b * id_stride + r: stride 0 for blocks that replay the same deals (cross-play), stride a.n for the blocks of one
// training env, whose row r of block b is the env's game b * a.n + r.
struct RuleGroups {
  const int32_t* set_of_block;   // [n_blocks]
  const hb_rule* rules;          // [n_sets][HB_MAX_RULES]
  const int32_t* n_rules;        // [n_sets]
  long long id_stride;           // (ahead of n_sets: the four 8-byte fields are then fetched by one kernel-argument load)
  int n_sets;
};
__global__ void __launch_bounds__(128) rule_grouped_kernel(RuleArgs a, RuleGroups grp) {
  const int b = static_cast<int>(blockIdx.y);
  const int set = grp.set_of_block[b];
  if (set < 0 || set >= grp.n_sets) return;   // (-1: a block of other agents)
  const long long r = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  const hb_rule* rules = grp.rules + static_cast<long long>(set) * HB_MAX_RULES;
  const int n_rules = min(max(grp.n_rules[set], 0), HB_MAX_RULES);
  const long long g = static_cast<long long>(b) * a.n + r;
  HB_RULE_GAME(b * grp.id_stride + r, n_rules, rules)
}

}  // namespace

static RuleArgs rule_args(const hb_config* cfg, const uint32_t* state_rows_dev, int64_t n_games, int64_t first_game_id, uint64_t seed,
                          uint64_t draw, int32_t* actions_dev, int32_t* fired_dev) {
  RuleArgs a{};
  a.rows = state_rows_dev;
  a.n = n_games;
  a.first_gid = first_game_id;
  a.P = cfg->players; a.C = cfg->colors; a.R = cfg->ranks; a.H = cfg->hand_size; a.INFO = cfg->max_info;
  a.SW = hb_state_words(cfg);
  a.CPC = hb_deck_size(cfg) / cfg->colors;
  a.seed = seed;
  a.draw = draw;
  a.actions = actions_dev;
  a.fired = fired_dev;
  return a;
}

extern "C" int hb_rule_act(const hb_config* cfg, const uint32_t* state_rows_dev, int64_t n_games, int64_t first_game_id,
                           const hb_rule* rules, int32_t n_rules, uint64_t seed, uint64_t draw, int32_t* actions_dev,
                           int32_t* fired_dev, void* stream) {
  if (!cfg || !state_rows_dev || !actions_dev) return hb::fail(HB_ERR_INVALID, "null argument");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (n_rules < 0 || n_rules > HB_MAX_RULES) return hb::fail(HB_ERR_INVALID, "n_rules must be 0..%d", HB_MAX_RULES);
  if (n_rules > 0 && !rules) return hb::fail(HB_ERR_INVALID, "null rules");
  for (int i = 0; i < n_rules; ++i)
    if (rules[i].kind < 0 || rules[i].kind >= HB_RULE_KINDS) return hb::fail(HB_ERR_INVALID, "rule %d: unknown kind %d", i, rules[i].kind);
  if (n_games <= 0) return HB_OK;
  RuleArgs a = rule_args(cfg, state_rows_dev, n_games, first_game_id, seed, draw, actions_dev, fired_dev);
  a.n_rules = n_rules;
  for (int i = 0; i < n_rules; ++i) a.rules[i] = rules[i];
  const unsigned blocks = static_cast<unsigned>((n_games + 127) / 128);
  hipLaunchKernelGGL(rule_kernel, dim3(blocks), dim3(128), 0, static_cast<hipStream_t>(stream), a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

static int rule_act_grouped(const hb_config* cfg, const uint32_t* state_rows_dev, int64_t n_blocks, int64_t block_rows,
                            int64_t first_game_id, int64_t id_stride, const int32_t* set_of_block_dev, const hb_rule* rules_dev,
                            const int32_t* n_rules_dev, int32_t n_sets, uint64_t seed, uint64_t draw, int32_t* actions_dev,
                            int32_t* fired_dev, void* stream) {
  if (!cfg || !state_rows_dev || !actions_dev || !set_of_block_dev || !rules_dev || !n_rules_dev) return hb::fail(HB_ERR_INVALID, "null argument");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (n_sets < 1) return hb::fail(HB_ERR_INVALID, "n_sets must be >= 1");
  if (n_blocks < 0 || n_blocks > 65535) return hb::fail(HB_ERR_INVALID, "n_blocks must be 0..65535 (one grid row per block)");
  if (block_rows < 0 || block_rows > (int64_t{1} << 31) * 128 - 1) return hb::fail(HB_ERR_INVALID, "block_rows out of range");
  if (n_blocks == 0 || block_rows == 0) return HB_OK;
  const RuleArgs a = rule_args(cfg, state_rows_dev, block_rows, first_game_id, seed, draw, actions_dev, fired_dev);
  const RuleGroups grp{set_of_block_dev, rules_dev, n_rules_dev, id_stride, n_sets};
  const dim3 grid(static_cast<unsigned>((block_rows + 127) / 128), static_cast<unsigned>(n_blocks));
  hipLaunchKernelGGL(rule_grouped_kernel, grid, dim3(128), 0, static_cast<hipStream_t>(stream), a, grp);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

extern "C" int hb_rule_act_grouped(const hb_config* cfg, const uint32_t* state_rows_dev, int64_t n_blocks, int64_t block_rows,
                                   int64_t first_game_id, const int32_t* set_of_block_dev, const hb_rule* rules_dev,
                                   const int32_t* n_rules_dev, int32_t n_sets, uint64_t seed, uint64_t draw, int32_t* actions_dev,
                                   int32_t* fired_dev, void* stream) {
  return rule_act_grouped(cfg, state_rows_dev, n_blocks, block_rows, first_game_id, 0, set_of_block_dev, rules_dev, n_rules_dev, n_sets,
                          seed, draw, actions_dev, fired_dev, stream);
}

extern "C" int hb_rule_act_blocks(const hb_config* cfg, const uint32_t* state_rows_dev, int64_t n_blocks, int64_t block_rows,
                                  int64_t first_game_id, const int32_t* set_of_block_dev, const hb_rule* rules_dev,
                                  const int32_t* n_rules_dev, int32_t n_sets, uint64_t seed, uint64_t draw, int32_t* actions_dev,
                                  int32_t* fired_dev, void* stream) {
  return rule_act_grouped(cfg, state_rows_dev, n_blocks, block_rows, first_game_id, block_rows, set_of_block_dev, rules_dev, n_rules_dev,
                          n_sets, seed, draw, actions_dev, fired_dev, stream);
}
