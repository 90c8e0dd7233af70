/*
 * hanabi_hip.h — C-ABI of the MI355X-native Hanabi self-play hot path.
 *
 * One shared library (libhanabi_hip.so, built from hanabi-agents_amd/csrc/) exports
 * exactly the entry points declared here. They are what a binding of the reference
 * would call in place of
 *   - the external C++ hanabi_learning_environment parallel env + canonical encoder
 *     (reference call sites: hanabi_agents/rule_based/ruleset.py:4,
 *      hanabi_agents/rule_based/rule_based.py:2,28,
 *      hanabi_agents/rainbow/run_experiment.py:36,127-128,266-273,308), and
 *   - the pybind11 sum_tree.SumTreef module
 *     (sum_tree/sum_tree/src/sum_tree_py.cc:9-22, used by
 *      hanabi_agents/rlax_dqn/priority_buffer.py:17,30-32,41-42,52).
 *
 * Conventions
 *   - Every pointer argument named *_dev is a DEVICE pointer (HBM). Sizes are element
 *     counts. No torch / C++ types cross this boundary.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream). All work is
 *     enqueued on it; no entry point synchronises unless its comment says so.
 *   - Every function returns HB_OK (0) or a negative HB_ERR_* code and never throws;
 *     hb_last_error() returns a thread-local message for the last failure.
 *   - Handles are owned by the caller and are bound to the HIP device that was current
 *     at creation. One handle per GPU; not re-entrant.
 *   - There is NO CPU fallback: on a machine without a gfx950 device hb_env_create /
 *     hb_tree_create fail with HB_ERR_NO_DEVICE.
 */
#ifndef HANABI_HIP_H
#define HANABI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HB_ABI_VERSION 1

/* ---- status codes ------------------------------------------------------------------ */
#define HB_OK 0
#define HB_ERR_INVALID (-1)   /* bad argument / unsupported configuration */
#define HB_ERR_NO_DEVICE (-2) /* no HIP device, or kernel image not loadable */
#define HB_ERR_HIP (-3)       /* a HIP runtime call failed */
#define HB_ERR_ALIGN (-4)     /* an output pointer is not 16-byte aligned */
#define HB_ERR_NOMEM (-5)

const char* hb_last_error(void);
int hb_abi_version(void);

/* ---- game configuration ------------------------------------------------------------- */
/* Mirrors the HanabiGame parameters the reference passes through rl_env.make
 * (hanabi_agents/rainbow/run_experiment.py:119-128: 'Hanabi-Full', 'Hanabi-Small', ...).
 * Limits: 2<=players<=5, 1<=colors<=5, 1<=ranks<=5, 1<=hand_size<=5,
 * 1<=max_info<=15, 1<=max_life<=7, players*hand_size <= deck size. */
typedef struct hb_config {
  int32_t players;
  int32_t colors;
  int32_t ranks;
  int32_t hand_size;
  int32_t max_info;
  int32_t max_life;
  int32_t flags; /* HB_FLAG_* */
} hb_config;

#define HB_FLAG_AUTO_RESET 1u       /* a game that ends is re-dealt inside the same step */
#define HB_FLAG_RESET_START_NEXT 2u /* auto-reset: new game starts with the seat after the one that just moved
                                       (keeps N lock-stepped games on one acting seat); otherwise seat 0 */
#define HB_FLAG_LENIENT_REWARD 4u   /* clamp negative rewards to 0 (run_experiment.py:41,310 LENIENT_SCORE) */

/* step types, as dm_env / hanabi_agents/rlax_dqn/rlax_rainbow.py:292-308 use them */
#define HB_STEP_FIRST 0
#define HB_STEP_MID 1
#define HB_STEP_LAST 2

/* Derived sizes (pure host functions, usable without a GPU). */
int hb_config_validate(const hb_config* cfg);
int hb_num_actions(const hb_config* cfg);   /* 2*hand + (P-1)*(colors+ranks): 20 / 48 / 11 */
int hb_obs_len(const hb_config* cfg);       /* canonical encoding length: 658 / 1280 / 171 */
int hb_deck_size(const hb_config* cfg);     /* 50 / 20 */
int hb_state_words(const hb_config* cfg);   /* u32 words per game-state row: 32 (P<=3) or 48 */
int hb_obs_words(const hb_config* cfg);     /* u32 words of a bit-packed observation row: ceil(obs_len / 32) = 21 / 40 / 6 */

/* ---- vectorised environment ----------------------------------------------------------
 * N independent games. Game state lives in HBM as one row of hb_state_words() u32 per
 * game (layout documented in DESIGN.md §3 and mirrored by oracle/hanabi_oracle.c).
 *
 * Replaces (external HLE, spec in SURVEY.md App. A): HanabiState::ApplyMove + deal +
 * terminal test + reward, HanabiState::MoveIsLegal over all uids, and
 * CanonicalObservationEncoder::Encode, fused into one kernel launch per step.          */
typedef struct hb_env hb_env;

/* first_game_id: global id of local game 0 (rank * n_games when sharding over GPUs);
 * decks of game g, episode e are a pure function of (seed, first_game_id + g, e).      */
int hb_env_create(const hb_config* cfg, int64_t n_games, uint64_t seed, int64_t first_game_id, hb_env** out);
int hb_env_destroy(hb_env* env);
int64_t hb_env_num_games(const hb_env* env);

/* Explicit-deck mode (parity / known-answer tests): decks_dev is [n_games, deck_size]
 * uint8 card indices (color*ranks+rank); decks_dev[g][0] is the first card dealt. Each
 * (re)deal of game g then uses that order instead of the Philox shuffle. NULL turns it
 * off. The buffer is borrowed and must outlive its use.                                */
int hb_env_set_decks(hb_env* env, const uint8_t* decks_dev);

/* (Re)deal games. mask_dev: [n_games] uint8, nonzero = reset this game, NULL = all.
 * start_player: seat that moves first (0..P-1). Clears the per-seat bookkeeping of the
 * games it resets and bumps their episode counter.                                     */
int hb_env_reset(hb_env* env, const uint8_t* mask_dev, int32_t start_player, void* stream);

/* Encode the current observation + legal-move mask of the seat to act, without changing
 * any state. obs_dev [n, obs_len] int8 0/1, legal_dev [n, n_actions] int8 0/1 (both
 * 16-byte aligned); agent_reward_dev [n] float / agent_step_type_dev [n] int8 may be
 * NULL.                                                                                */
int hb_env_observe(hb_env* env, int8_t* obs_dev, int8_t* legal_dev, float* agent_reward_dev,
                   int8_t* agent_step_type_dev, void* stream);

/* One move per game: actions_dev[g] is the move uid (App. A.2 order: discard, play,
 * reveal colour, reveal rank) chosen by game g's current seat. Then, for the seat that
 * acts next (after an auto-reset: the first seat of the fresh game):
 *   obs_dev / legal_dev          its canonical observation and legal mask   (required)
 *   reward_dev     [n] float     score delta of THIS move                   (nullable)
 *   terminal_dev   [n] int8      1 iff this move ended the game             (nullable)
 *   agent_reward_dev [n] float   rewards accumulated for that seat since its own last
 *                                move, frozen at the end of its episode     (nullable)
 *   agent_step_type_dev [n] int8 HB_STEP_FIRST (seat has no move pending), HB_STEP_LAST
 *                                (its episode ended since its last move), else MID
 *   score_dev      [n] int8      terminal: final score of the finished game (0 if all
 *                                lives lost); otherwise the running score   (nullable)
 * An illegal uid leaves the game untouched, re-emits its observation and increments the
 * counter read by hb_env_illegal_count().                                              */
int hb_env_step(hb_env* env, const int32_t* actions_dev, int8_t* obs_dev, int8_t* legal_dev,
                float* reward_dev, int8_t* terminal_dev, float* agent_reward_dev,
                int8_t* agent_step_type_dev, int8_t* score_dev, void* stream);

/* Bit-packed form of the same observation. The encoder builds every observation as hb_obs_words() u32 of bits before it
 * expands them to the reference's int8 layout; these entry points hand that form out directly:
 *   obs_bits_dev [n, hb_obs_words()] u32 (16-byte aligned; required): observation element i of game g is
 *                bit (i & 31) of word i >> 5 of row g; the pad bits of the last word are zero;
 *   obs_dev      the int8 [n, obs_len] form as well, or NULL to skip it (658 -> 84 bytes written per game for
 *                2-player full Hanabi). hb_obs_unpack of obs_bits_dev gives exactly what obs_dev would have held.
 * Everything else is as in hb_env_observe / hb_env_step. Consumers: hb_replay_insert (rows are plain bytes: pass
 * obs_len = 4 * hb_obs_words()), hb_replay_gather_packed, hb_actor_hidden_packed.                                   */
int hb_env_observe_packed(hb_env* env, uint32_t* obs_bits_dev, int8_t* obs_dev, int8_t* legal_dev, float* agent_reward_dev,
                          int8_t* agent_step_type_dev, void* stream);
int hb_env_step_packed(hb_env* env, const int32_t* actions_dev, uint32_t* obs_bits_dev, int8_t* obs_dev, int8_t* legal_dev,
                       float* reward_dev, int8_t* terminal_dev, float* agent_reward_dev, int8_t* agent_step_type_dev,
                       int8_t* score_dev, void* stream);

/* hb_env_step_packed with the acting agent's epsilon-greedy selection (DQNPolicy.policy's last step, rlax_rainbow.py:113-122)
 * fused into the env kernel: game g's move is chosen from q_dev[g, :] (fp32 [N, A], 16-byte aligned) and sel_legal_dev[g, :]
 * (int8 [N, A]: the previous step's legal output; it may be the same buffer as legal_dev) by the rule and Philox draws of
 * hb_policy_select — identical actions — written to actions_out_dev[g] and applied. At most 64 actions.                    */
int hb_env_step_select_packed(hb_env* env, const float* q_dev, const int8_t* sel_legal_dev, float epsilon, uint64_t seed,
                              uint64_t draw, int64_t first_game_id, int32_t* actions_out_dev, uint32_t* obs_bits_dev,
                              int8_t* obs_dev, int8_t* legal_dev, float* reward_dev, int8_t* terminal_dev,
                              float* agent_reward_dev, int8_t* agent_step_type_dev, int8_t* score_dev, void* stream);
/* int8 0/1 rows [rows, obs_len] <-> packed rows [rows, ceil(obs_len / 32)] u32 (any nonzero byte packs to 1).        */
int hb_obs_pack(const int8_t* obs_dev, uint32_t* bits_dev, int64_t rows, int32_t obs_len, void* stream);
int hb_obs_unpack(const uint32_t* bits_dev, int8_t* obs_dev, int64_t rows, int32_t obs_len, void* stream);

/* Number of illegal uids seen since creation (synchronises the stream).                */
int hb_env_illegal_count(hb_env* env, int64_t* out);

/* Running totals since creation: episodes finished and the sum of their final scores
 * (accumulated inside hb_env_step; synchronises the stream).                             */
int hb_env_stats(hb_env* env, int64_t* episodes, int64_t* score_sum);

/* Raw state rows for differential tests: rows_dev is [n_games, hb_state_words()] u32.  */
int hb_env_export_state(hb_env* env, uint32_t* rows_dev, void* stream);
int hb_env_import_state(hb_env* env, const uint32_t* rows_dev, void* stream);

/* ---- stateless encoder (csrc/encode_rows.hip) --------------------------------------------------
 * The canonical observation and legal-move mask of state rows that belong to no env: rows_dev [n_rows, hb_state_words()] u32
 * in hb_env_export_state's layout (logged rows, determinized rows, the K slabs of a [K, m, SW] buffer as one call with
 * n_rows = K * m), read only. No env, no deck pool, no counters; agent_reward / agent_step_type are not produced.
 *   seat = -1: every row is encoded for its own seat to act. Bit for bit what hb_env_import_state + hb_env_observe_packed /
 *     hb_env_observe write for that row on an env without colour shuffling, finished games and the zero pad bits of the last
 *     packed word included.
 *   seat = 0 .. players - 1: that seat is the observer of every row (the other hands, the missing-card flags, the last move's
 *     actor and target offsets and the knowledge order are relative to it); legal is all zero in the rows where it is not the
 *     seat to act and the ordinary mask where it is.
 * obs_bits_dev [n_rows, hb_obs_words()] u32 and obs_dev [n_rows, hb_obs_len()] int8: either may be NULL, not both;
 * legal_dev [n_rows, hb_num_actions()] int8 or NULL. The identity colour frame only.
 * One lane per row, 16 or 32 rows per wavefront (the env step's rule: 32 for packed-only output of >= 32 768 rows).
 * Checked before any device call: null cfg / rows_dev, a configuration without a compiled kernel, seat, both observation
 * outputs NULL (HB_ERR_INVALID); outputs and rows_dev not 16-byte aligned (HB_ERR_ALIGN). n_rows == 0 is a no-op; without a
 * device: HB_ERR_NO_DEVICE.                                                                                              */
int hb_encode_rows(const hb_config* cfg, const uint32_t* rows_dev, int64_t n_rows, int32_t seat, uint32_t* obs_bits_dev,
                   int8_t* obs_dev, int8_t* legal_dev, void* stream);

/* ---- colour-permuted frames (Other-Play, Hu et al. 2020) ------------------------------------
 * Each game g and seat p has a permutation sigma_{g,p} of the colours, fixed for one deal: the seat sees true colour c as
 * sigma(c). The observation and legal mask the env writes are in the frame of the seat to act, and the move it submits is in
 * that frame too (reveal-colour uid 2H + o*C + c names the colour the seat sees; the env applies 2H + o*C + sigma^-1(c); every
 * other uid is colour-free). The colour-carrying sections of the encoder move by colour block: the other hands' cards,
 * fireworks, discards, the last move's revealed colour and card, and each knowledge slot's plausible identities and
 * revealed-colour bits. sigma_{g,p} = the index-th permutation of 0..C-1 in lexicographic order, index =
 * (out[0] * C!) >> 32 of Philox4x32-10(counter 64 + p, deal counter (state word 6), game id lo, hi; key seed lo, hi), drawn
 * whenever the game is dealt. State rows, decks and hb_env_export_state stay byte-identical to an unshuffled env; importing
 * rows or resetting recomputes every game's sigma from its row.
 *
 * hb_env_set_color_shuffle: seat_mask_dev [n] uint8 (bit p: seat p of that game is shuffled) or NULL, in which case
 * all_seats_mask applies to every game; passing both non-zero is an error, as is a bit past the env's players. An all-zero
 * mask turns the option off (the plain kernels again). The seats' sigma is drawn at once for the deals in progress, so the
 * observation buffers are stale until the next hb_env_observe / step. Rule-based agents (hb_rule_act) read true state rows
 * and belong in unshuffled seats. A shuffled env has no one-launch actor + env step (hb_actor_fused_step_supported is 0).
 * Synchronises `stream` when seat_mask_dev is given (to validate it).
 * hb_env_color_perms: out_dev [n, players, colors] uint8 = sigma_{g,p}(c) (the identity for an unshuffled env or seat).
 * hb_env_color_shuffled: 1 when some seat of some game is shuffled.
 * hb_env_set_color_perms: overwrite the permutations of the deals in progress with perms_dev [n, players, colors] (each row a
 * permutation of 0..colors-1; synchronises `stream` to validate it). They hold until the game is dealt again, when the rule
 * above draws the next ones. For evaluations that replay fixed deals under another game-id layout (hanabi_hip.crossplay).  */
int hb_env_set_color_shuffle(hb_env* env, const uint8_t* seat_mask_dev, uint8_t all_seats_mask, void* stream);
int hb_env_color_perms(hb_env* env, uint8_t* out_dev, void* stream);
int hb_env_color_shuffled(const hb_env* env);
int hb_env_set_color_perms(hb_env* env, const uint8_t* perms_dev, void* stream);

/* Uniform-random legal policy used by bench/tests (Philox(seed, game, draw)):
 * actions_dev[g] = the k-th set entry of legal_dev[g], k uniform. No legal move -> 0.  */
int hb_random_legal_actions(const int8_t* legal_dev, int64_t n_games, int32_t n_actions, uint64_t seed,
                            uint64_t draw, int64_t first_game_id, int32_t* actions_dev, void* stream);

/* ---- rule-based partners (hanabi_agents/rule_based/) ------------------------------------
 * The reference's RulebasedAgent (rule_based.py:13-25) walks a priority list of rules over the rich observation
 * object of ONE game and takes the first move a rule returns, falling back to a random legal move. Here the same
 * walk runs for all games in one launch, straight from the env's state rows (a rule only ever reads what the
 * acting player may see: its own card knowledge, the other hands, fireworks, discards, tokens, deck size).
 * Rule semantics follow ruleset.py (line numbers at each kind); randomness is Philox(seed; draw, game) instead of
 * Python's `random` (word 0: card index, word 1: rank-or-colour coin, word 2: discard index, word 3: legal move).
 * Where ruleset.py hard-codes the full game's 8 information tokens / 5 ranks, the configuration's max_info /
 * ranks are used.                                                                                   */
enum {
  HB_RULE_LEGAL_RANDOM = 0,              /* ruleset.py:598-604                                          */
  HB_RULE_DISCARD_OLDEST_FIRST = 1,      /* :206-216                                                    */
  HB_RULE_OSAWA_DISCARD = 2,             /* :220-280                                                    */
  HB_RULE_TELL_UNKNOWN = 3,              /* :285-308  next player only, colour before rank              */
  HB_RULE_TELL_RANDOMLY = 4,             /* :314-346  next player only                                  */
  HB_RULE_PLAY_SAFE_CARD = 5,            /* :350-379  every plausible identity is playable              */
  HB_RULE_PLAY_IF_CERTAIN = 6,           /* :383-409  colour and rank hinted and playable               */
  HB_RULE_TELL_PLAYABLE_CARD_OUTER = 7,  /* :413-451  (= tell_anyone_useful_card :518-519), rank first  */
  HB_RULE_TELL_DISPENSABLE = 8,          /* :454-514  arg = min_information_tokens                      */
  HB_RULE_DISCARD_RANDOMLY = 9,          /* :607-614                                                    */
  HB_RULE_PLAY_PROBABLY_SAFE = 10,       /* :617-635  threshold; arg != 0: needs more than one life     */
  HB_RULE_DISCARD_PROBABLY_USELESS = 11, /* :638-650  threshold                                         */
  HB_RULE_HAIL_MARY = 12,                /* :653-655  empty deck and > 1 life: play the likeliest card  */
  HB_RULE_TELL_ANYONE_USELESS_CARD = 13, /* :522-535  needs > 1 information token                       */
  HB_RULE_TELL_PLAYABLE_CARD = 14,       /* :570-594  rank or colour by coin                            */
  HB_RULE_TELL_MOST_INFORMATION = 15,    /* :539-562  never returns a move in the reference (no return) */
  HB_RULE_KINDS = 16
};
#define HB_MAX_RULES 16
typedef struct hb_rule {
  int32_t kind;
  int32_t arg;
  float threshold;
} hb_rule;

/* Borrowed device pointer to the env's state rows [n_games, hb_state_words()] (layout: DESIGN.md §3). */
const uint32_t* hb_env_state(hb_env* env);

/* actions_dev[g] = move uid chosen by the first rule that fires for the player to act in game g;
 * fired_dev[g] (optional) = index of that rule, n_rules when none fired and the random-legal fallback
 * of rule_based.py:24 was taken. rules is a HOST array of n_rules <= HB_MAX_RULES entries.            */
int hb_rule_act(const hb_config* cfg, const uint32_t* state_rows_dev, int64_t n_games, int64_t first_game_id,
                const hb_rule* rules, int32_t n_rules, uint64_t seed, uint64_t draw, int32_t* actions_dev,
                int32_t* fired_dev, void* stream);
/* hb_rule_act over n_blocks equal blocks of block_rows games (rows [b * block_rows, (b + 1) * block_rows) of state_rows_dev,
 * actions_dev and fired_dev). Block b walks rule set set_of_block_dev[b] (-1: the block is skipped and nothing of it is
 * written; so is a block whose index is not below n_sets) of the DEVICE tables rules_dev [n_sets][HB_MAX_RULES] and
 * n_rules_dev [n_sets] (clamped to 0..HB_MAX_RULES); the game id of row r is first_game_id + r % block_rows. Each block's actions
 * and fired indices are bit for bit those of hb_rule_act on that block's rows with that rule set. The rule kinds are read on
 * the device and not checked (an unknown kind never fires).                                                                  */
int hb_rule_act_grouped(const hb_config* cfg, const uint32_t* state_rows_dev, int64_t n_blocks, int64_t block_rows,
                        int64_t first_game_id, const int32_t* set_of_block_dev, const hb_rule* rules_dev,
                        const int32_t* n_rules_dev, int32_t n_sets, uint64_t seed, uint64_t draw, int32_t* actions_dev,
                        int32_t* fired_dev, void* stream);
/* hb_rule_act_grouped for blocks of DISTINCT games (training against a partner pool, hanabi_hip.partner_pool): the same layout
 * and tables, but row r of block b is keyed by its global game id first_game_id + b * block_rows + r. Each block's actions and
 * fired indices are bit for bit those of hb_rule_act on that block's rows with first_game_id + b * block_rows.            */
int hb_rule_act_blocks(const hb_config* cfg, const uint32_t* state_rows_dev, int64_t n_blocks, int64_t block_rows,
                       int64_t first_game_id, const int32_t* set_of_block_dev, const hb_rule* rules_dev,
                       const int32_t* n_rules_dev, int32_t n_sets, uint64_t seed, uint64_t draw, int32_t* actions_dev,
                       int32_t* fired_dev, void* stream);

/* Tuning knob for measurements: games handled per 64-lane wavefront (8, 16, 32 or 64); 0 (the default) picks 16,
 * or 32 for a packed-only step over >= 32768 games. The results do not depend on it.  */
int hb_env_set_games_per_wave(hb_env* env, int32_t g);

/* Deck-pool refill placement. Every game keeps its NEXT deck pre-shuffled in HBM, so a re-deal inside
 * hb_env_step is a 52-byte copy; the shuffles that replace consumed decks run in a second small kernel.
 * on == 0 (default): it runs in order on the caller's stream right after the step kernel (graph-capturable).
 * on != 0: it is forked onto a stream owned by the env and joined by the next call that needs the pool, so
 * it overlaps the caller's following work — worthwhile only when the caller is not launch-bound (the fork /
 * join costs four extra runtime calls per step; measured slower in bench.py). Synchronises the device.    */
int hb_env_set_async_refill(hb_env* env, int32_t on);
/* How often that second kernel runs: every `steps` calls of hb_env_step (1..max_life). A game cannot end in fewer than
 * max_life moves, so a pooled deck consumed at step t is not needed again before step t + max_life; the default is
 * min(max_life, 3). Results do not depend on it (deck(g, e) is a pure function of seed, game id and deal counter).       */
int hb_env_set_refill_period(hb_env* env, int32_t steps);

/* Measurement hook: when both are non-NULL (hipEvent_t handles), every following env kernel
 * launch records its own start/stop into them (hipExtLaunchKernelGGL), i.e. the dispatch's
 * begin/end timestamps rather than a pair of stream markers. NULL, NULL turns it off.      */
int hb_env_set_profile_events(hb_env* env, void* start_event, void* stop_event);

/* Stream-ordering helpers for host drivers (hipEvent_t / hipStream_t as void*): the self-play loop orders its acting
 * and learner streams with a handful of events per step. No reference counterpart (the reference is single-threaded
 * host code); they exist so that a binding needs no HIP runtime binding of its own. Events are created with timing off. */
int hb_event_create(void** event_out);
int hb_event_destroy(void* event);
int hb_event_record(void* event, void* stream);
int hb_stream_wait_event(void* stream, void* event);

/* ---- GPU-resident sum tree ------------------------------------------------------------
 * Replaces sum_tree.SumTreef (sum_tree/sum_tree/include/sum_tree.h:22-130 through
 * sum_tree/sum_tree/src/sum_tree_py.cc:9-22). Flat fp32 heap array in HBM: node 1 is the
 * root, leaves are nodes [cap, 2*cap); every internal node is exactly fl(left + right). */
typedef struct hb_tree hb_tree;

int hb_tree_create(int64_t capacity, hb_tree** out); /* capacity rounds up to a power of two (sum_tree.h:28) */
int hb_tree_destroy(hb_tree* t);
int64_t hb_tree_capacity(const hb_tree* t);          /* get_capacity() */
/* device pointer to the 2*cap floats of the heap (zero-copy consumers). While lazy top levels are on (hb_tree_set_lazy_top), and
 * after they are switched off until the next hb_tree_* call that is given a stream, nodes[1 .. cap / 1024) — the levels above
 * the 1024-leaf subtrees, the root included — may be stale: read the total with hb_tree_total, never as nodes[1].           */
float* hb_tree_nodes(hb_tree* t);
/* copy of the whole heap into nodes_dev[2*cap] (differential tests) */
int hb_tree_export_nodes(hb_tree* t, float* nodes_dev, void* stream);
/* the inverse: overwrite the whole heap with nodes_dev[2*cap] as exported above (checkpoint resume: inner
 * nodes keep the exact fp32 values the incremental updates had produced)                          */
int hb_tree_import_nodes(hb_tree* t, const float* nodes_dev, void* stream);

/* Lazy top levels. Writers (hb_tree_update / hb_per_update with 96..1024 entries, hb_tree_fill_range) rebuild the 1024-leaf
 * subtrees they touch and then re-sum the levels above them in a second, one-workgroup launch. on != 0 drops that launch:
 * the levels above the subtree roots go stale and every READER makes them fresh first — hb_per_sample_gather inside its own
 * workgroups (in LDS, the same pairwise sums: identical bits), the other readers (hb_tree_sample, hb_per_sample[_philox],
 * hb_tree_total, hb_tree_export_nodes) by running the re-sum launch themselves. Results never depend on the mode.
 * on == 0 launches nothing (it has no stream): the levels are re-summed by the next reader or writer, on that call's stream. */
int hb_tree_set_lazy_top(hb_tree* t, int32_t on);

/* update_values(indices, values) (sum_tree.h:38-44). Duplicate indices inside one call:
 * the LAST occurrence wins (the sequential order of the reference loop). n<=0 is a no-op.
 * Out-of-range indices are ignored and counted in hb_tree_error_count().                */
int hb_tree_update(hb_tree* t, const int64_t* idx_dev, const float* val_dev, int64_t n, void* stream);

/* The replay ring this tree serves has ring_capacity slots, 1 <= ring_capacity <= hb_tree_capacity (default: the tree's
 * capacity, so a tree that is never told behaves as before). Leaf s stands for ring slot s; the leaves at and beyond
 * ring_capacity are no slots: hb_tree_fill_range wraps at ring_capacity and never writes them, and hb_per_sample,
 * hb_per_sample_philox and hb_per_sample_gather never return them (a key that ends beyond the ring, which only the key
 * float(1 - u) == 1 on the last stratum can do, returns slot ring_capacity - 1 and that leaf's value).
 * hb_tree_sample, hb_tree_update and hb_tree_get keep the tree's own range. Host-only: no launch, no synchronisation. */
int hb_tree_set_ring(hb_tree* t, int64_t ring_capacity);

/* Ring insert used by PriorityBuffer.add_transitions (priority_buffer.py:29-32): leaves
 * (start + i) mod ring_capacity (hb_tree_set_ring) for i in [0, n) take *value_dev (a device
 * scalar, so the running max priority never visits the host). start must be below
 * ring_capacity; n is clipped to it.                                                    */
int hb_tree_fill_range(hb_tree* t, int64_t start, int64_t n, const float* value_dev, void* stream);

/* get_indices + get_values (sum_tree.h:46-72): for each quantile q in [0,1]:
 * descend from the root with query = q * total, going left iff query < left (strict),
 * else query -= left and right (sum_tree.h:92-105). idx_dev[i] = leaf index,
 * val_dev[i] = its value (nullable).                                                    */
int hb_tree_sample(hb_tree* t, const float* quantile_dev, int64_t* idx_dev, float* val_dev, int64_t n,
                   void* stream);

/* get_values(indices) (sum_tree.h:65-72). Out-of-range -> 0 and counted as an error.    */
int hb_tree_get(hb_tree* t, const int64_t* idx_dev, float* val_dev, int64_t n, void* stream);

/* get_total_val() into a device scalar.                                                 */
int hb_tree_total(hb_tree* t, float* total_dev, void* stream);

int hb_tree_error_count(hb_tree* t, int64_t* out); /* synchronises the stream */

/* ---- fused prioritized-replay helpers (priority_buffer.py:36-52) ----------------------
 * hb_per_sample: keys_i = float(linspace(1/B, 1, B)_i - u_i) with u_i in [0, 1/B) given
 * as doubles (priority_buffer.py:37-40), tree descent, and
 * prob_i = (leaf_i + 1e-10) / total in double (priority_buffer.py:42). unit_uniforms != 0:
 * u_i is in [0, 1) and is divided by B inside the kernel (saves the caller a launch).    */
int hb_per_sample(hb_tree* t, const double* u_dev, int64_t batch, int32_t unit_uniforms, int64_t* idx_dev,
                  double* prob_dev, void* stream);
/* The same with the uniforms drawn inside the kernel (no generator launch, nothing for a captured graph to
 * re-seed): u_i = bits53(Philox4x32-10(key = seed; counter = (i, uint64(*counter_dev)))) * 2^-53 / B with
 * bits53 = (word0 >> 5) << 26 | word1 >> 6. counter_dev is any device scalar that changes between calls (the
 * learner passes its optimizer step count).                                                         */
int hb_per_sample_philox(hb_tree* t, uint64_t seed, const float* counter_dev, int64_t batch, int64_t* idx_dev,
                         double* prob_dev, void* stream);
/* hb_per_sample_philox and hb_replay_gather(_packed) (below) in ONE launch: workgroup i descends the tree for stratum i, then
 * expands the sampled transition's two observation rows into x_dev. Outputs and arithmetic are exactly those of the two
 * separate calls; `packed` != 0: the rings hold bit-packed rows (hb_replay_gather_packed), else int8 rows.              */
int hb_per_sample_gather(hb_tree* t, uint64_t seed, const float* counter_dev, int64_t batch, int64_t* idx_dev, double* prob_dev,
                         const void* ring_obs_tm1_dev, const void* ring_obs_t_dev, const int8_t* ring_act_dev,
                         const float* ring_rew_dev, const uint8_t* ring_term_dev, int32_t obs_len, int32_t packed, void* x_dev,
                         int32_t x_dtype, int32_t x_ld, int32_t* act_dev, float* rew_dev, float* term_dev, float* disc_dev,
                         int32_t n_step, float gamma, int64_t capacity, int64_t rows_per_insert, const int64_t* size_wp_dev,
                         void* stream);
/* hb_per_update: p_i = (|td_i| + 1e-10)^alpha (double pow, rounded to float as the
 * pybind float conversion does), max/min priority tracked in device scalars
 * (priority_buffer.py:48-52), then hb_tree_update.                                      */
int hb_per_update(hb_tree* t, const int64_t* idx_dev, const float* td_dev, int64_t n, double alpha,
                  float* max_prio_dev, float* min_prio_dev, void* stream);

/* ---- fused actor tail (hanabi_agents/rlax_dqn/rlax_rainbow.py:113-122,141-150) ---------
 * One pass over the C51 logits [n, n_actions * n_atoms] (logits_dtype 0 = f32, 1 = bf16,
 * 2 = f16): q = mean(softmax(logits) * support, -1), illegal moves -> -inf, then the legal
 * epsilon-greedy sample (epsilon = 0: greedy with uniform tie-breaking). Randomness is
 * Philox4x32-10(seed; draw, first_game_id + g): word 0 -> explore decision, word 1 -> which
 * candidate. support_dev [n_atoms] f32; actions_dev [n] int32; q_dev [n, n_actions] f32 or
 * NULL (receives the UNMASKED q). row_stride >= n_actions*n_atoms: elements between logits
 * rows (the second GEMM's N is padded 1020 -> 1024 because hipBLASLt is 1.4x faster there).  */
int hb_policy_act(const void* logits_dev, int32_t logits_dtype, const int8_t* legal_dev, const float* support_dev,
                  int64_t n_games, int32_t n_actions, int32_t n_atoms, int32_t row_stride, float epsilon, uint64_t seed,
                  uint64_t draw, int64_t first_game_id, int32_t* actions_dev, float* q_dev, void* stream);

/* int8 0/1 observation matrix [rows, cols] -> 16-bit float GEMM operand (out_dtype 1 = bf16,
 * 2 = f16) whose rows are out_ld >= cols elements apart (K padded 658 -> 704: the first GEMM
 * is 1.4x faster); padding columns are not written — zero them once.                       */
int hb_obs_cast(const int8_t* obs_dev, void* out_dev, int32_t out_dtype, int64_t rows, int32_t cols, int32_t out_ld,
                void* stream);

/* ---- fused replay insert (hanabi_agents/rlax_dqn/rlax_rainbow.py:297-308 +
 *      experience_buffer.py:26-81 for a batch without FIRST rows) --------------------------
 * Row i of the batch goes to ring slot (start + i) mod capacity:
 *   ring_obs_tm1 <- last_obs, ring_obs_t <- obs, ring_lms <- legal, ring_act <- actions,
 *   ring_rew <- rewards, ring_term <- (step_type == 2); then last_obs <- obs.
 * The caller advances its ring pointer (experience_buffer.py:58-61,79-81).                */
int hb_replay_insert(int8_t* last_obs_dev, const int8_t* obs_dev, const int8_t* legal_dev, const int32_t* actions_dev,
                     const float* rewards_dev, const int8_t* step_type_dev, int8_t* ring_obs_tm1_dev,
                     int8_t* ring_obs_t_dev, int8_t* ring_act_dev, int8_t* ring_lms_dev, float* ring_rew_dev,
                     uint8_t* ring_term_dev, int64_t n, int32_t obs_len, int32_t n_actions, int64_t capacity,
                     int64_t start, void* stream);

/* ---- off-belief insert (csrc/obl.hip; hanabi_hip/obl.py) -----------
 * hb_replay_insert's counterpart for transitions that come whole out of a fictitious branch of
 * n_steps = P env steps (the learner's move, then one per partner) instead of pairing last_obs
 * with the next observation. Row g of the batch goes to ring slot (start + g) mod capacity.
 *   obs_tm1 [n, row_bytes]   the observation the move was chosen on (plain bytes: int8 rows or
 *                            bit-packed int32 rows alike, as in hb_replay_insert)
 *   actions [n] int32, rewards [n_steps, n] f32, terminal [n_steps, n] int8 (step-major)
 *   obs_t [n, row_bytes], legal_t [n, n_actions]   what the learner sees after the last step
 * With e = the first step k with terminal[k][g] != 0, or n_steps when there is none:
 *   ring_obs_tm1 <- obs_tm1[g], ring_act <- actions[g],
 *   ring_rew  <- rewards[0][g] + ... + rewards[min(e, n_steps - 1)][g], added in this order in fp32
 *                (what a finished game emits after its ending step is not used),
 *   ring_term <- (e < n_steps),
 *   ring_obs_t, ring_lms <- obs_t[g], legal_t[g] when e == n_steps, else all-zero rows (the ring
 *                is a pure function of the inputs, whatever the env emits for a finished game).
 * No buffer is read and written by the same call. n_steps 1..5, n <= capacity, 0 <= start <
 * capacity; n == 0 is a no-op. The caller advances its ring pointer.                          */
int hb_obl_insert(const int8_t* obs_tm1_dev, const int32_t* actions_dev, const float* rewards_dev, const int8_t* terminal_dev,
                  const int8_t* obs_t_dev, const int8_t* legal_t_dev, int8_t* ring_obs_tm1_dev, int8_t* ring_obs_t_dev,
                  int8_t* ring_act_dev, int8_t* ring_lms_dev, float* ring_rew_dev, uint8_t* ring_term_dev, int64_t n,
                  int32_t n_steps, int32_t row_bytes, int32_t n_actions, int64_t capacity, int64_t start, void* stream);

/* ---- fused learner pieces (hanabi_agents/rlax_dqn/rlax_rainbow.py:152-217) ---------------
 * dtype codes: 0 = f32, 1 = bf16, 2 = f16.
 *
 * Precision contract. dtype selects the type of the GEMM operands only (observations, effective weights, hidden
 * activations; the reference runs its whole network in f16, rlax_rainbow.py:250-251); master weights, Adam moments,
 * softmax / projection / cross-entropy and every accumulation are f32, and since round 3 the bf16 path's logits are never
 * rounded (one-kernel actor: fp32 accumulators; learner: fp32 out of hb_thin_gemm). Against the f32 path on the same batch, weights and
 * sampling probabilities (tests/test_dtype_parity.py asserts these on the MI355X; hanabi_agents/rlax_dqn/tolerance.py):
 *                                                        bf16                      f16
 *   per-sample td (where the double-Q selection is     |d| <= 0.012 + 0.004 |td|  |d| <= 0.002 + 0.0005 |td|
 *     unambiguous in f32: top-2 gap > 4e-3 / 6e-4)
 *   loss mean(td * w)                                   2e-3 relative              1e-4 relative
 *   IS weights                                          1e-6 absolute              1e-6 absolute
 *   merged gradients dW1, db1, dW2, db2 (rel. L2)       0.05                       0.03
 *   actor q = mean_k softmax * atoms (|q| <= 0.49)      0.012 absolute             0.003 absolute
 *   chosen move = f32 arg-max where the f32 top-2 gap   > 0.024                    > 0.006
 * Both types run on the same kernels at the same speed (hb_actor_fused_*_dt, hb_thin_gemm bit 2, hb_chain_run): f16 is the
 * reference's own choice and 8 x finer; bf16 (the default) has f32's exponent range, i.e. needs no loss scaling whatever the
 * gradients do (f16 measured: dLoss/dlogits ~ 1e-5 is subnormal there, the hidden layer's gradient loses bits: 0.02 rel. L2).
 *
 * hb_replay_gather: batch gather experience_buffer.py:83-87 straight into the GEMM operand:
 *   x_dev [2*batch, x_ld >= obs_len] (rows 0..B-1 = obs_tm1[idx], B..2B-1 = obs_t[idx]) in x_dtype,
 *   act_dev [B] int32, rew_dev [B] f32, term_dev [B] f32 (0/1), disc_dev [B] f32 = gamma^m.
 * n_step > 1 assembles n-step transitions at sample time (spec: hanabi_agents/rainbow/replay_memory.py:316-345):
 * the seat's next transition of the same game is rows_per_insert slots further on; the chain stops at an episode
 * end or at the ring's write pointer (size_wp_dev = {entries, next slot to write}, device int64[2]);
 * rew = sum gamma^k r_k, obs_t / term from the last step, disc = gamma^m. n_step = 1 is the reference.      */
int hb_replay_gather(const int8_t* ring_obs_tm1_dev, const int8_t* ring_obs_t_dev, const int8_t* ring_act_dev,
                     const float* ring_rew_dev, const uint8_t* ring_term_dev, const int64_t* idx_dev, int64_t batch,
                     int32_t obs_len, void* x_dev, int32_t x_dtype, int32_t x_ld, int32_t* act_dev, float* rew_dev,
                     float* term_dev, float* disc_dev, int32_t n_step, float gamma, int64_t capacity, int64_t rows_per_insert,
                     const int64_t* size_wp_dev, void* stream);

/* The same gather from bit-packed rings (rows of ceil(obs_len / 32) u32, see hb_env_step_packed): x_dev receives the
 * identical 0 / 1 operand.                                                                                              */
int hb_replay_gather_packed(const uint32_t* ring_bits_tm1_dev, const uint32_t* ring_bits_t_dev, const int8_t* ring_act_dev,
                            const float* ring_rew_dev, const uint8_t* ring_term_dev, const int64_t* idx_dev, int64_t batch,
                            int32_t obs_len, void* x_dev, int32_t x_dtype, int32_t x_ld, int32_t* act_dev, float* rew_dev,
                            float* term_dev, float* disc_dev, int32_t n_step, float gamma, int64_t capacity,
                            int64_t rows_per_insert, const int64_t* size_wp_dev, void* stream);

/* hb_c51_loss_grad: rlax_rainbow.py:172-200 on precomputed logits.
 *   logits_online_dev [2B, row_stride >= A*K]: rows 0..B-1 = online(obs_tm1), rows B..2B-1 = online(obs_t);
 *   logits_target_dev [B, A*K] = target(obs_t); support_dev [K] uniform atoms.
 *   Outputs: td_dev [B] (cross-entropy "TD", its |.| is the new priority), w_dev [B] (IS
 *   weights (1/P)^beta / max), dlogits_dev [B, A*K] = d mean(td * w) / d online(obs_tm1).
 *   disc_dev [B]: per-sample discount (gamma for 1-step, gamma^m for n-step transitions).
 *   mask_terminal != 0 multiplies the discount by (1 - term) (off = the reference, App. C-5).
 *   update_counter_dev: NULL, or a device float that this launch increments by one: a per-update counter for the
 *   caller (the optimizer's step number, see hb_noisy_adam_multi's step_offset) without a launch of its own.
 *   bias_online_dev / bias_target_dev: NULL, or the output layers' biases [A*K] (same dtype as the logits) when the
 *   caller's GEMM has not added them (one batched GEMM for both networks has no bias epilogue).               */
int hb_c51_loss_grad(const void* logits_online_dev, const void* logits_target_dev, int32_t dtype, const int32_t* act_dev,
                     const float* rew_dev, const float* term_dev, const double* prios_dev, const float* beta_dev,
                     const float* disc_dev, int32_t mask_terminal, const float* support_dev, int64_t batch, int32_t n_actions,
                     int32_t n_atoms, int32_t row_stride, float* td_dev, float* w_dev, void* dlogits_dev,
                     float* update_counter_dev, const void* bias_online_dev, const void* bias_target_dev, void* stream);

/* The same loss with the gradient in its natural, compact form (csrc/learner2.hip): dLoss/dlogits is non-zero only in the
 * n_atoms atoms of the action each sample took, so instead of a dense [B, A*K] matrix this writes
 *   dl_dev [B, 64] fp32 (16-byte aligned): dl[b, k] = d mean(td * w) / d online(obs_tm1)[b, act[b], k], zero for k >= n_atoms.
 * Everything else (inputs, td_dev, w_dev, update_counter_dev, biases) as in hb_c51_loss_grad; the selector's softmax
 * expectations are spread over all 64 lanes of the sample's wavefront and the batch maximum of the IS weights comes from
 * the extreme probabilities (x -> x^beta is monotone) instead of B pow calls per sample.                                      */
int hb_c51_loss_sparse(const void* logits_online_dev, const void* logits_target_dev, int32_t dtype, const int32_t* act_dev,
                       const float* rew_dev, const float* term_dev, const double* prios_dev, const float* beta_dev,
                       const float* disc_dev, int32_t mask_terminal, const float* support_dev, int64_t batch, int32_t n_actions,
                       int32_t n_atoms, int32_t row_stride, float* td_dev, float* w_dev, float* dl_dev, float* update_counter_dev,
                       const void* bias_online_dev, const void* bias_target_dev, void* stream);

/* hb_thin_gemm: out[b][m, n] = act(sum_k x[b][m, k] * wt[b][n, k] + bias[b][n]) in bf16 with fp32 accumulation, both operands
 * k-contiguous (wt is the TRANSPOSED weight matrix, as hb_actor_pack_weights writes it), as a kernel small enough (one
 * wavefront per workgroup, 36 VGPRs, no LDS) to run on the CUs WHILE hb_actor_hidden / hb_actor_q hold them: the dense layers
 * of DQNLearning.update_q's forward pass (rlax_rainbow.py:172-185 over noisy_mlp.py:176-185) then proceed during the other
 * seat's policy forward instead of queueing behind it. m % 32 == 0, n % 16 == 0, k % 32 == 0; batch >= 1 with element strides;
 * bias (bf16 [batch][n], may be NULL) and ReLU are applied before the bf16 rounding, like a library GEMM epilogue.
 * relu: bit 0 = ReLU; bit 1 = write fp32 instead of bf16 (ldo / out_batch_stride then count floats, out_dev 16-byte aligned):
 * the learner's logits are the accumulators + bias as they are (round 3), so the loss sees no bf16 rounding of the logits;
 * bit 2 = x, wt, bias and a 16-bit output are fp16 instead of bf16 (v_mfma_f32_16x16x32_f16, the same rate).                  */
int hb_thin_gemm(const void* x_dev, const void* wt_dev, const void* bias_dev, void* out_dev, int64_t m, int32_t n, int32_t k,
                 int32_t ldx, int32_t ldw, int32_t ldo, int32_t batch, int64_t x_batch_stride, int64_t w_batch_stride,
                 int64_t out_batch_stride, int32_t relu, void* stream);

/* hb_thin_forward: the two hb_thin_gemm products of the C51 learner's forward pass, restricted to the elements the loss
 * (hb_c51_loss_sparse) and the backward (hb_c51_backward) read, on the same per-element arithmetic: every element it writes is
 * bit-identical to hb_thin_gemm's; the others are not touched. The 2 * batch operand rows are {obs_tm1 [0, batch), obs_t
 * [batch, 2 batch)}. Operands, strides, alignment and the relu flags are hb_thin_gemm's (m = 2 * batch).
 *   layer 1: hb_thin_gemm(m, n, k, batch entries 1) with wt = [online | target] rows (n = 2 * hidden): everything except rows
 *            [0, batch) x columns [n / 2, n) (the target network on obs_tm1, which nobody reads); act_dev and the batch strides unused
 *   layer 2: hb_thin_gemm(m, n, k, batch entries 2 = {online, target}): entry 0 and entry 1 on rows [batch, 2 batch) in full,
 *            entry 1 on rows [0, batch) not at all, and of entry 0 on rows [0, batch) the 16-column tiles that hold the n_atoms
 *            columns [act[b] * n_atoms, (act[b] + 1) * n_atoms) of each sample b (grouped by action inside the kernel; act_dev
 *            int32 [batch]; values outside [0, n_actions) select nothing). batch <= 256, n_actions, n_atoms <= 64
 * batch % 32 == 0, n % 16 == 0 (layer 1: n % 32 == 0, so that the online half [0, n / 2) is whole 16-column tiles: n = 96 is
 * computed, three tiles of the online half on rows [0, batch)), k % 32 == 0 (an odd number of 32-wide K steps included).
 * One wavefront per workgroup, at most 1 024 workgroups, 128 B of LDS: it runs beside the policy kernel like hb_thin_gemm, with
 * 768 (layer 1) / 582 (layer 2, two units each) wavefronts at the 2-player shape instead of 1 024, each unit with the K steps
 * of one product.                                                                                                             */
int hb_thin_forward(int32_t layer, const void* x_dev, const void* wt_dev, const void* bias_dev, void* out_dev, const int32_t* act_dev,
                    int64_t batch, int32_t n, int32_t k, int32_t ldx, int32_t ldw, int32_t ldo, int64_t x_batch_stride,
                    int64_t w_batch_stride, int64_t out_batch_stride, int32_t n_actions, int32_t n_atoms, int32_t relu, void* stream);

/* hb_dqn_loss_sparse: the scalar double-Q loss of the older agent (hanabi_agents/rlax_dqn/rlax_dqn.py:170-205: td = r + g * (1 -
 * terminal) * q_target(s')[argmax q_online(s')] - q_online(s)[a], loss = mean(w_IS * 0.5 * td^2)) on precomputed q values, in the
 * same compact-gradient form as hb_c51_loss_sparse: q_online_dev [2B, row_stride] (rows 0..B-1: obs_tm1, B..2B-1: obs_t),
 * q_target_dev [B, row_stride] (obs_t), action a at column a * col_stride (col_stride 2 stores the scalar head as a 2-atom head
 * whose second atom is unused, so that hb_c51_backward(n_atoms = 2) computes its backward pass); biases in `dtype` at the same
 * columns (may be NULL). Outputs td [B], IS weights [B], dl [B, 64] with dl[b, 0] = dLoss/dq[b, act[b]]. batch <= 256.       */
int hb_dqn_loss_sparse(const void* q_online_dev, const void* q_target_dev, int32_t dtype, const int32_t* act_dev, const float* rew_dev,
                       const float* term_dev, const double* prios_dev, const float* beta_dev, const float* disc_dev, int64_t batch,
                       int32_t n_actions, int32_t col_stride, int32_t row_stride, float* td_dev, float* w_dev, float* dl_dev,
                       const void* bias_online_dev, const void* bias_target_dev, void* stream);

/* hb_c51_backward: everything between that loss and the first layer's weight gradient, in ONE launch (the `jax.grad` of
 * rlax_rainbow.py:203-213 through the output layer and the ReLU of noisy_mlp.py:176-185), from the compact gradient:
 *   dh_dev  [B, hidden]  (dtype)  = (hidden_dev[b, j] > 0) * sum_k dl[b, k] * w2[j, act[b] * n_atoms + k]
 *   db1_dev [hidden]     fp32     = column sums of dh_dev as stored
 *   dw2_dev [hidden, dw2_ld] (dtype): columns a * n_atoms + k = sum over the samples with act == a of hidden[b, j] * dl[b, k]
 *                                  (zero for an action nobody took; columns >= A * n_atoms are not written)
 *   db2_dev [A * n_atoms] fp32    = sum over those samples of dl[b, k]
 * hidden_dev [B, hidden_ld] are the post-ReLU activations of obs_tm1, w2_dev [hidden, w2_ld] the effective output-layer
 * weights, both in `dtype` (0 f32, 1 bf16, 2 f16); batch <= 256. Every sum runs over samples in ascending order: results are
 * bit-reproducible (no atomics). Replaces two dense GEMMs (dW2, dH), hb_colsum and hb_relu_bwd_colsum.                    */
int hb_c51_backward(const float* dl_dev, const int32_t* act_dev, const void* hidden_dev, int32_t hidden_ld, const void* w2_dev,
                    int32_t w2_ld, int32_t dtype, int64_t batch, int32_t hidden, int32_t n_actions, int32_t n_atoms, void* dh_dev,
                    float* db1_dev, void* dw2_dev, int32_t dw2_ld, float* db2_dev, void* stream);

/* hb_colsum: out_dev[j] = sum_i x[i, j] with fp32 accumulation in a fixed order (bias gradients:
 * the column sums of dLoss/dlogits and of dLoss/dhidden). x_dev [rows, cols] contiguous.        */
int hb_colsum(const void* x_dev, int32_t dtype, int64_t rows, int64_t cols, float* out_dev, void* stream);

/* hb_noisy_adam: one Adam step (optix.adam form, rlax_rainbow.py:257) on the three parameters
 * behind one merged NoisyLinear tensor W = w + w_mu + w_sigma * noise (noisy_mlp.py:61-91), given
 * grad_dev = dLoss/dW (f32); writes the new merged tensor to eff_dev in eff_dtype. step_dev holds
 * the number of steps already taken (the caller increments it once per update). The parameter tensors
 * are [n/cols, cols] row-major; eff_dev rows are eff_ld >= cols elements apart (padded GEMM operand).      */
int hb_noisy_adam(float* w_dev, float* w_mu_dev, float* w_sigma_dev, const float* noise_dev, const float* grad_dev,
                  float* m_w_dev, float* v_w_dev, float* m_mu_dev, float* v_mu_dev, float* m_sigma_dev, float* v_sigma_dev,
                  const float* step_dev, void* eff_dev, int32_t eff_dtype, int64_t n, int32_t cols, int32_t eff_ld, float lr,
                  float beta1, float beta2, float eps, void* stream);

/* The same for up to 8 merged tensors (all layers' weights and biases) in ONE launch. w and w_mu see the same
 * gradient at every step, so their moments stay equal: m_mu == m_w and v_mu == v_w may be passed as the SAME arrays, and
 * w's step is then applied to w_mu without a second pass over the moments.                     */
typedef struct hb_adam_tensor {
  float *w, *w_mu, *w_sigma;
  const float* noise;
  const void* grad;      /* gradient of the merged tensor, dtype grad_dtype (0 f32, 1 bf16, 2 f16): e.g. the GEMM output itself */
  float *m_w, *v_w, *m_mu, *v_mu, *m_sigma, *v_sigma;
  void* eff;
  int64_t n;
  int32_t cols, eff_ld;
  int32_t grad_dtype, grad_ld; /* grad rows are grad_ld >= cols elements apart (0: contiguous)                       */
  /* Optional (hb_noisy_adam_multi only; NULL / 0 otherwise): a GRADIENT PRODUCT. An entry with gx != NULL is not stepped by the
   * launch; instead the launch computes this entry's gradient buffer for a later call that steps it:
   *   grad[k, j] = sum_b gx[b, k] * gdh[b, j]   for k < n / cols, j < cols   (dW = X^T dH of a dense layer)
   * gx [g_batch, g_ldx] and gdh [g_batch, g_ldh] in grad_dtype (1 bf16 or 2 f16), v_mfma_f32_16x16x32 with fp32 accumulation over
   * the samples in ascending order, rounded once to grad_dtype; nothing outside those rows and columns of grad is written. Of
   * such an entry only grad, grad_dtype, grad_ld, n, cols and these fields are read. g_batch 1 .. 256, cols % 8 == 0,
   * g_ldx >= n / cols, g_ldx % 8 == 0 (whole 16-byte pieces of a row of gx are read, up to n / cols rounded up to 8),
   * g_ldh >= cols, g_ldh % 8 == 0, grad row stride % 4 == 0; gx, gdh 16-byte and grad 8-byte aligned.                        */
  const void *gx, *gdh;
  int32_t g_batch, g_ldx, g_ldh, g_reserved;
} hb_adam_tensor;
/* This step's number (Adam's bias correction) is t = *step_dev + step_offset: 1 when step_dev counts completed steps
 * (hb_noisy_adam's convention), 0 when it already counts the running one (see hb_c51_loss_grad's counter).      */
/* With ONE gradient-product entry among `tensors` (see hb_adam_tensor) the launch is learner_tail_l2_dw1_kernel
 * (csrc/learner2.hip): its workgroups take one of two roles that share no data — the step of the other entries (same arithmetic
 * per element and same element -> thread mapping as without the product; 4 elements per thread or, where a tensor does not allow
 * 16-byte accesses, the scalar form) and one 32 x 64 tile of the product each (50 KB of LDS per workgroup: it runs in the
 * update's whole-CU window, not beside the policy kernel). eff_dtype must then equal the product's grad_dtype. The caller passes
 * the product together with the entries whose gradients are final (the output layer's W2 and b2 beside dW1) and steps the
 * product's tensor with a second call. A table of the product entry alone computes just the product.                         */
int hb_noisy_adam_multi(const hb_adam_tensor* tensors /* host array of device pointers */, int32_t count,
                        const float* step_dev, float step_offset, int32_t eff_dtype, float lr, float beta1, float beta2,
                        float eps, void* stream);

/* hb_noisy_adam_multi_pack (round 3): the same step for the (up to 4) merged tensors of the one-hidden-layer network, which ALSO
 * writes, in the same pass over the new effective weights, the copies the forward kernels read — what hb_actor_pack_weights (the
 * k-contiguous copies of hb_thin_gemm) and hb_actor_fused_pack (the fragment-major copies of the one-kernel actor) otherwise
 * produce in two more launches per update. eff_dtype 1 (bf16) or 2 (f16). packs[i] describes tensor i's extra outputs:
 *   weight tensors (more than one row): wt = transposed copy [cols][wt_ld] (wt_ld >= rows rounded up to 8), or NULL;
 *     frag + frag_kind = the one-kernel actor's copy: 1 = first layer (W1f; cols must be 512), 2 = output layer (W2f; needs
 *     col_map_dev = hb_actor_fused_columns' physical column of every logit column), 0 / NULL = none;
 *   bias tensors (one row): bias_f32 = fp32 copy of the ROUNDED effective bias, at col_map_dev[j] when that is given, or NULL.
 * Same arithmetic per element as hb_noisy_adam_multi; the copies equal what the two packers make of `eff` bit for bit
 * (tests/test_hip_policy.py).                                                                                                 */
typedef struct hb_adam_pack {
  void* wt;
  void* frag;
  const int32_t* col_map_dev;
  float* bias_f32;
  int32_t wt_ld, frag_kind;
} hb_adam_pack;
int hb_noisy_adam_multi_pack(const hb_adam_tensor* tensors, const hb_adam_pack* packs, int32_t count, const float* step_dev,
                             float step_offset, int32_t eff_dtype, float lr, float beta1, float beta2, float eps, void* stream);

/* ReLU backward fused with the bias gradient (the `jax.grad` of relu + the bias add, rlax_rainbow.py:203-206 through
 * noisy_mlp.py:176-185): dy_dev [rows, cols] is masked in place where act_dev (the post-activation) is <= 0, and
 * out_dev[j] = sum over rows of the masked values (fp32, fixed order).                                          */
int hb_relu_bwd_colsum(void* dy_dev, const void* act_dev, int64_t act_ld /* row stride of act_dev, 0 = cols */, int32_t dtype,
                       int64_t rows, int64_t cols, float* out_dev, void* stream);

/* ---- actor forward on MFMA (csrc/actor.hip): rlax_rainbow.py:113-122,141-150 over noisy_mlp.py:176-185 ------------
 * For the C51 network with ONE hidden layer and bf16 effective weights W = w + w_mu + w_sigma * eps:
 *   hb_actor_pack_weights  the GEMM kernels want both operands k-contiguous: per job, W [k_rows, n_cols] (row stride w_ld,
 *                          bf16) -> wt [n', k_pad] bf16 with n' = (n / group_cols) * 256 + n % group_cols (group_cols = 0:
 *                          n' = n) and bias (bf16 [n_cols]) -> bias_out (fp32, at n'). Entries no input maps to are
 *                          not written: zero-initialise both outputs once. For the output layer use group_cols =
 *                          (256 / n_atoms) * n_atoms (255 for 51 atoms), so that every 256-column tile holds whole actions.
 *   hb_actor_hidden        h_dev [n_rows, hidden] bf16 = relu(obs @ W1 + b1); obs_dev int8 [n_rows, obs_len] with entries in
 *                          0..127 (the canonical encoder emits 0 / 1), widened while staged; w1t_dev [hidden, k_pad],
 *                          k_pad a multiple of 64 >= obs_len, hidden a multiple of 256.
 *   hb_actor_q             q_dev [n_rows, n_actions] fp32 = mean_k(softmax_k(h @ W2 + b2) * support_k) (rlax_rainbow.py:
 *                          117-118); w2t_dev [ceil(n_actions / (256 / n_atoms)) * 256, hidden] packed as above. The logits
 *                          are rounded to bf16 before the softmax, like the output of a bf16 GEMM.
 *   hb_policy_select       the selection half of hb_policy_act on precomputed q (same Philox draws, same tie rule).   */
typedef struct hb_pack_job {
  const void* w;      /* bf16 [k_rows, n_cols], row stride w_ld */
  const void* bias;   /* bf16 [n_cols] */
  void* wt;           /* bf16 [n', k_pad] */
  float* bias_out;    /* fp32 [n'] */
  int32_t k_rows, n_cols, w_ld, group_cols, k_pad;
} hb_pack_job;
int hb_actor_pack_weights(const hb_pack_job* jobs /* host array of device pointers */, int32_t count /* 1..4: one launch */,
                          void* stream);
int hb_actor_hidden(const int8_t* obs_dev, int64_t n_rows, int32_t obs_len, const void* w1t_dev, int32_t k_pad,
                    const float* b1_dev, int32_t hidden, void* h_dev, void* stream);
/* hb_actor_hidden on bit-packed observation rows [n_rows, ceil(obs_len / 32)] u32 (hb_env_step_packed): bit-identical h_dev */
int hb_actor_hidden_packed(const uint32_t* obs_bits_dev, int64_t n_rows, int32_t obs_len, const void* w1t_dev, int32_t k_pad,
                           const float* b1_dev, int32_t hidden, void* h_dev, void* stream);
int hb_actor_q(const void* h_dev, int64_t n_rows, int32_t hidden, const void* w2t_dev, const float* b2_dev,
               const float* support_dev, int32_t n_actions, int32_t n_atoms, float* q_dev, void* stream);
int hb_policy_select(const float* q_dev, const int8_t* legal_dev, int64_t n_games, int32_t n_actions, float epsilon,
                     uint64_t seed, uint64_t draw, int64_t first_game_id, int32_t* actions_dev, void* stream);

/* hb_actor_q with the action selection fused in: the last of a 256-row tile's column-group workgroups to finish (ticket
 * counter per tile) applies hb_policy_select's rule to the tile's rows. tickets_dev: ceil(n_rows / 256) uint32, zero before the
 * first call (the kernel re-arms them); NULL: hb_actor_q followed by hb_policy_select (two launches). Identical actions.      */
int hb_actor_q_select(const void* h_dev, int64_t n_rows, int32_t hidden, const void* w2t_dev, const float* b2_dev,
                      const float* support_dev, int32_t n_actions, int32_t n_atoms, float* q_dev, const int8_t* legal_dev,
                      float epsilon, uint64_t seed, uint64_t draw, int64_t first_game_id, int32_t* actions_dev,
                      uint32_t* tickets_dev, void* stream);

/* hb_actor_hidden[_packed] + hb_actor_q_select behind one call (one binding round trip per policy call);
 * obs_is_packed != 0: obs_dev is the bit-row form. Same argument rules as the functions it wraps.                            */
int hb_actor_act(const void* obs_dev, int32_t obs_is_packed, const int8_t* legal_dev, int64_t n_rows, int32_t obs_len,
                 const void* w1t_dev, int32_t k_pad, const float* b1_dev, int32_t hidden, void* h_dev, const void* w2t_dev,
                 const float* b2_dev, const float* support_dev, int32_t n_actions, int32_t n_atoms, float* q_dev, float epsilon,
                 uint64_t seed, uint64_t draw, int64_t first_game_id, int32_t* actions_dev, uint32_t* tickets_dev, void* stream);

/* ---- The whole policy forward as ONE kernel (csrc/actor_fused.hip, round 3): bit-packed observation rows -> q values, the
 * hidden activations never leave the CU and the logits are never rounded (fp32 accumulators -> C51 expectation).
 * Replaces DQNPolicy's forward (hanabi_agents/rlax_dqn/rlax_rainbow.py:113-122 over noisy_mlp.py:176-185) for the reference
 * topology layers=[512], n_atoms=51 (params.py:13,18); other shapes use hb_actor_hidden[_packed] + hb_actor_q.
 *   hb_actor_fused_supported  1 when the shape is covered (hidden == 512, n_atoms == 51, n_actions <= 80, obs_len <= 4096)
 *   hb_actor_fused_sizes      bytes of the two fragment-major weight copies and floats of the physical-order output bias
 *   hb_actor_fused_pack       effective weights (bf16 row-major W1 [>= obs_len, 512] / W2 [512, >= A * 51], bf16 biases) -> the
 *                             copies the kernel streams: one launch; call after every weight change
 *   hb_actor_fused_q          q [n_rows, n_actions] fp32 from obs_bits [n_rows, ceil(obs_len / 32)] u32
 *   hb_actor_fused_act        the same launch followed, inside the kernel, by hb_policy_select's rule on the rows each workgroup
 *                             has just written (same Philox draws, same tie rule: identical actions); n_actions <= 64           */
int hb_actor_fused_supported(int32_t obs_len, int32_t hidden, int32_t n_actions, int32_t n_atoms);
int hb_actor_fused_sizes(int32_t obs_len, int32_t hidden, int32_t n_actions, int32_t n_atoms, int64_t* w1f_bytes,
                         int64_t* w2f_bytes, int32_t* b2f_floats);
int hb_actor_fused_pack(const void* w1_dev, int32_t w1_ld, const void* b1_dev, const void* w2_dev, int32_t w2_ld,
                        const void* b2_dev, int32_t obs_len, int32_t hidden, int32_t n_actions, int32_t n_atoms, void* w1f_dev,
                        float* b1f_dev, void* w2f_dev, float* b2f_dev, void* stream);
int hb_actor_fused_q(const uint32_t* obs_bits_dev, int64_t n_rows, int32_t obs_len, const void* w1f_dev, const float* b1f_dev,
                     const void* w2f_dev, const float* b2f_dev, const float* support_dev, int32_t hidden, int32_t n_actions,
                     int32_t n_atoms, float* q_dev, void* stream);
int hb_actor_fused_act(const uint32_t* obs_bits_dev, const int8_t* legal_dev, int64_t n_rows, int32_t obs_len, const void* w1f_dev,
                       const float* b1f_dev, const void* w2f_dev, const float* b2f_dev, const float* support_dev, int32_t hidden,
                       int32_t n_actions, int32_t n_atoms, float* q_dev, float epsilon, uint64_t seed, uint64_t draw,
                       int64_t first_game_id, int32_t* actions_dev, void* stream);
/* Physical column (0 .. 512 * ceil(n_actions / 10) - 1) of every logit column action * 51 + atom in the one-kernel actor's
 * output-layer copy / bias: n_actions * 51 ints into HOST memory (for hb_noisy_adam_multi_pack's col_map_dev: upload it).   */
int hb_actor_fused_columns(int32_t n_actions, int32_t* phys_of_logit_host);
/* The same three with the operand type of the 16-bit weights / hidden activations as an argument: dtype 1 = bf16 (what the
 * functions above use), 2 = fp16 — the reference's own network dtype (rlax_rainbow.py:250-251), same MFMA rate
 * (v_mfma_f32_16x16x32_f16), 8 x finer rounding of weights and hidden activations (Precision contract above). Copies packed
 * with one dtype must be run with the same one.                                                                               */
int hb_actor_fused_pack_dt(const void* w1_dev, int32_t w1_ld, const void* b1_dev, const void* w2_dev, int32_t w2_ld,
                           const void* b2_dev, int32_t obs_len, int32_t hidden, int32_t n_actions, int32_t n_atoms, void* w1f_dev,
                           float* b1f_dev, void* w2f_dev, float* b2f_dev, int32_t dtype, void* stream);
/* hb_actor_fused_pack_dt that ALSO writes the k-contiguous (transposed) copies hb_thin_gemm reads — w1t_dev [hidden][w1t_ld >=
 * obs_len rounded up to 64], w2t_dev [n_actions * n_atoms][w2t_ld >= hidden], 16-bit, either may be NULL — so that an update
 * needs ONE pack launch instead of hb_actor_pack_weights + hb_actor_fused_pack (round 3: 5.5 us and a hand-over per update).   */
int hb_actor_fused_pack_thin(const void* w1_dev, int32_t w1_ld, const void* b1_dev, const void* w2_dev, int32_t w2_ld,
                             const void* b2_dev, int32_t obs_len, int32_t hidden, int32_t n_actions, int32_t n_atoms,
                             void* w1f_dev, float* b1f_dev, void* w2f_dev, float* b2f_dev, void* w1t_dev, int32_t w1t_ld,
                             void* w2t_dev, int32_t w2t_ld, int32_t dtype, void* stream);
int hb_actor_fused_q_dt(const uint32_t* obs_bits_dev, int64_t n_rows, int32_t obs_len, const void* w1f_dev, const float* b1f_dev,
                        const void* w2f_dev, const float* b2f_dev, const float* support_dev, int32_t hidden, int32_t n_actions,
                        int32_t n_atoms, float* q_dev, int32_t dtype, void* stream);
int hb_actor_fused_act_dt(const uint32_t* obs_bits_dev, const int8_t* legal_dev, int64_t n_rows, int32_t obs_len,
                          const void* w1f_dev, const float* b1f_dev, const void* w2f_dev, const float* b2f_dev,
                          const float* support_dev, int32_t hidden, int32_t n_actions, int32_t n_atoms, float* q_dev, float epsilon,
                          uint64_t seed, uint64_t draw, int64_t first_game_id, int32_t* actions_dev, int32_t dtype, void* stream);
/* hb_actor_fused_act_dt followed by hb_env_step_packed(env, actions_dev, obs_bits_out_dev, NULL, legal_out_dev, ...) as ONE launch:
 * each workgroup of the policy kernel steps its own 128 games with the moves it has just selected, bit for bit what the two calls
 * compute. Around the launch it does what hb_env_step_packed does (deck-pool join, illegal-move and episode counters,
 * hb_env_set_profile_events timing), except that no refill launch follows: the kernel regenerates the flagged pool decks itself,
 * whatever the refill period and placement. The observation / legal inputs may be the output buffers themselves (in place).
 * n_rows must be the env's game count. Compiled for Hanabi-Full with 2 and 5 players (hb_actor_fused_step_supported); other
 * configurations: HB_ERR_INVALID.                                                                                           */
int hb_actor_fused_act_step(hb_env* env, const uint32_t* obs_bits_dev, const int8_t* legal_dev, int64_t n_rows, int32_t obs_len,
                            const void* w1f_dev, const float* b1f_dev, const void* w2f_dev, const float* b2f_dev,
                            const float* support_dev, int32_t hidden, int32_t n_actions, int32_t n_atoms, float* q_dev, float epsilon,
                            uint64_t seed, uint64_t draw, int64_t first_game_id, int32_t* actions_dev, int32_t dtype,
                            uint32_t* obs_bits_out_dev, int8_t* legal_out_dev, float* reward_dev, int8_t* terminal_dev,
                            float* agent_reward_dev, int8_t* agent_step_type_dev, int8_t* score_dev, void* stream);
int hb_actor_fused_step_supported(const hb_env* env); /* 1: hb_actor_fused_act_step serves this env's configuration */

/* Grouped one-kernel actor (cross-play: many networks over one batch of rows). hb_actor_fused_act_dt in which every 128-row tile
 * (row block [128 t, 128 t + 128)) reads its own descriptor tiles_dev[t] (a DEVICE array of n_rows / 128 entries; n_rows must be a
 * multiple of 128): the fragment-major copies and support of that tile's network and the Philox game id of the tile's first row.
 * For the rows of an active tile, q_dev and actions_dev are bit for bit what hb_actor_fused_act_dt writes for the same rows with
 * that tile's weights and first_game_id = tiles_dev[t].first_game_id; the workgroup of an inactive tile exits at once and writes
 * nothing. One operand dtype per launch (1 bf16, 2 f16): a pool that mixes them takes one launch per dtype with complementary
 * active tiles. All networks share obs_len / hidden / n_actions / n_atoms (checked against hb_actor_fused_supported).     */
typedef struct hb_fused_tile {
  const void* w1f;
  const float* b1f;
  const void* w2f;
  const float* b2f;        /* that network's fragment-major copies (hb_actor_fused_pack_dt), 16-byte aligned */
  const float* support;    /* [n_atoms] */
  int64_t first_game_id;   /* Philox game id of the tile's first row */
  int32_t active;          /* 0: the workgroup exits at once and writes nothing */
  int32_t pad;
} hb_fused_tile;
int hb_actor_fused_act_grouped(const hb_fused_tile* tiles_dev, int64_t n_rows, const uint32_t* obs_bits_dev, const int8_t* legal_dev,
                               int32_t obs_len, int32_t hidden, int32_t n_actions, int32_t n_atoms, float* q_dev, float epsilon,
                               uint64_t seed, uint64_t draw, int32_t* actions_dev, int32_t dtype, void* stream);

/* ---- greedy evaluation (csrc/eval.hip) ------------------------------------------------------------------------------------
 * A fixed set of n_games evaluation games (auto-reset off, lock-step: turn t is seat t mod P in every game) is played to the
 * end; hb_eval_tally is issued once per turn after hb_env_step on the same stream and tallies what that turn did.
 *   actions_dev [n] int32 the moves just stepped; reward_dev [n] f32, terminal_dev [n] int8, score_dev [n] int8: that step's
 *                         outputs (read only for games still live: a finished game's outputs are never relied on)
 *   done_dev    [n] uint8 per-game status, zeroed by the caller before turn 0: bit 7 = finished, bits 0-6 = lives lost
 *   final_score_dev [n] int8 / length_dev [n] int16: written once, on the turn a game ends (score 0 after a bomb-out, as
 *                         score_dev reports it; length = turn + 1)
 *   counters_dev [hb_eval_counters(cfg)] int64, set by the caller before turn 0 (live = n, the rest 0):
 *     [0]                               games still live
 *     [1 .. 1 + B)                      score histogram, B = colors * ranks + 1 bins (score 0 .. colors * ranks)
 *     [1 + B]                           bomb-outs (games that ended with every life lost)
 *     [2 + B + 4 * p + k]               moves of seat p of kind k: 0 discard, 1 play, 2 reveal colour, 3 reveal rank
 *                                       (decoded from the uid, App. A.2 order)
 *     [2 + B + 4 * P + p]               misplays of seat p (a play whose reward is <= 0)
 * A game counts on the turn it ends and only then; games already marked in done_dev are ignored.
 * A uid outside 0 .. A-1 is no move: it has no kind and is no misplay, whatever the reward; the turn still counts towards the
 * length and a terminal still ends the game. A score outside 0 .. B-1 (no env reports one) is counted in the nearest end bin,
 * and final_score_dev gets the raw value. (tests/test_tally_crafted_gpu.py pins both.) Counters are reduced per
 * wavefront (ballots) and per workgroup (LDS); each takes at most one global atomic per workgroup, from <= 128 workgroups. Without a device: HB_ERR_NO_DEVICE (arguments are checked first).                              */
int hb_eval_counters(const hb_config* cfg); /* number of int64 counters: 2 + colors * ranks + 1 + 5 * players */
int hb_eval_tally(const hb_config* cfg, int64_t n_games, int32_t seat, int32_t turn, const int32_t* actions_dev,
                  const float* reward_dev, const int8_t* terminal_dev, const int8_t* score_dev, uint8_t* done_dev,
                  int8_t* final_score_dev, int16_t* length_dev, int64_t* counters_dev, void* stream);
/* hb_eval_tally over n_blocks independent evaluations of block_games games each, stepped together (one seat and turn for all):
 * the per-game arrays hold the blocks one after another and counters_dev is [n_blocks][hb_eval_counters(cfg)]. Block b's
 * counters, done, final_score and length are exactly what hb_eval_tally computes on that block alone; a 2-D grid (one row of
 * workgroups per block) keeps its per-workgroup reduction and <= 128 atomics per counter and block.                         */
int hb_eval_tally_grouped(const hb_config* cfg, int64_t n_blocks, int64_t block_games, int32_t seat, int32_t turn,
                          const int32_t* actions_dev, const float* reward_dev, const int8_t* terminal_dev, const int8_t* score_dev,
                          uint8_t* done_dev, int8_t* final_score_dev, int16_t* length_dev, int64_t* counters_dev, void* stream);

/* ---- partner-response counts (csrc/eval.hip) ------------------------------------------------------------------------------
 * The conditional action counts "my move given the move made just before mine" of an evaluation. hb_eval_response_tally is
 * issued once per turn AFTER hb_env_step and BEFORE that turn's hb_eval_tally, on the same stream: bit 7 of done_dev[g] then
 * still means "game g was finished before this turn", so a game's last move is counted.
 *   actions_dev [n] int32 the moves just stepped (seat `seat` made them in every game)
 *   done_dev    [n] uint8 hb_eval_tally's status bytes; read only, and only bit 7
 *   prev_dev    [n] int32 the previous move of each game, set to -1 by the caller before turn 0
 *   resp_dev    [P][A + 1][A] int64 the counts (A = hb_num_actions(cfg)), zeroed by the caller before turn 0
 * For every game with bit 7 of done clear and 0 <= uid < A: resp[seat][prev + 1][uid] += 1, then prev[g] = uid. Row 0
 * (prev = -1) holds the first move of a game. A uid outside 0 .. A-1 is not counted and leaves prev[g] as it was; a finished
 * game is neither counted nor written. (A prev outside -1 .. A-1, which only a caller can put there, selects no bin.)
 * One lane per game, grid-stride, <= 128 workgroups; each workgroup fills an LDS histogram of hb_eval_response_bins(cfg)
 * int32 bins and flushes every non-zero bin with one 64-bit global atomic. Only the [seat] slab is touched. All sums are
 * integer sums: the result does not depend on the order of the adds. n == 0 is a no-op. Without a device: HB_ERR_NO_DEVICE
 * (arguments are checked first).                                                                                             */
int hb_eval_response_bins(const hb_config* cfg); /* bins per seat: (A + 1) * A */
int hb_eval_response_tally(const hb_config* cfg, int64_t n_games, int32_t seat, const int32_t* actions_dev, const uint8_t* done_dev,
                           int32_t* prev_dev, int64_t* resp_dev, void* stream);
/* hb_eval_response_tally over n_blocks blocks of block_games games stepped together (hb_eval_tally_grouped's layout): the
 * per-game arrays hold the blocks one after another and resp_dev is [n_blocks][P][A + 1][A]. Block b's counts and prev are
 * exactly what hb_eval_response_tally computes on that block alone; a 2-D grid, one row of workgroups per block.
 * n_blocks <= 65535 and n_blocks * block_games < 2^31.                                                                       */
int hb_eval_response_tally_grouped(const hb_config* cfg, int64_t n_blocks, int64_t block_games, int32_t seat,
                                   const int32_t* actions_dev, const uint8_t* done_dev, int32_t* prev_dev, int64_t* resp_dev,
                                   void* stream);

/* ---- training statistics against a partner pool (csrc/train_tally.hip) ----------------------------------------------------
 * A training env (auto-reset, lock-step) whose rows are cut into 128-game tiles, each tile owned by one member of a partner pool
 * (hanabi_hip.partner_pool). hb_train_tally is issued once per env step, after the step, on the same stream, and adds what that
 * step did to the counter row of the member owning each game's tile:
 *   actions_dev [n] int32 the moves just stepped (seat `seat` acted); reward_dev [n] f32, terminal_dev [n] int8, score_dev [n]
 *                         int8: that step's outputs
 *   tile_member_dev [n / 128] int32: the member of each tile (-1 or >= n_members: not counted); n must be a multiple of 128
 *   lost_dev [n] uint8 / length_dev [n] int16: per-game tally state, set by hb_train_tally_init. Bit 7 of lost = the game's deal
 *                         was not seen (its length and lives are unknown); bits 0-6 = lives lost. Both restart at each terminal:
 *                         every game is tracked from its next deal on.
 *   counters_dev [n_members][hb_train_counters(cfg)] int64, zeroed by the caller:
 *     [0] episodes ended, [1] sum of their scores, [2] sum of their squared scores (score 0 after a bomb-out, as score_dev and
 *     the env's own statistics report it), [3 .. 3 + B) score histogram (B = colors * ranks + 1),
 *     [3 + B] bomb-outs, [4 + B] sum of lengths, [5 + B] episodes counted in those two (deal seen),
 *     [6 + B + 4 * p + k] moves of seat p of kind k (App. A.2 order), [6 + B + 4 * P + p] misplays of seat p (a play whose reward
 *     is <= 0). Bomb-out and misplay rules are those of hb_eval_tally.
 * As there, a uid outside 0 .. A-1 is no move (no kind, no misplay); the step still counts towards the length and a terminal
 * still ends the episode. A score outside 0 .. B-1 is counted in the nearest end bin, and it is that clamped value that goes
 * into the sums [1] and [2], so the sums always equal the histogram's. Moves and misplays count whether or not the deal was seen.
 * Rows of a tile that nobody owns are neither read nor written, lost_dev and length_dev included.
 * Reduced per wavefront (ballots) and per workgroup (LDS); each counter takes at most one global atomic per workgroup, from
 * <= 128 workgroups. Without a device: HB_ERR_NO_DEVICE (arguments are checked first).
 * hb_train_tally_init arms game g (lost = 0, length = 0) when its state row is at the first move of a deal (every information
 * token, no firework, no discard, the deck less the hands: every game of a fresh or reset env), else leaves it unarmed.   */
#define HB_TRAIN_MAX_MEMBERS 64
int hb_train_counters(const hb_config* cfg); /* 6 + colors * ranks + 1 + 5 * players */
int hb_train_tally_init(const hb_config* cfg, const uint32_t* state_rows_dev, int64_t n_games, uint8_t* lost_dev, int16_t* length_dev,
                        void* stream);
int hb_train_tally(const hb_config* cfg, int64_t n_games, int32_t seat, const int32_t* actions_dev, const float* reward_dev,
                   const int8_t* terminal_dev, const int8_t* score_dev, const int32_t* tile_member_dev, int32_t n_members,
                   uint8_t* lost_dev, int16_t* length_dev, int64_t* counters_dev, void* stream);

/* ---- belief-sampled rollout search (csrc/belief.hip; hanabi_hip/search.py) -----------------------------
 * hb_belief_determinize: states the observing seat cannot tell apart from the real one. Output row i * replicas + r is source
 * row i (src_rows_dev [m, hb_state_words()], as hb_env_export_state writes them) with ONLY two things changed: the seat's hand
 * word and the undealt tail of the deck bytes. seat = -1: each row's current player. The pool is the multiset of cards the seat
 * cannot see, in a fixed order: its hand slots oldest first, then the undealt deck positions ascending (<= 64 elements). A card
 * is plausible for a slot iff the slot's knowledge bits (colour_plausible[5] rank_plausible[5]) allow its colour and its rank.
 * Sequential importance sampling, no rejection loop:
 *   for slot s = 0 .. hand size - 1: candidates = the pool elements not yet taken that are plausible for slot s, in pool order;
 *   n_s = their number; n_s == 0: the replica is dead (weight 0, the output row is the source row unchanged); otherwise slot s
 *   takes the k-th candidate, k = (u_s * n_s) >> 32;
 *   the remaining pool elements go to the undealt deck positions in the order of their keys (element l: (v_l & ~63) | l, all
 *   distinct; the element with the smallest key is dealt next): a uniform shuffle;
 *   weight_dev[i * replicas + r] = prod n_s (<= 55^5 < 2^32).
 * With these weights the rows estimate the uniform distribution over all assignments of the pool's PHYSICAL cards to (hand
 * slots, deck positions) that respect the slots' plausibility: the public-knowledge-plus-card-counting belief ("V0 belief"). It
 * does NOT model what the partners' policy implies about the hand (no range tracking): it is not the exact posterior.
 * Randomness: Philox4x32-10(counter (128 + j, draw lo, row id lo, row id hi); key (seed lo, seed hi ^ draw hi)) with row id =
 * first_row_id + output row index: u_s = word 0 of j = s, v_l = word 1 of j = l. A pure function of (seed, draw, row id, slot /
 * pool index): the result does not depend on how a call is split. (The deals use counter word 0 < 64 and the colour
 * permutations 64 .. 68 with the key seed; this kernel uses 128 .. 191.)
 * Rows whose status is not "running" (and rows whose current player is no seat) give weight 0 and an unchanged copy.
 * hb_search_reduce: score_dev [m, n_actions, replicas] int8 final scores of the rollouts, weight_dev [m, replicas] u32 (every
 * action of a root starts from the same replicas), legal_dev [m, n_actions] int8 the roots' legal masks ->
 *   value_dev [m, A] f32 = float(double(sum w * score) / double(sum w)), both sums exact in 64-bit integers;
 *   wsum_dev [m, A] int64 = sum w; n_live_dev [m, A] int32 = replicas with w > 0;
 *   best_dev [m] int32 (may be NULL) = the legal action of the largest value, the lowest uid winning ties; -1 when there is none.
 * An action that is illegal at the root, and every action of a root with sum w = 0: value NaN, wsum 0, n_live 0.
 * hb_search_layout: the determinized rows laid out as the rollout games of a per-root candidate list. det_rows_dev [m * replicas,
 * hb_state_words()] and weight_dev [m * replicas] as hb_belief_determinize wrote them, cand_dev [m, n_cand] int32 (an action uid,
 * or -1: no candidate in this slot), filler_dev [m] int32 (the move that games which are not played make, so that they stay in
 * lock step with the others: the root's lowest legal uid). Game (i, c, r) = index (i * n_cand + c) * replicas + r gets source row
 * i * replicas + r: every candidate of a root starts from the same replicas. It is PLAYED iff cand[i, c] >= 0 and
 * weight[i * replicas + r] != 0:
 *   rows_out_dev [m * n_cand * replicas, hb_state_words()]; forced_out_dev int32 = cand[i, c] where it is >= 0, else filler[i]
 *   (a dead replica is an unchanged copy of its root, so the candidate is as legal there; it is not counted);
 *   done_out_dev uint8 = 0 if played, else 0x80 (hb_eval_tally's "never counted"); n_played_out_dev [m] int32 = the played games
 *   of root i (one lane writes it, no atomics; the caller sums it into the tally's live count).
 * 1 <= n_cand <= 64, replicas >= 1, m * n_cand * replicas < 2^31. With n_cand = hb_num_actions() and cand[i, a] = a where a is
 * legal, -1 elsewhere, this is the [m, A, replicas] layout of RolloutSearch.run.
 * hb_search_compare: score_dev [m, n_cand, replicas] int8, weight_dev [m, replicas] u32, cand_dev [m, n_cand] int32,
 * base_slot_dev [m] int32 (the slot of the root's baseline candidate, the blueprint's move; < 0 or >= n_cand: none) -> per slot c
 * the paired difference to the baseline over the replicas with w_r > 0, d_r = score[i, c, r] - score[i, base, r]:
 *   diff_dev [m, n_cand] f64 = double(sum w_r d_r) / double(sum w_r), both sums exact in 64-bit integers;
 *   se_dev [m, n_cand] f64 = sqrt(sum (w_r (d_r - diff))^2) / sum w_r * sqrt(n / (n - 1)), the sum in double over non-negative
 *   terms (each lane its replicas r = lane, lane + 64, ... in ascending order, then the xor butterfly of the 64 lanes): with
 *   constant weights — every state reached by play — the textbook s / sqrt(n) of the paired differences; n < 2: +inf;
 *   n_pair_dev [m] int32 = n = replicas with w_r > 0.
 * c == base: diff = se = 0. cand[i, c] < 0, no baseline (or cand[i, base] < 0), or sum w = 0: both NaN.
 * 1 <= n_cand <= 64, 1 <= replicas <= 2^20, m * n_cand * replicas < 2^31.
 * hb_belief_splice_alive: "what the partner would have seen". prev_rows_dev [m, hb_state_words()] states the last mover moved
 * from, now or earlier, det_rows_dev [m * n_cand, SW] hb_belief_determinize's candidates for the observer `seat` (candidate (i, k)
 * = row i * n_cand + k). alive_dev [m] u8 (NULL: every slot alive): bit s set = the card in slot s of the observer's hand in prev
 * row i is still in its hand now. Hands are ordered by age (cards slide left on removal, a drawn card goes to the end), so the
 * cards still held are a prefix of the current hand in the same order, and the others were played or discarded, hence public.
 * out_rows_dev [n_cand * m, SW], candidate-major: row k * m + i = prev row i with ONLY word 10 + seat (the observer's hand word)
 * rebuilt: walk the slots s = 0 .. 4 of the previous hand that hold a card (field != 31), j = 0; if bit s is alive and slot j of
 * candidate (i, k)'s hand word holds a card, slot s takes that card and j += 1; in every other case (a dead slot; a candidate that
 * has run out of cards, which must not happen but then still leaves a legal state) slot s keeps the previous row's own card.
 * Empty slots stay empty, their alive bits are ignored, bits 25 .. 31 stay the previous row's. Knowledge, deck bytes and
 * everything else stay the previous state's (another seat's observation and legal mask read the observer's cards, the public
 * state and the deck size, never the deck's order). Slab k is m contiguous rows in the roots' order: it imports into an m-game env
 * whose game ids are the real games'. seat in 0 .. players - 1 (no -1: the observer is not the previous state's current player).
 * Finished rows are spliced like any other. One wavefront per output row, lane j < SW moves word j, the lane of the hand word
 * does the walk in registers.
 * hb_belief_splice = hb_belief_splice_alive with alive NULL: prev_rows_dev are the states the last mover JUST moved from, in
 * which the observer holds the cards it holds now, so word 10 + seat of row k * m + i is that word of candidate (i, k).
 * hb_belief_select_depth: keep the first `replicas` candidates under which the last mover's policy plays the most of its last
 * `depth` moves, 1 <= depth <= 8, entry 0 the most recent. src_rows_dev [m, SW] the current states, det_rows_dev [m * n_cand, SW]
 * / weight_dev [m * n_cand] u32 the candidates, hyp_moves_dev [depth][n_cand * m] int32 (each slab candidate-major: [k * m + i] =
 * the move under candidate (i, k) spliced into entry d's previous state), actual_dev [depth][m] int32 the moves made, valid_dev
 * [depth][m] u8 or NULL (all valid).
 * Per root i: L_i = the number of leading entries d = 0, 1, .. with valid[d][i] != 0 (an invalid entry cuts the chain: nothing
 * older is used); L_i = 0 for a root that is not running (status bits of src word 0). pass_k = the number of leading entries
 * d < L_i with hyp[d][k, i] == actual[d][i]; 0 if weight[i, k] == 0.
 *   n_surv_dev [depth][m] int32: n_surv[D - 1][i] = candidates with pass_k >= D, for D = 1 .. L_i; 0 for D > L_i;
 *   depth_used_dev [m] int32 = the largest D <= L_i with n_surv[D - 1][i] >= 1, 0 if there is none;
 *   depth_used = D > 0: the candidates with pass_k >= D in ascending k fill replicas 0 .. min(n_surv[D - 1], replicas) - 1 (the
 *   j-th becomes output replica i * replicas + j: its determinized row copied whole into out_rows_dev [m * replicas, SW], its
 *   weight into out_weight_dev [m * replicas] u32); the remaining replicas are dead (weight 0, an unchanged copy of src row i);
 *   fallback_dev [m] u8 = 0. D < L_i is a FALLBACK to a shallower filter (the deepest had no survivor), not the exact posterior
 *   given L_i moves: depth_used says which roots;
 *   depth_used = 0 < L_i: fallback = 1, the outputs are candidates 0 .. replicas - 1 with their own weights (the unconditioned
 *   belief: a policy the partner does not follow must not leave the searcher without one);
 *   L_i = 0: the same outputs, fallback = 2; hyp and actual are not read for the root.
 * One wavefront per root, candidates 64 at a time: the first sweep accumulates popc(ballot(pass_k >= D)) for each D, the second
 * places the survivors by running base plus prefix popcount and stops once `replicas` are placed; no atomics, no LDS, a pure
 * function of the inputs. n_cand >= replicas >= 1, m * n_cand * SW < 2^31.
 * hb_belief_select = hb_belief_select_depth with depth 1 and no depth_used output: hyp_moves_dev [n_cand * m], actual_dev [m],
 * valid_dev [m] and n_surv_dev [m] are the [1][..] layouts above. Candidate (i, k) survives iff weight[i, k] != 0 and
 * hyp[k, i] == actual[i]; fallback = 2 for a root that is not running or has valid[i] == 0, 1 for one without a survivor.
 * hb_belief_history_step: one observer's partner history (hanabi_hip.search.PartnerHistory: hist_rows_dev [depth, m, SW] the
 * states the partner moved from, hist_moves_dev [depth, m] int32 the uid it played, hist_alive_dev / hist_valid_dev [depth, m] u8;
 * entry 0 the newest) advanced by one turn for all m games, in place, in ONE launch. Per game g, in this order, each part skipped
 * when its pointer is NULL:
 *   own move: own_moves_dev[g] = uid, a play or discard (0 <= uid < 2 * hand_size) of slot s = uid % hand_size, clears in EVERY
 *   entry d (whatever its valid flag) the s-th set bit among bits 0 .. 4 of alive[d][g]; nothing when s >= their popcount;
 *   reset: reset_dev[g] != 0 sets valid[d][g] = alive[d][g] = 0 for all d (a new deal; rows and moves stay);
 *   push (cur_rows_dev and prev_rows_dev [m, SW], given together): every entry moves one deeper, the oldest is dropped, and entry
 *   0 becomes rows = prev row g; moves = the last move recorded in word 2 of cur row g (kind 1 play: idx; 0 discard: hand_size +
 *   idx; 2 colour hint: 2 * hand_size + (offset - 1) * colors + colour; 3 rank hint: 2 * hand_size + (players - 1) * colors +
 *   (offset - 1) * ranks + rank; -1 when the word's valid bit 0 is clear); alive = the slots s of word 10 + seat of prev row g whose
 *   5-bit field is not 31; valid = 1 iff cur is running (status bits 19-20 of word 0 are 0), word 2 of cur has bit 0 set, its
 *   mover (bits 1-3) is not `seat`, prev is running and prev's current player (bits 13-15 of word 0) is that mover.
 * 1 <= depth <= 8, 0 <= seat < players, m * depth * SW < 2^31. Every word of game g is read and written by that game's threads
 * alone: no LDS, no atomics, no second buffer. Rows move in 16-byte items where hist_rows_dev and prev_rows_dev are 16-byte
 * aligned, word by word otherwise; the result is the same.
 * hb_belief_select_soft: hb_belief_select_depth's inputs read as a likelihood instead of a filter (an epsilon-greedy partner:
 * a share of its moves is off the policy by construction). More inputs: n_legal_dev [depth][n_cand * m] int32 (laid out like
 * hyp_moves_dev: the number of legal moves in the hypothetical state the hypothetical move was computed on), p_table_dev
 * [2][A + 1] f64 on the device, A = hb_num_actions(cfg) (row 0: P(the real move | it is the policy's move, n legal moves), row 1:
 * P(the real move | it is not), indexed by n), and the Philox keys seed / draw / first_row_id. Per root i, L_i as above:
 *   lik_k = 0 if weight[i, k] == 0, else 1 times, for d = 0 .. L_i - 1 in that order, p_table[hyp[d][k, i] == actual[d][i] ? 0 : 1]
 *   [n_legal[d][k, i]] (f64, multiplications only; an n_legal outside 1 .. A makes the factor 0);
 *   mx = max_k lik_k; q_k = (u64) floor(lik_k / mx * 2^24); W_k = weight[i, k] * q_k in u64 (all 0 when mx == 0); T = sum_k W_k
 *   (integers: no order); ess_dev [m] f32 = (f64) T * T / sum_k (f64) W_k^2, 0 when T == 0;
 *   output replica r < replicas: u = (out[0] << 32 | out[1]) of Philox4x32-10 on counter (0x10000 + r, draw low word, row id low,
 *   row id high) with row id = first_row_id + i and hb_belief_determinize's key (seed low, seed high ^ draw high);
 *   target = (u * T) >> 64; the candidate is the first k whose inclusive prefix sum W_0 + .. + W_k exceeds target: its row
 *   copied whole, out_weight = 1 (the replicas are drawn in proportion to importance weight times likelihood, with
 *   replacement, so they weigh the same). T == 0: every replica is dead (weight 0, an unchanged copy of src row i);
 *   n_surv_dev as hb_belief_select_depth's (candidates with at least D leading matches); depth_used_dev [m] = L_i; fallback_dev
 *   [m] = 2 if L_i == 0 (lik = 1 for every live candidate: the draws follow the importance weights alone), else 0: there is no
 *   fallback to a shallower filter, a move that no candidate explains scales every likelihood alike.
 * One wavefront per root, candidates 64 at a time: a sweep for mx and n_surv, one for T, and per 64 outputs one with an inclusive
 * integer scan per chunk on a running base, ballot and find-first; no atomics, no LDS, a pure function of the inputs.
 * 1 <= n_cand <= 4096 (weights below 2^28 and q <= 2^24 keep T below 2^64), replicas >= 1 (n_cand < replicas is allowed),
 * 1 <= depth <= 8, m * max(n_cand, replicas) * SW < 2^31.
 * hb_belief_score: a belief scored against the cards the seat really holds. true_rows_dev [m, SW] the real states, det_rows_dev
 * [m * replicas, SW] / weight_dev [m * replicas] u32 replicas of them (replica r of root i = row i * replicas + r) from any of the
 * samplers above, seat as hb_belief_determinize's (-1: each true row's current player). H = hand_size, NC = colors * ranks. Per
 * root i whose true row is running and whose seat is < players, n = that seat's hand size in the TRUE row (word 1), slots s < n:
 *   truth_dev [m, H] int8 = the 5-bit field of slot s of true word 10 + seat (the card id colour * ranks + rank);
 *   counts_dev [m, H, NC] int64 (may be NULL: not written) = sum_r w_r [slot s of replica r's word 10 + seat == c];
 *   hit_dev [m, H] int64 = sum_r w_r [slot s of replica r == truth[i, s] < NC] (= counts[i, s, truth]; computed either way);
 *   joint_dev [m] int64 = sum_r w_r [every slot s < n of replica r equals the true one, and every one of those is < NC];
 *   wsum_dev [m] int64 = sum_r w_r; n_live_dev [m] int32 = replicas with w_r != 0;
 *   prior_dev [m, H, NC] int8 = the card-counting baseline from the true row alone: the copies of c in the seat's pool (its n hand
 *   slots plus the undealt deck bytes, as hb_belief_determinize reads them) if slot s's knowledge bits allow c's colour and its
 *   rank, else 0.
 * Slots s >= n: truth -1, everything else 0. A root that is not running, or whose seat is >= players: truth -1 and zeros everywhere.
 * A replica of weight 0 counts nothing (it is an unchanged copy of the true hand); a replica slot holding 31 or an id >= NC matches
 * nothing. Integers only (every ratio is the host's), 64-bit sums: no order, bit-equal to hanabi_hip.search.belief_score_ref.
 * 1 <= replicas <= 2^20 (wsum < 2^52), m < 2^31. One wavefront per root; no LDS, no atomics.
 * hb_belief_carry: range tracking, sampled: the hand samples ("particles") of my previous turn carried to my present one. cur_rows_dev
 * [m, SW] the real states now, in which `seat` (0 .. players - 1, the observer) is to act; old_rows_dev [m * K, SW] / old_weight_dev
 * [m * K] u32 the K = n_particles particles of each root at my previous turn (particle (i, k) = row i * K + k; ONLY word 10 + seat, the
 * observer's hand then, is read, and of the weight only whether it is 0); own_slot_dev [m] int32 the slot I played or discarded at
 * that turn (< 0: a hint), revealed_dev [m] int32 the card id that move turned face up (-1: none), drew_dev [m] int32 the card id
 * the partner has visibly drawn since (< 0: none). Per particle (i, k) -> out_rows_dev [m * K, SW], out_weight_dev [m * K] u32:
 *   1. Not usable: the particle is dead if old_weight == 0, if cur row i is not running, or if its current player is not `seat`. A
 *      dead particle has weight 0 and its row is an unchanged copy of cur row i, as in hb_belief_determinize.
 *   2. Card played: if own_slot >= 0, the old hand's 5-bit field in that slot must equal `revealed` (own_slot >= hand_size: no such
 *      slot), else dead; it is removed. The remaining fields that hold a card (!= 31), oldest first, are kept[0 .. k). More kept
 *      cards than the current hand has slots (word 1 of cur row i): dead.
 *   3. Pool: hb_belief_determinize's, built from cur row i: the observer's current hand slots, then the undealt deck positions
 *      ascending.
 *   4. Kept slots: for s < k, slot s takes the first pool element not yet taken whose card equals kept[s]; the CURRENT knowledge
 *      bits of slot s must allow that card's colour and rank (an id >= colors * ranks is never allowed). No such element, or not
 *      allowed: dead. No weight factor.
 *   5. Weight from the partner's draw: g = 1 + the number of pool elements not taken whose card equals `drew`, counted after step 4
 *      and before step 6; g = 1 when drew < 0.
 *   6. New slots: every remaining slot s = k .. hand size - 1 (normally one) takes hb_belief_determinize's step exactly: candidates
 *      (not taken, plausible for slot s), n_s, the (u_s * n_s) >> 32-th of them; n_s == 0: dead.
 *   7. Deck: the rest of the pool goes onto the undealt deck positions by hb_belief_determinize's keyed shuffle.
 *   8. out_weight = g * prod n_s (u32; < 2^32 on any real deck). The row is cur row i with ONLY word 10 + seat and the undealt deck
 *      bytes changed.
 * The input particles are taken as EQUALLY weighted, whatever non-zero weight they carry: that is what hb_belief_select_soft hands
 * out, and what hb_belief_determinize hands out on states reached by play (there its weights are constant per root). Then the
 * weighted output estimates the uniform distribution over the physical assignments of what I cannot see, given the old sample
 * and everything made public since ("Tracking the belief", has the derivation of g). Randomness:
 * hb_belief_determinize's own Philox words (same key, counter 128 + j, row id = first_row_id + output row): a split call gives the
 * same rows. One wavefront per output row, four per workgroup, everything in registers; no LDS, no atomics, a pure function of the
 * inputs. n_particles >= 1, m * n_particles < 2^31.
 * All twelve check their arguments before any launch; m == 0 is a no-op; without a device: HB_ERR_NO_DEVICE.                   */
int hb_belief_determinize(const hb_config* cfg, const uint32_t* src_rows_dev, int64_t m, int32_t seat, int32_t replicas, uint64_t seed,
                          uint64_t draw, int64_t first_row_id, uint32_t* out_rows_dev, uint32_t* weight_dev, void* stream);
int hb_search_reduce(const int8_t* score_dev, const uint32_t* weight_dev, const int8_t* legal_dev, int64_t m, int32_t n_actions,
                     int32_t replicas, float* value_dev, int64_t* wsum_dev, int32_t* n_live_dev, int32_t* best_dev, void* stream);
int hb_search_layout(const hb_config* cfg, const uint32_t* det_rows_dev, const uint32_t* weight_dev, const int32_t* cand_dev,
                     const int32_t* filler_dev, int64_t m, int32_t n_cand, int32_t replicas, uint32_t* rows_out_dev,
                     int32_t* forced_out_dev, uint8_t* done_out_dev, int32_t* n_played_out_dev, void* stream);
int hb_search_compare(const int8_t* score_dev, const uint32_t* weight_dev, const int32_t* cand_dev, const int32_t* base_slot_dev,
                      int64_t m, int32_t n_cand, int32_t replicas, double* diff_dev, double* se_dev, int32_t* n_pair_dev, void* stream);
int hb_belief_splice(const hb_config* cfg, const uint32_t* prev_rows_dev, const uint32_t* det_rows_dev, int64_t m, int32_t seat,
                     int32_t n_cand, uint32_t* out_rows_dev, void* stream);
int hb_belief_select(const hb_config* cfg, const uint32_t* src_rows_dev, const uint32_t* det_rows_dev, const uint32_t* weight_dev,
                     const int32_t* hyp_moves_dev, const int32_t* actual_dev, const uint8_t* valid_dev, int64_t m, int32_t n_cand,
                     int32_t replicas, uint32_t* out_rows_dev, uint32_t* out_weight_dev, int32_t* n_surv_dev, uint8_t* fallback_dev,
                     void* stream);
int hb_belief_splice_alive(const hb_config* cfg, const uint32_t* prev_rows_dev, const uint8_t* alive_dev, const uint32_t* det_rows_dev,
                           int64_t m, int32_t seat, int32_t n_cand, uint32_t* out_rows_dev, void* stream);
int hb_belief_select_depth(const hb_config* cfg, const uint32_t* src_rows_dev, const uint32_t* det_rows_dev, const uint32_t* weight_dev,
                           const int32_t* hyp_moves_dev, const int32_t* actual_dev, const uint8_t* valid_dev, int64_t m, int32_t n_cand,
                           int32_t replicas, int32_t depth, uint32_t* out_rows_dev, uint32_t* out_weight_dev, int32_t* n_surv_dev,
                           int32_t* depth_used_dev, uint8_t* fallback_dev, void* stream);
int hb_belief_select_soft(const hb_config* cfg, const uint32_t* src_rows_dev, const uint32_t* det_rows_dev, const uint32_t* weight_dev,
                          const int32_t* hyp_moves_dev, const int32_t* n_legal_dev, const int32_t* actual_dev, const uint8_t* valid_dev,
                          const double* p_table_dev, int64_t m, int32_t n_cand, int32_t replicas, int32_t depth, uint64_t seed,
                          uint64_t draw, int64_t first_row_id, uint32_t* out_rows_dev, uint32_t* out_weight_dev, int32_t* n_surv_dev,
                          int32_t* depth_used_dev, uint8_t* fallback_dev, float* ess_dev, void* stream);
int hb_belief_history_step(const hb_config* cfg, int64_t m, int32_t depth, int32_t seat, const int32_t* own_moves_dev,
                           const uint8_t* reset_dev, const uint32_t* cur_rows_dev, const uint32_t* prev_rows_dev,
                           uint32_t* hist_rows_dev, int32_t* hist_moves_dev, uint8_t* hist_alive_dev, uint8_t* hist_valid_dev,
                           void* stream);
int hb_belief_score(const hb_config* cfg, const uint32_t* true_rows_dev, const uint32_t* det_rows_dev, const uint32_t* weight_dev,
                    int64_t m, int32_t seat, int32_t replicas, int8_t* truth_dev, int64_t* hit_dev, int64_t* joint_dev,
                    int64_t* wsum_dev, int32_t* n_live_dev, int64_t* counts_dev, int8_t* prior_dev, void* stream);
int hb_belief_carry(const hb_config* cfg, const uint32_t* cur_rows_dev, const uint32_t* old_rows_dev, const uint32_t* old_weight_dev,
                    const int32_t* own_slot_dev, const int32_t* revealed_dev, const int32_t* drew_dev, int64_t m, int32_t seat,
                    int32_t n_particles, uint64_t seed, uint64_t draw, int64_t first_row_id, uint32_t* out_rows_dev,
                    uint32_t* out_weight_dev, void* stream);

/* ---- One host call per step: hb_chain_run (csrc/chain.hip, round 3) ------------------------------------------------------
 * The session that drives DQNAgent (rlax_rainbow.py:277-339: explore / add_experience / update once per env step) issues ~25
 * launches, event waits and event records per step. A host fills an array of hb_cmd ONCE with every pointer, size and stream of
 * one step and then replays it with one call per step, passing what changes (ring position, draw counter, epsilon ...) in two
 * small variable arrays. Each command forwards to the function of the same name above with
 *   p[] / i[] / f[]  its fixed arguments in declaration order (pointers / integers / floating point),
 *   var, fvar        index into vars_i / vars_f of its per-run arguments (-1: none),
 *   cond             index into vars_i of a run / skip switch (-1: always run), stream the hipStream_t it is issued on.
 * Per-run arguments: HB_CMD_REPLAY_INSERT vars_i[var] = start; HB_CMD_ACTOR_FUSED_ACT vars_i[var] = draw, vars_f[fvar] = epsilon
 * (i[5] = seed, i[6] = first_game_id, i[7] = operand dtype: 0 / 1 = bf16, 2 = f16; HB_CMD_ACTOR_FUSED_PACK: i[6] likewise); HB_CMD_TREE_FILL_RANGE vars_i[var], vars_i[var + 1] = start, n (n = 0: skipped);
 * HB_CMD_GRAPH_LAUNCH p[0] = a hipGraphExec_t of the caller (the captured learner update); events are hb_event_create handles.
 * Nothing is computed here: results are those of the individual calls.                                                        */
enum {
  HB_CMD_WAIT_EVENT = 1,       /* hb_stream_wait_event(stream, p[0]) */
  HB_CMD_RECORD_EVENT = 2,     /* hb_event_record(p[0], stream) */
  HB_CMD_REPLAY_INSERT = 3,    /* p[0..11], i[0..3] = n, obs_len (bytes per row), n_actions, capacity */
  HB_CMD_ACTOR_FUSED_ACT = 4,  /* p = obs_bits, legal, w1f, b1f, w2f, b2f, support, q, actions; i = n_rows, obs_len, hidden, A, atoms, seed, first_gid;
                                  p[9] != NULL: hb_actor_fused_act_step instead, p[9..14] = env, reward, terminal, agent_reward,
                                  agent_step_type, score, the step's observation / legal rows rewritten in place (p[0], p[1]) */
  HB_CMD_ENV_STEP_PACKED = 5,  /* p = env, actions, obs_bits, obs, legal, reward, terminal, agent_reward, agent_step_type, score */
  HB_CMD_TREE_FILL_RANGE = 6,  /* p = tree, value */
  HB_CMD_PER_SAMPLE_GATHER = 7,/* p = tree, counter, idx, prob, obs_tm1, obs_t, act, rew, term, x, act_out, rew_out, term_out, disc_out, size_wp;
                                  i = seed, batch, obs_len, packed, x_dtype, x_ld, n_step, capacity, rows_per_insert; f[0] = gamma */
  HB_CMD_GRAPH_LAUNCH = 8,     /* p = hipGraphExec_t */
  HB_CMD_PER_UPDATE = 9,       /* p = tree, idx, td, max_prio, min_prio; i[0] = n; f[0] = alpha */
  HB_CMD_ACTOR_FUSED_PACK = 10,/* p = w1, b1, w2, b2, w1f, b1f, w2f, b2f; i = w1_ld, w2_ld, obs_len, hidden, A, atoms */
  HB_CMD_ACTOR_PACK_WEIGHTS = 11 /* p[0] = hb_pack_job array (host memory), i[0] = count */
};
typedef struct hb_cmd {
  int32_t op, var, fvar, cond;
  void* stream;
  void* p[16];
  int64_t i[10];
  double f[2];
} hb_cmd;
int hb_chain_run(const hb_cmd* cmds, int32_t count, const int64_t* vars_i, const double* vars_f);

#ifdef __cplusplus
}
#endif
#endif /* HANABI_HIP_H */
