/* hanabi_hip_playout.h — hb_rule_playout, hb_rule_playout_grouped: games of rule-list teams played to the end in ONE kernel launch
 * (csrc/playout.hip); the grouped form, one team per block of games, is described above its prototype.
 *
 * Part of the C-ABI of hanabi_hip.h (same conventions: HB_OK or a negative HB_ERR_* code, hb_last_error() for the message,
 * arguments checked before the device is touched, `_dev` pointers are device memory, asynchronous on `stream`). It is declared
 * in a header of its own, and its ctypes signature is kept by hanabi_hip/playout.py, because hanabi_hip.h's prototypes and the
 * table of bounds cases that covers every one of them are pinned by tests that may not change with a feature; the entry points'
 * own guard-band tests (tests/test_playout_gpu.py, tests/test_playout_grouped_gpu.py) hold them to what that table holds the
 * others to. They belong in hanabi_hip.h and in that table as soon as those may change. HB_ABI_VERSION stays 1: nothing existing
 * changed.
 *
 * The loop it replaces (hanabi_hip.evaluate.Evaluator.run, hanabi_hip.search.rollout) issues, per turn t = 0 .. max_turns-1 with
 * seat = (first_seat + t) % P to act in every game: hb_rule_act (that seat's rule list, Philox seed `seed`, draw t + 1, game id
 * first_game_id + g), hb_env_step_packed with auto-reset off and no leniency (flags 0), and hb_eval_tally(seat, t). Here one lane
 * owns one game, holds its state row in LDS from the deal to the end, and runs the same rule walk, the same rules phase of the
 * env step and the same tally bookkeeping on it every turn; no observation or legal mask is encoded, nothing goes through HBM
 * between turns, and the counters take one global atomic per non-zero counter and workgroup at the end of the launch.
 *
 *   rows_dev [n, hb_state_words(cfg)] u32, in and out: the games' state rows (hb_env_export_state's layout), 16-byte aligned
 *   first_game_id                     game id of rows_dev[0] (keys the agents' draws)
 *   rules / n_rules                   HOST arrays of P entries: seat p plays rules[p][0 .. n_rules[p]), n_rules[p] <= HB_MAX_RULES
 *                                     (rules[p] may be NULL when n_rules[p] == 0: the random-legal fallback alone). Copied
 *                                     into the kernel arguments, as hb_rule_act copies its list.
 *   first_seat                        the seat to act on turn 0, 0 .. P-1 (the rows' current player; the kernel does not check)
 *   first_moves_dev [n] int32 or NULL the move of turn 0 of every game instead of its seat's rule walk
 *   max_turns                         turns played at most, 1 .. D - P*H + (INFO + D - P*H + C) + P (no game is longer: D the
 *                                     deck size; hanabi_hip.evaluate.max_turns). A cap below a game's length is legal: the
 *                                     game is then left running, its row as max_turns turns leave it.
 *   done_dev [n] uint8, final_score_dev [n] int8, length_dev [n] int16, counters_dev [hb_eval_counters(cfg)] int64:
 *                                     hb_eval_tally's buffers, prepared by the caller exactly as before turn 0 of the loop
 *                                     (done zero — or 0x80 in the slots not to be played —, counters[0] = games to be played,
 *                                     the rest zero)
 *   actions_log_dev [max_turns, n] int32 or NULL: entry [t, g] = the move of turn t while t < length[g] (or the game still runs),
 *                                     -1 from then on and in games not played. (The loop logs whatever the rule walk returns
 *                                     on a finished row; that is not reproduced.) Every entry is written.
 *   illegal_dev  one int64, ADDED to: the moves the env's rules refused (the loop's hb_env_illegal_count difference)
 *   max_len_dev  one int32, raised (atomic max) to the largest length written; the caller zeroes it
 *
 * For every game whose done bit 7 was clear at entry, rows, done, final_score and length are bit for bit what the loop leaves,
 * and so is counters (all integer sums: the order of the adds does not matter); counters[0] is the number of games still running
 * after max_turns. Games with done bit 7 set at entry (the uncounted slots of hb_search_layout) are NOT played: the loop moves
 * them in step on filler moves, here their rows stay as they were. Nothing reads those rows afterwards.
 *
 * One 64-lane wavefront owns 64 consecutive games, a 256-thread workgroup four wavefronts. The turn loop is a plain for with
 * max_turns as its bound; a wavefront leaves it when all its games are finished. No wavefront waits for another workgroup.
 * Rejected with HB_ERR_INVALID: a NULL cfg / rows_dev / rules / n_rules / done_dev / final_score_dev / length_dev /
 * counters_dev / illegal_dev / max_len_dev, n < 0 or n > 2^31, a configuration without a compiled kernel, n_rules[p] outside
 * 0 .. HB_MAX_RULES, an unknown rule kind, first_seat outside 0 .. P-1, max_turns outside its range; rows_dev not 16-byte
 * aligned: HB_ERR_ALIGN. n == 0 is a no-op; without a device: HB_ERR_NO_DEVICE (arguments are checked first).             */
#ifndef HANABI_HIP_PLAYOUT_H
#define HANABI_HIP_PLAYOUT_H

#include "hanabi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int hb_rule_playout(const hb_config* cfg, uint32_t* rows_dev, int64_t n, int64_t first_game_id, const hb_rule* const* rules,
                    const int32_t* n_rules, uint64_t seed, int32_t first_seat, const int32_t* first_moves_dev, int32_t max_turns,
                    uint8_t* done_dev, int8_t* final_score_dev, int16_t* length_dev, int64_t* counters_dev,
                    int32_t* actions_log_dev, int64_t* illegal_dev, int32_t* max_len_dev, void* stream);

/* hb_rule_playout over n_blocks equal blocks of block_games games, ONE TEAM PER BLOCK, in one launch: the playout form of
 * hb_rule_act_grouped / hb_rule_act_blocks and hb_eval_tally_grouped (cross-play's team blocks on repeated deals, a population of
 * rule lists on common deals, the members of a partner pool on the distinct games of one env).
 *
 *   The per-game arrays (rows_dev, first_moves_dev, done_dev, final_score_dev, length_dev, every row of actions_log_dev) hold the
 *   blocks one after another: n_blocks * block_games entries, block b at [b * block_games, (b + 1) * block_games).
 *   Row r of block b has game id first_game_id + b * id_stride + r. id_stride is 0 (every block replays the same deals:
 *   cross-play) or block_games (distinct games).
 *   team_of_block_dev [n_blocks][P] int32   the rule set of every seat of every block: an index into
 *   rules_dev [n_sets][HB_MAX_RULES], n_rules_dev [n_sets]   DEVICE tables, hb_rule_act_grouped's (n_rules clamped to
 *                                     0 .. HB_MAX_RULES; the kinds are read on the device and not checked: an unknown kind never
 *                                     fires)
 *   counters_dev [n_blocks][hb_eval_counters(cfg)] int64: one row per block, prepared as hb_rule_playout's one row
 *   actions_log_dev [max_turns, n_blocks * block_games] int32 or NULL
 *   illegal_dev  one int64, ADDED to (all blocks)
 *   max_len_dev [n_blocks] int32, each raised (atomic max) to its block's largest length written; the caller zeroes them
 *
 * For every block b, its rows, done, final_score, length, counter row, slice of the log and max_len are bit for bit what
 * hb_rule_playout leaves on that block alone: with the block's team, first_game_id + b * id_stride, the same seed, first_seat,
 * max_turns and the block's slice of first_moves_dev. A block with a seat whose index is negative or not below n_sets is skipped:
 * nothing of it is written, except that its log entries are -1.
 *
 * No wavefront holds games of two blocks: a block takes ceil(block_games / 256) workgroups of a linear grid and its last wavefront
 * may be partial; any block_games >= 1 is legal (a block's rows start 16-byte aligned whenever rows_dev does). The team of a
 * workgroup is uniform: its P rule lists are copied to LDS once and read from there at a uniform address. The LDS counters are
 * per workgroup and reach the block's counter row with one atomic per non-zero counter and workgroup. The turn loop keeps its
 * host-checked bound; no wavefront waits on another workgroup, nothing spins.
 * Rejected as hb_rule_playout rejects (config, NULL buffers, first_seat, max_turns, HB_ERR_ALIGN), and with HB_ERR_INVALID: a NULL
 * team_of_block_dev / rules_dev / n_rules_dev, n_sets < 1, n_blocks < 0, block_games < 1, id_stride neither 0 nor block_games,
 * n_blocks * block_games not below 2^31. n_blocks == 0 is a no-op; without a device: HB_ERR_NO_DEVICE (arguments are checked
 * first).                                                                                                                    */
int hb_rule_playout_grouped(const hb_config* cfg, uint32_t* rows_dev, int64_t n_blocks, int64_t block_games, int64_t first_game_id,
                            int64_t id_stride, const int32_t* team_of_block_dev, const hb_rule* rules_dev,
                            const int32_t* n_rules_dev, int32_t n_sets, uint64_t seed, int32_t first_seat,
                            const int32_t* first_moves_dev, int32_t max_turns, uint8_t* done_dev, int8_t* final_score_dev,
                            int16_t* length_dev, int64_t* counters_dev, int32_t* actions_log_dev, int64_t* illegal_dev,
                            int32_t* max_len_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HANABI_HIP_PLAYOUT_H */
