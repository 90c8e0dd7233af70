/* hanabi_hip_exact.h — hb_belief_enumerate: the EXACT belief of one seat against partners that play rule lists, by enumeration of
 * every hand the seat may hold (csrc/belief_exact.hip; DESIGN.md section 11f, "The exact belief").
 *
 * Part of the C-ABI of hanabi_hip.h (same conventions: HB_OK or a negative HB_ERR_* code, hb_last_error() for the message,
 * arguments checked before the device is touched, `_dev` pointers are device memory, asynchronous on `stream`). Like
 * hanabi_hip_playout.h it is declared in a header of its own, and its ctypes signature is kept by hanabi_hip/exact.py, because
 * hanabi_hip.h's prototypes and the table of bounds cases that covers every one of them are pinned by tests that may not change
 * with a feature; the entry point's own guard-band tests are in tests/test_belief_exact_gpu.py. HB_ABI_VERSION stays 1: nothing
 * existing changed.
 *
 * A team made only of rule lists reads no observation: a seat's move is a pure function of the state row and three Philox keys
 * (HB_RULE_WALK, csrc/rule_walk.hpp: the code of hb_rule_act and hb_rule_playout). The observer's hand enters that walk through
 * one word of the row, and the hands it may hold are few enough to walk them all.
 *
 * Definitions, per root i. They reuse the existing kernels' definitions word for word:
 *   scored      cur row i is running (status bits 19-20 of word 0 are 0) and seat < players      [hb_belief_score's `scored`]
 *   n           the seat's hand size in word 1 of cur row i, at most hand_size                   [hb_belief_determinize]
 *   cnt[c]      the copies of card id c in the seat's pool: its n hand slots, then the undealt deck bytes (the last
 *               min(word 0 & 63, deck size) positions of the deck)                               [hb_belief_determinize's pool]
 *   allowed_s   {c < NC : cnt[c] > 0 and slot s's knowledge bits allow c's colour and c's rank}  [prior[i, s, c] != 0 of
 *               hb_belief_score]; NC = colors * ranks
 *   hand        h = (h_0 .. h_{n-1}), h_s in allowed_s
 *   mass(h)     prod_s (cnt[h_s] - #{t < s : h_t = h_s}), 0 as soon as a factor is <= 0: the ways to pick distinct physical pool
 *               cards for the slots. The deck arrangements behind each pick are equally many, so mass is proportional to the V0
 *               belief of hb_belief_determinize (what its weighted replicas estimate). mass <= 243 and sum mass < 2^29 on rows
 *               reached by play.
 *   N_i         prod_{s < n} |allowed_s|, the enumeration space (1 for an empty hand)
 *   order       hand index e in [0, N_i) is a mixed-radix number, slot 0 the least significant digit; digit value j is the j-th
 *               smallest card id of allowed_s
 *   L_i         the leading entries d of the history with valid != 0 (0 when D = 0)              [hb_belief_select_depth's L]
 *   entry d     mover = the current player of hist row [d, i] (bits 13-15 of word 0). The hypothetical state is that row with
 *               ONLY word 10 + seat rebuilt from h by hb_belief_splice_alive's rule: over the occupied slots of the row's hand,
 *               an alive slot takes the next card of h (a prefix, in order); a dead or empty slot, or one h has no card left
 *               for, keeps its own. The hypothetical move is HB_RULE_WALK on it with the mover's list, seed partner_seed, draw
 *               draws[d], game id first_game_id + i: what hb_rule_act returns on the spliced slab.
 *   pass(h)     the leading entries d < L_i whose hypothetical move equals hist_moves[d, i]
 *
 * Inputs:
 *   cur_rows_dev [m, SW] u32                 the real states now (SW = hb_state_words(cfg))
 *   seat                                     the observer, 0 .. P-1
 *   hist_rows_dev [D, m, SW] u32, hist_moves_dev [D, m] int32, hist_alive_dev [D, m] u8 or NULL (every slot alive),
 *   hist_valid_dev [D, m] u8 or NULL (all valid): hanabi_hip.search.PartnerHistory's layout, entry 0 the newest; 0 <= D <= 8.
 *                                            D = 0 reads no history pointer and walks no rule.
 *   draws                                    HOST array of D Philox draws (may be NULL when D = 0)
 *   partner_seed, first_game_id              the partners' Philox seed and the game id of root 0
 *   rules / n_rules                          HOST arrays of P entries, exactly as hb_rule_playout takes them
 *   max_hands >= 1                           a root with N_i > max_hands is not enumerated (status 1)
 *   replicas R, 1 .. 2^20; seed, draw, first_row_id: the key of the drawn hands (below)
 *   scratch_dev                              hb_belief_enumerate_scratch(cfg, m, max_hands) bytes, 8-byte aligned: per root
 *                                            one pass byte per hand and one 64-bit sum per 1024 hands. Its contents on return
 *                                            are not specified; nothing outside that many bytes is written.
 *
 * Outputs (every element is written):
 *   status_dev [m] u8          0: enumerated; 1: N_i > max_hands; 2: not scored
 *   space_dev [m] int64        N_i (saturating at 2^62; 0 for status 2)
 *   mass_dev [D + 1, m] int64  mass[k, i] = sum of mass(h) over the hands with pass(h) >= k, for k <= L_i; 0 beyond
 *   n_hands_dev [D + 1, m] int32   the hands with mass(h) > 0 among those
 *   depth_used_dev [m] int32   the largest k <= L_i with mass[k, i] > 0
 *   fallback_dev [m] u8        hb_belief_select_depth's codes: 0: depth_used >= 1; 1: L_i > 0 but depth_used = 0; 2: L_i = 0
 *   marg_dev [m, H, NC] int64  sum of mass(h) [pass(h) >= depth_used][h_s = c]: the exact posterior marginal, unnormalised
 *   marg0_dev [m, H, NC] int64 or NULL: the same at level 0, the exact V0 marginal (NOT hb_belief_score's prior, which ignores
 *                              that two slots cannot hold the same physical card)
 *   hands_dev [m, R] u32       R hands drawn with replacement in proportion to mass(h) [pass(h) >= depth_used]. Replica r takes
 *                              u exactly as hb_belief_select_soft does: Philox counter (0x10000 + r, draw low, row id low, row
 *                              id high), row id = first_row_id + i, key (seed low, seed high ^ draw high), u = word 0 << 32 |
 *                              word 1; target = (u * T) >> 64 with T = mass[depth_used, i]; the hand is the first in enumeration
 *                              order whose inclusive prefix sum of the masked masses exceeds target. Written as the seat's hand
 *                              word: 5-bit fields, slots >= n hold 31, bits 25-31 those of cur row i's word. T = 0 (it cannot
 *                              happen for status 0 on a row reached by play): cur row i's own word.
 *   Slots s >= n of marg / marg0 are zero. A root of status 1 or 2 has zeros everywhere but in status and space (fallback
 *   included), and hands = its own hand word.
 *
 * Everything is integer: no result depends on the grid, on how a root's hands are split over lanes, wavefronts or workgroups, or
 * on the order of any sum. Four launches on `stream`: (1) status, space and the outputs' zeros; (2) one workgroup per 1024 hands
 * of a root, one lane per hand, the hypothetical row in LDS (one row per lane, as hb_rule_playout keeps its games): masses, the
 * pass byte of every hand, the per-level sums by integer atomics; (3) depth_used, the marginals (LDS accumulators, integer
 * atomics) and the masked sum of every 1024 hands; (4) one lane per (root, replica): the block of 1024 by a walk over those sums,
 * the hand by a walk over the block. Every loop has a host-checked bound (max_hands, D, H); no wavefront waits on another
 * workgroup, nothing spins.
 *
 * Rejected with HB_ERR_INVALID: a NULL cfg / cur_rows_dev / rules / n_rules / scratch_dev or mandatory output (all but
 * marg0_dev), m < 0, a configuration without a compiled kernel (built: those of hb_rule_playout), D outside 0 .. 8, seat outside
 * 0 .. P-1, R < 1 or R > 2^20, max_hands < 1, a NULL hist_rows_dev / hist_moves_dev / draws when D > 0, n_rules[p] outside
 * 0 .. HB_MAX_RULES (or a NULL list of a non-empty one), an unknown rule kind, m * R or m * ceil(min(max_hands, NC^H) / 1024) not
 * below 2^31 (split the call: first_row_id, first_game_id). scratch_dev not 8-byte aligned: HB_ERR_ALIGN. m == 0 is a no-op;
 * without a device: HB_ERR_NO_DEVICE (arguments are checked first).                                                          */
#ifndef HANABI_HIP_EXACT_H
#define HANABI_HIP_EXACT_H

#include "hanabi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HB_EXACT_MAX_DEPTH 8
#define HB_EXACT_MAX_REPLICAS (1 << 20)
#define HB_EXACT_BLOCK_HANDS 1024

/* Bytes of scratch_dev for m roots: m * (cap + 8 * ceil(cap / 1024)), cap = min(max_hands, NC^H). Negative (HB_ERR_INVALID)
 * for a NULL or invalid cfg, m < 0 or max_hands < 1. Pure host arithmetic. */
int64_t hb_belief_enumerate_scratch(const hb_config* cfg, int64_t m, int64_t max_hands);

int hb_belief_enumerate(const hb_config* cfg, const uint32_t* cur_rows_dev, int64_t m, int32_t seat, const uint32_t* hist_rows_dev,
                        const int32_t* hist_moves_dev, const uint8_t* hist_alive_dev, const uint8_t* hist_valid_dev, int32_t depth,
                        const uint64_t* draws, uint64_t partner_seed, int64_t first_game_id, const hb_rule* const* rules,
                        const int32_t* n_rules, int64_t max_hands, int32_t replicas, uint64_t seed, uint64_t draw,
                        int64_t first_row_id, uint8_t* status_dev, int64_t* space_dev, int64_t* mass_dev, int32_t* n_hands_dev,
                        int32_t* depth_used_dev, uint8_t* fallback_dev, int64_t* marg_dev, int64_t* marg0_dev, uint32_t* hands_dev,
                        void* scratch_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HANABI_HIP_EXACT_H */
