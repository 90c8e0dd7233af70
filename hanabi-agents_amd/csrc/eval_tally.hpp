// eval_tally.hpp — the evaluation tally of ONE game and one turn, in the lane that owns the game, and the wavefront's ballots
// into a workgroup's LDS copy of the counters. The one copy of the bookkeeping: eval.hip (hb_eval_tally, issued once per turn on
// the env step's outputs in HBM) and playout.hip (hb_rule_playout, every turn of a game inside one launch, on registers) both
// include it. The counters' layout is hb_eval_tally's (include/hanabi_hip.h).
//
// Macros, like HB_RULE_WALK (rule_walk.hpp) and for its reason: eval_tally_grouped_kernel expands to exactly the code it was
// written as, so its code object is unchanged. (A function template over an accessor object, measured: the same logic, but another
// instruction order and register numbering in that kernel.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hb {
__device__ __forceinline__ void wave_add(unsigned int* c, unsigned long long mask, int lane) {
  if (mask && lane == 0) atomicAdd(c, static_cast<unsigned int>(__popcll(mask)));
}
}  // namespace hb

// What one game contributes to the counters on this turn; a finished game, or a lane without a game, keeps these values.
#define HB_TALLY_VARS              \
  int kind = -1, bin = 0;          \
  bool ended = false, misplay = false, bomb = false;

// The tally of one game (the body of a block of its own, after HB_TALLY_VARS). DONE: the game's status byte (bit 7 = finished,
// bits 0-6 = lives lost); ACTION, REWARD, TERMINAL, SCORE: the move just stepped and that step's outputs, each evaluated only where
// the tally needs it; FINISH(score, length, status): statements run on the turn the game ends; SET_DONE(status): after a misplay
// that does not end it. A_, H_, P_, C_: actions, hand size, players, colours; B_: score bins; MAX_LIFE; TURN.
#define HB_TALLY_GAME(A_, H_, P_, C_, B_, MAX_LIFE, TURN, DONE, ACTION, REWARD, TERMINAL, SCORE, FINISH, SET_DONE)                        \
  const uint8_t st = (DONE);                                                                                                              \
  if (!(st & 0x80u)) {   /* a game counts only while it is live: finished games' env outputs are never read */                            \
    const int u = (ACTION);                                                                                                               \
    if (u >= 0 && u < (A_)) kind = u < (H_) ? 0 : u < 2 * (H_) ? 1 : u < 2 * (H_) + ((P_) - 1) * (C_) ? 2 : 3;   /* App. A.2 order */     \
    misplay = kind == 1 && (REWARD) <= 0.f;   /* a successful play always scores +1; a misplay 0, or -score at a bomb-out */              \
    const int lost = (st & 0x7f) + (misplay ? 1 : 0);                                                                                     \
    ended = (TERMINAL) != 0;                                                                                                              \
    if (ended) {                                                                                                                          \
      const int sc = (SCORE);   /* 0 after a bomb-out (hb_env_step) */                                                                    \
      bin = sc < 0 ? 0 : sc > (B_) - 1 ? (B_) - 1 : sc;                                                                                   \
      bomb = lost >= (MAX_LIFE);                                                                                                          \
      FINISH(static_cast<int8_t>(sc), static_cast<int16_t>((TURN) + 1), static_cast<uint8_t>(0x80 | lost));                               \
    } else if (misplay) {                                                                                                                 \
      SET_DONE(static_cast<uint8_t>(lost));                                                                                               \
    }                                                                                                                                     \
  }

// The wavefront's ballots over its 64 lanes' HB_TALLY_VARS into LC, the workgroup's LDS copy of the counters (slot 0 counts the
// games that ended: the kernel subtracts it from the live count at the end). Every lane of the wavefront must reach it.
#define HB_TALLY_WAVE(LC, B_, P_, SEAT, LANE)                                                                                             \
  unsigned long long m = __ballot(ended);                                                                                                 \
  if (m) {                                                                                                                                \
    hb::wave_add((LC), m, (LANE));                                                                                                        \
    hb::wave_add((LC) + 1 + (B_), __ballot(bomb), (LANE));                                                                                \
    while (m) {   /* histogram: one ballot per score that occurs in this wave (wave-uniform loop) */                                      \
      const int b = __shfl(bin, __ffsll(static_cast<unsigned long long>(m)) - 1);                                                         \
      const unsigned long long mb = __ballot(ended && bin == b);                                                                          \
      hb::wave_add((LC) + 1 + b, mb, (LANE));                                                                                             \
      m &= ~mb;                                                                                                                           \
    }                                                                                                                                     \
  }                                                                                                                                       \
  _Pragma("unroll") for (int k = 0; k < 4; ++k) hb::wave_add((LC) + 2 + (B_) + 4 * (SEAT) + k, __ballot(kind == k), (LANE));               \
  hb::wave_add((LC) + 2 + (B_) + 4 * (P_) + (SEAT), __ballot(misplay), (LANE));
