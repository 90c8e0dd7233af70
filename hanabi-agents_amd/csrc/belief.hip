// belief.hip — fictitious states drawn from a public-knowledge belief, and the reduction of the rollouts played from them
// (hanabi_hip/search.py).
//
// hb_belief_determinize: output row o = source row o / replicas with the observing seat's own hand and the undealt deck re-drawn
// from what that seat cannot see (the "pool": its hand's cards, oldest first, then the undealt deck positions ascending; at most
// 5 + 50 - 2 * 5 = 45 elements, one per lane). ONE wavefront per output row, everything in registers: lane j < SW holds word j of
// the row, lane l < npool holds pool element l; scalars travel by v_readlane, the hand slots are drawn with one ballot each
// (sequential importance sampling: the weight is the product of the candidate counts), the rest of the pool is shuffled onto the
// undealt deck positions by ranking distinct random keys (refill_kernel's shuffle, env_kernel.hpp). Waves share nothing: no LDS,
// no barrier.
//
// hb_search_reduce: per root, sum of weight * score and of weight over the replicas of every action in 64-bit integers (the
// result does not depend on the order of summation), one division per (root, action), and the arg-max over the legal actions.
//
// hb_search_layout: the determinized rows copied into the [m, C, replicas] rollout games of a per-root candidate list, with each
// game's forced first move and its "not played" mark. ONE wavefront per (root, replica): lane j < SW holds word j of the row and
// stores it C times, coalesced. hb_search_compare: per root, every candidate's paired difference to a baseline candidate over the
// shared replicas, and that difference's standard error; one wavefront per root like hb_search_reduce. Neither uses LDS, a
// barrier or an atomic.
//
// hb_belief_splice_alive / hb_belief_select_depth: the belief conditioned on the partner's last `depth` moves. Splice-alive: an
// earlier state's rows with the observer's hand rebuilt from each candidate, candidate-major (one wavefront per output row, a
// coalesced copy): the cards of that hand the observer still holds (the `alive` slots) are a prefix of the candidate's hand in
// the same order, the others are public and stay the previous row's (the lane of the hand word walks the 5 slots in registers).
// Select-depth: per root the first `replicas` candidates whose hypothetical partner moves reproduce the most leading real ones
// (a candidate's pass count = its leading matches; survivors of the deepest level that has any), ranked by ballot and prefix
// popcount (one wavefront per root, rows copied with lane j < SW holding word j). No LDS, barrier or atomic either.
// hb_belief_splice = splice-alive with alive NULL (the state the partner just moved from: every slot alive);
// hb_belief_select = select-depth with depth 1: the same two kernels.
//
// hb_belief_select_soft: select-depth's inputs read as a likelihood instead of a filter: every candidate weighs its importance
// weight times the product of P(real move | hypothetical move, legal moves) over the usable entries, quantised to integers, and the
// replicas are drawn in proportion (Philox, integer prefix sums: one wavefront per root, see the kernel). No LDS, barrier or atomic.
//
// hb_belief_history_step: a PartnerHistory (the [depth, m] stack of states the partner moved from, with its moves, alive masks and
// valid flags) advanced by one turn in place: own move out of the alive masks, reset of re-dealt games, push of a new entry. One
// launch; rows move as contiguous 16-byte items, the byte fields one game per lane (see the kernel).
//
// hb_belief_carry: the hand samples of my previous turn carried to my present one (range tracking, sampled): the card I played
// leaves the sample, the others keep their slots if the pool and the hints since still allow them, the new card and the deck are
// the determinizer's own draw, and the weight counts the copies of the card the partner drew. One wavefront per output row, like
// hb_belief_determinize, with which it shares the slot draw and the deck shuffle. No LDS, barrier or atomic.
//
// hb_belief_score: any of these beliefs scored against the cards the seat really holds: per slot the weight of the replicas that
// hold the true card (and, on request, of every card), the weight of those that hold the whole hand, and the card-counting prior
// read from the true row alone. One wavefront per root, 64-bit integer sums, no float arithmetic; no LDS, barrier or atomic.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/hanabi_hip.h"
#include "common.hpp"
#include "env_kernel.hpp"  // hb::philox4x32_10

namespace {

struct DetArgs {
  const uint32_t* src;
  uint32_t* out;
  uint32_t* weight;
  long long n_out, first_row;
  unsigned long long seed, draw;
  int replicas, seat, P, C, R, H, D, SW;
};

__device__ __forceinline__ uint32_t lane_read(uint32_t v, int l) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), l));
}

// One hand slot of the sequential importance sampler: `cand` marks this lane's pool element as free and plausible for the slot.
// Returns n = the number of candidates (0: none, nothing is taken); otherwise the k-th candidate in pool order, k = (u * n) >> 32,
// is marked in `taken` and its lane returned in idx.
__device__ __forceinline__ uint32_t draw_slot(bool cand, uint32_t u, int lane, unsigned long long& taken, int& idx) {
  const unsigned long long mask = __ballot(cand);
  const uint32_t n = static_cast<uint32_t>(__popcll(mask));
  idx = -1;
  if (n == 0) return 0u;
  const uint32_t k = static_cast<uint32_t>((static_cast<uint64_t>(u) * n) >> 32);
  const uint32_t before = static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
  idx = __ffsll(static_cast<unsigned long long>(__ballot(cand && before == k))) - 1;
  taken |= 1ull << idx;
  return n;
}

// The redrawn row: the pool elements not in `taken` go onto the undealt deck positions by the rank of a distinct random key
// (element l: (v_l & ~63) | l), lane hand_lane's word becomes new_hand, every other word stays the source's (wj).
__device__ __forceinline__ void store_redrawn(uint32_t wj, uint32_t card, uint32_t v, bool in_pool, unsigned long long taken, int lane,
                                              int W_DECK, int deck_pos, int D, int SW, int hand_lane, uint32_t new_hand, uint32_t* dst) {
  const unsigned long long rest = __ballot(in_pool && !((taken >> lane) & 1ull));
  const uint32_t key = (v & ~63u) | static_cast<uint32_t>(lane);
  int rank = 0;
  for (unsigned long long todo = rest; todo; todo &= todo - 1) {
    const uint32_t ki = lane_read(key, __ffsll(todo) - 1);
    rank += ki < key ? 1 : 0;
  }
  const int dest = deck_pos + rank;   // (meaningful in the lanes of `rest`)
  const int j = lane - W_DECK;   // deck word of this lane (bytes 4j .. 4j + 3), if 0 <= j < ceil(D / 4)
  uint32_t neww = wj;
  if (j >= 0 && 4 * j < D) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int p = 4 * j + b;
      if (p >= deck_pos && p < D) neww &= ~(255u << (8 * b));
    }
  }
  for (unsigned long long todo = rest; todo; todo &= todo - 1) {
    const int l = __ffsll(todo) - 1;
    const int d = static_cast<int>(lane_read(static_cast<uint32_t>(dest), l));
    const uint32_t c = lane_read(card, l);
    if ((d >> 2) == j) neww |= c << (8 * (d & 3));
  }
  if (lane == hand_lane) neww = new_hand;
  if (lane < SW) dst[lane] = neww;
}

__global__ void __launch_bounds__(256) belief_determinize_kernel(DetArgs a) {
  const int lane = threadIdx.x & 63;
  const long long o = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);   // output row of this wavefront
  if (o >= a.n_out) return;
  const long long i = o / a.replicas;
  const uint32_t wj = lane < a.SW ? a.src[i * a.SW + lane] : 0u;
  uint32_t* const dst = a.out + o * a.SW;
  const uint32_t w0 = lane_read(wj, 0), w1 = lane_read(wj, 1);
  const int seat = a.seat < 0 ? static_cast<int>((w0 >> 13) & 7u) : a.seat;
  if (((w0 >> 19) & 3u) != 0 || seat >= a.P) {   // not running (or no such seat): an unchanged copy that weighs nothing
    if (lane < a.SW) dst[lane] = wj;
    if (lane == 0) a.weight[o] = 0u;
    return;
  }
  const int W_DECK = 10 + 3 * a.P;
  const uint32_t hand = lane_read(wj, 10 + seat);
  const uint64_t know = (static_cast<uint64_t>(lane_read(wj, 10 + a.P + 2 * seat + 1)) << 32) | lane_read(wj, 10 + a.P + 2 * seat);
  const int n_hand = min(static_cast<int>((w1 >> (15 + 3 * seat)) & 7u), a.H);
  const int deck_size = min(static_cast<int>(w0 & 63u), a.D);
  const int deck_pos = a.D - deck_size;
  const int npool = n_hand + deck_size;

  // pool element of this lane: a hand slot, or the deck byte at position q (fetched from the lane that holds its word)
  const int q = deck_pos + lane - n_hand;
  const uint32_t wq = static_cast<uint32_t>(__shfl(static_cast<int>(wj), (W_DECK + (q >> 2)) & 63));
  const uint32_t card = lane < n_hand ? (hand >> (5 * lane)) & 31u : (wq >> (8 * (q & 3))) & 255u;
  const bool in_pool = lane < npool;
  const uint32_t col = card / static_cast<uint32_t>(a.R), rk = card - col * static_cast<uint32_t>(a.R);
  const bool card_ok = in_pool && col < static_cast<uint32_t>(a.C);

  const unsigned long long row_id = static_cast<unsigned long long>(a.first_row + o);
  uint32_t rnd[4];
  hb::philox4x32_10(128u + static_cast<uint32_t>(lane), static_cast<uint32_t>(a.draw), static_cast<uint32_t>(row_id),
                    static_cast<uint32_t>(row_id >> 32), static_cast<uint32_t>(a.seed),
                    static_cast<uint32_t>(a.seed >> 32) ^ static_cast<uint32_t>(a.draw >> 32), rnd);

  // ---- the hand, slot by slot: ballot of the free plausible pool elements, take the k-th -------------------------------------
  unsigned long long taken = 0;
  uint32_t weight = 1u, new_hand = hand;
  bool dead = false;
  for (int s = 0; s < n_hand; ++s) {
    const uint32_t kn = static_cast<uint32_t>(know >> (12 * s)) & 0xFFFu;
    const bool cand = card_ok && !((taken >> lane) & 1ull) && ((kn >> col) & 1u) && ((kn >> (5u + rk)) & 1u);
    int idx;
    const uint32_t n = draw_slot(cand, lane_read(rnd[0], s), lane, taken, idx);
    if (n == 0) {
      dead = true;
      break;
    }
    weight *= n;
    new_hand = (new_hand & ~(31u << (5 * s))) | (lane_read(card, idx) << (5 * s));
  }
  if (dead) {
    if (lane < a.SW) dst[lane] = wj;
    if (lane == 0) a.weight[o] = 0u;
    return;
  }
  store_redrawn(wj, card, rnd[1], in_pool, taken, lane, W_DECK, deck_pos, a.D, a.SW, 10 + seat, new_hand, dst);
  if (lane == 0) a.weight[o] = weight;
}

struct CarryArgs {
  const uint32_t* cur;
  const uint32_t* old_rows;
  const uint32_t* old_weight;
  const int32_t* own_slot;
  const int32_t* revealed;
  const int32_t* drew;
  uint32_t* out;
  uint32_t* weight;
  long long n_out, first_row;
  unsigned long long seed, draw;
  int K, seat, P, C, R, H, D, SW;
};

// hb_belief_carry: particle (i, k) of my previous turn carried to my present one (the rule is in include/hanabi_hip.h). One
// wavefront per output row, laid out like belief_determinize_kernel: lane j < SW holds word j of cur row i, lane l < npool pool
// element l. The kept cards take their pool elements by ballot and find-first, the new slots and the deck are the determinizer's
// own steps with its Philox words. Every decision is wave-uniform; no LDS, no atomics.
__global__ void __launch_bounds__(256) belief_carry_kernel(CarryArgs a) {
  const int lane = threadIdx.x & 63;
  const long long o = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);   // output row of this wavefront
  if (o >= a.n_out) return;
  const long long i = o / a.K;
  const uint32_t wj = lane < a.SW ? a.cur[i * a.SW + lane] : 0u;
  uint32_t* const dst = a.out + o * a.SW;
  const uint32_t w0 = lane_read(wj, 0), w1 = lane_read(wj, 1);
  const int seat = a.seat;
  const uint32_t old_hand = a.old_rows[o * a.SW + 10 + seat];
  const int slot = a.own_slot[i], drw = a.drew[i];
  const uint32_t rev = static_cast<uint32_t>(a.revealed[i]);
  const int W_DECK = 10 + 3 * a.P;
  const uint32_t hand = lane_read(wj, 10 + seat);
  const uint64_t know = (static_cast<uint64_t>(lane_read(wj, 10 + a.P + 2 * seat + 1)) << 32) | lane_read(wj, 10 + a.P + 2 * seat);
  const int n_hand = min(static_cast<int>((w1 >> (15 + 3 * seat)) & 7u), a.H);
  const int deck_size = min(static_cast<int>(w0 & 63u), a.D);
  const int deck_pos = a.D - deck_size;
  const int npool = n_hand + deck_size;

  // ---- steps 1 and 2: usable at all; the card I played leaves the old hand, the others are kept oldest first ------------------
  bool dead = a.old_weight[o] == 0u || ((w0 >> 19) & 3u) != 0 || static_cast<int>((w0 >> 13) & 7u) != seat;
  if (slot >= 0) dead = dead || slot >= a.H || ((old_hand >> (5 * min(slot, 4))) & 31u) != rev;
  uint32_t kept = 0;
  int n_kept = 0;
  for (int s = 0; s < a.H; ++s) {
    const uint32_t f = (old_hand >> (5 * s)) & 31u;
    if (s != slot && f != 31u) {
      kept |= f << (5 * n_kept);
      ++n_kept;
    }
  }
  dead = dead || n_kept > n_hand;

  // ---- step 3: the pool element of this lane, as in belief_determinize_kernel ---------------------------------------------------
  const int q = deck_pos + lane - n_hand;
  const uint32_t wq = static_cast<uint32_t>(__shfl(static_cast<int>(wj), (W_DECK + (q >> 2)) & 63));
  const uint32_t card = lane < n_hand ? (hand >> (5 * lane)) & 31u : (wq >> (8 * (q & 3))) & 255u;
  const bool in_pool = lane < npool;
  const uint32_t col = card / static_cast<uint32_t>(a.R), rk = card - col * static_cast<uint32_t>(a.R);
  const bool card_ok = in_pool && col < static_cast<uint32_t>(a.C);

  unsigned long long taken = 0;
  uint32_t weight = 1u, new_hand = hand;
  // ---- step 4: kept slot s takes the first free pool element of its card, if the slot's knowledge now allows that card ---------
  for (int s = 0; s < n_kept && !dead; ++s) {
    const uint32_t c = (kept >> (5 * s)) & 31u;
    const uint32_t kn = static_cast<uint32_t>(know >> (12 * s)) & 0xFFFu;
    const uint32_t cc = c / static_cast<uint32_t>(a.R), cr = c - cc * static_cast<uint32_t>(a.R);
    const bool allowed = cc < static_cast<uint32_t>(a.C) && ((kn >> cc) & 1u) && ((kn >> (5u + cr)) & 1u);
    const unsigned long long mask = __ballot(in_pool && !((taken >> lane) & 1ull) && card == c);
    if (!allowed || mask == 0) {
      dead = true;
      break;
    }
    taken |= 1ull << (__ffsll(mask) - 1);
    new_hand = (new_hand & ~(31u << (5 * s))) | (c << (5 * s));
  }
  // ---- step 5: the partner's visible draw: its copies still in the hypothesis's pool, plus the one the partner took ------------
  if (!dead && drw >= 0)
    weight += static_cast<uint32_t>(__popcll(__ballot(in_pool && !((taken >> lane) & 1ull) && card == static_cast<uint32_t>(drw))));

  // ---- step 6: the new slots, the determinizer's step with the determinizer's random words -------------------------------------
  const unsigned long long row_id = static_cast<unsigned long long>(a.first_row + o);
  uint32_t rnd[4];
  hb::philox4x32_10(128u + static_cast<uint32_t>(lane), static_cast<uint32_t>(a.draw), static_cast<uint32_t>(row_id),
                    static_cast<uint32_t>(row_id >> 32), static_cast<uint32_t>(a.seed),
                    static_cast<uint32_t>(a.seed >> 32) ^ static_cast<uint32_t>(a.draw >> 32), rnd);
  for (int s = n_kept; s < n_hand && !dead; ++s) {
    const uint32_t kn = static_cast<uint32_t>(know >> (12 * s)) & 0xFFFu;
    const bool cand = card_ok && !((taken >> lane) & 1ull) && ((kn >> col) & 1u) && ((kn >> (5u + rk)) & 1u);
    int idx;
    const uint32_t n = draw_slot(cand, lane_read(rnd[0], s), lane, taken, idx);
    if (n == 0) {
      dead = true;
      break;
    }
    weight *= n;
    new_hand = (new_hand & ~(31u << (5 * s))) | (lane_read(card, idx) << (5 * s));
  }
  if (dead) {
    if (lane < a.SW) dst[lane] = wj;
    if (lane == 0) a.weight[o] = 0u;
    return;
  }
  // ---- steps 7 and 8 ---------------------------------------------------------------------------------------------------------------
  store_redrawn(wj, card, rnd[1], in_pool, taken, lane, W_DECK, deck_pos, a.D, a.SW, 10 + seat, new_hand, dst);
  if (lane == 0) a.weight[o] = weight;
}

// 64-bit sum over the wavefront (xor butterfly on the two halves: every lane ends with the total)
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(v)), off));
    const uint32_t hi = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(static_cast<unsigned long long>(v) >> 32)), off));
    v += static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo);
  }
  return v;
}

// One wavefront per root: the replicas' weights are summed once (every action of a root starts from the same replicas), then
// sum of weight * score per legal action, lanes striding over the replicas.
__global__ void __launch_bounds__(256) search_reduce_kernel(const int8_t* __restrict__ score, const uint32_t* __restrict__ weight,
                                                            const int8_t* __restrict__ legal, long long m, int A, int R,
                                                            float* __restrict__ value, long long* __restrict__ wsum,
                                                            int32_t* __restrict__ n_live, int32_t* __restrict__ best) {
  const int lane = threadIdx.x & 63;
  const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= m) return;
  const uint32_t* w = weight + i * R;
  long long sw = 0, nl = 0;
  for (int r = lane; r < R; r += 64) {
    const uint32_t v = w[r];
    sw += v;
    nl += v != 0u ? 1 : 0;
  }
  sw = wave_sum(sw);
  nl = wave_sum(nl);
  float best_v = -INFINITY;
  int best_a = -1;
  for (int act = 0; act < A; ++act) {
    const bool ok = legal[i * A + act] != 0 && sw > 0;   // (wave-uniform)
    long long num = 0;
    if (ok) {
      const int8_t* s = score + (i * A + act) * static_cast<long long>(R);
      for (int r = lane; r < R; r += 64) num += static_cast<long long>(w[r]) * s[r];
      num = wave_sum(num);
    }
    const float v = ok ? static_cast<float>(static_cast<double>(num) / static_cast<double>(sw)) : NAN;
    if (ok && v > best_v) {   // strict: the lowest uid wins ties
      best_v = v;
      best_a = act;
    }
    if (lane == 0) {
      value[i * A + act] = v;
      wsum[i * A + act] = ok ? sw : 0;
      n_live[i * A + act] = ok ? static_cast<int32_t>(nl) : 0;
    }
  }
  if (best && lane == 0) best[i] = best_a;
}

struct LayoutArgs {
  const uint32_t* det;
  const uint32_t* weight;
  const int32_t* cand;
  const int32_t* filler;
  uint32_t* rows;
  int32_t* forced;
  uint8_t* done;
  int32_t* n_played;
  long long n_src;   // m * R
  int C, R, SW;
};

// One wavefront per (root i, replica r): source row i * R + r goes to games (i * C + c) * R + r, c = 0 .. C - 1. The wavefront of
// replica 0 also counts the root's played games: (candidates >= 0) * (replicas of weight != 0).
__global__ void __launch_bounds__(256) search_layout_kernel(LayoutArgs a) {
  const int lane = threadIdx.x & 63;
  const long long o = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);   // source row of this wavefront
  if (o >= a.n_src) return;
  const long long i = o / a.R;
  const int r = static_cast<int>(o - i * a.R);
  const uint32_t wj = lane < a.SW ? a.det[o * a.SW + lane] : 0u;
  const bool live = a.weight[o] != 0u;
  const int32_t fill = a.filler[i];
  const int32_t* cand = a.cand + i * a.C;
  for (int c = 0; c < a.C; ++c) {
    const int32_t uid = cand[c];   // (wave-uniform)
    const bool played = uid >= 0 && live;
    const long long g = (i * a.C + c) * a.R + r;
    if (lane < a.SW) a.rows[g * a.SW + lane] = wj;
    if (lane == 0) {
      a.forced[g] = uid >= 0 ? uid : fill;   // (a dead replica is a copy of its root: the candidate is as legal there)
      a.done[g] = played ? 0 : 0x80;
    }
  }
  if (r == 0) {
    const int n_cand = __popcll(__ballot(lane < a.C && cand[lane < a.C ? lane : 0] >= 0));
    long long nl = 0;
    for (int q = lane; q < a.R; q += 64) nl += a.weight[o + q] != 0u ? 1 : 0;
    nl = wave_sum(nl);
    if (lane == 0) a.n_played[i] = static_cast<int32_t>(nl * n_cand);
  }
}

// double sum over the wavefront (the butterfly of wave_sum: every lane ends with the same total)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(v));
    const uint32_t lo = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(b)), off));
    const uint32_t hi = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(b >> 32)), off));
    v += __longlong_as_double(static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo));
  }
  return v;
}

// One wavefront per root. d_r = score[c][r] - score[base][r] over the replicas of weight > 0: mu = sum w d / sum w from exact
// integer sums; then a second pass in double over the non-negative terms (w (d - mu))^2, each lane adding its replicas in
// ascending order, stride 64. se = sqrt(sum) / sum w * sqrt(n / (n - 1)): with constant weights the s / sqrt(n) of the d_r.
__global__ void __launch_bounds__(256) search_compare_kernel(const int8_t* __restrict__ score, const uint32_t* __restrict__ weight,
                                                             const int32_t* __restrict__ cand, const int32_t* __restrict__ base_slot,
                                                             long long m, int C, int R, double* __restrict__ diff,
                                                             double* __restrict__ se, int32_t* __restrict__ n_pair) {
  const int lane = threadIdx.x & 63;
  const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= m) return;
  const uint32_t* w = weight + i * R;
  long long sw = 0, nl = 0;
  for (int r = lane; r < R; r += 64) {
    const uint32_t v = w[r];
    sw += v;
    nl += v != 0u ? 1 : 0;
  }
  sw = wave_sum(sw);
  nl = wave_sum(nl);
  if (lane == 0) n_pair[i] = static_cast<int32_t>(nl);
  int base = base_slot[i];
  if (base >= C) base = -1;   // (no such slot: no baseline)
  const bool root_ok = base >= 0 && sw > 0 && cand[i * C + (base >= 0 ? base : 0)] >= 0;   // (wave-uniform)
  const int8_t* sb = score + (i * C + (base >= 0 ? base : 0)) * static_cast<long long>(R);
  const double dsw = static_cast<double>(sw);
  for (int c = 0; c < C; ++c) {
    double mu = NAN, err = NAN;
    if (root_ok && cand[i * C + c] >= 0) {
      if (c == base) {
        mu = 0.0;
        err = 0.0;
      } else {
        const int8_t* s = score + (i * C + c) * static_cast<long long>(R);
        long long num = 0;
        for (int r = lane; r < R; r += 64) num += static_cast<long long>(w[r]) * (static_cast<int>(s[r]) - static_cast<int>(sb[r]));
        num = wave_sum(num);
        mu = static_cast<double>(num) / dsw;
        err = INFINITY;
        if (nl >= 2) {
          double acc = 0.0;
          for (int r = lane; r < R; r += 64) {
            const double t = static_cast<double>(w[r]) * (static_cast<double>(static_cast<int>(s[r]) - static_cast<int>(sb[r])) - mu);
            acc += t * t;
          }
          acc = wave_sum_f64(acc);
          err = sqrt(acc) / dsw * sqrt(static_cast<double>(nl) / static_cast<double>(nl - 1));
        }
      }
    }
    if (lane == 0) {
      diff[i * C + c] = mu;
      se[i * C + c] = err;
    }
  }
}

struct SpliceAliveArgs {
  const uint32_t* prev;
  const uint8_t* alive;   // may be null: every slot alive
  const uint32_t* det;
  uint32_t* out;
  long long m, n_out;   // n_out = K * m
  int K, SW, hand_word;
};

// One wavefront per output row o = k * m + i, lane j < SW moves word j of previous row i. The lane of the hand word rebuilds it:
// over the occupied slots s of the previous hand, an alive slot takes the next card of candidate (i, k)'s hand (slot j = the
// number of alive slots before it: what is still held is a prefix of the current hand, in the same order); a dead slot, or one
// the candidate has no card left for, keeps the previous row's card.
__global__ void __launch_bounds__(256) belief_splice_alive_kernel(SpliceAliveArgs a) {
  const int lane = threadIdx.x & 63;
  const long long o = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (o >= a.n_out || lane >= a.SW) return;
  const long long k = o / a.m, i = o - k * a.m;
  uint32_t w = a.prev[i * a.SW + lane];
  if (lane == a.hand_word) {
    const uint32_t ch = a.det[(i * a.K + k) * a.SW + lane];
    const uint32_t alive = a.alive ? a.alive[i] : 0xFFu;
    int j = 0;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const uint32_t c = (ch >> (5 * j)) & 31u;   // (j <= s <= 4)
      const bool take = ((w >> (5 * s)) & 31u) != 31u && ((alive >> s) & 1u) && c != 31u;
      if (take) {
        w = (w & ~(31u << (5 * s))) | (c << (5 * s));
        ++j;
      }
    }
  }
  a.out[o * a.SW + lane] = w;
}

struct SelectDepthArgs {
  const uint32_t* src;
  const uint32_t* det;
  const uint32_t* weight;
  const int32_t* hyp;      // [depth][K * m]
  const int32_t* actual;   // [depth][m]
  const uint8_t* valid;    // [depth][m]; may be null: every entry valid
  uint32_t* out;
  uint32_t* out_weight;
  int32_t* n_surv;         // [depth][m]
  int32_t* depth_used;     // may be null: not written
  uint8_t* fallback;
  long long m;
  int K, R, SW, depth;
};

constexpr int MAX_DEPTH = 8;

// One wavefront per root. L = the leading valid entries of the root (0 when it is not running). Sweep 1: every lane's candidate
// stays `on` while its moves match, from entry 0 (never, for a weight of 0); cnt[D - 1] = candidates with at least D leading
// matches, by ballot over 64 candidates at a time. used = the deepest level with a survivor (cnt never grows with D). Sweep 2
// copies the first R candidates with at least `used` leading matches in candidate order, each one's rank = running base + prefix
// popcount of its chunk's ballot. Everything that decides a branch is wave-uniform. The loops over the levels are unrolled to
// MAX_DEPTH with wave-uniform guards, so that act[] and cnt[] stay in registers.
__global__ void __launch_bounds__(256) belief_select_depth_kernel(SelectDepthArgs a) {
  const int lane = threadIdx.x & 63;
  const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= a.m) return;
  const uint32_t* det = a.det + i * a.K * a.SW;
  const uint32_t* w = a.weight + i * a.K;
  uint32_t* out = a.out + i * a.R * a.SW;
  uint32_t* ow = a.out_weight + i * a.R;
  const long long slab = static_cast<long long>(a.K) * a.m;
  const bool running = ((a.src[i * a.SW] >> 19) & 3u) == 0;
  int L = 0;
  if (running) {
    while (L < a.depth && (!a.valid || a.valid[L * a.m + i] != 0)) ++L;
  }
  int32_t act[MAX_DEPTH];
  int cnt[MAX_DEPTH];
#pragma unroll
  for (int d = 0; d < MAX_DEPTH; ++d) {
    act[d] = d < L ? a.actual[d * a.m + i] : 0;
    cnt[d] = 0;
  }
  for (int k0 = 0; k0 < a.K && L > 0; k0 += 64) {
    const int k = k0 + lane;
    const bool live = k < a.K && w[k] != 0u;
    bool on = live;
#pragma unroll
    for (int d = 0; d < MAX_DEPTH; ++d) {
      if (d < L) {   // (wave-uniform)
        on = on && a.hyp[d * slab + k * a.m + i] == act[d];   // (read by the lanes still matching only)
        cnt[d] += __popcll(__ballot(on));
      }
    }
  }
  int used = 0;
#pragma unroll
  for (int d = 0; d < MAX_DEPTH; ++d) used += cnt[d] > 0 ? 1 : 0;
  int total = 0;
#pragma unroll
  for (int d = 0; d < MAX_DEPTH; ++d) {
    if (d < a.depth && lane == 0) a.n_surv[d * a.m + i] = cnt[d];
    total = d + 1 == used ? cnt[d] : total;
  }
  if (lane == 0) {
    if (a.depth_used) a.depth_used[i] = used;
    a.fallback[i] = L == 0 ? 2 : used == 0 ? 1 : 0;
  }
  if (used == 0) {   // the unconditioned belief: candidates 0 .. R - 1 as they are
    for (int r = 0; r < a.R; ++r)
      if (lane < a.SW) out[r * a.SW + lane] = det[r * a.SW + lane];
    for (int r = lane; r < a.R; r += 64) ow[r] = w[r];
    return;
  }
  int base = 0;
  for (int k0 = 0; k0 < a.K && base < a.R; k0 += 64) {
    const int k = k0 + lane;
    const uint32_t wk = k < a.K ? w[k] : 0u;
    bool s = wk != 0u;   // (k >= K: wk = 0, nothing is read)
#pragma unroll
    for (int d = 0; d < MAX_DEPTH; ++d) {
      if (d < used) s = s && a.hyp[d * slab + k * a.m + i] == act[d];
    }
    const unsigned long long mask = __ballot(s);
    const int rank = base + __popcll(mask & ((1ull << lane) - 1ull));
    if (s && rank < a.R) ow[rank] = wk;
    int r = base;
    for (unsigned long long todo = mask; todo && r < a.R; todo &= todo - 1, ++r) {
      const int kk = k0 + __ffsll(todo) - 1;
      if (lane < a.SW) out[r * a.SW + lane] = det[kk * a.SW + lane];
    }
    base += __popcll(mask);
  }
  const uint32_t sj = lane < a.SW ? a.src[i * a.SW + lane] : 0u;
  for (int r = total; r < a.R; ++r) {   // fewer survivors than replicas: dead copies of the root
    if (lane < a.SW) out[r * a.SW + lane] = sj;
    if (lane == 0) ow[r] = 0u;
  }
}

struct SelectSoftArgs {
  const uint32_t* src;
  const uint32_t* det;
  const uint32_t* weight;
  const int32_t* hyp;       // [depth][K * m]
  const int32_t* n_legal;   // [depth][K * m]
  const int32_t* actual;    // [depth][m]
  const uint8_t* valid;     // [depth][m]; may be null: every entry valid
  const double* p_table;    // [2][A + 1]
  uint32_t* out;
  uint32_t* out_weight;
  int32_t* n_surv;          // [depth][m]
  int32_t* depth_used;
  uint8_t* fallback;
  float* ess;
  long long m, first_row;
  unsigned long long seed, draw;
  int K, R, SW, depth, A;
};

// 64-bit values across the wavefront, as two 32-bit halves
__device__ __forceinline__ unsigned long long lane_read64(unsigned long long v, int l) {
  return (static_cast<unsigned long long>(lane_read(static_cast<uint32_t>(v >> 32), l)) << 32) | lane_read(static_cast<uint32_t>(v), l);
}

// inclusive prefix sum over the wavefront (six shuffle-up steps)
__device__ __forceinline__ unsigned long long wave_scan(unsigned long long v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t lo = static_cast<uint32_t>(__shfl_up(static_cast<int>(static_cast<uint32_t>(v)), off));
    const uint32_t hi = static_cast<uint32_t>(__shfl_up(static_cast<int>(static_cast<uint32_t>(v >> 32)), off));
    if (lane >= off) v += (static_cast<unsigned long long>(hi) << 32) | lo;
  }
  return v;
}

// the largest of a non-negative double over the wavefront (exact: no rounding, so no order)
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(v));
    const uint32_t lo = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(b)), off));
    const uint32_t hi = static_cast<uint32_t>(__shfl_xor(static_cast<int>(static_cast<uint32_t>(b >> 32)), off));
    const double o = __longlong_as_double(static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo));
    v = o > v ? o : v;
  }
  return v;
}

// The likelihood of this lane's candidate k of root i: the product over the entries d < L, in that order, of
// p_table[hyp == actual ? 0 : 1][n_legal]; 0 for a candidate that is not live or has an n_legal outside 1 .. A. `lead` = its
// leading matches. Multiplications only. The loop is unrolled to MAX_DEPTH with wave-uniform guards, as its callers' are.
__device__ __forceinline__ double soft_likelihood(const SelectSoftArgs& a, long long i, long long slab, int k, bool live, int L,
                                                  const int32_t (&act)[MAX_DEPTH], int& lead) {
  double lik = live ? 1.0 : 0.0;
  bool on = live;
  lead = 0;
#pragma unroll
  for (int d = 0; d < MAX_DEPTH; ++d) {
    if (d < L && live) {   // (d < L is wave-uniform)
      const long long at = d * slab + static_cast<long long>(k) * a.m + i;
      const bool match = a.hyp[at] == act[d];
      const int n = a.n_legal[at];
      const bool n_ok = n >= 1 && n <= a.A;
      lik *= n_ok ? a.p_table[(match ? 0 : a.A + 1) + n] : 0.0;
      on = on && match;
      lead += on ? 1 : 0;
    }
  }
  return lik;
}

// W_k = w_k * floor(lik_k / mx * 2^24) in 64-bit integers; 0 when mx == 0
__device__ __forceinline__ unsigned long long soft_weight(uint32_t wk, double lik, double mx) {
  if (!(mx > 0.0)) return 0ull;
  return static_cast<unsigned long long>(wk) * static_cast<unsigned long long>(floor(lik / mx * 16777216.0));
}

// One wavefront per root, candidates 64 at a time, one per lane. L = the leading valid entries of the root (0 when it is not
// running). Sweep 1: every candidate's likelihood; their largest (mx) and, by ballot, cnt[D - 1] = the candidates with at least D
// leading matches. Sweep 2: W_k, their integer sum T and the f64 sum of their squares. Then the outputs, 64 at a time, output r
// in lane r: its Philox target in [0, T), and sweep 3 over the candidates with an inclusive integer scan of W per chunk on a
// running base: output r belongs to the chunk with base <= target < base + chunk sum, and its candidate is the first lane whose
// prefix exceeds the target (ballot, find-first; such a lane has W > 0, hence k < K). Everything that decides a branch is
// wave-uniform; the likelihoods are recomputed per sweep instead of kept (K may be 64 chunks), so nothing is indexed dynamically.
__global__ void __launch_bounds__(256) belief_select_soft_kernel(SelectSoftArgs a) {
  const int lane = threadIdx.x & 63;
  const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= a.m) return;
  const uint32_t* det = a.det + i * a.K * a.SW;
  const uint32_t* w = a.weight + i * a.K;
  uint32_t* out = a.out + i * a.R * a.SW;
  uint32_t* ow = a.out_weight + i * a.R;
  const long long slab = static_cast<long long>(a.K) * a.m;
  const bool running = ((a.src[i * a.SW] >> 19) & 3u) == 0;
  int L = 0;
  if (running) {
    while (L < a.depth && (!a.valid || a.valid[L * a.m + i] != 0)) ++L;
  }
  int32_t act[MAX_DEPTH];
  int cnt[MAX_DEPTH];
#pragma unroll
  for (int d = 0; d < MAX_DEPTH; ++d) {
    act[d] = d < L ? a.actual[d * a.m + i] : 0;
    cnt[d] = 0;
  }
  double mx = 0.0;
  for (int k0 = 0; k0 < a.K; k0 += 64) {
    const int k = k0 + lane;
    const bool live = k < a.K && w[k] != 0u;
    int lead;
    const double lik = soft_likelihood(a, i, slab, k, live, L, act, lead);
    mx = lik > mx ? lik : mx;
#pragma unroll
    for (int d = 0; d < MAX_DEPTH; ++d) {
      if (d < L) cnt[d] += __popcll(__ballot(live && lead > d));
    }
  }
  mx = wave_max_f64(mx);
  unsigned long long T = 0;
  double sq = 0.0;
  for (int k0 = 0; k0 < a.K; k0 += 64) {
    const int k = k0 + lane;
    const uint32_t wk = k < a.K ? w[k] : 0u;
    int lead;
    const double lik = soft_likelihood(a, i, slab, k, wk != 0u, L, act, lead);
    const unsigned long long W = soft_weight(wk, lik, mx);
    T += W;
    sq += static_cast<double>(W) * static_cast<double>(W);
  }
  T = static_cast<unsigned long long>(wave_sum(static_cast<long long>(T)));
  sq = wave_sum_f64(sq);
#pragma unroll
  for (int d = 0; d < MAX_DEPTH; ++d) {
    if (d < a.depth && lane == 0) a.n_surv[d * a.m + i] = cnt[d];
  }
  if (lane == 0) {
    a.depth_used[i] = L;
    a.fallback[i] = L == 0 ? 2 : 0;
    a.ess[i] = T == 0 ? 0.0f : static_cast<float>(static_cast<double>(T) * static_cast<double>(T) / sq);
  }
  if (T == 0) {   // nothing to draw from: dead copies of the root
    const uint32_t sj = lane < a.SW ? a.src[i * a.SW + lane] : 0u;
    for (int r = 0; r < a.R; ++r)
      if (lane < a.SW) out[r * a.SW + lane] = sj;
    for (int r = lane; r < a.R; r += 64) ow[r] = 0u;
    return;
  }
  const unsigned long long row_id = static_cast<unsigned long long>(a.first_row + i);
  for (int r0 = 0; r0 < a.R; r0 += 64) {
    const int nr = min(64, a.R - r0);
    uint32_t rnd[4];
    hb::philox4x32_10(0x10000u + static_cast<uint32_t>(r0 + lane), static_cast<uint32_t>(a.draw), static_cast<uint32_t>(row_id),
                      static_cast<uint32_t>(row_id >> 32), static_cast<uint32_t>(a.seed),
                      static_cast<uint32_t>(a.seed >> 32) ^ static_cast<uint32_t>(a.draw >> 32), rnd);
    const unsigned long long target = __umul64hi((static_cast<unsigned long long>(rnd[0]) << 32) | rnd[1], T);   // < T
    if (lane < nr) ow[r0 + lane] = 1u;
    unsigned long long base = 0;
    for (int k0 = 0; k0 < a.K; k0 += 64) {
      const int k = k0 + lane;
      const uint32_t wk = k < a.K ? w[k] : 0u;
      int lead;
      const double lik = soft_likelihood(a, i, slab, k, wk != 0u, L, act, lead);
      const unsigned long long incl = base + wave_scan(soft_weight(wk, lik, mx), lane);
      const unsigned long long end = lane_read64(incl, 63);
      if (end != base) {
        for (int j = 0; j < nr; ++j) {
          const unsigned long long t = lane_read64(target, j);
          if (t >= base && t < end) {
            const int kk = k0 + __ffsll(static_cast<unsigned long long>(__ballot(incl > t))) - 1;
            if (lane < a.SW) out[(r0 + j) * a.SW + lane] = det[kk * a.SW + lane];
          }
        }
      }
      base = end;
    }
  }
}

struct HistoryArgs {
  const int32_t* own;     // [m] or null
  const uint8_t* reset;   // [m] or null
  const uint32_t* cur;    // [m, SW] or null: no push
  const uint32_t* prev;   // [m, SW], with cur
  uint32_t* rows;         // [depth, m, SW]
  int32_t* moves;         // [depth, m]
  uint8_t* alive;         // [depth, m]
  uint8_t* valid;         // [depth, m]
  long long m, n_items;   // n_items = m * SW / (words per item): the items of one entry's rows
  unsigned row_blocks;    // the first row_blocks workgroups move rows, the others do the per-game fields
  int depth, seat, SW, P, C, R, H;
};

// One launch, two kinds of workgroup, which touch disjoint memory. Workgroups below row_blocks shift the state rows: an entry's
// [m, SW] rows are one contiguous run of n_items items (V = uint4 where every base is 16-byte aligned, else one word), thread t
// owns item t of EVERY entry, loads entries 0 .. depth - 2 and the new row's item into registers and stores them one entry
// deeper: every load and store of a wavefront is one contiguous run, and no other thread ever touches item t. The other
// workgroups take one game per lane: its `depth` alive and valid bytes and moves live in registers through the three parts (own
// move, reset, push), byte loads and stores of consecutive lanes are consecutive. The loops over the entries are unrolled to
// MAX_DEPTH with uniform guards, so that the arrays stay in registers.
template <typename V>
__global__ void __launch_bounds__(256) belief_history_step_kernel(HistoryArgs a) {
  if (blockIdx.x < a.row_blocks) {
    const long long t = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= a.n_items) return;
    V* const rows = reinterpret_cast<V*>(a.rows);
    V v[MAX_DEPTH - 1];
#pragma unroll
    for (int d = 0; d < MAX_DEPTH - 1; ++d) {
      v[d] = V{};
      if (d + 1 < a.depth) v[d] = rows[d * a.n_items + t];
    }
    const V fresh = reinterpret_cast<const V*>(a.prev)[t];
#pragma unroll
    for (int d = 0; d < MAX_DEPTH - 1; ++d)
      if (d + 1 < a.depth) rows[(d + 1) * a.n_items + t] = v[d];
    rows[t] = fresh;
    return;
  }
  const long long g = static_cast<long long>(blockIdx.x - a.row_blocks) * 256 + threadIdx.x;
  if (g >= a.m) return;
  uint32_t al[MAX_DEPTH], vl[MAX_DEPTH];
  int32_t mv[MAX_DEPTH];
#pragma unroll
  for (int d = 0; d < MAX_DEPTH; ++d) {
    al[d] = d < a.depth ? a.alive[d * a.m + g] : 0u;
    vl[d] = d < a.depth ? a.valid[d * a.m + g] : 0u;
    mv[d] = d < a.depth && a.cur ? a.moves[d * a.m + g] : 0;
  }
  if (a.own) {   // a play or discard of slot s: the s-th set bit (of bits 0 .. 4) leaves every entry, valid or not
    const int uid = a.own[g];
    if (uid >= 0 && uid < 2 * a.H) {
      const int s = uid % a.H;
#pragma unroll
      for (int d = 0; d < MAX_DEPTH; ++d) {
        int seen = 0;
        uint32_t kill = 0u;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
          const int bit = static_cast<int>((al[d] >> b) & 1u);
          if (bit && seen == s) kill |= 1u << b;
          seen += bit;
        }
        al[d] &= ~kill;
      }
    }
  }
  if (a.reset && a.reset[g] != 0) {   // a new deal: nothing stored is usable (rows and moves stay)
#pragma unroll
    for (int d = 0; d < MAX_DEPTH; ++d) al[d] = vl[d] = 0u;
  }
  if (a.cur) {
    const uint32_t c0 = a.cur[g * a.SW], w2 = a.cur[g * a.SW + 2];
    const uint32_t p0 = a.prev[g * a.SW], hand = a.prev[g * a.SW + 10 + a.seat];
    // hanabi_hip.search.last_move_uid
    const int kind = static_cast<int>((w2 >> 4) & 3u), idx = static_cast<int>((w2 >> 6) & 7u);
    const int off = static_cast<int>((w2 >> 9) & 7u) - 1;
    const int col = static_cast<int>((w2 >> 12) & 7u), rank = static_cast<int>((w2 >> 15) & 7u);
    const int uid = kind == 1 ? idx : kind == 0 ? a.H + idx : kind == 2 ? 2 * a.H + off * a.C + col
                                                                        : 2 * a.H + (a.P - 1) * a.C + off * a.R + rank;
    const bool moved = (w2 & 1u) != 0;
    const int partner = static_cast<int>((w2 >> 1) & 7u);   // the last mover
    const bool ok = ((c0 >> 19) & 3u) == 0 && moved && partner != a.seat && ((p0 >> 19) & 3u) == 0 &&
                    static_cast<int>((p0 >> 13) & 7u) == partner;
    uint32_t occ = 0u;
#pragma unroll
    for (int s = 0; s < 5; ++s) occ |= ((hand >> (5 * s)) & 31u) != 31u ? 1u << s : 0u;
#pragma unroll
    for (int d = MAX_DEPTH - 1; d >= 1; --d) {
      al[d] = al[d - 1];
      vl[d] = vl[d - 1];
      mv[d] = mv[d - 1];
    }
    al[0] = occ;
    vl[0] = ok ? 1u : 0u;
    mv[0] = moved ? uid : -1;
  }
#pragma unroll
  for (int d = 0; d < MAX_DEPTH; ++d) {
    if (d < a.depth) {
      a.alive[d * a.m + g] = static_cast<uint8_t>(al[d]);
      a.valid[d * a.m + g] = static_cast<uint8_t>(vl[d]);
      if (a.cur) a.moves[d * a.m + g] = mv[d];
    }
  }
}

struct ScoreArgs {
  const uint32_t* truth_rows;   // [m, SW]
  const uint32_t* det;          // [m * R, SW]
  const uint32_t* weight;       // [m * R]
  int8_t* truth;                // [m, H]
  long long* hit;               // [m, H]
  long long* joint;             // [m]
  long long* wsum;              // [m]
  int32_t* n_live;              // [m]
  long long* counts;            // [m, H, NC] or null
  int8_t* prior;                // [m, H, NC]
  long long m;
  int seat, R, P, C, Rk, H, D, SW, NC;
};

constexpr int MAX_HAND = 5;   // hb_config_validate's largest hand: the slots of one hand word

// One wavefront per root, integers only. Lane j < SW holds word j of the TRUE row; its scalars travel by v_readlane. Lane c < NC
// owns card c: the copies of c in the seat's pool (its hand slots, then the undealt deck bytes, walked by v_readlane of the deck
// words) give prior[s][c] under slot s's knowledge bits. The replicas come 64 at a time, one (hand word, weight) pair per lane:
// wsum, n_live, joint and hit[s] are sums over the replicas, each lane adding its own and one xor butterfly at the end; counts (when
// asked for) walks the batch by v_readlane, lane c adding the weight of every replica whose slot s holds c to its H accumulators.
// The loops over the slots are unrolled to MAX_HAND with wave-uniform guards, so that the accumulators stay in registers.
__global__ void __launch_bounds__(256) belief_score_kernel(ScoreArgs a) {
  const int lane = threadIdx.x & 63;
  const long long i = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (i >= a.m) return;
  const uint32_t wj = lane < a.SW ? a.truth_rows[i * a.SW + lane] : 0u;
  const uint32_t w0 = lane_read(wj, 0), w1 = lane_read(wj, 1);
  const int seat = a.seat < 0 ? static_cast<int>((w0 >> 13) & 7u) : a.seat;
  const bool scored = ((w0 >> 19) & 3u) == 0 && seat < a.P;   // (wave-uniform)
  const int st = scored ? seat : 0;                           // (a seat whose words exist, whatever the row says)
  const uint32_t hand = lane_read(wj, 10 + st);
  const uint64_t know = (static_cast<uint64_t>(lane_read(wj, 10 + a.P + 2 * st + 1)) << 32) | lane_read(wj, 10 + a.P + 2 * st);
  const int n_hand = scored ? min(static_cast<int>((w1 >> (15 + 3 * st)) & 7u), a.H) : 0;
  const uint32_t hand_mask = (1u << (5 * n_hand)) - 1u;   // the fields of the slots that count (n_hand <= H <= 5)

  // ---- truth and prior, from the true row alone ---------------------------------------------------------------------------------
  const uint32_t me = static_cast<uint32_t>(lane);   // the card this lane owns (meaningful below NC)
  int pool = 0;
#pragma unroll
  for (int s = 0; s < MAX_HAND; ++s) pool += s < n_hand && ((hand >> (5 * s)) & 31u) == me ? 1 : 0;
  if (scored) {
    const int deck_size = min(static_cast<int>(w0 & 63u), a.D);
    const int W_DECK = 10 + 3 * a.P;
    for (int q = a.D - deck_size; q < a.D; ++q) {   // (wave-uniform bounds; W_DECK + (D - 1) / 4 < SW)
      const uint32_t card = (lane_read(wj, W_DECK + (q >> 2)) >> (8 * (q & 3))) & 255u;
      pool += card == me ? 1 : 0;
    }
  }
  const uint32_t col = me / static_cast<uint32_t>(a.Rk), rk = me - col * static_cast<uint32_t>(a.Rk);
  bool truth_ok = true;   // every slot of the true hand holds a card a replica can match
#pragma unroll
  for (int s = 0; s < MAX_HAND; ++s) {
    if (s < a.H) {
      const uint32_t t = (hand >> (5 * s)) & 31u;
      const uint32_t kn = static_cast<uint32_t>(know >> (12 * s)) & 0xFFFu;
      const bool allowed = s < n_hand && ((kn >> col) & 1u) && ((kn >> (5u + rk)) & 1u);
      if (lane < a.NC) a.prior[(i * a.H + s) * a.NC + lane] = static_cast<int8_t>(allowed ? pool : 0);
      if (lane == s) a.truth[i * a.H + s] = static_cast<int8_t>(s < n_hand ? static_cast<int>(t) : -1);
      if (s < n_hand) truth_ok = truth_ok && t < static_cast<uint32_t>(a.NC);
    }
  }

  // ---- the replicas, 64 at a time -------------------------------------------------------------------------------------------------
  long long sw = 0, nl = 0, jn = 0, hit[MAX_HAND], cnt[MAX_HAND];
#pragma unroll
  for (int s = 0; s < MAX_HAND; ++s) hit[s] = cnt[s] = 0;
  const uint32_t* w = a.weight + i * a.R;
  const uint32_t* dh = a.det + i * a.R * a.SW + 10 + st;   // the hand word of replica 0
  for (int r0 = 0; r0 < a.R && scored; r0 += 64) {
    const int r = r0 + lane;
    const uint32_t wr = r < a.R ? w[r] : 0u;
    const uint32_t hr = r < a.R ? dh[static_cast<long long>(r) * a.SW] : 0u;
    sw += wr;
    nl += wr != 0u ? 1 : 0;
    jn += truth_ok && ((hr ^ hand) & hand_mask) == 0u ? wr : 0u;
#pragma unroll
    for (int s = 0; s < MAX_HAND; ++s) {
      const uint32_t f = (hr >> (5 * s)) & 31u;
      hit[s] += s < n_hand && f < static_cast<uint32_t>(a.NC) && f == ((hand >> (5 * s)) & 31u) ? wr : 0u;
    }
    if (a.counts) {
      const int nb = min(64, a.R - r0);
      for (int j = 0; j < nb; ++j) {
        const uint32_t wv = lane_read(wr, j), hv = lane_read(hr, j);
        if (wv == 0u) continue;   // (wave-uniform)
#pragma unroll
        for (int s = 0; s < MAX_HAND; ++s) cnt[s] += s < n_hand && ((hv >> (5 * s)) & 31u) == me ? wv : 0u;
      }
    }
  }
  sw = wave_sum(sw);
  nl = wave_sum(nl);
  jn = wave_sum(jn);
  long long mine = 0;   // hit of slot `lane`
#pragma unroll
  for (int s = 0; s < MAX_HAND; ++s) {
    const long long h = wave_sum(hit[s]);
    mine = lane == s ? h : mine;
    if (a.counts && s < a.H && lane < a.NC) a.counts[(i * a.H + s) * a.NC + lane] = cnt[s];
  }
  if (lane < a.H) a.hit[i * a.H + lane] = mine;
  if (lane == 0) {
    a.joint[i] = jn;
    a.wsum[i] = sw;
    a.n_live[i] = static_cast<int32_t>(nl);
  }
}

int have_device() {
  static const int ndev = [] {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
  }();
  return ndev > 0 ? HB_OK : hb::fail(HB_ERR_NO_DEVICE, "no HIP device available");
}

// The launch hb_belief_select (depth 1, no depth_used) and hb_belief_select_depth share; arguments checked by the caller.
int launch_select(const hb_config* cfg, const uint32_t* src, const uint32_t* det, const uint32_t* weight, const int32_t* hyp,
                  const int32_t* actual, const uint8_t* valid, int64_t m, int n_cand, int replicas, int depth, uint32_t* out,
                  uint32_t* out_weight, int32_t* n_surv, int32_t* depth_used, uint8_t* fallback, void* stream) {
  if (m == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  SelectDepthArgs a{};
  a.src = src; a.det = det; a.weight = weight; a.hyp = hyp; a.actual = actual; a.valid = valid;
  a.out = out; a.out_weight = out_weight; a.n_surv = n_surv; a.depth_used = depth_used; a.fallback = fallback;
  a.m = m;
  a.K = n_cand; a.R = replicas; a.SW = hb_state_words(cfg); a.depth = depth;
  const unsigned blocks = static_cast<unsigned>((m + 3) / 4);   // four wavefronts = four roots per workgroup
  hipLaunchKernelGGL(belief_select_depth_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

}  // namespace

extern "C" int hb_belief_determinize(const hb_config* cfg, const uint32_t* src_rows_dev, int64_t m, int32_t seat, int32_t replicas,
                                     uint64_t seed, uint64_t draw, int64_t first_row_id, uint32_t* out_rows_dev, uint32_t* weight_dev,
                                     void* stream) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (m < 0) return hb::fail(HB_ERR_INVALID, "m must be >= 0");
  if (replicas < 1) return hb::fail(HB_ERR_INVALID, "replicas must be >= 1, got %d", replicas);
  if (seat < -1 || seat >= cfg->players)
    return hb::fail(HB_ERR_INVALID, "seat %d out of range: -1 (each row's current player) or 0..%d", seat, cfg->players - 1);
  if (!src_rows_dev || !out_rows_dev || !weight_dev) return hb::fail(HB_ERR_INVALID, "null argument");
  if (m > (static_cast<int64_t>(1) << 31) / replicas - 1)
    return hb::fail(HB_ERR_INVALID, "m * replicas must stay below 2^31 output rows: split the call (first_row_id)");
  if (m == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  DetArgs a{};
  a.src = src_rows_dev; a.out = out_rows_dev; a.weight = weight_dev;
  a.n_out = m * replicas;
  a.first_row = first_row_id;
  a.seed = seed; a.draw = draw;
  a.replicas = replicas; a.seat = seat;
  a.P = cfg->players; a.C = cfg->colors; a.R = cfg->ranks; a.H = cfg->hand_size;
  a.D = hb_deck_size(cfg);
  a.SW = hb_state_words(cfg);
  const unsigned blocks = static_cast<unsigned>((a.n_out + 3) / 4);   // four wavefronts = four output rows per workgroup
  hipLaunchKernelGGL(belief_determinize_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

extern "C" int hb_belief_carry(const hb_config* cfg, const uint32_t* cur_rows_dev, const uint32_t* old_rows_dev,
                               const uint32_t* old_weight_dev, const int32_t* own_slot_dev, const int32_t* revealed_dev,
                               const int32_t* drew_dev, int64_t m, int32_t seat, int32_t n_particles, uint64_t seed, uint64_t draw,
                               int64_t first_row_id, uint32_t* out_rows_dev, uint32_t* out_weight_dev, void* stream) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (m < 0) return hb::fail(HB_ERR_INVALID, "m must be >= 0");
  if (n_particles < 1) return hb::fail(HB_ERR_INVALID, "n_particles must be >= 1, got %d", n_particles);
  if (seat < 0 || seat >= cfg->players)
    return hb::fail(HB_ERR_INVALID, "seat %d out of range 0..%d (the observer, who is to act)", seat, cfg->players - 1);
  if (!cur_rows_dev || !old_rows_dev || !old_weight_dev || !own_slot_dev || !revealed_dev || !drew_dev || !out_rows_dev || !out_weight_dev)
    return hb::fail(HB_ERR_INVALID, "null argument");
  if (m > (static_cast<int64_t>(1) << 31) / n_particles - 1)
    return hb::fail(HB_ERR_INVALID, "m * n_particles must stay below 2^31 output rows: split the call (first_row_id)");
  if (m == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  CarryArgs a{};
  a.cur = cur_rows_dev; a.old_rows = old_rows_dev; a.old_weight = old_weight_dev;
  a.own_slot = own_slot_dev; a.revealed = revealed_dev; a.drew = drew_dev;
  a.out = out_rows_dev; a.weight = out_weight_dev;
  a.n_out = m * n_particles;
  a.first_row = first_row_id;
  a.seed = seed; a.draw = draw;
  a.K = n_particles; a.seat = seat;
  a.P = cfg->players; a.C = cfg->colors; a.R = cfg->ranks; a.H = cfg->hand_size;
  a.D = hb_deck_size(cfg);
  a.SW = hb_state_words(cfg);
  const unsigned blocks = static_cast<unsigned>((a.n_out + 3) / 4);   // four wavefronts = four output rows per workgroup
  hipLaunchKernelGGL(belief_carry_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

extern "C" int hb_search_reduce(const int8_t* score_dev, const uint32_t* weight_dev, const int8_t* legal_dev, int64_t m,
                                int32_t n_actions, int32_t replicas, float* value_dev, int64_t* wsum_dev, int32_t* n_live_dev,
                                int32_t* best_dev, void* stream) {
  if (m < 0) return hb::fail(HB_ERR_INVALID, "m must be >= 0");
  if (n_actions < 1 || n_actions > 64) return hb::fail(HB_ERR_INVALID, "n_actions %d out of range 1..64", n_actions);
  if (replicas < 1 || replicas > (1 << 20)) return hb::fail(HB_ERR_INVALID, "replicas %d out of range 1..2^20 (64-bit sums)", replicas);
  if (!score_dev || !weight_dev || !legal_dev || !value_dev || !wsum_dev || !n_live_dev) return hb::fail(HB_ERR_INVALID, "null argument");
  if (m > (static_cast<int64_t>(1) << 31) - 8) return hb::fail(HB_ERR_INVALID, "m must stay below 2^31 roots");
  if (m == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  const unsigned blocks = static_cast<unsigned>((m + 3) / 4);
  hipLaunchKernelGGL(search_reduce_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), score_dev, weight_dev, legal_dev,
                     static_cast<long long>(m), n_actions, replicas, value_dev, reinterpret_cast<long long*>(wsum_dev), n_live_dev,
                     best_dev);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

extern "C" int hb_search_layout(const hb_config* cfg, const uint32_t* det_rows_dev, const uint32_t* weight_dev, const int32_t* cand_dev,
                                const int32_t* filler_dev, int64_t m, int32_t n_cand, int32_t replicas, uint32_t* rows_out_dev,
                                int32_t* forced_out_dev, uint8_t* done_out_dev, int32_t* n_played_out_dev, void* stream) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (m < 0) return hb::fail(HB_ERR_INVALID, "m must be >= 0");
  if (n_cand < 1 || n_cand > 64) return hb::fail(HB_ERR_INVALID, "n_cand %d out of range 1..64", n_cand);
  if (replicas < 1) return hb::fail(HB_ERR_INVALID, "replicas must be >= 1, got %d", replicas);
  if (!det_rows_dev || !weight_dev || !cand_dev || !filler_dev || !rows_out_dev || !forced_out_dev || !done_out_dev || !n_played_out_dev)
    return hb::fail(HB_ERR_INVALID, "null argument");
  if (m > ((static_cast<int64_t>(1) << 31) - 1) / (static_cast<int64_t>(n_cand) * replicas))
    return hb::fail(HB_ERR_INVALID, "m * n_cand * replicas must stay below 2^31 rollout games: split the roots");
  if (m == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  LayoutArgs a{};
  a.det = det_rows_dev; a.weight = weight_dev; a.cand = cand_dev; a.filler = filler_dev;
  a.rows = rows_out_dev; a.forced = forced_out_dev; a.done = done_out_dev; a.n_played = n_played_out_dev;
  a.n_src = m * replicas;
  a.C = n_cand; a.R = replicas;
  a.SW = hb_state_words(cfg);
  const unsigned blocks = static_cast<unsigned>((a.n_src + 3) / 4);   // four wavefronts = four source rows per workgroup
  hipLaunchKernelGGL(search_layout_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

extern "C" int hb_search_compare(const int8_t* score_dev, const uint32_t* weight_dev, const int32_t* cand_dev, const int32_t* base_slot_dev,
                                 int64_t m, int32_t n_cand, int32_t replicas, double* diff_dev, double* se_dev, int32_t* n_pair_dev,
                                 void* stream) {
  if (m < 0) return hb::fail(HB_ERR_INVALID, "m must be >= 0");
  if (n_cand < 1 || n_cand > 64) return hb::fail(HB_ERR_INVALID, "n_cand %d out of range 1..64", n_cand);
  if (replicas < 1 || replicas > (1 << 20)) return hb::fail(HB_ERR_INVALID, "replicas %d out of range 1..2^20 (64-bit sums)", replicas);
  if (!score_dev || !weight_dev || !cand_dev || !base_slot_dev || !diff_dev || !se_dev || !n_pair_dev)
    return hb::fail(HB_ERR_INVALID, "null argument");
  if (m > ((static_cast<int64_t>(1) << 31) - 1) / (static_cast<int64_t>(n_cand) * replicas))
    return hb::fail(HB_ERR_INVALID, "m * n_cand * replicas must stay below 2^31 rollout games");
  if (m == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  const unsigned blocks = static_cast<unsigned>((m + 3) / 4);
  hipLaunchKernelGGL(search_compare_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), score_dev, weight_dev, cand_dev,
                     base_slot_dev, static_cast<long long>(m), n_cand, replicas, diff_dev, se_dev, n_pair_dev);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

extern "C" int hb_belief_splice(const hb_config* cfg, const uint32_t* prev_rows_dev, const uint32_t* det_rows_dev, int64_t m, int32_t seat,
                                int32_t n_cand, uint32_t* out_rows_dev, void* stream) {
  return hb_belief_splice_alive(cfg, prev_rows_dev, /*alive*/ nullptr, det_rows_dev, m, seat, n_cand, out_rows_dev, stream);
}

extern "C" int hb_belief_select(const hb_config* cfg, const uint32_t* src_rows_dev, const uint32_t* det_rows_dev, const uint32_t* weight_dev,
                                const int32_t* hyp_moves_dev, const int32_t* actual_dev, const uint8_t* valid_dev, int64_t m, int32_t n_cand,
                                int32_t replicas, uint32_t* out_rows_dev, uint32_t* out_weight_dev, int32_t* n_surv_dev,
                                uint8_t* fallback_dev, void* stream) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (m < 0) return hb::fail(HB_ERR_INVALID, "m must be >= 0");
  if (replicas < 1) return hb::fail(HB_ERR_INVALID, "replicas must be >= 1, got %d", replicas);
  if (n_cand < replicas) return hb::fail(HB_ERR_INVALID, "n_cand %d must be >= replicas %d", n_cand, replicas);
  if (!src_rows_dev || !det_rows_dev || !weight_dev || !hyp_moves_dev || !actual_dev || !out_rows_dev || !out_weight_dev || !n_surv_dev ||
      !fallback_dev)
    return hb::fail(HB_ERR_INVALID, "null argument");
  const int SW = hb_state_words(cfg);
  if (m > ((static_cast<int64_t>(1) << 31) - 1) / (static_cast<int64_t>(n_cand) * SW))
    return hb::fail(HB_ERR_INVALID, "m * n_cand * state words must stay below 2^31: split the roots");
  return launch_select(cfg, src_rows_dev, det_rows_dev, weight_dev, hyp_moves_dev, actual_dev, valid_dev, m, n_cand, replicas, /*depth*/ 1,
                       out_rows_dev, out_weight_dev, n_surv_dev, /*depth_used*/ nullptr, fallback_dev, stream);
}

extern "C" int hb_belief_splice_alive(const hb_config* cfg, const uint32_t* prev_rows_dev, const uint8_t* alive_dev,
                                      const uint32_t* det_rows_dev, int64_t m, int32_t seat, int32_t n_cand, uint32_t* out_rows_dev,
                                      void* stream) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (m < 0) return hb::fail(HB_ERR_INVALID, "m must be >= 0");
  if (n_cand < 1) return hb::fail(HB_ERR_INVALID, "n_cand must be >= 1, got %d", n_cand);
  if (seat < 0 || seat >= cfg->players)
    return hb::fail(HB_ERR_INVALID, "seat %d out of range 0..%d (the observer is not the previous state's current player)", seat,
                    cfg->players - 1);
  if (!prev_rows_dev || !det_rows_dev || !out_rows_dev) return hb::fail(HB_ERR_INVALID, "null argument");   // (alive may be null)
  const int SW = hb_state_words(cfg);
  if (m > ((static_cast<int64_t>(1) << 31) - 1) / (static_cast<int64_t>(n_cand) * SW))
    return hb::fail(HB_ERR_INVALID, "m * n_cand * state words must stay below 2^31: split the roots");
  if (m == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  SpliceAliveArgs a{};
  a.prev = prev_rows_dev; a.alive = alive_dev; a.det = det_rows_dev; a.out = out_rows_dev;
  a.m = m;
  a.n_out = m * n_cand;
  a.K = n_cand; a.SW = SW;
  a.hand_word = 10 + seat;
  const unsigned blocks = static_cast<unsigned>((a.n_out + 3) / 4);   // four wavefronts = four output rows per workgroup
  hipLaunchKernelGGL(belief_splice_alive_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

extern "C" int hb_belief_select_depth(const hb_config* cfg, const uint32_t* src_rows_dev, const uint32_t* det_rows_dev,
                                      const uint32_t* weight_dev, const int32_t* hyp_moves_dev, const int32_t* actual_dev,
                                      const uint8_t* valid_dev, int64_t m, int32_t n_cand, int32_t replicas, int32_t depth,
                                      uint32_t* out_rows_dev, uint32_t* out_weight_dev, int32_t* n_surv_dev, int32_t* depth_used_dev,
                                      uint8_t* fallback_dev, void* stream) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (m < 0) return hb::fail(HB_ERR_INVALID, "m must be >= 0");
  if (replicas < 1) return hb::fail(HB_ERR_INVALID, "replicas must be >= 1, got %d", replicas);
  if (n_cand < replicas) return hb::fail(HB_ERR_INVALID, "n_cand %d must be >= replicas %d", n_cand, replicas);
  if (depth < 1 || depth > MAX_DEPTH) return hb::fail(HB_ERR_INVALID, "depth %d out of range 1..%d", depth, MAX_DEPTH);
  if (!src_rows_dev || !det_rows_dev || !weight_dev || !hyp_moves_dev || !actual_dev || !out_rows_dev || !out_weight_dev || !n_surv_dev ||
      !depth_used_dev || !fallback_dev)
    return hb::fail(HB_ERR_INVALID, "null argument");
  const int SW = hb_state_words(cfg);
  if (m > ((static_cast<int64_t>(1) << 31) - 1) / (static_cast<int64_t>(n_cand) * SW))
    return hb::fail(HB_ERR_INVALID, "m * n_cand * state words must stay below 2^31: split the roots");
  return launch_select(cfg, src_rows_dev, det_rows_dev, weight_dev, hyp_moves_dev, actual_dev, valid_dev, m, n_cand, replicas, depth,
                       out_rows_dev, out_weight_dev, n_surv_dev, depth_used_dev, fallback_dev, stream);
}

extern "C" int hb_belief_select_soft(const hb_config* cfg, const uint32_t* src_rows_dev, const uint32_t* det_rows_dev,
                                     const uint32_t* weight_dev, const int32_t* hyp_moves_dev, const int32_t* n_legal_dev,
                                     const int32_t* actual_dev, const uint8_t* valid_dev, const double* p_table_dev, int64_t m,
                                     int32_t n_cand, int32_t replicas, int32_t depth, uint64_t seed, uint64_t draw, int64_t first_row_id,
                                     uint32_t* out_rows_dev, uint32_t* out_weight_dev, int32_t* n_surv_dev, int32_t* depth_used_dev,
                                     uint8_t* fallback_dev, float* ess_dev, void* stream) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (m < 0) return hb::fail(HB_ERR_INVALID, "m must be >= 0");
  if (replicas < 1) return hb::fail(HB_ERR_INVALID, "replicas must be >= 1, got %d", replicas);
  if (n_cand < 1 || n_cand > 4096)
    return hb::fail(HB_ERR_INVALID, "n_cand %d out of range 1..4096 (the 64-bit sum of the quantised weights)", n_cand);
  if (depth < 1 || depth > MAX_DEPTH) return hb::fail(HB_ERR_INVALID, "depth %d out of range 1..%d", depth, MAX_DEPTH);
  if (!src_rows_dev || !det_rows_dev || !weight_dev || !hyp_moves_dev || !n_legal_dev || !actual_dev || !p_table_dev || !out_rows_dev ||
      !out_weight_dev || !n_surv_dev || !depth_used_dev || !fallback_dev || !ess_dev)
    return hb::fail(HB_ERR_INVALID, "null argument");
  const int SW = hb_state_words(cfg);
  if (m > ((static_cast<int64_t>(1) << 31) - 1) / (static_cast<int64_t>(n_cand > replicas ? n_cand : replicas) * SW))
    return hb::fail(HB_ERR_INVALID, "m * max(n_cand, replicas) * state words must stay below 2^31: split the roots");
  if (m == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  SelectSoftArgs a{};
  a.src = src_rows_dev; a.det = det_rows_dev; a.weight = weight_dev; a.hyp = hyp_moves_dev; a.n_legal = n_legal_dev;
  a.actual = actual_dev; a.valid = valid_dev; a.p_table = p_table_dev;
  a.out = out_rows_dev; a.out_weight = out_weight_dev; a.n_surv = n_surv_dev; a.depth_used = depth_used_dev; a.fallback = fallback_dev;
  a.ess = ess_dev;
  a.m = m; a.first_row = first_row_id;
  a.seed = seed; a.draw = draw;
  a.K = n_cand; a.R = replicas; a.SW = SW; a.depth = depth; a.A = hb_num_actions(cfg);
  const unsigned blocks = static_cast<unsigned>((m + 3) / 4);   // four wavefronts = four roots per workgroup
  hipLaunchKernelGGL(belief_select_soft_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

extern "C" int hb_belief_history_step(const hb_config* cfg, int64_t m, int32_t depth, int32_t seat, const int32_t* own_moves_dev,
                                      const uint8_t* reset_dev, const uint32_t* cur_rows_dev, const uint32_t* prev_rows_dev,
                                      uint32_t* hist_rows_dev, int32_t* hist_moves_dev, uint8_t* hist_alive_dev, uint8_t* hist_valid_dev,
                                      void* stream) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (m < 0) return hb::fail(HB_ERR_INVALID, "m must be >= 0");
  if (depth < 1 || depth > MAX_DEPTH) return hb::fail(HB_ERR_INVALID, "depth %d out of range 1..%d", depth, MAX_DEPTH);
  if (seat < 0 || seat >= cfg->players) return hb::fail(HB_ERR_INVALID, "seat %d out of range 0..%d", seat, cfg->players - 1);
  if ((cur_rows_dev == nullptr) != (prev_rows_dev == nullptr))
    return hb::fail(HB_ERR_INVALID, "cur_rows and prev_rows go together: a push needs both, no push neither");
  if (!hist_rows_dev || !hist_moves_dev || !hist_alive_dev || !hist_valid_dev) return hb::fail(HB_ERR_INVALID, "null argument");
  const int SW = hb_state_words(cfg);
  if (m > ((static_cast<int64_t>(1) << 31) - 1) / (static_cast<int64_t>(depth) * SW))
    return hb::fail(HB_ERR_INVALID, "m * depth * state words must stay below 2^31: split the games");
  if (m == 0 || (!own_moves_dev && !reset_dev && !cur_rows_dev)) return HB_OK;
  if (int rc = have_device()) return rc;
  HistoryArgs a{};
  a.own = own_moves_dev; a.reset = reset_dev; a.cur = cur_rows_dev; a.prev = prev_rows_dev;
  a.rows = hist_rows_dev; a.moves = hist_moves_dev; a.alive = hist_alive_dev; a.valid = hist_valid_dev;
  a.m = m;
  a.depth = depth; a.seat = seat; a.SW = SW;
  a.P = cfg->players; a.C = cfg->colors; a.R = cfg->ranks; a.H = cfg->hand_size;
  // 16-byte items where the row buffers allow it (a row is 128 or 192 bytes, so every row then starts on a 16-byte boundary)
  const bool wide = cur_rows_dev && SW % 4 == 0 &&
                    ((reinterpret_cast<uintptr_t>(hist_rows_dev) | reinterpret_cast<uintptr_t>(prev_rows_dev)) & 15u) == 0;
  a.n_items = cur_rows_dev ? m * (wide ? SW / 4 : SW) : 0;
  a.row_blocks = static_cast<unsigned>((a.n_items + 255) / 256);
  const unsigned blocks = a.row_blocks + static_cast<unsigned>((m + 255) / 256);
  if (wide)
    hipLaunchKernelGGL(belief_history_step_kernel<uint4>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  else
    hipLaunchKernelGGL(belief_history_step_kernel<uint32_t>, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}

extern "C" int hb_belief_score(const hb_config* cfg, const uint32_t* true_rows_dev, const uint32_t* det_rows_dev, const uint32_t* weight_dev,
                               int64_t m, int32_t seat, int32_t replicas, int8_t* truth_dev, int64_t* hit_dev, int64_t* joint_dev,
                               int64_t* wsum_dev, int32_t* n_live_dev, int64_t* counts_dev, int8_t* prior_dev, void* stream) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (m < 0) return hb::fail(HB_ERR_INVALID, "m must be >= 0");
  if (replicas < 1 || replicas > (1 << 20)) return hb::fail(HB_ERR_INVALID, "replicas %d out of range 1..2^20 (64-bit sums)", replicas);
  if (seat < -1 || seat >= cfg->players)
    return hb::fail(HB_ERR_INVALID, "seat %d out of range: -1 (each row's current player) or 0..%d", seat, cfg->players - 1);
  if (!true_rows_dev || !det_rows_dev || !weight_dev || !truth_dev || !hit_dev || !joint_dev || !wsum_dev || !n_live_dev || !prior_dev)
    return hb::fail(HB_ERR_INVALID, "null argument");   // (counts may be null)
  if (m > (static_cast<int64_t>(1) << 31) - 8) return hb::fail(HB_ERR_INVALID, "m must stay below 2^31 roots");
  if (m == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  ScoreArgs a{};
  a.truth_rows = true_rows_dev; a.det = det_rows_dev; a.weight = weight_dev;
  a.truth = truth_dev; a.hit = reinterpret_cast<long long*>(hit_dev); a.joint = reinterpret_cast<long long*>(joint_dev);
  a.wsum = reinterpret_cast<long long*>(wsum_dev); a.n_live = n_live_dev; a.counts = reinterpret_cast<long long*>(counts_dev);
  a.prior = prior_dev;
  a.m = m;
  a.seat = seat; a.R = replicas;
  a.P = cfg->players; a.C = cfg->colors; a.Rk = cfg->ranks; a.H = cfg->hand_size;
  a.D = hb_deck_size(cfg);
  a.SW = hb_state_words(cfg);
  a.NC = cfg->colors * cfg->ranks;
  const unsigned blocks = static_cast<unsigned>((m + 3) / 4);   // four wavefronts = four roots per workgroup
  hipLaunchKernelGGL(belief_score_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}
