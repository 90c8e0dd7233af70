// belief_exact.hip — hb_belief_enumerate (include/hanabi_hip_exact.h): the exact belief of one seat against rule-list partners, by
// enumeration of every hand the seat may hold ("The exact belief").
//
// Four launches, all on the caller's stream, so each sees what the one before it wrote and nothing waits inside a kernel:
//   enum_prep_kernel   one workgroup per root: status, space, and every output's value for a root that is not enumerated
//   enum_walk_kernel   one workgroup per block of 1024 hands of a root, one lane per hand (four hands a lane, one after another):
//                      the hand of index e (mixed radix over the slots' allowed cards), its mass, and for the leading valid
//                      entries of the history the rule walk (rule_walk.hpp: the code of hb_rule_act) on the entry's row with the
//                      hand spliced in. The row lives in LDS, one per lane at stride SW + 1 words like hb_rule_playout's games; a
//                      workgroup's lanes all hold the same entry's row and differ in the one hand word, so the row is copied only
//                      when the entry changes. Pass byte per hand -> scratch; the per-level sums -> LDS -> integer atomics.
//   enum_marg_kernel   the same blocks: depth_used from the finished level sums, the marginals at that level (and at level 0) in
//                      LDS accumulators -> integer atomics, and the block's masked sum -> scratch
//   enum_draw_kernel   one lane per (root, replica): the Philox target, the block of 1024 that holds it by a walk over the block
//                      sums, the hand by a walk over the block in enumeration order
// All sums are integers added by atomics or in a fixed order: no result depends on the grid or on the order of an add. Workgroups
// whose block lies behind a root's last hand (the grid is sized by max_hands, not by the root) leave at once.
#include <hip/hip_runtime.h>

#include "../../include/hanabi_hip_exact.h"
#include "common.hpp"
#include "env_kernel.hpp"
#include "rule_walk.hpp"

namespace {

constexpr int kMaxPlayers = 5;
constexpr int MAX_DEPTH = HB_EXACT_MAX_DEPTH;
constexpr int MAX_HAND = 5;                   // hb_config_validate's largest hand: the slots of one hand word
constexpr int MAX_CARDS = 25;                 // ... and the most card ids (Cfg's limit)
constexpr int BLOCK_HANDS = HB_EXACT_BLOCK_HANDS;
constexpr int TPB = 256;
constexpr int HPL = BLOCK_HANDS / TPB;        // hands per lane

struct EnumArgs {
  const uint32_t* cur;
  const uint32_t* hist_rows;
  const int32_t* hist_moves;
  const uint8_t* hist_alive;
  const uint8_t* hist_valid;
  uint8_t* status;
  long long* space;
  unsigned long long* mass;
  int32_t* n_hands;
  int32_t* depth_used;
  uint8_t* fallback;
  unsigned long long* marg;
  unsigned long long* marg0;
  uint32_t* hands;
  unsigned long long* block_sum;   // scratch: [m][bpr]
  uint8_t* pass;                   // scratch: [m][cap]
  long long m, max_hands, cap, first_gid, first_row;
  unsigned long long pseed, seed, draw;
  unsigned long long draws[MAX_DEPTH];
  unsigned bpr;                    // blocks of 1024 hands per root: ceil(cap / 1024)
  unsigned rpb;                    // workgroups of 256 replicas per root: ceil(R / 256)
  int seat, depth, R, P, C, Rk, H, D, SW, NC;
  int n_rules[kMaxPlayers];
  hb_rule rules[kMaxPlayers][HB_MAX_RULES];
};

// what HB_RULE_WALK reads of its argument block: the game's dimensions (compile-time here) and the Philox key of the entry
template <class K>
struct WalkArgs {
  static constexpr int P = K::P, C = K::C, R = K::R, H = K::H, INFO = K::INFO, CPC = K::CPC;
  unsigned long long seed, draw;
};

// One root as every kernel here sees it, built in LDS by root_setup: the enumeration space and the tables that turn a hand index
// into cards.
struct Root {
  long long N;           // prod |allowed_s|
  uint32_t hand_word;    // cur row's word 10 + seat
  int n, scored, L;
  uint8_t cnt[32];                   // copies of card c in the seat's pool
  uint8_t nal[MAX_HAND];             // |allowed_s|
  uint8_t sel[MAX_HAND][32];         // the j-th smallest card id of allowed_s
};

// Called by every thread of a workgroup (it holds barriers). Thread c < NC counts card c in the pool, thread s < n lists slot s's
// allowed cards in ascending order, thread 0 forms N and L.
__device__ void root_setup(const EnumArgs& a, long long i, Root& rt) {
  const int tid = threadIdx.x;
  const uint32_t* row = a.cur + i * a.SW;
  const uint32_t w0 = row[0], w1 = row[1];
  const bool scored = ((w0 >> 19) & 3u) == 0;   // (seat < P: checked on the host)
  const int n = scored ? min(static_cast<int>((w1 >> (15 + 3 * a.seat)) & 7u), a.H) : 0;
  const uint32_t hand = row[10 + a.seat];
  if (tid < 32) {
    int c = 0;
    if (scored && tid < a.NC) {
      for (int s = 0; s < n; ++s) c += ((hand >> (5 * s)) & 31u) == static_cast<uint32_t>(tid) ? 1 : 0;
      const int deck_size = min(static_cast<int>(w0 & 63u), a.D);
      const int W_DECK = 10 + 3 * a.P;
      for (int q = a.D - deck_size; q < a.D; ++q)   // (W_DECK + (D - 1) / 4 < SW)
        c += ((row[W_DECK + (q >> 2)] >> (8 * (q & 3))) & 255u) == static_cast<uint32_t>(tid) ? 1 : 0;
    }
    rt.cnt[tid] = static_cast<uint8_t>(c);
  }
  __syncthreads();
  if (tid < MAX_HAND) {
    int k = 0;
    if (tid < n) {
      const uint64_t know = (static_cast<uint64_t>(row[10 + a.P + 2 * a.seat + 1]) << 32) | row[10 + a.P + 2 * a.seat];
      const uint32_t kn = static_cast<uint32_t>(know >> (12 * tid)) & 0xFFFu;
      for (int c = 0; c < a.NC; ++c) {
        const int col = c / a.Rk, rk = c - col * a.Rk;
        if (rt.cnt[c] > 0 && ((kn >> col) & 1u) && ((kn >> (5 + rk)) & 1u)) rt.sel[tid][k++] = static_cast<uint8_t>(c);
      }
    }
    rt.nal[tid] = static_cast<uint8_t>(k);
  }
  __syncthreads();
  if (tid == 0) {
    long long N = 1;
    for (int s = 0; s < n; ++s) N *= rt.nal[s];   // (<= 25^5)
    int L = 0;
    if (scored)
      while (L < a.depth && (!a.hist_valid || a.hist_valid[L * a.m + i] != 0)) ++L;
    rt.N = N;
    rt.hand_word = hand;
    rt.n = n;
    rt.scored = scored ? 1 : 0;
    rt.L = L;
  }
  __syncthreads();
}

// Hand e of the root: its cards into the 5-bit fields of `word` (slots >= n hold 31, bits 25-31 are the root's own), and its mass.
__device__ __forceinline__ uint32_t hand_of(const Root& rt, uint32_t e, uint32_t& word) {
  uint32_t c[MAX_HAND];
  uint32_t mass = 1u, w = rt.hand_word | 0x1FFFFFFu;
#pragma unroll
  for (int s = 0; s < MAX_HAND; ++s) {
    c[s] = 31u;
    if (s < rt.n) {
      const uint32_t r = rt.nal[s];
      const uint32_t quo = e / r;
      c[s] = rt.sel[s][e - quo * r];
      e = quo;
      uint32_t before = 0;
#pragma unroll
      for (int t = 0; t < s; ++t) before += c[t] == c[s] ? 1u : 0u;
      const uint32_t have = rt.cnt[c[s]];
      mass = have > before ? mass * (have - before) : 0u;
      w = (w & ~(31u << (5 * s))) | (c[s] << (5 * s));
    }
  }
  word = w;
  return mass;
}

// the largest level k <= L whose sum is not zero (the sums never grow with k)
__device__ __forceinline__ int level_used(const EnumArgs& a, long long i, int L) {
  int used = 0;
  for (int k = 1; k <= L; ++k) used = a.mass[k * a.m + i] != 0ull ? k : used;
  return used;
}

__global__ __launch_bounds__(TPB) void enum_prep_kernel(const EnumArgs a) {
  __shared__ Root rt;
  const long long i = blockIdx.x;
  const int tid = threadIdx.x;
  root_setup(a, i, rt);
  const int st = !rt.scored ? 2 : rt.N > a.max_hands ? 1 : 0;
  if (tid == 0) {
    a.status[i] = static_cast<uint8_t>(st);
    a.space[i] = rt.scored ? rt.N : 0ll;
    a.depth_used[i] = 0;
    a.fallback[i] = static_cast<uint8_t>(st != 0 ? 0 : rt.L == 0 ? 2 : 1);   // (the last: until enum_marg_kernel finds a level)
  }
  if (tid <= a.depth) {
    a.mass[tid * a.m + i] = 0ull;
    a.n_hands[tid * a.m + i] = 0;
  }
  const int cells = a.H * a.NC;
  for (int x = tid; x < cells; x += TPB) {
    a.marg[i * cells + x] = 0ull;
    if (a.marg0) a.marg0[i * cells + x] = 0ull;
  }
  for (int r = tid; r < a.R; r += TPB) a.hands[i * a.R + r] = rt.hand_word;
}

template <class K>
__global__ __launch_bounds__(TPB) void enum_walk_kernel(const EnumArgs a) {
  __shared__ uint32_t lds[TPB * K::SWP];
  __shared__ Root rt;
  __shared__ unsigned long long lm[MAX_DEPTH + 1];
  __shared__ unsigned int ln[MAX_DEPTH + 1];
  const int tid = threadIdx.x;
  const long long i = blockIdx.x / a.bpr;
  const unsigned q = blockIdx.x - static_cast<unsigned>(i) * a.bpr;
  if (tid <= MAX_DEPTH) {
    lm[tid] = 0ull;
    ln[tid] = 0u;
  }
  root_setup(a, i, rt);
  const long long first = static_cast<long long>(q) * BLOCK_HANDS;
  if (!rt.scored || rt.N > a.max_hands || first >= rt.N) return;   // (workgroup-uniform)
  const int L = rt.L;
  uint32_t* const myrow = lds + tid * K::SWP;
  uint32_t acc_m[MAX_DEPTH + 1], acc_n[MAX_DEPTH + 1];
#pragma unroll
  for (int k = 0; k <= MAX_DEPTH; ++k) acc_m[k] = acc_n[k] = 0u;
  int held = -1;   // the entry whose row the LDS rows hold
  for (int j = 0; j < HPL; ++j) {
    const long long e = first + j * TPB + tid;
    uint32_t word = 0u, mass = 0u;
    if (e < rt.N) mass = hand_of(rt, static_cast<uint32_t>(e), word);
    int pass = 0;
    bool on = mass != 0u;
    for (int d = 0; d < L; ++d) {   // (workgroup-uniform bound)
      const uint32_t* hrow = a.hist_rows + (static_cast<long long>(d) * a.m + i) * K::SW;
      if (held != d) {   // (workgroup-uniform)
        for (int w = 0; w < K::SW; ++w) myrow[w] = hrow[w];
        held = d;
      }
      const int mover = static_cast<int>((hrow[0] >> 13) & 7u);
      if (mover >= K::P) on = false;   // (uniform) a row that names no seat reproduces nothing
      if (on) {
        // hb_belief_splice_alive's rule on the entry's hand word
        uint32_t hw = hrow[10 + a.seat];
        const uint32_t alive = a.hist_alive ? a.hist_alive[d * a.m + i] : 0xFFu;
        int t = 0;
#pragma unroll
        for (int s = 0; s < 5; ++s) {
          const uint32_t c = (word >> (5 * t)) & 31u;   // (t <= s <= 4)
          const bool take = ((hw >> (5 * s)) & 31u) != 31u && ((alive >> s) & 1u) && c != 31u;
          if (take) {
            hw = (hw & ~(31u << (5 * s))) | (c << (5 * s));
            ++t;
          }
        }
        myrow[10 + a.seat] = hw;
        const WalkArgs<K> wa{a.pseed, a.draws[d]};
        HB_RULE_WALK(wa, myrow, a.first_gid + i, a.n_rules[mover], a.rules[mover])
        (void)fired;
        on = act == a.hist_moves[d * a.m + i];
        pass += on ? 1 : 0;
      }
    }
    if (e < rt.N) a.pass[i * a.cap + e] = static_cast<uint8_t>(pass);
#pragma unroll
    for (int k = 0; k <= MAX_DEPTH; ++k) {
      const bool in = mass != 0u && pass >= k;   // (pass <= L: nothing beyond level L)
      acc_m[k] += in ? mass : 0u;
      acc_n[k] += in ? 1u : 0u;
    }
  }
#pragma unroll
  for (int k = 0; k <= MAX_DEPTH; ++k) {
    if (acc_n[k]) {
      atomicAdd(&lm[k], static_cast<unsigned long long>(acc_m[k]));
      atomicAdd(&ln[k], acc_n[k]);
    }
  }
  __syncthreads();
  if (tid <= L && ln[tid]) {
    atomicAdd(a.mass + tid * a.m + i, lm[tid]);
    atomicAdd(a.n_hands + tid * a.m + i, static_cast<int>(ln[tid]));
  }
}

__global__ __launch_bounds__(TPB) void enum_marg_kernel(const EnumArgs a) {
  __shared__ Root rt;
  __shared__ unsigned long long acc[2][MAX_HAND * MAX_CARDS];
  __shared__ unsigned long long bsum;
  const int tid = threadIdx.x;
  const long long i = blockIdx.x / a.bpr;
  const unsigned q = blockIdx.x - static_cast<unsigned>(i) * a.bpr;
  for (int x = tid; x < 2 * MAX_HAND * MAX_CARDS; x += TPB) acc[0][x] = 0ull;
  if (tid == 0) bsum = 0ull;
  root_setup(a, i, rt);
  const long long first = static_cast<long long>(q) * BLOCK_HANDS;
  if (!rt.scored || rt.N > a.max_hands || first >= rt.N) return;   // (workgroup-uniform)
  const int used = level_used(a, i, rt.L);
  if (q == 0 && tid == 0) {
    a.depth_used[i] = used;
    a.fallback[i] = static_cast<uint8_t>(rt.L == 0 ? 2 : used == 0 ? 1 : 0);
  }
  unsigned long long local = 0ull;
  for (int j = 0; j < HPL; ++j) {
    const long long e = first + j * TPB + tid;
    if (e >= rt.N) continue;
    uint32_t word;
    const uint32_t mass = hand_of(rt, static_cast<uint32_t>(e), word);
    if (mass == 0u) continue;
    const uint32_t mm = static_cast<int>(a.pass[i * a.cap + e]) >= used ? mass : 0u;
    local += mm;
#pragma unroll
    for (int s = 0; s < MAX_HAND; ++s) {
      if (s < rt.n) {
        const int cell = s * a.NC + static_cast<int>((word >> (5 * s)) & 31u);
        if (mm) atomicAdd(&acc[0][cell], static_cast<unsigned long long>(mm));
        if (a.marg0) atomicAdd(&acc[1][cell], static_cast<unsigned long long>(mass));
      }
    }
  }
  if (local) atomicAdd(&bsum, local);
  __syncthreads();
  const int cells = a.H * a.NC;
  for (int x = tid; x < cells; x += TPB) {
    if (acc[0][x]) atomicAdd(a.marg + i * cells + x, acc[0][x]);
    if (a.marg0 && acc[1][x]) atomicAdd(a.marg0 + i * cells + x, acc[1][x]);
  }
  if (tid == 0) a.block_sum[i * a.bpr + q] = bsum;
}

__global__ __launch_bounds__(TPB) void enum_draw_kernel(const EnumArgs a) {
  __shared__ Root rt;
  const int tid = threadIdx.x;
  const long long i = blockIdx.x / a.rpb;
  const int r = static_cast<int>(blockIdx.x - static_cast<unsigned>(i) * a.rpb) * TPB + tid;
  root_setup(a, i, rt);
  if (!rt.scored || rt.N > a.max_hands || rt.N == 0) return;   // (workgroup-uniform) the root's own word is in place
  const int used = level_used(a, i, rt.L);
  const unsigned long long T = a.mass[used * a.m + i];
  if (T == 0ull || r >= a.R) return;
  const unsigned long long row_id = static_cast<unsigned long long>(a.first_row + i);
  uint32_t rnd[4];
  hb::philox4x32_10(0x10000u + static_cast<uint32_t>(r), static_cast<uint32_t>(a.draw), static_cast<uint32_t>(row_id),
                    static_cast<uint32_t>(row_id >> 32), static_cast<uint32_t>(a.seed),
                    static_cast<uint32_t>(a.seed >> 32) ^ static_cast<uint32_t>(a.draw >> 32), rnd);
  const unsigned long long target = __umul64hi((static_cast<unsigned long long>(rnd[0]) << 32) | rnd[1], T);   // < T
  const unsigned nblocks = static_cast<unsigned>((rt.N + BLOCK_HANDS - 1) / BLOCK_HANDS);   // (<= bpr: N <= max_hands)
  unsigned long long base = 0ull;
  unsigned q = 0;
  for (; q < nblocks; ++q) {
    const unsigned long long s = a.block_sum[i * a.bpr + q];
    if (target < base + s) break;
    base += s;
  }
  if (q == nblocks) return;   // (the sums add up to T: not reached)
  const long long first = static_cast<long long>(q) * BLOCK_HANDS;
  const long long last = min(first + BLOCK_HANDS, rt.N);
  for (long long e = first; e < last; ++e) {
    uint32_t word;
    const uint32_t mass = hand_of(rt, static_cast<uint32_t>(e), word);
    if (mass == 0u || static_cast<int>(a.pass[i * a.cap + e]) < used) continue;
    base += mass;
    if (base > target) {
      a.hands[i * a.R + r] = word;
      return;
    }
  }
}

template <class K>
void launch_walk(const EnumArgs& a, unsigned blocks, hipStream_t stream) {
  hipLaunchKernelGGL((enum_walk_kernel<K>), dim3(blocks), dim3(TPB), 0, stream, a);
}

struct EnumVariant {
  int P, C, R, H, INFO, LIFE;
  void (*walk)(const EnumArgs&, unsigned, hipStream_t);
};
template <class K>
constexpr EnumVariant variant() {
  return EnumVariant{K::P, K::C, K::R, K::H, K::INFO, K::LIFE, &launch_walk<K>};
}
using hb::Cfg;
// the configurations hb_rule_playout is compiled for (playout.hip)
const EnumVariant k_variants[] = {
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

// cap = min(max_hands, NC^H): no root has more hands
int64_t hand_cap(const hb_config* cfg, int64_t max_hands) {
  int64_t all = 1;
  for (int s = 0; s < cfg->hand_size; ++s) all *= cfg->colors * cfg->ranks;
  return max_hands < all ? max_hands : all;
}

}  // namespace

extern "C" int64_t hb_belief_enumerate_scratch(const hb_config* cfg, int64_t m, int64_t max_hands) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  if (m < 0) return hb::fail(HB_ERR_INVALID, "m must be >= 0");
  if (max_hands < 1) return hb::fail(HB_ERR_INVALID, "max_hands must be >= 1");
  const int64_t cap = hand_cap(cfg, max_hands);
  const int64_t bpr = (cap + BLOCK_HANDS - 1) / BLOCK_HANDS;
  return m * (cap + 8 * bpr);
}

extern "C" int hb_belief_enumerate(const hb_config* cfg, const uint32_t* cur_rows_dev, int64_t m, int32_t seat,
                                   const uint32_t* hist_rows_dev, const int32_t* hist_moves_dev, const uint8_t* hist_alive_dev,
                                   const uint8_t* hist_valid_dev, int32_t depth, const uint64_t* draws, uint64_t partner_seed,
                                   int64_t first_game_id, const hb_rule* const* rules, const int32_t* n_rules, int64_t max_hands,
                                   int32_t replicas, uint64_t seed, uint64_t draw, int64_t first_row_id, uint8_t* status_dev,
                                   int64_t* space_dev, int64_t* mass_dev, int32_t* n_hands_dev, int32_t* depth_used_dev,
                                   uint8_t* fallback_dev, int64_t* marg_dev, int64_t* marg0_dev, uint32_t* hands_dev,
                                   void* scratch_dev, void* stream) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  const EnumVariant* var = nullptr;
  for (const EnumVariant& v : k_variants)
    if (v.P == cfg->players && v.C == cfg->colors && v.R == cfg->ranks && v.H == cfg->hand_size && v.INFO == cfg->max_info &&
        v.LIFE == cfg->max_life)
      var = &v;
  if (!var)
    return hb::fail(HB_ERR_INVALID,
                    "no compiled kernel for players=%d colors=%d ranks=%d hand=%d info=%d life=%d "
                    "(built: Hanabi-Full / -Small / -Very-Small, 2..5 players)",
                    cfg->players, cfg->colors, cfg->ranks, cfg->hand_size, cfg->max_info, cfg->max_life);
  if (!cur_rows_dev) return hb::fail(HB_ERR_INVALID, "null cur_rows_dev");
  if (m < 0) return hb::fail(HB_ERR_INVALID, "m must be >= 0");
  const int P = cfg->players;
  if (seat < 0 || seat >= P) return hb::fail(HB_ERR_INVALID, "seat %d out of range 0..%d (the observer)", seat, P - 1);
  if (depth < 0 || depth > MAX_DEPTH) return hb::fail(HB_ERR_INVALID, "depth must be 0..%d, got %d", MAX_DEPTH, depth);
  if (depth > 0 && (!hist_rows_dev || !hist_moves_dev || !draws))
    return hb::fail(HB_ERR_INVALID, "null argument: hist_rows_dev, hist_moves_dev and draws are required when depth > 0");
  if (replicas < 1 || replicas > HB_EXACT_MAX_REPLICAS)
    return hb::fail(HB_ERR_INVALID, "replicas must be 1..%d, got %d", HB_EXACT_MAX_REPLICAS, replicas);
  if (max_hands < 1) return hb::fail(HB_ERR_INVALID, "max_hands must be >= 1");
  if (!rules || !n_rules) return hb::fail(HB_ERR_INVALID, "null rules: one rule list and its length per seat");
  for (int p = 0; p < P; ++p) {
    if (n_rules[p] < 0 || n_rules[p] > HB_MAX_RULES) return hb::fail(HB_ERR_INVALID, "seat %d: n_rules must be 0..%d", p, HB_MAX_RULES);
    if (n_rules[p] > 0 && !rules[p]) return hb::fail(HB_ERR_INVALID, "seat %d: null rules", p);
    for (int i = 0; i < n_rules[p]; ++i)
      if (rules[p][i].kind < 0 || rules[p][i].kind >= HB_RULE_KINDS)
        return hb::fail(HB_ERR_INVALID, "seat %d, rule %d: unknown kind %d", p, i, rules[p][i].kind);
  }
  if (!status_dev || !space_dev || !mass_dev || !n_hands_dev || !depth_used_dev || !fallback_dev || !marg_dev || !hands_dev)
    return hb::fail(HB_ERR_INVALID,
                    "null argument: status_dev, space_dev, mass_dev, n_hands_dev, depth_used_dev, fallback_dev, marg_dev and "
                    "hands_dev are required");
  if (!scratch_dev) return hb::fail(HB_ERR_INVALID, "null scratch_dev: hb_belief_enumerate_scratch(cfg, m, max_hands) bytes");
  if (reinterpret_cast<uintptr_t>(scratch_dev) & 7) return hb::fail(HB_ERR_ALIGN, "scratch_dev must be 8-byte aligned");
  const int64_t cap = hand_cap(cfg, max_hands);
  const int64_t bpr = (cap + BLOCK_HANDS - 1) / BLOCK_HANDS;
  const int64_t rpb = (static_cast<int64_t>(replicas) + TPB - 1) / TPB;
  constexpr int64_t kMaxGrid = (int64_t{1} << 31) - 1;
  if (m > 0 && (bpr > kMaxGrid / m || rpb > kMaxGrid / m || static_cast<int64_t>(replicas) > kMaxGrid / m))
    return hb::fail(HB_ERR_INVALID,
                    "m * replicas and m * ceil(min(max_hands, NC^H) / %d) must stay below 2^31: split the call (first_row_id, "
                    "first_game_id)", BLOCK_HANDS);
  if (m == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  EnumArgs a{};
  a.cur = cur_rows_dev;
  a.hist_rows = hist_rows_dev;
  a.hist_moves = hist_moves_dev;
  a.hist_alive = depth > 0 ? hist_alive_dev : nullptr;
  a.hist_valid = depth > 0 ? hist_valid_dev : nullptr;
  a.status = status_dev;
  a.space = reinterpret_cast<long long*>(space_dev);
  a.mass = reinterpret_cast<unsigned long long*>(mass_dev);
  a.n_hands = n_hands_dev;
  a.depth_used = depth_used_dev;
  a.fallback = fallback_dev;
  a.marg = reinterpret_cast<unsigned long long*>(marg_dev);
  a.marg0 = reinterpret_cast<unsigned long long*>(marg0_dev);
  a.hands = hands_dev;
  a.block_sum = static_cast<unsigned long long*>(scratch_dev);   // [m][bpr] 64-bit sums first: they stay 8-byte aligned
  a.pass = static_cast<uint8_t*>(scratch_dev) + m * bpr * 8;     // [m][cap] bytes
  a.m = m;
  a.max_hands = max_hands;
  a.cap = cap;
  a.first_gid = first_game_id;
  a.first_row = first_row_id;
  a.pseed = partner_seed;
  a.seed = seed;
  a.draw = draw;
  for (int d = 0; d < depth; ++d) a.draws[d] = draws[d];
  a.bpr = static_cast<unsigned>(bpr);
  a.rpb = static_cast<unsigned>(rpb);
  a.seat = seat;
  a.depth = depth;
  a.R = replicas;
  a.P = P;
  a.C = cfg->colors;
  a.Rk = cfg->ranks;
  a.H = cfg->hand_size;
  a.D = hb_deck_size(cfg);
  a.SW = hb_state_words(cfg);
  a.NC = cfg->colors * cfg->ranks;
  for (int p = 0; p < P; ++p) {
    a.n_rules[p] = n_rules[p];
    for (int i = 0; i < n_rules[p]; ++i) a.rules[p][i] = rules[p][i];
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned hand_blocks = static_cast<unsigned>(m * bpr);
  hipLaunchKernelGGL(enum_prep_kernel, dim3(static_cast<unsigned>(m)), dim3(TPB), 0, s, a);
  HB_HIP(hipGetLastError());
  var->walk(a, hand_blocks, s);
  HB_HIP(hipGetLastError());
  hipLaunchKernelGGL(enum_marg_kernel, dim3(hand_blocks), dim3(TPB), 0, s, a);
  HB_HIP(hipGetLastError());
  hipLaunchKernelGGL(enum_draw_kernel, dim3(static_cast<unsigned>(m * rpb)), dim3(TPB), 0, s, a);
  HB_HIP(hipGetLastError());
  return HB_OK;
}
