// exact_args_main.cpp — the argument checks of hb_belief_enumerate (include/hanabi_hip_exact.h) called with bad arguments from a
// stand-alone program, for a HOST sanitizer build (`make exact_args` in csrc/: belief_exact.hip's host code with
// -fsanitize=address,undefined; nothing is launched, no device is needed). Every pointer handed over as device memory is a
// number that must never be dereferenced; the host arrays (draws, rules, n_rules) are exactly as long as the call may read.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../../include/hanabi_hip_exact.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (!ok) {
    ++failures;
    std::printf("FAILED: %s (last error: %s)\n", what, hb_last_error());
  }
}

struct Call {
  hb_config cfg{2, 5, 5, 5, 8, 3, 0};
  const hb_config* cfgp = &cfg;
  void* dev = reinterpret_cast<void*>(uintptr_t{64});   // "device memory": never read on the host
  const uint32_t* cur = static_cast<const uint32_t*>(dev);
  const uint32_t* hist_rows = static_cast<const uint32_t*>(dev);
  const int32_t* hist_moves = static_cast<const int32_t*>(dev);
  int64_t m = 4, max_hands = 100;
  int32_t seat = 0, depth = 2, replicas = 3;
  std::vector<uint64_t> draws{5, 3};          // exactly `depth` entries
  std::vector<hb_rule> list{{3, 0, 0.f}, {10, 1, 0.6f}};
  std::vector<const hb_rule*> rules;          // exactly P entries
  std::vector<int32_t> n_rules{2, 0};
  void* outs[9];
  void* scratch = dev;
  bool null_draws = false, null_rules = false, null_n_rules = false;

  Call() {
    rules = {list.data(), nullptr};
    for (void*& o : outs) o = dev;
  }
  int run() {
    return hb_belief_enumerate(cfgp, cur, m, seat, hist_rows, hist_moves, nullptr, nullptr, depth, null_draws ? nullptr : draws.data(), 1, 0,
                               null_rules ? nullptr : rules.data(), null_n_rules ? nullptr : n_rules.data(), max_hands, replicas, 1, 1, 0,
                               static_cast<uint8_t*>(outs[0]), static_cast<int64_t*>(outs[1]), static_cast<int64_t*>(outs[2]),
                               static_cast<int32_t*>(outs[3]), static_cast<int32_t*>(outs[4]), static_cast<uint8_t*>(outs[5]),
                               static_cast<int64_t*>(outs[6]), static_cast<int64_t*>(outs[7]), static_cast<uint32_t*>(outs[8]), scratch,
                               nullptr);
  }
};

}  // namespace

int main() {
  { Call c; c.cfgp = nullptr; expect(c.run() == HB_ERR_INVALID, "null cfg"); }
  { Call c; c.cfg.players = 6; expect(c.run() == HB_ERR_INVALID, "invalid cfg"); }
  { Call c; c.cfg.colors = 3; expect(c.run() == HB_ERR_INVALID, "a configuration without a kernel"); }
  { Call c; c.cur = nullptr; expect(c.run() == HB_ERR_INVALID, "null cur_rows_dev"); }
  { Call c; c.m = -1; expect(c.run() == HB_ERR_INVALID, "m < 0"); }
  for (int seat : {-1, 2}) { Call c; c.seat = seat; expect(c.run() == HB_ERR_INVALID, "seat out of range"); }
  for (int d : {-1, 9}) { Call c; c.depth = d; c.draws.assign(9, 1); expect(c.run() == HB_ERR_INVALID, "depth out of range"); }
  { Call c; c.hist_rows = nullptr; expect(c.run() == HB_ERR_INVALID, "null hist_rows_dev at depth 2"); }
  { Call c; c.hist_moves = nullptr; expect(c.run() == HB_ERR_INVALID, "null hist_moves_dev at depth 2"); }
  { Call c; c.null_draws = true; expect(c.run() == HB_ERR_INVALID, "null draws at depth 2"); }
  for (int r : {0, (1 << 20) + 1}) { Call c; c.replicas = r; expect(c.run() == HB_ERR_INVALID, "replicas out of range"); }
  { Call c; c.max_hands = 0; expect(c.run() == HB_ERR_INVALID, "max_hands < 1"); }
  { Call c; c.null_rules = true; expect(c.run() == HB_ERR_INVALID, "null rules"); }
  { Call c; c.null_n_rules = true; expect(c.run() == HB_ERR_INVALID, "null n_rules"); }
  for (int n : {-1, HB_MAX_RULES + 1}) { Call c; c.n_rules[1] = n; expect(c.run() == HB_ERR_INVALID, "n_rules out of range"); }
  { Call c; c.n_rules[1] = 1; expect(c.run() == HB_ERR_INVALID, "a null list of a non-empty one"); }
  for (int k : {-1, static_cast<int>(HB_RULE_KINDS)}) { Call c; c.list[1].kind = k; expect(c.run() == HB_ERR_INVALID, "unknown rule kind"); }
  for (int o = 0; o < 9; ++o) {
    Call c;
    c.outs[o] = nullptr;
    c.m = o == 7 ? 0 : 4;   // marg0_dev may be NULL: the call passes every check (m == 0: a no-op)
    expect(c.run() == (o == 7 ? HB_OK : HB_ERR_INVALID), "a null output");
  }
  { Call c; c.scratch = nullptr; expect(c.run() == HB_ERR_INVALID, "null scratch_dev"); }
  { Call c; c.scratch = reinterpret_cast<void*>(uintptr_t{68}); expect(c.run() == HB_ERR_ALIGN, "scratch_dev not 8-byte aligned"); }
  { Call c; c.m = int64_t{1} << 22; c.max_hands = int64_t{1} << 40; expect(c.run() == HB_ERR_INVALID, "too many blocks of hands"); }
  { Call c; c.m = int64_t{1} << 12; c.replicas = 1 << 20; expect(c.run() == HB_ERR_INVALID, "too many replicas in all"); }
  { Call c; c.m = 0; expect(c.run() == HB_OK, "m == 0 is a no-op"); }
  { Call c; c.m = 0; c.depth = 0; c.hist_rows = nullptr; c.hist_moves = nullptr; c.null_draws = true; expect(c.run() == HB_OK, "depth 0 reads no history"); }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess) n_dev = 0;
  if (n_dev == 0) {   // (with a device the call would launch on the fake pointers: this program is for machines without one)
    Call c;
    c.depth = 8;
    c.draws.assign(8, 7);
    c.n_rules = {2, 2};
    c.rules[1] = c.list.data();
    expect(c.run() == HB_ERR_NO_DEVICE, "a call that passes every check asks for the device last");
  } else {
    std::printf("a HIP device is present: the call that passes every check is not made\n");
  }
  { hb_config cfg{2, 5, 5, 5, 8, 3, 0};
    expect(hb_belief_enumerate_scratch(&cfg, 3, 1025) == 3 * (1025 + 8 * 2), "scratch size");
    expect(hb_belief_enumerate_scratch(&cfg, 1, int64_t{1} << 40) == 9765625 + 8 * 9537, "scratch size is capped by NC^H");
    expect(hb_belief_enumerate_scratch(nullptr, 3, 5) < 0 && hb_belief_enumerate_scratch(&cfg, -1, 5) < 0 &&
           hb_belief_enumerate_scratch(&cfg, 1, 0) < 0, "scratch size of bad arguments"); }
  std::printf(failures ? "%d checks failed\n" : "exact_args: all argument checks hold\n", failures);
  return failures ? 1 : 0;
}
