// encode_rows.hip — hb_encode_rows: the canonical observation and legal mask of state rows that belong to no env.
// Host side only: the kernel (encode_rows_kernel) lives beside the env step in env_kernel.hpp, because it calls the env's own
// encoder (encode_seat) and is instantiated per configuration with the env variants (env_full / env_small / env_vsmall.hip).
// Every argument is checked before the device is touched; no CPU fallback exists.
#include <hip/hip_runtime.h>

#include "../../include/hanabi_hip.h"
#include "common.hpp"
#include "env_kernel.hpp"

namespace {
int have_device() {
  static const int ndev = [] {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
  }();
  return ndev > 0 ? HB_OK : hb::fail(HB_ERR_NO_DEVICE, "no HIP device available");
}
}  // namespace

extern "C" int hb_encode_rows(const hb_config* cfg, const uint32_t* rows_dev, int64_t n_rows, int32_t seat, uint32_t* obs_bits_dev,
                              int8_t* obs_dev, int8_t* legal_dev, void* stream) {
  if (!cfg) return hb::fail(HB_ERR_INVALID, "null config");
  if (int rc = hb_config_validate(cfg)) return rc;
  const hb::EnvVariant* var = hb::find_variant(cfg);
  if (!var)
    return hb::fail(HB_ERR_INVALID,
                    "no compiled kernel for players=%d colors=%d ranks=%d hand=%d info=%d life=%d "
                    "(built: Hanabi-Full / -Small / -Very-Small, 2..5 players)",
                    cfg->players, cfg->colors, cfg->ranks, cfg->hand_size, cfg->max_info, cfg->max_life);
  if (!rows_dev) return hb::fail(HB_ERR_INVALID, "rows_dev is required");
  if (n_rows < 0) return hb::fail(HB_ERR_INVALID, "n_rows must be >= 0");
  if (seat < -1 || seat >= cfg->players)
    return hb::fail(HB_ERR_INVALID, "seat %d out of range: -1 (each row's seat to act) or 0..%d", seat, cfg->players - 1);
  if (!obs_bits_dev && !obs_dev) return hb::fail(HB_ERR_INVALID, "one of obs_bits_dev and obs_dev is required");
  if ((reinterpret_cast<uintptr_t>(obs_bits_dev) & 15) || (reinterpret_cast<uintptr_t>(obs_dev) & 15) ||
      (reinterpret_cast<uintptr_t>(legal_dev) & 15))
    return hb::fail(HB_ERR_ALIGN, "obs_bits_dev / obs_dev / legal_dev must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(rows_dev) & 15) return hb::fail(HB_ERR_ALIGN, "rows_dev must be 16-byte aligned");
  if (n_rows > (static_cast<int64_t>(1) << 34)) return hb::fail(HB_ERR_INVALID, "n_rows must stay below 2^34: split the call");
  if (n_rows == 0) return HB_OK;
  if (int rc = have_device()) return rc;
  hb::EncodeArgs a{};
  a.rows = rows_dev;
  a.obs_bits = obs_bits_dev;
  a.obs = obs_dev;
  a.legal = legal_dev;
  a.n = n_rows;
  a.seat = seat;
  // games per wavefront: the env step's own rule (env_api.hip, launch): 32 when only packed rows leave the kernel and the batch
  // is large, 16 otherwise. Results do not depend on it.
  const bool wide = obs_bits_dev && !obs_dev && n_rows >= 32768;
  (wide ? var->e32 : var->e16)(a, static_cast<hipStream_t>(stream));
  HB_HIP(hipGetLastError());
  return HB_OK;
}
