// Host-side helpers shared by the C-ABI entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <set>
#include <utility>

#include "../../include/bt_hip.h"
#include "bt_device.h"

namespace bt {

int set_error(int code, const char* msg);  // records msg for bt_last_error_string(); returns code
void note_kernel(const char* name);         // records the kernel instance a fused launch chose (bt_last_kernel_name)
bool plan_only();                           // test seam (bt_debug_plan_only): launch_kernel records the name and launches nothing

inline int check_launch(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return BT_OK;
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: launch failed: %s", who, hipGetErrorString(e));
  return set_error(BT_ERR_HIP_BASE - (int)e, buf);
}

// Raises kern's dynamic-LDS limit to `bytes` (the most any of its launches asks for) once per (kernel, device).
inline int raise_lds_limit(const void* kern, int bytes, const char* who) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> done;
  char buf[256];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    snprintf(buf, sizeof(buf), "%s: hipGetDevice failed", who);
    return set_error(BT_ERR_HIP_BASE, buf);
  }
  std::lock_guard<std::mutex> lock(mu);
  if (done.count({kern, dev})) return BT_OK;
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
    snprintf(buf, sizeof(buf), "%s: cannot raise the dynamic LDS limit", who);
    return set_error(BT_ERR_HIP_BASE, buf);
  }
  done.insert({kern, dev});
  return BT_OK;
}

// Launches kern with `lds` bytes of dynamic LDS after raising its limit to lds_limit; records `name` for bt_last_kernel_name
// (null: not a fused forward, the name is left alone).
template <typename... P, typename... A>
int launch_kernel(void (*kern)(P...), const char* name, const char* who, dim3 grid, dim3 block, int lds, int lds_limit, hipStream_t stream,
                  const A&... args) {
  if (plan_only()) {
    if (name) note_kernel(name);
    return BT_OK;
  }
  if (int rc = raise_lds_limit(reinterpret_cast<const void*>(kern), lds_limit, who)) return rc;
  if (name) note_kernel(name);
  hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
  return check_launch(who);
}

inline RngKey make_key(const bt_rng& r, uint32_t tensor) {
  RngKey k;
  k.seed_lo = (uint32_t)r.seed;
  k.seed_hi = (uint32_t)(r.seed >> 32);
  k.call = r.call;
  k.layer_tensor = layer_tensor_word(r.layer_id, tensor);
  return k;
}

}  // namespace bt
