// Host-side helpers shared by the C-ABI entry points.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>

#include <atomic>
#include <mutex>
#include <set>
#include <utility>

#include "../../include/bt_hip.h"
#include "bt_device.h"

namespace bt {

int set_error(int code, const char* msg);  // records msg for bt_last_error_string(); returns code
void note_kernel(const char* name);         // records the kernel instance a fused launch chose (bt_last_kernel_name)
bool plan_only();                           // test seam (bt_debug_plan_only): launch_kernel records the launch and launches nothing
void note_launch(dim3 grid, dim3 block, int lds, int lds_limit, uint64_t args_digest);   // plan-only: bt_debug_last_launch_record

// A process-wide int knob: first read from an environment variable (`parse` gets getenv's answer, null when unset; env == null:
// no variable), overridable at any time by a hook (set).
class EnvKnob {
 public:
  constexpr EnvKnob(const char* env, int (*parse)(const char*)) : env_(env), parse_(parse) {}
  int get() {
    int v = v_.load(std::memory_order_relaxed);
    if (v == INT_MIN) {
      v = parse_(env_ ? getenv(env_) : nullptr);
      v_.store(v, std::memory_order_relaxed);
    }
    return v;
  }
  void set(int v) { v_.store(v, std::memory_order_relaxed); }

 private:
  const char* env_;
  int (*parse_)(const char*);
  std::atomic<int> v_{INT_MIN};
};
// 64-bit FNV-1a over a kernel argument's bytes (plan-only records). A type with padding overloads digest_arg (FwdArgs).
inline uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
  for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
  return h;
}
template <typename T>
uint64_t digest_arg(uint64_t h, const T& v) { return fnv1a(h, &v, sizeof(T)); }

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

// Launches kern with `lds` bytes of dynamic LDS after raising its limit to lds_limit (0: the kernel asks for none, nothing to raise);
// records `name` for bt_last_kernel_name (null: not a fused forward, the name is left alone).
template <typename... P, typename... A>
int launch_kernel(void (*kern)(P...), const char* name, const char* who, dim3 grid, dim3 block, int lds, int lds_limit, hipStream_t stream,
                  const A&... args) {
  if (plan_only()) {
    if (name) note_kernel(name);
    uint64_t h = 14695981039346656037ull;
    ((h = digest_arg(h, args)), ...);
    note_launch(grid, block, lds, lds_limit, h);
    return BT_OK;
  }
  if (lds_limit)
    if (int rc = raise_lds_limit(reinterpret_cast<const void*>(kern), lds_limit, who)) return rc;
  if (name) note_kernel(name);
  hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
  return check_launch(who);
}

// Output extent of a convolution along one axis (the one place the formula is written), and a bt_conv2d_geom's.
inline long long conv_out(long long in, int k, int s, int p, int d) { return (in + 2ll * p - (long long)d * (k - 1) - 1) / s + 1; }
inline long long conv_out_h(const bt_conv2d_geom& g) { return conv_out(g.H, g.kh, g.sh, g.ph, g.dh); }
inline long long conv_out_w(const bt_conv2d_geom& g) { return conv_out(g.W, g.kw, g.sw, g.pw, g.dw); }
// What every entry point refuses in a geometry before it divides by any of it: null, or the forward's text (in the forward's order).
// An empty output (conv_out_h / conv_out_w <= 0) is the caller's next question.
inline const char* geom_error(const bt_conv2d_geom& g) {
  if (g.B <= 0 || g.Ci <= 0 || g.H <= 0 || g.W <= 0 || g.Co <= 0 || g.kh <= 0 || g.kw <= 0) return "non-positive dimension";
  if (g.sh <= 0 || g.sw <= 0 || g.dh <= 0 || g.dw <= 0 || g.ph < 0 || g.pw < 0 || g.groups <= 0) return "bad stride / padding / dilation / groups";
  if (g.Ci % g.groups || g.Co % g.groups) return "invalid in_channels size";  // conv_variational.py:270-273
  return nullptr;
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
