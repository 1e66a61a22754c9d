// What the two INT8 forwards (bt_q8.hip: Reparameterization, bt_q8_flip.hip: Flipout) share: the tile geometry, the byte helpers, the
// walk over (live) taps, and the host's argument and geometry checks. One definition of each, so the two kernels walk K alike and the
// two entry points refuse alike.
#pragma once
#include "bt_api_internal.h"

namespace bt {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kQ8Threads = 256;
constexpr int kQ8TM = 64;    // output channels per workgroup
constexpr int kQ8TN = 128;   // output pixels per workgroup
constexpr int kQ8SU = 4;     // units (16 K positions each) per stage

__device__ __forceinline__ int clamp_i8(float v) { return (int)fminf(fmaxf(v, -128.f), 127.f); }

__device__ __forceinline__ int sext8(int word, int j) { return (int)(int8_t)((unsigned)word >> (8 * j)); }

// Walked unit v -> (tap t, 16-channel block cb): the v / CB-th live tap when taps are pruned, else the v / CB-th tap. A: a kernel's
// argument block with CB, pruned and live_taps.
template <class A>
__device__ __forceinline__ void q8_unit(const A& a, int v, int& t, int& cb) {
  const int tv = v / a.CB;
  cb = v - tv * a.CB;
  t = a.pruned ? (int)((a.live_taps >> (4 * tv)) & 15u) : tv;
}

// Taps that read padding for EVERY output pixel: where a padding position is the MFMA's zero and no correction term reads the row
// sum, such a tap contributes nothing and is not walked (a 3 x 3 kernel on a 1 x 1 map keeps its centre tap). -> whether taps are
// pruned; then `live` holds the live taps in ascending order, four bits each, and VU the units walked.
inline bool q8_live_taps(const bt_conv2d_geom& g, long long Ho, long long Wo, int CB, uint64_t& live, int& VU) {
  const long long taps = (long long)g.kh * g.kw;
  if (taps > 16) return false;
  uint64_t lv = 0;
  int n_live = 0;
  for (int ky = 0; ky < g.kh; ++ky) {
    bool row = false;
    for (long long oh = 0; oh < Ho && !row; ++oh) {
      const long long ih = oh * g.sh - g.ph + (long long)ky * g.dh;
      row = ih >= 0 && ih < g.H;
    }
    for (int kx = 0; kx < g.kw; ++kx) {
      bool col = false;
      for (long long ow = 0; ow < Wo && !col; ++ow) {
        const long long iw = ow * g.sw - g.pw + (long long)kx * g.dw;
        col = iw >= 0 && iw < g.W;
      }
      if (row && col) lv |= (uint64_t)(ky * g.kw + kx) << (4 * n_live++);
    }
  }
  if (n_live >= taps || n_live <= 0) return false;
  live = lv, VU = n_live * CB;
  return true;
}

// The refusals the INT8 forwards have in common, in two steps between which an entry point checks its own draws and (scale, zero
// point) pairs. Each returns BT_OK or the recorded error.
struct Q8Fail {
  const char* who;
  int operator()(int code, const char* what) const {
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return set_error(code, buf);
  }
};

inline int q8_check_operands(const Q8Fail& fail, const void* x, const void* p, const void* out, int S, long long x_sample_stride, const int8_t* mu_packed,
                             const int8_t* sigma_packed, const bt_conv2d_geom& g) {
  if (!x || !p || !out || S <= 0 || x_sample_stride < 0) return fail(BT_ERR_BAD_ARG, "null x / p / out, S <= 0 or a negative sample stride");
  if (!mu_packed || !sigma_packed) return fail(BT_ERR_BAD_ARG, "the int8 packs are missing (bt_q8_pack)");
  if ((((uintptr_t)mu_packed) | ((uintptr_t)sigma_packed)) & 15u) return fail(BT_ERR_BAD_ARG, "the int8 packs must be 16-byte aligned");
  if (const char* ge = geom_error(g)) return fail(BT_ERR_BAD_ARG, ge);
  return BT_OK;
}

// The int32 accumulator's bound, an empty output, and the index ranges of the draw streams -> Ho, Wo, npix.
inline int q8_check_sizes(const Q8Fail& fail, const bt_conv2d_geom& g, int S, long long& Ho, long long& Wo, long long& npix) {
  const long long taps = (long long)g.kh * g.kw, K = taps * g.Ci;
  if (K * 32640ll >= (1ll << 31)) return fail(BT_ERR_UNSUPPORTED, "K * 32640 >= 2^31: the int32 accumulator could overflow");
  Ho = conv_out_h(g), Wo = conv_out_w(g);
  if (Ho <= 0 || Wo <= 0) return fail(BT_ERR_BAD_ARG, "convolution output would be empty");
  npix = (long long)g.B * Ho * Wo;
  if (S > 65535 || npix >= (1ll << 31) || (long long)g.Ci * g.H * g.W * g.B >= (1ll << 40)) return fail(BT_ERR_UNSUPPORTED, "S > 65535 or tensor too large");
  if ((long long)g.Co * taps * (((long long)g.Ci + 3) >> 2) > (1ll << 32)) return fail(BT_ERR_UNSUPPORTED, "weight tensor too large for the draw stream");
  return BT_OK;
}

}  // namespace bt
