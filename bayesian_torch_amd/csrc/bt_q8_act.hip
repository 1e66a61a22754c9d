// u8 activations between the INT8 layers (quantization/qact.py): the element-wise operators of a quantised
// model on the channel-blocked image [N][CB][H][W][16] that bt_q8_common.h's walk reads and writes -- quantise, dequantise, ReLU,
// add / add_relu, max-pool, the global average pool and the un-blocking flatten. They replace, in the reference's QResNet /
// QuantizableResNet, quantize_per_tensor, dequantize, nn.ReLU, torch.ops.quantized.add / add_relu, nn.MaxPool2d, the average pool and
// flatten on quint8 tensors -- which exist on the CPU only -- bit for bit (include/bt_hip.h has the arithmetic). Each is one launch of
// grid-stride threads over 16-byte units (or single bytes where the result is small): nothing here is a hot path beside the convs.
#include "bt_q8_common.h"

namespace bt {

constexpr int kActThreads = 256;
constexpr long long kActMaxBlocks = 8192;

struct ActShape {
  long long N, C, HW, CB;
  int H, W;
};

__device__ __forceinline__ unsigned byte_of(const v4i& v, int j) { return ((unsigned)v[j >> 2] >> (8 * (j & 3))) & 0xFFu; }

#define BT_ACT_UNITS(u, n_units) for (long long u = (long long)blockIdx.x * kActThreads + threadIdx.x; u < (n_units); u += (long long)gridDim.x * kActThreads)

// unit u = (n, cb, p) of [N][CB][HW][16]
__global__ __launch_bounds__(kActThreads) void act_quantize_kernel(const float* __restrict__ x, ActShape s, float inv, int z, v4i* __restrict__ q) {
  BT_ACT_UNITS(u, s.N * s.CB * s.HW) {
    const long long p = u % s.HW, r = u / s.HW;
    const long long cb = r % s.CB, n = r / s.CB;
    v4i w = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const long long c = cb * 16 + j;
      const int lv = c < s.C ? q8_quant_x(x[(n * s.C + c) * s.HW + p], inv, z) : z;
      w[j >> 2] |= lv << (8 * (j & 3));
    }
    q[u] = w;
  }
}

__global__ __launch_bounds__(kActThreads) void act_dequantize_kernel(const v4i* __restrict__ q, ActShape s, float scale, int z, float* __restrict__ out) {
  BT_ACT_UNITS(u, s.N * s.CB * s.HW) {
    const long long p = u % s.HW, r = u / s.HW;
    const long long cb = r % s.CB, n = r / s.CB;
    const v4i w = q[u];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const long long c = cb * 16 + j;
      if (c < s.C) out[(n * s.C + c) * s.HW + p] = __fmul_rn((float)((int)byte_of(w, j) - z), scale);
    }
  }
}

// (q and out may be one buffer: a unit is read and written by one thread)
__global__ __launch_bounds__(kActThreads) void act_relu_kernel(const v4i* q, long long n_units, int z, v4i* out) {
  BT_ACT_UNITS(u, n_units) {
    const v4i w = q[u];
    v4i r = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const unsigned b = byte_of(w, j);
      r[j >> 2] |= (int)((b > (unsigned)z ? b : (unsigned)z) << (8 * (j & 3)));
    }
    out[u] = r;
  }
}

struct ActAdd {
  float s_a, nzs_a, s_b, nzs_b, inv_out;
  int z_out, relu;
};

__global__ __launch_bounds__(kActThreads) void act_add_kernel(const v4i* __restrict__ a, const v4i* __restrict__ b, ActShape s, ActAdd m, v4i* __restrict__ out) {
  BT_ACT_UNITS(u, s.N * s.CB * s.HW) {
    const long long cb = (u / s.HW) % s.CB;
    const v4i wa = a[u], wb = b[u];
    v4i r = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      float lv = (float)m.z_out;
      if (cb * 16 + j < s.C) {
        // torch's quantized.add: either operand dequantised by ONE fused rounding, the fp32 sum, times 1 / s_out
        const float da = __fmaf_rn((float)byte_of(wa, j), m.s_a, m.nzs_a);
        const float db = __fmaf_rn((float)byte_of(wb, j), m.s_b, m.nzs_b);
        lv = q8_level(__fmul_rn(__fadd_rn(da, db), m.inv_out), m.z_out);
        if (m.relu) lv = fmaxf(lv, (float)m.z_out);
      }
      r[j >> 2] |= (int)lv << (8 * (j & 3));
    }
    out[u] = r;
  }
}

struct ActPool {
  int kh, kw, sh, sw, ph, pw, Ho, Wo;
};

// output unit u = (n, cb, oh, ow): the bytewise maximum over the window's positions inside the image (a padding channel's bytes are z
// at every position, so z comes out)
__global__ __launch_bounds__(kActThreads) void act_max_pool_kernel(const v4i* __restrict__ q, ActShape s, ActPool g, v4i* __restrict__ out) {
  const long long hwo = (long long)g.Ho * g.Wo;
  BT_ACT_UNITS(u, s.N * s.CB * hwo) {
    const long long p = u % hwo, img = u / hwo;   // img = n * CB + cb
    const int oh = (int)(p / g.Wo), ow = (int)(p - (long long)oh * g.Wo);
    unsigned best[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) best[j] = 0u;
    for (int ky = 0; ky < g.kh; ++ky) {
      const int ih = oh * g.sh - g.ph + ky;
      if (ih < 0 || ih >= s.H) continue;
      for (int kx = 0; kx < g.kw; ++kx) {
        const int iw = ow * g.sw - g.pw + kx;
        if (iw < 0 || iw >= s.W) continue;
        const v4i w = q[img * s.HW + (long long)ih * s.W + iw];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const unsigned b = byte_of(w, j);
          best[j] = b > best[j] ? b : best[j];
        }
      }
    }
    v4i r = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) r[j >> 2] |= (int)(best[j] << (8 * (j & 3)));
    out[u] = r;
  }
}

// output byte i = (n, cb, j) of [N][CB][16]: the plane's sum, then torch's float(sum - z * n) * float(1 / n) + z, rounded once to an integer
__global__ __launch_bounds__(kActThreads) void act_avg_pool_kernel(const uint8_t* __restrict__ q, ActShape s, float inv_n, int z, uint8_t* __restrict__ out) {
  BT_ACT_UNITS(i, s.N * s.CB * 16) {
    const int j = (int)(i & 15);
    const long long img = i >> 4;
    int lv = z;
    if ((img % s.CB) * 16 + j < s.C) {
      const uint8_t* src = q + img * s.HW * 16 + j;
      int sum = 0;
      for (long long p = 0; p < s.HW; ++p) sum += src[p * 16];
      const float t = __fadd_rn(__fmul_rn((float)(sum - z * (int)s.HW), inv_n), (float)z);
      lv = (int)fminf(fmaxf(rintf(t), 0.f), 255.f);
    }
    out[i] = (uint8_t)lv;
  }
}

// output byte i = (n, f) of [N][F16], f = c * HW + p
__global__ __launch_bounds__(kActThreads) void act_unblock_kernel(const uint8_t* __restrict__ q, ActShape s, long long F, long long F16, int z, uint8_t* __restrict__ out) {
  BT_ACT_UNITS(i, s.N * F16) {
    const long long n = i / F16, f = i - n * F16;
    int lv = z;
    if (f < F) {
      const long long c = f / s.HW, p = f - c * s.HW;
      lv = q[((n * s.CB + (c >> 4)) * s.HW + p) * 16 + (c & 15)];
    }
    out[i] = (uint8_t)lv;
  }
}

static int act_shape(const Q8Fail& fail, long long N, long long C, long long H, long long W, ActShape& s) {
  if (N < 1 || C < 1 || H < 1 || W < 1) return fail(BT_ERR_BAD_ARG, "N, C, H or W < 1");
  if (H >= (1ll << 31) || W >= (1ll << 31) || N >= (1ll << 40) || C >= (1ll << 40)) return fail(BT_ERR_UNSUPPORTED, "image too large");
  const long long CB = (C + 15) / 16;
  if ((double)N * (double)CB * (double)H * (double)W * 16.0 >= (double)(1ll << 40)) return fail(BT_ERR_UNSUPPORTED, "an image of 2^40 bytes or more");
  s = {N, C, H * W, CB, (int)H, (int)W};
  return BT_OK;
}

static int act_pair(const Q8Fail& fail, double scale, int z) {
  const float sf = (float)scale;
  if (!(scale > 0.0) || !(sf > 0.f) || !(sf < INFINITY) || !(1.0f / sf < INFINITY)) return fail(BT_ERR_BAD_ARG, "a scale <= 0 (or one whose fp32 value or reciprocal is not finite)");
  if (z < 0 || z > 255) return fail(BT_ERR_BAD_ARG, "a zero point outside 0..255");
  return BT_OK;
}

static int act_aligned(const Q8Fail& fail, const void* p) {
  if (!p) return fail(BT_ERR_BAD_ARG, "a null pointer");
  if (((uintptr_t)p) & 15u) return fail(BT_ERR_BAD_ARG, "a blocked u8 image must be 16-byte aligned");
  return BT_OK;
}

static dim3 act_grid(long long n) {
  long long g = (n + kActThreads - 1) / kActThreads;
  return dim3((unsigned)(g > kActMaxBlocks ? kActMaxBlocks : (g < 1 ? 1 : g)));
}

}  // namespace bt

using namespace bt;

extern "C" int bt_q8_act_quantize(const float* x, int64_t N, int64_t C, int64_t H, int64_t W, double scale, int32_t zero_point, uint8_t* q, bt_stream_t stream) {
  const Q8Fail fail = {"bt_q8_act_quantize"};
  ActShape s;
  if (!x) return fail(BT_ERR_BAD_ARG, "a null pointer");
  if (int rc = act_aligned(fail, q)) return rc;
  if (int rc = act_shape(fail, N, C, H, W, s)) return rc;
  if (int rc = act_pair(fail, scale, zero_point)) return rc;
  return launch_kernel(act_quantize_kernel, nullptr, fail.who, act_grid(s.N * s.CB * s.HW), dim3(kActThreads), 0, 0, (hipStream_t)stream, x, s, 1.0f / (float)scale,
                       (int)zero_point, reinterpret_cast<v4i*>(q));
}

extern "C" int bt_q8_act_dequantize(const uint8_t* q, int64_t N, int64_t C, int64_t H, int64_t W, double scale, int32_t zero_point, float* out, bt_stream_t stream) {
  const Q8Fail fail = {"bt_q8_act_dequantize"};
  ActShape s;
  if (!out) return fail(BT_ERR_BAD_ARG, "a null pointer");
  if (int rc = act_aligned(fail, q)) return rc;
  if (int rc = act_shape(fail, N, C, H, W, s)) return rc;
  if (int rc = act_pair(fail, scale, zero_point)) return rc;
  return launch_kernel(act_dequantize_kernel, nullptr, fail.who, act_grid(s.N * s.CB * s.HW), dim3(kActThreads), 0, 0, (hipStream_t)stream,
                       reinterpret_cast<const v4i*>(q), s, (float)scale, (int)zero_point, out);
}

extern "C" int bt_q8_act_relu(const uint8_t* q, int64_t N, int64_t C, int64_t H, int64_t W, int32_t zero_point, uint8_t* out, bt_stream_t stream) {
  const Q8Fail fail = {"bt_q8_act_relu"};
  ActShape s;
  if (int rc = act_aligned(fail, q)) return rc;
  if (int rc = act_aligned(fail, out)) return rc;
  if (int rc = act_shape(fail, N, C, H, W, s)) return rc;
  if (int rc = act_pair(fail, 1.0, zero_point)) return rc;
  const long long n = s.N * s.CB * s.HW;
  return launch_kernel(act_relu_kernel, nullptr, fail.who, act_grid(n), dim3(kActThreads), 0, 0, (hipStream_t)stream, reinterpret_cast<const v4i*>(q), n,
                       (int)zero_point, reinterpret_cast<v4i*>(out));
}

extern "C" int bt_q8_act_add(const uint8_t* a, const int64_t* a_shape, double s_a, int32_t z_a, const uint8_t* b, const int64_t* b_shape, double s_b, int32_t z_b,
                             double s_out, int32_t z_out, int32_t relu, uint8_t* out, bt_stream_t stream) {
  const Q8Fail fail = {"bt_q8_act_add"};
  ActShape s;
  if (!a_shape || !b_shape) return fail(BT_ERR_BAD_ARG, "a null pointer");
  if (int rc = act_aligned(fail, a)) return rc;
  if (int rc = act_aligned(fail, b)) return rc;
  if (int rc = act_aligned(fail, out)) return rc;
  for (int i = 0; i < 4; ++i)
    if (a_shape[i] != b_shape[i]) return fail(BT_ERR_BAD_ARG, "a and b differ in shape");
  if (int rc = act_shape(fail, a_shape[0], a_shape[1], a_shape[2], a_shape[3], s)) return rc;
  if (int rc = act_pair(fail, s_a, z_a)) return rc;
  if (int rc = act_pair(fail, s_b, z_b)) return rc;
  if (int rc = act_pair(fail, s_out, z_out)) return rc;
  const float fa = (float)s_a, fb = (float)s_b;
  const ActAdd m = {fa, -((float)z_a * fa), fb, -((float)z_b * fb), 1.0f / (float)s_out, (int)z_out, relu != 0};
  return launch_kernel(act_add_kernel, nullptr, fail.who, act_grid(s.N * s.CB * s.HW), dim3(kActThreads), 0, 0, (hipStream_t)stream,
                       reinterpret_cast<const v4i*>(a), reinterpret_cast<const v4i*>(b), s, m, reinterpret_cast<v4i*>(out));
}

extern "C" int bt_q8_act_max_pool2d(const uint8_t* q, int64_t N, int64_t C, int64_t H, int64_t W, int32_t kh, int32_t kw, int32_t sh, int32_t sw, int32_t ph, int32_t pw,
                                    uint8_t* out, bt_stream_t stream) {
  const Q8Fail fail = {"bt_q8_act_max_pool2d"};
  ActShape s;
  if (int rc = act_aligned(fail, q)) return rc;
  if (int rc = act_aligned(fail, out)) return rc;
  if (int rc = act_shape(fail, N, C, H, W, s)) return rc;
  if (kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 || 2 * ph > kh || 2 * pw > kw)
    return fail(BT_ERR_BAD_ARG, "kernel or stride < 1, padding < 0 or more than half the kernel");
  const long long Ho = (H + 2ll * ph - kh) / sh + 1, Wo = (W + 2ll * pw - kw) / sw + 1;
  if (H + 2ll * ph < kh || W + 2ll * pw < kw || Ho < 1 || Wo < 1) return fail(BT_ERR_BAD_ARG, "pooling output would be empty");
  const ActPool g = {kh, kw, sh, sw, ph, pw, (int)Ho, (int)Wo};
  return launch_kernel(act_max_pool_kernel, nullptr, fail.who, act_grid(s.N * s.CB * Ho * Wo), dim3(kActThreads), 0, 0, (hipStream_t)stream,
                       reinterpret_cast<const v4i*>(q), s, g, reinterpret_cast<v4i*>(out));
}

extern "C" int bt_q8_act_avg_pool(const uint8_t* q, int64_t N, int64_t C, int64_t H, int64_t W, int32_t zero_point, uint8_t* out, bt_stream_t stream) {
  const Q8Fail fail = {"bt_q8_act_avg_pool"};
  ActShape s;
  if (int rc = act_aligned(fail, q)) return rc;
  if (int rc = act_aligned(fail, out)) return rc;
  if (int rc = act_shape(fail, N, C, H, W, s)) return rc;
  if (int rc = act_pair(fail, 1.0, zero_point)) return rc;
  if (s.HW >= (1ll << 23)) return fail(BT_ERR_UNSUPPORTED, "H * W >= 2^23");
  return launch_kernel(act_avg_pool_kernel, nullptr, fail.who, act_grid(s.N * s.CB * 16), dim3(kActThreads), 0, 0, (hipStream_t)stream, q, s, 1.0f / (float)s.HW,
                       (int)zero_point, out);
}

extern "C" int bt_q8_act_unblock(const uint8_t* q, int64_t N, int64_t C, int64_t H, int64_t W, int32_t zero_point, uint8_t* out, bt_stream_t stream) {
  const Q8Fail fail = {"bt_q8_act_unblock"};
  ActShape s;
  if (int rc = act_aligned(fail, q)) return rc;
  if (int rc = act_aligned(fail, out)) return rc;
  if (int rc = act_shape(fail, N, C, H, W, s)) return rc;
  if (int rc = act_pair(fail, 1.0, zero_point)) return rc;
  const long long F = s.C * s.HW, F16 = (F + 15) & ~15ll;
  return launch_kernel(act_unblock_kernel, nullptr, fail.who, act_grid(s.N * F16), dim3(kActThreads), 0, 0, (hipStream_t)stream, q, s, F, F16, (int)zero_point, out);
}
