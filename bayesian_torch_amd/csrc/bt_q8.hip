// INT8 post-training-quantised Reparameterization layers (layers/_quantized.py): one fused forward on v_mfma_i32_32x32x32_i8 for
// Conv2d and Linear (the 1 x 1 map), MC-batched over S. Replaces, in reference layers/variational_layers/quantize_conv_variational.py
// :495-547 and quantize_linear_variational.py:173-219, quantize_per_tensor(eps), quantized.mul, quantized.add, quantize_per_tensor(x)
// and the quantised conv2d / linear -- which exist on the CPU only. The arithmetic is include/bt_hip.h's (bt_q8_params): integer
// accumulation has no order, so the output is the reference's bit for bit.
//
// The kernel is bt_q8_common.h's walk, q8_walk_kernel, over the Q8Reparam chain below: ONE contraction, whose weights are
// w = qadd(qmul(q_sigma, e), q_mu) of the draws, whose activation is xq - 128 and whose output is one requantisation (fbgemm's).
// This file also holds bt_q8_pack, which both chains' packs come from.
#include "bt_q8_common.h"

namespace bt {

struct Q8Args : Q8Core {
  float m_mul, s_mul, s_mu, inv_add, m_out, inv_atw;   // inv_atw: 1 / (s_in * s_add); m_out: s_in * s_add / s_out -- fp32 operations
};

struct Q8Reparam {
  static constexpr int kC = 1;
  static constexpr bool kWords = true;   // xq - 128 of four levels is one sign-bit flip of their word
  typedef Q8Args Args;
  const Args& a;
  __device__ __forceinline__ Q8Reparam(const Args& args, int, uint32_t, uint32_t) : a(args) {}

  // b = mu_b + sigma_b * eps_b
  __device__ __forceinline__ void bias(float mu, bool has_sigma, float sigma, float eps, float (&b)[1]) const {
    b[0] = has_sigma ? __fadd_rn(mu, __fmul_rn(sigma, eps)) : mu;
  }
  // e -> p -> w of four weights (include/bt_hip.h): one fp32 rounding per operation.
  __device__ __forceinline__ void weights(int qm, int qs, const float (&eps)[4], int (&w)[1], int (&sum)[1]) const {
    int word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = clamp_i8(rintf(__fmul_rn(eps[j], a.inv_eps)));
      const int p = clamp_i8(rintf(__fmul_rn((float)(sext8(qs, j) * e), a.m_mul)));
      const float t = __fadd_rn(__fmul_rn((float)p, a.s_mul), __fmul_rn((float)sext8(qm, j), a.s_mu));
      const int v = clamp_i8(rintf(__fmul_rn(t, a.inv_add)));
      sum[0] += v;
      word |= (v & 0xFF) << (8 * j);
    }
    w[0] = word;
  }
  __device__ __forceinline__ void pads(int (&p)[1]) const { p[0] = (a.z_in - 128) & 0xFF; }
  __device__ __forceinline__ void activation(int xq, long long, int (&b)[1]) const { b[0] = (xq - 128) & 0xFF; }
  __device__ __forceinline__ void activation_words(int lv, int (&w)[1]) const { w[0] = lv ^ (int)0x80808080u; }
  __device__ __forceinline__ void corrections(int (&zc)[1]) const { zc[0] = 128 - a.z_in; }
  // fbgemm's: ONE rounding of b * (1 / a) + float(acc)
  __device__ __forceinline__ float output(const int (&acc)[1], const float (&b)[1], long long) const {
    return q8_level(__fmul_rn(__fmaf_rn(b[0], a.inv_atw, (float)acc[0]), a.m_out), a.z_out);
  }
};

// packed[(co * taps + t) * Ci16 + c] <- natural[co][c][t]; one thread per packed byte.
__global__ __launch_bounds__(256) void q8_pack_kernel(const int8_t* __restrict__ qmu, const int8_t* __restrict__ qsg, long long Co, long long Ci, long long taps,
                                                      int8_t* __restrict__ mu_p, int8_t* __restrict__ sg_p) {
  const long long Ci16 = (Ci + 15) & ~15ll, n = Co * taps * Ci16;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long c = i % Ci16, rt = i / Ci16;
    const long long t = rt % taps, co = rt / taps;
    int8_t m = 0, sg = 0;
    if (c < Ci) {
      const long long src = (co * Ci + c) * taps + t;
      m = qmu[src];
      sg = qsg[src];
    }
    mu_p[i] = m;
    sg_p[i] = sg;
  }
}

// [x u8][blocked destination][draws on chip]
static const char* const kQ8Names[2][2][2] = {
    {{"q8_fwd<i8 32x32x32,64x128,eps injected>", "q8_fwd<i8 32x32x32,64x128,eps on chip>"},
     {"q8_fwd<i8 32x32x32,64x128,eps injected,out u8 blocked>", "q8_fwd<i8 32x32x32,64x128,eps on chip,out u8 blocked>"}},
    {{"q8_fwd<i8 32x32x32,64x128,eps injected,x u8 blocked>", "q8_fwd<i8 32x32x32,64x128,eps on chip,x u8 blocked>"},
     {"q8_fwd<i8 32x32x32,64x128,eps injected,x u8 blocked,out u8 blocked>", "q8_fwd<i8 32x32x32,64x128,eps on chip,x u8 blocked,out u8 blocked>"}}};

// act: the *_act entry points -- x_kind says what x is, out_q is the BLOCKED image and out is optional beside it.
static int q8_forward(const char* who, const bt_conv2d_geom& g, int S, const void* x, long long x_sample_stride, const bt_q8_params* p, const float* eps_w,
                      const float* eps_b, const bt_rng* rng, float* out, uint8_t* out_q, hipStream_t stream, bool act = false, int x_kind = BT_Q8_X_F32) {
  const Q8Fail fail = {who};
  if (act)
    if (int rc = q8_check_act(fail, x_kind, x, out, out_q)) return rc;
  if (int rc = q8_check_operands(fail, x, p, act && !out ? (const void*)out_q : (const void*)out, S, x_sample_stride, p ? p->mu_packed : nullptr,
                                 p ? p->sigma_packed : nullptr, g))
    return rc;
  if (act)
    if (int rc = q8_check_act_stride(fail, x_kind, x_sample_stride)) return rc;
  if (!eps_w && !rng) return fail(BT_ERR_BAD_ARG, "neither eps_w nor rng");
  if (eps_w && !eps_b && p->mu_b && p->sigma_b) return fail(BT_ERR_BAD_ARG, "eps_w without eps_b for a bias that has a sigma");
  const bt_q8_pair* pairs[5] = {&p->eps, &p->mul, &p->add, &p->in, &p->out};
  for (const bt_q8_pair* q : pairs)
    if (!(q->scale > 0.0)) return fail(BT_ERR_BAD_ARG, "a scale <= 0");
  if (!(p->s_mu > 0.0) || !(p->s_sigma > 0.0)) return fail(BT_ERR_BAD_ARG, "a scale <= 0");
  if (p->in.zero_point < 0 || p->in.zero_point > 255 || p->out.zero_point < 0 || p->out.zero_point > 255)
    return fail(BT_ERR_BAD_ARG, "an in / out zero point outside 0..255");
  if (g.groups != 1) return fail(BT_ERR_UNSUPPORTED, "groups != 1");
  if (p->eps.zero_point || p->mul.zero_point || p->add.zero_point) return fail(BT_ERR_UNSUPPORTED, "a nonzero eps / mul / add zero point");
  long long Ho, Wo, npix;
  if (int rc = q8_check_sizes(fail, g, S, Ho, Wo, npix)) return rc;

  Q8Args a = {};
  const float s_add = (float)p->add.scale, s_in = (float)p->in.scale, s_out = (float)p->out.scale;
  a.m_mul = (float)(p->s_sigma * p->eps.scale / p->mul.scale);
  a.s_mul = (float)p->mul.scale, a.s_mu = (float)p->s_mu;
  a.inv_add = 1.0f / s_add;
  const float atw = s_in * s_add;   // fbgemm's act_times_w_scale and output multiplier: fp32 operations on the fp32 scales
  if (!(atw > 0.f) || !(atw / s_out > 0.f)) return fail(BT_ERR_BAD_ARG, "in scale * add scale (/ out scale) underflows fp32");
  a.m_out = atw / s_out;
  a.inv_atw = 1.0f / atw;
  // With z_in == 128 a padding position is the MFMA's zero and no correction term reads the row sum.
  dim3 grid;
  if (int rc = q8_plan(fail, g, S, Ho, Wo, npix, {x, x_sample_stride, eps_w, eps_b, rng, out, out_q}, *p, p->in.zero_point == 128, a, grid)) return rc;
  return q8_launch_walk<Q8Reparam>(act && x_kind == BT_Q8_X_U8, act && out_q, !eps_w, kQ8Names, who, grid, stream, a);
}

}  // namespace bt

extern "C" int bt_q8_pack(const int8_t* q_mu, const int8_t* q_sigma, int64_t Co, int64_t Ci, int64_t taps, int8_t* mu_packed, int8_t* sigma_packed,
                          bt_stream_t stream) {
  using namespace bt;
  if (!q_mu || !q_sigma || !mu_packed || !sigma_packed || Co <= 0 || Ci <= 0 || taps <= 0) return set_error(BT_ERR_BAD_ARG, "bt_q8_pack: bad argument");
  const long long n = (long long)Co * taps * ((Ci + 15) & ~15ll);
  if (n >= (1ll << 40)) return set_error(BT_ERR_UNSUPPORTED, "bt_q8_pack: tensor too large");
  long long gx = (n + 255) / 256;
  if (gx > 4096) gx = 4096;
  return launch_kernel(q8_pack_kernel, nullptr, "bt_q8_pack", dim3((unsigned)gx), dim3(256), 0, 0, (hipStream_t)stream, q_mu, q_sigma, (long long)Co, (long long)Ci,
                       (long long)taps, mu_packed, sigma_packed);
}

extern "C" int bt_q8_conv2d_fwd(const bt_conv2d_geom* g, int32_t S, const float* x, int64_t x_sample_stride, const bt_q8_params* p, const float* eps_w,
                                const float* eps_b, const bt_rng* rng, float* out, uint8_t* out_q, bt_stream_t stream) {
  if (!g) return bt::set_error(BT_ERR_BAD_ARG, "bt_q8_conv2d_fwd: null geometry");
  return bt::q8_forward("bt_q8_conv2d_fwd", *g, S, x, x_sample_stride, p, eps_w, eps_b, rng, out, out_q, (hipStream_t)stream);
}

extern "C" int bt_q8_linear_fwd(int32_t B, int32_t In, int32_t Out, int32_t S, const float* x, int64_t x_sample_stride, const bt_q8_params* p,
                                const float* eps_w, const float* eps_b, const bt_rng* rng, float* out, uint8_t* out_q, bt_stream_t stream) {
  const bt_conv2d_geom g = {B, In, 1, 1, Out, 1, 1, 1, 1, 0, 0, 1, 1, 1};
  return bt::q8_forward("bt_q8_linear_fwd", g, S, x, x_sample_stride, p, eps_w, eps_b, rng, out, out_q, (hipStream_t)stream);
}

extern "C" int bt_q8_conv2d_fwd_act(const bt_conv2d_geom* g, int32_t S, const void* x, int32_t x_kind, int64_t x_sample_stride, const bt_q8_params* p,
                                    const float* eps_w, const float* eps_b, const bt_rng* rng, float* out, uint8_t* out_blocked, bt_stream_t stream) {
  if (!g) return bt::set_error(BT_ERR_BAD_ARG, "bt_q8_conv2d_fwd_act: null geometry");
  return bt::q8_forward("bt_q8_conv2d_fwd_act", *g, S, x, x_sample_stride, p, eps_w, eps_b, rng, out, out_blocked, (hipStream_t)stream, true, x_kind);
}

extern "C" int bt_q8_linear_fwd_act(int32_t B, int32_t In, int32_t Out, int32_t S, const void* x, int32_t x_kind, int64_t x_sample_stride, const bt_q8_params* p,
                                    const float* eps_w, const float* eps_b, const bt_rng* rng, float* out, uint8_t* out_blocked, bt_stream_t stream) {
  const bt_conv2d_geom g = {B, In, 1, 1, Out, 1, 1, 1, 1, 0, 0, 1, 1, 1};
  return bt::q8_forward("bt_q8_linear_fwd_act", g, S, x, x_sample_stride, p, eps_w, eps_b, rng, out, out_blocked, (hipStream_t)stream, true, x_kind);
}
