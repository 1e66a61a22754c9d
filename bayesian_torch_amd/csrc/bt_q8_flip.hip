// INT8 post-training-quantised Flipout layers (layers/_quantized.py: QuantizedConv2dFlipout, QuantizedLinearFlipout): one fused forward
// on v_mfma_i32_32x32x32_i8 that runs BOTH contractions of the Flipout estimator, MC-batched over S. Replaces the operator chain of
// reference layers/flipout_layers/quantized_conv_flipout.py:257-514 and quantized_linear_flipout.py:119-261 -- quantize_per_tensor of x,
// eps and the two sign tensors, two quantised convolutions, three quantized.mul and one quantized.add -- which exists on the CPU only.
// The arithmetic is include/bt_hip.h's (bt_q8_flip_params); integer accumulation has no order, so the output is that chain's bit for bit.
//
// The kernel is bt_q8_common.h's walk, q8_walk_kernel, over the Q8Flip chain below: TWO contractions over the same K, the mean path
// (0) and the perturbation path (1).
//   * weights: the q_mu word as it is (the mean path draws nothing) and d = qmul(q_sigma, e) from the tensor 0 draws;
//   * activation: xq - 128 and x' - 128, x' = umul(xq, sign) from the same xq. The sign of an element is hash_sign(tensor 2's key of the
//     sample, the element's offset in one sample's [B][Ci][H][W]) -- the float Flipout kernels' and bt_rng_sign_fill's -- so an element
//     read by nine taps gets one sign nine times, and samples that share x still differ;
//   * output: both requantisations (fbgemm's fma stage), the output sign (tensor 3, offset in [B][Co][Ho][Wo]), umul, uadd.
// Padding is a real zero in both contractions: the B tiles hold z_in - 128 and z_xp - 128 there and the corrections (128 - z_in) * sum
// q_mu and (128 - z_xp) * sum d take it out; with both zero points 128 the taps that read padding only are not walked.
#include "bt_q8_common.h"

namespace bt {

struct Q8FlipArgs : Q8Core {
  const float* sign_in;    // fp32 [S][B][Ci][H][W], < 0: -1, anything else +1 (null: tensor 2's stream)
  const float* sign_out;   // fp32 [S][B][Co][Ho][Wo] (null: tensor 3's stream)
  RngKey ksi, kso;
  long long x_elems;              // one sample's x
  float m_delta;                  // d = rne(float(q_sigma * e) * m_delta), m_delta = float(s_sigma * s_eps / s_delta)
  float m_xp;                     // x' = rne(float((xq - z_in) * (qsi - z_si)) * m_xp) + z_xp
  float inv_a1, m1, inv_a2, m2;   // the two requantisations: a = f32(s_act) * f32(s_w), m = a / f32(s_result)
  float m_ps;                     // p' = rne(float((p - z_pert) * (qso - z_so)) * m_ps) + z_ps
  float s_mean, nzs_mean, s_ps, nzs_ps, inv_out;   // uadd: fma(q, s, -(z * s)) of either operand, the sum times 1 / s_out
  int z_xp, z_mean, z_pert, z_ps;
  int dsi_pos, dsi_neg, dso_pos, dso_neg;   // the quantised signs less their zero points: q(+1) - z and q(-1) - z
};

struct Q8Flip {
  static constexpr int kC = 2;
  static constexpr bool kWords = false;   // every element has a sign of its own: bytes, with their offsets
  typedef Q8FlipArgs Args;
  const Args& a;
  uint32_t skey_in, skey_out;       // the sample's sign streams
  const float *sin_s, *sout_s;      // the sample's supplied signs, or null
  __device__ __forceinline__ Q8Flip(const Args& args, int s, uint32_t sample, uint32_t call_base) : a(args) {
    RngKey ksi = a.ksi, kso = a.kso;
    ksi.call += call_base, kso.call += call_base;
    skey_in = sign_stream_key(ksi, sample), skey_out = sign_stream_key(kso, sample);
    sin_s = a.sign_in ? a.sign_in + (long long)s * a.x_elems : nullptr;
    sout_s = a.sign_out ? a.sign_out + (long long)s * a.npix * a.Co : nullptr;
  }
  static __device__ __forceinline__ bool negative(const float* supplied, uint32_t key, long long i) {
    return supplied ? supplied[i] < 0.f : (__float_as_uint(hash_sign(key, (uint32_t)i)) >> 31) != 0u;
  }

  // mu_b on the mean path, sigma_b * eps_b on the perturbation path
  __device__ __forceinline__ void bias(float mu, bool has_sigma, float sigma, float eps, float (&b)[2]) const {
    b[0] = mu;
    b[1] = has_sigma ? __fmul_rn(sigma, eps) : 0.f;
  }
  __device__ __forceinline__ void weights(int qm, int qs, const float (&eps)[4], int (&w)[2], int (&sum)[2]) const {
    int word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = clamp_i8(rintf(__fmul_rn(eps[j], a.inv_eps)));
      const int d = clamp_i8(rintf(__fmul_rn((float)(sext8(qs, j) * e), a.m_delta)));   // (q_sigma is 0 beyond Ci: d is 0 there)
      sum[1] += d;
      sum[0] += sext8(qm, j);
      word |= (d & 0xFF) << (8 * j);
    }
    w[0] = qm, w[1] = word;
  }
  __device__ __forceinline__ void pads(int (&p)[2]) const { p[0] = (a.z_in - 128) & 0xFF, p[1] = (a.z_xp - 128) & 0xFF; }
  __device__ __forceinline__ void activation(int xq, long long off, int (&b)[2]) const {
    const int qp = q8_umul((xq - a.z_in) * (negative(sin_s, skey_in, off) ? a.dsi_neg : a.dsi_pos), a.m_xp, a.z_xp);
    b[0] = (xq - 128) & 0xFF;
    b[1] = (qp - 128) & 0xFF;
  }
  __device__ __forceinline__ void corrections(int (&zc)[2]) const { zc[0] = 128 - a.z_in, zc[1] = 128 - a.z_xp; }
  __device__ __forceinline__ float output(const int (&acc)[2], const float (&b)[2], long long off) const {
    // the two requantisations, fbgemm's: ONE rounding of b * (1 / a) + float(acc)
    const float o1 = q8_level(__fmul_rn(__fmaf_rn(b[0], a.inv_a1, (float)acc[0]), a.m1), a.z_mean);
    const int p = (int)q8_level(__fmul_rn(__fmaf_rn(b[1], a.inv_a2, (float)acc[1]), a.m2), a.z_pert);
    // the output sign and p' = umul(p, sign)
    const int ps = q8_umul((p - a.z_pert) * (negative(sout_s, skey_out, off) ? a.dso_neg : a.dso_pos), a.m_ps, a.z_ps);
    // uadd: either operand dequantised by ONE fused rounding of float(q) * s + (-(float(z) * s)), the fp32 sum, times 1 / s_out
    const float da = __fmaf_rn(o1, a.s_mean, a.nzs_mean);
    const float db = __fmaf_rn((float)ps, a.s_ps, a.nzs_ps);
    return q8_level(__fmul_rn(__fadd_rn(da, db), a.inv_out), a.z_out);
  }
};

// clamp(rne(v * (1 / s)) + z, 0, 255) of v = +1 or -1, less z: what quantize_per_tensor makes of a sign, on the host in fp32.
static int q8_sign_level(float v, float s, int z) {
  const float inv = 1.0f / s;
  float q = nearbyintf(v * inv) + (float)z;
  q = q < 0.f ? 0.f : (q > 255.f ? 255.f : q);
  return (int)q - z;
}

// [x u8][blocked destination][draws on chip]
static const char* const kQ8FlipNames[2][2][2] = {
    {{"q8_flip_fwd<i8 32x32x32,64x128,draws injected>", "q8_flip_fwd<i8 32x32x32,64x128,draws on chip>"},
     {"q8_flip_fwd<i8 32x32x32,64x128,draws injected,out u8 blocked>", "q8_flip_fwd<i8 32x32x32,64x128,draws on chip,out u8 blocked>"}},
    {{"q8_flip_fwd<i8 32x32x32,64x128,draws injected,x u8 blocked>", "q8_flip_fwd<i8 32x32x32,64x128,draws on chip,x u8 blocked>"},
     {"q8_flip_fwd<i8 32x32x32,64x128,draws injected,x u8 blocked,out u8 blocked>",
      "q8_flip_fwd<i8 32x32x32,64x128,draws on chip,x u8 blocked,out u8 blocked>"}}};

// act: the *_act entry points -- x_kind says what x is, out_q is the BLOCKED image and out is optional beside it.
static int q8_flip_forward(const char* who, const bt_conv2d_geom& g, int S, const void* x, long long x_sample_stride, const bt_q8_flip_params* p,
                           const float* eps_w, const float* eps_b, const float* sign_in, const float* sign_out, const bt_rng* rng, float* out, uint8_t* out_q,
                           hipStream_t stream, bool act = false, int x_kind = BT_Q8_X_F32) {
  const Q8Fail fail = {who};
  if (act)
    if (int rc = q8_check_act(fail, x_kind, x, out, out_q)) return rc;
  if (int rc = q8_check_operands(fail, x, p, act && !out ? (const void*)out_q : (const void*)out, S, x_sample_stride, p ? p->mu_packed : nullptr,
                                 p ? p->sigma_packed : nullptr, g))
    return rc;
  if (act)
    if (int rc = q8_check_act_stride(fail, x_kind, x_sample_stride)) return rc;
  if (!eps_w && !rng) return fail(BT_ERR_BAD_ARG, "neither eps_w nor rng");
  if (eps_w && (!sign_in || !sign_out)) return fail(BT_ERR_BAD_ARG, "eps_w without sign_in and sign_out: a supplied draw is whole or absent");
  if (!eps_w && (sign_in || sign_out)) return fail(BT_ERR_BAD_ARG, "a sign tensor without eps_w: a supplied draw is whole or absent");
  if (eps_w && !eps_b && p->mu_b && p->sigma_b) return fail(BT_ERR_BAD_ARG, "eps_w without eps_b for a bias that has a sigma");
  const bt_q8_pair* pairs[10] = {&p->eps, &p->delta, &p->in, &p->mean, &p->sign_in, &p->sign_out, &p->xp, &p->pert, &p->pert_signed, &p->out};
  for (const bt_q8_pair* q : pairs)
    if (!(q->scale > 0.0)) return fail(BT_ERR_BAD_ARG, "a scale <= 0");
  if (!(p->s_mu > 0.0) || !(p->s_sigma > 0.0)) return fail(BT_ERR_BAD_ARG, "a scale <= 0");
  for (int i = 2; i < 10; ++i)
    if (pairs[i]->zero_point < 0 || pairs[i]->zero_point > 255) return fail(BT_ERR_BAD_ARG, "a zero point outside 0..255 (in, mean, signs, xp, pert, pert_signed, out)");
  if (g.groups != 1) return fail(BT_ERR_UNSUPPORTED, "groups != 1");
  if (p->eps.zero_point || p->delta.zero_point) return fail(BT_ERR_UNSUPPORTED, "a nonzero eps / delta zero point");
  long long Ho, Wo, npix;
  if (int rc = q8_check_sizes(fail, g, S, Ho, Wo, npix)) return rc;
  const long long x_elems = (long long)g.B * g.Ci * g.H * g.W, out_elems = npix * g.Co;
  if (x_elems >= (1ll << 32) || out_elems >= (1ll << 32)) return fail(BT_ERR_UNSUPPORTED, "2^32 or more elements in one sample's x or output: the sign streams' index");

  Q8FlipArgs a = {};
  a.sign_in = sign_in, a.sign_out = sign_out, a.x_elems = x_elems;
  if (rng) a.ksi = make_key(*rng, 2), a.kso = make_key(*rng, 3);
  const float s_eps = (float)p->eps.scale, s_delta = (float)p->delta.scale, s_in = (float)p->in.scale, s_mean = (float)p->mean.scale;
  const float s_si = (float)p->sign_in.scale, s_so = (float)p->sign_out.scale, s_xp = (float)p->xp.scale, s_pert = (float)p->pert.scale;
  const float s_ps = (float)p->pert_signed.scale, s_out = (float)p->out.scale, s_mu = (float)p->s_mu;
  a.m_delta = (float)(p->s_sigma * p->eps.scale / p->delta.scale);   // quantized.mul of two qint8 tensors: the quotient in double, rounded once
  a.m_xp = s_in * s_si * (1.0f / s_xp);                              // quantized.mul of two quint8 tensors: fp32 operations, left to right
  a.m_ps = s_pert * s_so * (1.0f / s_ps);
  const float a1 = s_in * s_mu, a2 = s_xp * s_delta;                 // fbgemm's act_times_w_scale and output multiplier: fp32 operations
  a.m1 = a1 / s_mean, a.m2 = a2 / s_pert;
  for (float v : {a.m_delta, a.m_xp, a.m_ps, a1, a2, a.m1, a.m2, s_mean, s_ps, s_out, 1.0f / s_eps, 1.0f / s_in})
    if (!(v > 0.f) || !(v < INFINITY)) return fail(BT_ERR_BAD_ARG, "a product of scales underflows (or overflows) fp32");
  a.inv_a1 = 1.0f / a1, a.inv_a2 = 1.0f / a2;
  a.s_mean = s_mean, a.nzs_mean = -((float)p->mean.zero_point * s_mean);
  a.s_ps = s_ps, a.nzs_ps = -((float)p->pert_signed.zero_point * s_ps);
  a.inv_out = 1.0f / s_out;
  a.z_xp = p->xp.zero_point, a.z_mean = p->mean.zero_point, a.z_pert = p->pert.zero_point, a.z_ps = p->pert_signed.zero_point;
  a.dsi_pos = q8_sign_level(1.f, s_si, p->sign_in.zero_point), a.dsi_neg = q8_sign_level(-1.f, s_si, p->sign_in.zero_point);
  a.dso_pos = q8_sign_level(1.f, s_so, p->sign_out.zero_point), a.dso_neg = q8_sign_level(-1.f, s_so, p->sign_out.zero_point);
  // Only where BOTH activations' zero points are 128 is a padding position the MFMA's zero in both B tiles.
  dim3 grid;
  if (int rc = q8_plan(fail, g, S, Ho, Wo, npix, {x, x_sample_stride, eps_w, eps_b, rng, out, out_q}, *p, p->in.zero_point == 128 && p->xp.zero_point == 128, a, grid))
    return rc;
  return q8_launch_walk<Q8Flip>(act && x_kind == BT_Q8_X_U8, act && out_q, !eps_w, kQ8FlipNames, who, grid, stream, a);
}

}  // namespace bt

extern "C" int bt_q8_flip_conv2d_fwd(const bt_conv2d_geom* g, int32_t S, const float* x, int64_t x_sample_stride, const bt_q8_flip_params* p, const float* eps_w,
                                     const float* eps_b, const float* sign_in, const float* sign_out, const bt_rng* rng, float* out, uint8_t* out_q,
                                     bt_stream_t stream) {
  if (!g) return bt::set_error(BT_ERR_BAD_ARG, "bt_q8_flip_conv2d_fwd: null geometry");
  return bt::q8_flip_forward("bt_q8_flip_conv2d_fwd", *g, S, x, x_sample_stride, p, eps_w, eps_b, sign_in, sign_out, rng, out, out_q, (hipStream_t)stream);
}

extern "C" int bt_q8_flip_linear_fwd(int32_t B, int32_t In, int32_t Out, int32_t S, const float* x, int64_t x_sample_stride, const bt_q8_flip_params* p,
                                     const float* eps_w, const float* eps_b, const float* sign_in, const float* sign_out, const bt_rng* rng, float* out,
                                     uint8_t* out_q, bt_stream_t stream) {
  const bt_conv2d_geom g = {B, In, 1, 1, Out, 1, 1, 1, 1, 0, 0, 1, 1, 1};
  return bt::q8_flip_forward("bt_q8_flip_linear_fwd", g, S, x, x_sample_stride, p, eps_w, eps_b, sign_in, sign_out, rng, out, out_q, (hipStream_t)stream);
}

extern "C" int bt_q8_flip_conv2d_fwd_act(const bt_conv2d_geom* g, int32_t S, const void* x, int32_t x_kind, int64_t x_sample_stride, const bt_q8_flip_params* p,
                                         const float* eps_w, const float* eps_b, const float* sign_in, const float* sign_out, const bt_rng* rng, float* out,
                                         uint8_t* out_blocked, bt_stream_t stream) {
  if (!g) return bt::set_error(BT_ERR_BAD_ARG, "bt_q8_flip_conv2d_fwd_act: null geometry");
  return bt::q8_flip_forward("bt_q8_flip_conv2d_fwd_act", *g, S, x, x_sample_stride, p, eps_w, eps_b, sign_in, sign_out, rng, out, out_blocked, (hipStream_t)stream,
                             true, x_kind);
}

extern "C" int bt_q8_flip_linear_fwd_act(int32_t B, int32_t In, int32_t Out, int32_t S, const void* x, int32_t x_kind, int64_t x_sample_stride,
                                         const bt_q8_flip_params* p, const float* eps_w, const float* eps_b, const float* sign_in, const float* sign_out,
                                         const bt_rng* rng, float* out, uint8_t* out_blocked, bt_stream_t stream) {
  const bt_conv2d_geom g = {B, In, 1, 1, Out, 1, 1, 1, 1, 0, 0, 1, 1, 1};
  return bt::q8_flip_forward("bt_q8_flip_linear_fwd_act", g, S, x, x_sample_stride, p, eps_w, eps_b, sign_in, sign_out, rng, out, out_blocked, (hipStream_t)stream,
                             true, x_kind);
}
