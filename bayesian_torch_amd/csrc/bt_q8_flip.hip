// INT8 post-training-quantised Flipout layers (layers/_quantized.py: QuantizedConv2dFlipout, QuantizedLinearFlipout): one fused forward
// on v_mfma_i32_32x32x32_i8 that runs BOTH contractions of the Flipout estimator, MC-batched over S. Replaces the operator chain of
// reference layers/flipout_layers/quantized_conv_flipout.py:257-514 and quantized_linear_flipout.py:119-261 -- quantize_per_tensor of x,
// eps and the two sign tensors, two quantised convolutions, three quantized.mul and one quantized.add -- which exists on the CPU only.
// The arithmetic is include/bt_hip.h's (bt_q8_flip_params); integer accumulation has no order, so the output is that chain's bit for bit.
//
// The geometry is q8_fwd_kernel's (bt_q8.hip): a workgroup (256 threads, 4 waves as 2 x 2) owns 64 output channels x 128 output pixels
// of one sample and walks K in stages of four 16-channel units, operands fetched one stage ahead, the same [Co][taps][Ci16] packs and
// the same LDS operand layout. Per stage there are two A tiles and two B tiles, and every wave keeps two accumulator sets:
//   * producers, weight side: thread (row, unit) copies its 16 bytes of q_mu (the mean path draws nothing) and forms the 16 bytes of
//     d = qmul(q_sigma, e) from the tensor 0 draws (Philox, or the injected eps); it keeps a row sum for either tile;
//   * producers, x side: thread (pixel, two units) quantises the fetched fp32 x to xq and forms x' = umul(xq, sign) in registers from
//     the same value; xq - 128 and x' - 128 go to the two B tiles. The sign of an element is hash_sign(tensor 2's key of the sample,
//     the element's offset in one sample's [B][Ci][H][W]) -- the float Flipout kernels' and bt_rng_sign_fill's -- so an element read by
//     nine taps gets one sign nine times, and samples that share x still differ;
//   * consumers: 2 K-chunks x 2 pixel blocks x 2 contractions of 32x32x32 MFMAs per wave and stage.
// The output stage runs per element in registers: both requantisations (fbgemm's fma stage), the output sign (tensor 3, offset in
// [B][Co][Ho][Wo]), umul, uadd, the fp32 store and the u8 store when asked. Padding is a real zero in both contractions: the B tiles
// hold z_in - 128 and z_xp - 128 there and the corrections (128 - z_in) * sum q_mu and (128 - z_xp) * sum d take it out; with both zero
// points 128 the taps that read padding only are not walked.
#include "bt_q8_common.h"

namespace bt {

struct Q8FlipArgs {
  const float* x;
  long long x_sample_stride;
  const int8_t* qmu;
  const int8_t* qsg;
  const float* eps_w;
  const float* eps_b;
  const float* sign_in;    // fp32 [S][B][Ci][H][W], < 0: -1, anything else +1 (null: tensor 2's stream)
  const float* sign_out;   // fp32 [S][B][Co][Ho][Wo] (null: tensor 3's stream)
  const float* mu_b;
  const float* sigma_b;
  float* out;
  uint8_t* out_q;
  const uint32_t* call_base;
  RngKey kw, kb, ksi, kso;
  uint32_t sample0;
  int B, Ci, H, W, Co, KH, KW, sh, sw, ph, pw, dh, dw, Ho, Wo;
  int CB, U, taps, VU, pruned;
  uint64_t live_taps;
  long long npix;
  long long x_elems, out_elems;   // one sample's x and output
  float inv_eps, m_delta;         // e = rne(eps * inv_eps); d = rne(float(q_sigma * e) * m_delta), m_delta = float(s_sigma * s_eps / s_delta)
  float inv_in, m_xp;             // xq; x' = rne(float((xq - z_in) * (qsi - z_si)) * m_xp) + z_xp
  float inv_a1, m1, inv_a2, m2;   // the two requantisations: a = f32(s_act) * f32(s_w), m = a / f32(s_result)
  float m_ps;                     // p' = rne(float((p - z_pert) * (qso - z_so)) * m_ps) + z_ps
  float s_mean, nzs_mean, s_ps, nzs_ps, inv_out, s_out;   // uadd: fma(q, s, -(z * s)) of either operand, the sum times 1 / s_out
  int z_in, z_xp, z_mean, z_pert, z_ps, z_out;
  int dsi_pos, dsi_neg, dso_pos, dso_neg;   // the quantised signs less their zero points: q(+1) - z and q(-1) - z
};

// clamp(rne(float(prod) * m) + z, 0, 255): quantized.mul of two quint8 values whose zero-point-free product is prod.
__device__ __forceinline__ int q8_umul(int prod, float m, int z) {
  return (int)fminf(fmaxf(__fadd_rn(rintf(__fmul_rn((float)prod, m)), (float)z), 0.f), 255.f);
}

__global__ __launch_bounds__(kQ8Threads) void q8_flip_fwd_kernel(Q8FlipArgs a) {
  __shared__ v4i lds_am[kQ8SU * kQ8TM];   // q_mu, 4 KiB
  __shared__ v4i lds_ad[kQ8SU * kQ8TM];   // d, 4 KiB
  __shared__ v4i lds_bx[kQ8SU * kQ8TN];   // xq - 128, 8 KiB
  __shared__ v4i lds_bp[kQ8SU * kQ8TN];   // x' - 128, 8 KiB
  __shared__ int row_sum_m[kQ8TM], row_sum_d[kQ8TM];
  __shared__ float bias_m[kQ8TM], bias_p[kQ8TM];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int s = blockIdx.z;
  const int co0 = blockIdx.y * kQ8TM;
  const long long n0 = (long long)blockIdx.x * kQ8TN;
  RngKey kw = a.kw, kb = a.kb, ksi = a.ksi, kso = a.kso;
  if (a.call_base) {
    const uint32_t cb = *a.call_base;
    kw.call += cb, kb.call += cb, ksi.call += cb, kso.call += cb;
  }
  const uint32_t sample = a.sample0 + (uint32_t)s;
  const uint32_t skey_in = sign_stream_key(ksi, sample), skey_out = sign_stream_key(kso, sample);

  // the two bias terms of this sample's channels: mu_b on the mean path, sigma_b * eps_b on the perturbation path (0 without one)
  if (tid < kQ8TM) {
    const int co = co0 + tid;
    float bm = 0.f, bp = 0.f;
    if (a.mu_b && co < a.Co) {
      bm = a.mu_b[co];
      if (a.sigma_b) {
        float eb;
        if (a.eps_b) {
          eb = a.eps_b[(long long)s * a.Co + co];
        } else {
          float z[4];
          philox_normal4(kb, sample, (uint32_t)(co >> 2), z);
          eb = z[co & 3];
        }
        bp = __fmul_rn(a.sigma_b[co], eb);
      }
    }
    bias_m[tid] = bm, bias_p[tid] = bp;
  }

  // weight side: this thread's (row, unit of the stage)
  const int a_row = tid >> 2, a_ul = tid & 3;
  const int a_co = co0 + a_row;
  const bool a_live = a_co < a.Co;
  const long long inner4 = ((long long)a.Ci + 3) & ~3ll;
  int msum = 0, dsum = 0;

  // x side: this thread's pixel and its two units of the stage
  const int b_pl = tid & (kQ8TN - 1), b_u2 = (tid >> 7) * 2;
  const long long b_n = n0 + b_pl;
  const bool b_live = b_n < a.npix;
  int ih0 = 0, iw0 = 0;
  const float* xb = a.x + (long long)s * a.x_sample_stride;
  long long xoff0 = 0;   // the offset of this pixel's image in one sample's x: the sign stream's index base
  if (b_live) {
    const long long hw = (long long)a.Ho * a.Wo;
    const long long bi = b_n / hw;
    const int r = (int)(b_n - bi * hw);
    const int oh = r / a.Wo, ow = r - oh * a.Wo;
    ih0 = oh * a.sh - a.ph;
    iw0 = ow * a.sw - a.pw;
    xoff0 = bi * (long long)a.Ci * a.H * a.W;
    xb += xoff0;
  }
  const long long plane = (long long)a.H * a.W;
  const int pad_x = (a.z_in - 128) & 0xFF, pad_p = (a.z_xp - 128) & 0xFF;
  const float* sin_s = a.sign_in ? a.sign_in + (long long)s * a.x_elems : nullptr;

  v16i am0, am1, ap0, ap1;
#pragma unroll
  for (int i = 0; i < 16; ++i) am0[i] = 0, am1[i] = 0, ap0[i] = 0, ap1[i] = 0;
  const int wm = wv & 1, wn = wv >> 1;

  // The global operands of a stage are fetched one stage ahead, into registers (as in q8_fwd_kernel).
  v4i pqm = {0, 0, 0, 0}, pqs = {0, 0, 0, 0};
  float px[2][16];
  auto prefetch = [&](int u0) {
    const int va = u0 + a_ul;
    if (a_live && va < a.VU) {
      int t, cb;
      q8_unit(a, va, t, cb);
      const long long off = ((long long)a_co * a.U + t * a.CB + cb) * 16;
      pqm = *reinterpret_cast<const v4i*>(a.qmu + off);
      pqs = *reinterpret_cast<const v4i*>(a.qsg + off);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int v = u0 + b_u2 + k;
      bool inside = false;
      int c0 = 0;
      const float* xp = xb;
      if (b_live && v < a.VU) {
        int t, cb;
        q8_unit(a, v, t, cb);
        const int ky = t / a.KW, kx = t - ky * a.KW;
        const int ih = ih0 + ky * a.dh, iw = iw0 + kx * a.dw;
        inside = ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
        c0 = cb * 16;
        if (inside) xp = xb + (long long)c0 * plane + (long long)ih * a.W + iw;
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) px[k][j] = (inside && c0 + j < a.Ci) ? xp[(long long)j * plane] : 0.f;
    }
  };
  prefetch(0);

  for (int u0 = 0; u0 < a.VU; u0 += kQ8SU) {
    // ---- weight producer: the q_mu bytes as they are, d from q_sigma and the draws
    {
      const int v = u0 + a_ul;
      v4i mq = {0, 0, 0, 0}, dq = {0, 0, 0, 0};
      if (a_live && v < a.VU) {
        int t, cb;
        q8_unit(a, v, t, cb);
        const v4i qs = pqs;
        mq = pqm;
        const int c0 = cb * 16;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = c0 + 4 * q;
          float eps[4] = {0.f, 0.f, 0.f, 0.f};
          if (c < a.Ci) {
            if (a.eps_w) {
              const float* ep = a.eps_w + (((long long)s * a.Co + a_co) * a.Ci + c) * a.taps + t;
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (c + j < a.Ci) eps[j] = ep[(long long)j * a.taps];
            } else {
              const long long e0 = ((long long)a_co * a.taps + t) * inner4 + c;
              philox_normal4(kw, sample, (uint32_t)(e0 >> 2), eps);
            }
          }
          int word = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int e = clamp_i8(rintf(__fmul_rn(eps[j], a.inv_eps)));
            const int d = clamp_i8(rintf(__fmul_rn((float)(sext8(qs[q], j) * e), a.m_delta)));   // (q_sigma is 0 beyond Ci: d is 0 there)
            dsum += d;
            msum += sext8(mq[q], j);
            word |= (d & 0xFF) << (8 * j);
          }
          dq[q] = word;
        }
      }
      lds_am[a_ul * kQ8TM + a_row] = mq;
      lds_ad[a_ul * kQ8TM + a_row] = dq;
    }
    // ---- x producer: xq and x' = umul(xq, sign) from the same fetched value
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int ul = b_u2 + k, v = u0 + ul;
      v4i xq = {0, 0, 0, 0}, xs = {0, 0, 0, 0};
      if (b_live && v < a.VU) {
        int t, cb;
        q8_unit(a, v, t, cb);
        const int ky = t / a.KW, kx = t - ky * a.KW;
        const int ih = ih0 + ky * a.dh, iw = iw0 + kx * a.dw;
        const bool inside = ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
        const int c0 = cb * 16;
        const long long e0 = xoff0 + (long long)c0 * plane + (long long)ih * a.W + iw;   // (read only where inside)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          int wx = 0, wp = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = c0 + 4 * q + j;
            int bx = pad_x, bp = pad_p;
            if (c >= a.Ci) {
              bx = 0, bp = 0;
            } else if (inside) {
              const float xv = px[k][4 * q + j];
              const int qx = (int)fminf(fmaxf(__fadd_rn(rintf(__fmul_rn(xv, a.inv_in)), (float)a.z_in), 0.f), 255.f);
              const long long ei = e0 + (long long)(4 * q + j) * plane;
              const bool neg = sin_s ? sin_s[ei] < 0.f : (__float_as_uint(hash_sign(skey_in, (uint32_t)ei)) >> 31) != 0u;
              const int qp = q8_umul((qx - a.z_in) * (neg ? a.dsi_neg : a.dsi_pos), a.m_xp, a.z_xp);
              bx = (qx - 128) & 0xFF;
              bp = (qp - 128) & 0xFF;
            }
            wx |= bx << (8 * j);
            wp |= bp << (8 * j);
          }
          xq[q] = wx;
          xs[q] = wp;
        }
      }
      lds_bx[ul * kQ8TN + b_pl] = xq;
      lds_bp[ul * kQ8TN + b_pl] = xs;
    }
    __syncthreads();
    if (u0 + kQ8SU < a.VU) prefetch(u0 + kQ8SU);
    // ---- consumers: the mean contraction and the perturbation contraction
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const int ul = 2 * ch + (lane >> 5);
      const int ar = ul * kQ8TM + 32 * wm + (lane & 31), br = ul * kQ8TN + 64 * wn + (lane & 31);
      const v4i avm = lds_am[ar], avd = lds_ad[ar];
      const v4i x0 = lds_bx[br], x1 = lds_bx[br + 32];
      const v4i p0 = lds_bp[br], p1 = lds_bp[br + 32];
      am0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(avm, x0, am0, 0, 0, 0);
      am1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(avm, x1, am1, 0, 0, 0);
      ap0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(avd, p0, ap0, 0, 0, 0);
      ap1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(avd, p1, ap1, 0, 0, 0);
    }
    __syncthreads();   // the stage has been consumed
  }

  // the row sums: a row's four producer threads are four adjacent lanes
  msum += __shfl_xor(msum, 1, 64);
  msum += __shfl_xor(msum, 2, 64);
  dsum += __shfl_xor(dsum, 1, 64);
  dsum += __shfl_xor(dsum, 2, 64);
  if (a_ul == 0) row_sum_m[a_row] = msum, row_sum_d[a_row] = dsum;
  __syncthreads();

  const long long hw = (long long)a.Ho * a.Wo;
  const int zcm = 128 - a.z_in, zcp = 128 - a.z_xp;
  const float* sout_s = a.sign_out ? a.sign_out + (long long)s * a.out_elems : nullptr;
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    const long long n = n0 + 64 * wn + 32 * blk + (lane & 31);
    if (n >= a.npix) continue;
    const long long bi = n / hw;
    const long long obase = bi * a.Co * hw + (n - bi * hw);   // in one sample's [B][Co][Ho][Wo]
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 32 * wm + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
      const int co = co0 + row;
      if (co >= a.Co) continue;
      const long long oi = obase + (long long)co * hw;
      const int acc_m = (blk ? am1[i] : am0[i]) + zcm * row_sum_m[row];
      const int acc_p = (blk ? ap1[i] : ap0[i]) + zcp * row_sum_d[row];
      // the two requantisations, fbgemm's: ONE rounding of b * (1 / a) + float(acc)
      const float tm = __fmul_rn(__fmaf_rn(bias_m[row], a.inv_a1, (float)acc_m), a.m1);
      const float o1 = fminf(fmaxf(__fadd_rn(rintf(tm), (float)a.z_mean), 0.f), 255.f);
      const float tp = __fmul_rn(__fmaf_rn(bias_p[row], a.inv_a2, (float)acc_p), a.m2);
      const int p = (int)fminf(fmaxf(__fadd_rn(rintf(tp), (float)a.z_pert), 0.f), 255.f);
      // the output sign and p' = umul(p, sign)
      const bool neg = sout_s ? sout_s[oi] < 0.f : (__float_as_uint(hash_sign(skey_out, (uint32_t)oi)) >> 31) != 0u;
      const int ps = q8_umul((p - a.z_pert) * (neg ? a.dso_neg : a.dso_pos), a.m_ps, a.z_ps);
      // uadd: either operand dequantised by ONE fused rounding of float(q) * s + (-(float(z) * s)), the fp32 sum, times 1 / s_out
      const float da = __fmaf_rn(o1, a.s_mean, a.nzs_mean);
      const float db = __fmaf_rn((float)ps, a.s_ps, a.nzs_ps);
      const float t = __fmul_rn(__fadd_rn(da, db), a.inv_out);
      const float oq = fminf(fmaxf(__fadd_rn(rintf(t), (float)a.z_out), 0.f), 255.f);
      const long long o = (long long)s * a.out_elems + oi;
      a.out[o] = __fmul_rn(__fsub_rn(oq, (float)a.z_out), a.s_out);
      if (a.out_q) a.out_q[o] = (uint8_t)oq;
    }
  }
}

// clamp(rne(v * (1 / s)) + z, 0, 255) of v = +1 or -1, less z: what quantize_per_tensor makes of a sign, on the host in fp32.
static int q8_sign_level(float v, float s, int z) {
  const float inv = 1.0f / s;
  float q = nearbyintf(v * inv) + (float)z;
  q = q < 0.f ? 0.f : (q > 255.f ? 255.f : q);
  return (int)q - z;
}

static int q8_flip_forward(const char* who, const bt_conv2d_geom& g, int S, const float* x, long long x_sample_stride, const bt_q8_flip_params* p,
                           const float* eps_w, const float* eps_b, const float* sign_in, const float* sign_out, const bt_rng* rng, float* out, uint8_t* out_q,
                           hipStream_t stream) {
  const Q8Fail fail = {who};
  if (int rc = q8_check_operands(fail, x, p, out, S, x_sample_stride, p ? p->mu_packed : nullptr, p ? p->sigma_packed : nullptr, g)) return rc;
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
  const long long taps = (long long)g.kh * g.kw, Ci16 = ((long long)g.Ci + 15) & ~15ll;
  const long long x_elems = (long long)g.B * g.Ci * g.H * g.W, out_elems = npix * g.Co;
  if (x_elems >= (1ll << 32) || out_elems >= (1ll << 32)) return fail(BT_ERR_UNSUPPORTED, "2^32 or more elements in one sample's x or output: the sign streams' index");

  Q8FlipArgs a = {};
  a.x = x, a.x_sample_stride = x_sample_stride, a.qmu = p->mu_packed, a.qsg = p->sigma_packed, a.eps_w = eps_w, a.eps_b = eps_b;
  a.sign_in = sign_in, a.sign_out = sign_out;
  a.mu_b = p->mu_b, a.sigma_b = p->mu_b ? p->sigma_b : nullptr, a.out = out, a.out_q = out_q;
  bt_rng none = {};
  const bt_rng& R = rng ? *rng : none;
  a.call_base = R.call_base_dev, a.kw = make_key(R, 0), a.kb = make_key(R, 1), a.ksi = make_key(R, 2), a.kso = make_key(R, 3), a.sample0 = R.sample0;
  a.B = g.B, a.Ci = g.Ci, a.H = g.H, a.W = g.W, a.Co = g.Co, a.KH = g.kh, a.KW = g.kw, a.sh = g.sh, a.sw = g.sw, a.ph = g.ph, a.pw = g.pw, a.dh = g.dh, a.dw = g.dw;
  a.Ho = (int)Ho, a.Wo = (int)Wo, a.CB = (int)(Ci16 / 16), a.taps = (int)taps, a.U = (int)(taps * (Ci16 / 16)), a.npix = npix;
  a.x_elems = x_elems, a.out_elems = out_elems;
  // Only where BOTH activations' zero points are 128 is a padding position the MFMA's zero in both B tiles (q8_live_taps).
  a.VU = a.U;
  if (p->in.zero_point == 128 && p->xp.zero_point == 128 && q8_live_taps(g, Ho, Wo, a.CB, a.live_taps, a.VU)) a.pruned = 1;

  const float s_eps = (float)p->eps.scale, s_delta = (float)p->delta.scale, s_in = (float)p->in.scale, s_mean = (float)p->mean.scale;
  const float s_si = (float)p->sign_in.scale, s_so = (float)p->sign_out.scale, s_xp = (float)p->xp.scale, s_pert = (float)p->pert.scale;
  const float s_ps = (float)p->pert_signed.scale, s_out = (float)p->out.scale, s_mu = (float)p->s_mu;
  a.inv_eps = 1.0f / s_eps;
  a.m_delta = (float)(p->s_sigma * p->eps.scale / p->delta.scale);   // quantized.mul of two qint8 tensors: the quotient in double, rounded once
  a.inv_in = 1.0f / s_in;
  a.m_xp = s_in * s_si * (1.0f / s_xp);                              // quantized.mul of two quint8 tensors: fp32 operations, left to right
  a.m_ps = s_pert * s_so * (1.0f / s_ps);
  const float a1 = s_in * s_mu, a2 = s_xp * s_delta;                 // fbgemm's act_times_w_scale and output multiplier: fp32 operations
  a.m1 = a1 / s_mean, a.m2 = a2 / s_pert;
  for (float v : {a.m_delta, a.m_xp, a.m_ps, a1, a2, a.m1, a.m2, s_mean, s_ps, s_out, a.inv_eps, a.inv_in})
    if (!(v > 0.f) || !(v < INFINITY)) return fail(BT_ERR_BAD_ARG, "a product of scales underflows (or overflows) fp32");
  a.inv_a1 = 1.0f / a1, a.inv_a2 = 1.0f / a2;
  a.s_mean = s_mean, a.nzs_mean = -((float)p->mean.zero_point * s_mean);
  a.s_ps = s_ps, a.nzs_ps = -((float)p->pert_signed.zero_point * s_ps);
  a.inv_out = 1.0f / s_out, a.s_out = s_out;
  a.z_in = p->in.zero_point, a.z_xp = p->xp.zero_point, a.z_mean = p->mean.zero_point, a.z_pert = p->pert.zero_point;
  a.z_ps = p->pert_signed.zero_point, a.z_out = p->out.zero_point;
  a.dsi_pos = q8_sign_level(1.f, s_si, p->sign_in.zero_point), a.dsi_neg = q8_sign_level(-1.f, s_si, p->sign_in.zero_point);
  a.dso_pos = q8_sign_level(1.f, s_so, p->sign_out.zero_point), a.dso_neg = q8_sign_level(-1.f, s_so, p->sign_out.zero_point);
  const dim3 grid((unsigned)((npix + kQ8TN - 1) / kQ8TN), (unsigned)((g.Co + kQ8TM - 1) / kQ8TM), (unsigned)S);
  if (grid.y > 65535u) return fail(BT_ERR_UNSUPPORTED, "more than 65535 * 64 output channels");
  return launch_kernel(q8_flip_fwd_kernel, eps_w ? "q8_flip_fwd<i8 32x32x32,64x128,draws injected>" : "q8_flip_fwd<i8 32x32x32,64x128,draws on chip>", who, grid,
                       dim3(kQ8Threads), 0, 0, stream, a);
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
