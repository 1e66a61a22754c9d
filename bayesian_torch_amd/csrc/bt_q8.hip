// INT8 post-training-quantised Reparameterization layers (layers/_quantized.py): one fused forward on v_mfma_i32_32x32x32_i8 for
// Conv2d and Linear (the 1 x 1 map), MC-batched over S. Replaces, in reference layers/variational_layers/quantize_conv_variational.py
// :495-547 and quantize_linear_variational.py:173-219, quantize_per_tensor(eps), quantized.mul, quantized.add, quantize_per_tensor(x)
// and the quantised conv2d / linear -- which exist on the CPU only. The arithmetic is include/bt_hip.h's (bt_q8_params): integer
// accumulation has no order, so the output is the reference's bit for bit.
//
// A workgroup (256 threads, 4 waves as 2 x 2) owns a tile of 64 output channels x 128 output pixels of one sample and walks K in
// stages of four units; a unit is the 16 (padded) input channels of one tap, 16 bytes of either operand:
//   * producers, weight side: thread (row, unit) reads its 16 bytes of q_mu and q_sigma from the [Co][taps][Ci16] packs, takes the
//     unit's 16 draws (Philox blocks of the tensor 0 stream, or the injected fp32 eps), runs e -> p -> w and writes the 16 int8 weights
//     to LDS in the MFMA's operand layout; it also sums them (the zero-point correction needs sum_k w over ALL K positions);
//   * producers, x side: thread (pixel, two units) fetches the fp32 NCHW values, quantises them to xq - 128 (padding: z_in - 128, so
//     that the correction (128 - z_in) * sum_k w makes padding a real zero) and writes them to LDS likewise;
//   * consumers: every wave runs 2 K-chunks x 2 pixel blocks of 32x32x32 MFMAs on its 32 x 64 quarter.
// The global operands of a stage are fetched one stage ahead into registers; with z_in == 128 the taps that read padding for every
// output pixel are not walked (DESIGN.md section 4.6f has the measurements).
// Operand layout in LDS: [unit][row or pixel][16 bytes]; lane l of a wave reads the 16 bytes of row l & 31 in unit 2 * chunk + (l >> 5)
// for A and B alike -- the contraction only needs A and B to agree on which k a (lane half, byte) pair means, and they are written
// by the same rule. C/D: column (pixel) l & 31, row (channel) (reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5).
#include "bt_q8_common.h"

namespace bt {

struct Q8Args {
  const float* x;
  long long x_sample_stride;
  const int8_t* qmu;
  const int8_t* qsg;
  const float* eps_w;
  const float* eps_b;
  const float* mu_b;
  const float* sigma_b;
  float* out;
  uint8_t* out_q;
  const uint32_t* call_base;
  RngKey kw, kb;
  uint32_t sample0;
  int B, Ci, H, W, Co, KH, KW, sh, sw, ph, pw, dh, dw, Ho, Wo;
  int CB;     // 16-channel blocks per tap (Ci16 / 16)
  int U;      // units: taps * CB
  int taps;
  int VU;     // units walked: live taps * CB (== U unless taps are pruned)
  int pruned;           // z_in == 128 and some tap reads padding for every output pixel: such a tap contributes 0 and is skipped
  uint64_t live_taps;   // pruned: the live taps in ascending order, four bits each (taps <= 16)
  long long npix;   // B * Ho * Wo
  float inv_eps, m_mul, s_mul, s_mu, inv_add, inv_in, m_out, inv_atw, s_out;   // inv_atw: 1 / (s_in * s_add); m_out: s_in * s_add / s_out -- fp32 operations
  int z_in, z_out;
};

// e -> p -> w of one weight (include/bt_hip.h): one fp32 rounding per operation.
__device__ __forceinline__ int q8_weight(int qm, int qs, float eps, const Q8Args& a) {
  const int e = clamp_i8(rintf(__fmul_rn(eps, a.inv_eps)));
  const int p = clamp_i8(rintf(__fmul_rn((float)(qs * e), a.m_mul)));
  const float t = __fadd_rn(__fmul_rn((float)p, a.s_mul), __fmul_rn((float)qm, a.s_mu));
  return clamp_i8(rintf(__fmul_rn(t, a.inv_add)));
}

__global__ __launch_bounds__(kQ8Threads) void q8_fwd_kernel(Q8Args a) {
  __shared__ v4i lds_a[kQ8SU * kQ8TM];   // 4 KiB
  __shared__ v4i lds_b[kQ8SU * kQ8TN];   // 8 KiB
  __shared__ int row_sum[kQ8TM];
  __shared__ float bias_term[kQ8TM];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int s = blockIdx.z;
  const int co0 = blockIdx.y * kQ8TM;
  const long long n0 = (long long)blockIdx.x * kQ8TN;
  RngKey kw = a.kw, kb = a.kb;
  if (a.call_base) {
    const uint32_t cb = *a.call_base;
    kw.call += cb;
    kb.call += cb;
  }
  const uint32_t sample = a.sample0 + (uint32_t)s;

  // the bias of this sample's channels, b = mu_b + sigma_b * eps_b (0 without one): the output stage takes it into the accumulator's scale
  if (tid < kQ8TM) {
    const int co = co0 + tid;
    float bt = 0.f;
    if (a.mu_b && co < a.Co) {
      float b = a.mu_b[co];
      if (a.sigma_b) {
        float eb;
        if (a.eps_b) {
          eb = a.eps_b[(long long)s * a.Co + co];
        } else {
          float z[4];
          philox_normal4(kb, sample, (uint32_t)(co >> 2), z);
          eb = z[co & 3];
        }
        b = __fadd_rn(b, __fmul_rn(a.sigma_b[co], eb));
      }
      bt = b;
    }
    bias_term[tid] = bt;
  }

  // weight side: this thread's (row, unit of the stage)
  const int a_row = tid >> 2, a_ul = tid & 3;
  const int a_co = co0 + a_row;
  const bool a_live = a_co < a.Co;
  const long long inner4 = ((long long)a.Ci + 3) & ~3ll;
  int wsum = 0;

  // x side: this thread's pixel and its two units of the stage
  const int b_pl = tid & (kQ8TN - 1), b_u2 = (tid >> 7) * 2;
  const long long b_n = n0 + b_pl;
  const bool b_live = b_n < a.npix;
  int ih0 = 0, iw0 = 0;
  const float* xb = a.x + (long long)s * a.x_sample_stride;
  if (b_live) {
    const long long hw = (long long)a.Ho * a.Wo;
    const long long bi = b_n / hw;
    const int r = (int)(b_n - bi * hw);
    const int oh = r / a.Wo, ow = r - oh * a.Wo;
    ih0 = oh * a.sh - a.ph;
    iw0 = ow * a.sw - a.pw;
    xb += bi * (long long)a.Ci * a.H * a.W;
  }
  const long long plane = (long long)a.H * a.W;
  const int pad_byte = (a.z_in - 128) & 0xFF;

  v16i acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc0[i] = 0, acc1[i] = 0;
  const int wm = wv & 1, wn = wv >> 1;

  // The global operands of a stage are fetched one stage ahead, into registers: this thread's 16 bytes of either pack and its 2 x 16
  // fp32 values of x (0 where nothing is read). The loads are issued behind the barrier that publishes the current stage and are in
  // flight under its MFMAs and the next stage's Philox rounds.
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
    // ---- weight producer
    {
      const int v = u0 + a_ul;
      v4i wq = {0, 0, 0, 0};
      if (a_live && v < a.VU) {
        int t, cb;
        q8_unit(a, v, t, cb);
        const v4i qm = pqm, qs = pqs;
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
            const int w = q8_weight(sext8(qm[q], j), sext8(qs[q], j), eps[j], a);
            wsum += w;
            word |= (w & 0xFF) << (8 * j);
          }
          wq[q] = word;
        }
      }
      lds_a[a_ul * kQ8TM + a_row] = wq;
    }
    // ---- x producer
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int ul = b_u2 + k, v = u0 + ul;
      v4i xq = {0, 0, 0, 0};
      if (b_live && v < a.VU) {
        int t, cb;
        q8_unit(a, v, t, cb);
        const int ky = t / a.KW, kx = t - ky * a.KW;
        const int ih = ih0 + ky * a.dh, iw = iw0 + kx * a.dw;
        const bool inside = ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
        const int c0 = cb * 16;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          int word = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = c0 + 4 * q + j;
            int byte = pad_byte;
            if (c >= a.Ci) {
              byte = 0;
            } else if (inside) {
              const float v = px[k][4 * q + j];
              const float qv = fminf(fmaxf(__fadd_rn(rintf(__fmul_rn(v, a.inv_in)), (float)a.z_in), 0.f), 255.f);
              byte = ((int)qv - 128) & 0xFF;
            }
            word |= byte << (8 * j);
          }
          xq[q] = word;
        }
      }
      lds_b[ul * kQ8TN + b_pl] = xq;
    }
    __syncthreads();
    if (u0 + kQ8SU < a.VU) prefetch(u0 + kQ8SU);
    // ---- consumers
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const int ul = 2 * ch + (lane >> 5);
      const v4i av = lds_a[ul * kQ8TM + 32 * wm + (lane & 31)];
      const v4i b0 = lds_b[ul * kQ8TN + 64 * wn + (lane & 31)];
      const v4i b1 = lds_b[ul * kQ8TN + 64 * wn + 32 + (lane & 31)];
      acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, b1, acc1, 0, 0, 0);
    }
    __syncthreads();   // the stage has been consumed
  }

  // sum_k w of a row: its four producer threads are four adjacent lanes
  wsum += __shfl_xor(wsum, 1, 64);
  wsum += __shfl_xor(wsum, 2, 64);
  if (a_ul == 0) row_sum[a_row] = wsum;
  __syncthreads();

  const long long hw = (long long)a.Ho * a.Wo;
  const int zc = 128 - a.z_in;
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    const long long n = n0 + 64 * wn + 32 * blk + (lane & 31);
    if (n >= a.npix) continue;
    const long long bi = n / hw;
    const long long base = ((long long)s * a.B + bi) * a.Co * hw + (n - bi * hw);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = 32 * wm + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
      const int co = co0 + row;
      if (co >= a.Co) continue;
      const int acc = (blk ? acc1[i] : acc0[i]) + zc * row_sum[row];
      const float t = __fmul_rn(__fmaf_rn(bias_term[row], a.inv_atw, (float)acc), a.m_out);   // fbgemm's: ONE rounding of b * (1 / a) + float(acc)
      const float oq = fminf(fmaxf(__fadd_rn(rintf(t), (float)a.z_out), 0.f), 255.f);
      const long long o = base + (long long)co * hw;
      a.out[o] = __fmul_rn(__fsub_rn(oq, (float)a.z_out), a.s_out);
      if (a.out_q) a.out_q[o] = (uint8_t)oq;
    }
  }
}

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

static int q8_forward(const char* who, const bt_conv2d_geom& g, int S, const float* x, long long x_sample_stride, const bt_q8_params* p, const float* eps_w,
                      const float* eps_b, const bt_rng* rng, float* out, uint8_t* out_q, hipStream_t stream) {
  const Q8Fail fail = {who};
  if (int rc = q8_check_operands(fail, x, p, out, S, x_sample_stride, p ? p->mu_packed : nullptr, p ? p->sigma_packed : nullptr, g)) return rc;
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
  const long long taps = (long long)g.kh * g.kw, Ci16 = ((long long)g.Ci + 15) & ~15ll;

  Q8Args a = {};
  a.x = x, a.x_sample_stride = x_sample_stride, a.qmu = p->mu_packed, a.qsg = p->sigma_packed, a.eps_w = eps_w;
  a.eps_b = eps_b;   // (a supplied bias draw beside on-chip weight draws is read)
  a.mu_b = p->mu_b, a.sigma_b = p->mu_b ? p->sigma_b : nullptr, a.out = out, a.out_q = out_q;
  bt_rng none = {};
  const bt_rng& R = rng ? *rng : none;
  a.call_base = R.call_base_dev, a.kw = make_key(R, 0), a.kb = make_key(R, 1), a.sample0 = R.sample0;
  a.B = g.B, a.Ci = g.Ci, a.H = g.H, a.W = g.W, a.Co = g.Co, a.KH = g.kh, a.KW = g.kw, a.sh = g.sh, a.sw = g.sw, a.ph = g.ph, a.pw = g.pw, a.dh = g.dh, a.dw = g.dw;
  a.Ho = (int)Ho, a.Wo = (int)Wo, a.CB = (int)(Ci16 / 16), a.taps = (int)taps, a.U = (int)(taps * (Ci16 / 16)), a.npix = npix;
  // With z_in == 128 a padding position is the MFMA's zero and no correction term reads the row sum: taps that read padding for every
  // output pixel are not walked (q8_live_taps).
  a.VU = a.U;
  if (p->in.zero_point == 128 && q8_live_taps(g, Ho, Wo, a.CB, a.live_taps, a.VU)) a.pruned = 1;
  const float s_eps = (float)p->eps.scale, s_add = (float)p->add.scale, s_in = (float)p->in.scale, s_out = (float)p->out.scale;
  a.inv_eps = 1.0f / s_eps;
  a.m_mul = (float)(p->s_sigma * p->eps.scale / p->mul.scale);
  a.s_mul = (float)p->mul.scale, a.s_mu = (float)p->s_mu;
  a.inv_add = 1.0f / s_add, a.inv_in = 1.0f / s_in;
  const float atw = s_in * s_add;   // fbgemm's act_times_w_scale and output multiplier: fp32 operations on the fp32 scales
  if (!(atw > 0.f) || !(atw / s_out > 0.f)) return fail(BT_ERR_BAD_ARG, "in scale * add scale (/ out scale) underflows fp32");
  a.m_out = atw / s_out;
  a.inv_atw = 1.0f / atw, a.s_out = s_out;
  a.z_in = p->in.zero_point, a.z_out = p->out.zero_point;
  const dim3 grid((unsigned)((npix + kQ8TN - 1) / kQ8TN), (unsigned)((g.Co + kQ8TM - 1) / kQ8TM), (unsigned)S);
  if (grid.y > 65535u) return fail(BT_ERR_UNSUPPORTED, "more than 65535 * 64 output channels");
  return launch_kernel(q8_fwd_kernel, eps_w ? "q8_fwd<i8 32x32x32,64x128,eps injected>" : "q8_fwd<i8 32x32x32,64x128,eps on chip>", who, grid, dim3(kQ8Threads), 0, 0,
                       stream, a);
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
