// The INT8 forwards (bt_q8.hip: Reparameterization, bt_q8_flip.hip: Flipout) are one walk with different arithmetic. This header
// holds the walk -- q8_walk_kernel<Chain> -- with its argument core, its byte helpers and the host's checks and plan for that core; a
// translation unit adds a chain (the arithmetic), the chain's own arguments and the entry points.
//
// The walk. A workgroup (256 threads, 4 waves as 2 x 2) owns a tile of 64 output channels x 128 output pixels of one sample and walks K
// in stages of four units; a unit is the 16 (padded) input channels of one tap, 16 bytes of either operand. A chain runs kC
// contractions over the same K (1: Reparameterization, 2: Flipout's mean and perturbation), so everything below exists kC times:
//   * producers, weight side: thread (row, unit) reads its 16 bytes of q_mu and q_sigma from the [Co][taps][Ci16] packs, takes the
//     unit's 16 draws (Philox blocks of the tensor 0 stream, or the injected fp32 eps), has the chain turn every four of them into one
//     packed word per contraction and writes the 16 int8 weights to LDS in the MFMA's operand layout; it also sums them (the
//     zero-point correction needs sum_k w over ALL K positions);
//   * producers, x side: thread (pixel, two units) fetches the fp32 NCHW values, quantises them to xq, has the chain turn xq into one
//     byte per contraction (padding: the chain's pad byte, z - 128, so that the correction (128 - z) * sum_k w makes padding a real
//     zero) and writes them to LDS likewise;
//   * consumers: every wave runs 2 K-chunks x 2 pixel blocks x kC contractions of 32x32x32 MFMAs on its 32 x 64 quarter.
// The global operands of a stage are fetched one stage ahead into registers; where padding is the MFMA's zero in every B tile the taps
// that read padding for every output pixel are not walked (DESIGN.md section 4.6f has the measurements). The output stage runs per
// element in registers: the chain makes the u8 level of the kC corrected accumulators and bias terms, the walk stores it.
// Operand layout in LDS: [unit][row or pixel][16 bytes]; lane l of a wave reads the 16 bytes of row l & 31 in unit 2 * chunk + (l >> 5)
// for A and B alike -- the contraction only needs A and B to agree on which k a (lane half, byte) pair means, and they are written
// by the same rule. C/D: column (pixel) l & 31, row (channel) (reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5).
#pragma once
#include "bt_api_internal.h"

namespace bt {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kQ8Threads = 256;
constexpr int kQ8TM = 64;    // output channels per workgroup
constexpr int kQ8TN = 128;   // output pixels per workgroup
constexpr int kQ8SU = 4;     // units (16 K positions each) per stage

// What the walk reads; a chain's argument block derives from it.
struct Q8Core {
  const void* x;   // fp32 [B][Ci][H][W], or (kXU8) the u8 blocked image [B][CB][H][W][16]
  long long x_sample_stride;   // in elements of x's own layout
  const int8_t* qmu;
  const int8_t* qsg;
  const float* eps_w;
  const float* eps_b;
  const float* mu_b;
  const float* sigma_b;
  float* out;        // fp32 [S][B][Co][Ho][Wo]; optional where the kernel writes the blocked image (kOutB)
  uint8_t* out_q;    // u8, optional: [S][B][Co][Ho][Wo] beside out, or (kOutB) the blocked image [S][B][CBo][Ho][Wo][16]
  const uint32_t* call_base;
  RngKey kw, kb;
  uint32_t sample0;
  int B, Ci, H, W, Co, KH, KW, sh, sw, ph, pw, dh, dw, Ho, Wo;
  int CB;     // 16-channel blocks per tap (Ci16 / 16)
  int U;      // units: taps * CB
  int taps;
  int VU;     // units walked: live taps * CB (== U unless taps are pruned)
  int pruned;           // some tap reads padding for every output pixel and padding is the MFMA's zero: such a tap contributes 0 and is skipped
  uint64_t live_taps;   // pruned: the live taps in ascending order, four bits each (taps <= 16)
  long long npix;       // B * Ho * Wo
  float inv_eps, inv_in, s_out;
  int z_in, z_out;
};

__device__ __forceinline__ int clamp_i8(float v) { return (int)fminf(fmaxf(v, -128.f), 127.f); }

__device__ __forceinline__ int sext8(int word, int j) { return (int)(int8_t)((unsigned)word >> (8 * j)); }

// clamp(rne(t) + z, 0, 255): the last stage of every quint8 quantisation, as a float.
__device__ __forceinline__ float q8_level(float t, int z) { return fminf(fmaxf(__fadd_rn(rintf(t), (float)z), 0.f), 255.f); }

// quantize_per_tensor of one activation: clamp(rne(v * (1 / s)) + z, 0, 255).
__device__ __forceinline__ int q8_quant_x(float v, float inv_s, int z) { return (int)q8_level(__fmul_rn(v, inv_s), z); }

// clamp(rne(float(prod) * m) + z, 0, 255): quantized.mul of two quint8 values whose zero-point-free product is prod.
__device__ __forceinline__ int q8_umul(int prod, float m, int z) { return (int)q8_level(__fmul_rn((float)prod, m), z); }

// Walked unit v -> (tap t, 16-channel block cb): the v / CB-th live tap when taps are pruned, else the v / CB-th tap.
__device__ __forceinline__ void q8_unit(const Q8Core& a, int v, int& t, int& cb) {
  const int tv = v / a.CB;
  cb = v - tv * a.CB;
  t = a.pruned ? (int)((a.live_taps >> (4 * tv)) & 15u) : tv;
}

// Walked unit v as the x side sees it, for the output pixel whose window starts at (ih0, iw0): the unit's first channel c0, whether
// its tap lies inside the image, and the offset of (c0, tap) in that image (meaningful only where inside). plane: H * W, which the
// caller holds once (formed here, from a.H and a.W, it costs q8_walk_kernel<Q8Reparam> two registers and with them its third wave).
struct Q8Tap {
  int c0;
  bool inside;
  long long off;
};
__device__ __forceinline__ Q8Tap q8_tap(const Q8Core& a, int v, int ih0, int iw0, long long plane) {
  int t, cb;
  q8_unit(a, v, t, cb);
  const int ky = t / a.KW, kx = t - ky * a.KW;
  const int ih = ih0 + ky * a.dh, iw = iw0 + kx * a.dw;
  Q8Tap r;
  r.c0 = cb * 16;
  r.inside = ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
  r.off = (long long)r.c0 * plane + (long long)ih * a.W + iw;
  return r;
}

// A Chain has
//   kC                                   contractions;
//   Args                                 : Q8Core, the kernel's argument block;
//   Chain(a, s, sample, call_base)       per-workgroup set-up (call_base: what *a.call_base adds to a key's call, 0 without one);
//   bias(mu, has_sigma, sigma, eps, b)   mu_b, sigma_b, eps_b of a channel -> kC bias terms;
//   weights(qm, qs, eps, w, sum)         one packed q_mu word, one packed q_sigma word, their four draws -> kC packed weight words,
//                                        whose bytes it adds to the kC row sums;
//   pads(p)                              the kC bytes of a padding position;
//   activation(xq, off, b)               a quantised x and its offset in one sample's x -> kC bytes;
//   corrections(zc)                      what multiplies the kC row sums;
//   output(acc, b, off)                  kC corrected accumulators, bias terms, the offset in one sample's output -> the u8 level.
//   activation_words(lv, w)              (kWords only) four u8 levels in one word -> kC words, where no byte needs its own offset.
// kXU8: x is the u8 blocked image at the pair (s_in, z_in) -- the 16 channels of one (pixel, tap) are one
// aligned 16-byte load and the producer quantises nothing; bytes of channels >= Ci hold anything (the packs hold 0 there).
// kOutB: the u8 level goes to the blocked image a.out_q, four consecutive channels of a lane as one dword (channels >= Co of the last
// block: z_out), and the fp32 a.out is optional.
template <class Chain, bool kXU8 = false, bool kOutB = false>
__global__ __launch_bounds__(kQ8Threads) void q8_walk_kernel(typename Chain::Args a) {
  constexpr int kC = Chain::kC;
  __shared__ v4i lds_a[kC][kQ8SU * kQ8TM];   // 4 KiB each
  __shared__ v4i lds_b[kC][kQ8SU * kQ8TN];   // 8 KiB each
  __shared__ int row_sum[kC][kQ8TM];
  __shared__ float bias_term[kC][kQ8TM];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int s = blockIdx.z;
  const int co0 = blockIdx.y * kQ8TM;
  const long long n0 = (long long)blockIdx.x * kQ8TN;
  const uint32_t call_base = a.call_base ? *a.call_base : 0u;
  RngKey kw = a.kw, kb = a.kb;
  kw.call += call_base, kb.call += call_base;
  const uint32_t sample = a.sample0 + (uint32_t)s;
  const Chain chain(a, s, sample, call_base);

  // the bias terms of this sample's channels (0 without a bias): the output stage takes them into the accumulators' scales
  if (tid < kQ8TM) {
    const int co = co0 + tid;
    float bt[kC];
#pragma unroll
    for (int c = 0; c < kC; ++c) bt[c] = 0.f;
    if (a.mu_b && co < a.Co) {
      const float mu = a.mu_b[co];
      float sg = 0.f, eb = 0.f;
      if (a.sigma_b) {
        if (a.eps_b) {
          eb = a.eps_b[(long long)s * a.Co + co];
        } else {
          float z[4];
          philox_normal4(kb, sample, (uint32_t)(co >> 2), z);
          eb = z[co & 3];
        }
        sg = a.sigma_b[co];
      }
      chain.bias(mu, a.sigma_b != nullptr, sg, eb, bt);
    }
#pragma unroll
    for (int c = 0; c < kC; ++c) bias_term[c][tid] = bt[c];
  }

  // weight side: this thread's (row, unit of the stage)
  const int a_row = tid >> 2, a_ul = tid & 3;
  const int a_co = co0 + a_row;
  const bool a_live = a_co < a.Co;
  const long long inner4 = ((long long)a.Ci + 3) & ~3ll;
  int wsum[kC];
#pragma unroll
  for (int c = 0; c < kC; ++c) wsum[c] = 0;

  // x side: this thread's pixel and its two units of the stage
  const int b_pl = tid & (kQ8TN - 1), b_u2 = (tid >> 7) * 2;
  const long long b_n = n0 + b_pl;
  const bool b_live = b_n < a.npix;
  int ih0 = 0, iw0 = 0;
  long long xoff0 = 0;   // the offset of this pixel's image in one sample's x
  if (b_live) {
    const long long hw = (long long)a.Ho * a.Wo;
    const long long bi = b_n / hw;
    const int r = (int)(b_n - bi * hw);
    const int oh = r / a.Wo, ow = r - oh * a.Wo;
    ih0 = oh * a.sh - a.ph;
    iw0 = ow * a.sw - a.pw;
    xoff0 = bi * (long long)a.Ci * a.H * a.W;
  }
  const long long plane = (long long)a.H * a.W;
  // this pixel's image: fp32 [Ci][H][W], or the blocked u8 [CB][H][W][16]
  const float* xb = static_cast<const float*>(a.x) + (long long)s * a.x_sample_stride + xoff0;
  const uint8_t* xb8 = nullptr;
  if constexpr (kXU8) xb8 = static_cast<const uint8_t*>(a.x) + (long long)s * a.x_sample_stride + (b_live ? (b_n / ((long long)a.Ho * a.Wo)) : 0) * a.CB * plane * 16;
  int pad[kC];
  chain.pads(pad);

  v16i acc[kC][2];
#pragma unroll
  for (int c = 0; c < kC; ++c)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[c][0][i] = 0, acc[c][1][i] = 0;
  const int wm = wv & 1, wn = wv >> 1;

  // The global operands of a stage are fetched one stage ahead, into registers: this thread's 16 bytes of either pack and its 2 x 16
  // fp32 values of x (0 where nothing is read) -- kXU8: its 2 x 16 bytes. The loads are issued behind the barrier that publishes the
  // current stage and are in flight under its MFMAs and the next stage's Philox rounds.
  v4i pqm = {0, 0, 0, 0}, pqs = {0, 0, 0, 0};
  float px[kXU8 ? 1 : 2][kXU8 ? 1 : 16];
  v4i pxq[kXU8 ? 2 : 1];
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
      Q8Tap tp = {0, false, 0};
      if constexpr (kXU8) {
        pxq[k] = v4i{0, 0, 0, 0};
        if (b_live && v < a.VU) {
          tp = q8_tap(a, v, ih0, iw0, plane);
          // (c0, ih, iw) of [CB][H][W][16]: block c0 / 16, pixel off - c0 * plane
          if (tp.inside) pxq[k] = *reinterpret_cast<const v4i*>(xb8 + ((long long)(tp.c0 >> 4) * plane + (tp.off - (long long)tp.c0 * plane)) * 16);
        }
      } else {
        const float* xp = xb;
        if (b_live && v < a.VU) {
          tp = q8_tap(a, v, ih0, iw0, plane);
          if (tp.inside) xp = xb + tp.off;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) px[k][j] = (tp.inside && tp.c0 + j < a.Ci) ? xp[(long long)j * plane] : 0.f;
      }
    }
  };
  prefetch(0);

  for (int u0 = 0; u0 < a.VU; u0 += kQ8SU) {
    // ---- weight producer
    {
      const int v = u0 + a_ul;
      v4i wq[kC];
#pragma unroll
      for (int c = 0; c < kC; ++c) wq[c] = v4i{0, 0, 0, 0};
      if (a_live && v < a.VU) {
        int t, cb;
        q8_unit(a, v, t, cb);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = cb * 16 + 4 * q;
          float eps[4] = {0.f, 0.f, 0.f, 0.f};
          if (c < a.Ci) {
            if (a.eps_w) {
              const float* ep = a.eps_w + (((long long)s * a.Co + a_co) * a.Ci + c) * a.taps + t;
#pragma unroll
              for (int j = 0; j < 4; ++j)
                if (c + j < a.Ci) eps[j] = ep[(long long)j * a.taps];
            } else {
              philox_normal4(kw, sample, (uint32_t)(eps_stream_index(a_co, c, t, inner4, a.taps) >> 2), eps);
            }
          }
          int w[kC];
          chain.weights(pqm[q], pqs[q], eps, w, wsum);
#pragma unroll
          for (int cc = 0; cc < kC; ++cc) wq[cc][q] = w[cc];
        }
      }
#pragma unroll
      for (int c = 0; c < kC; ++c) lds_a[c][a_ul * kQ8TM + a_row] = wq[c];
    }
    // ---- x producer
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int ul = b_u2 + k, v = u0 + ul;
      v4i xq[kC];
#pragma unroll
      for (int c = 0; c < kC; ++c) xq[c] = v4i{0, 0, 0, 0};
      if (b_live && v < a.VU) {
        const Q8Tap tp = q8_tap(a, v, ih0, iw0, plane);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          int word[kC];
          if constexpr (kXU8 && Chain::kWords) {
            // whole words: a byte of a channel >= Ci meets a zero weight, whatever it holds
            if (tp.inside) {
              chain.activation_words(pxq[k][q], word);
            } else {
#pragma unroll
              for (int c = 0; c < kC; ++c) word[c] = pad[c] * 0x01010101;
            }
#pragma unroll
            for (int c = 0; c < kC; ++c) xq[c][q] = word[c];
            continue;
          }
#pragma unroll
          for (int c = 0; c < kC; ++c) word[c] = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            int byte[kC];
#pragma unroll
            for (int c = 0; c < kC; ++c) byte[c] = pad[c];
            if (tp.c0 + 4 * q + j >= a.Ci) {
#pragma unroll
              for (int c = 0; c < kC; ++c) byte[c] = 0;
            } else if (tp.inside) {
              int lv;
              if constexpr (kXU8) lv = (int)(((unsigned)pxq[k][q] >> (8 * j)) & 0xFFu);
              else lv = q8_quant_x(px[k][4 * q + j], a.inv_in, a.z_in);
              chain.activation(lv, xoff0 + tp.off + (long long)(4 * q + j) * plane, byte);
            }
#pragma unroll
            for (int c = 0; c < kC; ++c) word[c] |= byte[c] << (8 * j);
          }
#pragma unroll
          for (int c = 0; c < kC; ++c) xq[c][q] = word[c];
        }
      }
#pragma unroll
      for (int c = 0; c < kC; ++c) lds_b[c][ul * kQ8TN + b_pl] = xq[c];
    }
    __syncthreads();
    if (u0 + kQ8SU < a.VU) prefetch(u0 + kQ8SU);
    // ---- consumers
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const int ul = 2 * ch + (lane >> 5);
      const int ar = ul * kQ8TM + 32 * wm + (lane & 31), br = ul * kQ8TN + 64 * wn + (lane & 31);
#pragma unroll
      for (int c = 0; c < kC; ++c) {
        const v4i av = lds_a[c][ar];
        acc[c][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, lds_b[c][br], acc[c][0], 0, 0, 0);
        acc[c][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, lds_b[c][br + 32], acc[c][1], 0, 0, 0);
      }
    }
    __syncthreads();   // the stage has been consumed
  }

  // sum_k w of a row: its four producer threads are four adjacent lanes
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    wsum[c] += __shfl_xor(wsum[c], 1, 64);
    wsum[c] += __shfl_xor(wsum[c], 2, 64);
    if (a_ul == 0) row_sum[c][a_row] = wsum[c];
  }
  __syncthreads();

  const long long hw = (long long)a.Ho * a.Wo;
  int zc[kC];
  chain.corrections(zc);
  if constexpr (kOutB) {
    const int CBo = (a.Co + 15) >> 4;
    float* const out_s = a.out ? a.out + (long long)s * a.npix * a.Co : nullptr;
    uint8_t* const outb_s = a.out_q + (long long)s * a.npix * CBo * 16;   // this sample's [B][CBo][Ho][Wo][16]
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const long long n = n0 + 64 * wn + 32 * blk + (lane & 31);
      if (n >= a.npix) continue;
      const long long bi = n / hw, pix = n - bi * hw;
      const long long obase = bi * a.Co * hw + pix;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        // the lane's rows (i & 3) of register group g: four consecutive channels, one dword of the blocked image
        const int row0 = 32 * wm + 8 * g + 4 * (lane >> 5);
        const int cg = co0 + row0;
        if (cg >= CBo * 16) continue;
        unsigned word = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int co = cg + j, row = row0 + j;
          unsigned lv = (unsigned)a.z_out;
          if (co < a.Co) {
            const long long oi = obase + (long long)co * hw;
            int av[kC];
            float bt[kC];
#pragma unroll
            for (int c = 0; c < kC; ++c) av[c] = acc[c][blk][4 * g + j] + zc[c] * row_sum[c][row], bt[c] = bias_term[c][row];
            const float oq = chain.output(av, bt, oi);
            if (out_s) out_s[oi] = __fmul_rn(__fsub_rn(oq, (float)a.z_out), a.s_out);
            lv = (unsigned)oq;
          }
          word |= lv << (8 * j);
        }
        *reinterpret_cast<unsigned*>(outb_s + ((bi * CBo + (cg >> 4)) * hw + pix) * 16 + (cg & 15)) = word;
      }
    }
  } else {
    float* const out_s = a.out + (long long)s * a.npix * a.Co;   // this sample's [B][Co][Ho][Wo]
    uint8_t* const outq_s = a.out_q ? a.out_q + (long long)s * a.npix * a.Co : nullptr;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
      const long long n = n0 + 64 * wn + 32 * blk + (lane & 31);
      if (n >= a.npix) continue;
      const long long bi = n / hw;
      const long long obase = bi * a.Co * hw + (n - bi * hw);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = 32 * wm + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        const int co = co0 + row;
        if (co >= a.Co) continue;
        const long long oi = obase + (long long)co * hw;
        int av[kC];
        float bt[kC];
#pragma unroll
        for (int c = 0; c < kC; ++c) av[c] = acc[c][blk][i] + zc[c] * row_sum[c][row], bt[c] = bias_term[c][row];
        const float oq = chain.output(av, bt, oi);
        out_s[oi] = __fmul_rn(__fsub_rn(oq, (float)a.z_out), a.s_out);
        if (outq_s) outq_s[oi] = (uint8_t)oq;
      }
    }
  }
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

// The refusals the INT8 forwards have in common, in steps between which an entry point checks its own draws, its (scale, zero point)
// pairs and its multipliers. Each returns BT_OK or the recorded error.
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

// What an entry point hands the plan besides the geometry: the operands both chains have. P: bt_q8_params or bt_q8_flip_params.
struct Q8Operands {
  const void* x;
  long long x_sample_stride;
  const float* eps_w;
  const float* eps_b;
  const bt_rng* rng;
  float* out;
  uint8_t* out_q;
};

// The last step: fills the walk's core from checked operands and sizes, and sets the grid. `zero_pad`: a padding position is the
// MFMA's zero in every B tile (all the activations' zero points are 128), so taps that read padding only are not walked (q8_live_taps).
template <class P>
inline int q8_plan(const Q8Fail& fail, const bt_conv2d_geom& g, int S, long long Ho, long long Wo, long long npix, const Q8Operands& o, const P& p, bool zero_pad,
                   Q8Core& a, dim3& grid) {
  a.x = o.x, a.x_sample_stride = o.x_sample_stride, a.qmu = p.mu_packed, a.qsg = p.sigma_packed, a.eps_w = o.eps_w;
  a.eps_b = o.eps_b;   // (a supplied bias draw beside on-chip weight draws is read)
  a.mu_b = p.mu_b, a.sigma_b = p.mu_b ? p.sigma_b : nullptr, a.out = o.out, a.out_q = o.out_q;
  bt_rng none = {};
  const bt_rng& R = o.rng ? *o.rng : none;
  a.call_base = R.call_base_dev, a.kw = make_key(R, 0), a.kb = make_key(R, 1), a.sample0 = R.sample0;
  a.B = g.B, a.Ci = g.Ci, a.H = g.H, a.W = g.W, a.Co = g.Co, a.KH = g.kh, a.KW = g.kw, a.sh = g.sh, a.sw = g.sw, a.ph = g.ph, a.pw = g.pw, a.dh = g.dh, a.dw = g.dw;
  const long long taps = (long long)g.kh * g.kw, CB = (((long long)g.Ci + 15) & ~15ll) / 16;
  a.Ho = (int)Ho, a.Wo = (int)Wo, a.CB = (int)CB, a.taps = (int)taps, a.U = (int)(taps * CB), a.npix = npix;
  a.VU = a.U;
  if (zero_pad && q8_live_taps(g, Ho, Wo, a.CB, a.live_taps, a.VU)) a.pruned = 1;
  a.inv_eps = 1.0f / (float)p.eps.scale, a.inv_in = 1.0f / (float)p.in.scale, a.s_out = (float)p.out.scale;
  a.z_in = p.in.zero_point, a.z_out = p.out.zero_point;
  grid = dim3((unsigned)((npix + kQ8TN - 1) / kQ8TN), (unsigned)((g.Co + kQ8TM - 1) / kQ8TM), (unsigned)S);
  if (grid.y > 65535u) return fail(BT_ERR_UNSUPPORTED, "more than 65535 * 64 output channels");
  return BT_OK;
}

// The *_act entry points: x is fp32 NCHW or the u8 blocked image, the result goes to fp32 `out`, to the u8
// blocked image `out_b`, or to both. What they refuse beyond q8_check_operands, before any launch.
inline int q8_check_act(const Q8Fail& fail, int x_kind, const void* x, const float* out, const uint8_t* out_b) {
  if (x_kind != BT_Q8_X_F32 && x_kind != BT_Q8_X_U8) return fail(BT_ERR_BAD_ARG, "x_kind is neither BT_Q8_X_F32 nor BT_Q8_X_U8");
  if (!out && !out_b) return fail(BT_ERR_BAD_ARG, "neither out nor out_blocked");
  if (x_kind == BT_Q8_X_U8 && (((uintptr_t)x) & 15u)) return fail(BT_ERR_BAD_ARG, "a u8 blocked x must be 16-byte aligned");
  if (((uintptr_t)out_b) & 15u) return fail(BT_ERR_BAD_ARG, "out_blocked must be 16-byte aligned");
  return BT_OK;
}

// One sample's x in elements of its own layout: what x_sample_stride must be a multiple of 16 of for the blocked image.
inline int q8_check_act_stride(const Q8Fail& fail, int x_kind, long long x_sample_stride) {
  if (x_kind == BT_Q8_X_U8 && (x_sample_stride & 15)) return fail(BT_ERR_BAD_ARG, "the sample stride of a u8 blocked x must be a multiple of 16");
  return BT_OK;
}

// The walk's instantiation for (x source, destination). names: [x u8][blocked destination][draws on chip].
template <class Chain>
inline int q8_launch_walk(bool x_u8, bool out_b, bool on_chip, const char* const (&names)[2][2][2], const char* who, dim3 grid, hipStream_t stream,
                          const typename Chain::Args& a) {
  const char* name = names[x_u8][out_b][on_chip];
  const dim3 block(kQ8Threads);
  if (x_u8) {
    if (out_b) return launch_kernel(q8_walk_kernel<Chain, true, true>, name, who, grid, block, 0, 0, stream, a);
    return launch_kernel(q8_walk_kernel<Chain, true, false>, name, who, grid, block, 0, 0, stream, a);
  }
  if (out_b) return launch_kernel(q8_walk_kernel<Chain, false, true>, name, who, grid, block, 0, 0, stream, a);
  return launch_kernel(q8_walk_kernel<Chain, false, false>, name, who, grid, block, 0, 0, stream, a);
}

}  // namespace bt
