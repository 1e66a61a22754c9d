// Backward of the four fused forwards: hand-written data-gradient and weight-gradient
// kernels that REGENERATE the draws on chip from the forward's counter coordinates -- no eps / sign / sampled-weight
// tensor is ever written to or read from HBM (injected draws, the parity mode, are read instead) -- and apply the chain
// rule to (mu, rho) in the weight-gradient's own output stage:
//     W_s = mu + softplus(rho) * eps_s        dL/dmu = sum_s dL/dW_s        dL/drho = sigmoid(rho) * sum_s eps_s * dL/dW_s
//     Flipout: out = conv(x, mu) + conv(x o s_in, softplus(rho) * eps) o s_out   -> the mean path feeds mu, the
//     perturbation path (inputs x o s_in, upstream g o s_out) feeds rho.
// Reference arithmetic differentiated: layers/variational_layers/linear_variational.py:163-181, conv_variational.py:366-385,
// flipout_layers/linear_flipout.py:149-174, conv_flipout.py:376-417 (the reference itself relies on torch autograd).
//
// Both kernels are implicit GEMMs on fp32 MFMA (v_mfma_f32_32x32x2_f32: the exact fp32 FMA chain), 64 x 64 output tiles,
// 4 waves (one 32 x 32 sub-tile each), operands staged through LDS 16 reduction steps at a time:
//   dgrad  dX_s[ci][(b,h,w)]  = sum_{co,tap} W_s[co][ci][tap] * g_s[co][(b,ho,wo)]      W_s regenerated per stage
//   wgrad  D_s[co][(tap,ci)]  = sum_{(b,ho,wo)} g_s[co][.] * x_s[ci][tap window]        then  acc_mu += D_s, acc_rho += eps_s o D_s
// wgrad splits the samples over `groups` workgroups per tile (enough to fill the chip), writes one partial per group, and
// a finishing kernel adds the partials in index order (deterministic), multiplies by sigmoid(rho) and un-permutes the
// tap-major draw layout into the parameters' own [Co][Ci/g][kh][kw].
#include "bt_bwd_plan.h"

namespace bt {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct BwdArgs {
  const float *x, *g;               // x [S or 1][B][Ci][H][W], g = dL/dout [S][B][Co][Ho][Wo]
  const float *mu_pk, *sig_pk;      // tap-major packed (mu, softplus(rho)): [Co][T][Cig4]
  const float *rho_w;               // natural layout (finishing kernel: sigmoid)
  const float *eps_w, *sign_in, *sign_out;  // injected draws (natural layouts) or null
  float *dx, *dmu, *drho;           // dx [S][B][Ci][H][W]; dmu / drho natural [Co][Cig][T]
  float *part;                      // wgrad partials [2][groups][Co][T][Cig4]
  float *part_d;                    // dgrad partials [dchunks][S][x_elems] (behind wgrad's: the two passes may run in ONE launch)
  int pair_wx, pair_wy, pair_nw, pair_dx, pair_dy;   // bwd_pair_kernel: wgrad's grid (x, y) and block count, dgrad's grid (x, y)
  int fin_nw;                       // bwd_finish_pair_kernel: blocks of wgrad's finishing pass (the rest are dgrad's)
  long long x_sample_stride, x_elems, out_elems, w_elems;
  int B, Ci, H, W, Co, KH, KW, SH, SW, PH, PW, DH, DW, G;
  int Ho, Wo, Cig, Cog, Cig4, T, S, flip, groups;
  int dchunks, dchunk;              // dgrad: the reduction over output channels in dchunks pieces of dchunk channels (partials in `part`)
  int sgroups, mchunk;              // wgrad: groups = sgroups (sample s handled by s % sgroups) x chunks of mchunk rows of M = B*Ho*Wo
  uint32_t seed_lo, seed_hi, call, layer_id, sample0;
  const uint32_t* call_base;
  // bt_conv2d_bwd_kl: the layer's KL term differentiated in wgrad's finishing pass (all null / 0 otherwise)
  const float *mu_w, *pmu_w, *psig_w, *gkl;
  int kl_laplace;
};

constexpr int kLS = 68;   // LDS row stride (floats): 64 + 4 keeps the float4 stores aligned and the row reads conflict-free

__device__ __forceinline__ RngKey bwd_key(const BwdArgs& a, uint32_t tensor) {
  RngKey k;
  k.seed_lo = a.seed_lo, k.seed_hi = a.seed_hi;
  k.call = a.call + (a.call_base ? *a.call_base : 0u);
  k.layer_tensor = layer_tensor_word(a.layer_id, tensor);
  return k;
}

// ------------------------------------------------------------------------------------------------------------ dgrad
// grid: (m tiles of 64 positions of one sample) x (ci tiles of 64 per group) x (S * G * dchunks). Taps that connect no
// position of the tile to an output are skipped (3x3 on 1x1 maps: 8 of 9). With dchunks > 1 a workgroup reduces over its
// piece of the output channels and writes a partial; dgrad_finish_kernel adds the pieces in order.
template <bool FLIP>
__device__ __forceinline__ void dgrad_body(const BwdArgs& a, float (*As)[kBK][kLS], float (*Bs)[kBK][kLS], const int bx, const int by, const int bz) {
  // As [kk][ci]: W (Flipout: mu | sigma*eps); Bs [kk][col]: g (Flipout: g | g o s_out)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  const int kc = bz / (a.S * a.G), zr = bz - kc * (a.S * a.G);
  const int s = zr / a.G, grp = zr % a.G;
  const int co_lo = kc * a.dchunk, co_hi = co_lo + a.dchunk < a.Cog ? co_lo + a.dchunk : a.Cog;
  const int ci0 = by * 64, m0 = bx * 64;
  const int HW = a.H * a.W, M = a.B * HW, HoWo = a.Ho * a.Wo;
  const uint32_t sample = a.sample0 + (uint32_t)s;
  const RngKey kw = bwd_key(a, 0);
  uint32_t skey_in = 0, skey_out = 0;
  if (FLIP && !a.sign_in) skey_in = sign_stream_key(bwd_key(a, 2), sample), skey_out = sign_stream_key(bwd_key(a, 3), sample);
  const float* const gs = a.g + (long long)s * a.out_elems;
  // this thread's B-stage columns: col = tid & 63 for kk = (tid >> 6) + 4 j
  const int bcol = tid & 63, m = m0 + bcol;
  const bool mok = m < M;
  const int mb = mok ? m / HW : 0, mh = mok ? (m % HW) / a.W : 0, mw = mok ? m % a.W : 0;
  // A stage: thread = (kk = tid >> 4, ci quad = tid & 15)
  const int akk = tid >> 4, acq = tid & 15, aci = ci0 + 4 * acq;

  f32x16 acc[FLIP ? 2 : 1];
#pragma unroll
  for (int w = 0; w < (FLIP ? 2 : 1); ++w)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[w][r] = 0.f;

  for (int tap = 0; tap < a.T; ++tap) {
    const int kh = tap / a.KW, kwi = tap - kh * a.KW;
    // output position feeding input pixel (mh, mw) through this tap: ho = (mh + PH - kh*DH) / SH when divisible and in range
    const int nh = mh + a.PH - kh * a.DH, nw = mw + a.PW - kwi * a.DW;
    const int ho = nh / a.SH, wo = nw / a.SW;
    const bool pok = mok && nh >= 0 && nw >= 0 && nh - ho * a.SH == 0 && nw - wo * a.SW == 0 && ho < a.Ho && wo < a.Wo;
    const long long gpix = pok ? (long long)mb * a.Co * HoWo + (long long)ho * a.Wo + wo : 0;
    if (!__syncthreads_or(pok ? 1 : 0)) continue;  // this tap meets only padding for every position of the tile
    for (int co0 = co_lo; co0 < co_hi; co0 += kBK) {
      __syncthreads();
      {  // ---- A: 4 consecutive input channels of (co, tap) = one Philox block of the forward's stream
        const int cog = co0 + akk, co = grp * a.Cog + cog;
        float4 wmu = make_float4(0, 0, 0, 0), wd = make_float4(0, 0, 0, 0);
        if (cog < co_hi && aci < a.Cig4) {
          const uint32_t e = ((uint32_t)co * (uint32_t)a.T + (uint32_t)tap) * (uint32_t)a.Cig4 + (uint32_t)aci;
          const float4 m4 = *reinterpret_cast<const float4*>(a.mu_pk + e), s4 = *reinterpret_cast<const float4*>(a.sig_pk + e);
          float ep[4];
          if (a.eps_w) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ep[j] = aci + j < a.Cig ? a.eps_w[(long long)s * a.w_elems + ((long long)co * a.Cig + aci + j) * a.T + tap] : 0.f;
          } else {
            philox_normal4(kw, sample, e >> 2, ep);
          }
          wd = make_float4(__fmul_rn(s4.x, ep[0]), __fmul_rn(s4.y, ep[1]), __fmul_rn(s4.z, ep[2]), __fmul_rn(s4.w, ep[3]));
          wmu = FLIP ? m4 : make_float4(__fadd_rn(m4.x, wd.x), __fadd_rn(m4.y, wd.y), __fadd_rn(m4.z, wd.z), __fadd_rn(m4.w, wd.w));
        }
        *reinterpret_cast<float4*>(&As[0][akk][4 * acq]) = wmu;
        if (FLIP) *reinterpret_cast<float4*>(&As[FLIP ? 1 : 0][akk][4 * acq]) = wd;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // ---- B: upstream gradient at the position this tap connects
        const int kk = (tid >> 6) + 4 * j, cog = co0 + kk;
        float v = 0.f, vp = 0.f;
        if (pok && cog < co_hi) {
          const long long oi = gpix + (long long)(grp * a.Cog + cog) * HoWo;
          v = gs[oi];
          if (FLIP) vp = __fmul_rn(v, a.sign_out ? a.sign_out[(long long)s * a.out_elems + oi] : hash_sign(skey_out, (uint32_t)oi));
        }
        Bs[0][kk][bcol] = v;
        if (FLIP) Bs[FLIP ? 1 : 0][kk][bcol] = vp;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kBK / 2; ++q) {
#pragma unroll
        for (int w = 0; w < (FLIP ? 2 : 1); ++w)
          acc[w] = __builtin_amdgcn_mfma_f32_32x32x2f32(As[w][2 * q + lh][wr + li], Bs[w][2 * q + lh][wc + li], acc[w], 0, 0, 0);
      }
    }
  }
  // D[row = ci][col = position]: lane holds column wc + li, registers hold rows (r&3) + 8 (r>>2) + 4 lh
  const int mcol = m0 + wc + li;
  if (mcol < M) {
    const int b = mcol / HW, hw = mcol - b * HW;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = ci0 + wr + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (ci < a.Cig) {
        const long long xi = ((long long)b * a.Ci + grp * a.Cig + ci) * HW + hw;
        float v = acc[0][r];
        if (FLIP) v = __fadd_rn(v, __fmul_rn(acc[FLIP ? 1 : 0][r], a.sign_in ? a.sign_in[(long long)s * a.x_elems + xi] : hash_sign(skey_in, (uint32_t)xi)));
        if (a.dchunks > 1) a.part_d[((long long)kc * a.S + s) * a.x_elems + xi] = v;
        else a.dx[(long long)s * a.x_elems + xi] = v;
      }
    }
  }
}

template <bool FLIP>
__global__ __launch_bounds__(256) void dgrad_kernel(const BwdArgs a) {
  __shared__ __attribute__((aligned(16))) float As[FLIP ? 2 : 1][kBK][kLS];
  __shared__ __attribute__((aligned(16))) float Bs[FLIP ? 2 : 1][kBK][kLS];
  dgrad_body<FLIP>(a, As, Bs, blockIdx.x, blockIdx.y, blockIdx.z);
}

// dx <- sum of the dchunks partials, in piece order (block bid of nb)
__device__ __forceinline__ void dgrad_finish_body(const BwdArgs& a, const int bid, const int nb) {
  const long long n = (long long)a.S * a.x_elems;
  for (long long i = (long long)bid * 256 + threadIdx.x; i < n; i += (long long)nb * 256) {
    float v = 0.f;
    for (int c = 0; c < a.dchunks; ++c) v = __fadd_rn(v, a.part_d[(long long)c * n + i]);
    a.dx[i] = v;
  }
}
__global__ __launch_bounds__(256) void dgrad_finish_kernel(const BwdArgs a) { dgrad_finish_body(a, blockIdx.x, gridDim.x); }

// n / d (0 <= n < 2^31, d >= 1) through the reciprocal inv = ceil(2^32 / d): the estimate is the quotient or one more, one compare fixes it.
__device__ __forceinline__ uint32_t recip32(int d) { return d > 1 ? 0xFFFFFFFFu / (uint32_t)d + 1u : 0u; }
__device__ __forceinline__ int div_recip(int n, int d, uint32_t inv) {
  if (d == 1) return n;
  uint32_t q = __umulhi((uint32_t)n, inv);
  if (q * (uint32_t)d > (uint32_t)n) --q;
  return (int)q;
}

// ------------------------------------------------------------------------------------------------------------ wgrad
// grid: (k' tiles of 64 over T*Cig4) x (co tiles of 64 per group) x (groups * G); group q = (sample group q % sgroups: samples
// s = q % sgroups + i * sgroups) x (chunk q / sgroups of the reduction axis M = B*Ho*Wo: rows [c * mchunk, (c + 1) * mchunk))
template <bool FLIP>
__device__ __forceinline__ void wgrad_body(const BwdArgs& a, float (*As)[kBK][kLS], float (*Bs)[kBK][kLS], const int bx, const int by, const int bz) {
  // As [mm][co]: g (Flipout: g | g o s_out); Bs [mm][k']: x window (Flipout: x | x o s_in)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  const int sgrp = bz / a.G, grp = bz % a.G;
  const int co0 = by * 64, k0 = bx * 64;
  const int KP = a.T * a.Cig4, HW = a.H * a.W, HoWo = a.Ho * a.Wo, M = a.B * HoWo;
  const RngKey kw = bwd_key(a, 0);
  // this thread's staging columns: col = tid & 63 (a co for A, a k' for B), mm = (tid >> 6) + 4 j
  const int scol = tid & 63;
  const int kp = k0 + scol, tap = kp < KP ? kp / a.Cig4 : 0, kci = kp - tap * a.Cig4;
  const bool kok = kp < KP && kci < a.Cig;
  const int kh = tap / a.KW, kwi = tap - kh * a.KW;
  const int aco = co0 + scol;
  const bool cok = aco < a.Cog;

  f32x16 acc_mu, acc_rho;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc_mu[r] = 0.f, acc_rho[r] = 0.f;

  const uint32_t inv_howo = recip32(HoWo), inv_wo = recip32(a.Wo);
  const int sg0 = sgrp % a.sgroups, mlo = (sgrp / a.sgroups) * a.mchunk, mhi = mlo + a.mchunk < M ? mlo + a.mchunk : M;
  for (int s = sg0; s < a.S; s += a.sgroups) {
    const uint32_t sample = a.sample0 + (uint32_t)s;
    uint32_t skey_in = 0, skey_out = 0;
    if (FLIP && !a.sign_in) skey_in = sign_stream_key(bwd_key(a, 2), sample), skey_out = sign_stream_key(bwd_key(a, 3), sample);
    const float* const gs = a.g + (long long)s * a.out_elems;
    const float* const xs = a.x + (long long)s * a.x_sample_stride;
    f32x16 d[FLIP ? 2 : 1];
#pragma unroll
    for (int w = 0; w < (FLIP ? 2 : 1); ++w)
#pragma unroll
      for (int r = 0; r < 16; ++r) d[w][r] = 0.f;
    for (int mm0 = mlo; mm0 < mhi; mm0 += kBK) {
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int mm = (tid >> 6) + 4 * j, m = mm0 + mm;
        const bool mok = m < mhi;
        // (reciprocal multiplies: two integer divisions per element and stage were ~a quarter of this loop's instructions)
        const int b = mok ? div_recip(m, HoWo, inv_howo) : 0, p = mok ? m - b * HoWo : 0, ho = div_recip(p, a.Wo, inv_wo), wo = p - ho * a.Wo;
        float ga = 0.f, gp = 0.f, xv = 0.f, xp = 0.f;
        if (mok && cok) {
          const long long oi = ((long long)b * a.Co + grp * a.Cog + aco) * HoWo + p;
          ga = gs[oi];
          if (FLIP) gp = __fmul_rn(ga, a.sign_out ? a.sign_out[(long long)s * a.out_elems + oi] : hash_sign(skey_out, (uint32_t)oi));
        }
        const int hi = ho * a.SH - a.PH + kh * a.DH, wi = wo * a.SW - a.PW + kwi * a.DW;
        if (mok && kok && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W) {
          const long long xi = ((long long)b * a.Ci + grp * a.Cig + kci) * HW + (long long)hi * a.W + wi;
          xv = xs[xi];
          if (FLIP) xp = __fmul_rn(xv, a.sign_in ? a.sign_in[(long long)s * a.x_elems + xi] : hash_sign(skey_in, (uint32_t)xi));
        }
        As[0][mm][scol] = ga, Bs[0][mm][scol] = xv;
        if (FLIP) As[FLIP ? 1 : 0][mm][scol] = gp, Bs[FLIP ? 1 : 0][mm][scol] = xp;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kBK / 2; ++q) {
#pragma unroll
        for (int w = 0; w < (FLIP ? 2 : 1); ++w)
          d[w] = __builtin_amdgcn_mfma_f32_32x32x2f32(As[w][2 * q + lh][wr + li], Bs[w][2 * q + lh][wc + li], d[w], 0, 0, 0);
      }
    }
    // chain rule of this sample: the mean path adds to dmu, the eps-weighted (perturbation) path to the rho accumulator
    const int kpl = k0 + wc + li, ltap = kpl < KP ? kpl / a.Cig4 : 0, lci = kpl - ltap * a.Cig4;
    // On-chip draws: the four lanes of a quad (columns 4 q .. 4 q + 3 = the four channels of ONE Philox block of a row) used to run the
    // same block each, once per accumulator row -- 16 blocks per lane and sample. Now lane j of the quad draws the blocks of the rows
    // r = j (mod 4) and the quad exchanges them: 4 blocks per lane, the same values.
    float Z[4][4];
    if (!a.eps_w) {
      const bool quad_ok = (kpl & ~3) < KP && (lci & ~3) < a.Cig;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int r = 4 * t + (li & 3), cog = co0 + wr + (r & 3) + 8 * (r >> 2) + 4 * lh;
        Z[t][0] = Z[t][1] = Z[t][2] = Z[t][3] = 0.f;
        if (quad_ok && cog < a.Cog)
          philox_normal4(kw, sample, (((uint32_t)(grp * a.Cog + cog) * (uint32_t)a.T + (uint32_t)ltap) * (uint32_t)a.Cig4 + (uint32_t)lci) >> 2, Z[t]);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int cog = co0 + wr + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const bool ok = kpl < KP && lci < a.Cig && cog < a.Cog;
      float e = 0.f;
      if (a.eps_w) {
        if (ok) e = a.eps_w[(long long)s * a.w_elems + ((long long)(grp * a.Cog + cog) * a.Cig + lci) * a.T + ltap];
      } else {
        const int src = (lane & ~3) | (r & 3);   // the quad lane that drew row r's block
        const float v0 = __shfl(Z[r >> 2][0], src, 64), v1 = __shfl(Z[r >> 2][1], src, 64), v2 = __shfl(Z[r >> 2][2], src, 64), v3 = __shfl(Z[r >> 2][3], src, 64);
        const int sel = lci & 3;
        e = sel == 0 ? v0 : sel == 1 ? v1 : sel == 2 ? v2 : v3;
        if (!ok) e = 0.f;
      }
      acc_mu[r] = __fadd_rn(acc_mu[r], d[0][r]);
      acc_rho[r] = __fadd_rn(acc_rho[r], __fmul_rn(e, d[FLIP ? 1 : 0][r]));
    }
  }
  // partials [2][groups][Co][KP]
  const int kpl = k0 + wc + li;
  if (kpl < KP) {
    const long long plane = (long long)a.Co * KP;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int cog = co0 + wr + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (cog < a.Cog) {
        const long long o = ((long long)sgrp * a.Co + grp * a.Cog + cog) * KP + kpl;
        a.part[o] = acc_mu[r];
        a.part[(long long)a.groups * plane + o] = acc_rho[r];
      }
    }
  }
}

template <bool FLIP>
__global__ __launch_bounds__(256) void wgrad_kernel(const BwdArgs a) {
  __shared__ __attribute__((aligned(16))) float As[FLIP ? 2 : 1][kBK][kLS];
  __shared__ __attribute__((aligned(16))) float Bs[FLIP ? 2 : 1][kBK][kLS];
  wgrad_body<FLIP>(a, As, Bs, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Both passes of a layer in ONE launch: they read the same upstream gradient and are independent of each other, and at one sample per
// step each is a few hundred short workgroups -- 28 + 35 us back to back on ResNet18 / CIFAR, the longer of the two side by side.
// Blocks [0, pair_nw) are wgrad's grid (x fastest, then y, then z) -- the longer pass first --, the rest dgrad's.
template <bool FLIP>
__global__ __launch_bounds__(256) void bwd_pair_kernel(const BwdArgs a) {
  __shared__ __attribute__((aligned(16))) float As[FLIP ? 2 : 1][kBK][kLS];
  __shared__ __attribute__((aligned(16))) float Bs[FLIP ? 2 : 1][kBK][kLS];
  int L = blockIdx.x;
  if (L < a.pair_nw) {
    const int q = L / a.pair_wx, bx = L - q * a.pair_wx, bz = q / a.pair_wy, by = q - bz * a.pair_wy;
    wgrad_body<FLIP>(a, As, Bs, bx, by, bz);
  } else {
    L -= a.pair_nw;
    const int q = L / a.pair_dx, bx = L - q * a.pair_dx, bz = q / a.pair_dy, by = q - bz * a.pair_dy;
    dgrad_body<FLIP>(a, As, Bs, bx, by, bz);
  }
}

// natural element (co, ci, tap) <- sum over the groups' partials at the tap-major position, in group order; with a.gkl also the
// layer's KL term: grad = (contraction path) + (KL path), the sum autograd's AccumulateGrad would have made of the two tensors.
__device__ __forceinline__ void wgrad_finish_body(const BwdArgs& a, const int bid, const int nb) {
  const long long n = (long long)a.Co * a.Cig * a.T;
  const int KP = a.T * a.Cig4;
  const long long plane = (long long)a.Co * KP;
  const float gkl_s = a.gkl ? a.gkl[0] / (float)n : 0.f;
  for (long long i = (long long)bid * 256 + threadIdx.x; i < n; i += (long long)nb * 256) {
    const int tap = (int)(i % a.T);
    const long long rc = i / a.T;
    const int ci = (int)(rc % a.Cig), co = (int)(rc / a.Cig);
    const long long o = (long long)co * KP + (long long)tap * a.Cig4 + ci;
    float sm = 0.f, sr = 0.f;
    for (int gq = 0; gq < a.groups; ++gq) sm = __fadd_rn(sm, a.part[gq * plane + o]), sr = __fadd_rn(sr, a.part[(a.groups + gq) * plane + o]);
    const float r = a.rho_w[i];
    const float sg = __builtin_amdgcn_rcpf(__fadd_rn(1.0f, __builtin_amdgcn_exp2f(__fmul_rn(-1.4426950408889634f, r))));  // sigmoid(rho)
    float om = sm, orr = __fmul_rn(sr, sg);
    if (a.gkl) {
      float km, kr;
      kl_elem_grad(a.mu_w[i], r, a.pmu_w, a.psig_w, i, a.kl_laplace, gkl_s, km, kr);
      om = __fadd_rn(om, km), orr = __fadd_rn(orr, kr);
    }
    if (a.dmu) a.dmu[i] = om;
    if (a.drho) a.drho[i] = orr;
  }
}
__global__ __launch_bounds__(256) void wgrad_finish_kernel(const BwdArgs a) { wgrad_finish_body(a, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(256) void bwd_finish_pair_kernel(const BwdArgs a) {   // blocks [0, fin_nw): wgrad's finishing pass, the rest dgrad's
  if ((int)blockIdx.x < a.fin_nw) wgrad_finish_body(a, blockIdx.x, a.fin_nw);
  else dgrad_finish_body(a, (int)blockIdx.x - a.fin_nw, (int)gridDim.x - a.fin_nw);
}

// Plan-only digest of the argument block: what it means, not its bytes (the struct has tail padding). Pointers, then every scalar, in this order.
uint64_t digest_arg(uint64_t h, const BwdArgs& a) {
  for (const void* p : std::initializer_list<const void*>{a.x, a.g, a.mu_pk, a.sig_pk, a.rho_w, a.eps_w, a.sign_in, a.sign_out, a.dx, a.dmu, a.drho, a.part, a.part_d,
                                                          a.call_base, a.mu_w, a.pmu_w, a.psig_w, a.gkl})
    h = digest_arg(h, p);
  for (long long v : {a.x_sample_stride, a.x_elems, a.out_elems, a.w_elems}) h = digest_arg(h, v);
  for (int v : {a.pair_wx, a.pair_wy, a.pair_nw, a.pair_dx, a.pair_dy, a.fin_nw, a.B, a.Ci, a.H, a.W, a.Co, a.KH, a.KW, a.SH, a.SW, a.PH, a.PW, a.DH, a.DW, a.G,
                a.Ho, a.Wo, a.Cig, a.Cog, a.Cig4, a.T, a.S, a.flip, a.groups, a.dchunks, a.dchunk, a.sgroups, a.mchunk, a.kl_laplace})
    h = digest_arg(h, v);
  for (uint32_t v : {a.seed_lo, a.seed_hi, a.call, a.layer_id, a.sample0}) h = digest_arg(h, v);
  return h;
}

}  // namespace bt

extern "C" size_t bt_conv2d_bwd_workspace(const bt_conv2d_geom* g, int32_t S) {
  bt::BwdPlan pl;
  return g && bt::bwd_plan(*g, S, true, true, &pl) == bt::kBwdOk ? pl.wgrad_bytes + pl.dgrad_bytes : 0;
}

static int conv2d_bwd_impl(const bt_conv2d_geom* g, int32_t S, int32_t flipout, const float* x, int64_t x_sample_stride, const float* grad_out,
                           const bt_params* p, const bt_draws* d, const float* grad_kl, float* dx, float* dmu_w, float* drho_w, void* workspace,
                           size_t workspace_bytes, bt_stream_t stream) {
  using namespace bt;
  if (!g || !x || !grad_out || !p || !d) return set_error(BT_ERR_BAD_ARG, "bt_conv2d_bwd: null argument");
  if (grad_kl) {
    const bool lap = p->prior_kind == BT_PRIOR_LAPLACE;
    if (!dmu_w) return set_error(BT_ERR_BAD_ARG, "bt_conv2d_bwd_kl: grad_kl needs dmu_w / drho_w");
    if (!p->mu_w || (!lap && (!p->prior_mu_w || !p->prior_sigma_w))) return set_error(BT_ERR_BAD_ARG, "bt_conv2d_bwd_kl: needs mu_w and the weight priors");
  }
  if (!p->mu_packed || !p->sigma_packed || !p->rho_w) return set_error(BT_ERR_BAD_ARG, "bt_conv2d_bwd: needs rho_w and the packed parameters (bt_pack_params)");
  // dgrad reads the packs as float4 quads (the one access of this file wider than 4 bytes); a pack is a buffer of its own, never a slice
  if ((((uintptr_t)p->mu_packed | (uintptr_t)p->sigma_packed) & 15u) != 0) return set_error(BT_ERR_BAD_ARG, "bt_conv2d_bwd: mu_packed / sigma_packed must be 16-byte aligned");
  BwdPlan pl;
  const int refused = bwd_plan(*g, S, dx != nullptr, dmu_w != nullptr, &pl);
  if (refused == kBwdBadGeometry || x_sample_stride < 0) return set_error(BT_ERR_BAD_ARG, "bt_conv2d_bwd: bad geometry");
  if ((dmu_w == nullptr) != (drho_w == nullptr)) return set_error(BT_ERR_BAD_ARG, "bt_conv2d_bwd: dmu_w and drho_w go together");
  const bool inj = d->eps_w != nullptr;
  if (flipout && inj != (d->sign_in != nullptr && d->sign_out != nullptr)) return set_error(BT_ERR_BAD_ARG, "bt_conv2d_bwd: inject all draws or none");
  if (refused == kBwdEmptyOutput) return set_error(BT_ERR_BAD_ARG, "bt_conv2d_bwd: empty output");
  if (refused == kBwdTooLarge) return set_error(BT_ERR_UNSUPPORTED, "bt_conv2d_bwd: tensor too large for the 32-bit sign / draw indices");
  if (((dx && pl.dchunks > 1) || dmu_w) && (!workspace || workspace_bytes < pl.wgrad_bytes + pl.dgrad_bytes))
    return set_error(BT_ERR_WORKSPACE, "bt_conv2d_bwd: workspace smaller than bt_conv2d_bwd_workspace()");
  BwdArgs a = {};
  a.x = x, a.g = grad_out, a.mu_pk = p->mu_packed, a.sig_pk = p->sigma_packed, a.rho_w = p->rho_w;
  a.eps_w = d->eps_w, a.sign_in = flipout ? d->sign_in : nullptr, a.sign_out = flipout ? d->sign_out : nullptr;
  a.dx = dx, a.dmu = dmu_w, a.drho = drho_w, a.part = (float*)workspace;
  a.part_d = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + pl.part_d_offset);   // dgrad's partials live behind wgrad's
  if (grad_kl) a.gkl = grad_kl, a.mu_w = p->mu_w, a.pmu_w = p->prior_mu_w, a.psig_w = p->prior_sigma_w, a.kl_laplace = p->prior_kind == BT_PRIOR_LAPLACE ? 1 : 0;
  a.B = g->B, a.Ci = g->Ci, a.H = g->H, a.W = g->W, a.Co = g->Co, a.KH = g->kh, a.KW = g->kw;
  a.SH = g->sh, a.SW = g->sw, a.PH = g->ph, a.PW = g->pw, a.DH = g->dh, a.DW = g->dw, a.G = g->groups;
  a.Ho = pl.Ho, a.Wo = pl.Wo, a.Cig = pl.Cig, a.Cog = pl.Cog, a.Cig4 = pl.Cig4, a.T = pl.T, a.S = S, a.flip = flipout ? 1 : 0;
  a.x_sample_stride = x_sample_stride, a.x_elems = pl.x_elems, a.out_elems = pl.out_elems, a.w_elems = pl.w_elems;
  if (dx) a.dchunks = pl.dchunks, a.dchunk = pl.dchunk;
  if (dmu_w) a.groups = pl.groups, a.sgroups = pl.sgroups, a.mchunk = pl.mchunk;
  a.seed_lo = (uint32_t)d->rng.seed, a.seed_hi = (uint32_t)(d->rng.seed >> 32);
  a.call = d->rng.call, a.call_base = d->rng.call_base_dev, a.layer_id = d->rng.layer_id, a.sample0 = d->rng.sample0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 wgrid(pl.wgrid[0], pl.wgrid[1], pl.wgrid[2]), dgrid(pl.dgrid[0], pl.dgrid[1], pl.dgrid[2]), block(256);
  if (pl.pair) {   // both passes: ONE launch, and one for the two finishing passes
    a.pair_wx = (int)wgrid.x, a.pair_wy = (int)wgrid.y, a.pair_nw = (int)pl.wblocks, a.pair_dx = (int)dgrid.x, a.pair_dy = (int)dgrid.y;
    if (int rc = launch_kernel(flipout ? bwd_pair_kernel<true> : bwd_pair_kernel<false>, nullptr, "bt_conv2d_bwd (wgrad + dgrad)", dim3((unsigned)(pl.wblocks + pl.dblocks)), block, 0, 0, st, a)) return rc;
    a.fin_nw = pl.n_wfin;
    return launch_kernel(bwd_finish_pair_kernel, nullptr, "bt_conv2d_bwd (finish)", dim3((unsigned)(pl.n_wfin + pl.n_dfin)), block, 0, 0, st, a);
  }
  if (dx) {
    if (int rc = launch_kernel(flipout ? dgrad_kernel<true> : dgrad_kernel<false>, nullptr, "bt_conv2d_bwd (dgrad)", dgrid, block, 0, 0, st, a)) return rc;
    if (pl.n_dfin)
      if (int rc = launch_kernel(dgrad_finish_kernel, nullptr, "bt_conv2d_bwd (dgrad finish)", dim3((unsigned)pl.n_dfin), block, 0, 0, st, a)) return rc;
  }
  if (dmu_w) {
    if (int rc = launch_kernel(flipout ? wgrad_kernel<true> : wgrad_kernel<false>, nullptr, "bt_conv2d_bwd (wgrad)", wgrid, block, 0, 0, st, a)) return rc;
    if (int rc = launch_kernel(wgrad_finish_kernel, nullptr, "bt_conv2d_bwd (finish)", dim3((unsigned)pl.n_wfin), block, 0, 0, st, a)) return rc;
  }
  return BT_OK;
}

extern "C" int bt_conv2d_bwd(const bt_conv2d_geom* g, int32_t S, int32_t flipout, const float* x, int64_t x_sample_stride, const float* grad_out,
                             const bt_params* p, const bt_draws* d, float* dx, float* dmu_w, float* drho_w, void* workspace, size_t workspace_bytes,
                             bt_stream_t stream) {
  return conv2d_bwd_impl(g, S, flipout, x, x_sample_stride, grad_out, p, d, nullptr, dx, dmu_w, drho_w, workspace, workspace_bytes, stream);
}

extern "C" int bt_conv2d_bwd_kl(const bt_conv2d_geom* g, int32_t S, int32_t flipout, const float* x, int64_t x_sample_stride, const float* grad_out,
                                const bt_params* p, const bt_draws* d, const float* grad_kl, float* dx, float* dmu_w, float* drho_w, void* workspace,
                                size_t workspace_bytes, bt_stream_t stream) {
  return conv2d_bwd_impl(g, S, flipout, x, x_sample_stride, grad_out, p, d, grad_kl, dx, dmu_w, drho_w, workspace, workspace_bytes, stream);
}

// Test hooks (not part of include/bt_hip.h): the workgroup targets of the two passes (<= 0: the default), and pairing on / off.
extern "C" void bt_debug_bwd_targets(int wgrad, int dgrad) { bt::g_wgrad_wgs.set(wgrad > 0 ? wgrad : bt::kWgradWgs), bt::g_dgrad_wgs.set(dgrad > 0 ? dgrad : bt::kDgradWgs); }
extern "C" void bt_debug_bwd_pair(int on) { bt::g_no_bwd_pair.set(on ? 0 : 1); }
