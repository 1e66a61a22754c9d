// Training backward of the low-rank multivariate Conv2d layer (layers/_lowrank.py; the forward is fused_fwd_kernel's LOWRANK form, the KL
// bt_kl_lowrank). The reference differentiates conv_variational.py:516-552 with torch autograd over a materialised [S, n] weight tensor.
//   lr_dgrad    dX_s[ci][(b,h,w)] = sum_{co,tap} W_s[co][ci][tap] * g_s[co][(b,ho,wo)],  W_s regenerated per LDS stage as the forward forms it:
//               w = mean_s[i] + sum_{q < R} L[i][q] * z_s[q] + sd * eps_s[i]   (q ascending, one rounding per operation), mean and L read in
//               the parameters' natural layout [Co][Ci][kh][kw], eps at the forward's element-to-block mapping (tap-major, quad-aligned);
//   lr_wgrad    D_s[co][ci][tap] = sum_{(b,ho,wo)} g_s[co][.] * x_s[ci][tap window], per sample (it needs no draws), natural layout;
//   lr_finish   dmu[i] = sum_s D_s[i],  dL[i][j] = sum_s D_s[i] * z_s[j]   (s ascending) over the n x (1 + r) parameter gradients;
//   bt_kl_lowrank_bwd   the closed-form KL's gradient in fp64 from the forward's sweep, its Cholesky factor and an explicit r x r inverse.
// The two implicit GEMMs are bt_bwd.hip's: fp32 MFMA (v_mfma_f32_32x32x2_f32), 64 x 64 tiles, 4 waves, 16 reduction steps per LDS stage, and
// bwd_plan's split of dgrad's output channels and of wgrad's reduction axis; partials are added in a fixed order by kernels of their own
// -- no atomics: the same coordinates give the same bits.
#include <float.h>
#include <math.h>
#include <string.h>

#include "bt_bwd_plan.h"

namespace bt {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct LrBwdArgs {
  const float *x, *g;                  // x [S or 1][B][Ci][H][W], g = dL/dout [S][B][Co][Ho][Wo]
  const float *mean, *L;               // natural [Co][Ci][T] (mean: + s * mean_stride), L [n][R]
  const float *z, *eps_w;              // supplied draws z [S][R], eps_w [S][n], or null
  float *dx, *dw;                      // dx [S][B][Ci][H][W]; dw [S][n]
  float *part_w;                       // wgrad partials [S][mchunks][n] (mchunks > 1)
  float *part_d;                       // dgrad partials [dchunks][S][x_elems] (dchunks > 1)
  const uint32_t* call_base;
  long long x_sample_stride, mean_stride, x_elems, out_elems, w_elems;
  int B, Ci, H, W, Co, KH, KW, SH, SW, PH, PW, DH, DW;
  int Ho, Wo, Ci4, T, S, R;
  int dchunks, dchunk;                 // dgrad: the output channels in dchunks pieces of dchunk
  int mchunks, mchunk;                 // wgrad: M = B*Ho*Wo in mchunks chunks of mchunk rows
  float sd;
  uint32_t seed_lo, seed_hi, call, layer_id, sample0;
};

constexpr int kLS = 68;   // LDS row stride (floats): 64 + 4 keeps the float4 stores aligned and the row reads conflict-free

__device__ __forceinline__ RngKey lr_key(const LrBwdArgs& a, uint32_t tensor) {
  RngKey k;
  k.seed_lo = a.seed_lo, k.seed_hi = a.seed_hi;
  k.call = a.call + (a.call_base ? *a.call_base : 0u);
  k.layer_tensor = layer_tensor_word(a.layer_id, tensor);
  return k;
}

// ------------------------------------------------------------------------------------------------------------ dgrad
// grid: (m tiles of 64 positions of one sample) x (ci tiles of 64) x (S * dchunks). Taps that connect no position of the tile to an
// output are skipped. With dchunks > 1 a workgroup reduces over its piece of the output channels and writes a partial.
__global__ __launch_bounds__(256) void lr_dgrad_kernel(const LrBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float As[kBK][kLS];   // [kk][ci]: W_s
  __shared__ __attribute__((aligned(16))) float Bs[kBK][kLS];   // [kk][col]: g
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  const int kc = blockIdx.z / a.S, s = blockIdx.z - kc * a.S;
  const int co_lo = kc * a.dchunk, co_hi = co_lo + a.dchunk < a.Co ? co_lo + a.dchunk : a.Co;
  const int ci0 = blockIdx.y * 64, m0 = blockIdx.x * 64;
  const int HW = a.H * a.W, M = a.B * HW, HoWo = a.Ho * a.Wo;
  const uint32_t sample = a.sample0 + (uint32_t)s;
  const RngKey kw = lr_key(a, 0);
  float zs[4] = {0.f, 0.f, 0.f, 0.f};   // z_s[0..R): entries past R are never multiplied
  if (a.R > 0) {
    if (a.z) {
#pragma unroll
      for (int q = 0; q < 4; ++q) zs[q] = q < a.R ? a.z[(long long)s * a.R + q] : 0.f;
    } else {
      philox_normal4(lr_key(a, 4), sample, 0u, zs);
    }
  }
  const float* const gs = a.g + (long long)s * a.out_elems;
  const float* const mean_s = a.mean + (long long)s * a.mean_stride;
  // this thread's B-stage columns: col = tid & 63 for kk = (tid >> 6) + 4 j
  const int bcol = tid & 63, m = m0 + bcol;
  const bool mok = m < M;
  const int mb = mok ? m / HW : 0, mh = mok ? (m % HW) / a.W : 0, mw = mok ? m % a.W : 0;
  // A stage: thread = (kk = tid >> 4, ci quad = tid & 15)
  const int akk = tid >> 4, acq = tid & 15, aci = ci0 + 4 * acq;

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

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
        const int co = co0 + akk;
        float w4[4] = {0.f, 0.f, 0.f, 0.f};
        if (co < co_hi && aci < a.Ci) {
          float ep[4] = {0.f, 0.f, 0.f, 0.f};
          if (a.eps_w) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (aci + j < a.Ci) ep[j] = a.eps_w[(long long)s * a.w_elems + ((long long)co * a.Ci + aci + j) * a.T + tap];
          } else {
            const uint32_t e = ((uint32_t)co * (uint32_t)a.T + (uint32_t)tap) * (uint32_t)a.Ci4 + (uint32_t)aci;
            philox_normal4(kw, sample, e >> 2, ep);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (aci + j < a.Ci) {
              const long long i = ((long long)co * a.Ci + aci + j) * a.T + tap;
              float w = mean_s[i];
#pragma unroll
              for (int q = 0; q < 4; ++q)
                if (q < a.R) w = __fadd_rn(w, __fmul_rn(a.L[i * a.R + q], zs[q]));
              w4[j] = __fadd_rn(w, __fmul_rn(a.sd, ep[j]));
            }
          }
        }
        *reinterpret_cast<float4*>(&As[akk][4 * acq]) = make_float4(w4[0], w4[1], w4[2], w4[3]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // ---- B: upstream gradient at the position this tap connects
        const int kk = (tid >> 6) + 4 * j, co = co0 + kk;
        float v = 0.f;
        if (pok && co < co_hi) v = gs[gpix + (long long)co * HoWo];
        Bs[kk][bcol] = v;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < kBK / 2; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * q + lh][wr + li], Bs[2 * q + lh][wc + li], acc, 0, 0, 0);
    }
  }
  // D[row = ci][col = position]: lane holds column wc + li, registers hold rows (r&3) + 8 (r>>2) + 4 lh
  const int mcol = m0 + wc + li;
  if (mcol < M) {
    const int b = mcol / HW, hw = mcol - b * HW;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ci = ci0 + wr + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (ci < a.Ci) {
        const long long xi = ((long long)b * a.Ci + ci) * HW + hw;
        if (a.dchunks > 1) a.part_d[((long long)kc * a.S + s) * a.x_elems + xi] = acc[r];
        else a.dx[(long long)s * a.x_elems + xi] = acc[r];
      }
    }
  }
}

// out[i] <- sum over c < pieces of part[c * piece_stride + (i / inner) * outer_stride + i % inner], in piece order.
//   dgrad: part [dchunks][S * x_elems]   -> inner = total, outer_stride = 0, piece_stride = total;
//   wgrad: part [S][mchunks][n] -> dw [S][n]: inner = n, outer_stride = mchunks * n, piece_stride = n.
__global__ __launch_bounds__(256) void lr_sum_pieces_kernel(const float* __restrict__ part, int pieces, long long piece_stride, long long inner, long long outer_stride,
                                                            long long total, float* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long o = i / inner, base = o * outer_stride + (i - o * inner);
    float v = 0.f;
    for (int c = 0; c < pieces; ++c) v = __fadd_rn(v, part[(long long)c * piece_stride + base]);
    out[i] = v;
  }
}

// n / d (0 <= n < 2^31, d >= 1) through the reciprocal inv = ceil(2^32 / d): the estimate is the quotient or one more, one compare fixes it.
__device__ __forceinline__ uint32_t lr_recip32(int d) { return d > 1 ? 0xFFFFFFFFu / (uint32_t)d + 1u : 0u; }
__device__ __forceinline__ int lr_div_recip(int n, int d, uint32_t inv) {
  if (d == 1) return n;
  uint32_t q = __umulhi((uint32_t)n, inv);
  if (q * (uint32_t)d > (uint32_t)n) --q;
  return (int)q;
}

// ------------------------------------------------------------------------------------------------------------ wgrad
// grid: (k' tiles of 64 over T*Ci4, tap-major) x (co tiles of 64) x (S * mchunks): one sample and one chunk of the reduction axis
// M = B*Ho*Wo (rows [c * mchunk, (c + 1) * mchunk)) per workgroup; the tile goes to the natural element (co, ci, tap).
__global__ __launch_bounds__(256) void lr_wgrad_kernel(const LrBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float As[kBK][kLS];   // [mm][co]: g
  __shared__ __attribute__((aligned(16))) float Bs[kBK][kLS];   // [mm][k']: x window
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  const int s = blockIdx.z / a.mchunks, c = blockIdx.z - s * a.mchunks;
  const int co0 = blockIdx.y * 64, k0 = blockIdx.x * 64;
  const int KP = a.T * a.Ci4, HW = a.H * a.W, HoWo = a.Ho * a.Wo, M = a.B * HoWo;
  // this thread's staging columns: col = tid & 63 (a co for A, a k' for B), mm = (tid >> 6) + 4 j
  const int scol = tid & 63;
  const int kp = k0 + scol, tap = kp < KP ? kp / a.Ci4 : 0, kci = kp - tap * a.Ci4;
  const bool kok = kp < KP && kci < a.Ci;
  const int kh = tap / a.KW, kwi = tap - kh * a.KW;
  const int aco = co0 + scol;
  const bool cok = aco < a.Co;
  const uint32_t inv_howo = lr_recip32(HoWo), inv_wo = lr_recip32(a.Wo);
  const int mlo = c * a.mchunk, mhi = mlo + a.mchunk < M ? mlo + a.mchunk : M;
  const float* const gs = a.g + (long long)s * a.out_elems;
  const float* const xs = a.x + (long long)s * a.x_sample_stride;
  f32x16 d;
#pragma unroll
  for (int r = 0; r < 16; ++r) d[r] = 0.f;
  for (int mm0 = mlo; mm0 < mhi; mm0 += kBK) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int mm = (tid >> 6) + 4 * j, m = mm0 + mm;
      const bool mok = m < mhi;
      const int b = mok ? lr_div_recip(m, HoWo, inv_howo) : 0, p = mok ? m - b * HoWo : 0, ho = lr_div_recip(p, a.Wo, inv_wo), wo = p - ho * a.Wo;
      float ga = 0.f, xv = 0.f;
      if (mok && cok) ga = gs[((long long)b * a.Co + aco) * HoWo + p];
      const int hi = ho * a.SH - a.PH + kh * a.DH, wi = wo * a.SW - a.PW + kwi * a.DW;
      if (mok && kok && (unsigned)hi < (unsigned)a.H && (unsigned)wi < (unsigned)a.W) xv = xs[((long long)b * a.Ci + kci) * HW + (long long)hi * a.W + wi];
      As[mm][scol] = ga, Bs[mm][scol] = xv;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kBK / 2; ++q) d = __builtin_amdgcn_mfma_f32_32x32x2f32(As[2 * q + lh][wr + li], Bs[2 * q + lh][wc + li], d, 0, 0, 0);
  }
  // D[row = co][col = k']: lane holds column wc + li, registers hold rows (r&3) + 8 (r>>2) + 4 lh
  const int kpl = k0 + wc + li, ltap = kpl < KP ? kpl / a.Ci4 : 0, lci = kpl - ltap * a.Ci4;
  if (kpl < KP && lci < a.Ci) {
    float* const dst = a.mchunks > 1 ? a.part_w + ((long long)s * a.mchunks + c) * a.w_elems : a.dw + (long long)s * a.w_elems;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wr + (r & 3) + 8 * (r >> 2) + 4 * lh;
      if (co < a.Co) dst[((long long)co * a.Ci + lci) * a.T + ltap] = d[r];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ the chain rule
// One thread per output of the n x (1 + r) parameter gradients (column 0: dmu, column 1 + j: dL[.][j]); s ascending, one rounding per
// operation. z_s[j]: read, or normal j & 3 of Philox block j >> 2 of tensor 4 (bt_rng_normal_fill's z stream).
__global__ __launch_bounds__(256) void lr_finish_kernel(const float* __restrict__ dw, long long n, int r, int S, const float* __restrict__ z, RngKey kz,
                                                        const uint32_t* call_base, uint32_t sample0, float* __restrict__ dmu, float* __restrict__ dL) {
  if (call_base) kz.call += *call_base;
  const long long total = n * (long long)(r + 1);
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long i = idx / (r + 1);
    const int jj = (int)(idx - i * (r + 1));
    float acc = 0.f;
    if (jj == 0) {
      if (!dmu) continue;
      for (int s = 0; s < S; ++s) acc = __fadd_rn(acc, dw[(long long)s * n + i]);
      dmu[i] = acc;
    } else {
      if (!dL) continue;
      const int j = jj - 1;
      for (int s = 0; s < S; ++s) {
        float zj;
        if (z) {
          zj = z[(long long)s * r + j];
        } else {
          float v[4];
          philox_normal4(kz, sample0 + (uint32_t)s, (uint32_t)(j >> 2), v);
          const int sel = j & 3;
          zj = sel == 0 ? v[0] : sel == 1 ? v[1] : sel == 2 ? v[2] : v[3];
        }
        acc = __fadd_rn(acc, __fmul_rn(dw[(long long)s * n + i], zj));
      }
      dL[i * r + j] = acc;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------ KL gradient
// With A = I + L^T L / d = C C^T (bt_lowrank.hip keeps the factor C in A's lower triangle):  (d I + L^T L)^-1 = (1 / d) C^-T C^-1.
// Column j of C^-1 by forward substitution, one wave per column, the column kept in LDS (r doubles):
//   Cinv[j][j] = 1 / C[j][j],   Cinv[i][j] = -(sum_{j <= k < i} C[i][k] Cinv[k][j]) / C[i][i]   for i > j;
// the lanes split the sum (k = j + lane, + 64, ...: coalesced reads of C's row), their partials are added in lane order through LDS.
// One thread per column ran the r = 432 inverse in ~5 ms: r^2 / 2 dependent steps per thread, each a global load. Only the lower
// triangle is written, and only it is read afterwards.
__global__ __launch_bounds__(64) void kl_lr_inv_factor_kernel(const double* __restrict__ Cf, int r, double* __restrict__ Cinv) {
  extern __shared__ double ycol[];   // [r]: entries j .. i - 1 of this column
  __shared__ double red[64];
  const int j = blockIdx.x, lane = threadIdx.x;
  for (int i = j; i < r; ++i) {
    const double* const row = Cf + (long long)i * r;
    double acc = 0.0;
    for (int k = j + lane; k < i; k += 64) acc += row[k] * ycol[k];
    red[lane] = acc;
    __syncthreads();
    if (lane == 0) {
      double t = 0.0;
      const int used = i - j < 64 ? i - j : 64;
      for (int q = 0; q < used; ++q) t += red[q];
      const double y = i == j ? 1.0 / row[j] : -t / row[i];
      ycol[i] = y;
      Cinv[(long long)i * r + j] = y;
    }
    __syncthreads();
  }
}

// Minv[a][b] = (1 / d) sum_{k >= max(a, b)} Cinv[k][a] Cinv[k][b]: the explicit r x r inverse of d I + L^T L, one thread per entry.
__global__ __launch_bounds__(256) void kl_lr_inv_kernel(const double* __restrict__ Cinv, int r, double d, double* __restrict__ Minv) {
  const long long rr = (long long)r * r;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < rr; idx += (long long)gridDim.x * 256) {
    const int a = (int)(idx / r), b = (int)(idx - (long long)a * r);
    double acc = 0.0;
    for (int k = a > b ? a : b; k < r; ++k) acc += Cinv[(long long)k * r + a] * Cinv[(long long)k * r + b];
    Minv[idx] = acc / d;
  }
}

// dmu[i] = c (mu_i - m_i) / P_i,  dL[i][j] = c (L_ij / P_i - sum_k L_ik Minv[k][j]),  c = grad_kl[0]; fp64, rounded once to fp32.
// status[0] != 1 (a pivot of the factorisation was not positive): NaN everywhere.
__global__ __launch_bounds__(256) void kl_lr_grad_kernel(const float* __restrict__ mu, const float* __restrict__ L, const float* __restrict__ pm,
                                                         const float* __restrict__ pv, long long n, int r, const double* __restrict__ Minv,
                                                         const double* __restrict__ status, const float* __restrict__ grad_kl, float* __restrict__ dmu,
                                                         float* __restrict__ dL) {
  const bool ok = status[0] == 1.0;
  const double c = (double)grad_kl[0];
  const long long total = n * (long long)r;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long i = idx / r;
    const int j = (int)(idx - i * r);
    const double P = (double)pv[i];
    if (j == 0 && dmu) dmu[i] = ok ? (float)(c * ((double)mu[i] - (double)pm[i]) / P) : NAN;
    if (dL) {
      const float* const row = L + i * r;
      double acc = 0.0;
      for (int k = 0; k < r; ++k) acc += (double)row[k] * Minv[(long long)k * r + j];
      dL[idx] = ok ? (float)(c * ((double)row[j] / P - acc)) : NAN;
    }
  }
}

// Plan-only digest of the argument block: what it means, not its bytes. Pointers, then every scalar, in this order.
uint64_t digest_arg(uint64_t h, const LrBwdArgs& a) {
  for (const void* p : std::initializer_list<const void*>{a.x, a.g, a.mean, a.L, a.z, a.eps_w, a.dx, a.dw, a.part_w, a.part_d, a.call_base}) h = digest_arg(h, p);
  for (long long v : {a.x_sample_stride, a.mean_stride, a.x_elems, a.out_elems, a.w_elems}) h = digest_arg(h, v);
  for (int v : {a.B, a.Ci, a.H, a.W, a.Co, a.KH, a.KW, a.SH, a.SW, a.PH, a.PW, a.DH, a.DW, a.Ho, a.Wo, a.Ci4, a.T, a.S, a.R, a.dchunks, a.dchunk, a.mchunks, a.mchunk})
    h = digest_arg(h, v);
  h = digest_arg(h, a.sd);
  for (uint32_t v : {a.seed_lo, a.seed_hi, a.call, a.layer_id, a.sample0}) h = digest_arg(h, v);
  return h;
}

// bt_lowrank.hip
int kl_lowrank_factor(const char* who_sweep, const char* who_finish, const float* mu, const float* L, long long n, int r, float d, const float* prior_mean,
                      const float* prior_var, float* kl_out, int32_t* bad_pivots, double* part, double* A, bool keep, double* status, hipStream_t stream);
long long kl_lowrank_partials(long long n, int r);

constexpr int kLrMaxRank = 4096;   // bt_kl_lowrank's limit
static thread_local int64_t g_lr_info[10] = {};

static unsigned capped_blocks(long long items) {
  const long long b = (items + 255) / 256;
  return (unsigned)(b > 65535 ? 65535 : (b < 1 ? 1 : b));
}

// The two slabs of partials of a plan: wgrad's [S][mchunks][n] (more than one chunk), then dgrad's [dchunks][S][x_elems] (more than one piece).
struct LrSlabs {
  int mchunks;
  size_t w_bytes, d_bytes;
};
static LrSlabs lr_slabs(const BwdPlan& pl, int S) {
  LrSlabs s;
  s.mchunks = pl.groups / pl.sgroups;
  s.w_bytes = s.mchunks > 1 ? (size_t)S * s.mchunks * (size_t)pl.w_elems * sizeof(float) : 0;
  s.d_bytes = pl.dchunks > 1 ? (size_t)pl.dchunks * S * (size_t)pl.x_elems * sizeof(float) : 0;
  return s;
}

}  // namespace bt

extern "C" size_t bt_lowrank_conv2d_bwd_workspace(const bt_conv2d_geom* g, int32_t S, int32_t r) {
  using namespace bt;
  BwdPlan pl;
  if (!g || r < 0 || r > kLrMaxRank || bwd_plan(*g, S, true, true, &pl) != kBwdOk || g->groups != 1) return 0;
  const LrSlabs sl = lr_slabs(pl, S);
  // (a rank above the in-kernel bound: the [S][n] slab of the caller's recomputed pre-pass, behind the partials)
  const size_t mean_bytes = r > BT_LOWRANK_MAX_R ? (size_t)S * (size_t)pl.w_elems * sizeof(float) : 0;
  const size_t parts = (sl.w_bytes + sl.d_bytes + 15) & ~(size_t)15;
  return (parts < 16 ? 16 : parts) + mean_bytes;
}

extern "C" int bt_lowrank_conv2d_bwd(const bt_conv2d_geom* g, int32_t S, const float* x, int64_t x_sample_stride, const float* grad_out, const float* mean,
                                     int64_t mean_sample_stride, const float* L, int32_t R, float sd, const float* z, const bt_rng* rng, const float* eps_w, float* dx,
                                     float* dW_per_sample, void* workspace, size_t workspace_bytes, bt_stream_t stream) {
  using namespace bt;
  char msg[256];
  auto fail = [&](int code, const char* what) {
    snprintf(msg, sizeof(msg), "bt_lowrank_conv2d_bwd: %s", what);
    return set_error(code, msg);
  };
  if (!g) return fail(BT_ERR_BAD_ARG, "null geometry");
  if (!x || !grad_out) return fail(BT_ERR_BAD_ARG, "null argument");
  if (!dx && !dW_per_sample) return fail(BT_ERR_BAD_ARG, "neither dx nor dW_per_sample is wanted");
  if (const char* ge = geom_error(*g)) return fail(BT_ERR_BAD_ARG, ge);
  if (g->groups != 1) return fail(BT_ERR_BAD_ARG, "groups must be 1");
  if (S <= 0 || x_sample_stride < 0 || mean_sample_stride < 0) return fail(BT_ERR_BAD_ARG, "bad S / sample stride");
  if (dx) {   // the data gradient regenerates W_s
    if (!mean) return fail(BT_ERR_BAD_ARG, "dx needs mean");
    if (R < 0 || R > BT_LOWRANK_MAX_R) return fail(BT_ERR_BAD_ARG, "R must be in [0, BT_LOWRANK_MAX_R] (above: the bt_lowrank_mean pre-pass and R = 0)");
    if (R > 0 && !L) return fail(BT_ERR_BAD_ARG, "R > 0 needs L");
    if (!(sd > 0.f && sd <= FLT_MAX)) return fail(BT_ERR_BAD_ARG, "sd must be positive and finite");
    if (!eps_w && !rng) return fail(BT_ERR_BAD_ARG, "neither draws nor rng");
    if ((eps_w && R > 0 && !z) || (!eps_w && z)) return fail(BT_ERR_BAD_ARG, "supply both draws (z, eps_w) or neither");
  }
  BwdPlan pl;
  const int refused = bwd_plan(*g, S, dx != nullptr, dW_per_sample != nullptr, &pl);
  if (refused == kBwdBadGeometry) return fail(BT_ERR_BAD_ARG, "bad geometry");
  if (refused == kBwdEmptyOutput) return fail(BT_ERR_BAD_ARG, "empty output");
  if (refused == kBwdTooLarge) return fail(BT_ERR_UNSUPPORTED, "tensor too large for the 32-bit draw indices");
  const LrSlabs sl = lr_slabs(pl, S);
  const long long wz = (long long)S * sl.mchunks;
  if (wz > 65535 || pl.dgrid[2] > 65535u || pl.dgrid[1] > 65535u || pl.wgrid[1] > 65535u) return fail(BT_ERR_UNSUPPORTED, "too many samples x pieces for one grid");
  const bool need_ws = (dx && pl.dchunks > 1) || (dW_per_sample && sl.mchunks > 1);
  if (need_ws && (!workspace || (((uintptr_t)workspace) & 7u) || workspace_bytes < sl.w_bytes + sl.d_bytes)) {
    snprintf(msg, sizeof(msg), "bt_lowrank_conv2d_bwd: workspace smaller than bt_lowrank_conv2d_bwd_workspace(), or not 8-byte aligned");
    return set_error(BT_ERR_WORKSPACE, msg);
  }
  bt_rng none = {};
  const bt_rng& rg = rng ? *rng : none;
  LrBwdArgs a = {};
  a.x = x, a.g = grad_out, a.mean = mean, a.L = R > 0 ? L : nullptr, a.z = (eps_w && R > 0) ? z : nullptr, a.eps_w = eps_w;
  a.dx = dx, a.dw = dW_per_sample;
  a.part_w = reinterpret_cast<float*>(workspace);
  a.part_d = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + sl.w_bytes);
  a.call_base = rg.call_base_dev;
  a.x_sample_stride = x_sample_stride, a.mean_stride = mean_sample_stride, a.x_elems = pl.x_elems, a.out_elems = pl.out_elems, a.w_elems = pl.w_elems;
  a.B = g->B, a.Ci = g->Ci, a.H = g->H, a.W = g->W, a.Co = g->Co, a.KH = g->kh, a.KW = g->kw;
  a.SH = g->sh, a.SW = g->sw, a.PH = g->ph, a.PW = g->pw, a.DH = g->dh, a.DW = g->dw;
  a.Ho = pl.Ho, a.Wo = pl.Wo, a.Ci4 = pl.Cig4, a.T = pl.T, a.S = S, a.R = dx ? R : 0;
  a.dchunks = pl.dchunks, a.dchunk = pl.dchunk, a.mchunks = sl.mchunks, a.mchunk = pl.mchunk;
  a.sd = sd;
  a.seed_lo = (uint32_t)rg.seed, a.seed_hi = (uint32_t)(rg.seed >> 32), a.call = rg.call, a.layer_id = rg.layer_id, a.sample0 = rg.sample0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 dgrid(pl.dgrid[0], pl.dgrid[1], pl.dgrid[2]), wgrid(pl.wgrid[0], pl.wgrid[1], (unsigned)wz), block(256);
  int64_t info[10] = {0, 0, pl.dchunks, sl.mchunks, dgrid.x, dgrid.y, dgrid.z, wgrid.x, wgrid.y, wgrid.z};
  if (dx) {
    if (int rc = launch_kernel(lr_dgrad_kernel, nullptr, "bt_lowrank_conv2d_bwd (dgrad)", dgrid, block, 0, 0, st, a)) return rc;
    ++info[0];
    if (pl.dchunks > 1) {
      const long long total = (long long)S * pl.x_elems;
      if (int rc = launch_kernel(lr_sum_pieces_kernel, nullptr, "bt_lowrank_conv2d_bwd (dgrad finish)", dim3(capped_blocks(total)), block, 0, 0, st, (const float*)a.part_d,
                                 pl.dchunks, total, total, 0ll, total, dx))
        return rc;
      ++info[0];
    }
  }
  if (dW_per_sample) {
    if (int rc = launch_kernel(lr_wgrad_kernel, nullptr, "bt_lowrank_conv2d_bwd (wgrad)", wgrid, block, 0, 0, st, a)) return rc;
    ++info[1];
    if (sl.mchunks > 1) {
      const long long n = pl.w_elems, total = (long long)S * n;
      if (int rc = launch_kernel(lr_sum_pieces_kernel, nullptr, "bt_lowrank_conv2d_bwd (wgrad finish)", dim3(capped_blocks(total)), block, 0, 0, st, (const float*)a.part_w,
                                 sl.mchunks, n, n, (long long)sl.mchunks * n, total, dW_per_sample))
        return rc;
      ++info[1];
    }
  }
  memcpy(g_lr_info, info, sizeof(info));
  return BT_OK;
}

extern "C" int bt_lowrank_conv2d_bwd_info(int64_t* out, int32_t n) {
  if (!out || n <= 0) return bt::set_error(BT_ERR_BAD_ARG, "bt_lowrank_conv2d_bwd_info: bad argument");
  for (int i = 0; i < n && i < 10; ++i) out[i] = bt::g_lr_info[i];
  return BT_OK;
}

extern "C" int bt_lowrank_wgrad_finish(const float* dW_per_sample, int64_t n, int32_t r, int32_t S, const float* z, const bt_rng* rng, float* dmu, float* dL,
                                       bt_stream_t stream) {
  using namespace bt;
  if (!dW_per_sample || n <= 0 || r <= 0 || S <= 0 || (!dmu && !dL) || (dL && !z && !rng)) return set_error(BT_ERR_BAD_ARG, "bt_lowrank_wgrad_finish: bad argument");
  if (r > kLrMaxRank || n >= (1ll << 31) || (long long)n * r >= (1ll << 40)) return set_error(BT_ERR_UNSUPPORTED, "bt_lowrank_wgrad_finish: rank above 4096 or L too large");
  bt_rng none = {};
  const bt_rng& rg = rng ? *rng : none;
  return launch_kernel(lr_finish_kernel, nullptr, "bt_lowrank_wgrad_finish", dim3(capped_blocks((long long)n * (r + 1))), dim3(256), 0, 0, (hipStream_t)stream, dW_per_sample,
                       (long long)n, (int)r, (int)S, z, make_key(rg, 4), rg.call_base_dev, rg.sample0, dmu, dL);
}

extern "C" size_t bt_kl_lowrank_bwd_workspace(int64_t n, int32_t r) {
  if (n <= 0 || r <= 0 || r > bt::kLrMaxRank) return 0;
  return (size_t)((bt::kl_lowrank_partials(n, r) + 3ll * r * r + 1) * 8);   // partials | A -> C | Cinv | Minv | status
}

extern "C" int bt_kl_lowrank_bwd(const float* mu, const float* L, int64_t n, int32_t r, float d, const float* prior_mean, const float* prior_var, const float* grad_kl,
                                 float* dmu, float* dL, int32_t* bad_pivots, void* workspace, size_t workspace_bytes, bt_stream_t stream) {
  using namespace bt;
  if (!mu || !L || !prior_mean || !prior_var || !grad_kl || (!dmu && !dL) || n <= 0 || r <= 0 || !(d > 0.f)) return set_error(BT_ERR_BAD_ARG, "bt_kl_lowrank_bwd: bad argument");
  if (r > kLrMaxRank || (long long)n * r >= (1ll << 40)) return set_error(BT_ERR_UNSUPPORTED, "bt_kl_lowrank_bwd: rank above 4096 or L too large");
  if (!workspace || (((uintptr_t)workspace) & 7u) || workspace_bytes < bt_kl_lowrank_bwd_workspace(n, r))
    return set_error(BT_ERR_WORKSPACE, "bt_kl_lowrank_bwd: workspace smaller than bt_kl_lowrank_bwd_workspace(n, r), or not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long long rr = (long long)r * r;
  double* const part = reinterpret_cast<double*>(workspace);
  double* const A = part + kl_lowrank_partials(n, r);
  double* const Cinv = A + rr;
  double* const Minv = Cinv + rr;
  double* const status = Minv + rr;
  if (int rc = kl_lowrank_factor("bt_kl_lowrank_bwd (sweep)", "bt_kl_lowrank_bwd (factor)", mu, L, (long long)n, (int)r, d, prior_mean, prior_var, nullptr, bad_pivots, part, A,
                                 true, status, st))
    return rc;
  if (int rc = launch_kernel(kl_lr_inv_factor_kernel, nullptr, "bt_kl_lowrank_bwd (factor inverse)", dim3((unsigned)r), dim3(64), r * (int)sizeof(double), 0, st,
                             (const double*)A, (int)r, Cinv))
    return rc;
  if (int rc = launch_kernel(kl_lr_inv_kernel, nullptr, "bt_kl_lowrank_bwd (inverse)", dim3(capped_blocks(rr)), dim3(256), 0, 0, st, (const double*)Cinv, (int)r, (double)d, Minv))
    return rc;
  return launch_kernel(kl_lr_grad_kernel, nullptr, "bt_kl_lowrank_bwd (gradient)", dim3(capped_blocks((long long)n * r)), dim3(256), 0, 0, st, mu, L, prior_mean, prior_var,
                       (long long)n, (int)r, (const double*)Minv, (const double*)status, grad_kl, dmu, dL);
}
