// The low-rank multivariate layer's two side kernels (layers/_lowrank.py; the forward itself is fused_fwd_kernel's LOWRANK form):
//   bt_lowrank_mean  m[s][i] = mu[i] + sum_j L[i][j] * z_s[j] for ranks above the forward kernel's in-kernel bound (BT_LOWRANK_MAX_R);
//   bt_kl_lowrank    KL(N(mu, L L^T + d I) || N(m, diag(P))) in closed form, fp64: a sweep over the weight index and an r x r Cholesky.
// Replaces, in reference layers/variational_layers/conv_variational.py:516-552, LowRankMultivariateNormal.rsample's batched matmul and
// kl_divergence's two Cholesky factorisations per forward.
#include <math.h>

#include "bt_api_internal.h"

namespace bt {

// ---------------------------------------------------------------------------- mean pre-pass
constexpr int kLrThreads = 64;
constexpr int kLrSC = 8;     // samples per workgroup: one accumulator register each
constexpr int kLrJT = 128;   // columns of L per staged z tile (kLrSC * kLrJT floats of LDS = 4 KiB); a multiple of 4

// One thread per weight element i, blockIdx.y per group of kLrSC samples. z is staged tile by tile in LDS (generated from tensor 4 of the
// call's draw streams -- element j of sample s is normal j & 3 of Philox block j >> 2 -- or read); the thread reads its row of L once
// per sample group and extends kLrSC chains  acc = acc + L[i][j] * z_s[j]  (j ascending, two roundings per step: the chain the forward
// kernel's LOWRANK form runs in registers). Small workgroups and sample groups: the layers that come here are small (the 432-weight
// stem), and one wave per 64 weights x 8 samples spreads them over the chip; a row of L is fetched from HBM once and re-read from L2 by
// the other sample groups (256 threads x 32 samples ran the stem's S = 32 on two CUs in 573 us).
__global__ __launch_bounds__(kLrThreads) void lowrank_mean_kernel(const float* __restrict__ mu, const float* __restrict__ L, long long n, int r, int S,
                                                                  const float* __restrict__ z, RngKey kz, const uint32_t* call_base, uint32_t sample0,
                                                                  float* __restrict__ m) {
  __shared__ float zt[kLrSC * kLrJT];
  if (call_base) kz.call += *call_base;
  const int tid = threadIdx.x;
  const int s0 = blockIdx.y * kLrSC;
  const int sc = (S - s0) < kLrSC ? (S - s0) : kLrSC;
  const long long i = (long long)blockIdx.x * kLrThreads + tid;
  const bool live = i < n;
  const float m0 = live ? mu[i] : 0.f;
  float acc[kLrSC];
#pragma unroll
  for (int s = 0; s < kLrSC; ++s) acc[s] = m0;
  const float* const Lrow = L + (live ? i : 0) * (long long)r;
  for (int j0 = 0; j0 < r; j0 += kLrJT) {
    const int jt = (r - j0) < kLrJT ? (r - j0) : kLrJT;
    __syncthreads();   // the previous tile has been consumed
    if (z) {
      for (int e = tid; e < sc * kLrJT; e += kLrThreads) {
        const int s = e / kLrJT, j = e - s * kLrJT;
        zt[e] = j < jt ? z[(long long)(s0 + s) * r + j0 + j] : 0.f;
      }
    } else {
      for (int q = tid; q < sc * (kLrJT / 4); q += kLrThreads) {
        const int s = q / (kLrJT / 4), jq = q - s * (kLrJT / 4);
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (4 * jq < jt) philox_normal4(kz, sample0 + (uint32_t)(s0 + s), (uint32_t)((j0 >> 2) + jq), v);
#pragma unroll
        for (int e = 0; e < 4; ++e) zt[s * kLrJT + 4 * jq + e] = v[e];
      }
    }
    __syncthreads();
    for (int jb = 0; jb < jt; jb += 8) {   // eight loads of the row in flight, then their 8 x sc chain steps in j order
      float l[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) l[u] = Lrow[j0 + (jb + u < jt ? jb + u : jt - 1)];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (jb + u < jt) {
#pragma unroll
          for (int s = 0; s < kLrSC; ++s)
            if (s < sc) acc[s] = __fadd_rn(acc[s], __fmul_rn(l[u], zt[s * kLrJT + jb + u]));
        }
      }
    }
  }
  if (live) {
#pragma unroll
    for (int s = 0; s < kLrSC; ++s)
      if (s < sc) m[(long long)(s0 + s) * n + i] = acc[s];
  }
}

// ---------------------------------------------------------------------------- KL
// Partials of one chunk of the weight index: [r * r] entries of G = L^T diag(1 / d) L (lower triangle, row-major) + 4 scalars.
constexpr int kKlLrScalars = 4;   // sum log P, sum_i sum_j L_ij^2 / P_i, sum d / P, sum (mu - m)^2 / P
constexpr int kKlLrMaxRank = 4096;   // the factorisation keeps a panel of at least one column (r doubles) in LDS
constexpr long long kKlLrMaxPartials = 1ll << 20;   // doubles of partials per call (8 MiB): bounds the chunk count of a high rank

struct KlLrPlan {
  int T, nt, C;
  long long chunk, stride;   // weight indices per chunk; doubles per chunk's partials
};

// T x T entries of G per workgroup; the 256 / T^2 lanes left over run along the weight index. Chunks: >= 64 indices per lane.
static KlLrPlan kl_lowrank_plan(long long n, int r) {
  KlLrPlan p;
  p.T = r > 4 ? 16 : 4;
  p.nt = (r + p.T - 1) / p.T;
  p.stride = (long long)r * r + kKlLrScalars;
  const int IL = 256 / (p.T * p.T);
  long long C = (n + 64ll * IL - 1) / (64ll * IL);
  const long long cap = kKlLrMaxPartials / p.stride;
  if (C > cap) C = cap;
  if (C > 256) C = 256;
  if (C < 1) C = 1;
  p.chunk = (n + C - 1) / C;
  p.C = (int)((n + p.chunk - 1) / p.chunk);
  return p;
}

template <int T>
__global__ __launch_bounds__(256) void kl_lowrank_sweep_kernel(const float* __restrict__ mu, const float* __restrict__ L, const float* __restrict__ pm,
                                                               const float* __restrict__ pv, long long n, int r, double d, int nt, long long chunk,
                                                               long long stride, double* __restrict__ part) {
  constexpr int TT = T * T, IL = 256 / TT;
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const long long lo = (long long)blockIdx.y * chunk;
  const long long hi = (lo + chunk < n) ? lo + chunk : n;
  double* const out = part + (long long)blockIdx.y * stride;
  if ((int)blockIdx.x == nt * nt) {   // the scalars of this chunk: lanes along the weight index, fixed-order block sums
    double s[kKlLrScalars] = {0.0, 0.0, 0.0, 0.0};
    for (long long i = lo + tid; i < hi; i += 256) {
      const double P = (double)pv[i], dm = (double)mu[i] - (double)pm[i];
      double l2 = 0.0;
      for (int j = 0; j < r; ++j) {
        const double l = (double)L[i * r + j];
        l2 += l * l;
      }
      s[0] += log(P), s[1] += l2 / P, s[2] += d / P, s[3] += dm * dm / P;
    }
    for (int q = 0; q < kKlLrScalars; ++q) {
      const double t = block_sum_256(s[q], red);
      if (tid == 0) out[(long long)r * r + q] = t;
      __syncthreads();   // (red is free again)
    }
    return;
  }
  const int ta = blockIdx.x / nt, tb = blockIdx.x - ta * nt;
  if (tb > ta) return;   // the lower triangle only (the whole workgroup leaves)
  const int il = tid / TT, e = tid - il * TT;
  const int a = ta * T + e / T, b = tb * T + e % T;
  const bool valid = a < r && b <= a;
  double acc = 0.0;
  if (valid)
    for (long long i = lo + il; i < hi; i += IL) acc += (double)L[i * r + a] * (double)L[i * r + b];
  red[tid] = acc;
  __syncthreads();
  if (il == 0 && valid) {
    double t = 0.0;
    for (int q = 0; q < IL; ++q) t += red[q * TT + e];   // lanes in index order
    out[(long long)a * r + b] = t / d;
  }
}

// One workgroup: A = I + sum over the chunks (in chunk order) of the partials of G, then an fp64 Cholesky of A's lower triangle in global
// memory, blocked by panels of nb columns that live in LDS: a panel's columns are factorised left-looking (column k takes the updates of
// the panel's earlier columns from LDS, its pivot is logged, the rest is scaled), then the trailing matrix takes the panel's rank-nb update
// in one pass -- one read and one write of a trailing element per panel instead of per column. Only the pivots are kept:
// logdet = sum log pivot, and the closed form
//   KL = 1/2 [ sum log P - n log d - logdet + sum (d + sum_j L_ij^2) / P + sum (mu - m)^2 / P - n ]   -> kl[0], kl[1] = KL / n.
// A pivot that is not positive: NaN in both, and one more in *bad (when given).
// KEEP (bt_kl_lowrank_bwd): the factor C (A = C C^T) is left in A's lower triangle, kl may be null, and *status says whether every
// pivot was positive (1.0) or not (NaN).
constexpr int kFinThreads = 1024;
constexpr int kFinPanelDoubles = 8192;   // LDS doubles of one panel (64 KiB): nb = min(16, 8192 / r) columns, >= 1 up to the rank limit
static_assert(kFinPanelDoubles >= kKlLrMaxRank, "a panel holds at least one column");
template <bool KEEP>
__global__ __launch_bounds__(kFinThreads) void kl_lowrank_finish_kernel(const double* __restrict__ part, int C, long long stride, long long n, int r, int NB, double d,
                                                                        double* A, float* kl, int* bad, double* status) {
  extern __shared__ double pan[];   // [NB][r]: column p of the panel at pan + p * r (rows below the panel's first are used)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long rr = (long long)r * r;
  for (long long idx = tid; idx < rr; idx += kFinThreads) {
    const int a = (int)(idx / r), b = (int)(idx - (long long)a * r);
    if (b > a) continue;
    double t = 0.0;
    for (int c = 0; c < C; ++c) t += part[(long long)c * stride + idx];
    A[idx] = t + (a == b ? 1.0 : 0.0);
  }
  double sc[kKlLrScalars] = {0.0, 0.0, 0.0, 0.0};
  if (tid == 0)
    for (int q = 0; q < kKlLrScalars; ++q)
      for (int c = 0; c < C; ++c) sc[q] += part[(long long)c * stride + rr + q];
  __syncthreads();
  double logdet = 0.0;
  bool neg = false;
  for (int k0 = 0; k0 < r; k0 += NB) {
    const int nb = (r - k0) < NB ? (r - k0) : NB;
    // the panel's rows from k0 into LDS in one coalesced pass (entries above the diagonal are never read)
    for (int e = tid; e < (r - k0) * nb; e += kFinThreads) {
      const int i = k0 + e / nb, p = e - (e / nb) * nb;
      pan[(long long)p * r + i] = A[(long long)i * r + k0 + p];
    }
    __syncthreads();
    for (int p = 0; p < nb; ++p) {
      const int k = k0 + p;
      double* const cp = pan + (long long)p * r;
      for (int i = k + tid; i < r; i += kFinThreads) {   // column k below (and at) the diagonal, less the panel's earlier columns
        double v = cp[i];
        for (int q = 0; q < p; ++q) v -= pan[(long long)q * r + i] * pan[(long long)q * r + k];
        cp[i] = v;
      }
      __syncthreads();
      const double piv = cp[k];   // stays unscaled: no later step reads a column's own diagonal entry
      if (tid == 0) {
        neg = neg || !(piv > 0.0);
        logdet += log(piv);
      }
      const double inv = 1.0 / sqrt(piv);
      for (int i = k + 1 + tid; i < r; i += kFinThreads) cp[i] *= inv;
      __syncthreads();
    }
    if constexpr (KEEP) {   // the panel's columns of the factor, diagonal included (the trailing update below touches later columns only)
      for (int e = tid; e < (r - k0) * nb; e += kFinThreads) {
        const int i = k0 + e / nb, p = e - (e / nb) * nb;
        if (i >= k0 + p) A[(long long)i * r + k0 + p] = i == k0 + p ? sqrt(pan[(long long)p * r + i]) : pan[(long long)p * r + i];
      }
    }
    const int t0 = k0 + nb;   // trailing matrix: rows and columns from t0
    // (a wave takes four rows at a time: one LDS read of the panel's column entry serves four multiply-adds, and the rows' own
    // entries are wave-uniform reads -- the update is LDS-bound: one row at a time ran the r = 432 call in 1577 us)
    for (int i0 = t0 + 4 * wv; i0 < r; i0 += 4 * (kFinThreads / 64)) {
      const int ilast = (i0 + 3 < r) ? i0 + 3 : r - 1;
      for (int j = t0 + lane; j <= ilast; j += 64) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (i0 + u <= ilast && j <= i0 + u) ? A[(long long)(i0 + u) * r + j] : 0.0;
        for (int q = 0; q < nb; ++q) {
          const double pj = pan[(long long)q * r + j];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] -= pan[(long long)q * r + (i0 + u <= ilast ? i0 + u : ilast)] * pj;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (i0 + u <= ilast && j <= i0 + u) A[(long long)(i0 + u) * r + j] = v[u];
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    double v = 0.5 * (sc[0] - (double)n * log(d) - logdet + sc[1] + sc[2] + sc[3] - (double)n);
    if (neg) {
      v = (double)NAN;
      if (bad) *bad += 1;
    }
    if (kl) {
      kl[0] = (float)v;
      kl[1] = (float)(v / (double)n);
    }
    if constexpr (KEEP) *status = neg ? (double)NAN : 1.0;
  }
}

// The sweep and the factorisation: bt_kl_lowrank's two launches (keep = false), and the first two of bt_kl_lowrank_bwd's.
int kl_lowrank_factor(const char* who_sweep, const char* who_finish, const float* mu, const float* L, long long n, int r, float d, const float* prior_mean,
                      const float* prior_var, float* kl_out, int32_t* bad_pivots, double* part, double* A, bool keep, double* status, hipStream_t stream) {
  const KlLrPlan p = kl_lowrank_plan(n, r);
  const dim3 grid((unsigned)(p.nt * p.nt + 1), (unsigned)p.C);
  if (int rc = launch_kernel(p.T == 16 ? kl_lowrank_sweep_kernel<16> : kl_lowrank_sweep_kernel<4>, nullptr, who_sweep, grid, dim3(256), 0, 0, stream, mu, L, prior_mean,
                             prior_var, n, r, (double)d, p.nt, p.chunk, p.stride, part))
    return rc;
  int NB = kFinPanelDoubles / r;
  NB = NB > 16 ? 16 : NB;
  const int lds = NB * r * (int)sizeof(double);   // <= 64 KiB
  return launch_kernel(keep ? kl_lowrank_finish_kernel<true> : kl_lowrank_finish_kernel<false>, nullptr, who_finish, dim3(1), dim3(kFinThreads), lds,
                       kFinPanelDoubles * (int)sizeof(double), stream, part, p.C, p.stride, n, r, NB, (double)d, A, kl_out, bad_pivots, status);
}

long long kl_lowrank_partials(long long n, int r) {   // doubles of the sweep's partials (A begins behind them)
  const KlLrPlan p = kl_lowrank_plan(n, r);
  return (long long)p.C * p.stride;
}

}  // namespace bt

extern "C" int bt_lowrank_mean(const float* mu, const float* L, int64_t n, int32_t r, int32_t S, const float* z, const bt_rng* rng, float* m, bt_stream_t stream) {
  using namespace bt;
  if (!mu || !L || !m || n <= 0 || r <= 0 || S <= 0 || (!z && !rng)) return set_error(BT_ERR_BAD_ARG, "bt_lowrank_mean: bad argument");
  if (n >= (1ll << 30) || (long long)n * r >= (1ll << 40) || S > 65535 * kLrSC) return set_error(BT_ERR_UNSUPPORTED, "bt_lowrank_mean: tensor too large");
  bt_rng none = {};
  const bt_rng& R = rng ? *rng : none;
  const dim3 grid((unsigned)((n + kLrThreads - 1) / kLrThreads), (unsigned)((S + kLrSC - 1) / kLrSC));
  return launch_kernel(lowrank_mean_kernel, nullptr, "bt_lowrank_mean", grid, dim3(kLrThreads), 0, 0, (hipStream_t)stream, mu, L, (long long)n, (int)r, (int)S, z,
                       make_key(R, 4), R.call_base_dev, R.sample0, m);
}

extern "C" size_t bt_kl_lowrank_workspace(int64_t n, int32_t r) {
  if (n <= 0 || r <= 0 || r > bt::kKlLrMaxRank) return 0;
  const bt::KlLrPlan p = bt::kl_lowrank_plan(n, r);
  return (size_t)(((long long)p.C * p.stride + (long long)r * r) * 8);
}

extern "C" int bt_kl_lowrank(const float* mu, const float* L, int64_t n, int32_t r, float d, const float* prior_mean, const float* prior_var, float* kl_out,
                             int32_t* bad_pivots, void* workspace, size_t workspace_bytes, bt_stream_t stream) {
  using namespace bt;
  if (!mu || !L || !prior_mean || !prior_var || !kl_out || n <= 0 || r <= 0 || !(d > 0.f)) return set_error(BT_ERR_BAD_ARG, "bt_kl_lowrank: bad argument");
  if (r > kKlLrMaxRank || (long long)n * r >= (1ll << 40)) return set_error(BT_ERR_UNSUPPORTED, "bt_kl_lowrank: rank above 4096 or L too large");
  if (!workspace || (((uintptr_t)workspace) & 7u) || workspace_bytes < bt_kl_lowrank_workspace(n, r))
    return set_error(BT_ERR_WORKSPACE, "bt_kl_lowrank: workspace smaller than bt_kl_lowrank_workspace(n, r), or not 8-byte aligned");
  double* const part = reinterpret_cast<double*>(workspace);
  return kl_lowrank_factor("bt_kl_lowrank (sweep)", "bt_kl_lowrank (finish)", mu, L, (long long)n, (int)r, d, prior_mean, prior_var, kl_out, bad_pivots, part,
                           part + kl_lowrank_partials(n, r), false, nullptr, (hipStream_t)stream);
}
