// AvUC calibration losses (utils/avuc_loss.py: AvULoss, AUAvULoss): a row pass, a one-workgroup finish pass and one backward launch.
// No host read, no floating-point atomics, every sum in a fixed order: capturable in a graph and the same bits from run to run.
#include <math.h>

#include "bt_api_internal.h"

namespace bt {

constexpr float AVU_EPS = 1e-10f;   // the loss classes' guard (the numpy metrics' 1e-15 never reaches a kernel)
constexpr double AVU_EPS_D = 1e-10;  // the same in the finish pass's double arithmetic

// Reductions over the NT threads that own one batch row: NT == 64 is one wave (butterflies only, no barrier), NT == 256 the whole
// workgroup (four waves through `red`, added in wave order). Every thread of the group gets the result.
template <int NT>
__device__ __forceinline__ float grp_sum(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (NT == 64) return v;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}

template <int NT>
__device__ __forceinline__ float grp_max(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if (NT == 64) return v;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return v;
}

// The larger value, and among equal values the smaller index: torch.max's choice (the first index of the maximum).
__device__ __forceinline__ void first_max(float& v, int& i, float ov, int oi) {
  if (ov > v || (ov == v && oi < i)) v = ov, i = oi;
}

template <int NT>
__device__ __forceinline__ void grp_first_max(float& v, int& i, float* red, int* redi) {
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    first_max(v, i, ov, oi);
  }
  if (NT == 64) return;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v, redi[threadIdx.x >> 6] = i;
  __syncthreads();
  v = red[0], i = redi[0];
  for (int w = 1; w < 4; ++w) first_max(v, i, red[w], redi[w]);
  __syncthreads();
}

// Workspace of one call (bt_avu_workspace_bytes): rec_f [3][B] = confidence c, uncertainty u, tanh(u); rec_i [3][B] = pred, acc and
// j_i, the number of thresholds below u (the row is uncertain at j < j_i and certain from j_i on); stats [S][B][2] = each sample
// row's max logit and softmax denominator, which the backward reads instead of reducing again.
struct AvuWs {
  float* rec_f;
  int* rec_i;
  float* stats;
};
__host__ __device__ inline AvuWs avu_ws(void* ws, long long B) {
  AvuWs w;
  w.rec_f = static_cast<float*>(ws);
  w.rec_i = reinterpret_cast<int*>(w.rec_f + 3 * B);
  w.stats = w.rec_f + 6 * B;
  return w;
}

// Row pass. NT == 64 (C <= 64): one wave per batch row, four rows per workgroup, lane k owns class k. NT == 256: one workgroup per
// row, thread k owns classes k, k + 256, ... First every sample's max and denominator (stats), then per class the mean probability
// over the samples in sample order, its entropy term and the running first maximum.
template <int NT>
__global__ __launch_bounds__(256) void avu_rows_kernel(int S, int B, int C, int unc_type, const float* __restrict__ logits,
                                                       const long long* __restrict__ labels, void* ws) {
  __shared__ float red[4];
  __shared__ int redi[4];
  const int k = threadIdx.x % NT;
  const int b_raw = blockIdx.x * (256 / NT) + threadIdx.x / NT;
  const bool active = b_raw < B;             // (a wave past the last row walks row B - 1 again and writes nothing: it stays for the barrier)
  const int b = active ? b_raw : B - 1;
  const AvuWs w = avu_ws(ws, B);
  for (int s = 0; s < S; ++s) {
    const float* row = logits + ((long long)s * B + b) * C;
    float mx = -INFINITY;
    for (int c = k; c < C; c += NT) mx = fmaxf(mx, row[c]);
    mx = grp_max<NT>(mx, red);
    float den = 0.f;
    for (int c = k; c < C; c += NT) den += expf(row[c] - mx);
    den = grp_sum<NT>(den, red);
    if (k == 0 && active) {
      w.stats[((long long)s * B + b) * 2] = mx;
      w.stats[((long long)s * B + b) * 2 + 1] = den;
    }
  }
  __syncthreads();   // the stats of this row, written by thread 0 of its group, are read by all of them below
  float hbar = 0.f, hs = 0.f, best = -INFINITY;
  int bi = INT_MAX;
  for (int c = k; c < C; c += NT) {
    float ps = 0.f;
    for (int s = 0; s < S; ++s) {
      const long long r = (long long)s * B + b;
      const float p = expf(logits[r * C + c] - w.stats[r * 2]) / w.stats[r * 2 + 1];
      ps += p;
      if (unc_type) hs -= p * logf(p + AVU_EPS);
    }
    const float pbar = ps / (float)S;
    hbar -= pbar * logf(pbar + AVU_EPS);
    if (pbar > best) best = pbar, bi = c;
  }
  hbar = grp_sum<NT>(hbar, red);
  if (unc_type) hs = grp_sum<NT>(hs, red);
  grp_first_max<NT>(best, bi, red, redi);
  if (k == 0 && active) {
    const float u = unc_type ? hbar - hs / (float)S : hbar;
    w.rec_f[b] = best;
    w.rec_f[(long long)B + b] = u;
    w.rec_f[2ll * B + b] = tanhf(u);
    w.rec_i[b] = bi;
    w.rec_i[(long long)B + b] = (long long)bi == labels[b] ? 1 : 0;   // the label is compared, never an index
  }
}

// np.linspace(0, 1, 21): arange(21) * (1 / 20) with the last point set to the stop value.
__device__ __forceinline__ double avu_x(int j) { return j >= 20 ? 1.0 : j * 0.05; }

// Finish pass, one workgroup of 16 waves. Thresholds in double from the fp32 u (T == 21: th_0 = umin and th_20 = umax exactly), wave
// w sums thresholds w and w + 16 over the rows (lane l takes rows l, l + 64, ...; butterfly), then thread 0 forms AvU_j, V, the loss
// and the backward's coefficients.  coef [4][T + 1]: with g = -beta / (V + eps), a_j = g w_j (1 / D_j - N_j / D_j^2) for a term in
// the numerator and b_j = -g w_j N_j / D_j^2 for one outside it (D_j with its eps, w the trapezoid weights): rows 0, 1 are
// sum_{k < j} a_k and sum_{k >= j} a_k, rows 2, 3 the same of b.
__global__ __launch_bounds__(1024) void avu_finish_kernel(int B, int T, const float* __restrict__ th_dev, float beta, void* ws,
                                                          float* __restrict__ loss, float* __restrict__ v_out, float* __restrict__ sums,
                                                          int* __restrict__ counts, double* __restrict__ thr, float* __restrict__ coef) {
  __shared__ float rmin[16], rmax[16];
  __shared__ double th[21], ca[21], cb[21];
  __shared__ float ssum[21][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const AvuWs w = avu_ws(ws, B);
  const float *cf = w.rec_f, *uf = w.rec_f + B, *tf = w.rec_f + 2ll * B;
  const int* accp = w.rec_i + B;
  int* jip = w.rec_i + 2ll * B;
  if (T == 1) {
    if (tid == 0) th[0] = (double)th_dev[0];
  } else {
    float mn = INFINITY, mx = -INFINITY;
    for (int i = tid; i < B; i += 1024) mn = fminf(mn, uf[i]), mx = fmaxf(mx, uf[i]);
    for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64)), mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) rmin[wv] = mn, rmax[wv] = mx;
    __syncthreads();
    if (tid < T) {
      mn = rmin[0], mx = rmax[0];
      for (int i = 1; i < 16; ++i) mn = fminf(mn, rmin[i]), mx = fmaxf(mx, rmax[i]);
      const double lo = mn, hi = mx;
      th[tid] = tid == 0 ? lo : tid == T - 1 ? hi : fmin(lo + avu_x(tid) * (hi - lo), hi);
    }
  }
  __syncthreads();
  if (tid < T) thr[tid] = th[tid];
  for (int j = wv; j < T; j += 16) {
    const double thj = th[j];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    for (int i = lane; i < B; i += 64) {
      const float c = cf[i], t = tf[i];
      const bool acc = accp[i] != 0, cert = (double)uf[i] <= thj;
      const float term = (acc ? c : 1.f - c) * (cert ? 1.f - t : t);
      const int cls = (acc ? 0 : 2) + (cert ? 0 : 1);   // n_ac, n_au, n_ic, n_iu
      s0 += cls == 0 ? term : 0.f, s1 += cls == 1 ? term : 0.f, s2 += cls == 2 ? term : 0.f, s3 += cls == 3 ? term : 0.f;
      n0 += cls == 0, n1 += cls == 1, n2 += cls == 2, n3 += cls == 3;
    }
    for (int o = 32; o > 0; o >>= 1) {
      s0 += __shfl_xor(s0, o, 64), s1 += __shfl_xor(s1, o, 64), s2 += __shfl_xor(s2, o, 64), s3 += __shfl_xor(s3, o, 64);
      n0 += __shfl_xor(n0, o, 64), n1 += __shfl_xor(n1, o, 64), n2 += __shfl_xor(n2, o, 64), n3 += __shfl_xor(n3, o, 64);
    }
    if (lane == 0) {
      ssum[j][0] = s0, ssum[j][1] = s1, ssum[j][2] = s2, ssum[j][3] = s3;
      sums[j * 4] = s0, sums[j * 4 + 1] = s1, sums[j * 4 + 2] = s2, sums[j * 4 + 3] = s3;
      counts[j * 4] = n0, counts[j * 4 + 1] = n1, counts[j * 4 + 2] = n2, counts[j * 4 + 3] = n3;
    }
  }
  for (int i = tid; i < B; i += 1024) {
    const double u = uf[i];
    int ji = 0;
    for (int j = 0; j < T; ++j) ji += u > th[j];
    jip[i] = ji;
  }
  __syncthreads();
  if (tid != 0) return;
  double V = 0.0, prev = 0.0;
  for (int j = 0; j < T; ++j) {
    // In double from the fp32 sums: in fp32 the eps vanishes in D, and 1 / D - N / D^2 = (D - N) / D^2 is then pure cancellation
    // wherever every row is in the numerator (the reference's fp32 autograd returns a zero gradient there).
    const double N = (double)ssum[j][0] + (double)ssum[j][3], rest = (double)ssum[j][1] + (double)ssum[j][2] + AVU_EPS_D;
    const double D = N + rest;
    const double avu = N / D;
    const double wj = T == 1 ? 1.0 : 0.5 * ((j < T - 1 ? avu_x(j + 1) - avu_x(j) : 0.0) + (j > 0 ? avu_x(j) - avu_x(j - 1) : 0.0));
    if (T == 1) V = avu;
    else if (j > 0) V += (avu_x(j) - avu_x(j - 1)) * (avu + prev) / 2.0;   // the trapezoid rule, what sklearn.metrics.auc computes
    prev = avu;
    ca[j] = wj * (rest / (D * D));
    cb[j] = wj * (-N / (D * D));
  }
  v_out[0] = (float)V;
  loss[0] = (float)(-(double)beta * log(V + AVU_EPS_D));
  const double g = -(double)beta / (V + AVU_EPS_D);
  double pa = 0.0, pb = 0.0;
  for (int j = 0; j <= T; ++j) {
    coef[j] = (float)(g * pa), coef[2 * (T + 1) + j] = (float)(g * pb);
    if (j < T) pa += ca[j], pb += cb[j];
  }
  pa = 0.0, pb = 0.0;
  for (int j = T; j >= 0; --j) {
    if (j < T) pa += ca[j], pb += cb[j];
    coef[(T + 1) + j] = (float)(g * pa), coef[3 * (T + 1) + j] = (float)(g * pb);
  }
}

// Backward, the row pass's launch shape. Per row: d loss / d c and d loss / d u from the row's class and j_i (four reads of coef),
// G_k = d loss / d pbar_k per class, parked in the row's slab of the LAST sample's gradient (each thread reads back only what it
// wrote); then per sample q_k = d loss / d p_sk, the row's sum of p q, and the softmax Jacobian p (q - sum). The last sample's pass
// reads each G_k before it stores that element's result.
template <int NT>
__global__ __launch_bounds__(256) void avu_bwd_kernel(int S, int B, int C, int unc_type, int T, const float* __restrict__ logits,
                                                      const void* ws, const float* __restrict__ coef, const float* __restrict__ gout,
                                                      float* dlogits) {
  __shared__ float red[4];
  const int k = threadIdx.x % NT;
  const int b = blockIdx.x * (256 / NT) + threadIdx.x / NT;
  if (b >= B) return;   // (NT == 64 only, whose reductions hold no barrier)
  const AvuWs w = avu_ws(const_cast<void*>(ws), B);
  const float c_ = w.rec_f[b], t = w.rec_f[2ll * B + b];
  const int pred = w.rec_i[b], acc = w.rec_i[(long long)B + b], ji = w.rec_i[2ll * B + b];
  const float a_lo = coef[ji], a_hi = coef[(T + 1) + ji], b_lo = coef[2 * (T + 1) + ji], b_hi = coef[3 * (T + 1) + ji];
  float dc, dt;
  if (acc) {   // certain: c (1 - t) in the numerator; uncertain: c t outside it
    dc = a_hi * (1.f - t) + b_lo * t;
    dt = c_ * (b_lo - a_hi);
  } else {     // certain: (1 - c)(1 - t) outside the numerator; uncertain: (1 - c) t in it
    dc = -((1.f - t) * b_hi + t * a_lo);
    dt = (1.f - c_) * (a_lo - b_hi);
  }
  const float up = gout[0];
  dc *= up;
  const float du = up * dt * (1.f - t * t);
  const float inv_s = 1.f / (float)S;
  float* G = dlogits + ((long long)(S - 1) * B + b) * C;
  for (int c = k; c < C; c += NT) {
    float ps = 0.f;
    for (int s = 0; s < S; ++s) {
      const long long r = (long long)s * B + b;
      ps += expf(logits[r * C + c] - w.stats[r * 2]) / w.stats[r * 2 + 1];
    }
    const float pbar = ps / (float)S;
    G[c] = -du * (logf(pbar + AVU_EPS) + pbar / (pbar + AVU_EPS)) + (c == pred ? dc : 0.f);
  }
  for (int s = 0; s < S; ++s) {
    const long long r = (long long)s * B + b;
    const float* row = logits + r * C;
    float* out = dlogits + r * C;
    const float mx = w.stats[r * 2], den = w.stats[r * 2 + 1];
    float dot = 0.f;
    for (int c = k; c < C; c += NT) {
      const float p = expf(row[c] - mx) / den;
      float q = G[c] * inv_s;
      if (unc_type) q += du * inv_s * (logf(p + AVU_EPS) + p / (p + AVU_EPS));
      dot += p * q;
    }
    dot = grp_sum<NT>(dot, red);
    for (int c = k; c < C; c += NT) {
      const float p = expf(row[c] - mx) / den;
      float q = G[c] * inv_s;
      if (unc_type) q += du * inv_s * (logf(p + AVU_EPS) + p / (p + AVU_EPS));
      out[c] = p * (q - dot);
    }
  }
}

static size_t avu_ws_bytes(long long S, long long B) { return (size_t)(4 * (6 * B + 2 * S * B) + 15) / 16 * 16; }

static int avu_check_shape(const char* who, int32_t S, int32_t B, int32_t C, int32_t unc_type, int32_t T) {
  char buf[160];
  const char* what = nullptr;
  if (S <= 0 || B <= 0 || C <= 0) what = "S, B and C must be positive";
  else if (T != 1 && T != 21) what = "T must be 1 or 21";
  else if (unc_type != 0 && unc_type != 1) what = "unc_type must be 0 or 1";
  else if (unc_type == 1 && S == 1) what = "unc_type 1 (model uncertainty) needs S > 1 Monte Carlo samples";
  else if (B > (1 << 28)) what = "B above 2^28";
  if (!what) return BT_OK;
  snprintf(buf, sizeof(buf), "%s: bad argument: %s", who, what);
  return set_error(BT_ERR_BAD_ARG, buf);
}

}  // namespace bt

extern "C" size_t bt_avu_workspace_bytes(int32_t S, int32_t B, int32_t C, int32_t T) {
  if (S <= 0 || B <= 0 || C <= 0 || (T != 1 && T != 21)) return 0;
  return bt::avu_ws_bytes(S, B);
}

extern "C" int bt_avu_fwd(int32_t S, int32_t B, int32_t C, const float* logits, const int64_t* labels, int32_t unc_type, int32_t T,
                          const float* threshold, float beta, float* loss, float* v, float* sums, int32_t* counts, double* thresholds,
                          float* coef, void* workspace, size_t workspace_bytes, bt_stream_t stream) {
  using namespace bt;
  if (int rc = avu_check_shape("bt_avu_fwd", S, B, C, unc_type, T)) return rc;
  if (!logits || !labels || !loss || !v || !sums || !counts || !thresholds || !coef || !workspace || (T == 1 && !threshold))
    return set_error(BT_ERR_BAD_ARG, "bt_avu_fwd: bad argument: null pointer");
  if (((uintptr_t)workspace & 7u) || ((uintptr_t)thresholds & 7u) || ((uintptr_t)labels & 7u))
    return set_error(BT_ERR_BAD_ARG, "bt_avu_fwd: bad argument: labels, thresholds and workspace must be 8-byte aligned");
  if (workspace_bytes < avu_ws_bytes(S, B)) return set_error(BT_ERR_WORKSPACE, "bt_avu_fwd: workspace smaller than bt_avu_workspace_bytes");
  const hipStream_t st = (hipStream_t)stream;
  const long long* lab = reinterpret_cast<const long long*>(labels);
  if (int rc = launch_kernel(C <= 64 ? avu_rows_kernel<64> : avu_rows_kernel<256>, nullptr, "bt_avu_fwd", dim3(C <= 64 ? (B + 3) / 4 : B), dim3(256), 0, 0, st, S, B, C,
                             unc_type, logits, lab, workspace))
    return rc;
  return launch_kernel(avu_finish_kernel, nullptr, "bt_avu_fwd", dim3(1), dim3(1024), 0, 0, st, B, T, threshold, beta, workspace, loss, v, sums, counts, thresholds, coef);
}

extern "C" int bt_avu_bwd(int32_t S, int32_t B, int32_t C, const float* logits, int32_t unc_type, int32_t T, const float* coef,
                          const float* grad_loss, const void* workspace, size_t workspace_bytes, float* dlogits, bt_stream_t stream) {
  using namespace bt;
  if (int rc = avu_check_shape("bt_avu_bwd", S, B, C, unc_type, T)) return rc;
  if (!logits || !coef || !grad_loss || !workspace || !dlogits) return set_error(BT_ERR_BAD_ARG, "bt_avu_bwd: bad argument: null pointer");
  if ((uintptr_t)workspace & 7u) return set_error(BT_ERR_BAD_ARG, "bt_avu_bwd: bad argument: workspace must be 8-byte aligned");
  if (workspace_bytes < avu_ws_bytes(S, B)) return set_error(BT_ERR_WORKSPACE, "bt_avu_bwd: workspace smaller than bt_avu_workspace_bytes");
  const hipStream_t st = (hipStream_t)stream;
  return launch_kernel(C <= 64 ? avu_bwd_kernel<64> : avu_bwd_kernel<256>, nullptr, "bt_avu_bwd", dim3(C <= 64 ? (B + 3) / 4 : B), dim3(256), 0, 0, st, S, B, C, unc_type, T,
                       logits, workspace, coef, grad_loss, dlogits);
}
