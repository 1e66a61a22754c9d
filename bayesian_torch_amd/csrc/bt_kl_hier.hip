// KL of the hierarchical (inverse-gamma hyper-prior) layers, reference layers/variational_layers/hiearchial_variational_layers.py
// (:331-381 Linear, :477-522 Conv2d): every weight has its own variational Inv-Gamma(a, b) over its prior variance. Per element,
// with a = exp(log_a), b = exp(log_b), sigma = log1p(exp(rho)), m = prior_mu and the hyper-prior (a0, b0):
//   A = 1/2 [ ln b - psi(a) - ln sigma^2 + (a/b)(sigma^2 + (mu - m)^2) - 1 ]
//   B = (a - a0) psi(a) - lnGamma(a) + lnGamma(a0) + a0 (ln b - ln b0) + (b0 - b)(a/b)
//   kl = SUM (A + B)                                     (a sum, not the mean of the Gaussian layers)
// The reference makes ~40 full-tensor ATen passes of it per layer and call; here one sweep, 28 B/element (seven tensors), for up to
// 64 tensors per launch, and one element-wise launch for the four gradients. Reductions as in bt_kl.hip: fp64 block sums, a ticket,
// a fixed-order finish.
#include "bt_api_internal.h"
#include "bt_special.h"

namespace bt {

struct KlHierSegs {
  const float* mu[BT_KL_MAX_SEGMENTS];
  const float* rho[BT_KL_MAX_SEGMENTS];
  const float* pmu[BT_KL_MAX_SEGMENTS];
  const float* la[BT_KL_MAX_SEGMENTS];
  const float* lb[BT_KL_MAX_SEGMENTS];
  const float* a0[BT_KL_MAX_SEGMENTS];
  const float* b0[BT_KL_MAX_SEGMENTS];
  long long n[BT_KL_MAX_SEGMENTS];
  int first_block[BT_KL_MAX_SEGMENTS + 1];  // blocks [first_block[i], first_block[i+1]) work on segment i
  unsigned long long new_layer;             // bit i: segment i starts a new layer (fp32 summation grouping)
  int nseg;
};

constexpr int kHierThreads = 256;
constexpr int kHierElemsPerPass = kHierThreads * 4;      // one float4 per tensor and thread in flight: the sweep is bound by its arithmetic
constexpr int kHierElemsPerBlock = 4 * kHierElemsPerPass;
constexpr int kHierMaxBlocksPerSeg = 2048;               // above 8,388,608 elements a segment's blocks stride over it

// sigma = log1p(exp(rho)) as the reference writes it, on the accurate library functions: here sigma^2 is multiplied by a/b, which
// reaches e^40, and the KL's error bound has no room for the forward kernels' exp2-based softplus (bt_device.h).
__device__ __forceinline__ float hier_sigma(float rho) { return log1pf(expf(rho)); }

// One element's A + B. ln b is log_b itself (the reference takes log(exp(log_b))); ln sigma^2 is 2 ln sigma (sigma^2 underflows first).
__device__ __forceinline__ float hier_term(float mu, float rho, float pm, float la, float lb, float a0, float b0) {
  const float a = expf(la), b = expf(lb);
  const float sg = hier_sigma(rho);
  const float r = a / b;
  const float d = mu - pm;
  const float s = sg * sg + d * d;
  const float psi = digamma(a);
  const float A = 0.5f * ((((lb - psi) - 2.0f * logf(sg)) + r * s) - 1.0f);
  const float B = ((((a - a0) * psi - lgamma_pos(a)) + lgamma_pos(a0)) + a0 * (lb - logf(b0))) + (b0 - b) * r;
  return A + B;
}

__global__ __launch_bounds__(kHierThreads) void kl_hier_kernel(KlHierSegs sg, float* kl_out, float* seg_out, double* slots, unsigned* counter,
                                                              int total_blocks) {
  __shared__ double red[4];
  __shared__ int is_last;
  int seg = 0;
  while (seg + 1 < sg.nseg && (int)blockIdx.x >= sg.first_block[seg + 1]) ++seg;
  const int nb = sg.first_block[seg + 1] - sg.first_block[seg];
  const int lb_ = blockIdx.x - sg.first_block[seg];
  const long long n = sg.n[seg];
  const float* __restrict__ mu = sg.mu[seg];
  const float* __restrict__ rho = sg.rho[seg];
  const float* __restrict__ pmu = sg.pmu[seg];
  const float* __restrict__ la = sg.la[seg];
  const float* __restrict__ lb = sg.lb[seg];
  const float* __restrict__ a0 = sg.a0[seg];
  const float* __restrict__ b0 = sg.b0[seg];
  const bool vec_ok =
      ((((uintptr_t)mu | (uintptr_t)rho | (uintptr_t)pmu | (uintptr_t)la | (uintptr_t)lb | (uintptr_t)a0 | (uintptr_t)b0) & 15u) == 0);

  double acc = 0.0;
  const long long n4 = vec_ok ? (n >> 2) : 0;  // float4 groups
  for (long long i = (long long)lb_ * kHierThreads + threadIdx.x; i < n4; i += (long long)nb * kHierThreads) {
    const float4 m = reinterpret_cast<const float4*>(mu)[i], r = reinterpret_cast<const float4*>(rho)[i];
    const float4 p = reinterpret_cast<const float4*>(pmu)[i], x = reinterpret_cast<const float4*>(la)[i];
    const float4 y = reinterpret_cast<const float4*>(lb)[i], u = reinterpret_cast<const float4*>(a0)[i];
    const float4 v = reinterpret_cast<const float4*>(b0)[i];
    const float t0 = hier_term(m.x, r.x, p.x, x.x, y.x, u.x, v.x) + hier_term(m.y, r.y, p.y, x.y, y.y, u.y, v.y);
    const float t1 = hier_term(m.z, r.z, p.z, x.z, y.z, u.z, v.z) + hier_term(m.w, r.w, p.w, x.w, y.w, u.w, v.w);
    acc += (double)t0 + (double)t1;
  }
  // tail (or everything, when a pointer is not 16-B aligned)
  for (long long i = (n4 << 2) + (long long)lb_ * kHierThreads + threadIdx.x; i < n; i += (long long)nb * kHierThreads)
    acc += (double)hier_term(mu[i], rho[i], pmu[i], la[i], lb[i], a0[i], b0[i]);

  const double bsum = block_sum_256(acc, red);
  if (threadIdx.x == 0) is_last = publish_and_ticket_wt(slots, counter, blockIdx.x, bsum, (unsigned)total_blocks) ? 1 : 0;
  __syncthreads();
  if (!is_last) return;
  // last arriver: the fixed-order parallel finish of kl_normal_kernel (bt_kl.hip). A segment's fp64 sum -> fp32; segments of one
  // layer added in fp32, layers added in fp32 in order.
  __shared__ double seg_sum[BT_KL_MAX_SEGMENTS];
  for (int s = 0; s < sg.nseg; ++s) {
    double t = 0.0;
    for (int b = sg.first_block[s] + (int)threadIdx.x; b < sg.first_block[s + 1]; b += kHierThreads) {
      t += __hip_atomic_load(&slots[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&slots[b], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // leave the workspace zeroed
    }
    t = wave_sum(t);
    __syncthreads();   // (red is free again)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) seg_sum[s] = (red[0] + red[1]) + (red[2] + red[3]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = 0.0f, layer = 0.0f;
    for (int s = 0; s < sg.nseg; ++s) {
      const float v = (float)seg_sum[s];
      if (seg_out) seg_out[s] = v;
      if ((sg.new_layer >> s) & 1ull) {
        if (s) total += layer;  // 0.0f + x is exact, so the first layer enters unrounded
        layer = v;
      } else {
        layer += v;
      }
    }
    kl_out[0] = total + layer;
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // leave the workspace zeroed
  }
}

// d kl / d(mu, rho, log_a, log_b) of one element, times the upstream gradient g. With r = a/b, s = sigma^2 + (mu - m)^2, c = a0 + 1/2:
//   d/dmu = r (mu - m)      d/drho = (r sigma - 1/sigma) sigmoid(rho)      d/dlog_b = 1/2 + a0 - r (s/2 + b0)
//   d/dlog_a = a [ (a - c) psi'(a) + (s/2 + b0)/b - 1 ] = a (a psi'(a) - 1) - c (a psi'(a)) + r (s/2 + b0)
// (psi cancels). The last form keeps the 1 - 1 of large a out of the arithmetic (trigamma_pair) and never squares 1/a.
struct KlHierBwdSegs {
  const float *mu[BT_KL_MAX_SEGMENTS], *rho[BT_KL_MAX_SEGMENTS], *pmu[BT_KL_MAX_SEGMENTS], *la[BT_KL_MAX_SEGMENTS], *lb[BT_KL_MAX_SEGMENTS];
  const float *a0[BT_KL_MAX_SEGMENTS], *b0[BT_KL_MAX_SEGMENTS];
  float *dmu[BT_KL_MAX_SEGMENTS], *drho[BT_KL_MAX_SEGMENTS], *dla[BT_KL_MAX_SEGMENTS], *dlb[BT_KL_MAX_SEGMENTS];      // each may be null
  long long n[BT_KL_MAX_SEGMENTS];
  int boff[BT_KL_MAX_SEGMENTS + 1];  // first block of every segment
  int nseg;
};

__global__ __launch_bounds__(256) void kl_hier_bwd_kernel(const KlHierBwdSegs a, const float* __restrict__ gup) {
  int seg = 0;
  while (seg + 1 < a.nseg && (int)blockIdx.x >= a.boff[seg + 1]) ++seg;   // uniform
  const long long n = a.n[seg];
  const float g = gup[0];
  const float *mu = a.mu[seg], *rho = a.rho[seg], *pmu = a.pmu[seg], *la = a.la[seg], *lb = a.lb[seg], *a0 = a.a0[seg], *b0 = a.b0[seg];
  float *dmu = a.dmu[seg], *drho = a.drho[seg], *dla = a.dla[seg], *dlb = a.dlb[seg];
  const long long base = (long long)((int)blockIdx.x - a.boff[seg]) * 1024;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = base + threadIdx.x + 256 * k;
    if (i < n) {
      const float av = expf(la[i]), bv = expf(lb[i]);
      const float r = av / bv;
      const float rh = rho[i];
      const float sg = hier_sigma(rh);
      const float d = mu[i] - pmu[i];
      if (dmu) dmu[i] = (r * d) * g;
      if (drho) {
        const float sgm = 1.0f / (1.0f + expf(-rh));
        drho[i] = ((r * sg - 1.0f / sg) * sgm) * g;
      }
      if (dla || dlb) {
        const float s = sg * sg + d * d;
        const float q = r * (0.5f * s + b0[i]);
        const float a0v = a0[i];
        if (dlb) dlb[i] = ((0.5f + a0v) - q) * g;
        if (dla) {
          float p1, xm1;
          trigamma_pair(av, p1, xm1);
          dla[i] = ((av * xm1 - (a0v + 0.5f) * (xm1 + 1.0f)) + q) * g;
        }
      }
    }
  }
}

static bool hier_null_segment(int i, const float* const* mu, const float* const* rho, const float* const* prior_mu, const float* const* log_a,
                              const float* const* log_b, const float* const* a0, const float* const* b0, const int64_t* numel) {
  return numel[i] <= 0 || !mu[i] || !rho[i] || !prior_mu[i] || !log_a[i] || !log_b[i] || !a0[i] || !b0[i];
}

}  // namespace bt

extern "C" int bt_kl_hier(int32_t n_segments, const float* const* mu, const float* const* rho, const float* const* prior_mu,
                          const float* const* log_a, const float* const* log_b, const float* const* a0, const float* const* b0,
                          const int64_t* numel, const int32_t* layer_of_segment, float* kl_out, float* seg_out, void* workspace,
                          size_t workspace_bytes, bt_stream_t stream) {
  using namespace bt;
  if (n_segments <= 0 || n_segments > BT_KL_MAX_SEGMENTS) return set_error(BT_ERR_BAD_ARG, "bt_kl_hier: n_segments must be in [1, 64]");
  if (!mu || !rho || !prior_mu || !log_a || !log_b || !a0 || !b0 || !numel || !kl_out) return set_error(BT_ERR_BAD_ARG, "bt_kl_hier: null argument");
  if (!workspace || workspace_bytes < BT_WORKSPACE_BYTES) return set_error(BT_ERR_BAD_ARG, "bt_kl_hier: workspace smaller than BT_WORKSPACE_BYTES");
  KlHierSegs sg;
  int blocks = 0;
  for (int i = 0; i < n_segments; ++i) {
    if (hier_null_segment(i, mu, rho, prior_mu, log_a, log_b, a0, b0, numel)) return set_error(BT_ERR_BAD_ARG, "bt_kl_hier: empty or null segment");
    sg.mu[i] = mu[i], sg.rho[i] = rho[i], sg.pmu[i] = prior_mu[i], sg.la[i] = log_a[i], sg.lb[i] = log_b[i], sg.a0[i] = a0[i], sg.b0[i] = b0[i];
    sg.n[i] = numel[i];
    long long nb = (numel[i] + kHierElemsPerBlock - 1) / kHierElemsPerBlock;
    if (nb > kHierMaxBlocksPerSeg) nb = kHierMaxBlocksPerSeg;
    sg.first_block[i] = blocks;
    blocks += (int)nb;
    if (blocks > kMaxSlots) return set_error(BT_ERR_UNSUPPORTED, "bt_kl_hier: too many blocks for the workspace; split the call");
  }
  sg.first_block[n_segments] = blocks;
  sg.nseg = n_segments;
  sg.new_layer = 0;
  for (int i = 0; i < n_segments; ++i) {
    if (layer_of_segment && i && layer_of_segment[i] < layer_of_segment[i - 1]) return set_error(BT_ERR_BAD_ARG, "bt_kl_hier: layer_of_segment must be non-decreasing");
    if (i == 0 || !layer_of_segment || layer_of_segment[i] != layer_of_segment[i - 1]) sg.new_layer |= 1ull << i;
  }
  hipLaunchKernelGGL(kl_hier_kernel, dim3(blocks), dim3(kHierThreads), 0, (hipStream_t)stream, sg, kl_out, seg_out, ws_slots(workspace),
                     ws_counter(workspace), blocks);
  return check_launch("bt_kl_hier");
}

extern "C" int bt_kl_hier_bwd(int32_t n_segments, const float* const* mu, const float* const* rho, const float* const* prior_mu,
                              const float* const* log_a, const float* const* log_b, const float* const* a0, const float* const* b0,
                              const int64_t* numel, const float* grad_kl, float* const* dmu, float* const* drho, float* const* dlog_a,
                              float* const* dlog_b, bt_stream_t stream) {
  using namespace bt;
  if (n_segments <= 0 || n_segments > BT_KL_MAX_SEGMENTS) return set_error(BT_ERR_BAD_ARG, "bt_kl_hier_bwd: n_segments must be in [1, 64]");
  if (!mu || !rho || !prior_mu || !log_a || !log_b || !a0 || !b0 || !numel || !grad_kl) return set_error(BT_ERR_BAD_ARG, "bt_kl_hier_bwd: null argument");
  if (!dmu && !drho && !dlog_a && !dlog_b) return set_error(BT_ERR_BAD_ARG, "bt_kl_hier_bwd: no gradient was asked for");
  KlHierBwdSegs a = {};
  long long blocks = 0;
  for (int i = 0; i < n_segments; ++i) {
    if (hier_null_segment(i, mu, rho, prior_mu, log_a, log_b, a0, b0, numel)) return set_error(BT_ERR_BAD_ARG, "bt_kl_hier_bwd: empty or null segment");
    a.mu[i] = mu[i], a.rho[i] = rho[i], a.pmu[i] = prior_mu[i], a.la[i] = log_a[i], a.lb[i] = log_b[i], a.a0[i] = a0[i], a.b0[i] = b0[i];
    a.dmu[i] = dmu ? dmu[i] : nullptr, a.drho[i] = drho ? drho[i] : nullptr;
    a.dla[i] = dlog_a ? dlog_a[i] : nullptr, a.dlb[i] = dlog_b ? dlog_b[i] : nullptr;
    a.n[i] = numel[i];
    a.boff[i] = (int)blocks;
    blocks += (numel[i] + 1023) / 1024;
    if (blocks > 0x7FFFFFFFll) return set_error(BT_ERR_UNSUPPORTED, "bt_kl_hier_bwd: too many elements for one launch");
  }
  a.boff[n_segments] = (int)blocks;
  a.nseg = n_segments;
  hipLaunchKernelGGL(kl_hier_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, grad_kl);
  return check_launch("bt_kl_hier_bwd");
}

// Host-only: the special functions of bt_special.h evaluated on the CPU (the same source the kernels compile), so that they can be
// checked where there is no device.
extern "C" int bt_special_eval(int32_t kind, const float* x, int64_t n, float* out) {
  using namespace bt;
  if (!x || !out || n <= 0) return set_error(BT_ERR_BAD_ARG, "bt_special_eval: null argument or empty input");
  if (kind < BT_SPECIAL_DIGAMMA || kind > BT_SPECIAL_X_TRIGAMMA_M1) return set_error(BT_ERR_BAD_ARG, "bt_special_eval: unknown kind");
  for (int64_t i = 0; i < n; ++i) {
    float p, q;
    switch (kind) {
      case BT_SPECIAL_DIGAMMA: out[i] = digamma(x[i]); break;
      case BT_SPECIAL_TRIGAMMA: out[i] = trigamma(x[i]); break;
      case BT_SPECIAL_LGAMMA: out[i] = lgamma_pos(x[i]); break;
      default: trigamma_pair(x[i], p, q); out[i] = q; break;
    }
  }
  return BT_OK;
}
