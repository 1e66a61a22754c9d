// KL of the hierarchical (inverse-gamma hyper-prior) layers, reference layers/variational_layers/hiearchial_variational_layers.py
// (:331-381 Linear, :477-522 Conv2d): every weight has its own variational Inv-Gamma(a, b) over its prior variance. Per element,
// with a = exp(log_a), b = exp(log_b), sigma = log1p(exp(rho)), m = prior_mu and the hyper-prior (a0, b0):
//   A = 1/2 [ ln b - psi(a) - ln sigma^2 + (a/b)(sigma^2 + (mu - m)^2) - 1 ]
//   B = (a - a0) psi(a) - lnGamma(a) + lnGamma(a0) + a0 (ln b - ln b0) + (b0 - b)(a/b)
//   kl = SUM (A + B)                                     (a sum, not the mean of the Gaussian layers)
// The reference makes ~40 full-tensor ATen passes of it per layer and call; here one sweep, 28 B/element (seven tensors), for up to
// 64 tensors per launch, and one element-wise launch for the four gradients. Reductions as in bt_kl.hip: fp64 block sums, a ticket,
// a fixed-order finish.
#include "bt_segments.h"
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
  SegTable t;
};
inline uint64_t digest_arg(uint64_t h, const KlHierSegs& a) { return digest_segs(h, a.t, a.mu, a.rho, a.pmu, a.la, a.lb, a.a0, a.b0); }

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
  int seg, nb, lb_;
  seg_locate(sg.t, seg, nb, lb_);
  const long long n = sg.t.n[seg];
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
  // last arriver: a segment's fp64 sum -> fp32, grouped by layer
  seg_finish(sg.t, slots, counter, red, kl_out, seg_out, [](double sum, long long) { return (float)sum; });
}

// d kl / d(mu, rho, log_a, log_b) of one element, times the upstream gradient g. With r = a/b, s = sigma^2 + (mu - m)^2, c = a0 + 1/2:
//   d/dmu = r (mu - m)      d/drho = (r sigma - 1/sigma) sigmoid(rho)      d/dlog_b = 1/2 + a0 - r (s/2 + b0)
//   d/dlog_a = a [ (a - c) psi'(a) + (s/2 + b0)/b - 1 ] = a (a psi'(a) - 1) - c (a psi'(a)) + r (s/2 + b0)
// (psi cancels). The last form keeps the 1 - 1 of large a out of the arithmetic (trigamma_pair) and never squares 1/a.
struct KlHierBwdSegs {
  const float *mu[BT_KL_MAX_SEGMENTS], *rho[BT_KL_MAX_SEGMENTS], *pmu[BT_KL_MAX_SEGMENTS], *la[BT_KL_MAX_SEGMENTS], *lb[BT_KL_MAX_SEGMENTS];
  const float *a0[BT_KL_MAX_SEGMENTS], *b0[BT_KL_MAX_SEGMENTS];
  float *dmu[BT_KL_MAX_SEGMENTS], *drho[BT_KL_MAX_SEGMENTS], *dla[BT_KL_MAX_SEGMENTS], *dlb[BT_KL_MAX_SEGMENTS];      // each may be null
  SegTable t;
};
inline uint64_t digest_arg(uint64_t h, const KlHierBwdSegs& a) {
  return digest_segs(h, a.t, a.mu, a.rho, a.pmu, a.la, a.lb, a.a0, a.b0, a.dmu, a.drho, a.dla, a.dlb);
}
static_assert(sizeof(KlHierSegs) <= kMaxSegArgBytes && sizeof(KlHierBwdSegs) == kMaxSegArgBytes, "kl_hier_bwd_kernel's block is the largest there is");
constexpr int kHierBwdElemsPerBlock = 1024;

__global__ __launch_bounds__(256) void kl_hier_bwd_kernel(const KlHierBwdSegs a, const float* __restrict__ gup) {
  int seg, nb, lb_;
  seg_locate(a.t, seg, nb, lb_);   // uniform
  const long long n = a.t.n[seg];
  const float g = gup[0];
  const float *mu = a.mu[seg], *rho = a.rho[seg], *pmu = a.pmu[seg], *la = a.la[seg], *lb = a.lb[seg], *a0 = a.a0[seg], *b0 = a.b0[seg];
  float *dmu = a.dmu[seg], *drho = a.drho[seg], *dla = a.dla[seg], *dlb = a.dlb[seg];
  const long long base = (long long)lb_ * kHierBwdElemsPerBlock;
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
  KlHierSegs sg = {};
  int i = 0;   // (stops at the first bad segment: the partition's refusal of the segments in front of it comes first)
  for (; i < n_segments && !hier_null_segment(i, mu, rho, prior_mu, log_a, log_b, a0, b0, numel); ++i) {
    sg.mu[i] = mu[i], sg.rho[i] = rho[i], sg.pmu[i] = prior_mu[i], sg.la[i] = log_a[i], sg.lb[i] = log_b[i], sg.a0[i] = a0[i], sg.b0[i] = b0[i];
    sg.t.n[i] = numel[i];
  }
  const int blocks = seg_partition(sg.t, i, numel, kHierElemsPerBlock, kHierMaxBlocksPerSeg, kMaxSlots, "bt_kl_hier");   // (a slot per block)
  if (blocks < 0) return blocks;
  if (i < n_segments) return set_error(BT_ERR_BAD_ARG, "bt_kl_hier: empty or null segment");
  if (int rc = seg_layers(sg.t, n_segments, layer_of_segment, "bt_kl_hier")) return rc;
  return launch_kernel(kl_hier_kernel, nullptr, "bt_kl_hier", dim3(blocks), dim3(kHierThreads), 0, 0, (hipStream_t)stream, sg, kl_out, seg_out, ws_slots(workspace),
                       ws_counter(workspace), blocks);
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
  int i = 0;   // (as in bt_kl_hier)
  for (; i < n_segments && !hier_null_segment(i, mu, rho, prior_mu, log_a, log_b, a0, b0, numel); ++i) {
    a.mu[i] = mu[i], a.rho[i] = rho[i], a.pmu[i] = prior_mu[i], a.la[i] = log_a[i], a.lb[i] = log_b[i], a.a0[i] = a0[i], a.b0[i] = b0[i];
    a.dmu[i] = dmu ? dmu[i] : nullptr, a.drho[i] = drho ? drho[i] : nullptr;
    a.dla[i] = dlog_a ? dlog_a[i] : nullptr, a.dlb[i] = dlog_b ? dlog_b[i] : nullptr;
    a.t.n[i] = numel[i];
  }
  const int blocks = seg_partition(a.t, i, numel, kHierBwdElemsPerBlock, 0, 0, "bt_kl_hier_bwd");
  if (blocks < 0) return blocks;
  if (i < n_segments) return set_error(BT_ERR_BAD_ARG, "bt_kl_hier_bwd: empty or null segment");
  return launch_kernel(kl_hier_bwd_kernel, nullptr, "bt_kl_hier_bwd", dim3((unsigned)blocks), dim3(256), 0, 0, (hipStream_t)stream, a, grad_kl);
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
