// K6: standalone closed-form KL of mean-field Gaussians against per-element Gaussian priors.
// Replaces kl_loss() / get_kl_loss() (reference layers/base_variational_layer.py:68-72,
// variational_layers/linear_variational.py:146-158, models/dnn_to_bnn.py:157-165): there it is
// ~12 full-tensor ATen passes per layer; here one pass, 16 B/element (mu, rho, prior_mu,
// prior_sigma), HBM-bound, for up to 64 tensors (a whole model) per launch.
// Its gradient kernels live here too: one tensor per launch (bt_kl_normal_bwd) and a whole model's tensors in one (bt_kl_normal_bwd_segs).
#include "bt_segments.h"

namespace bt {

struct KlSegs {
  const float* mu[kMaxSegs];
  const float* rho[kMaxSegs];
  const float* pmu[kMaxSegs];
  const float* psig[kMaxSegs];
  SegTable t;
  int rho_is_sigma;
  int laplace;  // 'laplace' branch of kl_div (prior tensors are ignored, as in the reference) instead of the Gaussian closed form
};
inline uint64_t digest_arg(uint64_t h, const KlSegs& a) {
  return digest_arg(digest_arg(digest_segs(h, a.t, a.mu, a.rho, a.pmu, a.psig), a.rho_is_sigma), a.laplace);
}

constexpr int kKlThreads = 256;
constexpr int kKlVecPerThread = 4;                                   // float4 loads in flight per tensor per thread
constexpr int kKlElemsPerBlock = kKlThreads * 4 * kKlVecPerThread;  // 4096 elements per block-iteration
constexpr int kKlMaxBlocksPerSeg = 1024;

__global__ __launch_bounds__(kKlThreads) void kl_normal_kernel(KlSegs sg, float* kl_out, double* slots, unsigned* counter,
                                                              int total_blocks) {
  __shared__ double red[4];
  __shared__ int is_last;
  int seg, nb, lb;
  seg_locate(sg.t, seg, nb, lb);
  const long long n = sg.t.n[seg];
  const float* __restrict__ mu = sg.mu[seg];
  const float* __restrict__ rho = sg.rho[seg];
  const float* __restrict__ pmu = sg.pmu[seg];
  const float* __restrict__ psig = sg.psig[seg];
  const bool vec_ok = ((((uintptr_t)mu | (uintptr_t)rho | (uintptr_t)pmu | (uintptr_t)psig) & 15u) == 0);

  const bool is_sigma = sg.rho_is_sigma != 0;
  auto sig = [&](float v) { return is_sigma ? v : softplus(v); };
  const bool lap = sg.laplace != 0;
  auto kl_term = [&](float mq, float sq, float mp, float sp) { return lap ? kl_term_laplace(mq, sq) : bt::kl_term(mq, sq, mp, sp); };
  double acc = 0.0;
  const long long n4 = vec_ok ? (n >> 2) : 0;  // float4 groups
  for (long long base = (long long)lb * (kKlThreads * kKlVecPerThread); base < n4; base += (long long)nb * (kKlThreads * kKlVecPerThread)) {
    float4 m[kKlVecPerThread], r[kKlVecPerThread], pm[kKlVecPerThread], ps[kKlVecPerThread];
#pragma unroll
    for (int v = 0; v < kKlVecPerThread; ++v) {
      const long long i = base + v * kKlThreads + threadIdx.x;
      if (i < n4) {
        m[v] = reinterpret_cast<const float4*>(mu)[i];
        r[v] = reinterpret_cast<const float4*>(rho)[i];
        pm[v] = reinterpret_cast<const float4*>(pmu)[i];
        ps[v] = reinterpret_cast<const float4*>(psig)[i];
      }
    }
#pragma unroll
    for (int v = 0; v < kKlVecPerThread; ++v) {
      const long long i = base + v * kKlThreads + threadIdx.x;
      if (i < n4) {
        float t = kl_term(m[v].x, sig(r[v].x), pm[v].x, ps[v].x);
        t += kl_term(m[v].y, sig(r[v].y), pm[v].y, ps[v].y);
        float t2 = kl_term(m[v].z, sig(r[v].z), pm[v].z, ps[v].z);
        t2 += kl_term(m[v].w, sig(r[v].w), pm[v].w, ps[v].w);
        acc += (double)t + (double)t2;
      }
    }
  }
  // tail (or everything, when a pointer is not 16-B aligned)
  for (long long i = (n4 << 2) + (long long)lb * kKlThreads + threadIdx.x; i < n; i += (long long)nb * kKlThreads)
    acc += (double)kl_term(mu[i], sig(rho[i]), pmu[i], psig[i]);

  const double bsum = block_sum_256(acc, red);
  if (threadIdx.x == 0) is_last = publish_and_ticket_wt(slots, counter, blockIdx.x, bsum, (unsigned)total_blocks) ? 1 : 0;
  __syncthreads();
  if (!is_last) return;
  // last arriver: the segments' means in fp64 -> fp32, grouped by layer
  seg_finish(sg.t, slots, counter, red, kl_out, nullptr, [](double sum, long long cnt) { return (float)(sum / (double)cnt); });
}

// dKL/dmu, dKL/drho of the normal-prior KL (base_variational_layer.py:70-72), scaled by the upstream gradient g[0] / n
__global__ __launch_bounds__(256) void kl_normal_bwd_kernel(const float* __restrict__ mu, const float* __restrict__ rho, const float* __restrict__ pmu,
                                                            const float* __restrict__ psig, const float* __restrict__ gup, long long n, int laplace,
                                                            float* __restrict__ dmu, float* __restrict__ drho) {
  const float gs = gup[0] / (float)n;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    kl_elem_grad(mu[i], rho[i], pmu, psig, i, laplace, gs, dmu[i], drho[i]);
  }
}

// All tensors of a model in one launch (get_kl_loss under autograd): block b works on 1024 elements of segment seg(b).
struct KlBwdSegs {
  const float *mu[kMaxSegs], *rho[kMaxSegs], *pmu[kMaxSegs], *psig[kMaxSegs];
  float *dmu[kMaxSegs], *drho[kMaxSegs];
  SegTable t;
  int laplace;
};
inline uint64_t digest_arg(uint64_t h, const KlBwdSegs& a) { return digest_arg(digest_segs(h, a.t, a.mu, a.rho, a.pmu, a.psig, a.dmu, a.drho), a.laplace); }
static_assert(sizeof(KlSegs) <= kMaxSegArgBytes && sizeof(KlBwdSegs) <= kMaxSegArgBytes, "argument block larger than kl_hier_bwd_kernel's");
constexpr int kKlBwdElemsPerBlock = 1024;

__global__ __launch_bounds__(256) void kl_normal_bwd_segs_kernel(const KlBwdSegs a, const float* __restrict__ gup) {
  int seg, nb, lb;
  seg_locate(a.t, seg, nb, lb);   // uniform
  const long long n = a.t.n[seg];
  const float gs = gup[0] / (float)n;
  const float *mu = a.mu[seg], *rho = a.rho[seg], *pmu = a.pmu[seg], *psig = a.psig[seg];
  float *dmu = a.dmu[seg], *drho = a.drho[seg];
  const long long base = (long long)lb * kKlBwdElemsPerBlock;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i = base + threadIdx.x + 256 * k;
    if (i < n) kl_elem_grad(mu[i], rho[i], pmu, psig, i, a.laplace, gs, dmu[i], drho[i]);
  }
}

}  // namespace bt

extern "C" int bt_kl_normal(int32_t n_segments, const float* const* mu, const float* const* rho, const float* const* prior_mu,
                            const float* const* prior_sigma, const int64_t* numel, const int32_t* layer_of_segment, uint32_t flags,
                            float* kl_out, void* workspace, size_t workspace_bytes, bt_stream_t stream) {
  using namespace bt;
  if (n_segments <= 0 || n_segments > BT_KL_MAX_SEGMENTS) return set_error(BT_ERR_BAD_ARG, "bt_kl_normal: n_segments must be in [1, 64]");
  if (!mu || !rho || !prior_mu || !prior_sigma || !numel || !kl_out) return set_error(BT_ERR_BAD_ARG, "bt_kl_normal: null argument");
  if (!workspace || workspace_bytes < BT_WORKSPACE_BYTES) return set_error(BT_ERR_WORKSPACE, "bt_kl_normal: workspace smaller than BT_WORKSPACE_BYTES");
  KlSegs sg = {};
  for (int i = 0; i < n_segments; ++i) {
    if (numel[i] <= 0 || !mu[i] || !rho[i] || !prior_mu[i] || !prior_sigma[i]) return set_error(BT_ERR_BAD_ARG, "bt_kl_normal: empty or null segment");
    sg.mu[i] = mu[i], sg.rho[i] = rho[i], sg.pmu[i] = prior_mu[i], sg.psig[i] = prior_sigma[i], sg.t.n[i] = numel[i];
  }
  sg.rho_is_sigma = (flags & BT_KL_RHO_IS_SIGMA) ? 1 : 0;
  sg.laplace = (flags & BT_KL_PRIOR_LAPLACE) ? 1 : 0;
  if (int rc = seg_layers(sg.t, n_segments, layer_of_segment, "bt_kl_normal")) return rc;
  const int blocks = seg_partition(sg.t, n_segments, numel, kKlElemsPerBlock, kKlMaxBlocksPerSeg, kMaxSlots, "bt_kl_normal");   // (a slot per block)
  if (blocks < 0) return blocks;
  return launch_kernel(kl_normal_kernel, nullptr, "bt_kl_normal", dim3(blocks), dim3(kKlThreads), 0, 0, (hipStream_t)stream, sg, kl_out, ws_slots(workspace),
                       ws_counter(workspace), blocks);
}

extern "C" int bt_kl_normal_bwd(const float* mu, const float* rho, const float* prior_mu, const float* prior_sigma, const float* grad_kl, int64_t numel,
                                uint32_t flags, float* dmu, float* drho, bt_stream_t stream) {
  using namespace bt;
  if (!mu || !rho || !grad_kl || !dmu || !drho || numel <= 0) return set_error(BT_ERR_BAD_ARG, "bt_kl_normal_bwd: null argument");
  const int lap = (flags & BT_KL_PRIOR_LAPLACE) ? 1 : 0;
  if (!lap && (!prior_mu || !prior_sigma)) return set_error(BT_ERR_BAD_ARG, "bt_kl_normal_bwd: priors are required for the normal prior");
  const long long nb = (numel + 255) / 256;
  return launch_kernel(kl_normal_bwd_kernel, nullptr, "bt_kl_normal_bwd", dim3((unsigned)(nb > 4096 ? 4096 : nb)), dim3(256), 0, 0, (hipStream_t)stream, mu, rho, prior_mu,
                       prior_sigma, grad_kl, (long long)numel, lap, dmu, drho);
}

extern "C" int bt_kl_normal_bwd_segs(int32_t n_segments, const float* const* mu, const float* const* rho, const float* const* prior_mu,
                                     const float* const* prior_sigma, const int64_t* numel, const float* grad_kl, uint32_t flags,
                                     float* const* dmu, float* const* drho, bt_stream_t stream) {
  using namespace bt;
  if (n_segments <= 0 || n_segments > BT_KL_MAX_SEGMENTS || !mu || !rho || !numel || !grad_kl || !dmu || !drho)
    return set_error(BT_ERR_BAD_ARG, "bt_kl_normal_bwd_segs: bad argument");
  const int lap = (flags & BT_KL_PRIOR_LAPLACE) ? 1 : 0;
  if (!lap && (!prior_mu || !prior_sigma)) return set_error(BT_ERR_BAD_ARG, "bt_kl_normal_bwd_segs: priors are required for the normal prior");
  KlBwdSegs a = {};
  int i = 0;   // (stops at the first bad segment: the partition's refusal of the segments in front of it comes first)
  for (; i < n_segments; ++i) {
    if (!mu[i] || !rho[i] || !dmu[i] || !drho[i] || numel[i] <= 0 || (!lap && (!prior_mu[i] || !prior_sigma[i]))) break;
    a.mu[i] = mu[i], a.rho[i] = rho[i], a.pmu[i] = lap ? nullptr : prior_mu[i], a.psig[i] = lap ? nullptr : prior_sigma[i];
    a.dmu[i] = dmu[i], a.drho[i] = drho[i], a.t.n[i] = numel[i];
  }
  const int blocks = seg_partition(a.t, i, numel, kKlBwdElemsPerBlock, 0, 0, "bt_kl_normal_bwd_segs");
  if (blocks < 0) return blocks;
  if (i < n_segments) return set_error(BT_ERR_BAD_ARG, "bt_kl_normal_bwd_segs: null tensor or empty segment");
  a.laplace = lap;
  return launch_kernel(kl_normal_bwd_segs_kernel, nullptr, "bt_kl_normal_bwd_segs", dim3((unsigned)blocks), dim3(256), 0, 0, (hipStream_t)stream, a, grad_kl);
}
