// Calibration of the INT8 layers (layers/_quantized.py): the seven MinMaxObservers of the reference's post-training flow
// (layers/variational_layers/conv_variational.py:331-337, :387-397; the same in linear_variational.py) as two sweeps that keep their
// statistics on the device, and the input-side sweep of the Flipout layers' twelve (flipout_layers/conv_flipout.py:339-345, :419-434). The reference materialises sigma, eps, sigma * eps and mu + sigma * eps as weight-sized tensors on the CPU
// and hands seven tensors to seven observers; here
//   * bt_q8_observe_w reads (mu, rho) once per sample, regenerates the sample's draws from the call's RNG coordinates (or reads the
//     supplied ones) and merges the ranges of q = sigma * coef, m = mu * coef, eps, t = q * eps and w = m + t -- the five qint8 stubs
//     in the reference's order -- into stats[10]; nothing weight-sized is written;
//   * bt_minmax_update merges the ranges of up to four fp32 tensors (a layer's input and output) into (min, max) pairs;
//   * bt_q8_flip_observe_x sweeps x once per sample and merges the ranges of x, sign_in and x * sign_in.
// The reduction, the (min, max) pair, the merge, the walk over one fp32 run and the host helpers: bt_observe.h.
#include "bt_observe.h"

namespace bt {

constexpr int kObsStats = 5;   // sigma, mu, eps, mul, add

// One weight: each product and the sum ONE fp32 rounding, as quantize() (mu * coef, sigma * coef) and the float forward
// (sigma * eps, mu + sigma * eps) form them.
__device__ __forceinline__ void obs_weight(float mu, float rho, float c, float eps, Range (&r)[kObsStats], unsigned& bad) {
  const float q = __fmul_rn(softplus(rho), c);
  const float m = __fmul_rn(mu, c);
  const float t = __fmul_rn(q, eps);
  const float w = __fadd_rn(m, t);
  r[0].take(q, bad), r[1].take(m, bad), r[2].take(eps, bad), r[3].take(t, bad), r[4].take(w, bad);
}

struct ObsWArgs {
  const float* mu;
  const float* rho;
  const float* coef;   // [rows] or null (1)
  const float* eps;    // [S][n] or null: the tensor 0 stream of `key`
  float* stats;        // [5][2]
  unsigned* nonfinite;
  const uint32_t* call_base;
  RngKey key;
  uint32_t sample0;
  long long rows, inner, taps, n;
};

// A thread per four consecutive elements of the weight's natural order, of sample blockIdx.y: 16-byte loads where mu, rho (and this
// sample's supplied eps) are all 16-byte aligned, element by element for the last n & 3 elements and where they are not. kRng: the
// element's draw is regenerated instead -- number e & 3 of Philox block e >> 2 of the tensor 0 stream, e = eps_stream_index(row,
// channel, tap), the rule bt_rng_normal_fill materialises; consecutive taps of one channel lie in different blocks (the stream is
// tap-major), so a 3 x 3 kernel runs one Philox block per element and a Linear layer one per four. The loads stay coalesced either way.
template <bool kRng>
__global__ __launch_bounds__(kObsThreads) void q8_observe_w_kernel(ObsWArgs a) {
  __shared__ float lds[4 * (2 * kObsStats + 1)];
  const float* const eps = kRng ? nullptr : a.eps + (long long)blockIdx.y * a.n;
  RngKey k = a.key;
  if (kRng && a.call_base) k.call += *a.call_base;
  const uint32_t sample = a.sample0 + blockIdx.y;
  const long long per_row = a.inner * a.taps, inner4 = (a.inner + 3) & ~3ll;
  const int taps = (int)a.taps, inner = (int)a.inner;
  const bool quads = ((((uintptr_t)a.mu) | ((uintptr_t)a.rho) | ((uintptr_t)eps)) & 15u) == 0;
  const long long n4 = (a.n + 3) >> 2;
  Range r[kObsStats];
  unsigned bad = 0;
  obs_init(r);
  for (long long g = (long long)blockIdx.x * kObsThreads + threadIdx.x; g < n4; g += (long long)gridDim.x * kObsThreads) {
    const long long i0 = g * 4;
    const int cnt = a.n - i0 < 4 ? (int)(a.n - i0) : 4;
    float m[4] = {0.f, 0.f, 0.f, 0.f}, rr[4] = {0.f, 0.f, 0.f, 0.f}, e[4] = {0.f, 0.f, 0.f, 0.f};
    if (quads && cnt == 4) {
      const float4 m4 = *reinterpret_cast<const float4*>(a.mu + i0);
      const float4 r4 = *reinterpret_cast<const float4*>(a.rho + i0);
      m[0] = m4.x, m[1] = m4.y, m[2] = m4.z, m[3] = m4.w;
      rr[0] = r4.x, rr[1] = r4.y, rr[2] = r4.z, rr[3] = r4.w;
      if (!kRng) {
        const float4 e4 = *reinterpret_cast<const float4*>(eps + i0);
        e[0] = e4.x, e[1] = e4.y, e[2] = e4.z, e[3] = e4.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) {
          m[j] = a.mu[i0 + j], rr[j] = a.rho[i0 + j];
          if (!kRng) e[j] = eps[i0 + j];
        }
    }
    long long row = i0 / per_row;                       // (per_row < 2^31: the rest is 32-bit)
    const int rem = (int)(i0 - row * per_row);
    int c = rem / taps, t = rem - c * taps;
    long long blk = -1;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) {
        if (kRng) {
          const long long el = eps_stream_index(row, c, t, inner4, taps);
          if ((el >> 2) != blk) {
            blk = el >> 2;
            philox_normal4(k, sample, (uint32_t)blk, z);
          }
          const int w = (int)(el & 3);
          e[j] = w == 0 ? z[0] : w == 1 ? z[1] : w == 2 ? z[2] : z[3];
        }
        obs_weight(m[j], rr[j], a.coef ? a.coef[row] : 1.0f, e[j], r, bad);
        if (++t == taps) {
          t = 0;
          if (++c == inner) c = 0, ++row;
        }
      }
  }
  float* const dst[kObsStats] = {a.stats, a.stats + 2, a.stats + 4, a.stats + 6, a.stats + 8};
  obs_merge<kObsStats>(r, bad, dst, a.nonfinite, lds);
}

struct MinMaxArgs {
  const float* x[BT_MINMAX_MAX_SEGS];
  long long n[BT_MINMAX_MAX_SEGS];
  float* dst[BT_MINMAX_MAX_SEGS];
  unsigned* nonfinite;
};

// Segment blockIdx.y, walked as obs_walk walks a run.
__global__ __launch_bounds__(kObsThreads) void minmax_update_kernel(MinMaxArgs a) {
  __shared__ float lds[4 * 3];
  const int sg = blockIdx.y;
  Range r[1];
  unsigned bad = 0;
  obs_init(r);
  obs_walk(
      a.x[sg], a.n[sg], [&](long long, float v) { r[0].take(v, bad); },
      [&](long long, float4 v) { r[0].take(v.x, bad), r[0].take(v.y, bad), r[0].take(v.z, bad), r[0].take(v.w, bad); });
  float* const dst[1] = {a.dst[sg]};
  obs_merge<1>(r, bad, dst, a.nonfinite, lds);
}

struct ObsXArgs {
  const float* x;
  const float* sign_in;   // [S][n] or null: tensor 2's stream of `key`
  float* dst[3];          // (min, max) of x, sign_in, x * sign_in
  unsigned* nonfinite;
  const uint32_t* call_base;
  RngKey key;             // tensor 2
  uint32_t sample0;
  long long n, x_sample_stride;
};

// Sample blockIdx.y's x, walked as obs_walk walks a run; supplied signs are read as 16-byte loads too where they share x's alignment.
// kRng: the sign of element i is hash_sign of the sample's tensor 2 stream at i, the element's offset within ONE sample's tensor, as
// the forward indexes it.
template <bool kRng>
__global__ __launch_bounds__(kObsThreads) void q8_flip_observe_x_kernel(ObsXArgs a) {
  __shared__ float lds[(kObsThreads / 64) * 7];
  const int s = blockIdx.y;
  const float* const x = a.x + (long long)s * a.x_sample_stride;
  const float* const sg = kRng ? nullptr : a.sign_in + (long long)s * a.n;
  uint32_t skey = 0;
  if (kRng) {
    RngKey k = a.key;
    if (a.call_base) k.call += *a.call_base;
    skey = sign_stream_key(k, a.sample0 + (uint32_t)s);
  }
  const bool sg_quads = !kRng && ((((uintptr_t)sg) ^ ((uintptr_t)x)) & 15u) == 0;   // x's quads are the signs' quads
  Range r[3];
  unsigned bad = 0;
  obs_init(r);
  auto take = [&](float v, float sn) { r[0].take(v, bad), r[1].take(sn, bad), r[2].take(__fmul_rn(v, sn), bad); };
  auto sign_of = [&](long long i) -> float { return kRng ? hash_sign(skey, (uint32_t)i) : obs_sign(sg[i]); };
  obs_walk(
      x, a.n, [&](long long i, float v) { take(v, sign_of(i)); },
      [&](long long i0, float4 v) {
        float sn[4];
        if (sg_quads) {
          const float4 s4 = *reinterpret_cast<const float4*>(sg + i0);
          sn[0] = obs_sign(s4.x), sn[1] = obs_sign(s4.y), sn[2] = obs_sign(s4.z), sn[3] = obs_sign(s4.w);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) sn[j] = sign_of(i0 + j);
        }
        take(v.x, sn[0]), take(v.y, sn[1]), take(v.z, sn[2]), take(v.w, sn[3]);
      });
  float* const dst[3] = {a.dst[0], a.dst[1], a.dst[2]};
  obs_merge<3>(r, bad, dst, a.nonfinite, lds);
}

static const char* const kMinMaxNames[BT_MINMAX_MAX_SEGS] = {"minmax_update<1 segs>", "minmax_update<2 segs>", "minmax_update<3 segs>", "minmax_update<4 segs>"};

}  // namespace bt

extern "C" int bt_q8_observe_w(const float* mu, const float* rho, const float* coef, int64_t rows, int64_t inner, int64_t taps, int32_t S, const float* eps,
                               const bt_rng* rng, float* stats, uint32_t* nonfinite, bt_stream_t stream) {
  using namespace bt;
  if (!mu || !rho || !stats || !nonfinite) return set_error(BT_ERR_BAD_ARG, "bt_q8_observe_w: null mu / rho / stats / nonfinite");
  if (S < 1 || rows < 1 || inner < 1 || taps < 1) return set_error(BT_ERR_BAD_ARG, "bt_q8_observe_w: S < 1 or an empty weight tensor (n < 1)");
  if (!eps == !rng) return set_error(BT_ERR_BAD_ARG, "bt_q8_observe_w: exactly one draw source, eps or rng");
  if (!obs_aligned4(mu, rho, coef, eps, stats, nonfinite)) return set_error(BT_ERR_BAD_ARG, "bt_q8_observe_w: a pointer that is not 4-byte aligned");
  if (S > 65535 || rows >= (1ll << 31) || inner >= (1ll << 31) || taps >= (1ll << 31)) return set_error(BT_ERR_UNSUPPORTED, "bt_q8_observe_w: S > 65535 or tensor too large");
  const long long nq = (long long)rows * taps * (((long long)inner + 3) >> 2);
  if ((long long)inner * taps >= (1ll << 31) || (long long)rows * inner >= (1ll << 40) / taps || nq > (1ll << 32)) return set_error(BT_ERR_UNSUPPORTED, "bt_q8_observe_w: weight tensor too large for the draw stream");
  ObsWArgs a = {};
  a.mu = mu, a.rho = rho, a.coef = coef, a.eps = eps, a.stats = stats, a.nonfinite = nonfinite;
  a.rows = rows, a.inner = inner, a.taps = taps, a.n = (long long)rows * inner * taps;
  if (rng) a.call_base = rng->call_base_dev, a.key = make_key(*rng, 0), a.sample0 = rng->sample0;
  return obs_launch(rng != nullptr, q8_observe_w_kernel<true>, "q8_observe_w<eps on chip>", q8_observe_w_kernel<false>, "q8_observe_w<eps injected>",
                    "bt_q8_observe_w", obs_grid(a.n, S, obs_cap(S)), stream, a);
}

extern "C" int bt_minmax_update(int32_t n_segs, const bt_minmax_seg* segs, uint32_t* nonfinite, bt_stream_t stream) {
  using namespace bt;
  if (n_segs < 1 || n_segs > BT_MINMAX_MAX_SEGS) return set_error(BT_ERR_BAD_ARG, "bt_minmax_update: 1 to 4 segments");
  if (!segs || !nonfinite || !obs_aligned4(nonfinite)) return set_error(BT_ERR_BAD_ARG, "bt_minmax_update: null segs / nonfinite");
  MinMaxArgs a = {};
  long long most = 0;
  for (int i = 0; i < BT_MINMAX_MAX_SEGS; ++i) {
    const bt_minmax_seg& s = segs[i < n_segs ? i : 0];   // (the unused slots repeat segment 0; no workgroup reads them)
    if (i < n_segs) {
      if (!s.x || !s.dst || s.n < 1) return set_error(BT_ERR_BAD_ARG, "bt_minmax_update: a segment with a null pointer or n < 1");
      if (!obs_aligned4(s.x, s.dst)) return set_error(BT_ERR_BAD_ARG, "bt_minmax_update: a pointer that is not 4-byte aligned");
      if (s.n >= (1ll << 40)) return set_error(BT_ERR_UNSUPPORTED, "bt_minmax_update: segment too large");
      if (s.n > most) most = s.n;
    }
    a.x[i] = s.x, a.n[i] = s.n, a.dst[i] = s.dst;
  }
  a.nonfinite = nonfinite;
  // (segments differ in length: the longest one's row may take the whole cap)
  return launch_kernel(minmax_update_kernel, kMinMaxNames[n_segs - 1], "bt_minmax_update", obs_grid(most, n_segs, kObsGrid), dim3(kObsThreads), 0, 0,
                       (hipStream_t)stream, a);
}

extern "C" int bt_q8_flip_observe_x(int64_t n, int32_t S, const float* x, int64_t x_sample_stride, const float* sign_in, const bt_rng* rng, float* in_mm,
                                    float* sign_in_mm, float* xp_mm, uint32_t* nonfinite, bt_stream_t stream) {
  using namespace bt;
  if (!x || !in_mm || !sign_in_mm || !xp_mm || !nonfinite) return set_error(BT_ERR_BAD_ARG, "bt_q8_flip_observe_x: null x / statistics / nonfinite");
  if (S < 1 || n < 1 || x_sample_stride < 0) return set_error(BT_ERR_BAD_ARG, "bt_q8_flip_observe_x: S < 1, n < 1 or a negative x_sample_stride");
  if (!sign_in == !rng) return set_error(BT_ERR_BAD_ARG, "bt_q8_flip_observe_x: exactly one draw source, sign_in or rng");
  if (!obs_aligned4(x, sign_in, in_mm, sign_in_mm, xp_mm, nonfinite)) return set_error(BT_ERR_BAD_ARG, "bt_q8_flip_observe_x: a pointer that is not 4-byte aligned");
  if (S > 65535 || n >= (1ll << 32)) return set_error(BT_ERR_UNSUPPORTED, "bt_q8_flip_observe_x: S > 65535 or 2^32 or more elements in one sample's x (the sign stream's index)");
  ObsXArgs a = {};
  a.x = x, a.sign_in = sign_in, a.dst[0] = in_mm, a.dst[1] = sign_in_mm, a.dst[2] = xp_mm, a.nonfinite = nonfinite;
  a.n = n, a.x_sample_stride = x_sample_stride;
  if (rng) a.call_base = rng->call_base_dev, a.key = make_key(*rng, 2), a.sample0 = rng->sample0;
  return obs_launch(rng != nullptr, q8_flip_observe_x_kernel<true>, "q8_flip_observe_x<signs on chip>", q8_flip_observe_x_kernel<false>,
                    "q8_flip_observe_x<signs injected>", "bt_q8_flip_observe_x", obs_grid(n, S, obs_cap(S)), stream, a);
}
