// Calibration of the INT8 Flipout layers: the activation-side observers of the reference's twelve-observer prepare() / calibrate /
// convert() flow (flipout_layers/conv_flipout.py:339-345, :419-434; linear_flipout.py:115-118, :178-191) with the statistics kept on the
// device. The reference materialises the two partial outputs and both sign tensors and hands them to MinMaxObservers on the CPU; here
//   * the observing two-contraction launch (launch_flipout_obs: fused_fwd_kernel's OBS form, bt_fused_fwd.h) repeats both contractions
//     of the float Flipout forward on the fp32 general kernel, with the forward's draws, and merges the ranges of the mean output, the
//     perturbation output, the perturbation output times sign_out, and sign_out; nothing output-sized is written;
//   * bt_q8_flip_observe_x sweeps x once per sample and merges the ranges of x, sign_in and x * sign_in.
// The weight side is bt_q8_observe_w's (bt_q8_observe.hip), unchanged; the merge is bt_observe.h's.
#include "bt_fused_dispatch.h"

namespace bt {

// ---------------------------------------------------------------------------- the observing two-contraction launch
// ONE tile, 64 output channels x 64 output positions: calibration runs a handful of times per model, so the launch is planned for
// the tile every geometry can take and not for speed. Planned as a launch with supplied natural-layout draws is (always the general
// kernel), whichever the draw source.
template <bool LINEAR, bool TRANS, bool INJ>
static int launch_obs_inst(const FwdArgs& a, hipStream_t stream) {
  constexpr int BN = 64, BM = 64, CWN = 2;
  constexpr int lds = fused_lds_bytes<BN, BM, true>();
  static_assert(lds <= 160 * 1024, "LDS budget of one CU");
  static_assert(4 * BN + (kThreads / 64) * 9 <= 2 * 2 * (kBK * (BN + 1) + x_words<BM, true>()), "the merge's words lie inside the stage memory");
  char nm[160];
  snprintf(nm, sizeof(nm), "fused_fwd_kernel<%d,%d,%d,flip,%s,%s,inj=%d,obs>", BN, BM, CWN, LINEAR ? "linear" : "conv", TRANS ? "trans" : "notrans", INJ ? 1 : 0);
  return launch_kernel(fused_fwd_kernel<BN, BM, CWN, true, LINEAR, TRANS, INJ, false, false, false, true>, nm, "bt_q8_flip_observe", dim3((unsigned)a.total_blocks),
                       dim3(kThreads), lds, lds, stream, a);
}

template <bool INJ>
static int launch_obs_form(const FwdArgs& a, const Fp32Plan& p, hipStream_t stream) {
  if (p.linear) return launch_obs_inst<true, true, INJ>(a, stream);
  if (p.trans) return launch_obs_inst<false, true, INJ>(a, stream);
  return launch_obs_inst<false, false, INJ>(a, stream);
}

int launch_flipout_obs(bool linear, const FwdArgs& a, FwdArgs& ran, hipStream_t stream) {
  Fp32Plan p;
  ran = a;
  p.linear = linear && ran.w_vec && ran.x_vec;   // float4 rows; any other Linear is a 1x1 conv over 1x1 images (fp32_plan)
  p.trans = p.linear || ran.HoWo == 1 || ran.pixel_major;
  p.bn = 64, p.bm = 64, p.cwn = 2;
  if (int rc = plan_tile(ran, true, true, false, false, &p)) return rc;
  if (p.fast) return set_error(BT_ERR_UNSUPPORTED, "bt_q8_flip_observe: the plan left the general kernel");
  return ran.eps_w ? launch_obs_form<true>(ran, p, stream) : launch_obs_form<false>(ran, p, stream);
}

// ---------------------------------------------------------------------------- the input-side sweep
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

// Sample blockIdx.y: the elements before x's first 16-byte boundary one by one, whole quads as 16-byte loads (the supplied signs too
// where they share x's alignment), the rest one by one. kRng: the sign of element i is hash_sign of the sample's tensor 2 stream at i,
// the element's offset within ONE sample's tensor, as the forward indexes it.
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
  const long long n = a.n;
  long long head = (long long)(((16u - (unsigned)(((uintptr_t)x) & 15u)) & 15u) >> 2);
  if (head > n) head = n;
  const long long nquad = (n - head) >> 2;
  const long long tail0 = head + 4 * nquad;
  const bool sg_quads = kRng || ((((uintptr_t)(sg + head)) & 15u) == 0);
  Range r[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k].lo = INFINITY, r[k].hi = -INFINITY;
  unsigned bad = 0;
  auto one = [&](float v, float sn) {
    r[0].take(v, bad), r[1].take(sn, bad), r[2].take(__fmul_rn(v, sn), bad);
  };
  auto sign_of = [&](long long i) -> float { return kRng ? hash_sign(skey, (uint32_t)i) : obs_sign(sg[i]); };
  const long long tid = (long long)blockIdx.x * kObsThreads + threadIdx.x, stride = (long long)gridDim.x * kObsThreads;
  const float4* const x4 = reinterpret_cast<const float4*>(x + head);
  for (long long g = tid; g < nquad; g += stride) {
    const float4 v = x4[g];
    const long long i0 = head + 4 * g;
    float sn[4];
    if (!kRng && sg_quads) {
      const float4 s4 = *reinterpret_cast<const float4*>(sg + i0);
      sn[0] = obs_sign(s4.x), sn[1] = obs_sign(s4.y), sn[2] = obs_sign(s4.z), sn[3] = obs_sign(s4.w);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) sn[j] = sign_of(i0 + j);
    }
    one(v.x, sn[0]), one(v.y, sn[1]), one(v.z, sn[2]), one(v.w, sn[3]);
  }
  if (tid < head) one(x[tid], sign_of(tid));                                   // head < 4
  if (tid < n - tail0) one(x[tail0 + tid], sign_of(tail0 + tid));              // n - tail0 < 4
  float* const dst[3] = {a.dst[0], a.dst[1], a.dst[2]};
  obs_merge<3>(r, bad, dst, a.nonfinite, lds);
}

}  // namespace bt

extern "C" int bt_q8_flip_observe_x(int64_t n, int32_t S, const float* x, int64_t x_sample_stride, const float* sign_in, const bt_rng* rng, float* in_mm,
                                    float* sign_in_mm, float* xp_mm, uint32_t* nonfinite, bt_stream_t stream) {
  using namespace bt;
  if (!x || !in_mm || !sign_in_mm || !xp_mm || !nonfinite) return set_error(BT_ERR_BAD_ARG, "bt_q8_flip_observe_x: null x / statistics / nonfinite");
  if (S < 1 || n < 1 || x_sample_stride < 0) return set_error(BT_ERR_BAD_ARG, "bt_q8_flip_observe_x: S < 1, n < 1 or a negative x_sample_stride");
  if (!sign_in == !rng) return set_error(BT_ERR_BAD_ARG, "bt_q8_flip_observe_x: exactly one draw source, sign_in or rng");
  if ((((uintptr_t)x) | ((uintptr_t)sign_in) | ((uintptr_t)in_mm) | ((uintptr_t)sign_in_mm) | ((uintptr_t)xp_mm) | ((uintptr_t)nonfinite)) & 3u)
    return set_error(BT_ERR_BAD_ARG, "bt_q8_flip_observe_x: a pointer that is not 4-byte aligned");
  if (S > 65535 || n >= (1ll << 32)) return set_error(BT_ERR_UNSUPPORTED, "bt_q8_flip_observe_x: S > 65535 or 2^32 or more elements in one sample's x (the sign stream's index)");
  ObsXArgs a = {};
  a.x = x, a.sign_in = sign_in, a.dst[0] = in_mm, a.dst[1] = sign_in_mm, a.dst[2] = xp_mm, a.nonfinite = nonfinite;
  a.n = n, a.x_sample_stride = x_sample_stride;
  if (rng) a.call_base = rng->call_base_dev, a.key = make_key(*rng, 2), a.sample0 = rng->sample0;
  long long gx = (n + 4 * kObsThreads - 1) / (4 * kObsThreads);   // a thread takes at least one quad
  const long long cap = (kObsGrid + S - 1) / S;
  if (gx > cap) gx = cap;
  const dim3 grid((unsigned)gx, (unsigned)S);
  if (rng) return launch_kernel(q8_flip_observe_x_kernel<true>, "q8_flip_observe_x<signs on chip>", "bt_q8_flip_observe_x", grid, dim3(kObsThreads), 0, 0, (hipStream_t)stream, a);
  return launch_kernel(q8_flip_observe_x_kernel<false>, "q8_flip_observe_x<signs injected>", "bt_q8_flip_observe_x", grid, dim3(kObsThreads), 0, 0, (hipStream_t)stream, a);
}
