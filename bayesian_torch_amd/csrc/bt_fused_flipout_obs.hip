// Calibration of the INT8 Flipout layers: the activation-side observers of the reference's twelve-observer prepare() / calibrate /
// convert() flow (flipout_layers/conv_flipout.py:339-345, :419-434; linear_flipout.py:115-118, :178-191) with the statistics kept on the
// device. The reference materialises the two partial outputs and both sign tensors and hands them to MinMaxObservers on the CPU; here
//   * the observing two-contraction launch (launch_flipout_obs: fused_fwd_kernel's OBS form, bt_fused_fwd.h) repeats both contractions
//     of the float Flipout forward on the fp32 general kernel, with the forward's draws, and merges the ranges of the mean output, the
//     perturbation output, the perturbation output times sign_out, and sign_out; nothing output-sized is written;
//   * the input-side sweep (bt_q8_flip_observe_x: x, sign_in, x * sign_in) and the weight side (bt_q8_observe_w) are element sweeps
//     and live with the third one in bt_q8_observe.hip; the merge is bt_observe.h's.
#include "bt_fused_dispatch.h"

namespace bt {

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

}  // namespace bt
