// The LOWRANK instantiations of fused_fwd_kernel (bt_fused_fwd.h): the low-rank multivariate weight source of bt_lowrank_conv2d_fwd, with
// on-chip and with supplied draws. A unit of its own: the mean-field instantiations carry none of it.
#include "bt_fused_dispatch.h"

namespace bt {

template <int BN, int BM, int CWN, bool TRANS, bool INJ>
static int launch_lowrank_inst(const FwdArgs& a, hipStream_t stream) {
  static_assert(fp32_exists(0, BN, BM, false, false, TRANS, true, false, 0, false), "a tile the general kernel has");
  constexpr int lds = fused_lds_bytes<BN, BM, false>();
  static_assert(lds <= 160 * 1024, "LDS budget of one CU");
  char nm[160];
  snprintf(nm, sizeof(nm), "fused_fwd_kernel<%d,%d,%d,lowrank,conv,%s,inj=%d,R=%d>", BN, BM, CWN, TRANS ? "trans" : "notrans", INJ ? 1 : 0, a.lr_R);
  return launch_kernel(fused_fwd_kernel<BN, BM, CWN, false, false, TRANS, INJ, false, false, true>, nm, "fused forward (low rank)", dim3((unsigned)a.total_blocks),
                       dim3(kThreads), lds, lds, stream, a);
}

template <int BN, int BM, int CWN>
static int launch_lowrank_tile(const FwdArgs& a, const Fp32Plan& p, bool inj, hipStream_t stream) {
  if (p.trans) return inj ? launch_lowrank_inst<BN, BM, CWN, true, true>(a, stream) : launch_lowrank_inst<BN, BM, CWN, true, false>(a, stream);
  return inj ? launch_lowrank_inst<BN, BM, CWN, false, true>(a, stream) : launch_lowrank_inst<BN, BM, CWN, false, false>(a, stream);
}

// Plans `a` (bt::run's geometry + the low-rank fields) with the fp32 planner as a launch of the general kernel -- the plan of a
// Reparameterization convolution with natural-layout supplied draws, whichever way this launch draws -- and launches the LOWRANK
// instantiation of the planned tile. The form exists for the tiles whose build holds a row of L per weight element in registers
// without scratch (64x64, 32x128, 64x128: at most 3 weight units per producer thread); where the planner names a 128-channel or a
// 256-column tile, the launch is planned again on the 64-channel tile of at most 128 columns. On BT_OK the plan that ran is in `ran`.
int launch_lowrank(const FwdArgs& a, FwdArgs& ran, hipStream_t stream) {
  Fp32Plan p;
  ran = a;
  if (int rc = fp32_plan(ran, false, false, true, false, &p)) return rc;
  const int tile = p.bn * 1024 + p.bm;
  if (tile != 64 * 1024 + 64 && tile != 32 * 1024 + 128 && tile != 64 * 1024 + 128) {
    ran = a;
    p.bn = 64, p.bm = p.bm <= 64 ? 64 : 128, p.cwn = 2;
    if (int rc = plan_tile(ran, false, true, false, false, &p)) return rc;
  }
  if (p.fast || p.linear) return set_error(BT_ERR_UNSUPPORTED, "low-rank forward: the plan names a kernel without a low-rank form");
  const bool inj = a.eps_w != nullptr;
  switch (p.bn * 1024 + p.bm) {
    case 64 * 1024 + 64: return launch_lowrank_tile<64, 64, 2>(ran, p, inj, stream);
    case 32 * 1024 + 128: return launch_lowrank_tile<32, 128, 1>(ran, p, inj, stream);
    case 64 * 1024 + 128: return launch_lowrank_tile<64, 128, 2>(ran, p, inj, stream);
  }
  return set_error(BT_ERR_UNSUPPORTED, "low-rank forward: the plan names a tile that is not instantiated");
}

}  // namespace bt
