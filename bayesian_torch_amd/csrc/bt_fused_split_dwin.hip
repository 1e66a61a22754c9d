// The general split kernel over a depth-windowed input (bt_fused_split.h, XM 6; FwdArgs::dwin): Conv3d without the depth-unfolded
// copy. On-chip draws; the exact split and the bf16 mode of the Reparameterization, the exact split of Flipout, on every tile the
// variant has. The plan is the one split_plan made for the virtual operand (bt_fused_split.hip, bt_fused_split_flip.hip).
#include "bt_fused_split_host.h"
#include "bt_fused_split_launch.h"

namespace bt {

template <int NP, bool FLIP>
static int launch_dwin(const FwdArgs& a, int bm, hipStream_t stream) {
  if (bm == 256) return launch_split_inst<NP, FLIP, false, 64, 256, 6>(a, stream);
  if constexpr (!FLIP) {
    if (bm == 512) return launch_split_inst<NP, FLIP, false, 64, 512, 6>(a, stream);
    if (a.bn32) return launch_split_inst<NP, FLIP, false, 32, 128, 6>(a, stream);
  }
  return launch_split_inst<NP, FLIP, false, 64, 128, 6>(a, stream);
}

int launch_split_dwin_cfg(const FwdArgs& a, int bm, int np, bool flip, hipStream_t stream) {
  if (!a.dwin || a.updil || a.eps_w || (bm != 128 && bm != 256 && bm != 512) || (flip && (np != 3 || bm == 512)))
    return set_error(BT_ERR_UNSUPPORTED, "fused forward (split): no depth-window instantiation of this launch");
  if (flip) return launch_dwin<3, true>(a, bm, stream);
  if (np == 3) return launch_dwin<3, false>(a, bm, stream);
  if (np == 1) return launch_dwin<1, false>(a, bm, stream);
  return set_error(BT_ERR_UNSUPPORTED, "fused forward (split): the depth-window fetch exists for the exact split and the bf16 mode");
}

}  // namespace bt
