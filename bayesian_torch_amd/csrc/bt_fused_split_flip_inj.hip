// The split-precision Flipout kernels with SUPPLIED draws and signs (bt_draws.rng.flags = BT_DRAWS_EPS_PACKED | BT_DRAWS_SIGNS_PACKED):
// the FLIP && INJ instantiations of everything launch_split_flip_one / launch_quad_flip (bt_fused_split_flip.hip) can select, in a
// translation unit of their own so the build stays parallel. Flavour and geometry are chosen there exactly as for on-chip draws; a
// kernel's name is its on-chip twin's with `,inj` before the closing bracket.
#include "bt_fused_split_launch.h"

namespace bt {

int launch_split_flip_inj_cfg(const FwdArgs& a, int bm, int xm, hipStream_t stream) { return launch_split_general<3, true, true>(a, bm, xm, stream); }
int launch_quad_flip_inj(const FwdArgs& a, hipStream_t stream) { return launch_split_quad<3, true, true>(a, stream); }

}  // namespace bt
