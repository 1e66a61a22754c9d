// The split-precision kernels with INJECTED draws (bt_draws.rng.flags & BT_DRAWS_EPS_PACKED): the INJ instantiations of the general,
// quad, direct and skinny kernels, in a translation unit of their own so the build stays parallel. Flavour and geometry are chosen by
// bt_fused_split.hip exactly as for on-chip draws; a kernel's name is its on-chip twin's plus the `inj` marker. Exact split only.
#include "bt_fused_split_launch.h"

namespace bt {

int launch_split_inj_cfg(const FwdArgs& a, int bm, int xm, hipStream_t stream) { return launch_split_general<3, false, true>(a, bm, xm, stream); }
int launch_quad_inj(const FwdArgs& a, hipStream_t stream) { return launch_split_quad<3, false, true>(a, stream); }   // (one sample per workgroup)
int launch_direct_inj(const FwdArgs& a, bool resident, hipStream_t stream) { return launch_split_direct<3, true>(a, resident, stream); }
int launch_skinny_inj(const FwdArgs& a, int ks, hipStream_t stream) { return launch_split_skinny<true>(a, ks, stream); }

}  // namespace bt
