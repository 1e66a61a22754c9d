// Reparameterization forward over a depth-windowed input (FwdArgs::dwin: Conv3d without the depth-unfolded copy): the split-precision
// chain first (the general split kernel's xm 6 fetch), then the fp32 general kernel's DWIN instantiations for what the split tiles do
// not hold. In a translation unit of its own so the build stays parallel.
#include "bt_fused_dispatch.h"
namespace bt {
int launch_reparam_dwin(bool linear, const FwdArgs& a, FwdArgs& ran, hipStream_t stream) { return run_fp32<false, false, true, true>(linear, a, ran, stream); }
}  // namespace bt
