// Flipout forward over a depth-windowed input (FwdArgs::dwin): as bt_fused_reparam_dwin.hip, for the Flipout chain.
#include "bt_fused_dispatch.h"
namespace bt {
int launch_flipout_dwin(bool linear, const FwdArgs& a, FwdArgs& ran, hipStream_t stream) { return run_fp32<true, false, true, true>(linear, a, ran, stream); }
}  // namespace bt
