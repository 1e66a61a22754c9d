// Flipout forward over an input-dilated image (FwdArgs::updil): as bt_fused_reparam_updil.hip, for the Flipout chain.
#include "bt_fused_dispatch.h"
namespace bt {
int launch_flipout_updil(bool linear, const FwdArgs& a, FwdArgs& ran, hipStream_t stream) { return run_fp32<true, false, true>(linear, a, ran, stream); }
}  // namespace bt
