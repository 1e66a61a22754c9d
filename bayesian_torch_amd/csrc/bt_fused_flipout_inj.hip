#include "bt_fused_dispatch.h"
namespace bt {
int launch_flipout_inj(bool linear, const FwdArgs& a, FwdArgs& ran, hipStream_t stream) { return run_fp32<true, true>(linear, a, ran, stream); }
}  // namespace bt
