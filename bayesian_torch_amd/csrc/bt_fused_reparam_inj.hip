#include "bt_fused_dispatch.h"
namespace bt {
int launch_reparam_inj(bool linear, const FwdArgs& a, FwdArgs& ran, hipStream_t stream) { return run_fp32<false, true>(linear, a, ran, stream); }
}  // namespace bt
