#include "bt_fused_dispatch.h"
namespace bt {
int launch_reparam_inj(bool linear, const FwdArgs& a, FwdArgs& ran, hipStream_t stream) { return launch_flavour<false, true>(linear, a, ran, stream); }
}  // namespace bt
