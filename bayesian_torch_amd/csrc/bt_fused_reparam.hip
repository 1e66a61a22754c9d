#include "bt_fused_dispatch.h"
namespace bt {
int launch_reparam(bool linear, const FwdArgs& a, FwdArgs& ran, hipStream_t stream) { return run_fp32<false, false>(linear, a, ran, stream); }   // (a Linear layer is a 1x1 convolution over 1x1 images: the same memory layout)
}  // namespace bt
