#include "bt_fused_dispatch.h"
namespace bt {
int launch_reparam(bool linear, const FwdArgs& a, FwdArgs& ran, hipStream_t stream) {
  // (a Linear layer is a 1x1 convolution over 1x1 images: the same memory layout)
  const int rc = launch_split(a, ran, stream);
  if (rc <= 0) return rc;
  return launch_flavour<false, false>(linear, a, ran, stream);
}
}  // namespace bt
