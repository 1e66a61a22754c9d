#include "bt_fused_dispatch.h"
namespace bt {
int launch_flipout(bool linear, const FwdArgs& a, FwdArgs& ran, hipStream_t stream) {
  const int rc = launch_split_flip(a, ran, stream);
  if (rc <= 0) return rc;
  return launch_flavour<true, false>(linear, a, ran, stream);
}
}  // namespace bt
