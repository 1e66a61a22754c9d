// Flipout forward over an input-dilated image (FwdArgs::updil): as bt_fused_reparam_updil.hip, for the Flipout chain.
#include "bt_fused_dispatch.h"
namespace bt {
int launch_flipout_updil(const FwdArgs& a, FwdArgs& ran, hipStream_t stream) {
  const int rc = launch_split_flip(a, ran, stream);
  if (rc <= 0) return rc;
  return launch_flavour_updil<true>(a, ran, stream);
}
}  // namespace bt
