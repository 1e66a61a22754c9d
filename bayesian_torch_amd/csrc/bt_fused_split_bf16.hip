// The split-precision kernels in the bf16 contraction mode (bt_set_contraction(3) / BT_CONTRACTION=bf16): the NP = 1 instantiations
// of the general, stem (quad) and direct kernels, in a translation unit of their own so the build stays parallel. Every operand
// value is rounded ONCE to bf16 (nearest even), one MFMA term per K16 step, fp32 accumulation; the sampled weight is formed in fp32
// exactly as in the exact split and then rounded. Flavour, tile plan, K order, draw streams, bias draw, output stage and KL sweep
// are chosen and run by bt_fused_split.hip exactly as in the automatic mode; a kernel's name is its exact twin's with
// `bf16x1,1 terms` where that one carries `bf16x3,6 terms`. Reparameterization with on-chip draws only: no stem sample walk
// (launch_quad plans the one-sample path in this mode), no skinny split-K kernel, no injected instantiations. The general kernel's
// LDS is one piece per value (or one 32-channel staging pass, where that is larger); the stem kernel keeps the exact split's.
#include "bt_fused_split_launch.h"

namespace bt {

int launch_split_bf16_cfg(const FwdArgs& a, int bm, int xm, hipStream_t stream) { return launch_split_general<1, false, false>(a, bm, xm, stream); }
int launch_quad_bf16(const FwdArgs& a, hipStream_t stream) { return launch_split_quad<1, false, false>(a, stream); }
int launch_direct_bf16(const FwdArgs& a, bool resident, hipStream_t stream) { return launch_split_direct<1, false>(a, resident, stream); }

}  // namespace bt
