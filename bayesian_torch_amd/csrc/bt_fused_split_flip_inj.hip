// The split-precision Flipout kernels with SUPPLIED draws and signs (bt_draws.rng.flags = BT_DRAWS_EPS_PACKED | BT_DRAWS_SIGNS_PACKED):
// the FLIP && INJ instantiations of everything launch_split_flip_one / launch_quad_flip (bt_fused_split_flip.hip) can select, in a
// translation unit of their own so the build stays parallel. Flavour and geometry are chosen there exactly as for on-chip draws; a
// kernel's name is its on-chip twin's with `,inj` before the closing bracket.
#include "bt_fused_split_quad.h"
#include "bt_fused_split_host.h"

namespace bt {

template <int BM, int NPW, int XM>
static int launch_flip_inj(const FwdArgs& a, hipStream_t stream) {
  constexpr int BN = 64, NP = 3;
  constexpr int lds = split_lds_bytes<BN, BM, NP, true>();
  static_assert(lds <= 160 * 1024, "LDS budget of one CU");
  char nm[160];
  snprintf(nm, sizeof(nm), "fused_split_kernel<%d,%d,bf16x%d,2x6 terms,flip,npw=%d,xm=%d,inj>", BN, BM, NP, NPW, XM);
  return launch_kernel(fused_split_kernel<BN, BM, NP, NPW, XM, true, true>, nm, "fused forward (split, flipout, injected)", dim3((unsigned)a.total_blocks),
                       dim3(256 + 64 * NPW), lds, lds, stream, a);
}

// (tile width, x fetch mode) -> instantiation: the table of launch_split_flip_one
int launch_split_flip_inj_cfg(const FwdArgs& a, int bm, int xm, hipStream_t stream) {
  if (bm == 256) return xm == 3 ? launch_flip_inj<256, 4, 3>(a, stream) : launch_flip_inj<256, 4, 0>(a, stream);
  if (xm == 1) return launch_flip_inj<128, 8, 1>(a, stream);
  if (xm == 2) return launch_flip_inj<128, 8, 2>(a, stream);
  return launch_flip_inj<128, 8, 0>(a, stream);
}

// the stems, with or without the fused max-pool
int launch_quad_flip_inj(const FwdArgs& a, hipStream_t stream) {
  constexpr int lds = quad_lds_bytes<true>();
  auto launch = [&](auto kern, const char* nm) {
    return launch_kernel(kern, nm, "fused forward (split, flipout, quad, injected)", dim3((unsigned)a.total_blocks), dim3(512), lds, lds, stream, a);
  };
  if (a.ep_pool) return launch(fused_split_quad_kernel<3, true, true, false, true>, "fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=1,inj>");
  return launch(fused_split_quad_kernel<3, false, true, false, true>, "fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=0,inj>");
}

}  // namespace bt
