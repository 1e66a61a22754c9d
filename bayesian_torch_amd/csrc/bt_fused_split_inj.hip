// The split-precision kernels with INJECTED draws (bt_draws.rng.flags & BT_DRAWS_EPS_PACKED): the INJ instantiations of the general,
// quad, direct and skinny kernels, in a translation unit of their own so the build stays parallel. Flavour and geometry are chosen by
// bt_fused_split.hip exactly as for on-chip draws; a kernel's name is its on-chip twin's plus the `inj` marker.
#include "bt_fused_split_quad.h"
#include "bt_fused_split_direct.h"
#include "bt_fused_split_skinny.h"
#include "bt_fused_split_host.h"

namespace bt {

template <int BM, int NPW, int XM, int BN = 64>
static int launch_inj_cfg(const FwdArgs& a, hipStream_t stream) {
  constexpr int lds = split_lds_bytes<BN, BM, 3>();
  static_assert(lds <= 160 * 1024, "LDS budget of one CU");
  char nm[160];
  snprintf(nm, sizeof(nm), "fused_split_kernel<%d,%d,bf16x3,6 terms,npw=%d,xm=%d,inj>", BN, BM, NPW, XM);
  return launch_kernel(fused_split_kernel<BN, BM, 3, NPW, XM, false, true>, nm, "fused forward (split, injected)", dim3((unsigned)a.total_blocks),
                       dim3(256 + 64 * NPW), lds, lds, stream, a);
}

// (tile width, x fetch mode) -> instantiation: the table of launch_split_xm (bt_fused_split.hip), exact split only
int launch_split_inj_cfg(const FwdArgs& a, int bm, int xm, hipStream_t stream) {
  if (bm == 128) {
    if (a.bn32) {
      if (xm == 1) return launch_inj_cfg<128, 8, 1, 32>(a, stream);
      if (xm == 2) return launch_inj_cfg<128, 8, 2, 32>(a, stream);
      return launch_inj_cfg<128, 8, 0, 32>(a, stream);
    }
    if (xm == 1) return launch_inj_cfg<128, 8, 1>(a, stream);
    if (xm == 2) return launch_inj_cfg<128, 8, 2>(a, stream);
    return launch_inj_cfg<128, 8, 0>(a, stream);
  }
  if (bm == 256) {
    if (xm == 3) return launch_inj_cfg<256, 8, 3>(a, stream);
    if (xm == 4) return launch_inj_cfg<256, 8, 4>(a, stream);
    if (xm == 2) return launch_inj_cfg<256, 8, 2>(a, stream);
    return launch_inj_cfg<256, 8, 0>(a, stream);
  }
  if (xm == 3) return launch_inj_cfg<512, 4, 3>(a, stream);
  if (xm == 4) return launch_inj_cfg<512, 4, 4>(a, stream);
  return launch_inj_cfg<512, 4, 0>(a, stream);
}

// the stems: one sample per workgroup, with or without the fused max-pool
int launch_quad_inj(const FwdArgs& a, hipStream_t stream) {
  constexpr int lds = split_lds_bytes<64, 512, 3>();
  auto launch = [&](auto kern, const char* nm) {
    return launch_kernel(kern, nm, "fused forward (split, quad, injected)", dim3((unsigned)a.total_blocks), dim3(512), lds, lds, stream, a);
  };
  if (a.ep_pool) return launch(fused_split_quad_kernel<3, true, false, false, true>, "fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=1,inj>");
  return launch(fused_split_quad_kernel<3, false, false, false, true>, "fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=0,inj>");
}

int launch_direct_inj(const FwdArgs& a, bool resident, hipStream_t stream) {
  auto launch = [&](auto kern, const char* nm, int max_lds) {
    return launch_kernel(kern, nm, "fused forward (split, direct, injected)", dim3((unsigned)a.total_blocks), dim3(kDirectThreads), direct_lds_bytes(a.Cig),
                         max_lds, stream, a);
  };
  if (resident) return launch(fused_split_direct_kernel<true, true>, "fused_split_direct_kernel<64,8x64,bf16x3,6 terms,resident W,inj>", direct_lds_bytes(kDirectMaxK));
  return launch(fused_split_direct_kernel<false, true>, "fused_split_direct_kernel<64,8x64,bf16x3,6 terms,streamed W,inj>", direct_lds_bytes(kDirectMaxK + 1));
}

int launch_skinny_inj(const FwdArgs& a, int ks, hipStream_t stream) {
  return launch_kernel(fused_split_skinny_kernel<true>,
                       ks == 128 ? "fused_split_skinny_kernel<64,4x32,bf16x3,6 terms,split-K 128,inj>" : "fused_split_skinny_kernel<64,4x32,bf16x3,6 terms,split-K 64,inj>",
                       "fused forward (split, skinny, injected)", dim3((unsigned)a.total_blocks), dim3(kSkinnyThreads), skinny_lds_bytes(ks), skinny_lds_bytes(128),
                       stream, a);
}

}  // namespace bt
