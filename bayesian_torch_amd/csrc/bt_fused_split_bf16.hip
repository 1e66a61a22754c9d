// The split-precision kernels in the bf16 contraction mode (bt_set_contraction(3) / BT_CONTRACTION=bf16): the NP = 1 instantiations
// of the general, stem (quad) and direct kernels, in a translation unit of their own so the build stays parallel. Every operand
// value is rounded ONCE to bf16 (nearest even), one MFMA term per K16 step, fp32 accumulation; the sampled weight is formed in fp32
// exactly as in the exact split and then rounded. Flavour, tile plan, K order, draw streams, bias draw, output stage and KL sweep
// are chosen and run by bt_fused_split.hip exactly as in the automatic mode; a kernel's name is its exact twin's with
// `bf16x1,1 terms` where that one carries `bf16x3,6 terms`. Reparameterization with on-chip draws only: no stem sample walk, no
// skinny split-K kernel, no injected instantiations.
#include "bt_fused_split_quad.h"
#include "bt_fused_split_direct.h"
#include "bt_fused_split_host.h"

namespace bt {

template <int BM, int NPW, int XM, int BN = 64>
static int launch_bf16_cfg(const FwdArgs& a, hipStream_t stream) {
  constexpr int lds = split_lds_bytes<BN, BM, 1>();   // one piece per value (or one 32-channel staging pass, where that is larger)
  static_assert(lds <= split_lds_bytes<BN, BM, 3>(), "never more than the exact split asks for");
  char nm[160];
  snprintf(nm, sizeof(nm), "fused_split_kernel<%d,%d,bf16x1,1 terms,npw=%d,xm=%d>", BN, BM, NPW, XM);
  return launch_kernel(fused_split_kernel<BN, BM, 1, NPW, XM>, nm, "fused forward (split, bf16)", dim3((unsigned)a.total_blocks), dim3(256 + 64 * NPW),
                       lds, lds, stream, a);
}

// (tile width, x fetch mode) -> instantiation: the table of launch_split_xm (bt_fused_split.hip) for the exact split
int launch_split_bf16_cfg(const FwdArgs& a, int bm, int xm, hipStream_t stream) {
  if (bm == 128) {
    if (a.bn32) {
      if (xm == 1) return launch_bf16_cfg<128, 8, 1, 32>(a, stream);
      if (xm == 2) return launch_bf16_cfg<128, 8, 2, 32>(a, stream);
      return launch_bf16_cfg<128, 8, 0, 32>(a, stream);
    }
    if (xm == 1) return launch_bf16_cfg<128, 8, 1>(a, stream);
    if (xm == 2) return launch_bf16_cfg<128, 8, 2>(a, stream);
    return launch_bf16_cfg<128, 8, 0>(a, stream);
  }
  if (bm == 256) {
    if (xm == 3) return launch_bf16_cfg<256, 8, 3>(a, stream);
    if (xm == 4) return launch_bf16_cfg<256, 8, 4>(a, stream);
    if (xm == 2) return launch_bf16_cfg<256, 8, 2>(a, stream);
    return launch_bf16_cfg<256, 8, 0>(a, stream);
  }
  if (xm == 3) return launch_bf16_cfg<512, 4, 3>(a, stream);
  if (xm == 4) return launch_bf16_cfg<512, 4, 4>(a, stream);
  return launch_bf16_cfg<512, 4, 0>(a, stream);
}

// the stems: one sample per workgroup (the sample walk is not instantiated: launch_quad plans the one-sample path in this mode)
int launch_quad_bf16(const FwdArgs& a, hipStream_t stream) {
  constexpr int lds = split_lds_bytes<64, 512, 3>();   // (the stem kernel keeps the exact split's buffer strides: bt_fused_split_quad.h)
  auto launch = [&](auto kern, const char* nm) {
    return launch_kernel(kern, nm, "fused forward (split, quad, bf16)", dim3((unsigned)a.total_blocks), dim3(512), lds, lds, stream, a);
  };
  if (a.ep_pool) return launch(fused_split_quad_kernel<1, true>, "fused_split_quad_kernel<64,512,bf16x1,1 terms,pool=1>");
  return launch(fused_split_quad_kernel<1, false>, "fused_split_quad_kernel<64,512,bf16x1,1 terms,pool=0>");
}

int launch_direct_bf16(const FwdArgs& a, bool resident, hipStream_t stream) {
  auto launch = [&](auto kern, const char* nm, int max_lds) {
    return launch_kernel(kern, nm, "fused forward (split, direct, bf16)", dim3((unsigned)a.total_blocks), dim3(kDirectThreads), direct_lds_bytes(a.Cig, 1),
                         max_lds, stream, a);
  };
  if (resident) return launch(fused_split_direct_kernel<true, false, 1>, "fused_split_direct_kernel<64,8x64,bf16x1,1 terms,resident W>", direct_lds_bytes(kDirectMaxK, 1));
  return launch(fused_split_direct_kernel<false, false, 1>, "fused_split_direct_kernel<64,8x64,bf16x1,1 terms,streamed W>", direct_lds_bytes(kDirectMaxK + 1, 1));
}

}  // namespace bt
