// Chains of same-shape layers as one launch of the general split kernel's CHAIN form (bt_fused_split.h): planner call, argument
// table, launch. Reparameterization, on-chip draws, the exact split, the whole-image 64 x 512 tile; x fetch modes 3 and 0.
#include <string.h>

#include "bt_fused_split_host.h"
#include "bt_fused_split_launch.h"

namespace bt {

static_assert(BT_CHAIN_MAX == kChainMax, "the header's limit is the kernel's table");

template <int XM>
static int launch_chain_inst(const FwdArgs& a, const ChainTab& tab, hipStream_t stream) {
  constexpr int BN = 64, BM = 512, NP = 3, NPW = split_npw(BM, false), lds = split_lds_bytes<BN, BM, NP>();
  static_assert(lds <= 160 * 1024, "LDS budget of one CU");
  SplitNames nm;
  snprintf(nm.name, sizeof(nm.name), "fused_split_chain_kernel<%d,%d,bf16x%d,%s terms,npw=%d,xm=%d,n=%d>", BN, BM, NP, split_terms(NP, false), NPW, XM, tab.n);
  snprintf(nm.who, sizeof(nm.who), "fused forward (split, chain)");
  return launch_kernel(fused_split_chain_kernel<BN, BM, NP, NPW, XM>, nm.name, nm.who, dim3((unsigned)a.total_blocks), dim3(256 + 64 * NPW), lds, lds, stream, a, tab);
}

// m[0..n): the members' argument blocks as bt::run fills them, in execution order. BT_OK: launched, `ran` is the plan (member 0's:
// every member has the same). 1: not a chain, nothing launched. < 0: error.
int launch_split_chain(int n, FwdArgs* m, FwdArgs& ran, hipStream_t stream) {
  int xm;
  if (split_chain_plan(n, m, contraction_mode(), &xm)) return 1;
  ChainTab tab;
  memset(&tab, 0, sizeof(tab));
  tab.n = n;
  for (int k = 0; k < n; ++k) tab.m[k] = split_layer_of(m[k]);
  ran = m[0];
  return xm == 3 ? launch_chain_inst<3>(m[0], tab, stream) : launch_chain_inst<0>(m[0], tab, stream);
}

}  // namespace bt
