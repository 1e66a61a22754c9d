// The one place that knows which split-precision kernels exist: the launch templates of the general, stem (quad), direct and skinny
// kernels and the builders of their names, parameterised by the variant <NP, FLIP, INJ> -- pieces per value (3: the exact split,
// 2: the opt-in bf16x2 form, 1: the bf16 mode), Flipout, supplied (packed) draws. Each of the five translation units
// (bt_fused_split{,_inj,_bf16,_flip,_flip_inj}.hip: one per variant, so the build stays parallel) defines its launchers as
// one-line calls of these, and so instantiates exactly its variant's kernels.
#pragma once
#include <stdio.h>

#include "bt_fused_split_quad.h"
#include "bt_fused_split_direct.h"
#include "bt_fused_split_skinny.h"

namespace bt {

// The variants' launchers that another translation unit calls: the flavour functions of bt_fused_split.hip / bt_fused_split_flip.hip
// choose flavour and geometry exactly as for on-chip draws in the automatic mode -- a launch's plan depends on neither -- and hand
// the launch to the twin of the kernel they would have taken.
int launch_split_inj_cfg(const FwdArgs& a, int bm, int xm, hipStream_t stream);   // bt_fused_split_inj.hip: BT_DRAWS_EPS_PACKED
int launch_quad_inj(const FwdArgs& a, hipStream_t stream);
int launch_direct_inj(const FwdArgs& a, bool resident, hipStream_t stream);
int launch_skinny_inj(const FwdArgs& a, int ks, hipStream_t stream);
int launch_split_bf16_cfg(const FwdArgs& a, int bm, int xm, hipStream_t stream);   // bt_fused_split_bf16.hip: the bf16 mode
int launch_quad_bf16(const FwdArgs& a, hipStream_t stream);
int launch_direct_bf16(const FwdArgs& a, bool resident, hipStream_t stream);
int launch_split_flip_inj_cfg(const FwdArgs& a, int bm, int xm, hipStream_t stream);   // bt_fused_split_flip_inj.hip: + BT_DRAWS_SIGNS_PACKED
int launch_quad_flip_inj(const FwdArgs& a, hipStream_t stream);
// bt_fused_split_updil.hip: the input-dilated fetch (xm 5, FwdArgs::updil) of the general kernel, on-chip draws -- np 3 / 1
// Reparameterization (every tile), Flipout (np 3). BT_ERR_UNSUPPORTED, nothing launched, for anything else.
int launch_split_updil_cfg(const FwdArgs& a, int bm, int np, bool flip, hipStream_t stream);
// bt_fused_split_dwin.hip: the depth-window fetch (xm 6, FwdArgs::dwin) of the general kernel, on-chip draws -- the set xm 5 has.
int launch_split_dwin_cfg(const FwdArgs& a, int bm, int np, bool flip, hipStream_t stream);

// ---------------------------------------------------------------------------- names
// bt_last_kernel_name's strings (tests, bench.py's tables and the tools parse them) and the `who` of the error messages.
struct SplitNames {
  char name[160], who[64];
};
constexpr const char* split_terms(int np, bool flip) { return flip ? "2x6" : np == 3 ? "6" : np == 2 ? "3" : "1"; }
// family: "", ", quad", ", direct", ", skinny"
inline void split_who(SplitNames& n, const char* family, int np, bool flip, bool inj) {
  snprintf(n.who, sizeof(n.who), "fused forward (split%s%s%s)", flip ? ", flipout" : "", family, inj ? ", injected" : np == 1 ? ", bf16" : "");
}
inline SplitNames split_kernel_names(int bn, int bm, int np, int npw, int xm, bool flip, bool inj) {
  SplitNames n;
  snprintf(n.name, sizeof(n.name), "fused_split_kernel<%d,%d,bf16x%d,%s terms%s,npw=%d,xm=%d%s>", bn, bm, np, split_terms(np, flip), flip ? ",flip" : "", npw,
           xm, inj ? ",inj" : "");
  split_who(n, "", np, flip, inj);
  return n;
}
inline SplitNames quad_kernel_names(int np, bool flip, bool inj, bool pool, bool walk) {
  SplitNames n;
  snprintf(n.name, sizeof(n.name), "fused_split_quad_kernel<64,%d,bf16x%d,%s terms%s,pool=%d%s%s>", flip ? 256 : 512, np, split_terms(np, flip),
           flip ? ",flip" : "", pool ? 1 : 0, walk ? ",walk" : "", inj ? ",inj" : "");
  split_who(n, ", quad", np, flip, inj);
  return n;
}
inline SplitNames direct_kernel_names(int np, bool inj, bool resident) {
  SplitNames n;
  snprintf(n.name, sizeof(n.name), "fused_split_direct_kernel<64,8x64,bf16x%d,%s terms,%s W%s>", np, split_terms(np, false), resident ? "resident" : "streamed",
           inj ? ",inj" : "");
  split_who(n, ", direct", np, false, inj);
  return n;
}
inline SplitNames skinny_kernel_names(bool inj, int ks) {
  SplitNames n;
  snprintf(n.name, sizeof(n.name), "fused_split_skinny_kernel<64,4x32,bf16x3,6 terms,split-K %d%s>", ks == 128 ? 128 : 64, inj ? ",inj" : "");
  split_who(n, ", skinny", 3, false, inj);
  return n;
}

// ---------------------------------------------------------------------------- the general kernel
// fused_split_kernel<BN, BM, NP, NPW, XM, FLIP, INJ>: producer waves of a tile, and the (channel tile, width, x fetch mode) that are
// instantiated per variant:
//                            BM 128                        BM 256                  BM 512
//   NP 3 / 1, Reparam.       xm {0,1,2} x BN {64,32}       xm {0,2,3,4}            xm {0,3,4}
//   NP 2 (bf16x2, opt-in)    xm 0 (the generic fetch)      xm 0                    xm 0
//   Flipout                  xm {0,1}                      xm {0,3}                --
// xm 5 (input-dilated images) exists for every tile of the np 3 / 1 Reparameterization and of the Flipout variant with on-chip draws. No
// other fetch can stand in for it -- the generic one would read the real image as if it were the virtual one -- so launch_split_xm never
// reaches it: launch_split_updil_cfg names its instantiations one by one.
// xm 6 (depth windows: Conv3d without the unfolded copy) exists for the same set and is reached the same way, through
// launch_split_dwin_cfg alone: a missing instantiation is an error, never the generic fetch.
// (Flipout's 128-wide xm 2 -- whole 2x2 planes of a pixel-major 3x3 -- is not instantiated: DESIGN 4.0c.)
constexpr int split_npw(int bm, bool flip) { return flip ? (bm == 128 ? 8 : 4) : (bm == 512 ? 4 : 8); }
constexpr bool split_exists(int bn, int bm, int np, bool flip, int xm) {
  if (flip ? (bn != 64 || bm == 512) : (bn == 32 && (bm != 128 || np == 2))) return false;
  if (xm == 0) return true;
  if (np == 2) return false;
  if (xm == 5 || xm == 6) return true;
  if (flip) return bm == 128 ? xm == 1 : xm == 3;
  return bm == 128 ? xm <= 2 : bm == 256 ? xm >= 2 : xm >= 3;
}

template <int NP, bool FLIP, bool INJ, int BN, int BM, int XM>
int launch_split_inst(const FwdArgs& a, hipStream_t stream) {
  if constexpr (XM == 5 && (INJ || !split_exists(BN, BM, NP, FLIP, XM))) {
    return set_error(BT_ERR_UNSUPPORTED, "fused forward (split): no input-dilated instantiation of this tile and variant");
  } else if constexpr (XM == 6 && (INJ || !split_exists(BN, BM, NP, FLIP, XM))) {
    return set_error(BT_ERR_UNSUPPORTED, "fused forward (split): no depth-window instantiation of this tile and variant");
  } else if constexpr (!split_exists(BN, BM, NP, FLIP, XM)) {
    static_assert(XM != 0, "the generic fetch exists for every tile a variant has");
    return launch_split_inst<NP, FLIP, INJ, BN, BM, 0>(a, stream);   // a fetch mode without an instantiation: the generic fetch
  } else {
    constexpr int NPW = split_npw(BM, FLIP), lds = split_lds_bytes<BN, BM, NP, FLIP>();
    static_assert(lds <= 160 * 1024, "LDS budget of one CU");
    static_assert(lds <= split_lds_bytes<BN, BM, 3, FLIP>(), "never more than the exact split asks for");
    const SplitNames n = split_kernel_names(BN, BM, NP, NPW, XM, FLIP, INJ);
    return launch_kernel(fused_split_kernel<BN, BM, NP, NPW, XM, FLIP, INJ>, n.name, n.who, dim3((unsigned)a.total_blocks), dim3(256 + 64 * NPW), lds, lds,
                         stream, a);
  }
}
template <int NP, bool FLIP, bool INJ, int BN, int BM>
int launch_split_xm(const FwdArgs& a, int xm, hipStream_t stream) {
  switch (xm) {
    case 1: return launch_split_inst<NP, FLIP, INJ, BN, BM, 1>(a, stream);
    case 2: return launch_split_inst<NP, FLIP, INJ, BN, BM, 2>(a, stream);
    case 3: return launch_split_inst<NP, FLIP, INJ, BN, BM, 3>(a, stream);
    case 4: return launch_split_inst<NP, FLIP, INJ, BN, BM, 4>(a, stream);
    default: return launch_split_inst<NP, FLIP, INJ, BN, BM, 0>(a, stream);
  }
}
// bm: 128, 256 or (Reparameterization) 512, as split_plan chose it; a.bn32: 32-channel tiles of a 128-wide launch (same K order, same bits)
template <int NP, bool FLIP, bool INJ>
int launch_split_general(const FwdArgs& a, int bm, int xm, hipStream_t stream) {
  if (bm == 256) return launch_split_xm<NP, FLIP, INJ, 64, 256>(a, xm, stream);
  if constexpr (!FLIP) {
    if (bm == 512) return launch_split_xm<NP, FLIP, INJ, 64, 512>(a, xm, stream);
  }
  if constexpr (split_exists(32, 128, NP, FLIP, 0)) {
    if (a.bn32) return launch_split_xm<NP, FLIP, INJ, 32, 128>(a, xm, stream);
  }
  return launch_split_xm<NP, FLIP, INJ, 64, 128>(a, xm, stream);
}

// ---------------------------------------------------------------------------- the stems
// Layers with <= 4 input channels per group (the ResNet stems): bt_fused_split_quad.h. Reparameterization: whole-image 512-wide
// tiles, the exact split's LDS (the bf16 mode keeps its buffer strides). Flipout: 64 x 256 tiles of whole images or of bands of whole
// rows; the patch has to fit the 1600 pixels the two weight images leave. Output through the LDS-staged read-out, optionally with
// the fused 3x3 / stride-2 max-pool (a.ep_pool). WALK: the sample walk (launch_quad), an on-chip exact-split Reparameterization special.
// (The opt-in two-piece form is not instantiated for the stems: they run the exact split in every split mode.)
template <int NP, bool FLIP, bool INJ, bool WALK = false>
int launch_split_quad(const FwdArgs& a, hipStream_t stream) {
  static_assert(!WALK || (NP == 3 && !FLIP && !INJ), "the walk is instantiated for the on-chip exact split alone");
  constexpr int lds = FLIP ? quad_lds_bytes<true>() : split_lds_bytes<64, 512, 3>();
  static_assert(lds <= 160 * 1024, "LDS budget of one CU");
  auto launch = [&](auto kern, bool pool) {
    const SplitNames n = quad_kernel_names(NP, FLIP, INJ, pool, WALK);
    return launch_kernel(kern, n.name, n.who, dim3((unsigned)a.total_blocks), dim3(512), lds, lds, stream, a);
  };
  if constexpr (WALK) return launch(fused_split_quad_kernel<NP, true, FLIP, true, INJ>, true);
  else return a.ep_pool ? launch(fused_split_quad_kernel<NP, true, FLIP, false, INJ>, true) : launch(fused_split_quad_kernel<NP, false, FLIP, false, INJ>, false);
}

// ---------------------------------------------------------------------------- direct and skinny
// (the LDS limit is raised to the largest launch of each variant: K = 256 resident, any K streamed)
template <int NP, bool INJ>
int launch_split_direct(const FwdArgs& a, bool resident, hipStream_t stream) {
  const SplitNames n = direct_kernel_names(NP, INJ, resident);
  auto launch = [&](auto kern, int max_lds) {
    return launch_kernel(kern, n.name, n.who, dim3((unsigned)a.total_blocks), dim3(kDirectThreads), direct_lds_bytes(a.Cig, NP), max_lds, stream, a);
  };
  if (resident) return launch(fused_split_direct_kernel<true, INJ, NP>, direct_lds_bytes(kDirectMaxK, NP));
  return launch(fused_split_direct_kernel<false, INJ, NP>, direct_lds_bytes(kDirectMaxK + 1, NP));
}

template <bool INJ>
int launch_split_skinny(const FwdArgs& a, int ks, hipStream_t stream) {
  const SplitNames n = skinny_kernel_names(INJ, ks);
  return launch_kernel(fused_split_skinny_kernel<INJ>, n.name, n.who, dim3((unsigned)a.total_blocks), dim3(kSkinnyThreads), skinny_lds_bytes(ks),
                       skinny_lds_bytes(128), stream, a);
}

}  // namespace bt
