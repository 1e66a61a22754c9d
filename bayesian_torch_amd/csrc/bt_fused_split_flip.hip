// Host side of the split-precision Flipout forward (bt_fused_split.h, FLIP = true): eligibility, tile geometry, launch.
#include "bt_fused_split_quad.h"
#include "bt_fused_split_host.h"

namespace bt {

// The instantiations that READ the draws and both sign streams (bt_fused_split_flip_inj.hip). A launch that reaches this chain with
// a.eps_w set carries BT_DRAWS_EPS_PACKED | BT_DRAWS_SIGNS_PACKED (bt_fused_api.hip): flavour and geometry are chosen below exactly as
// for on-chip draws, and the launch goes to the twin of the kernel they would have taken.
int launch_split_flip_inj_cfg(const FwdArgs& a, int bm, int xm, hipStream_t stream);
int launch_quad_flip_inj(const FwdArgs& a, hipStream_t stream);

template <int BM, int NPW, int XM>
static int launch_split_flip_cfg(const FwdArgs& a, hipStream_t stream) {
  constexpr int BN = 64, NP = 3;
  if (a.eps_w) return launch_split_flip_inj_cfg(a, BM, XM, stream);
  constexpr int lds = split_lds_bytes<BN, BM, NP, true>();
  static_assert(lds <= 160 * 1024, "LDS budget of one CU");
  char nm[160];
  snprintf(nm, sizeof(nm), "fused_split_kernel<%d,%d,bf16x%d,2x6 terms,flip,npw=%d,xm=%d>", BN, BM, NP, NPW, XM);
  return launch_kernel(fused_split_kernel<BN, BM, NP, NPW, XM, true>, nm, "fused forward (split, flipout)", dim3((unsigned)a.total_blocks),
                       dim3(256 + 64 * NPW), lds, lds, stream, a);
}

// Flipout stems (<= 3 input channels per group): bt_fused_split_quad.h with FLIP = true, 64 x 256 tiles of whole images or of
// bands of whole rows; the patch has to fit the 1600 pixels the two weight images leave.
template <bool POOL>
static int launch_quad_flip_cfg(const FwdArgs& a, hipStream_t stream) {
  constexpr int lds = quad_lds_bytes<true>();
  static_assert(lds <= 160 * 1024, "LDS budget of one CU");
  if (a.eps_w) return launch_quad_flip_inj(a, stream);
  return launch_kernel(fused_split_quad_kernel<3, POOL, true>,
                       POOL ? "fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=1>" : "fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=0>",
                       "fused forward (split, flipout, quad)", dim3((unsigned)a.total_blocks), dim3(512), lds, lds, stream, a);
}

// The flavour functions below work on their own copy of the arguments and, when they launch, hand the plan that ran to `ran`.
// Each returns BT_OK when the launch was taken, 1 when the flavour does not apply, < 0 on error.
static int launch_quad_flip(FwdArgs a, FwdArgs& ran, hipStream_t stream) {
  if (a.Cig > 3 || !quad_geometry(a, 256, kQuadXBytesFlip / 24)) return 1;
  if (!set_grid(a, (long long)a.G * a.n_tiles * a.S * a.m_tiles)) return 1;
  split_fill_inverses(a);
  ran = a;
  return a.ep_pool ? launch_quad_flip_cfg<true>(a, stream) : launch_quad_flip_cfg<false>(a, stream);
}

// Tiles: 64 channels x 256 output positions of whole images / row bands (the two accumulator sets of Flipout fill the
// consumers' registers at 32 x 128 per wave), or x 128 (the small feature maps: pixel-major tiles prune the padding taps per
// pixel, 1x1 maps); the patch of one octet plane has to fit 301 pixels (two planes when a single tap is active).
static int launch_split_flip_one(FwdArgs a, FwdArgs& ran, hipStream_t stream) {
  {   // f32: the fp32 kernels; bf16x2: Reparameterization only. (The bf16 mode leaves Flipout as it is in the automatic mode.)
    const int mode = contraction_mode();
    if (mode == 1 || mode == 2) return 1;
  }
  if (!packed_ok(a)) return 1;
  if (a.Cig <= 4) return launch_quad_flip(a, ran, stream);   // the stems
  if ((a.Cig & 7) || a.T > 9 || a.ep_pool) return 1;
  const int Mdom = a.pixel_major ? a.B : a.M;
  if (Mdom < 112) return 1;
  a.n_tiles = (a.Cog + 63) / 64;
  FwdArgs b256 = a, b128 = a;
  const int live256 = (Mdom >= 256 && !a.pixel_major) ? split_geometry<256, true>(b256) : 0;
  const int live128 = split_geometry<128, true>(b128);
  const double c256 = split_tile_cost(b256, live256, 256, 128, 48), c128 = split_tile_cost(b128, live128, 128, 128, 48);
  int bm = 0;
  if (c256 < 1e30 && c256 <= c128) bm = 256;
  else if (c128 < 1e30) bm = 128;
  if (!bm) return 1;
  a = bm == 256 ? b256 : b128;
  if (!set_grid(a, (long long)a.G * a.n_tiles * a.S * a.m_tiles)) return 1;
  const bool xal = (((uintptr_t)a.x) & 15u) == 0 && (a.x_sample_stride & 3) == 0;
  split_fill_inverses(a);
  ran = a;
  if (bm == 256) {
    const bool rows = xal && a.HW > 1 && a.SH == 1 && a.SW == 1 && (a.W & 3) == 0 && a.t_Wt == a.Wo && split_rows_cover(a);
    return rows ? launch_split_flip_cfg<256, 4, 3>(a, stream) : launch_split_flip_cfg<256, 4, 0>(a, stream);
  }
  if (xal && a.HW == 1) return launch_split_flip_cfg<128, 8, 1>(a, stream);
  if (xal && a.pixel_major && a.H == 2 && a.W == 2 && a.KH == 3 && a.KW == 3 && a.PH == 1 && a.PW == 1 && a.SH == 1 && a.SW == 1 && a.DH == 1 && a.DW == 1)
    return launch_split_flip_cfg<128, 8, 2>(a, stream);
  return launch_split_flip_cfg<128, 8, 0>(a, stream);
}

// Pixel-major tiles first; when none fits, tiles of whole images (as launch_split, bt_fused_split.hip).
int launch_split_flip(FwdArgs a, FwdArgs& ran, hipStream_t stream) {
  const int rc = launch_split_flip_one(a, ran, stream);
  if (rc != 1 || !a.pixel_major) return rc;
  a.pixel_major = 0;
  a.out_vec4 = 0;
  return launch_split_flip_one(a, ran, stream);
}

}  // namespace bt
