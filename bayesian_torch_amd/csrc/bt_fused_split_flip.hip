// Host side of the split-precision Flipout forward (bt_fused_split.h, FLIP = true): eligibility, tile geometry, launch.
#include "bt_fused_split_host.h"
#include "bt_fused_split_launch.h"

namespace bt {

// The flavour functions below work on their own copy of the arguments and, when they launch, hand the plan that ran to `ran`.
// Each returns BT_OK when the launch was taken, 1 when the flavour does not apply, < 0 on error. A launch that reaches this chain
// with a.eps_w set carries BT_DRAWS_EPS_PACKED | BT_DRAWS_SIGNS_PACKED (bt_fused_api.hip).
static int launch_quad_flip(FwdArgs a, FwdArgs& ran, hipStream_t stream) {
  if (a.Cig > 3 || !quad_geometry(a, 256, kQuadXBytesFlip / 24)) return 1;
  if (!set_grid(a, (long long)a.G * a.n_tiles * a.S * a.m_tiles)) return 1;
  split_fill_inverses(a);
  ran = a;
  return a.eps_w ? launch_quad_flip_inj(a, stream) : launch_split_quad<3, true, false>(a, stream);
}

// Tiles: 64 channels x 256 output positions of whole images / row bands, or x 128 (the small feature maps: pixel-major tiles prune
// the padding taps per pixel, 1x1 maps); the patch of one octet plane has to fit 301 pixels (two planes when a single tap is active).
static int launch_split_flip_one(FwdArgs a, FwdArgs& ran, hipStream_t stream) {
  // f32: the fp32 kernels; bf16x2: Reparameterization only. (The bf16 mode leaves Flipout as it is in the automatic mode.)
  const int mode = contraction_mode();
  if (mode == 1 || mode == 2) return 1;
  if (!packed_ok(a)) return 1;
  if ((a.updil || a.dwin) && (a.eps_w || a.Cig <= 4)) return 1;   // an input-dilated image / a depth window: the general kernel's xm 5 / 6 fetch, on-chip draws (else the fp32 general kernel)
  if (a.Cig <= 4) return launch_quad_flip(a, ran, stream);   // the stems
  if ((a.Cig & 7) || a.ep_pool) return 1;   // whole channel octets, no fused pooling
  int bm, xm;
  if (split_plan<true>(a, mode, &bm, &xm)) return 1;
  ran = a;
  if (a.updil) return launch_split_updil_cfg(a, bm, 3, true, stream);
  if (a.dwin) return launch_split_dwin_cfg(a, bm, 3, true, stream);
  return a.eps_w ? launch_split_flip_inj_cfg(a, bm, xm, stream) : launch_split_general<3, true, false>(a, bm, xm, stream);
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
