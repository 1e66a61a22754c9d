// Host side of the split-precision flavour (bt_fused_split.h): eligibility, tile geometry, launch.
#include <stdlib.h>
#include <string.h>

#include "bt_fused_split_host.h"
#include "bt_fused_split_launch.h"

namespace bt {

// 0: automatic (6-term exact split where the launch is eligible), 1: fp32 MFMA only, 2: 3-term split (opt-in, ~1e-5 relative),
// 3: bf16 (opt-in: operands rounded once to bf16, 1 term, where mode 0 runs the general split, stem or direct kernel; else as mode 0)
static EnvKnob g_contraction{"BT_CONTRACTION", [](const char* e) { return !e ? 0 : (!strcmp(e, "f32") ? 1 : !strcmp(e, "bf16x2") ? 2 : !strcmp(e, "bf16") ? 3 : 0); }};
int contraction_mode() { return g_contraction.get(); }
EnvKnob g_bn32{"BT_BN32", [](const char* e) { return e ? (atoi(e) ? 1 : 0) : -1; }};   // -1 automatic; 0 / 1 forced (split_plan)
static EnvKnob g_direct_off{nullptr, [](const char*) { return 0; }};   // (bt_debug_disable_direct alone)
static EnvKnob g_skinny_off{"BT_NO_SKINNY", [](const char* e) { return (e && *e && *e != '0') ? 1 : 0; }};   // measurement knob (tools/trace_layers.py), like its test hook

// Samples per workgroup of the quad flavour's sample walk (0: the one-sample path). Pooled 16x16 maps in tiles of two images over
// an input that every sample shares: the patch is staged once for a run of samples. The largest of 8 / 4 / 2 that still gives a
// workgroup to every CU (at least kKlSlices workgroups: the fused KL sweep keeps its slices, so its sum is the one-sample path's).
// BT_QUAD_SPW (measurement knob, read at every launch) caps it: 1 = the one-sample path.
static int quad_spw(const FwdArgs& a, long long tiles, int mode) {
  if (a.eps_w) return 0;   // injected draws: the one-sample path (bit-identical to the walk)
  if (mode == 3) return 0;   // the bf16 mode: the walk is not instantiated (the one-sample path computes the same function)
  if (!a.ep_pool || a.x_sample_stride != 0 || a.S < 2 || a.Ho != 16 || a.Wo != 16 || a.t_NI != 2 || a.ep_Hp != 8 || a.ep_Wp != 8) return 0;
  int nd[2] = {};
  tap_window(a.KH, a.DH, a.SH, a.PH, a.H, a.Ho, false, &nd[0], &nd[1]);
  int nw, dxs;
  tap_window(a.KW, a.DW, a.SW, a.PW, a.W, a.Wo, false, &nw, &dxs);
  const long long PHt = 15ll * (nd[1] ? a.SH : 1) + nd[1] + 1, PWt = 15ll * (dxs ? a.SW : 1) + dxs + 1;
  if (2 * PHt * PWt * 24 + kWalkBytes > kQuadXBytes) return 0;   // the walk's slots sit behind the patch
  static int n_cu[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (!n_cu[dev] && hipDeviceGetAttribute(&n_cu[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n_cu[dev] = 0;
  const long long fill = n_cu[dev] > 256 ? n_cu[dev] : 256;
  const char* e = getenv("BT_QUAD_SPW");
  const int cap = e ? atoi(e) : 8;
  for (int spw = 8; spw >= 2; spw >>= 1)
    if (spw <= cap && spw <= a.S && tiles * ((a.S + spw - 1) / spw) >= fill) return spw;
  return 0;
}

// The flavour functions below work on their own copy of the arguments and, when they launch, hand the plan that ran to `ran`.
// Each returns BT_OK when the launch was taken, 1 when the flavour does not apply, < 0 on error.
static int launch_quad(FwdArgs a, FwdArgs& ran, int mode, hipStream_t stream) {
  if (!quad_geometry(a, 512, kQuadXBytes / 24)) return 1;
  const long long tiles = (long long)a.G * a.n_tiles * a.m_tiles;
  const int spw = quad_spw(a, tiles, mode);
  a.spw = spw ? spw : 1, a.n_sg = (a.S + a.spw - 1) / a.spw;
  if (!set_grid(a, tiles * a.n_sg)) return 1;
  split_fill_inverses(a);
  ran = a;
  if (a.eps_w) return launch_quad_inj(a, stream);
  if (mode == 3) return launch_quad_bf16(a, stream);
  return spw ? launch_split_quad<3, false, false, true>(a, stream) : launch_split_quad<3, false, false>(a, stream);
}

// 1x1 / stride-1 convolutions with K <= 256 and many pixels (the bottleneck ResNets' expanding / reducing layers): the persistent
// kernel of bt_fused_split_direct.h. Eligibility is geometric (never a matter of S or of the launch split), and its arithmetic is the
// general kernel's, so a layer's results do not depend on which of the two serves it.
static int launch_direct(FwdArgs a, FwdArgs& ran, int mode, hipStream_t stream) {
  if (g_direct_off.get()) return 1;
  if (a.ep_pool) return 1;
  // a 1x1 kernel without padding (any stride), or any window over a 1x1 image whose ONE live tap sits on the pixel (ResNet18 / CIFAR
  // layer4: 3x3, padding 1, 1x1 maps -- the centre tap; Linear layers are 1x1 kernels over 1x1 images)
  if (a.KH == 1 && a.KW == 1 && a.PH == 0 && a.PW == 0) {
    a.d_tap = 0;
  } else if (a.H == 1 && a.W == 1 && a.Ho == 1 && a.Wo == 1 && a.PH % a.DH == 0 && a.PW % a.DW == 0 && a.PH / a.DH < a.KH && a.PW / a.DW < a.KW) {
    a.d_tap = (a.PH / a.DH) * a.KW + a.PW / a.DW;
  } else {
    return 1;
  }
  const bool resident = a.Cig <= kDirectMaxK;
  // K > 256 streams the weights in chunks that all 8 waves draw and meet at: it needs every wave to own pixels (>= 4096 per sample).
  // CIFAR-sized layers with K = 512 (128 pixels per sample: 2 of 8 waves would multiply, on 2 of the 4 matrix pipes) measured
  // 87 us against the general kernel's 57 (profiles/r03f_layers_cfg3.json): they stay there. K <= 256 wins at any size.
  if ((a.Cig & 63) || (!resident && ((a.Cig % (16 * kDirectChunk)) || a.M < 4096)) || a.M < 64) return 1;
  a.n_tiles = (a.Cog + 63) / 64;
  const long long pairs = (long long)a.G * a.n_tiles * a.S;
  const int nsub = (a.M + 63) / 64;
  // chunks of the pixel range per (group, channel tile, sample): ~1024 workgroups in all (four per CU: the tail of an uneven split
  // is a quarter of a workgroup's work), each with at least 64 sub-tiles (8 per wave) to walk
  // Measured at ResNet50 / b256 / S = 16 (tools/ab_direct_wgs.sh, env BT_DIRECT_WGS): the STREAMED flavour re-draws its weight chunks per
  // 512 pixels whatever the split, so extra workgroups only add prologues and KL slices -- one per CU is best (K = 2048 -> 512 on 7x7:
  // 3260 -> 2805 us; K = 1024 -> 256 on 14x14: 3065 -> 2947); a STRIDED resident layer (the downsamples: half of every fetched line
  // is unused) likes short workgroups that spread its fetches (256 -> 512 stride 2 on 56x56: 8001 -> 7253 us at 4096); everything else
  // stays at four per CU.
  static const int wg_env = [] { const char* e = getenv("BT_DIRECT_WGS"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 0; }();   // measurement knob
  static const int n_cu = [] { int dev = 0, v = 0; if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256; return v; }();
  const int wg_target = wg_env ? wg_env : !resident ? n_cu : (a.SH > 1 || a.SW > 1) ? 16 * n_cu : 4 * n_cu;
  long long chunks = (wg_target + pairs - 1) / pairs;
  if (chunks > nsub / 64) chunks = nsub / 64;
  if (chunks < 1) {   // few pixels (CIFAR-sized maps): down to FOUR sub-tiles per workgroup (half its waves), as long as that still adds workgroups the
                      // chip has room for (ResNet18 layer3's downsample: 128 -> 256 workgroups, 45.8 -> 39 us; two sub-tiles per workgroup: 47 us)
    chunks = (256 + pairs - 1) / pairs;
    if (chunks > nsub / 4) chunks = nsub / 4;
    if (chunks < 1) chunks = 1;
  }
  int spc = (int)((nsub + chunks - 1) / chunks);
  if (!resident) spc = (spc + 7) & ~7;   // the 8 waves walk 512-pixel tiles together
  chunks = (nsub + spc - 1) / spc;
  const long long total = pairs * chunks;
  if (!set_grid(a, total)) return 1;
  a.m_tiles = (int)chunks, a.t_NI = spc, a.t_R = 1, a.t_Wt = 64, a.n_bt = (int)chunks, a.n_rt = a.n_ct = 1;
  a.inv_n_tiles = inv_u32(a.n_tiles, total), a.inv_m_tiles = inv_u32(a.m_tiles, total), a.inv_S = inv_u32(a.S, total);
  a.inv_rw = inv_u32(a.HoWo, (long long)a.M + 64 * 8 * 2);   // pixel index -> (image, output position)
  a.inv_wt = inv_u32(a.Wo, a.HoWo);                          // output position -> (row, column): strided layers
  ran = a;
  if (a.eps_w) return launch_direct_inj(a, resident, stream);
  return mode == 3 ? launch_direct_bf16(a, resident, stream) : launch_split_direct<3, false>(a, resident, stream);
}

// Layers whose output map is one pixel and whose batch is small (Linear, CIFAR-sized layer4, the classifier head): the split-K kernel of
// bt_fused_split_skinny.h. Geometry of the slices from the layer alone, so the K order never depends on S or on the launch split.
struct SkinnyPlan { int ks, cpt, kh0, nh, kw0, nw, nsl, n_tiles, m_tiles; long long tiles, scratch; };
static bool skinny_plan(int B, int Ci, int H, int W, int Co, int KH, int KW, int PH, int PW, int DH, int DW, int G, int Ho, int Wo, int S, SkinnyPlan* p) {
  if (Ho != 1 || Wo != 1 || B > 1024 || KH * KW > 64) return false;
  const int Cig = Ci / G, Cog = Co / G;
  if (Cig & 63) return false;
  const int kh0 = (PH + DH - 1) / DH, kw0 = (PW + DW - 1) / DW;              // first tap with kh * DH - PH >= 0
  int kh1 = (PH + H - 1) / DH, kw1 = (PW + W - 1) / DW;                      // last tap with kh * DH - PH <= H - 1
  if (kh1 > KH - 1) kh1 = KH - 1;
  if (kw1 > KW - 1) kw1 = KW - 1;
  if (kh1 < kh0 || kw1 < kw0) return false;
  p->kh0 = kh0, p->nh = kh1 - kh0 + 1, p->kw0 = kw0, p->nw = kw1 - kw0 + 1;
  p->ks = (Cig & 127) ? 64 : 128;
  p->cpt = Cig / p->ks;
  p->nsl = p->nh * p->nw * p->cpt;
  p->n_tiles = (Cog + 63) / 64, p->m_tiles = (B + kSkinnyCols - 1) / kSkinnyCols;
  // Measured on ResNet18 / CIFAR (S = 32, b128, rocprofv3 inside the bench graph, tools/trace_layers.py): the classifier head (4
  // workgroups per sample) 37.6 -> 23.8 us; the 1x1 stride-2 downsample into layer4 (16 per sample) 40.7 -> 43.9 against the direct
  // kernel; layer4's 3x3 layers with one live tap (32 per sample) 53 ... 60 -> 60; layer4.0.conv1 with four live taps (64 per sample,
  // 2048 workgroups) 71 -> 140: past a few slices per sample the slabs' HBM round trip (2 x 32 KB per workgroup) and the second round
  // of workgroups cost more than the shorter chains save. So: narrow heads only. The bound is per SAMPLE -- geometry, not S.
  static const int gate = [] { const char* e = getenv("BT_SKINNY_MAX"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 8; }();   // measurement knob
  if ((long long)G * p->m_tiles * p->n_tiles * p->nsl > gate) return false;
  p->tiles = (long long)G * S * p->m_tiles * p->n_tiles;
  if (p->tiles > kSkinnyMaxTiles || p->tiles * p->nsl > 0x7FFFFFFFll) return false;
  p->scratch = p->tiles * p->nsl * (64ll * kSkinnyCols * 4);
  return true;
}
long long skinny_scratch_bytes(const bt_conv2d_geom& g, int S) {
  if (geom_error(g)) return 0;
  const int Ho = (int)conv_out_h(g), Wo = (int)conv_out_w(g);
  SkinnyPlan p;
  return skinny_plan(g.B, g.Ci, g.H, g.W, g.Co, g.kh, g.kw, g.ph, g.pw, g.dh, g.dw, g.groups, Ho, Wo, S, &p) ? p.scratch : 0;
}
static int launch_skinny(FwdArgs a, FwdArgs& ran, hipStream_t stream) {
  if (g_skinny_off.get() || a.ep_pool || !a.sk_scratch || !a.sk_tickets) return 1;
  SkinnyPlan p;
  if (!skinny_plan(a.B, a.Ci, a.H, a.W, a.Co, a.KH, a.KW, a.PH, a.PW, a.DH, a.DW, a.G, a.Ho, a.Wo, a.S, &p)) return 1;
  if (p.scratch > a.sk_scratch_bytes) return 1;   // the caller brought no (or too little) scratch: the other flavours serve the launch
  if ((((uintptr_t)a.sk_scratch) & 15u)) return 1;
  a.sk_ks = p.ks, a.sk_cpt = p.cpt, a.sk_nsl = p.nsl, a.sk_kh0 = p.kh0, a.sk_nh = p.nh, a.sk_kw0 = p.kw0, a.sk_nw = p.nw;
  a.n_tiles = p.n_tiles, a.m_tiles = p.m_tiles;
  a.t_NI = kSkinnyCols, a.t_R = 1, a.t_Wt = 1, a.n_bt = p.m_tiles, a.n_rt = a.n_ct = 1;
  // every workgroup of the split-K grid (skinny_plan bounds it); the KL sweep keeps 256 slices (spread over every workgroup it
  // lengthened all of them: 50 -> 62 us on ResNet18 layer4)
  if (!set_grid(a, p.tiles * p.nsl)) return 1;
  a.x_vec = (a.HW == 1 && ((((uintptr_t)a.x) & 15u) == 0) && (a.x_sample_stride & 3) == 0 && (a.Ci & 3) == 0) ? 1 : 0;
  ran = a;
  return a.eps_w ? launch_skinny_inj(a, p.ks, stream) : launch_split_skinny<false>(a, p.ks, stream);
}

// The stems', split-K, direct and general split kernels for one tile kind (the caller runs the fp32 kernels when none applies).
static int launch_split_one(FwdArgs a, FwdArgs& ran, hipStream_t stream) {
  const int mode = contraction_mode();
  if (mode == 1) return 1;
  // Reparameterization, on-chip draws or PACKED injected ones, packed parameters, 32-bit byte offsets
  if (!packed_ok(a)) return 1;
  const bool inj = a.eps_w != nullptr;
  if (inj && mode >= 2) return 1;   // (the opt-in forms have no injected instantiation)
  // An input-dilated image (bt_reparam_conv2d_updil_fwd) is read by the general kernel's xm 5 fetch alone: on-chip draws, the exact split
  // or the bf16 mode; the stem, split-K and direct kernels never take it (the fp32 general kernel serves what is left).
  // A depth-window launch (bt_reparam_conv2d_dwin_fwd) in the same way: the xm 6 fetch alone.
  if ((a.updil || a.dwin) && (inj || mode == 2 || a.Cig <= 4)) return 1;
  if (a.Cig <= 4) return launch_quad(a, ran, mode, stream);   // the stems
  // whole channel octets, no fused pooling
  if ((a.Cig & 7) || a.ep_pool) return 1;
  if (mode != 2 && !a.updil && !a.dwin) {   // (the flavours with a single live tap per slice / layer take any window size)
    // (the bf16 mode has no split-K instantiation: the direct / general kernels serve those launches)
    const int rck = mode == 3 ? 1 : launch_skinny(a, ran, stream);
    if (rck <= 0) return rck;
    const int rcd = launch_direct(a, ran, mode, stream);
    if (rcd <= 0) return rcd;
  }
  int bm, xm;
  if (split_plan<false>(a, mode, &bm, &xm)) return 1;
  ran = a;
  if (a.updil) return launch_split_updil_cfg(a, bm, mode == 3 ? 1 : 3, false, stream);
  if (a.dwin) return launch_split_dwin_cfg(a, bm, mode == 3 ? 1 : 3, false, stream);
  if (inj) return launch_split_inj_cfg(a, bm, xm, stream);
  if (mode == 3) return launch_split_bf16_cfg(a, bm, xm, stream);
  return mode == 2 ? launch_split_general<2, false, false>(a, bm, xm, stream) : launch_split_general<3, false, false>(a, bm, xm, stream);   // (bf16x2: the generic fetch alone)
}

// Pixel-major tiles (2..4-pixel outputs) prune the padding taps per pixel: the first choice. When their patch does not fit (a
// stride-2 3x3 from 4x4 to 2x2 maps: up to 9 input pixels per output pixel and image), tiles of whole images -- every active
// tap once for all pixels -- usually do, and beat the fp32 kernels (165 -> 104 us on ResNet18's layer3.0.conv1).
int launch_split(FwdArgs a, FwdArgs& ran, hipStream_t stream) {
  // Two-row maps with a stride-1 window (ResNet18 / CIFAR layer3: 3x3 on 2x2): tiles of (images x ONE output row) before the
  // pixel-major ones. A row's pixels share 6 of the 9 taps: 3 MFMA steps and 6 weight draws per octet for 2 pixels instead of
  // 2 x (2 steps, 4 draws), and half the workgroups. The choice is geometric (never a matter of S or of the tile width), so
  // the tap pairing -- the K order -- of a layer stays the same for every launch split.
  if (a.pixel_major && a.Ho == 2 && a.Wo >= 2 && a.SH == 1 && a.KH == 3 && a.PH == 1 && a.DH == 1 && !a.ep_pool) {
    FwdArgs t = a;
    t.pixel_major = 0, t.out_vec4 = 0, t.row_taps = 1;
    const int rc = launch_split_one(t, ran, stream);
    if (rc <= 0) return rc;
  }
  const int rc = launch_split_one(a, ran, stream);
  if (rc != 1 || !a.pixel_major) return rc;
  a.pixel_major = 0;
  a.out_vec4 = 0;   // 2..4-pixel rows: the scalar output stage
  return launch_split_one(a, ran, stream);
}

}  // namespace bt

// Test hook (not part of include/bt_hip.h): 1 keeps 1x1 convolutions off the direct kernel, so a test can compare the two flavours.
extern "C" void bt_debug_disable_direct(int off) { bt::g_direct_off.set(off ? 1 : 0); }
extern "C" void bt_debug_force_bn32(int v) { bt::g_bn32.set(v < 0 ? -1 : (v ? 1 : 0)); }
extern "C" void bt_debug_disable_skinny(int off) { bt::g_skinny_off.set(off ? 1 : 0); }

// Contraction arithmetic of the fused forwards (process-wide knob, read at every launch; also env BT_CONTRACTION = f32 | bf16x3 |
// bf16x2 | bf16): 0 automatic -- exact bf16x3 split (6 product terms, fp32 accumulate) on the bf16 matrix pipe wherever the launch is
// eligible, 1 fp32 MFMA everywhere (the bit-exact fp32 FMA chain), 2 bf16x2 split (3 terms; relative error ~1e-5, opt-in), 3 bf16
// (opt-in, inference: operands rounded once to bf16, 1 term, on the Reparameterization launches that mode 0 gives to the general
// split, stem or direct kernel -- same plan; every other launch as in mode 0).
extern "C" int bt_set_contraction(int mode) {
  if (mode < 0 || mode > 3) return bt::set_error(BT_ERR_BAD_ARG, "bt_set_contraction: mode must be 0 (auto), 1 (f32), 2 (bf16x2) or 3 (bf16)");
  bt::g_contraction.set(mode);
  return BT_OK;
}
extern "C" int bt_get_contraction(void) { return bt::contraction_mode(); }
