// Host-side helpers shared by the split flavour's translation units: the process-wide knobs, the tile geometry and the planner of
// the general kernel's tile (bt_fused_split.hip, bt_fused_split_flip.hip). The launchers are in bt_fused_split_launch.h.
#pragma once
#include <stdlib.h>

#include "bt_fused_split.h"

namespace bt {

extern EnvKnob g_bn32;   // bt_fused_split.hip: -1 automatic; 0 / 1 forced (BT_BN32, bt_debug_force_bn32)

// ceil(2^32 / d): __umulhi(n, .) == n / d for every dividend n with n * d < 2^32. 0 when that cannot be promised (or d == 1):
// the kernel then divides.
static inline uint32_t inv_u32(long long d, long long nmax) {
  if (d <= 1 || nmax < 0 || (unsigned long long)nmax * (unsigned long long)d >= (1ull << 32)) return 0u;
  return (uint32_t)(((1ull << 32) + (unsigned long long)d - 1ull) / (unsigned long long)d);
}
// Reciprocals of the launch-uniform divisors of the tile decode (every workgroup used to spend ~2,000 cycles dividing).
static inline void split_fill_inverses(FwdArgs& a) {
  static const bool off = getenv("BT_NO_HOST_INV") != nullptr;   // test hook: every kernel-side division takes its fallback path
  if (off) {
    a.inv_m_tiles = a.inv_S = a.inv_n_tiles = a.inv_n_bt = a.inv_n_ct = a.inv_rw = a.inv_wt = a.inv_kw = a.inv_n_sg = a.inv_uh = a.inv_uw = a.inv_kd = a.inv_do = 0u;
    return;
  }
  const long long tb = a.total_blocks;
  a.inv_m_tiles = inv_u32(a.m_tiles, tb);
  a.inv_S = inv_u32(a.S, tb);
  a.inv_n_tiles = inv_u32(a.n_tiles, tb);
  a.inv_n_bt = inv_u32(a.n_bt, a.m_tiles);
  a.inv_n_ct = inv_u32(a.n_ct, a.m_tiles);
  a.inv_rw = inv_u32((long long)a.t_R * a.t_Wt, 1024);
  a.inv_wt = inv_u32(a.t_Wt, 1024);
  a.inv_kw = inv_u32(a.KW, 64);
  a.inv_n_sg = inv_u32(a.n_sg, tb);
  a.inv_uh = a.updil ? inv_u32(a.UH, a.H) : 0u, a.inv_uw = a.updil ? inv_u32(a.UW, a.W) : 0u;   // (virtual pixel -> real element, XM 5)
  a.inv_kd = a.dwin ? inv_u32(a.KD, a.Cig + 64) : 0u, a.inv_do = a.dwin ? inv_u32(a.Do, a.B + 1024) : 0u;   // (launch channel -> (ci, j), launch image -> (b, dz): XM 6)
}

// Extent of the window of taps that can meet data along one axis (the kernel's own rule: bt_fused_split.h), for the whole
// output axis or -- pixel-major tiles prune per pixel -- the widest window of any single output position.
static void tap_window(int K, int D, int S, int P, int In, int Out, bool per_pixel, int* n_act, int* extent, int* n_min = nullptr) {
  int best_n = 0, best_ext = 0, least_n = 1 << 30;
  if (per_pixel) {
    for (int o = 0; o < Out; ++o) {
      int lo = 1 << 30, hi = -1, n = 0;
      for (int k = 0; k < K; ++k)
        if ((unsigned)(o * S - P + k * D) < (unsigned)In) lo = k * D < lo ? k * D : lo, hi = k * D > hi ? k * D : hi, ++n;
      if (n > best_n) best_n = n;
      if (n < least_n) least_n = n;
      if (hi - lo > best_ext) best_ext = hi - lo;
    }
    if (n_min) *n_min = least_n;
  } else {
    int lo = 1 << 30, hi = -1;
    for (int k = 0; k < K; ++k) {
      const int l = P - k * D, c = l > 0 ? (l + S - 1) / S : 0;
      if (c < Out && c * S - l < In) lo = k * D < lo ? k * D : lo, hi = k * D > hi ? k * D : hi, ++best_n;
    }
    best_ext = hi >= lo ? hi - lo : 0;
  }
  *n_act = best_n, *extent = best_ext;
}

// One axis of a tile that spans the whole output axis: how many input positions does the patch keep (the kernel's own rule,
// bt_fused_split.h: the window of the active taps on a grid of spacing gs = 1, or the stride when a single tap is active)?
static int split_axis_kept(int K, int D, int S, int P, int In, int Out, int* gs_out) {
  int lo = 1 << 30, hi = -1;
  for (int k = 0; k < K; ++k) {
    const int l = P - k * D, c = l > 0 ? (l + S - 1) / S : 0;
    if (c < Out && c * S - l < In) lo = k * D < lo ? k * D : lo, hi = k * D > hi ? k * D : hi;
  }
  *gs_out = 1;
  if (hi < 0) return 0;
  const int ext = hi - lo, gs = ext ? 1 : S, ps = ext ? S : 1;
  const int x_lo = -P + lo, Pt = (Out - 1) * ps + ext + 1;
  const int kmin = x_lo < 0 ? (-x_lo + gs - 1) / gs : 0;
  int kmax = In - 1 - x_lo >= 0 ? (In - 1 - x_lo) / gs : -1;
  if (kmax > Pt - 1) kmax = Pt - 1;
  *gs_out = gs;
  return kmax >= kmin ? kmax - kmin + 1 : 0;
}
// Tiles of whole output rows (t_Wt == Wo): which columns of its input rows does the patch keep? 3: every column (the x fetch can
// move 16-byte row pieces, XM 3), 4: every second column (XM 4), 0: neither / W % 4 != 0.
static int split_row_mode(const FwdArgs& a) {
  int gs;
  const int kept = split_axis_kept(a.KW, a.DW, a.SW, a.PW, a.W, a.Wo, &gs);
  if (gs > 2 || (a.W & 3)) return 0;
  if (gs == 1) return kept == a.W ? 3 : 0;
  return kept == a.W / 2 ? 4 : 0;
}
// Tiles of whole images whose patch is the whole input plane (every row, every column): a plane is then one contiguous run of
// H*W floats in memory AND in the patch, so with H*W % 4 == 0 the 16-byte fetch of XM 3 works on the flattened plane whatever
// W is (ResNet50's 14x14 maps).
static bool split_plane_flat(const FwdArgs& a) {
  if ((a.HW & 3) || a.t_R != a.Ho || a.t_Wt != a.Wo) return false;
  int gh, gw;
  const int kh = split_axis_kept(a.KH, a.DH, a.SH, a.PH, a.H, a.Ho, &gh), kw = split_axis_kept(a.KW, a.DW, a.SW, a.PW, a.W, a.Wo, &gw);
  return gh == 1 && gw == 1 && kh == a.H && kw == a.W;
}

// Tile geometry as bt_fused_dispatch.h's fast_geometry (tile_shape), with the split flavour's capacity: the patch of ONE octet plane has to
// fit XPO pixels. Fills the tile fields and returns the tile's live columns (0: does not fit).
template <int BM, bool FLIP = false>
static int split_geometry(FwdArgs& a) {
  int nh, nw, dys, dxs, nh_min = 0, nw_min = 0;
  tap_window(a.KH, a.DH, a.SH, a.PH, a.H, a.Ho, a.pixel_major != 0 || a.row_taps != 0, &nh, &dys, &nh_min);   // (row tiles: the window of ONE output row)
  tap_window(a.KW, a.DW, a.SW, a.PW, a.W, a.Wo, a.pixel_major != 0, &nw, &dxs, &nw_min);
  // One active tap: the canonical K order pairs consecutive octets in one MFMA step, so a stage has to hold TWO octet planes
  // whatever the tile (otherwise the pairing, and with it the rounding, would depend on the tile choice). Pixel-major tiles
  // prune per pixel: the rule applies when some pixel is left with a single tap.
  const bool one_tap = a.pixel_major ? nh_min * nw_min <= 1 : nh * nw <= 1;
  const long long XPO = one_tap ? (split_xpo<BM, FLIP>() - 1) / 2 : split_xpo<BM, FLIP>() - 1;   // (one slot is the shared zero pixel)
  auto fits = [&](int NI, int R, int Wt) {
    // the patch stores only pixels that exist: at most the window's rows / columns, at most the image's (on the patch grid)
    long long PHt = (long long)(R - 1) * (dys ? a.SH : 1) + dys + 1, PWt = (long long)(Wt - 1) * (dxs ? a.SW : 1) + dxs + 1;
    const long long rows_max = dys ? a.H : (a.H - 1) / a.SH + 1, cols_max = dxs ? a.W : (a.W - 1) / a.SW + 1;
    if (PHt > rows_max) PHt = rows_max;
    if (PWt > cols_max) PWt = cols_max;
    return NI * PHt * PWt <= XPO;
  };
  int NI, R, Wt;
  if (!tile_shape(a, BM, a.HoWo == 1 || a.pixel_major, true, fits, &NI, &R, &Wt)) return 0;   // (row tiles, bt_fused_split.hip: images x one output row of 2-row maps)
  a.t_NI = NI, a.t_R = R, a.t_Wt = Wt;
  a.n_bt = (a.B + NI - 1) / NI;
  a.n_rt = (a.pixel_major || a.row_taps) ? a.Ho : (a.HoWo > 1 ? (a.Ho + R - 1) / R : 1);
  a.n_ct = a.pixel_major ? a.Wo : (a.HoWo > 1 ? (a.Wo + Wt - 1) / Wt : 1);
  a.m_tiles = a.n_bt * a.n_rt * a.n_ct;
  return NI * R * Wt;
}

// Cost of a launch of BM-wide tiles (b: split_geometry's plan, live: its return) in column-equivalents: rounds of 256 workgroups x
// (the tile's columns, but never less than the weight synthesis of a stage costs the producers (synth), + the prologue / output
// stage of a workgroup (fixed)). Tiles that do not fit or waste more than a quarter of their columns cost 1e30.
static double split_tile_cost(const FwdArgs& b, int live, int BM, int synth, int fixed) {
  if (!live) return 1e30;
  const double eff = (double)b.M / ((double)b.m_tiles * BM);
  if (eff < 0.75) return 1e30;
  const double rounds = (double)(((long long)b.G * b.n_tiles * b.S * b.m_tiles + 255) / 256);
  return rounds * ((BM > synth ? BM : synth) + fixed);
}

// Tiles of the stems' quad flavour (bt_fused_split_quad.h): BM columns of whole images, or of a band of whole rows of one image,
// whose patch fits xcap pixels. Fills the tile fields; false when the layer has no such tile.
static bool quad_geometry(FwdArgs& a, int BM, long long xcap) {
  if (a.pixel_major || a.T > 64 || !a.out_vec4 || a.HoWo < 2 || a.Wo > BM) return false;
  int nh, nw, dys, dxs;
  tap_window(a.KH, a.DH, a.SH, a.PH, a.H, a.Ho, false, &nh, &dys);
  tap_window(a.KW, a.DW, a.SW, a.PW, a.W, a.Wo, false, &nw, &dxs);
  const long long PWt = (long long)(a.Wo - 1) * (dxs ? a.SW : 1) + dxs + 1;
  auto rows_px = [&](int R) { return ((long long)(R - 1) * (dys ? a.SH : 1) + dys + 1) * PWt; };
  // whole images, or a band of whole rows of one image (ImageNet stems: 112 x 112 outputs -> 4 rows per 512-wide tile)
  if (a.HoWo > BM && a.ep_pool) return false;   // (the pooled read-out needs whole images: the caller pools in a separate pass)
  int NI, R, Wt;
  if (!tile_shape(a, BM, false, true, [&](int ni, int r, int) { return ni * rows_px(r) <= xcap; }, &NI, &R, &Wt)) return false;
  const long long tiles_per_sample = (long long)((a.B + NI - 1) / NI) * ((a.Ho + R - 1) / R);
  if ((double)a.M / ((double)tiles_per_sample * BM) < 0.75) return false;   // the wide tile must be filled
  if (a.ep_pool) {
    const int Wp = a.ep_Wp;
    if ((Wp & (Wp - 1)) != 0 || Wp < 4 || Wp > 16 || a.ep_res) return false;
  }
  a.n_tiles = (a.Cog + 63) / 64;
  a.t_NI = NI, a.t_R = R, a.t_Wt = a.Wo, a.n_bt = (a.B + NI - 1) / NI, a.n_rt = (a.Ho + R - 1) / R, a.n_ct = 1, a.m_tiles = a.n_bt * a.n_rt;
  return true;
}

// ---------------------------------------------------------------------------- the general kernel's tile
// What the two chains plan differently. Candidate widths, widest first: 512 / 256 / 128 for Reparameterization; 256 / 128 for Flipout
// (its two accumulator sets fill the consumers' registers at 32 x 128 per wave), and no 256 for pixel-major tiles. The producers'
// synthesis floor of a width (the 128-wide Reparameterization tile has 8 producer waves, the others 4) and the fixed cost of a
// workgroup, both in column-equivalents (split_tile_cost).
constexpr int kSplitWidths[3] = {512, 256, 128};
template <bool FLIP>
constexpr int split_synth(int bm) { return FLIP || bm == 128 ? 128 : 256; }
template <bool FLIP>
constexpr int split_fixed() { return FLIP ? 48 : 96; }

// x fetch mode of a planned tile (bt_fused_split.h): tiny input planes are read as 16-byte vectors. Flipout's rule is the
// Reparameterization one restricted to what it instantiates: whole stride-1 rows (3) for the 256-wide tile, 1x1 planes (1) for the
// 128-wide one.
template <bool FLIP>
static int split_x_mode(FwdArgs& a, int bm) {
  if ((((uintptr_t)a.x) & 15u) || (a.x_sample_stride & 3)) return 0;
  int xm = 0;
  if (a.HW == 1) xm = 1;
  else if (bm != 128 && !a.pixel_major && a.HW > 1 && (a.W & 3) == 0 && a.t_Wt == a.Wo && split_row_mode(a)) xm = split_row_mode(a);
  else if constexpr (!FLIP) {
    if (bm != 128 && !a.pixel_major && a.HW > 1 && split_plane_flat(a)) xm = 3, a.x_flat = 1;
    else if (bm == 128 && !a.pixel_major && a.H == 2 && a.W == 2 && split_plane_flat(a)) xm = 2;   // whole 2x2 planes (a strided 3x3 down to 1x1 maps)
    else if (bm != 512 && a.row_taps && a.H == 2 && a.W == 2 && a.KW == 3 && a.PW == 1 && a.SW == 1 && a.DW == 1) xm = 2;   // a row tile's patch is the whole 2x2 plane
    else if (a.pixel_major && a.H == 2 && a.W == 2 && a.KH == 3 && a.KW == 3 && a.PH == 1 && a.PW == 1 && a.SH == 1 && a.SW == 1 && a.DH == 1 && a.DW == 1) xm = 2;
  }
  if constexpr (FLIP) {
    if (bm == 256 ? !(xm == 3 && a.SH == 1 && a.SW == 1) : xm != 1) xm = 0;
  }
  return xm;
}

// The general split kernel's tile for one tile kind: the cheapest candidate width (split_geometry, split_tile_cost), the grid, the x
// fetch mode and the decode's reciprocals. Fills `a` and returns BT_OK with (bm, xm), or 1 when no tile applies.
template <bool FLIP>
static int split_plan(FwdArgs& a, int mode, int* bm_out, int* xm_out) {
  if (a.T > 9) return 1;   // at most 9 taps
  const int Mdom = a.pixel_major ? a.B : a.M;
  if (Mdom < 112) return 1;
  a.n_tiles = (a.Cog + 63) / 64;
  FwdArgs cand[3] = {a, a, a};
  int live[3] = {0, 0, 0};
  if constexpr (!FLIP) {
    if (Mdom >= 512) live[0] = split_geometry<512>(cand[0]);
  }
  if (Mdom >= 256 && !(FLIP && a.pixel_major)) live[1] = split_geometry<256, FLIP>(cand[1]);
  live[2] = split_geometry<128, FLIP>(cand[2]);
  double cost[3];
  for (int i = 0; i < 3; ++i) cost[i] = split_tile_cost(cand[i], live[i], kSplitWidths[i], split_synth<FLIP>(kSplitWidths[i]), split_fixed<FLIP>());
  int pick = -1;
  if constexpr (!FLIP) {
    static const int force_bm = [] { const char* e = getenv("BT_FORCE_BM"); return e ? atoi(e) : 0; }();   // measurement knob: prefer this tile width where it is eligible
    for (int i = 0; i < 3; ++i)
      if (force_bm == kSplitWidths[i] && cost[i] < 1e30) pick = i;
  }
  for (int i = 0; i < 3 && pick < 0; ++i) {   // the widest tile that no narrower one beats
    bool best = cost[i] < 1e30;
    for (int j = i + 1; j < 3; ++j) best = best && cost[i] <= cost[j];
    if (best) pick = i;
  }
  if (pick < 0) return 1;
  const int bm = kSplitWidths[pick];
  const long long per = (long long)a.G * a.n_tiles * a.S;
  a = cand[pick];
  if constexpr (!FLIP) {
    // A 128-wide launch that offers at most one workgroup per two CUs (a training step's single sample; an MLP's wide first layer at 8
    // samples) runs in 32-channel tiles instead: twice the workgroups, each drawing half the weights -- the chain of a workgroup of such a
    // layer IS its weight synthesis. The K order does not depend on the channel tile, so the results are the same bits (and the choice may
    // depend on S). BT_BN32 = 0 | 1 forces it off / on where eligible (tests, measurement).
    a.bn32 = 0;
    if (bm == 128 && mode != 2 && a.Cog > 32) {
      const int forced = g_bn32.get();
      a.bn32 = forced >= 0 ? forced : (2 * per * a.m_tiles <= 256 ? 1 : 0);
    }
    if (a.bn32) a.n_tiles = (a.Cog + 31) / 32;
  }
  if (!set_grid(a, (long long)a.G * a.n_tiles * a.S * a.m_tiles)) return 1;
  *bm_out = bm, *xm_out = split_x_mode<FLIP>(a, bm);
  split_fill_inverses(a);
  return BT_OK;
}

// ---------------------------------------------------------------------------- chains of same-shape layers
// Can the n layers m[0..n) -- each as bt::run fills it for a launch of its own, in execution order -- run as ONE launch of the chain
// kernel (bt_fused_split.h, CHAIN)? Every member is planned by split_plan exactly as its own launch would be, so a chained layer
// computes what it computes alone; the chain needs every plan to be the same whole-image 64 x 512 tile, member k to read what member
// k - 1 wrote, and no buffer to overlap another. BT_OK: m[k] hold their plans and *xm_out the common x fetch mode. 1: not a chain (a
// refusal is never an error: the caller launches the layers one by one).
static inline bool chain_overlap(const void* p, long long pn, const void* q, long long qn) {   // byte ranges [p, p + pn) and [q, q + qn)
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}
static int split_chain_plan(int n, FwdArgs* m, int mode, int* xm_out) {
  if (n < 1 || n > kChainMax || mode != 0) return 1;   // the exact split alone
  int xm0 = 0;
  for (int k = 0; k < n; ++k) {
    FwdArgs& a = m[k];
    // what launch_split_one asks of the general kernel's launches, and what only single launches do: a KL sweep, a pool, supplied draws
    if (!packed_ok(a) || a.eps_w || a.eps_b || a.sign_in || a.sign_out || a.updil || a.dwin || a.lowrank || a.ep_pool || a.do_kl || a.kl_out) return 1;
    if (a.Cig <= 4 || (a.Cig & 7) || a.pixel_major || a.HoWo <= 1 || a.H * a.W <= 1 || (a.KH == 1 && a.KW == 1)) return 1;   // (stems, one-pixel maps and 1x1 kernels have kernels of their own)
    if (a.G != 1 || a.SH != 1 || a.SW != 1) return 1;
    if (!a.out_vec4 && a.HoWo <= 4) return 1;   // the scalar output stage: not in the chain kernel (bt_fused_split.h, staged_out)
    int bm, xm;
    if (split_plan<false>(a, mode, &bm, &xm)) return 1;
    if (bm != 512 || (xm != 3 && xm != 0) || a.n_tiles != 1 || a.t_R != a.Ho || a.t_Wt != a.Wo || a.row_taps || a.bn32) return 1;
    if (k == 0) { xm0 = xm; continue; }
    const FwdArgs& f = m[0], &p = m[k - 1];
    if (xm != xm0 || a.t_NI != f.t_NI || a.n_bt != f.n_bt || a.m_tiles != f.m_tiles || a.total_blocks != f.total_blocks || a.S != f.S || a.B != f.B ||
        a.H != f.H || a.W != f.W || a.Ho != f.Ho || a.Wo != f.Wo)
      return 1;
    // one geometry: the workgroup decodes it once (the shapes, the window, the output layout)
    if (a.Ci != f.Ci || a.Co != f.Co || a.Cig != p.Cog || a.KH != f.KH || a.KW != f.KW || a.PH != f.PH || a.PW != f.PW || a.DH != f.DH || a.DW != f.DW ||
        a.out_vec4 != f.out_vec4 || a.x_flat != f.x_flat || a.x_elems != f.x_elems || a.out_elems != f.out_elems || a.seed_lo != f.seed_lo ||
        a.seed_hi != f.seed_hi || a.sample0 != f.sample0 || a.dbg != f.dbg)
      return 1;
    if (a.x != p.out || a.x_sample_stride != p.out_elems) return 1;   // member k reads what member k - 1 wrote, sample by sample
  }
  // No two of {chain input, outs} overlap; a residual is the chain input, something outside the chain, or exactly an EARLIER member's out.
  const long long xin = 4 * ((long long)(m[0].S - 1) * m[0].x_sample_stride + m[0].x_elems), on = 4 * (long long)m[0].S * m[0].out_elems;
  for (int k = 0; k < n; ++k) {
    if (chain_overlap(m[0].x, xin, m[k].out, on)) return 1;
    for (int j = 0; j < k; ++j)
      if (chain_overlap(m[j].out, on, m[k].out, on)) return 1;
    if (!m[k].ep_res) continue;
    const long long rn = 4 * ((long long)(m[k].S - 1) * m[k].ep_res_stride + m[k].out_elems);
    for (int j = 0; j < n; ++j) {
      if (!chain_overlap(m[k].ep_res, rn, m[j].out, on)) continue;
      if (j >= k || m[k].ep_res != m[j].out || m[k].ep_res_stride != m[j].out_elems) return 1;
    }
  }
  *xm_out = xm0;
  return BT_OK;
}

}  // namespace bt
