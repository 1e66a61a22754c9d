// Host dispatch of the fp32-MFMA forwards (bt_fused_fwd.h, bt_fused_fast.h). fp32_plan, a plain function, plans: form, tile, fast or
// general kernel, x staging mode and every plan field of FwdArgs; launch_fp32 turns the plan into the instantiation fp32_exists says
// there is. Included by bt_fused_{reparam,flipout}{,_inj,_updil,_dwin}.hip, one (FLIP, INJ, UPD, DWIN) each, so that their instantiations compile
// in parallel. tests/test_fp32_plan_parity.py pins what is planned.
#pragma once
#include "bt_fused_fast.h"

namespace bt {

extern EnvKnob g_force_generic;   // bt_fused_api.hip: A/B hook for tests and benchmarks (BT_FORCE_GENERIC: any value; bt_debug_force_generic)

// Workgroup tile = bn output channels x bm output positions, 4 consumer waves of (bn / cwn) x (bm / cwm) each; form; fast or general
// kernel; the fast flavour's pooled twin and x staging (bt_fused_fast.h: 0 patch, 1 row chunks, 2 channel vectors).
struct Fp32Plan { int bn, bm, cwn; bool linear, trans, fast, pool; int xmode; };

// ---------------------------------------------------------------------------- the instantiation table
// The kernels there are. kind 0: fused_fwd_kernel (general), 1: fused_fast_kernel (on-chip draws, not dilated). Forms: LINEAR (float4
// rows; always TRANS), conv TRANS, conv. Wide tiles: Reparameterization has one accumulator set, Flipout two; Flipout's 64x256 and the
// 64x512 stage x as a patch (fast flavour only).
constexpr bool fp32_exists(int kind, int bn, int bm, bool flip, bool linear, bool trans, bool inj, bool upd, int xmode, bool pool) {
  const bool onchip = !inj && !upd;
  if ((linear && !trans) || (upd && (linear || inj))) return false;
  const bool narrow = (bn == 128 && bm == 32) || (bn == 64 && bm == 64) || (bn == 32 && bm == 128) || (bn == 128 && bm == 128) || (bn == 64 && bm == 128);
  const bool wide = flip ? (bn == 64 && bm == 256 && !linear && onchip)
                         : ((bn == 128 && bm == 256) || (bn == 64 && bm == 256) || (bn == 64 && bm == 512 && !linear && onchip));
  if (!narrow && !wide) return false;
  if (kind == 0) return bm <= (flip ? 128 : 256) && xmode == 0 && !pool;
  if (!onchip) return false;
  if (pool) return xmode == 1 && trans && !linear && !flip && bm >= 128;
  return xmode == 0 || (xmode == 1 && !linear && !flip && bm >= 128) || (xmode == 2 && !linear && bm <= 128);
}

// ---------------------------------------------------------------------------- the planner
// Tile geometry of the specialised kernel (bt_fused_fast.h): t_NI images x t_R output rows x t_Wt output columns per tile,
// chosen so the x patch of 4 channels (worst case: every tap active) fits the LDS x buffer. Returns false, with `a` untouched,
// when this launch has to run the general kernel.
static bool fast_geometry(FwdArgs& a, int bm, bool linear, bool flip) {
  if (g_force_generic.get() || !packed_ok(a) || a.T > kMaxTaps / 2) return false;
  const long long XW = x_words(bm, flip);
  const int dys = (a.KH - 1) * a.DH, dxs = (a.KW - 1) * a.DW;
  auto fits = [&](int NI, int R, int Wt) {
    if (linear) return true;
    const long long PHt = (long long)(R - 1) * (dys ? a.SH : 1) + dys + 1, PWt = (long long)(Wt - 1) * (dxs ? a.SW : 1) + dxs + 1;
    const long long PCH = NI * PHt * PWt;
    return 4 * PCH <= XW && PCH < 65536;
  };
  int NI, R, Wt;
  if (!tile_shape(a, bm, linear || a.HoWo == 1 || a.pixel_major, false, fits, &NI, &R, &Wt)) return false;
  const bool grid = a.pixel_major || (!linear && a.HoWo > 1);
  // Row-chunk staging of the x patch (16-byte pieces of input rows copied straight into LDS): needs 16-byte aligned rows
  // and the slightly wider patch to fit with the same tile. Flipout stages x through registers (it multiplies by the signs).
  a.x_cvec = (!linear && (((uintptr_t)a.x) & 15u) == 0 && (a.x_sample_stride & 3) == 0 && (((long long)a.Ci * a.HW) & 3) == 0 && (a.Cig & 3) == 0) ? 1 : 0;
  a.x_rows = 0;
  if (!linear && !flip && !a.pixel_major && a.HoWo > 1 && (a.W & 3) == 0 && (((uintptr_t)a.x) & 15u) == 0 && (a.x_sample_stride & 3) == 0) {
    const long long PHt = (long long)(R - 1) * (dys ? a.SH : 1) + dys + 1;
    int xa;   // chunks per row. The tile spans the row: exact (all taps active is the worst case); column segments: any alignment of the first column
    const int n = Wt == a.Wo ? row_chunks(-a.PW, -a.PW + (Wt - 1) * a.SW + dxs, a.W, &xa) : (((Wt - 1) * a.SW + dxs + 1 + 3) >> 2) + 1;
    const long long PCH = NI * PHt * 4 * n + 4;
    if (4 * PCH <= XW && PCH < 65536) a.x_rows = 1;
  }
  a.t_NI = NI, a.t_R = R, a.t_Wt = Wt;
  a.n_bt = (a.B + NI - 1) / NI;
  a.n_rt = grid ? (a.Ho + R - 1) / R : 1;
  a.n_ct = grid ? (a.Wo + Wt - 1) / Wt : 1;
  a.m_tiles = a.n_bt * a.n_rt * a.n_ct;
  return true;
}

static inline long long tiles_for(const FwdArgs& a, int BN, int BM) {
  const long long nt = (a.Cog + BN - 1) / BN;
  long long mt = a.pixel_major ? (long long)a.HoWo * ((a.B + BM - 1) / BM) : (a.M + BM - 1) / BM;
  if (!a.pixel_major && a.HoWo > 1 && a.HoWo <= BM) mt = (a.B + BM / a.HoWo - 1) / (BM / a.HoWo);  // whole-image tiles
  return (long long)a.G * nt * a.S * mt;
}

// The size-driven tile. Wide BM amortises one weight draw over more MFMA work (the producers' VALU budget); a launch should still
// offer >= 256 workgroups (one per CU), so tiles shrink when the grid would not fill the chip. The two fast-only wide tiles are taken
// only when their geometry fills them, and that geometry is then already planned into `a`: returns true.
static bool tile_by_size(FwdArgs& a, bool flip, bool linear, bool onchip, Fp32Plan* p) {
  constexpr long long kCUs = 256;
  const int Mdom = a.pixel_major ? a.B : a.M;
  auto tile = [&](int bn, int bm, int cwn, bool planned = false) { return p->bn = bn, p->bm = bm, p->cwn = cwn, planned; };
  auto filled = [&](int bm, int live) {   // (a 256-pixel image whose 2-image patch does not fit would leave half of a 512-wide tile dead)
    FwdArgs g = a;
    if (!fast_geometry(g, bm, false, flip) || g.t_NI * g.t_R * g.t_Wt < live) return false;
    a = g;
    return true;
  };
  if (Mdom <= 32) return tile(128, 32, 4);
  if (Mdom <= 64) return tile(64, 64, 2);
  if (a.Cog <= 32) return tile(32, 128, 1);
  if (!flip) {  // wide tiles: one accumulator set fits in the consumers' registers (Flipout carries two)
    // 512-wide: fast flavour only (x as a patch); halves the weight-synthesis work per MFMA
    if (!linear && onchip && Mdom >= 512 && tiles_for(a, 64, 512) >= kCUs && filled(512, 448)) return tile(64, 512, 1, true);
    if (Mdom >= 256 && a.Cog > 64 && tiles_for(a, 128, 256) >= kCUs) return tile(128, 256, 2);
    if (Mdom >= 256 && tiles_for(a, 64, 256) >= kCUs) return tile(64, 256, 1);
  } else if (!linear && onchip) {
    // Flipout's wide tile: 64x256, fast flavour only (two accumulator sets of 64 registers; x as a patch within the
    // 128-column LDS budget). Halves the weight synthesis per MFMA on the large feature maps.
    if (Mdom >= 256 && ((a.SH == 1 && a.SW == 1) || a.T > 9) && tiles_for(a, 64, 256) >= kCUs && filled(256, 224))  // (strided 3x3: measured slower; stems: faster)
      return tile(64, 256, 1, true);
  }
  if (a.Cog > 64 && tiles_for(a, 128, 128) >= kCUs) return tile(128, 128, 2);
  return tile(64, 128, 2);
}

// The rest of the plan for the tile in `p`: fast or general kernel, its geometry, the grid, the x staging mode.
static int plan_tile(FwdArgs& a, bool flip, bool inj, bool upd, bool planned, Fp32Plan* p) {
  const int bn = p->bn, bm = p->bm;
  auto exists = [&](int kind, int xmode, bool pool) { return fp32_exists(kind, bn, bm, flip, p->linear, p->trans, inj, upd, xmode, pool); };
  a.n_tiles = (a.Cog + bn - 1) / bn;
  // draws injected in the NATURAL layout: always the general kernel (packed ones, BT_DRAWS_EPS_PACKED, never come here: bt_fused_split_inj.hip)
  p->fast = planned || (!inj && !upd && fast_geometry(a, bm, p->linear, flip));
  p->pool = a.ep_pool != 0, p->xmode = 0;
  if (a.ep_pool && !(p->fast && a.x_rows && exists(1, 1, true) && a.out_vec4 && !a.pixel_major && a.t_R == a.Ho && a.t_Wt == a.Wo))
    return set_error(BT_ERR_UNSUPPORTED, "fused max-pool: this launch's tiles do not hold whole output images");
  if (!p->fast) {  // general kernel: BM consecutive (b, ho, wo), or pixel-major
    a.mt_per_pixel = a.pixel_major ? (a.B + bm - 1) / bm : 1;
    a.m_tiles = a.pixel_major ? a.HoWo * a.mt_per_pixel : (a.M + bm - 1) / bm;
    a.patch_ok = (!p->linear && (a.pixel_major || (a.HoWo <= bm && bm % a.HoWo == 0))) ? 1 : 0;
  }
  if (!set_grid(a, (long long)a.G * a.n_tiles * a.S * a.m_tiles)) return set_error(BT_ERR_UNSUPPORTED, "fused forward: grid too large");
  if (!p->fast) return exists(0, 0, false) ? BT_OK : set_error(BT_ERR_UNSUPPORTED, "fused forward: this tile exists in the fast flavour only");
  // x staging mode (bt_fused_fast.h): row chunks need the wide spatial tiles, channel vectors the narrow ones
  if (a.x_rows && exists(1, 1, false)) p->xmode = 1;
  else if (a.x_cvec && (a.HW == 1 || a.HW == 4) && exists(1, 2, false)) p->xmode = 2;
  return BT_OK;
}

// Plans the launch of `a` (the geometry bt::run filled; `linear`: a Linear entry point) and fills a's plan fields: BT_OK, or the
// refusal set_error made. upd: an input-dilated launch (FwdArgs::updil). Its tile is chosen as for the launch over the virtual image,
// among the tiles the general kernel has.
static int fp32_plan(FwdArgs& a, bool flip, bool linear, bool inj, bool upd, Fp32Plan* p) {
  if (upd && a.ep_pool) return set_error(BT_ERR_UNSUPPORTED, "fused max-pool: not available on an input-dilated or depth-window launch");
  p->linear = !upd && linear && a.w_vec && a.x_vec;   // float4 rows; any other Linear is a 1x1 conv over 1x1 images: the same memory layout
  p->trans = p->linear || a.HoWo == 1 || a.pixel_major || a.out_vec4;
  const bool onchip = !inj && !upd;
  const FwdArgs a0 = a;
  const bool planned = tile_by_size(a, flip, p->linear, onchip, p);
  int rc = plan_tile(a, flip, inj, upd, planned, p);
  // The fused max-pool needs tiles of whole images. When the size-driven tile is refused (small batches pick narrow tiles): the
  // narrowest tile that can hold an image (the pooled read-out lives in the row-chunk instantiations: Reparameterization, aligned x).
  if (rc == BT_ERR_UNSUPPORTED && a0.ep_pool && !flip && !p->linear && onchip && a0.HoWo <= 512) {
    a = a0;
    if (a.HoWo <= 128) p->bn = 64, p->bm = 128, p->cwn = 2;
    else p->bn = 64, p->bm = a.HoWo <= 256 ? 256 : 512, p->cwn = 1;
    rc = plan_tile(a, flip, inj, upd, false, p);
  }
  return rc;
}

// ---------------------------------------------------------------------------- the launch
// DWIN (with UPD: planned like an input-dilated launch, the general kernel alone): a depth-window launch (FwdArgs::dwin), the
// kernel's DWIN form instead of its UPD one.
template <int KIND, int BN, int BM, int CWN, bool FLIP, bool LINEAR, bool TRANS, bool INJ, bool UPD, int XMODE, bool POOL, bool DWIN = false>
static int launch_inst(const FwdArgs& a, hipStream_t stream) {
  if constexpr (!fp32_exists(KIND, BN, BM, FLIP, LINEAR, TRANS, INJ, UPD, XMODE, POOL)) {
    return set_error(BT_ERR_UNSUPPORTED, KIND ? "fused forward: the plan names a fast kernel that is not instantiated" : "fused forward: this tile exists in the fast flavour only");
  } else {
    constexpr int lds = fused_lds_bytes<BN, BM, FLIP>();
    static_assert(lds <= 160 * 1024, "LDS budget of one CU");
    char nm[160];   // (bt_last_kernel_name: tests and bench.py's tables parse the two formats)
    const char *fl = FLIP ? "flip" : "reparam", *li = LINEAR ? "linear" : "conv", *tr = TRANS ? "trans" : "notrans";
    if constexpr (KIND == 0) {
      snprintf(nm, sizeof(nm), "fused_fwd_kernel<%d,%d,%d,%s,%s,%s,inj=%d%s>", BN, BM, CWN, fl, li, tr, INJ ? 1 : 0, DWIN ? ",dwin" : UPD ? ",updil" : "");
      return launch_kernel(fused_fwd_kernel<BN, BM, CWN, FLIP, LINEAR, TRANS, INJ, UPD && !DWIN, DWIN>, nm, "fused forward", dim3((unsigned)a.total_blocks), dim3(kThreads),
                           lds, lds, stream, a);
    } else {
      // narrow conv tiles: 8 producer waves (their accumulators leave room for 12 waves of <= 168 registers)
      constexpr int NPW = (!LINEAR && BM <= 128 && BN * BM <= 128 * 128) ? 8 : 4;
      snprintf(nm, sizeof(nm), "fused_fast_kernel<%d,%d,%d,%s,%s,%s,inj=0,xmode=%d,npw=%d,pool=%d>", BN, BM, CWN, fl, li, tr, XMODE, NPW, POOL ? 1 : 0);
      return launch_kernel(fused_fast_kernel<BN, BM, CWN, FLIP, LINEAR, TRANS, false, XMODE, NPW, POOL>, nm, "fused forward (fast)",
                           dim3((unsigned)a.total_blocks), dim3(256 + 64 * NPW), lds, lds, stream, a);
    }
  }
}

template <int BN, int BM, int CWN, bool FLIP, bool LINEAR, bool TRANS, bool INJ, bool UPD, bool DWIN>
static int launch_form(const FwdArgs& a, const Fp32Plan& p, hipStream_t stream) {
  if (!p.fast) return launch_inst<0, BN, BM, CWN, FLIP, LINEAR, TRANS, INJ, UPD, 0, false, DWIN>(a, stream);
  if (p.pool) return launch_inst<1, BN, BM, CWN, FLIP, LINEAR, TRANS, INJ, UPD, 1, true>(a, stream);
  if (p.xmode == 1) return launch_inst<1, BN, BM, CWN, FLIP, LINEAR, TRANS, INJ, UPD, 1, false>(a, stream);
  if (p.xmode == 2) return launch_inst<1, BN, BM, CWN, FLIP, LINEAR, TRANS, INJ, UPD, 2, false>(a, stream);
  return launch_inst<1, BN, BM, CWN, FLIP, LINEAR, TRANS, INJ, UPD, 0, false>(a, stream);
}

template <int BN, int BM, int CWN, bool FLIP, bool INJ, bool UPD, bool DWIN>
static int launch_tile(const FwdArgs& a, const Fp32Plan& p, hipStream_t stream) {
  if (p.linear) return launch_form<BN, BM, CWN, FLIP, true, true, INJ, UPD, DWIN>(a, p, stream);
  if (p.trans) return launch_form<BN, BM, CWN, FLIP, false, true, INJ, UPD, DWIN>(a, p, stream);
  return launch_form<BN, BM, CWN, FLIP, false, false, INJ, UPD, DWIN>(a, p, stream);
}

// The planned kernel, among those of this translation unit's (FLIP, INJ, UPD).
template <bool FLIP, bool INJ, bool UPD, bool DWIN>
static int launch_fp32(const FwdArgs& a, const Fp32Plan& p, hipStream_t stream) {
  switch (p.bn * 1024 + p.bm) {
    case 128 * 1024 + 32: return launch_tile<128, 32, 4, FLIP, INJ, UPD, DWIN>(a, p, stream);
    case 64 * 1024 + 64: return launch_tile<64, 64, 2, FLIP, INJ, UPD, DWIN>(a, p, stream);
    case 32 * 1024 + 128: return launch_tile<32, 128, 1, FLIP, INJ, UPD, DWIN>(a, p, stream);
    case 64 * 1024 + 512: return launch_tile<64, 512, 1, FLIP, INJ, UPD, DWIN>(a, p, stream);
    case 128 * 1024 + 256: return launch_tile<128, 256, 2, FLIP, INJ, UPD, DWIN>(a, p, stream);
    case 64 * 1024 + 256: return launch_tile<64, 256, 1, FLIP, INJ, UPD, DWIN>(a, p, stream);
    case 128 * 1024 + 128: return launch_tile<128, 128, 2, FLIP, INJ, UPD, DWIN>(a, p, stream);
    case 64 * 1024 + 128: return launch_tile<64, 128, 2, FLIP, INJ, UPD, DWIN>(a, p, stream);
  }
  return set_error(BT_ERR_UNSUPPORTED, "fused forward: the plan names a tile that is not instantiated");
}

// One translation unit's launcher. On-chip draws: the split-precision chain first (natural-layout injected draws never take it). Then
// plan and launch: on BT_OK the plan that ran is in `ran`.
template <bool FLIP, bool INJ, bool UPD = false, bool DWIN = false>
static int run_fp32(bool linear, const FwdArgs& a, FwdArgs& ran, hipStream_t stream) {
  if constexpr (!INJ) {
    const int rc = FLIP ? launch_split_flip(a, ran, stream) : launch_split(a, ran, stream);
    if (rc <= 0) return rc;
  }
  Fp32Plan p;
  ran = a;
  if (int rc = fp32_plan(ran, FLIP, linear, INJ, UPD, &p)) return rc;
  return launch_fp32<FLIP, INJ, UPD, DWIN>(ran, p, stream);
}

}  // namespace bt
