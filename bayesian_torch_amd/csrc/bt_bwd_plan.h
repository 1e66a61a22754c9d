// The training backward's launch plan: everything bt_bwd.hip's host side derives from a geometry before it launches -- extents, the
// split of wgrad's reduction and of dgrad's output channels, the two grids, the finishing passes, whether the passes pair, and the
// workspace's two slabs. Host only: no kernel, no HIP call (tools/bwd_plan_check.hip walks it under the sanitizers).
#pragma once
#include <initializer_list>

#include "bt_api_internal.h"

namespace bt {

constexpr int kBK = 16;   // reduction steps per LDS stage

// Measurement knobs (hooks: bt_debug_bwd_targets, bt_debug_bwd_pair): the workgroups a pass should offer; the passes as launches of their own.
// wgrad: one workgroup per CU -- the pass runs beside dgrad in one launch (bwd_pair_kernel) and every group costs a partial that the
// finishing pass reads back (ResNet18 step, env sweep: 512 -> 3.14 ms, 256 -> 2.97, 192 -> 2.98, 128 -> 3.24, 1024 -> 3.22).
constexpr int kWgradWgs = 256, kDgradWgs = 512;
inline EnvKnob g_wgrad_wgs{"BT_WGRAD_WGS", [](const char* e) { const int v = e ? atoi(e) : 0; return v > 0 ? v : kWgradWgs; }};
inline EnvKnob g_dgrad_wgs{"BT_DGRAD_WGS", [](const char* e) { const int v = e ? atoi(e) : 0; return v > 0 ? v : kDgradWgs; }};
inline EnvKnob g_no_bwd_pair{"BT_NO_BWD_PAIR", [](const char* e) { return (e && *e && *e != '0') ? 1 : 0; }};

struct BwdPlan {
  int Ho, Wo, Cig, Cog, Cig4, T;
  long long M;                              // wgrad's reduction axis B*Ho*Wo
  long long x_elems, out_elems, w_elems;
  int groups, sgroups, mchunk;              // wgrad: groups = sgroups (sample s handled by s % sgroups) x chunks of mchunk rows of M
  int dchunks, dchunk;                      // dgrad: the output channels in dchunks pieces of dchunk
  unsigned wgrid[3], dgrid[3];              // wgrad: (k' tiles, co tiles, groups * G); dgrad: (position tiles, ci tiles, S * G * dchunks)
  long long wblocks, dblocks;
  int n_wfin, n_dfin;                       // blocks of the finishing passes (n_dfin 0: dgrad in one piece writes dx itself)
  bool pair;                                // both gradients asked for: one launch for the two passes, one for the two finishing passes
  size_t wgrad_bytes, dgrad_bytes;          // the workspace: wgrad's partials [2][groups][Co][T][Cig4], then dgrad's [dchunks][S][x_elems]
  size_t part_d_offset;                     // where dgrad's begin
};
enum BwdRefusal { kBwdOk = 0, kBwdBadGeometry, kBwdEmptyOutput, kBwdTooLarge };

// f[0] * f[1] * ... when it stays below 2^31 (factors >= 1), else -1
inline long long product_below_2_31(std::initializer_list<long long> f) {
  long long v = 1;
  for (long long x : f)
    if (x >= (1ll << 31) || (v *= x) >= (1ll << 31)) return -1;
  return v;
}

// Workgroups per output tile: first the samples (each group keeps whole samples), then chunks of the reduction axis
// M = B*Ho*Wo (a training step has ONE sample: layer1's 9 output tiles would otherwise be 9 workgroups on 256 CUs).
// Chunks are multiples of the LDS stage and at least 8 stages long.
inline void wgrad_groups(const bt_conv2d_geom& g, int S, BwdPlan& p) {
  const long long tiles = (long long)((p.T * p.Cig4 + 63) / 64) * ((p.Cog + 63) / 64) * g.groups;
  long long gr = (g_wgrad_wgs.get() + tiles - 1) / tiles;
  if (gr < 1) gr = 1;
  const long long gs = gr > S ? S : gr;
  long long gm = (gr + gs - 1) / gs;
  const long long max_gm = (p.M + 8 * kBK - 1) / (8 * kBK);
  if (gm > max_gm) gm = max_gm;
  if (gm < 1) gm = 1;
  long long chunk = (p.M + gm - 1) / gm;
  chunk = (chunk + kBK - 1) / kBK * kBK;
  gm = (p.M + chunk - 1) / chunk;
  p.sgroups = (int)gs, p.mchunk = (int)chunk, p.groups = (int)(gs * gm);
}

// dgrad: pieces of the output-channel reduction, so that a launch offers ~512 workgroups (layer4 of a CIFAR ResNet at one
// sample: 16 tiles); pieces are multiples of the LDS stage and at least 32 channels.
inline void dgrad_chunks(const bt_conv2d_geom& g, int S, BwdPlan& p) {
  const long long M = (long long)g.B * g.H * g.W;
  const long long tiles = ((M + 63) / 64) * ((p.Cig + 63) / 64) * S * g.groups;
  long long c = (g_dgrad_wgs.get() + tiles - 1) / tiles;
  const long long max_c = (p.Cog + 31) / 32;
  if (c > max_c) c = max_c;
  if (c < 1) c = 1;
  long long per = (p.Cog + c - 1) / c;
  per = (per + kBK - 1) / kBK * kBK;
  p.dchunk = (int)per, p.dchunks = (int)((p.Cog + per - 1) / per);
}

// The plan of one backward over g with S samples, or why there is none. The gradients asked for decide only whether the passes pair.
inline int bwd_plan(const bt_conv2d_geom& g, int S, bool want_dx, bool want_w, BwdPlan* out) {
  BwdPlan p = {};
  if (S <= 0 || geom_error(g)) return kBwdBadGeometry;
  const long long Ho = conv_out_h(g), Wo = conv_out_w(g);
  if (Ho <= 0 || Wo <= 0) return kBwdEmptyOutput;
  p.Cig = g.Ci / g.groups, p.Cog = g.Co / g.groups;
  p.x_elems = product_below_2_31({g.B, g.Ci, g.H, g.W});
  p.out_elems = product_below_2_31({g.B, g.Co, Ho, Wo});
  p.w_elems = product_below_2_31({g.Co, p.Cig, g.kh, g.kw});
  if (p.x_elems < 0 || p.out_elems < 0 || p.w_elems < 0 || p.w_elems * 4 >= (1ll << 31)) return kBwdTooLarge;   // the 32-bit sign / draw indices
  p.Ho = (int)Ho, p.Wo = (int)Wo, p.Cig4 = (p.Cig + 3) & ~3, p.T = g.kh * g.kw, p.M = (long long)g.B * Ho * Wo;
  wgrad_groups(g, S, p);
  dgrad_chunks(g, S, p);
  const long long Md = (long long)g.B * g.H * g.W, dz = (long long)S * g.groups * p.dchunks, wz = (long long)p.groups * g.groups;
  if (dz > 0x7FFFFFFFll || wz > 0x7FFFFFFFll || p.M > 0x7FFFFFFFll - kBK) return kBwdTooLarge;   // (a grid dimension, or M rounded up to a stage, past an int)
  p.wgrid[0] = (unsigned)((p.T * p.Cig4 + 63) / 64), p.wgrid[1] = (unsigned)((p.Cog + 63) / 64), p.wgrid[2] = (unsigned)wz;
  p.dgrid[0] = (unsigned)((Md + 63) / 64), p.dgrid[1] = (unsigned)((p.Cig + 63) / 64), p.dgrid[2] = (unsigned)dz;
  p.wblocks = (long long)p.wgrid[0] * p.wgrid[1] * p.wgrid[2], p.dblocks = (long long)p.dgrid[0] * p.dgrid[1] * p.dgrid[2];
  const long long wfin = (p.w_elems + 255) / 256, dfin = ((long long)S * p.x_elems + 255) / 256;
  p.n_wfin = (int)(wfin > 4096 ? 4096 : wfin);
  p.n_dfin = p.dchunks > 1 ? (int)(dfin > 4096 ? 4096 : dfin) : 0;
  p.pair = want_dx && want_w && !g_no_bwd_pair.get() && p.wblocks + p.dblocks < 0x7FFFFFFFll;
  p.wgrad_bytes = (size_t)2 * p.groups * g.Co * p.T * p.Cig4 * sizeof(float);
  p.dgrad_bytes = p.dchunks > 1 ? (size_t)p.dchunks * S * (size_t)p.x_elems * sizeof(float) : 0;
  p.part_d_offset = p.wgrad_bytes;   // (the two passes run side by side in one launch when both are asked for)
  *out = p;
  return kBwdOk;
}

}  // namespace bt
