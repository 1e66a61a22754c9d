// Stand-alone host check of bt_bwd_plan.h, meant for AddressSanitizer / UBSan (no GPU, not loaded into Python):
//   make -C bayesian_torch_amd/csrc bwdcheck
// Over the launch sweep's geometries (tools/record_bwd_launches.py), the degenerate ones and extremes up to the 2^31 limits, at the
// sweep's workgroup targets, paired and not: a refusal is the one a slow restatement of the rules expects; a plan's wgrad_bytes and
// dgrad_bytes equal a recomputation written on its own (128-bit products, loops instead of closed forms), dgrad's partials begin
// exactly at wgrad_bytes, the chunks and pieces cover M and Cog with none empty, the grids multiply to the block counts.
#include <limits.h>
#include <stdio.h>

#include <vector>

#include "../bayesian_torch_amd/csrc/bt_bwd_plan.h"

static int failures = 0, plans = 0, refusals = 0;
#define CHECK(c)                                                                                        \
  do {                                                                                                  \
    if (!(c)) {                                                                                         \
      if (++failures <= 20) printf("FAILED line %d: %s   [%s]\n", __LINE__, #c, g_case);                \
    }                                                                                                   \
  } while (0)
static char g_case[256];

typedef __int128 wide;
static wide cdiv(wide a, wide b) { return (a + b - 1) / b; }

static bt_conv2d_geom geom(int B, int Ci, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int G) {
  bt_conv2d_geom g;
  g.B = B, g.Ci = Ci, g.H = H, g.W = W, g.Co = Co, g.kh = kh, g.kw = kw, g.sh = sh, g.sw = sw, g.ph = ph, g.pw = pw, g.dh = dh, g.dw = dw, g.groups = G;
  return g;
}

// the refusal a reading of the rules gives, in 128-bit arithmetic; for a plan also the output extents
static int expect(const bt_conv2d_geom& g, int S, wide& Ho, wide& Wo) {
  const int all[] = {g.B, g.Ci, g.H, g.W, g.Co, g.kh, g.kw, g.sh, g.sw, g.dh, g.dw, g.groups};
  for (int v : all)
    if (v <= 0) return bt::kBwdBadGeometry;
  if (S <= 0 || g.ph < 0 || g.pw < 0 || g.Ci % g.groups || g.Co % g.groups) return bt::kBwdBadGeometry;
  const wide nh = (wide)g.H + 2 * (wide)g.ph - (wide)g.dh * (g.kh - 1) - 1, nw = (wide)g.W + 2 * (wide)g.pw - (wide)g.dw * (g.kw - 1) - 1;
  Ho = nh / g.sh + 1, Wo = nw / g.sw + 1;   // (C++ division, as the library's)
  if (Ho <= 0 || Wo <= 0) return bt::kBwdEmptyOutput;
  const wide lim = (wide)1 << 31;
  if ((wide)g.B * g.Ci * g.H * g.W >= lim || (wide)g.B * g.Co * Ho * Wo >= lim || (wide)g.Co * (g.Ci / g.groups) * g.kh * g.kw * 4 >= lim) return bt::kBwdTooLarge;
  return bt::kBwdOk;
}

static void plan_case(const bt_conv2d_geom& g, int S, int wt, int dt, bool pair_on) {
  snprintf(g_case, sizeof(g_case), "B%d Ci%d %dx%d Co%d k%dx%d s%d,%d p%d,%d d%d,%d G%d S%d targets %d/%d pair %d", g.B, g.Ci, g.H, g.W, g.Co, g.kh, g.kw, g.sh, g.sw,
           g.ph, g.pw, g.dh, g.dw, g.groups, S, wt, dt, (int)pair_on);
  bt::g_wgrad_wgs.set(wt), bt::g_dgrad_wgs.set(dt), bt::g_no_bwd_pair.set(pair_on ? 0 : 1);
  // the plan sits in a heap block of exactly its size, so that a write past it is the sanitizer's to see
  bt::BwdPlan* p = new bt::BwdPlan();
  wide Ho = 0, Wo = 0;
  const int want = expect(g, S, Ho, Wo);
  const int got = bt::bwd_plan(g, S, true, true, p);
  if (want == bt::kBwdOk && got == bt::kBwdTooLarge) {   // the refusals beyond the tensor sizes: a grid dimension, or M rounded up to a stage, of 2^31 or more
    CHECK((wide)S * g.groups >= ((wide)1 << 31) / 4096 || (wide)g.B * Ho * Wo > ((wide)1 << 31) - 1 - bt::kBK);
    ++refusals;
    delete p;
    return;
  }
  CHECK(got == want);
  if (got != bt::kBwdOk || want != bt::kBwdOk) {
    ++refusals;
    delete p;
    return;
  }
  ++plans;
  const int G = g.groups, Cig = g.Ci / G, Cog = g.Co / G, T = g.kh * g.kw;
  int Cig4 = Cig;
  while (Cig4 % 4) ++Cig4;
  CHECK(p->Ho == (int)Ho && p->Wo == (int)Wo && p->Cig == Cig && p->Cog == Cog && p->Cig4 == Cig4 && p->T == T);
  const wide M = (wide)g.B * Ho * Wo, x_elems = (wide)g.B * g.Ci * g.H * g.W;
  CHECK(p->M == (long long)M && p->x_elems == (long long)x_elems && p->out_elems == (long long)(M * g.Co) && p->w_elems == (long long)((wide)g.Co * Cig * T));
  // wgrad: workgroups per tile towards the target, samples first, then chunks of M: whole LDS stages, at least 8 of them
  const wide wtiles = cdiv((wide)T * Cig4, 64) * cdiv(Cog, 64) * G;
  wide per_tile = cdiv(wt, wtiles);
  if (per_tile < 1) per_tile = 1;
  const wide sg = per_tile < S ? per_tile : S;
  wide chunks = cdiv(per_tile, sg);
  if (chunks > cdiv(M, 128)) chunks = cdiv(M, 128);
  wide rows = cdiv(M, chunks);
  while (rows % 16) ++rows;
  chunks = cdiv(M, rows);
  CHECK(p->sgroups == (int)sg && p->mchunk == (int)rows && p->groups == (int)(sg * chunks));
  CHECK(p->mchunk % bt::kBK == 0 && (wide)(p->groups / p->sgroups) * p->mchunk >= M && (wide)(p->groups / p->sgroups - 1) * p->mchunk < M);
  CHECK((wide)(p->groups / p->sgroups) <= cdiv(M, 8 * bt::kBK));   // (no more chunks than M holds runs of 8 stages)
  // dgrad: pieces of the output channels towards the target: whole LDS stages, at least 32 channels where there are several
  const wide dtiles = cdiv((wide)g.B * g.H * g.W, 64) * cdiv(Cig, 64) * S * G;
  wide pieces = cdiv(dt, dtiles);
  if (pieces > cdiv(Cog, 32)) pieces = cdiv(Cog, 32);
  if (pieces < 1) pieces = 1;
  wide per = cdiv(Cog, pieces);
  while (per % 16) ++per;
  pieces = cdiv(Cog, per);
  CHECK(p->dchunk == (int)per && p->dchunks == (int)pieces);
  CHECK((wide)p->dchunks * p->dchunk >= Cog && (wide)(p->dchunks - 1) * p->dchunk < Cog && (p->dchunks == 1 || p->dchunk >= 32));
  // the workspace
  const wide wbytes = (wide)2 * p->groups * g.Co * T * Cig4 * 4, dbytes = p->dchunks > 1 ? (wide)p->dchunks * S * x_elems * 4 : 0;
  CHECK((wide)p->wgrad_bytes == wbytes && (wide)p->dgrad_bytes == dbytes);
  CHECK(p->part_d_offset == p->wgrad_bytes);
  // grids and finishing passes
  CHECK((wide)p->wgrid[0] == cdiv((wide)T * Cig4, 64) && (wide)p->wgrid[1] == cdiv(Cog, 64) && (wide)p->wgrid[2] == (wide)p->groups * G);
  CHECK((wide)p->dgrid[0] == cdiv((wide)g.B * g.H * g.W, 64) && (wide)p->dgrid[1] == cdiv(Cig, 64) && (wide)p->dgrid[2] == (wide)S * G * p->dchunks);
  CHECK((wide)p->wblocks == (wide)p->wgrid[0] * p->wgrid[1] * p->wgrid[2] && (wide)p->dblocks == (wide)p->dgrid[0] * p->dgrid[1] * p->dgrid[2]);
  CHECK(p->n_wfin >= 1 && p->n_wfin <= 4096 && (wide)p->n_wfin == (cdiv((wide)g.Co * Cig * T, 256) > 4096 ? 4096 : cdiv((wide)g.Co * Cig * T, 256)));
  CHECK(p->dchunks > 1 ? (p->n_dfin >= 1 && p->n_dfin <= 4096 && (wide)p->n_dfin == (cdiv(S * x_elems, 256) > 4096 ? 4096 : cdiv(S * x_elems, 256))) : p->n_dfin == 0);
  CHECK(p->pair == (pair_on && (wide)p->wblocks + p->dblocks < 0x7FFFFFFF));
  bt::BwdPlan q = {};
  CHECK(bt::bwd_plan(g, S, true, false, &q) == bt::kBwdOk && !q.pair && q.wgrad_bytes == p->wgrad_bytes && q.dgrad_bytes == p->dgrad_bytes);
  CHECK(bt::bwd_plan(g, S, false, true, &q) == bt::kBwdOk && !q.pair && q.groups == p->groups && q.dchunks == p->dchunks);
  delete p;
}

int main() {
  std::vector<std::pair<bt_conv2d_geom, int>> cases;
  auto add = [&](bt_conv2d_geom g, int S) { cases.push_back({g, S}); };
  auto sq = [&](int B, int Ci, int HW, int Co, int k, int s, int p, int S) { add(geom(B, Ci, HW, HW, Co, k, k, s, s, p, p, 1, 1, 1), S); };
  // the rows of the gradient tests
  add(geom(5, 64, 7, 7, 72, 3, 3, 1, 1, 1, 1, 1, 1, 1), 2), add(geom(3, 12, 9, 8, 20, 3, 2, 2, 1, 1, 0, 1, 2, 2), 2), add(geom(4, 16, 7, 7, 24, 3, 3, 2, 2, 1, 1, 1, 1, 2), 2);
  add(geom(6, 4096, 1, 1, 130, 1, 1, 1, 1, 0, 0, 1, 1, 1), 3), add(geom(9, 130, 1, 1, 70, 1, 1, 1, 1, 0, 0, 1, 1, 1), 2), sq(2, 3, 16, 16, 7, 2, 3, 1), sq(3, 70, 5, 136, 3, 1, 1, 3);
  // ResNet-18 / CIFAR at B 128, S 1 and B 8, S 4
  for (int v = 0; v < 2; ++v) {
    const int B = v ? 8 : 128, S = v ? 4 : 1;
    sq(B, 3, 32, 64, 3, 1, 1, S);
    int c = 64, hw = 32;
    for (int co : {64, 128, 256, 512})
      for (int blk = 0; blk < 2; ++blk) {
        const int s = (co > 64 && blk == 0) ? 2 : 1;
        sq(B, c, hw, co, 3, s, 1, S);
        if (s == 2) sq(B, c, hw, co, 1, 2, 0, S);
        hw /= s, c = co;
        sq(B, co, hw, co, 3, 1, 1, S);
      }
    sq(B, 512, 1, 10, 1, 1, 0, S);
  }
  // groups, stride, dilation, rectangles; Cig, Cog and M around the planners' edges
  add(geom(4, 32, 8, 8, 64, 3, 3, 1, 1, 1, 1, 1, 1, 2), 2), add(geom(4, 32, 8, 8, 64, 3, 3, 2, 2, 1, 1, 1, 1, 4), 1), add(geom(4, 24, 9, 9, 40, 3, 3, 1, 1, 2, 2, 2, 2, 1), 2);
  add(geom(3, 20, 6, 11, 36, 1, 5, 1, 2, 0, 2, 1, 1, 1), 2), add(geom(3, 20, 11, 6, 36, 5, 2, 2, 1, 2, 0, 1, 2, 1), 1);
  for (int ci : {1, 3, 4, 5, 130}) sq(4, ci, 6, 40, 3, 1, 1, 2);
  for (int co : {16, 31, 32, 33, 64, 65, 136}) sq(2, 16, 4, co, 3, 1, 1, 1);
  for (int m : {1, 15, 16, 17, 127, 128, 129, 245, 1023, 1025}) add(geom(1, 16, 1, m, 24, 1, 1, 1, 1, 0, 0, 1, 1, 1), 1);
  // degenerate: every field 0, negative and at the ends of int, one at a time; S too
  const bt_conv2d_geom good = geom(2, 4, 6, 6, 8, 3, 3, 1, 1, 1, 1, 1, 1, 2);
  for (int f = 0; f < 14; ++f)
    for (int v : {0, -1, INT_MIN, INT_MAX, INT_MAX - 1, 1 << 30, 65536, 46341}) {
      bt_conv2d_geom g = good;
      reinterpret_cast<int*>(&g)[f] = v;
      for (int S : {1, 0, -1, INT_MIN, INT_MAX}) add(g, S);
    }
  static_assert(sizeof(bt_conv2d_geom) == 14 * sizeof(int), "bt_conv2d_geom is fourteen ints");
  // empty outputs
  add(geom(2, 4, 1, 1, 4, 3, 3, 1, 1, 0, 0, 1, 1, 1), 1), add(geom(2, 4, 5, 2, 4, 3, 3, 1, 1, 0, 0, 1, 1, 1), 1), add(geom(2, 4, 2, 5, 4, 3, 3, 1, 1, 0, 0, 2, 1, 1), 1);
  add(geom(1, 1, 1, 1, 1, INT_MAX, INT_MAX, 1, 1, 0, 0, INT_MAX, INT_MAX, 1), 1), add(geom(1, 1, INT_MAX, INT_MAX, 1, 1, 1, INT_MAX, INT_MAX, INT_MAX, INT_MAX, 1, 1, 1), 1);
  // the 2^31 limits: x, out and 4 * weights one step below, at and above them
  for (int d : {-1, 0, 1}) {
    add(geom(1, 2048 + d, 1024, 1024, 4, 1, 1, 1, 1, 0, 0, 1, 1, 1), 1);          // x_elems = 2^31 + d * 2^20
    add(geom(1, 4, 1024, 1024, 2048 + d, 1, 1, 1, 1, 0, 0, 1, 1, 1), 1);          // out_elems
    add(geom(1, 32768, 1, 1, 16384 + d, 1, 1, 1, 1, 0, 0, 1, 1, 1), 1);           // 4 * w_elems = 2^31 + d * 2^17
    add(geom(1, 1, 46341 + d, 46340, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), 1);           // a map of almost 2^31 pixels
    add(geom(1, 4096, 1, 1, 4096, 4 + d, 8, 1, 1, 2, 4, 1, 1, 1), 1);             // taps
    add(geom(INT_MAX / 2 + d, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), INT_MAX);   // every sample its own slice of the grid
    add(geom(1, 1 << 20, 1, 1, 1 << 20, 1, 1, 1, 1, 0, 0, 1, 1, 1 << 20), 2048 + d);   // S * groups around 2^31
  }
  add(geom(1, INT_MAX, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, INT_MAX), 1), add(geom(1, 1, 1, 1, INT_MAX, 1, 1, 1, 1, 0, 0, 1, 1, 1), 1);
  add(geom(1, 1, 3, 3, 1, 3, 3, INT_MAX, INT_MAX, INT_MAX, INT_MAX, 1, 1, 1), 1), add(geom(1, 1, 1, INT_MAX, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1), 1);
  const int targets[][2] = {{256, 512}, {128, 256}, {512, 1024}, {1, 1}, {INT_MAX, INT_MAX}};
  for (const auto& t : targets)
    for (const auto& c : cases)
      for (int pair = 1; pair >= 0; --pair) plan_case(c.first, c.second, t[0], t[1], pair != 0);
  printf("bwd_plan_check: %s (%d failed checks, %d plans, %d refusals)\n", failures ? "FAILED" : "ok", failures, plans, refusals);
  return failures ? 1 : 0;
}
