// C-ABI entry points of the four fused forwards: argument validation, geometry, launch.
#include <math.h>
#include <string.h>

#include "bt_fused_fwd.h"

namespace bt {
// The fp32 launchers by (Flipout, kind): on-chip draws, natural-layout injected draws, an input-dilated image (bt_*_conv2d_updil_fwd;
// on-chip draws), a depth-windowed input (bt_*_conv2d_dwin_fwd; on-chip draws). Each launches the layer and, on BT_OK, leaves the plan that ran (tile geometry, grid) in `ran`.
typedef int Launcher(bool linear, const FwdArgs& a, FwdArgs& ran, hipStream_t stream);
Launcher launch_reparam, launch_reparam_inj, launch_reparam_updil, launch_reparam_dwin, launch_flipout, launch_flipout_inj, launch_flipout_updil, launch_flipout_dwin;
static Launcher* const kLaunchers[2][4] = {{launch_reparam, launch_reparam_inj, launch_reparam_updil, launch_reparam_dwin},
                                           {launch_flipout, launch_flipout_inj, launch_flipout_updil, launch_flipout_dwin}};

EnvKnob g_force_generic{"BT_FORCE_GENERIC", [](const char* e) { return e ? 1 : 0; }};   // the fast flavour off: every fp32 launch takes the general kernel
static unsigned long long* g_dbg = nullptr;
static thread_local long long g_launch_info[16] = {};
static inline bool al16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
// tile geometry of the launch just made (bt_last_launch_info)
static void record_plan(const FwdArgs& r, int fused_kl) {
  const long long v[16] = {r.total_blocks, r.m_tiles, r.n_tiles, r.S, r.t_NI, r.t_R, r.t_Wt, r.pixel_major, r.row_taps, r.kl_slices, r.G, r.n_bt, r.n_rt, r.n_ct, fused_kl, 0};
  for (int i = 0; i < 16; ++i) g_launch_info[i] = v[i];
}

// One forward call as the C ABI hands it over. u: the input dilation and explicit padding of bt_*_conv2d_updil_fwd (g holds the REAL
// input dims), or null. w: the depth window of bt_*_conv2d_dwin_fwd (g describes the launch over the VIRTUAL, unfolded operand), or null.
struct Call {
  bool flip, linear;
  const bt_conv2d_geom& g;
  int S;
  const float* x;
  int64_t x_sample_stride;
  const bt_params* p;
  const bt_draws* d;
  const bt_epilogue* ep;
  float *out, *kl_out;
  void* ws;
  size_t ws_bytes;
  const char* who;   // the entry point's name, for its messages
  const bt_updil* u;
  const bt_dwin* w;
  // an input-dilated launch convolves the VIRTUAL image: the real one with u - 1 zeros between its pixels, padded by lo / hi
  long long virt_H() const { return u ? (long long)(g.H - 1) * u->uh + 1 + u->lo_h + u->hi_h : g.H; }
  long long virt_W() const { return u ? (long long)(g.W - 1) * u->uw + 1 + u->lo_w + u->hi_w : g.W; }
  int out_H() const { return (int)conv_out(virt_H(), g.kh, g.sh, g.ph, g.dh); }
  int out_W() const { return (int)conv_out(virt_W(), g.kw, g.sw, g.pw, g.dw); }
  bool updil() const { return u && (u->uh > 1 || u->uw > 1 || u->lo_h || u->hi_h || u->lo_w || u->hi_w); }   // (else: the plain convolution, launch for launch)
  bool dwin() const { return w && !(w->kd == 1 && w->D == 1 && w->pd == 0); }   // (else: the plain convolution, launch for launch)
  long long out_D() const { return conv_out(w->D, w->kd, w->sd, w->pd, w->dd); }
  long long real_x_elems() const { return dwin() ? (long long)(g.B / out_D()) * (g.Ci / w->kd) * w->D * g.H * g.W : (long long)g.B * g.Ci * g.H * g.W; }
  bool packed_eps() const { return (d->rng.flags & BT_DRAWS_EPS_PACKED) != 0; }
  bool pooled() const { return ep && ep->pool != BT_POOL_NONE; }

  // Every refusal of a call, in a fixed order: BT_OK, or what set_error made.
  int validate() const {
    char msg[256];
    auto bad = [&](const char* what) {
      snprintf(msg, sizeof(msg), "%s: %s", who, what);
      return set_error(BT_ERR_BAD_ARG, msg);
    };
    auto too_large = [] { return set_error(BT_ERR_UNSUPPORTED, "fused forward: a tensor of 2^30 elements or more exceeds the kernel's 32-bit offsets"); };
    if (!x || !p || !d || !out) return bad("null argument");
    if (!p->mu_w || !p->rho_w) return bad("mu_w / rho_w are required");
    if ((p->mu_b == nullptr) != (p->rho_b == nullptr)) return bad("mu_b and rho_b must both be given or both be NULL");
    if (S <= 0) return bad("S must be >= 1");
    if (const char* e = geom_error(g)) return bad(e);
    if (x_sample_stride < 0) return bad("negative x_sample_stride");
    if (u) {
      if (u->uh < 1 || u->uw < 1) return bad("input dilation must be >= 1");
      if (u->lo_h < 0 || u->hi_h < 0 || u->lo_w < 0 || u->hi_w < 0) return bad("negative explicit padding (a crop: materialise the input instead)");
      if (g.ph != 0 || g.pw != 0) return bad("ph / pw must be 0: the padding of the dilated image is explicit (lo / hi)");
    }
    if (w) {
      if (w->kd < 1 || w->D < 1 || w->sd < 1 || w->dd < 1) return bad("depth taps, depth, depth stride and depth dilation must be >= 1");
      if (w->pd < 0) return bad("negative depth padding");
      const long long num = (long long)w->D + 2ll * w->pd - (long long)w->dd * (w->kd - 1) - 1;
      if (num < 0 || out_D() < 1) return bad("empty output depth");
      if (out_D() >= (1ll << 30) || g.B % out_D()) return bad("g->B is not a multiple of the output depth (B * Do launch images)");
      if ((g.Ci / g.groups) % w->kd) return bad("g->Ci / groups is not a multiple of kd (Ci * kd launch channels)");
      if ((long long)g.B * g.Ci * g.H * g.W >= (1ll << 30) || (long long)(g.B / out_D()) * (g.Ci / w->kd) * w->D * g.H * g.W >= (1ll << 30))
        return bad("a real or unfolded x of 2^30 elements or more exceeds the kernel's 32-bit offsets");
    }
    if (kl_out) {
      if (!p->prior_mu_w || !p->prior_sigma_w) return bad("kl_out given but weight priors are NULL");
      if (p->mu_b && (!p->prior_mu_b || !p->prior_sigma_b)) return bad("kl_out given but bias priors are NULL");
      if (!ws || ws_bytes < BT_WORKSPACE_BYTES) {
        snprintf(msg, sizeof(msg), "%s: workspace smaller than BT_WORKSPACE_BYTES", who);
        return set_error(BT_ERR_WORKSPACE, msg);
      }
    }
    if (p->mu_b == nullptr && d->eps_b) return bad("eps_b given for a layer without bias");
    if (!flip && (d->sign_in || d->sign_out)) return bad("sign tensors are Flipout-only");
    if (ep && ((ep->scale == nullptr) != (ep->shift == nullptr))) return bad("epilogue scale and shift must both be given or both be NULL");
    if (ep && ep->residual_sample_stride < 0) return bad("negative residual_sample_stride");
    // packed draws (bt_pack_eps, bt_pack_signs): the split-precision kernels' injected instantiations, or nothing
    if (d->rng.flags & ~(BT_DRAWS_EPS_PACKED | BT_DRAWS_SIGNS_PACKED)) return bad("unknown bt_rng.flags bit");
    const bool eps_packed = packed_eps(), signs_packed = (d->rng.flags & BT_DRAWS_SIGNS_PACKED) != 0;
    if (signs_packed && (!eps_packed || !flip)) return bad("bt_rng.flags: BT_DRAWS_SIGNS_PACKED goes with BT_DRAWS_EPS_PACKED, on a Flipout entry point");
    if (eps_packed) {
      auto unsupported = [&](const char* what) {
        snprintf(msg, sizeof(msg), "%s: BT_DRAWS_EPS_PACKED: %s", who, what);
        return set_error(BT_ERR_UNSUPPORTED, msg);
      };
      if (!d->eps_w) return bad("BT_DRAWS_EPS_PACKED without eps_w");
      if (!signs_packed && (flip || d->sign_in || d->sign_out))
        return unsupported("Flipout needs its sign tensors packed too (bt_pack_signs, BT_DRAWS_SIGNS_PACKED), or inject the natural layout");
      if (signs_packed && (!d->sign_in || !d->sign_out)) return bad("BT_DRAWS_SIGNS_PACKED without sign_in / sign_out");
      if (!p->mu_packed || !p->sigma_packed) return bad("BT_DRAWS_EPS_PACKED needs mu_packed / sigma_packed");
      if (!al16(d->eps_w)) return bad("BT_DRAWS_EPS_PACKED: eps_w must be 16-byte aligned");
      if (signs_packed && (!al16(d->sign_in) || !al16(d->sign_out))) return bad("BT_DRAWS_SIGNS_PACKED: sign_in / sign_out must be 16-byte aligned");
      if (contraction_mode() != 0) return unsupported("the contraction is forced to f32 / bf16x2 / bf16 (bt_set_contraction, BT_CONTRACTION): only the exact split reads packed draws");
    }
    const long long Hv = virt_H(), Wv = virt_W();
    if (Hv >= (1ll << 30) || Wv >= (1ll << 30) || Hv * Wv >= (1ll << 30))
      return set_error(BT_ERR_UNSUPPORTED, "fused forward: a dilated image of 2^30 pixels or more exceeds the kernel's 32-bit offsets");
    const int Ho = out_H(), Wo = out_W();
    if (Ho <= 0 || Wo <= 0) return bad("empty output");
    if (updil()) {   // nothing is launched for what the dilated fetch does not cover
      if (d->eps_w || d->eps_b || d->sign_in || d->sign_out || eps_packed)
        return set_error(BT_ERR_UNSUPPORTED, "input-dilated launch: on-chip draws only (supplied draws take the materialised input)");
      if (pooled()) return set_error(BT_ERR_UNSUPPORTED, "input-dilated launch: no fused max-pool");
    }
    if (dwin()) {   // nothing is launched for what the depth-window fetch does not cover
      auto unsupported = [&](const char* what) {
        snprintf(msg, sizeof(msg), "%s: %s", who, what);
        return set_error(BT_ERR_UNSUPPORTED, msg);
      };
      if (d->eps_w || d->eps_b || d->sign_in || d->sign_out || eps_packed) return unsupported("on-chip draws only (supplied draws take the unfolded input)");
      if (pooled()) return unsupported("no fused max-pool on a depth-window launch");
    }
    if ((p->mu_packed == nullptr) != (p->sigma_packed == nullptr)) return bad("mu_packed and sigma_packed must both be given or both be NULL");
    // 32-bit index budget of the kernel (tile indices, hashed sign indices, Philox block index)
    const long long M = (long long)g.B * Ho * Wo, K = (long long)(g.Ci / g.groups) * g.kh * g.kw;
    if ((long long)g.B * g.Ci * Hv * Wv >= (1ll << 30)) return too_large();
    if (M >= (1ll << 30) || K >= (1ll << 30) || (long long)g.B * g.Ci * g.H * g.W >= (1ll << 30) || M * g.Co >= (1ll << 30) || (long long)g.Co * K >= (1ll << 30))
      return too_large();
    if (g.kh * g.kw > kMaxTaps) return set_error(BT_ERR_UNSUPPORTED, "fused forward: kernels larger than 128 taps are not supported");
    if (p->prior_kind != BT_PRIOR_NORMAL && p->prior_kind != BT_PRIOR_LAPLACE) return bad("unknown prior_kind");
    if (pooled()) {
      if (ep->pool != BT_POOL_MAX_3x3_S2_P1) return bad("unknown epilogue pool mode");
      if (linear) return bad("the fused max-pool belongs to the conv2d entry points");
      if (ep->residual) return bad("the fused max-pool takes no residual");
    }
    // draws are either all injected or all generated on chip (one compile-time flavour each)
    const bool all_inj = d->eps_w && (!p->mu_b || d->eps_b) && (!flip || (d->sign_in && d->sign_out));
    const bool none_inj = !d->eps_w && !d->eps_b && !d->sign_in && !d->sign_out;
    if (!all_inj && !none_inj) return bad("inject all draws of the layer (eps_w, eps_b when biased, both sign tensors for Flipout) or none");
    if (d->eps_w && pooled() && !eps_packed) return set_error(BT_ERR_UNSUPPORTED, "fused max-pool: not available with injected draws");
    return BT_OK;
  }

  // The argument block of a validated call, before any plan: operands, geometry (the virtual image of an input-dilated launch), element
  // counts, alignment flags, epilogue, RNG coordinates. kl_after: a Laplace prior's KL follows the forward (run).
  void fill_args(bool kl_after, FwdArgs& a) const {
    const FwdArgs zero = {};
    a = zero;
    a.x = x, a.mu_w = p->mu_w, a.rho_w = p->rho_w, a.mu_b = p->mu_b, a.rho_b = p->rho_b;
    a.pmu_w = p->prior_mu_w, a.psig_w = p->prior_sigma_w, a.pmu_b = p->prior_mu_b, a.psig_b = p->prior_sigma_b;
    a.mu_pk = p->mu_packed, a.sig_pk = p->sigma_packed;
    a.eps_w = d->eps_w, a.eps_b = d->eps_b, a.sign_in = d->sign_in, a.sign_out = d->sign_out;
    a.out = out, a.kl_out = kl_after ? nullptr : kl_out;
    a.slots = kl_out ? ws_slots(ws) : nullptr;
    a.counter = kl_out ? ws_counter(ws) : nullptr;
    // a workspace larger than BT_WORKSPACE_BYTES carries scratch for the split-K (skinny) flavour behind its zeroed head
    if (ws && ws_bytes > BT_WORKSPACE_BYTES) {
      a.sk_scratch = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + BT_WORKSPACE_BYTES);
      a.sk_scratch_bytes = (long long)(ws_bytes - BT_WORKSPACE_BYTES);
      a.sk_tickets = reinterpret_cast<unsigned*>(ws_slots(ws) + 4000);
    }
    const long long Hv = virt_H(), Wv = virt_W();
    const int Ho = out_H(), Wo = out_W();
    a.B = g.B, a.Ci = g.Ci, a.H = (int)Hv, a.W = (int)Wv, a.Co = g.Co, a.KH = g.kh, a.KW = g.kw;
    if (updil()) a.updil = 1, a.UH = u->uh, a.UW = u->uw, a.LH = u->lo_h, a.LW = u->lo_w, a.Hr = g.H, a.Wr = g.W, a.HWr = g.H * g.W;
    a.SH = g.sh, a.SW = g.sw, a.PH = g.ph, a.PW = g.pw, a.DH = g.dh, a.DW = g.dw, a.G = g.groups;
    a.Ho = Ho, a.Wo = Wo, a.HoWo = Ho * Wo;
    const long long M = (long long)g.B * Ho * Wo;
    a.Cig = g.Ci / g.groups, a.Cog = g.Co / g.groups;
    const long long K = (long long)a.Cig * g.kh * g.kw;
    a.x_elems = real_x_elems();   // (the REAL elements of an input-dilated / depth-window launch: what x holds and what the input signs index)
    if (dwin()) a.dwin = 1, a.KD = w->kd, a.D = w->D, a.Do = (int)out_D(), a.SD = w->sd, a.DD = w->dd, a.PD = w->pd, a.Cigr = a.Cig / w->kd;
    a.out_elems = M * g.Co;
    a.w_elems = (long long)g.Co * K;
    a.M = (int)M, a.K = (int)K, a.S = S;
    a.T = g.kh * g.kw, a.HW = (int)(Hv * Wv);
    // pixel-major tiles prune padding taps per output pixel; worth it when images are tiny (2x2 outputs: 4 of 9 taps)
    a.pixel_major = (!linear && a.HoWo >= 2 && a.HoWo <= 4 && (g.ph > 0 || g.pw > 0)) ? 1 : 0;
    a.x_sample_stride = x_sample_stride;
    a.w_vec = linear && ((K & 3) == 0) && al16(p->mu_w) && al16(p->rho_w) && (!d->eps_w || al16(d->eps_w));
    a.x_vec = linear && ((K & 3) == 0) && al16(x) && ((x_sample_stride & 3) == 0) && (!d->sign_in || al16(d->sign_in));
    a.do_kl = kl_out != nullptr && !kl_after;
    a.seed_lo = (uint32_t)d->rng.seed, a.seed_hi = (uint32_t)(d->rng.seed >> 32);
    if (ep) a.ep_scale = ep->scale, a.ep_shift = ep->shift, a.ep_res = ep->residual, a.ep_res_stride = ep->residual_sample_stride, a.ep_relu = ep->relu;
    if (pooled()) {
      a.ep_pool = 1, a.ep_Hp = (Ho - 1) / 2 + 1, a.ep_Wp = (Wo - 1) / 2 + 1;
      a.out_elems = (long long)g.B * g.Co * a.ep_Hp * a.ep_Wp;
    }
    a.out_vec4 = (!linear && !a.pixel_major && a.HoWo > 1 && (a.Wo & 3) == 0 && al16(out) && (!a.ep_res || (al16(a.ep_res) && (a.ep_res_stride & 3) == 0)) &&
                  (!d->sign_out || al16(d->sign_out))) ? 1 : 0;
    a.dbg = g_dbg;
    a.call = d->rng.call, a.call_base = d->rng.call_base_dev, a.layer_id = d->rng.layer_id, a.sample0 = d->rng.sample0;
  }

  // Packed draws: the split chain alone (it launches nothing when it declines). Else the fp32 launcher of the call's kind; those with
  // on-chip draws try the split chain first themselves.
  int dispatch(const FwdArgs& a, FwdArgs& ran, hipStream_t stream) const {
    if (!packed_eps()) return kLaunchers[flip][dwin() ? 3 : updil() ? 2 : d->eps_w ? 1 : 0](linear, a, ran, stream);
    const int rc = flip ? launch_split_flip(a, ran, stream) : launch_split(a, ran, stream);
    if (rc != 1) return rc;
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: BT_DRAWS_EPS_PACKED: no split-precision flavour takes this launch (inject the natural layout)", who);
    return set_error(BT_ERR_UNSUPPORTED, msg);
  }
};

static int run(const Call& c, bt_stream_t stream) {
  if (int rc = c.validate()) return rc;
  // The fused KL sweep is the Gaussian closed form. A Laplace-prior layer gets its KL from the standalone kernel, enqueued
  // right behind the forward on the same stream (same result slot, same workspace).
  const bool kl_after = c.kl_out && c.p->prior_kind == BT_PRIOR_LAPLACE;
  FwdArgs a, r;   // r: the plan that ran
  c.fill_args(kl_after, a);
  int rc = c.dispatch(a, r, (hipStream_t)stream);
  if (rc != BT_OK) return rc;
  record_plan(r, r.do_kl);
  if (kl_after) {
    const bt_params* p = c.p;
    const float* mu[2] = {p->mu_w, p->mu_b};
    const float* rho[2] = {p->rho_w, p->rho_b};
    const float* pm[2] = {p->prior_mu_w, p->prior_mu_b};
    const float* ps[2] = {p->prior_sigma_w, p->prior_sigma_b};
    const int64_t n[2] = {a.w_elems, (int64_t)c.g.Co};
    const int32_t lay[2] = {0, 0};
    rc = bt_kl_normal(p->mu_b ? 2 : 1, mu, rho, pm, ps, n, lay, BT_KL_PRIOR_LAPLACE, c.kl_out, c.ws, c.ws_bytes, stream);
  }
  return rc;
}

static bt_conv2d_geom linear_geom(int B, int In, int Out) {
  bt_conv2d_geom g;
  g.B = B, g.Ci = In, g.H = 1, g.W = 1, g.Co = Out, g.kh = 1, g.kw = 1;
  g.sh = g.sw = 1, g.ph = g.pw = 0, g.dh = g.dw = 1, g.groups = 1;
  return g;
}
}  // namespace bt

extern "C" int bt_reparam_linear_fwd(int32_t B, int32_t In, int32_t Out, int32_t S, const float* x, int64_t x_sample_stride,
                                     const bt_params* p, const bt_draws* d, const bt_epilogue* ep, float* out, float* kl_out, void* ws, size_t ws_bytes,
                                     bt_stream_t stream) {
  return bt::run({false, true, bt::linear_geom(B, In, Out), S, x, x_sample_stride, p, d, ep, out, kl_out, ws, ws_bytes, "bt_reparam_linear_fwd", nullptr, nullptr}, stream);
}
extern "C" int bt_flipout_linear_fwd(int32_t B, int32_t In, int32_t Out, int32_t S, const float* x, int64_t x_sample_stride,
                                     const bt_params* p, const bt_draws* d, const bt_epilogue* ep, float* out, float* kl_out, void* ws, size_t ws_bytes,
                                     bt_stream_t stream) {
  return bt::run({true, true, bt::linear_geom(B, In, Out), S, x, x_sample_stride, p, d, ep, out, kl_out, ws, ws_bytes, "bt_flipout_linear_fwd", nullptr, nullptr}, stream);
}
extern "C" int bt_reparam_conv2d_fwd(const bt_conv2d_geom* g, int32_t S, const float* x, int64_t x_sample_stride, const bt_params* p,
                                     const bt_draws* d, const bt_epilogue* ep, float* out, float* kl_out, void* ws, size_t ws_bytes, bt_stream_t stream) {
  if (!g) return bt::set_error(BT_ERR_BAD_ARG, "bt_reparam_conv2d_fwd: null geometry");
  return bt::run({false, false, *g, S, x, x_sample_stride, p, d, ep, out, kl_out, ws, ws_bytes, "bt_reparam_conv2d_fwd", nullptr, nullptr}, stream);
}
extern "C" int bt_flipout_conv2d_fwd(const bt_conv2d_geom* g, int32_t S, const float* x, int64_t x_sample_stride, const bt_params* p,
                                     const bt_draws* d, const bt_epilogue* ep, float* out, float* kl_out, void* ws, size_t ws_bytes, bt_stream_t stream) {
  if (!g) return bt::set_error(BT_ERR_BAD_ARG, "bt_flipout_conv2d_fwd: null geometry");
  return bt::run({true, false, *g, S, x, x_sample_stride, p, d, ep, out, kl_out, ws, ws_bytes, "bt_flipout_conv2d_fwd", nullptr, nullptr}, stream);
}

extern "C" int bt_reparam_conv2d_chain_fwd(int32_t n, const bt_chain_member* m, int32_t S, bt_stream_t stream) {
  using namespace bt;
  const char* who = "bt_reparam_conv2d_chain_fwd";
  if (!m || n < 1) return set_error(BT_ERR_BAD_ARG, "bt_reparam_conv2d_chain_fwd: no members");
  if (n > BT_CHAIN_MAX) return BT_CHAIN_DECLINED;
  FwdArgs a[BT_CHAIN_MAX], r;
  for (int k = 0; k < n; ++k) {
    if (!m[k].g) return set_error(BT_ERR_BAD_ARG, "bt_reparam_conv2d_chain_fwd: null geometry");
    if (m[k].kl_out) return BT_CHAIN_DECLINED;   // (a KL sweep takes a workspace: the member's own call)
    const Call c{false, false, *m[k].g, S, m[k].x, m[k].x_sample_stride, m[k].p, m[k].d, m[k].ep, m[k].out, nullptr, nullptr, 0, who, nullptr, nullptr};
    if (int rc = c.validate()) return rc;
    if (c.packed_eps()) return BT_CHAIN_DECLINED;
    c.fill_args(false, a[k]);
  }
  const int rc = launch_split_chain(n, a, r, (hipStream_t)stream);
  if (rc != BT_OK) return rc == 1 ? BT_CHAIN_DECLINED : rc;
  record_plan(r, 0);
  return BT_OK;
}

extern "C" int bt_reparam_conv2d_updil_fwd(const bt_conv2d_geom* g, const bt_updil* u, int32_t S, const float* x, int64_t x_sample_stride, const bt_params* p,
                                           const bt_draws* d, const bt_epilogue* ep, float* out, float* kl_out, void* ws, size_t ws_bytes, bt_stream_t stream) {
  if (!g || !u) return bt::set_error(BT_ERR_BAD_ARG, "bt_reparam_conv2d_updil_fwd: null geometry");
  return bt::run({false, false, *g, S, x, x_sample_stride, p, d, ep, out, kl_out, ws, ws_bytes, "bt_reparam_conv2d_updil_fwd", u, nullptr}, stream);
}
extern "C" int bt_flipout_conv2d_updil_fwd(const bt_conv2d_geom* g, const bt_updil* u, int32_t S, const float* x, int64_t x_sample_stride, const bt_params* p,
                                           const bt_draws* d, const bt_epilogue* ep, float* out, float* kl_out, void* ws, size_t ws_bytes, bt_stream_t stream) {
  if (!g || !u) return bt::set_error(BT_ERR_BAD_ARG, "bt_flipout_conv2d_updil_fwd: null geometry");
  return bt::run({true, false, *g, S, x, x_sample_stride, p, d, ep, out, kl_out, ws, ws_bytes, "bt_flipout_conv2d_updil_fwd", u, nullptr}, stream);
}

extern "C" int bt_reparam_conv2d_dwin_fwd(const bt_conv2d_geom* g, const bt_dwin* w, int32_t S, const float* x, int64_t x_sample_stride, const bt_params* p,
                                          const bt_draws* d, const bt_epilogue* ep, float* out, float* kl_out, void* ws, size_t ws_bytes, bt_stream_t stream) {
  if (!g || !w) return bt::set_error(BT_ERR_BAD_ARG, "bt_reparam_conv2d_dwin_fwd: null geometry");
  return bt::run({false, false, *g, S, x, x_sample_stride, p, d, ep, out, kl_out, ws, ws_bytes, "bt_reparam_conv2d_dwin_fwd", nullptr, w}, stream);
}
extern "C" int bt_flipout_conv2d_dwin_fwd(const bt_conv2d_geom* g, const bt_dwin* w, int32_t S, const float* x, int64_t x_sample_stride, const bt_params* p,
                                          const bt_draws* d, const bt_epilogue* ep, float* out, float* kl_out, void* ws, size_t ws_bytes, bt_stream_t stream) {
  if (!g || !w) return bt::set_error(BT_ERR_BAD_ARG, "bt_flipout_conv2d_dwin_fwd: null geometry");
  return bt::run({true, false, *g, S, x, x_sample_stride, p, d, ep, out, kl_out, ws, ws_bytes, "bt_flipout_conv2d_dwin_fwd", nullptr, w}, stream);
}

namespace bt {
int launch_lowrank(const FwdArgs& a, FwdArgs& ran, hipStream_t stream);   // bt_fused_lowrank.hip
}

extern "C" int bt_lowrank_conv2d_fwd(const bt_conv2d_geom* g, int32_t S, const float* x, int64_t x_sample_stride, const float* mean, int64_t mean_stride,
                                     const float* L, int32_t R, float d, const float* z, const float* eps_w, const bt_rng* rng, const bt_epilogue* ep,
                                     float* out, bt_stream_t stream) {
  using namespace bt;
  const char* who = "bt_lowrank_conv2d_fwd";
  char msg[256];
  auto bad = [&](const char* what) {
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return set_error(BT_ERR_BAD_ARG, msg);
  };
  if (!g) return bad("null geometry");
  if (!mean || !rng) return bad("null argument");
  if (R < 0 || R > BT_LOWRANK_MAX_R) return bad("R must be in [0, BT_LOWRANK_MAX_R]");
  if (R > 0 && !L) return bad("R > 0 needs L");
  if (!(d > 0.f)) return bad("d must be > 0");
  if (mean_stride < 0) return bad("negative mean_stride");
  if (g->groups != 1) return bad("groups must be 1");
  if ((eps_w && R > 0 && !z) || (!eps_w && z)) return bad("supply both draws (z, eps_w) or neither");
  if (ep && (ep->pool != BT_POOL_NONE || ep->residual || ep->relu || ep->scale || ep->shift))
    return set_error(BT_ERR_UNSUPPORTED, "bt_lowrank_conv2d_fwd: no fused output stage (max-pool, residual, ReLU, scale / shift)");
  // the mean-field call's checks of the geometry and the 32-bit offsets, on a parameter block whose (mu, rho) is the mean
  bt_params p;
  memset(&p, 0, sizeof(p));
  p.mu_w = mean, p.rho_w = mean, p.prior_kind = BT_PRIOR_NORMAL;
  bt_draws dr;
  memset(&dr, 0, sizeof(dr));
  dr.eps_w = eps_w, dr.rng = *rng;
  dr.rng.flags = 0;
  const Call c{false, false, *g, S, x, x_sample_stride, &p, &dr, nullptr, out, nullptr, nullptr, 0, who, nullptr, nullptr};
  if (int rc = c.validate()) return rc;
  FwdArgs a, r;
  c.fill_args(false, a);
  if (a.w_elems * (R > 0 ? R : 1) >= (1ll << 30) || (long long)(S - 1) * mean_stride + a.w_elems >= (1ll << 40))
    return set_error(BT_ERR_UNSUPPORTED, "bt_lowrank_conv2d_fwd: L of 2^30 elements or more exceeds the kernel's 32-bit offsets");
  a.lowrank = 1, a.lr_R = R, a.lr_L = R > 0 ? L : mean, a.lr_z = (eps_w && R > 0) ? z : nullptr, a.lr_mean_stride = mean_stride, a.lr_sd = sqrtf(d);
  const int rc = launch_lowrank(a, r, (hipStream_t)stream);
  if (rc != BT_OK) return rc;
  record_plan(r, 0);
  return BT_OK;
}

// The observing two-contraction launch of a calibrating Flipout layer (include/bt_hip.h; bt_fused_flipout_obs.hip): the float Flipout
// call's checks of operands, draws, geometry and 32-bit offsets, then the general kernel's OBS form.
namespace bt {
int launch_flipout_obs(bool linear, const FwdArgs& a, FwdArgs& ran, hipStream_t stream);   // bt_fused_flipout_obs.hip

static int observe_flip(const char* who, bool linear, const bt_conv2d_geom& g, int32_t S, const float* x, int64_t x_sample_stride, const bt_params* p, const bt_draws* d,
                        const float* coef, const float* shift, float* mean_mm, float* pert_mm, float* pert_signed_mm, float* sign_out_mm, uint32_t* nonfinite,
                        bt_stream_t stream) {
  char msg[256];
  auto fail = [&](int code, const char* what) {
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return set_error(code, msg);
  };
  if (!mean_mm || !pert_mm || !pert_signed_mm || !sign_out_mm || !nonfinite) return fail(BT_ERR_BAD_ARG, "null statistics / nonfinite");
  uintptr_t bits = (uintptr_t)x | (uintptr_t)coef | (uintptr_t)shift | (uintptr_t)mean_mm | (uintptr_t)pert_mm | (uintptr_t)pert_signed_mm | (uintptr_t)sign_out_mm | (uintptr_t)nonfinite;
  if (p) bits |= (uintptr_t)p->mu_w | (uintptr_t)p->rho_w | (uintptr_t)p->mu_b | (uintptr_t)p->rho_b;
  if (d) bits |= (uintptr_t)d->eps_w | (uintptr_t)d->eps_b | (uintptr_t)d->sign_in | (uintptr_t)d->sign_out;
  if (bits & 3u) return fail(BT_ERR_BAD_ARG, "a pointer that is not 4-byte aligned");
  if (d && d->rng.flags) return fail(BT_ERR_BAD_ARG, "supplied draws in the natural layouts only (bt_rng.flags must be 0)");
  bt_params pp;
  if (p) pp = *p, pp.mu_packed = pp.sigma_packed = nullptr, pp.prior_kind = BT_PRIOR_NORMAL;   // (the general kernel reads the natural layout)
  bt_epilogue ep;
  memset(&ep, 0, sizeof(ep));
  ep.scale = coef, ep.shift = shift;
  const Call c{true, linear, g, S, x, x_sample_stride, p ? &pp : nullptr, d, &ep, mean_mm, nullptr, nullptr, 0, who, nullptr, nullptr};
  if (int rc = c.validate()) return rc;
  if (g.groups != 1) return fail(BT_ERR_UNSUPPORTED, "groups must be 1 (the INT8 Flipout layers')");
  if (S > 65535) return fail(BT_ERR_UNSUPPORTED, "S > 65535");
  FwdArgs a, r;
  c.fill_args(false, a);
  a.out = nullptr, a.out_vec4 = 0;   // nothing is stored
  a.obs_dst[0] = mean_mm, a.obs_dst[1] = pert_mm, a.obs_dst[2] = pert_signed_mm, a.obs_dst[3] = sign_out_mm, a.obs_nonfinite = nonfinite;
  if (int rc = launch_flipout_obs(linear, a, r, (hipStream_t)stream)) return rc;
  record_plan(r, 0);
  return BT_OK;
}
}  // namespace bt

extern "C" int bt_q8_flip_observe_conv2d(const bt_conv2d_geom* g, int32_t S, const float* x, int64_t x_sample_stride, const bt_params* p, const bt_draws* d,
                                         const float* coef, const float* shift, float* mean_mm, float* pert_mm, float* pert_signed_mm, float* sign_out_mm,
                                         uint32_t* nonfinite, bt_stream_t stream) {
  if (!g) return bt::set_error(BT_ERR_BAD_ARG, "bt_q8_flip_observe_conv2d: null geometry");
  return bt::observe_flip("bt_q8_flip_observe_conv2d", false, *g, S, x, x_sample_stride, p, d, coef, shift, mean_mm, pert_mm, pert_signed_mm, sign_out_mm, nonfinite, stream);
}
extern "C" int bt_q8_flip_observe_linear(int32_t B, int32_t In, int32_t Out, int32_t S, const float* x, int64_t x_sample_stride, const bt_params* p, const bt_draws* d,
                                         const float* coef, const float* shift, float* mean_mm, float* pert_mm, float* pert_signed_mm, float* sign_out_mm,
                                         uint32_t* nonfinite, bt_stream_t stream) {
  return bt::observe_flip("bt_q8_flip_observe_linear", true, bt::linear_geom(B, In, Out), S, x, x_sample_stride, p, d, coef, shift, mean_mm, pert_mm, pert_signed_mm,
                          sign_out_mm, nonfinite, stream);
}

extern "C" size_t bt_fused_scratch_bytes(const bt_conv2d_geom* g, int32_t S) {
  if (!g || S <= 0) return 0;
  const long long n = bt::skinny_scratch_bytes(*g, S);
  return n > 0 ? (size_t)n : 0;
}

extern "C" int bt_last_launch_info(int64_t* out, int32_t n) {
  if (!out || n <= 0) return bt::set_error(BT_ERR_BAD_ARG, "bt_last_launch_info: bad argument");
  for (int i = 0; i < n; ++i) out[i] = i < 16 ? (int64_t)bt::g_launch_info[i] : 0;
  return BT_OK;
}

// Diagnostic hook (not part of include/bt_hip.h): device buffer of >= 256 u64 that block 0 of every fused launch
// fills with s_memtime stamps per stage (consumer wave 0: [2+2st, 3+2st]; producer wave 4: [128+2st, 129+2st]).
extern "C" void bt_debug_set_stamp_buffer(void* p) { bt::g_dbg = (unsigned long long*)p; }
extern "C" void bt_debug_force_generic(int on) { bt::g_force_generic.set(on ? 1 : 0); }
