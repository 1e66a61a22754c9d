// What every fused forward kernel computes the same way, once: the argument block, the draw-stream keys, the bias draw and the
// output-stage constants of a channel, the KL sweep of a workgroup's slice and its close by the last arriver, the tile-column decode.
// These are not tuning surfaces: they define what a layer computes, and the flavours' bit-identity (tests/test_gpu_family_parity.py,
// test_gpu_round3.py) follows from their having one definition. What differs per kernel -- WHEN a KL group is consumed, how the
// partials are published, where the constants are kept -- stays in the kernels.
#pragma once
#include "bt_api_internal.h"

namespace bt {

struct FwdArgs {
  const float *x, *mu_w, *rho_w, *mu_b, *rho_b, *pmu_w, *psig_w, *pmu_b, *psig_b;
  const float *mu_pk, *sig_pk;  // optional tap-major packed parameters (bt_params.mu_packed / sigma_packed): fast flavour only
  const float *eps_w, *eps_b, *sign_in, *sign_out;
  float* out;
  float* kl_out;
  double* slots;
  unsigned* counter;
  long long x_sample_stride, x_elems, out_elems, w_elems;
  int B, Ci, H, W, Co, KH, KW, SH, SW, PH, PW, DH, DW, G;
  int Ho, Wo, HoWo, M, K, Cig, Cog, S, T, HW;
  int n_tiles, m_tiles, total_blocks;
  int t_NI, t_R, t_Wt, n_bt, n_rt, n_ct;  // fast flavour: tile = t_NI images x t_R rows x t_Wt cols; tile grid per (n-tile, sample)
  int patch_ok;                   // host: tiles are whole images (or pixel-major), so the x operand can be staged as a patch
  int x_cvec;                     // host (fast flavour): x is 16-byte aligned per image -> tiny planes are staged as channel vectors
  int x_rows;                     // host (fast flavour): stage the x patch as 16-byte row chunks written straight to LDS
  int pixel_major, mt_per_pixel;  // m-tile = (one output pixel, BM images) instead of BM consecutive (b, ho, wo)
  int w_vec, x_vec;               // float4 paths allowed (taps == 1, K % 4 == 0, 16-B aligned bases)
  int do_kl, kl_slices;
  uint32_t seed_lo, seed_hi, call, layer_id, sample0;
  const uint32_t* call_base;  // device word added to `call` (fresh draws on graph replay), or null
  const float *ep_scale, *ep_shift, *ep_res;  // fused output stage (bt_epilogue)
  long long ep_res_stride;
  int ep_relu;
  int ep_pool, ep_Hp, ep_Wp;  // fused 3x3 / stride 2 / pad 1 max-pool of the output stage (fast flavour, whole-image tiles)
  int out_vec4;  // spatial output stored as float4 along the pixel index (TRANS orientation; Ho*Wo % 4 == 0, aligned tensors)
  int bn32;                 // general split kernel: 32-channel tiles (split_plan)
  unsigned long long* dbg;  // diagnostic stamps (bt_debug_set_stamp_buffer); null in normal operation
  // split flavour: ceil(2^32 / d) of the launch-uniform divisors (0: divide), so the tile decode is a few multiplies
  uint32_t inv_m_tiles, inv_S, inv_n_tiles, inv_n_bt, inv_n_ct, inv_rw, inv_wt, inv_kw;
  int x_flat;  // split flavour, XM 3: the patch is the whole input plane -- fetch it as one row of H*W pixels
  int row_taps;  // split flavour: tiles = t_NI images x ONE output row; the active taps are those of the tile's row (2-row maps)
  // skinny flavour (bt_fused_split_skinny.h): scratch slabs behind the workspace, tickets inside it, slice geometry
  float* sk_scratch;
  unsigned* sk_tickets;
  long long sk_scratch_bytes;
  int sk_nsl, sk_ks, sk_cpt;           // slices per tile, slice width (channels), slices per tap
  int sk_kh0, sk_nh, sk_kw0, sk_nw;    // the rectangle of taps whose input pixel exists for the one output pixel
  int d_tap;     // direct flavour: the ONE tap of the kernel window that meets data (0 for 1x1 kernels; the centre of a padded window over a 1x1 image)
  int spw, n_sg;        // quad flavour, sample walk: samples per workgroup, sample groups = ceil(S / spw) (launch_quad)
  uint32_t inv_n_sg;
  // input-dilated launches (bt_*_conv2d_updil_fwd: the transposed convolutions without the upsampled copy). H, W, HW above are the
  // VIRTUAL image's -- planner, tile geometry, tap pruning and draw streams are those of the launch over the materialised tensor --
  // and x is [B][Ci][Hr][Wr]: virtual pixel (y, x) is the real element ((y - LH) / UH, (x - LW) / UW) where both divide and the
  // quotients are inside the real image, else a zero of the dilation or of the explicit padding. x_elems counts the REAL elements.
  int updil;
  int UH, UW, LH, LW, Hr, Wr, HWr;
  uint32_t inv_uh, inv_uw;   // ceil(2^32 / UH), ceil(2^32 / UW) (0: divide), split_fill_inverses
  // depth-window launches (bt_*_conv2d_dwin_fwd: Conv3d without the depth-unfolded copy). B, Ci, Cig, K above are the VIRTUAL operand's
  // -- B = real batch x Do images, Ci = real channels x KD -- and x is the real [B / Do][Ci / KD][D][H][W]: launch image b' = b * Do + dz,
  // launch channel c' = ci * KD + j reads depth plane z = dz * SD - PD + j * DD of real channel ci, a zero where z is outside [0, D).
  // x_elems counts the REAL elements. Cigr: real channels per group (Cig / KD).
  int dwin;
  int KD, D, Do, SD, DD, PD, Cigr;
  uint32_t inv_kd, inv_do;   // ceil(2^32 / KD), ceil(2^32 / Do) (0: divide), split_fill_inverses
  // low-rank weight source (bt_lowrank_conv2d_fwd, the kernel's LOWRANK form): w = mean + sum_{j < lr_R} L[i][j] * z_s[j] + lr_sd * eps.
  // mu_w above is the mean, read at mu_w + s * lr_mean_stride; lr_L is row-major [w_elems][lr_R] (never null: the mean when lr_R == 0);
  // lr_z is the supplied [S][lr_R] (the injected instantiation), else null: tensor 4 of the call's draw streams, Philox block 0.
  int lowrank;
  const float *lr_L, *lr_z;
  long long lr_mean_stride;
  float lr_sd;
  int lr_R;
  // observing launch (bt_q8_flip_observe_conv2d / _linear, the general Flipout kernel's OBS form): nothing is stored through `out`; the
  // ranges of mean, pert, pert_signed and sign_out (bt_hip.h) are merged into the four (min, max) pairs obs_dst[0..3] and the non-finite
  // values counted into *obs_nonfinite. All null on every other launch.
  float* obs_dst[4];
  unsigned* obs_nonfinite;
};

// Plan-only digest of the argument block: every field in declaration order, without the two padding holes (behind sample0, at the end).
// The depth-window fields behind inv_uw are folded in only when the launch is one, and the low-rank fields behind those likewise: every
// other launch hashes the bytes it always did. The observer fields behind those: only on an observing launch.
inline uint64_t digest_arg(uint64_t h, const FwdArgs& a) {
  constexpr size_t hole = offsetof(FwdArgs, sample0) + sizeof(uint32_t), end = offsetof(FwdArgs, inv_uw) + sizeof(uint32_t);
  constexpr size_t end_dw = offsetof(FwdArgs, inv_do) + sizeof(uint32_t);
  constexpr size_t end_lr = offsetof(FwdArgs, lr_R) + sizeof(int);
  constexpr size_t end_obs = offsetof(FwdArgs, obs_nonfinite) + sizeof(unsigned*);
  static_assert(offsetof(FwdArgs, call_base) == hole + 4 && offsetof(FwdArgs, dwin) == end && offsetof(FwdArgs, lowrank) == end_dw &&
                    offsetof(FwdArgs, obs_dst) == end_lr && sizeof(FwdArgs) == end_obs,
                "FwdArgs padding moved: name the holes here");
  h = fnv1a(h, &a, hole);
  h = fnv1a(h, &a.call_base, end - offsetof(FwdArgs, call_base));
  if (a.dwin) h = fnv1a(h, &a.dwin, end_dw - end);
  if (a.lowrank) h = fnv1a(h, &a.lowrank, end_lr - end_dw);
  return a.obs_nonfinite ? fnv1a(h, &a.obs_dst, end_obs - end_lr) : h;
}

// The split-precision chains (bt_fused_split.hip, bt_fused_split_flip.hip), for every translation unit that calls them. Each works on
// its own copy of the arguments: BT_OK and the plan that ran in `ran` when a flavour took the launch, 1 when none applies, < 0 on error.
int launch_split(FwdArgs a, FwdArgs& ran, hipStream_t stream);
int launch_split_flip(FwdArgs a, FwdArgs& ran, hipStream_t stream);
int launch_split_chain(int n, FwdArgs* m, FwdArgs& ran, hipStream_t stream);   // bt_fused_split_chain.hip: n same-shape layers as one launch, or 1
int contraction_mode();   // 0 automatic, 1 fp32 MFMA only, 2 bf16x2 (opt-in), 3 bf16 (opt-in)
long long skinny_scratch_bytes(const bt_conv2d_geom& g, int S);   // the split-K flavour's scratch behind the workspace (0: not its launch)

// ---------------------------------------------------------------------------- draw-stream keys
// The weight draws' key of this launch: (seed, call + the device-side call word, layer, tensor 0).
__device__ __forceinline__ RngKey weight_key(uint32_t seed_lo, uint32_t seed_hi, uint32_t call, const uint32_t* call_base, uint32_t layer_id) {
  RngKey key_w;
  key_w.seed_lo = seed_lo;
  key_w.seed_hi = seed_hi;
  key_w.call = call + (call_base ? __builtin_nontemporal_load(call_base) : 0u);
  key_w.layer_tensor = layer_tensor_word(layer_id, 0);
  return key_w;
}
__device__ __forceinline__ RngKey weight_key(const FwdArgs& a) { return weight_key(a.seed_lo, a.seed_hi, a.call, a.call_base, a.layer_id); }

// Flipout: the keys of the two sign streams (tensors 2 and 3) of one MC sample.
__device__ __forceinline__ void sign_keys(const FwdArgs& a, const RngKey& key_w, uint32_t sample, uint32_t* skey_in, uint32_t* skey_out) {
  RngKey ks = key_w;
  ks.layer_tensor = layer_tensor_word(a.layer_id, 2);
  *skey_in = sign_stream_key(ks, sample);
  ks.layer_tensor = layer_tensor_word(a.layer_id, 3);
  *skey_out = sign_stream_key(ks, sample);
}

// ---------------------------------------------------------------------------- bias draw + output-stage constants
// The on-chip bias draw of channel co (tensor 1): element co & 3 of Philox block co >> 2.
__device__ __forceinline__ float bias_eps(const RngKey& key_w, uint32_t layer_id, uint32_t sample, int co) {
  RngKey kb = key_w;
  kb.layer_tensor = layer_tensor_word(layer_id, 1);
  float z[4];
  philox_normal4(kb, sample, (uint32_t)(co >> 2), z);
  const int sel = co & 3;
  return sel == 0 ? z[0] : sel == 1 ? z[1] : sel == 2 ? z[2] : z[3];
}

// What the output stage needs per channel. Reparameterization: bias0 = mu_b + sigma_b * eps_b. Flipout: bias0 = mu_b and bias1 =
// sigma_b * eps_b (it joins the perturbation path). No bias / a channel past the group's: zeros; no folded scale / shift: 1 and 0.
struct ChannelConsts {
  float bias0, bias1, scale, shift;
};

// Channel co_g of group g for the launch's sample s (the index into a.eps_b when the draws are INJected, sample0 + s on chip).
// The layer's own operands of that computation (one launch: the launch's arguments; a chained launch: the member's, bt_fused_split.h).
struct ChannelSrc {
  const float *mu_b, *rho_b, *eps_b, *ep_scale, *ep_shift;
  uint32_t layer_id;
};
template <bool FLIP, bool INJ>
__device__ __forceinline__ ChannelConsts channel_consts(const FwdArgs& a, const ChannelSrc& l, const RngKey& key_w, int s, int g, int co_g) {
  ChannelConsts c;
  c.bias0 = 0.f, c.bias1 = 0.f;
  if (l.mu_b && co_g < a.Cog) {
    const int co = g * a.Cog + co_g;
    float e;
    if constexpr (INJ) e = l.eps_b[(long long)s * a.Co + co];
    else e = bias_eps(key_w, l.layer_id, a.sample0 + (uint32_t)s, co);
    const float dl = __fmul_rn(softplus(l.rho_b[co]), e);
    c.bias0 = FLIP ? l.mu_b[co] : __fadd_rn(l.mu_b[co], dl);
    c.bias1 = dl;
  }
  const bool cv = l.ep_scale && co_g < a.Cog;
  const int cs = cv ? g * a.Cog + co_g : 0;
  const float sc = l.ep_scale ? l.ep_scale[cs] : 1.f, sh = l.ep_shift ? l.ep_shift[cs] : 0.f;
  c.scale = cv ? sc : 1.f;
  c.shift = cv ? sh : 0.f;
  return c;
}
template <bool FLIP, bool INJ>
__device__ __forceinline__ ChannelConsts channel_consts(const FwdArgs& a, const RngKey& key_w, int s, int g, int co_g) {
  return channel_consts<FLIP, INJ>(a, ChannelSrc{a.mu_b, a.rho_b, a.eps_b, a.ep_scale, a.ep_shift, a.layer_id}, key_w, s, g, co_g);
}

// ---------------------------------------------------------------------------- KL sweep
// One thread's share of its workgroup's slice of the flat parameter tensors: float4 groups STRIDE elements apart (STRIDE = 4 x the
// threads that sweep), then a scalar tail. The workgroups blockIdx.x < a.kl_slices own one slice each. However the groups are
// consumed -- one per K-stage behind the MFMAs, all at once, N loads deep -- a thread adds them in the same order.
template <int STRIDE>
struct KlSlice {
  long long i = 0, hi = 0;
  double acc = 0.0;
  bool v4 = false;
  __device__ __forceinline__ void open(const FwdArgs& a, int t) {  // t: this thread's index among the sweeping threads
    long long chunk = (a.w_elems + a.kl_slices - 1) / a.kl_slices;
    chunk = (chunk + 3) & ~3ll;
    const long long lo = (long long)blockIdx.x * chunk;
    hi = (lo + chunk < a.w_elems) ? lo + chunk : a.w_elems;
    v4 = ((((uintptr_t)a.mu_w | (uintptr_t)a.rho_w | (uintptr_t)a.pmu_w | (uintptr_t)a.psig_w) & 15u) == 0);
    i = lo + 4ll * t;
  }
  __device__ __forceinline__ bool group(const FwdArgs& a) {  // -> false when this thread has no whole float4 group left
    if (!(v4 && i + 3 < hi)) return false;
    const float4 m4 = *reinterpret_cast<const float4*>(a.mu_w + i), r4 = *reinterpret_cast<const float4*>(a.rho_w + i);
    const float4 p4 = *reinterpret_cast<const float4*>(a.pmu_w + i), q4 = *reinterpret_cast<const float4*>(a.psig_w + i);
    acc += kl_quad(m4, r4, p4, q4);
    i += STRIDE;
    return true;
  }
  __device__ __forceinline__ double tail(const FwdArgs& a) {  // tail quad / unaligned bases -> the wave's sum
    for (; i < hi; i += STRIDE)
      for (int j = 0; j < 4; ++j)
        if (i + j < hi) acc += (double)kl_term(a.mu_w[i + j], softplus(a.rho_w[i + j]), a.pmu_w[i + j], a.psig_w[i + j]);
    return wave_sum(acc);
  }
  __device__ __forceinline__ double rest(const FwdArgs& a) {  // the remaining groups, one at a time, and the tail
    while (group(a)) {}
    return tail(a);
  }
  // The same with N groups per trip, all 4 N loads in flight before the first use: for the kernels that sweep at their head, where
  // one group at a time is one exposed memory round trip per group.
  template <int N>
  __device__ __forceinline__ double rest_batched(const FwdArgs& a) {
    if (v4) {
      while (i + 3 < hi) {
        float4 m4[N], r4[N], p4[N], q4[N];
        bool ok[N];
#pragma unroll
        for (int u = 0; u < N; ++u) {
          const long long iu = i + (long long)u * STRIDE;
          ok[u] = iu + 3 < hi;
          if (ok[u]) {
            m4[u] = *reinterpret_cast<const float4*>(a.mu_w + iu), r4[u] = *reinterpret_cast<const float4*>(a.rho_w + iu);
            p4[u] = *reinterpret_cast<const float4*>(a.pmu_w + iu), q4[u] = *reinterpret_cast<const float4*>(a.psig_w + iu);
          }
        }
#pragma unroll
        for (int u = 0; u < N; ++u) {
          if (ok[u]) {
            acc += kl_quad(m4[u], r4[u], p4[u], q4[u]);
            i += STRIDE;
          }
        }
      }
    }
    return tail(a);
  }
};

// The last arriver's close: every slot is published. `t` is the calling lane's share of the slot sum, added in the kernel's own slot
// order (kl_slot_sum below, or the skinny kernel's eight-deep loop); + the bias term, -> kl_out, and the counter back to zero.
__device__ __forceinline__ void kl_close(const FwdArgs& a, double t, int lane) {
  t = wave_sum(t);
  double bt_ = 0.0;
  if (a.mu_b)
    for (int c = lane; c < a.Co; c += 64) bt_ += (double)kl_term(a.mu_b[c], softplus(a.rho_b[c]), a.pmu_b[c], a.psig_b[c]);
  bt_ = wave_sum(bt_);
  if (lane == 0) {
    float kl = (float)(t / (double)a.w_elems);
    if (a.mu_b) kl += (float)(bt_ / (double)a.Co);
    a.kl_out[0] = kl;
    __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // leave the workspace zeroed
  }
}
__device__ __forceinline__ double kl_slot_sum(const FwdArgs& a, int nslots, int lane) {  // slots lane, lane + 64, ... in index order
  double t = 0.0;
  for (int q = lane; q < nslots; q += 64) t += __hip_atomic_load(&a.slots[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // calls leave the workspace zeroed (include/bt_hip.h); a loop of its own, so that the loads above stay back to back
  for (int q = lane; q < nslots; q += 64) __hip_atomic_store(&a.slots[q], 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return t;
}

// ---------------------------------------------------------------------------- tile column -> output coordinates
// A tile is t_NI images x t_R output rows x t_Wt output columns starting at (b0, r0, w0); tile column ml = (img * t_R + r) * t_Wt + w,
// RW = t_R * t_Wt, columns >= Mt are dead. inv_rw / inv_wt: ceil(2^32 / RW), ceil(2^32 / t_Wt) (0 where the divisor is 1), from the
// host or computed by the kernel.
struct ColDecode {
  int b0, r0, w0, RW, Mt, t_Wt;
  uint32_t inv_rw, inv_wt;
  int B, Ho, Wo;
  __device__ __forceinline__ bool decode(int ml, int& b, int& ho, int& wo) const {  // false: dead column
    const int img = RW == 1 ? ml : (int)__umulhi((uint32_t)ml, inv_rw);
    const int rem = ml - img * RW;
    const int r = t_Wt == 1 ? rem : (int)__umulhi((uint32_t)rem, inv_wt);
    b = b0 + img, ho = r0 + r, wo = w0 + (rem - r * t_Wt);
    return ml < Mt && b < B && ho < Ho && wo < Wo;
  }
};

}  // namespace bt
