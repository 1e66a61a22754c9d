/*
 * bt_hip.h -- C ABI of libbtorch_hip.so: the MI355X (gfx950) implementation of
 * bayesian-torch's stochastic variational-layer forward + KL hot path.
 *
 * The reference (godhj93/bayesian-torch) has no FFI of its own: the path is a
 * chain of ATen calls inside four nn.Module.forward() methods.  Each entry point
 * below replaces one such chain; the Python layer classes in
 * bayesian_torch_amd/layers/ bind them with ctypes (INTEGRATION.md shows the
 * stub a maintainer of the reference would add).  Citations are relative to
 * /root/reference/bayesian_torch/.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless it says "host";
 *   - no allocation, no host synchronisation, no global state inside a call
 *     (graph-capturable); work is enqueued on `stream` (a hipStream_t);
 *   - return 0 on success, <0 on error (BT_ERR_*); bt_last_error_string() gives
 *     the text for the calling thread;
 *   - `S` MC samples are computed per call: out is [S][...]; sample s uses global
 *     sample id rng.sample0 + s, so results do not depend on how samples are
 *     split over calls, streams or ranks;
 *   - draws: when an eps_* / sign_* pointer is non-NULL the kernel READS the draw
 *     (parity mode: the caller supplies what torch's generator produced); when it
 *     is NULL the kernel generates it on chip from `rng` (Philox4x32-10 + Box-Muller
 *     for eps, a Philox-keyed integer hash for the Flipout signs) and nothing
 *     weight-sized or activation-sized is written to HBM besides `out`;
 *   - kl_out: NULL to skip; otherwise receives kl_weight + kl_bias of the layer
 *     (a function of the parameters only -- computed once, not per sample);
 *   - workspace: BT_WORKSPACE_BYTES device bytes per in-flight call, zero-filled
 *     once by the caller; calls leave it zeroed.
 */
#ifndef BT_HIP_H
#define BT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BT_VERSION 302
#define BT_WORKSPACE_BYTES 65536

#define BT_OK 0
#define BT_ERR_BAD_ARG (-1)
#define BT_ERR_UNSUPPORTED (-2)
#define BT_ERR_WORKSPACE (-3)
#define BT_ERR_HIP_BASE (-1000) /* -(1000 + hipError_t) */

typedef void *bt_stream_t; /* hipStream_t */

/* Counter-based RNG coordinates; used only for draws whose pointer is NULL. */
typedef struct bt_rng {
  uint64_t seed;                 /* Philox key */
  const uint32_t *call_base_dev; /* optional DEVICE word added to `call` when the kernel runs: lets a captured
                                    hipGraph draw fresh eps on every replay (advance the word between replays) */
  uint32_t call;                 /* advance once per forward call (a fresh draw per call) */
  uint32_t layer_id;             /* < 2^28: distinct per Bayesian layer of a model */
  uint32_t sample0;              /* global id of this call's first MC sample */
  uint32_t flags;                /* BT_DRAWS_*: layout of the injected draws (0: the natural layouts of bt_draws) */
} bt_rng;
/* bt_draws.eps_w holds [S] packed images as written by bt_pack_eps (the layout of bt_params.mu_packed) instead of [S][Co*K];
 * eps_b stays [S][Co]. Reparameterization only. The launch is offered to the split-precision (bf16x3) kernels alone, whose
 * injected instantiations read a unit's four draws with one 16-byte load where the on-chip ones run Philox: the same draws give
 * the same output bits as the on-chip launch. Needs mu_packed / sigma_packed; BT_ERR_UNSUPPORTED (nothing launched) with sign
 * tensors, under bt_set_contraction(1 | 2 | 3) / BT_CONTRACTION=f32 | bf16x2 | bf16, or when no split flavour takes the launch -- call again
 * with the natural layout then. The fused max-pool is available on this path. */
#define BT_DRAWS_EPS_PACKED 1u
/* With BT_DRAWS_EPS_PACKED, on the Flipout entry points: bt_draws.sign_in / sign_out point at the [S] BYTE images written by
 * bt_pack_signs (one byte per element, 0x00 = +1, 0x80 = -1, BT_SIGNS_PACKED_STRIDE(n) bytes per sample) instead of fp32 tensors,
 * and the launch is offered to the split-precision Flipout kernels alone, whose injected instantiations read the weight draws, the
 * bias draws (eps_b [S][Co], exactly when the layer has a bias) and both sign streams where the on-chip ones run Philox and the sign
 * hash: the draw an on-chip launch made (bt_rng_normal_fill / bt_rng_sign_fill) gives the same output bits. Needs eps_w and both
 * images, 16-byte aligned, and mu_packed / sigma_packed. CONTRACT FOR THE SIGNS ON THIS PATH: +1 or -1. A byte image has no third
 * value: an exact 0 (torch's uniform_(-1, 1).sign() yields one with probability 2^-24 per element) is read as +1, and bt_pack_signs
 * counts it; the natural-layout path keeps multiplying by whatever value it is given. BT_ERR_BAD_ARG without BT_DRAWS_EPS_PACKED or
 * on a Reparameterization entry point; BT_ERR_UNSUPPORTED (nothing launched) under a forced f32 / bf16x2 / bf16 contraction or when no
 * split-precision Flipout flavour takes the geometry -- call again with the natural layouts then. BT_DRAWS_EPS_PACKED alone on a
 * Flipout entry point stays BT_ERR_UNSUPPORTED. The fused max-pool is available on this path (the Flipout stem kernel). */
#define BT_DRAWS_SIGNS_PACKED 2u
#define BT_SIGNS_PACKED_STRIDE(n) ((((int64_t)(n)) + 15) & ~(int64_t)15) /* bytes of one sample's image of n signs */

/* Variational parameters and priors of one layer. weight is [Co][K] row-major
 * (Linear: K = in_features; Conv2d: K = (Ci/groups)*kh*kw, i.e. the native
 * [Co][Ci/groups][kh][kw] tensor).  Priors are full per-element tensors, read at
 * call time (users overwrite them: utils/util.py:102-117); only read when
 * kl_out != NULL. */
typedef struct bt_params {
  const float *mu_w, *rho_w;
  const float *mu_b, *rho_b; /* [Co] or both NULL */
  const float *prior_mu_w, *prior_sigma_w;
  const float *prior_mu_b, *prior_sigma_b;
  /* optional tap-major re-layout of the parameters, built by bt_pack_params and valid until mu_w / rho_w change:
   * mu_packed[(co*T + tap)*Ci4 + ci] = mu_w[co][ci][tap], sigma_packed[...] = log1p(exp(rho_w[co][ci][tap])),
   * Ci4 = Ci/groups rounded up to a multiple of 4 (padding holds 0). With them a weight unit (4 channels of one tap) is one
   * 16-byte load at the byte offset of its draw index, pruned taps are never touched in memory, and the kernel does no
   * softplus. Both NULL: the general kernel reads the natural layout. */
  const float *mu_packed, *sigma_packed;
  int32_t prior_kind; /* BT_PRIOR_NORMAL (kl_div 'normal'), BT_PRIOR_LAPLACE (kl_div 'laplace': base_variational_layer.py:74-97) */
  int32_t reserved;
} bt_params;
#define BT_PRIOR_NORMAL 0
#define BT_PRIOR_LAPLACE 1

/* Injected draws (NULL => generate on chip). Layouts: eps_w [S][Co*K],
 * eps_b [S][Co], sign_in [S][elements of one sample's x], sign_out
 * [S][elements of one sample's out]; sign values are the fp32 +1/-1/0 that
 * torch's uniform_(-1,1).sign() yields. */
typedef struct bt_draws {
  const float *eps_w, *eps_b;
  const float *sign_in, *sign_out; /* Flipout only */
  bt_rng rng;
} bt_draws;

typedef struct bt_conv2d_geom {
  int32_t B, Ci, H, W;    /* input  [B][Ci][H][W]  (NCHW) */
  int32_t Co, kh, kw;     /* weight [Co][Ci/groups][kh][kw] */
  int32_t sh, sw, ph, pw, dh, dw, groups;
} bt_conv2d_geom;

/* Optional fused output stage (inference-time Conv+BN(+add)(+ReLU) folding, SURVEY.md section 8(f) rank 4;
 * the reference folds BN only in its quantised path, models/bnn_to_qbnn.py:174-196). Applied per output
 * element after the layer's own result v (bias and Flipout perturbation included):
 *     v = v * scale[co] + shift[co]   (when scale != NULL; BatchNorm in eval mode is exactly this affine map)
 *     v = v + residual_s[idx]         (when residual != NULL; same layout as one sample of out)
 *     v = max(v, 0)                   (when relu != 0)                                                      */
typedef struct bt_epilogue {
  const float *scale, *shift;      /* [Co] each, or both NULL */
  const float *residual;           /* NULL, or [S][elements of one sample's out] / shared when stride is 0 */
  int64_t residual_sample_stride;  /* elements between samples, or 0 */
  int32_t relu;
  int32_t pool;                    /* BT_POOL_NONE, or BT_POOL_MAX_3x3_S2_P1: conv2d entry points only (see below) */
} bt_epilogue;

/* Fused max-pool of the output stage's result -- the ResNet stem's conv -> (folded BN) -> ReLU -> MaxPool2d(3, 2, 1) as one
 * launch: out is [S][B][Co][Hp][Wp] with Hp = (Ho - 1) / 2 + 1, Wp = (Wo - 1) / 2 + 1, NaN-propagating like
 * torch.nn.functional.max_pool2d. No residual with it. The launch returns BT_ERR_UNSUPPORTED (nothing written) when it cannot
 * fuse -- tiles that do not hold whole output images (large feature maps), Flipout, injected draws in the natural layout (packed
 * ones, BT_DRAWS_EPS_PACKED, pool on the stem kernel), input rows that are not 16-byte aligned (W % 4 != 0): pool separately then. */
#define BT_POOL_NONE 0
#define BT_POOL_MAX_3x3_S2_P1 1

int bt_version(void);
const char *bt_last_error_string(void);
/* Diagnostic: the kernel instance (template name and tile) the calling thread's last fused-forward launch selected --
 * lets a benchmark attribute per-launch times to kernel instances the way rocprofv3's kernel trace does. */
const char *bt_last_kernel_name(void);
/* Scratch the split-K flavour of the forwards wants for this geometry (layers whose output map is one pixel: Linear, 1x1-map
 * convolutions; 0 for every other layer). Optional: hand the forward a workspace of BT_WORKSPACE_BYTES + this many bytes -- the
 * head zero-filled as always, the rest uninitialised -- and it may split the contraction over K-slices that meet in the scratch (a
 * fixed-order, deterministic combine); with a plain BT_WORKSPACE_BYTES workspace the other kernels serve the launch. */
size_t bt_fused_scratch_bytes(const bt_conv2d_geom *g, int32_t S);

/* ... and that launch's tile geometry, for a benchmark's roofline model: out[0..n) <- {workgroups, m_tiles, n_tiles, S, images per
 * tile, output rows per tile, output columns per tile, pixel_major, row_tiles, kl_slices, groups, n_bt, n_rt, n_ct, fused KL, 0}. */
int bt_last_launch_info(int64_t *out, int32_t n);

/* a5: LinearReparameterization.forward  (layers/variational_layers/linear_variational.py:160-181)
 *   out[s][b][o] = sum_k x_s[b][k] * (mu_w + log1p(exp(rho_w)) * eps_w[s])[o][k] + (mu_b + log1p(exp(rho_b)) * eps_b[s])[o]
 * x_sample_stride: 0 when all S samples share x [B][In]; else elements between samples (B*In). */
int bt_reparam_linear_fwd(int32_t B, int32_t In, int32_t Out, int32_t S,
                          const float *x, int64_t x_sample_stride,
                          const bt_params *p, const bt_draws *d, const bt_epilogue *ep /* or NULL */,
                          float *out /* [S][B][Out] */, float *kl_out /* [1] or NULL */,
                          void *workspace, size_t workspace_bytes, bt_stream_t stream);

/* a8: Conv2dReparameterization.forward  (layers/variational_layers/conv_variational.py:362-385)
 *   F.conv2d(x_s, mu + log1p(exp(rho)) * eps[s], bias_s, stride, padding, dilation, groups) as an implicit GEMM. */
int bt_reparam_conv2d_fwd(const bt_conv2d_geom *g, int32_t S,
                          const float *x, int64_t x_sample_stride,
                          const bt_params *p, const bt_draws *d, const bt_epilogue *ep /* or NULL */,
                          float *out /* [S][B][Co][Ho][Wo] */, float *kl_out,
                          void *workspace, size_t workspace_bytes, bt_stream_t stream);

/* A CHAIN of n <= BT_CHAIN_MAX Conv2dReparameterization layers of one shape -- member k + 1 convolves what member k wrote, as in the
 * identity-shortcut blocks of a ResNet stage -- as ONE launch: every workgroup walks the n layers over its own images. m[k] is the call
 * bt_reparam_conv2d_fwd would get for member k (its geometry, x, parameters, draws, epilogue, out), in execution order; the results are
 * bit for bit those of the n calls. The launch is taken only when every member, planned exactly as its own call would be, gets the same
 * tile of whole images and all of a layer's channels (64 channels x 512 positions: small maps, Co <= 64, groups 1, stride 1, a window
 * larger than 1x1), with on-chip draws, packed parameters, the automatic contraction mode, no fused max-pool and no KL sweep
 * (kl_out NULL); m[k].x is m[k - 1].out with x_sample_stride = one sample's out; a residual is the chain's input, exactly an earlier
 * member's out, or a buffer outside the chain; and no two of {m[0].x, the outs} overlap. Returns BT_OK, an error (< 0), or
 * BT_CHAIN_DECLINED when the members are valid but not such a chain: NOTHING is launched then, and the caller makes the n calls.
 * bt_last_kernel_name / bt_last_launch_info describe the chain launch (the tile geometry every member shares). */
#define BT_CHAIN_MAX 4
#define BT_CHAIN_DECLINED 1
typedef struct bt_chain_member {
  const bt_conv2d_geom *g;
  const float *x;
  int64_t x_sample_stride;
  const bt_params *p;
  const bt_draws *d;
  const bt_epilogue *ep; /* or NULL */
  float *out;            /* [S][B][Co][Ho][Wo] */
  float *kl_out;         /* NULL in a chain (a member that asks for its KL is declined) */
} bt_chain_member;
int bt_reparam_conv2d_chain_fwd(int32_t n, const bt_chain_member *m, int32_t S, bt_stream_t stream);

/* The same two convolutions over an INPUT-DILATED image: the forward of a transposed convolution without its zero-upsampled copy.
 * x is the real input [B][Ci][g->H][g->W]; the kernels convolve the virtual image of
 *     Hv = (H - 1) * uh + 1 + lo_h + hi_h,   Wv = (W - 1) * uw + 1 + lo_w + hi_w
 * pixels -- uh - 1 / uw - 1 zeros between neighbouring input pixels, lo / hi zeros around them -- with the weights in Conv2d layout
 * [Co][Ci/groups][kh][kw] (a ConvTranspose kernel with its channel axes swapped and its taps flipped), stride g->sh / g->sw and
 * dilation g->dh / g->dw as usual: out is [S][B][Co][Ho][Wo] over (Hv, Wv). g->ph and g->pw must be 0 (the padding is explicit).
 * The virtual pixels are resolved where the kernels form their x addresses: nothing of size Hv x Wv is written or read. Tile plan,
 * tap pruning, K order and draw streams are those of bt_*_conv2d_fwd on the materialised image, so Reparameterization results are the
 * same bits where both run the general split-precision kernel; Flipout draws ONE input sign per real element, indexed in
 * [B][Ci][H][W] (bt_rng_sign_fill, tensor 2, n = B*Ci*H*W) -- the reference's distribution, not the materialised launch's stream.
 * Kernels: the general split-precision kernel (x fetch mode 5; bt_set_contraction modes 0 and 3) or the fp32 general kernel. On-chip
 * draws only and no fused max-pool: BT_ERR_UNSUPPORTED with nothing launched otherwise. uh, uw < 1, a negative lo / hi, or
 * ph / pw != 0: BT_ERR_BAD_ARG. With uh == uw == 1 and no padding the call is bt_*_conv2d_fwd, launch for launch. */
typedef struct bt_updil {
  int32_t uh, uw;                 /* input dilation, >= 1 */
  int32_t lo_h, hi_h, lo_w, hi_w; /* explicit zero padding of the dilated image, >= 0 */
} bt_updil;
int bt_reparam_conv2d_updil_fwd(const bt_conv2d_geom *g, const bt_updil *u, int32_t S,
                                const float *x, int64_t x_sample_stride,
                                const bt_params *p, const bt_draws *d, const bt_epilogue *ep /* or NULL */,
                                float *out /* [S][B][Co][Ho][Wo] */, float *kl_out,
                                void *workspace, size_t workspace_bytes, bt_stream_t stream);
int bt_flipout_conv2d_updil_fwd(const bt_conv2d_geom *g, const bt_updil *u, int32_t S,
                                const float *x, int64_t x_sample_stride,
                                const bt_params *p, const bt_draws *d, const bt_epilogue *ep /* or NULL */,
                                float *out, float *kl_out,
                                void *workspace, size_t workspace_bytes, bt_stream_t stream);

/* The same two convolutions over a DEPTH-WINDOWED input: the forward of a Conv3d as ONE Conv2d launch, without its depth-unfolded copy.
 * g describes the launch over the virtual (unfolded) operand -- B' = B * Do images of Ci' = Ci * kd channels, with
 *     Do = (D + 2 * pd - dd * (kd - 1) - 1) / sd + 1;
 * H, W, spatial stride / padding / dilation and groups are the real ones -- and x is the real [B][Ci][D][H][W] (x_sample_stride in real
 * elements). Launch image b' = b * Do + dz, launch channel c' = ci * kd + j, pixel (y, x) reads x[b][ci][dz * sd - pd + j * dd][y][x],
 * a zero where that depth is outside [0, D); the weights are the Conv3d kernel as it lies in memory, [Co][(Ci / groups) * kd][kh][kw];
 * out is [S][B * Do][Co][Ho][Wo]. The window is resolved where the kernels form their x addresses: nothing of the unfolded size is
 * written or read. Tile plan, tap pruning, K order and weight-draw streams are those of bt_*_conv2d_fwd on the materialised operand, so
 * Reparameterization results are the same bits where both run the general split-precision kernel; Flipout draws ONE input sign per real
 * element, indexed in [B][Ci][D][H][W] (bt_rng_sign_fill, tensor 2, n = B*Ci*D*H*W) -- the reference's distribution, not the stream over
 * the unfolded operand, where an element has one sign per window it appears in.
 * Kernels: the general split-precision kernel (x fetch mode 6; bt_set_contraction modes 0 and 3) or the fp32 general kernel. On-chip
 * draws only and no fused max-pool: BT_ERR_UNSUPPORTED with nothing launched otherwise. BT_ERR_BAD_ARG: kd, D, sd, dd < 1; pd < 0;
 * Do < 1; g->B % Do != 0; (g->Ci / g->groups) % kd != 0; a real or virtual x of 2^30 elements or more. With kd == 1, D == 1 and
 * pd == 0 the call is bt_*_conv2d_fwd, launch for launch. */
typedef struct bt_dwin {
  int32_t kd, D;      /* depth taps, real depth */
  int32_t sd, dd, pd; /* depth stride / dilation / padding */
} bt_dwin;
int bt_reparam_conv2d_dwin_fwd(const bt_conv2d_geom *g, const bt_dwin *w, int32_t S,
                               const float *x, int64_t x_sample_stride,
                               const bt_params *p, const bt_draws *d, const bt_epilogue *ep /* or NULL */,
                               float *out /* [S][B*Do][Co][Ho][Wo] */, float *kl_out,
                               void *workspace, size_t workspace_bytes, bt_stream_t stream);
int bt_flipout_conv2d_dwin_fwd(const bt_conv2d_geom *g, const bt_dwin *w, int32_t S,
                               const float *x, int64_t x_sample_stride,
                               const bt_params *p, const bt_draws *d, const bt_epilogue *ep /* or NULL */,
                               float *out, float *kl_out,
                               void *workspace, size_t workspace_bytes, bt_stream_t stream);

/* a9: LinearFlipout.forward  (layers/flipout_layers/linear_flipout.py:145-174)
 *   out = x W_mu^T + mu_b + ((x o s_in) (sigma o eps)^T + sigma_b o eps_b) o s_out  -- both contractions share one x tile. */
int bt_flipout_linear_fwd(int32_t B, int32_t In, int32_t Out, int32_t S,
                          const float *x, int64_t x_sample_stride,
                          const bt_params *p, const bt_draws *d, const bt_epilogue *ep /* or NULL */,
                          float *out, float *kl_out,
                          void *workspace, size_t workspace_bytes, bt_stream_t stream);

/* a10: Conv2dFlipout.forward  (layers/flipout_layers/conv_flipout.py:370-417) */
int bt_flipout_conv2d_fwd(const bt_conv2d_geom *g, int32_t S,
                          const float *x, int64_t x_sample_stride,
                          const bt_params *p, const bt_draws *d, const bt_epilogue *ep /* or NULL */,
                          float *out, float *kl_out,
                          void *workspace, size_t workspace_bytes, bt_stream_t stream);

/* a1/a6/a12: kl_div 'normal' branch + kl_loss() + get_kl_loss()
 * (layers/base_variational_layer.py:68-72, linear_variational.py:146-158, models/dnn_to_bnn.py:157-165)
 *   kl_out[0] = sum_seg mean_i( log sp - log sq + (sq^2 + (mq - mp)^2) / (2 sp^2) - 0.5 ),  sq = log1p(exp(rho))
 * one launch over up to BT_KL_MAX_SEGMENTS tensors (a layer's weight and bias are two segments;
 * a whole model's layers can go in one call). Segment arrays are HOST arrays. */
#define BT_KL_MAX_SEGMENTS 64
#define BT_KL_RHO_IS_SIGMA 1u /* flags: the `rho` arrays already hold sigma (kl_div() called directly) */
#define BT_KL_PRIOR_LAPLACE 2u /* flags: kl_div's 'laplace' branch (base_variational_layer.py:74-97) for every segment:
                                  mean_i( log 2 - 0.5 log(2 pi sq^2) - 0.5 + E|w_i| ) against Laplace(0, 1) -- the reference
                                  hard-codes that prior and ignores the prior tensors; so does this flag (pass any valid tensors) */
int bt_kl_normal(int32_t n_segments, const float *const *mu, const float *const *rho,
                 const float *const *prior_mu, const float *const *prior_sigma, const int64_t *numel,
                 const int32_t *layer_of_segment /* host, non-decreasing, or NULL: the fp32 sum is formed as
                                                    sum_layers( sum_{segments of layer} mean ) like get_kl_loss */,
                 uint32_t flags, float *kl_out /* [1] */, void *workspace, size_t workspace_bytes, bt_stream_t stream);

/* Fills bt_params.mu_packed / sigma_packed (each Co * taps * Ci4 floats) from the natural [Co][Ci][taps] tensors; sigma uses
 * the kernels' own softplus, so a forward with or without the packed copies is bit-identical. */
int bt_pack_params(const float *mu_w, const float *rho_w, int64_t Co, int64_t Ci, int64_t taps,
                   float *mu_packed, float *sigma_packed, bt_stream_t stream);

/* Re-lays S draws of a weight tensor, eps_w [S][Co][Ci][taps] (Ci = in_channels / groups: the natural layout of bt_draws), into
 * eps_packed [S][(co*taps + tap)*Ci4 + ci] -- per sample the layout of mu_packed, padding channels 0.0 -- for
 * BT_DRAWS_EPS_PACKED launches. S * Co * taps * Ci4 floats. Stream-ordered, no host synchronisation, graph-capturable. */
int bt_pack_eps(const float *eps_w, int32_t S, int64_t Co, int64_t Ci, int64_t taps, float *eps_packed, bt_stream_t stream);

/* Packs S Flipout sign tensors, signs [S][n] fp32 (sign_in: n = elements of one sample's x; sign_out: n = elements of one sample's
 * contraction output, before any fused pooling), into signs_packed [S][BT_SIGNS_PACKED_STRIDE(n)] bytes for BT_DRAWS_SIGNS_PACKED
 * launches: byte i of a sample's image is 0x80 when element i is negative, else 0x00, in the tensor's own element order (byte << 24
 * is the fp32 sign mask, byte << 8 the bf16 one); the stride is n rounded up to 16 and the padding bytes are 0, so a kernel that
 * fetches four consecutive elements as one float4 fetches their signs as one aligned dword at the same element index. signs_packed
 * must be 16-byte aligned. *not_pm1_count (DEVICE word) <- the number of elements of THIS call that are not exactly +1 or -1 (an
 * exact 0 or a NaN is packed as +1, any other value by its sign): set, not accumulated. Stream-ordered (a memset node and one
 * launch), no host synchronisation, graph-capturable. */
int bt_pack_signs(const float *signs, int32_t S, int64_t n, uint8_t *signs_packed, uint32_t *not_pm1_count, bt_stream_t stream);

/* Keeps the packed copies of up to BT_PACK_MAX_SEGMENTS layers in step with their parameters, checked ON THE DEVICE in the
 * stream (two launches, no host synchronisation, graph-capturable): a 64-bit fingerprint of every layer's natural-layout
 * (mu_w, rho_w) -- the wrapping sum of a 64-bit mix of (element index, mu bits, rho bits): order-independent, so deterministic --
 * is compared with the one stored in `state` when the pack was last built, and exactly the layers that differ (or carry
 * `force`) are re-packed in place. The reference's own code writes parameters through `.data` (models/dnn_to_bnn.py:65-71,95-101,
 * utils/util.py:102-117 in MOPED()), which no host-side version counter can see: with this call in front of the forward a
 * stale pack cannot be read. Segment array: HOST. */
#define BT_PACK_MAX_SEGMENTS 64
typedef struct bt_pack_seg {
  const float *mu_w, *rho_w;       /* the parameters, natural layout: what the fingerprint covers */
  const float *src_mu, *src_rho;   /* optional: an exact re-arrangement of them to pack from ([Co][Ci][taps]; the transposed-convolution
                                      layers pack their channel-transposed, flipped kernel); both NULL = mu_w / rho_w */
  float *mu_packed, *sigma_packed; /* [Co][taps][Ci4], rewritten in place when the fingerprint differs */
  uint64_t *state;                 /* DEVICE, 4 words owned by the layer, zero-filled once: accumulator (left zero), fingerprint
                                      of the packed copy, dirty flag of the last call, number of rebuilds so far */
  int64_t Co, Ci, taps;            /* geometry of the pack source */
  int32_t force;                   /* rebuild whatever the fingerprint says (first use of fresh buffers) */
  int32_t reserved;
} bt_pack_seg;
int bt_pack_sync(int32_t n_segments, const bt_pack_seg *segs, void *workspace, size_t workspace_bytes, bt_stream_t stream);

/* bt_pack_sync that also produces layers' KL terms from the sweep it makes anyway: for every segment whose kls[i].kl_out is
 * not NULL, kl_out (DEVICE float) <- mean over the weights of kl_div's 'normal' branch + (bias given) the mean over the bias,
 * the value a fused forward with kl_out writes (each mean accumulated in double, then rounded to fp32 and added), so that the
 * layer's forward can run without its own KL sweep. The priors have mu_w's shape; the bias tensors have n_bias elements, or
 * are all NULL. kls: HOST array of n_segments entries, or NULL (= bt_pack_sync). */
typedef struct bt_pack_kl {
  const float *prior_mu_w, *prior_sigma_w;
  const float *mu_b, *rho_b, *prior_mu_b, *prior_sigma_b;
  float *kl_out;
  int64_t n_bias;
} bt_pack_kl;
int bt_pack_sync_kl(int32_t n_segments, const bt_pack_seg *segs, const bt_pack_kl *kls, void *workspace, size_t workspace_bytes,
                    bt_stream_t stream);

/* The on-chip draws, materialised (test / replay hook: the fused kernels never call these).
 * They emit exactly the streams the fused kernels consume for (rng, tensor_id):
 * tensor_id 0 = eps_w, 1 = eps_b, 2 = sign_in, 3 = sign_out, 4 = z (the low-rank layers' factor draw, bt_lowrank_conv2d_fwd:
 * bt_rng_normal_fill(rng, 4, S, 1, r, 1, ...) gives z [S][r], element j = normal number (j & 3) of Philox block (j >> 2)).
 * Stream definition. eps element (row r, inner index c, tap t) of a [rows][inner][taps] tensor (a conv kernel
 * [Co][Ci/g][kh*kw]; Linear and bias: taps = 1) is normal number (c & 3) of Philox block (e >> 2) with
 * e = (r*taps + t)*inner4 + c,  inner4 = inner rounded up to a multiple of 4  -- tap-major and quad-aligned, so the
 * 4 values of one Philox block are 4 consecutive input channels of ONE tap: a kernel that skips taps which only ever
 * meet zero padding skips their RNG as well, and no block straddles two taps.
 * out is [S][rows*inner*taps] in the tensor's natural memory order. Signs: element i of the flat tensor. */
int bt_rng_normal_fill(const bt_rng *rng, uint32_t tensor_id, int32_t S, int64_t rows, int64_t inner, int64_t taps,
                       float *out, bt_stream_t stream);
int bt_rng_sign_fill(const bt_rng *rng, uint32_t tensor_id, int32_t S, int64_t n, float *out, bt_stream_t stream);
int bt_rng_philox_raw(uint64_t seed, const uint32_t ctr[4], uint32_t out_host[4]); /* host-side Philox4x32-10 KAT hook */

/* Backward of the four fused forwards (the reference relies on torch autograd of
 * linear_variational.py:163-181, conv_variational.py:366-385, linear_flipout.py:149-174, conv_flipout.py:376-417).
 * grad_out is dL/dout [S][B][Co][Ho][Wo] of a forward made with the same (geometry, S, p, d): the draws are REGENERATED on chip
 * from d->rng (or read, when d carries injected draws) -- nothing weight-sized is written to HBM.
 *   dx      [S][B][Ci][H][W] or NULL: per-sample input gradient (sum over S yourself when the forward shared x);
 *   dmu_w / drho_w  the parameters' own layout [Co][Ci/groups][kh][kw], both or neither:
 *           dmu = sum_s dW_s,  drho = sigmoid(rho) * sum_s eps_s o dW_s  (Flipout: mean path -> mu, perturbation path -> rho);
 *   workspace: bt_conv2d_bwd_workspace(g, S) bytes (partials of wgrad's sample / reduction groups and of dgrad's pieces of the
 *           output-channel reduction, summed in a fixed order; contents need not be initialised; needed whenever dx or dmu_w is).
 * Linear layers: g = {B, In, 1, 1, Out, 1, 1, 1, 1, 0, 0, 1, 1, 1}. p needs rho_w, mu_packed, sigma_packed. Bias gradients are
 * row sums of grad_out (not part of this call). */
size_t bt_conv2d_bwd_workspace(const bt_conv2d_geom *g, int32_t S);
int bt_conv2d_bwd(const bt_conv2d_geom *g, int32_t S, int32_t flipout, const float *x, int64_t x_sample_stride, const float *grad_out,
                  const bt_params *p, const bt_draws *d, float *dx, float *dmu_w, float *drho_w,
                  void *workspace, size_t workspace_bytes, bt_stream_t stream);
/* bt_conv2d_bwd with the layer's KL term differentiated in the same pass (a training step's loss holds both: the reference adds
 * get_kl_loss(model) / batch to the criterion, examples/main_bayesian_cifar_dnn2bnn.py:402-420): grad_kl = device scalar, the
 * upstream gradient of THIS layer's weight-KL mean (base_variational_layer.py:70-72; p->prior_kind selects :74-97). Then
 *   dmu_w[i] += grad_kl[0] / n * dKL_i/dmu,  drho_w[i] += grad_kl[0] / n * dKL_i/drho   (n = elements of mu_w)
 * in the op order autograd would add bt_kl_normal_bwd's tensors to bt_conv2d_bwd's: same bits, no second sweep, no KL-gradient
 * tensors. p additionally needs mu_w and (normal prior) prior_mu_w / prior_sigma_w. grad_kl NULL = bt_conv2d_bwd. Bias KL
 * gradients (bias-sized) stay with the caller. */
int bt_conv2d_bwd_kl(const bt_conv2d_geom *g, int32_t S, int32_t flipout, const float *x, int64_t x_sample_stride, const float *grad_out,
                     const bt_params *p, const bt_draws *d, const float *grad_kl, float *dx, float *dmu_w, float *drho_w,
                     void *workspace, size_t workspace_bytes, bt_stream_t stream);
/* Gradient of bt_kl_normal's mean over ONE tensor: dmu[i], drho[i] = d kl / d(mu_i, rho_i) * grad_kl[0] (grad_kl: device
 * scalar); flags: BT_KL_PRIOR_LAPLACE for the 'laplace' branch (priors unused then). */
int bt_kl_normal_bwd(const float *mu, const float *rho, const float *prior_mu, const float *prior_sigma, const float *grad_kl,
                     int64_t numel, uint32_t flags, float *dmu, float *drho, bt_stream_t stream);
/* The same for up to BT_KL_MAX_SEGMENTS tensors in ONE launch (the backward of a whole model's get_kl_loss): segment arrays are
 * HOST arrays like bt_kl_normal's; dmu[i] / drho[i] have numel[i] elements. */
int bt_kl_normal_bwd_segs(int32_t n_segments, const float *const *mu, const float *const *rho, const float *const *prior_mu,
                          const float *const *prior_sigma, const int64_t *numel, const float *grad_kl, uint32_t flags,
                          float *const *dmu, float *const *drho, bt_stream_t stream);

/* kl_loss() of the hierarchical layers (layers/variational_layers/hiearchial_variational_layers.py:331-381, :477-522): every weight
 * has its own variational Inv-Gamma(a, b), a = exp(log_a), b = exp(log_b), over its prior variance, against the hyper-prior (a0, b0):
 *   kl_out[0] = sum_seg SUM_i( 1/2 [ ln b - psi(a) - ln sq^2 + (a/b)(sq^2 + (mu - pm)^2) - 1 ]
 *                              + (a - a0) psi(a) - lnGamma(a) + lnGamma(a0) + a0 (ln b - ln b0) + (b0 - b)(a/b) ),   sq = log1p(exp(rho))
 * -- a SUM over the elements, not bt_kl_normal's mean. One launch over up to BT_KL_MAX_SEGMENTS tensors; segment arrays are HOST
 * arrays, all seven tensors of a segment have numel[i] fp32 elements. A segment's fp64 sum is rounded to fp32; the segments of a
 * layer (layer_of_segment as in bt_kl_normal) are added in fp32, then the layers in order. seg_out: NULL, or n_segments device
 * floats that receive every segment's own fp32 sum. Deterministic; the workspace is left zeroed. Checked on the host before any
 * launch: BT_ERR_BAD_ARG for a bad count, a null pointer, an empty segment or a workspace below BT_WORKSPACE_BYTES. */
int bt_kl_hier(int32_t n_segments, const float *const *mu, const float *const *rho, const float *const *prior_mu,
               const float *const *log_a, const float *const *log_b, const float *const *a0, const float *const *b0,
               const int64_t *numel, const int32_t *layer_of_segment, float *kl_out, float *seg_out, void *workspace,
               size_t workspace_bytes, bt_stream_t stream);
/* Its gradient, element-wise, in ONE launch: d kl / d(mu, rho, log_a, log_b) * grad_kl[0] (grad_kl: device scalar). Each of the
 * four output arrays may be NULL, and so may each of their entries: that gradient is not written. */
int bt_kl_hier_bwd(int32_t n_segments, const float *const *mu, const float *const *rho, const float *const *prior_mu,
                   const float *const *log_a, const float *const *log_b, const float *const *a0, const float *const *b0,
                   const int64_t *numel, const float *grad_kl, float *const *dmu, float *const *drho, float *const *dlog_a,
                   float *const *dlog_b, bt_stream_t stream);
/* Host-side: the kernels' fp32 special functions (csrc/bt_special.h) evaluated on the CPU at n HOST floats x > 0, for tests on a
 * machine without a device. */
#define BT_SPECIAL_DIGAMMA 0       /* psi(x) */
#define BT_SPECIAL_TRIGAMMA 1      /* psi'(x) */
#define BT_SPECIAL_LGAMMA 2        /* ln Gamma(x) */
#define BT_SPECIAL_X_TRIGAMMA_M1 3 /* x psi'(x) - 1, as the log_a gradient uses it (no cancellation at large x) */
int bt_special_eval(int32_t kind, const float *x, int64_t n, float *out);

/* Contraction arithmetic of the fused forwards (process-wide; read at every launch, so a captured graph keeps the kernels it was
 * captured with; default from env BT_CONTRACTION = f32 | bf16x3 | bf16x2 | bf16):
 *   0  automatic: wherever a launch is eligible, every fp32 operand is cut into three bf16 pieces (an EXACT split of the
 *      24-bit significand) and the product runs as the 6 piece products of weight >= 2^-16 on the bf16 matrix pipe with
 *      fp32 accumulation -- fp32-level accuracy at 6/16 of the fp32-MFMA time; other launches use fp32 MFMA;
 *   1  fp32 MFMA everywhere (the bit-exact fp32 FMA chain of round 1);
 *   2  two pieces, 3 product terms (relative error ~1e-5 per product): opt-in;
 *   3  bf16, opt-in, meant for inference: every operand value -- x, and the sampled weight mu + sigma * eps formed in fp32 exactly as
 *      in mode 0 -- is rounded ONCE to bf16 (nearest even) and the product is ONE term per K16 step, fp32 accumulate: relative error
 *      <= 2^-8 per product. It applies to the Reparameterization launches with on-chip draws that mode 0 gives to the general split,
 *      stem or direct kernel, with the same launch plan (the kernel name carries `bf16x1,1 terms` where mode 0's carries
 *      `bf16x3,6 terms`); K order, draw streams, bias draw, output stage and KL (bit-identical to mode 0's) are unchanged. Every
 *      other launch -- Flipout, whatever mode 0 runs on fp32 MFMA, natural-layout injected draws -- runs exactly as in mode 0;
 *      packed injected draws are BT_ERR_UNSUPPORTED as in modes 1 and 2. The backward is not affected: a forward made in this mode
 *      is differentiated by the fp32 backward of the unrounded function.
 * BT_ERR_BAD_ARG for any other mode. */
int bt_set_contraction(int mode);
/* The mode in force (0..3): what bt_set_contraction last set, else BT_CONTRACTION, else 0. */
int bt_get_contraction(void);

/* Conv2dReparameterization_Multivariate (layers/variational_layers/conv_variational.py:409-554): the posterior is a low-rank
 * multivariate normal over the n = Co * Ci * kh * kw weights, and sample s convolves with
 *   w_s[i] = mean_s[i] + sum_{j < R} L[i][j] * z_s[j] + sqrt(d) * eps_s[i]      (j ascending, one fp32 rounding per operation),
 * formed in the producers' registers of the fp32 fused forward; w_s is never written to memory. mean_s = mean + s * mean_stride
 * (0: one mean for all samples -- mu_kernel; n: the [S][n] output of bt_lowrank_mean). L: row-major [n][R], 0 <= R <=
 * BT_LOWRANK_MAX_R (may be NULL when R == 0). d > 0: the constant diagonal of the covariance. Draws: z [S][R] and eps_w [S][n] (the
 * weights' natural order) are both read, or both NULL: z_s is then the first R normals of Philox block 0 of tensor 4, eps the
 * tensor 0 stream of the mean-field layers. groups must be 1; no bias, no KL (bt_kl_lowrank). BT_ERR_BAD_ARG: R outside the range, R > 0
 * without L, d <= 0, one draw without the other. BT_ERR_UNSUPPORTED, nothing launched: any output stage in ep (max-pool, residual, ReLU,
 * scale / shift). out: [S][B][Co][Ho][Wo]. */
#define BT_LOWRANK_MAX_R 4
int bt_lowrank_conv2d_fwd(const bt_conv2d_geom *g, int32_t S, const float *x, int64_t x_sample_stride, const float *mean,
                          int64_t mean_stride, const float *L, int32_t R, float d, const float *z, const float *eps_w, const bt_rng *rng,
                          const bt_epilogue *ep, float *out, bt_stream_t stream);
/* The mean pre-pass of a rank above BT_LOWRANK_MAX_R: m[s][i] = mu[i] + sum_{j < r} L[i][j] * z_s[j], the same fp32 chain (j ascending,
 * one rounding per operation), for all S samples; the forward then runs with R = 0, mean = m, mean_stride = n. z: [S][r], or NULL for
 * the tensor 4 stream of rng (sample rng->sample0 + s). m: [S][n]. L: row-major [n][r]. */
int bt_lowrank_mean(const float *mu, const float *L, int64_t n, int32_t r, int32_t S, const float *z, const bt_rng *rng, float *m,
                    bt_stream_t stream);
/* KL( N(mu, L L^T + d I) || N(prior_mean, diag(prior_var)) ) in closed form, accumulated in fp64 in a fixed order:
 *   KL = 1/2 [ sum log P_i - n log d - logdet(I_r + L^T L / d) + sum (d + sum_j L_ij^2) / P_i + sum (mu_i - m_i)^2 / P_i - n ].
 * Two launches, no host synchronisation: a sweep over the weight index (per-chunk partials of the four sums and of the lower triangle of
 * L^T L / d), then one workgroup that adds the partials in chunk order and factorises I + G by an fp64 Cholesky in the workspace.
 * kl_out[0] = KL, kl_out[1] = KL / n. A pivot that is not positive gives NaN in both and adds 1 to *bad_pivots (may be NULL).
 * workspace: bt_kl_lowrank_workspace(n, r) bytes, 8-byte aligned, contents need not be initialised (0: r above 4096, unsupported). */
size_t bt_kl_lowrank_workspace(int64_t n, int32_t r);
int bt_kl_lowrank(const float *mu, const float *L, int64_t n, int32_t r, float d, const float *prior_mean, const float *prior_var,
                  float *kl_out, int32_t *bad_pivots, void *workspace, size_t workspace_bytes, bt_stream_t stream);

/* Training backward of bt_lowrank_conv2d_fwd (the reference differentiates conv_variational.py:516-552 with torch autograd). Two
 * implicit GEMMs on fp32 MFMA, 64 x 64 tiles, with bt_conv2d_bwd's split of the two reductions (summed in a fixed order, no atomics:
 * the same coordinates give the same bits):
 *   dx   [S][B][Ci][H][W] or NULL: dX_s = conv_transpose(g_s, W_s), W_s regenerated per LDS stage as the forward forms it,
 *        w_s[i] = mean_s[i] + sum_{q < R} L[i][q] * z_s[q] + sd * eps_s[i]   (q ascending, one rounding per operation; sd = sqrtf(d)),
 *        mean and L read in the weights' natural order [Co][Ci][kh][kw] -- nothing weight-sized per sample is written;
 *   dW   [S][n] or NULL: D_s[co][ci][tap] = sum_{b,ho,wo} g_s * x_s window, per sample, the weights' natural order (it needs no draws).
 * mean_s = mean + s * mean_sample_stride (0, or n for the [S][n] output of a bt_lowrank_mean pre-pass recomputed by the caller: a rank
 * above BT_LOWRANK_MAX_R runs with L = NULL, R = 0). Draws: z [S][R] and eps_w [S][n] are read when eps_w is given (z too when R > 0),
 * else both come from rng (tensors 4 and 0, the forward's streams). workspace: bt_lowrank_conv2d_bwd_workspace(g, S, r) bytes (r: the
 * layer's rank; 0 for a refused geometry), contents need not be initialised, 8-byte aligned. Refused before any launch, BT_ERR_BAD_ARG:
 * a null operand, bad geometry, groups != 1, R outside [0, BT_LOWRANK_MAX_R] or R > 0 without L, sd <= 0 or not finite, neither draws
 * nor rng, z without eps_w; BT_ERR_UNSUPPORTED: the sizes bt_conv2d_bwd refuses, or more than 65535 samples x pieces in a grid. r above
 * BT_LOWRANK_MAX_R adds S * n floats behind the partials (at offset bt_lowrank_conv2d_bwd_workspace(g, S, 0)) for that pre-pass. */
size_t bt_lowrank_conv2d_bwd_workspace(const bt_conv2d_geom *g, int32_t S, int32_t r);
int bt_lowrank_conv2d_bwd(const bt_conv2d_geom *g, int32_t S, const float *x, int64_t x_sample_stride, const float *grad_out,
                          const float *mean, int64_t mean_sample_stride, const float *L, int32_t R, float sd, const float *z,
                          const bt_rng *rng, const float *eps_w, float *dx, float *dW_per_sample, void *workspace,
                          size_t workspace_bytes, bt_stream_t stream);
/* What the calling thread's last bt_lowrank_conv2d_bwd planned, as up to 10 values: dgrad launches, wgrad launches, pieces of dgrad's
 * output-channel reduction, chunks of wgrad's reduction axis, dgrad's grid (x, y, z), wgrad's grid (x, y, z). */
int bt_lowrank_conv2d_bwd_info(int64_t *out, int32_t n);
/* The chain rule's finishing pass over the n x (1 + r) parameter gradients, s ascending, one rounding per operation:
 *   dmu[i] = sum_s dW[s][i],   dL[i][j] = sum_s dW[s][i] * z_s[j]     (any rank r in [1, 4096]).
 * z: [S][r], or NULL for the tensor 4 stream of rng. dmu or dL may be NULL (not wanted), not both. */
int bt_lowrank_wgrad_finish(const float *dW_per_sample, int64_t n, int32_t r, int32_t S, const float *z, const bt_rng *rng, float *dmu,
                            float *dL, bt_stream_t stream);
/* Gradient of bt_kl_lowrank's KL (kl_out[0]) times grad_kl[0] (a device scalar, never read on the host), in fp64 with fp32 results:
 *   dmu = c (mu - m) / P,   dL = c (L / P - L (d I + L^T L)^-1)   (row i of L over P_i).
 * The forward's sweep of L^T L / d, its Cholesky with the factor kept, an explicit r x r inverse from the factor, and one pass over
 * the n x r gradient: five launches, no host synchronisation. A pivot that is not positive: NaN in every gradient, one more in
 * *bad_pivots (may be NULL). dmu or dL may be NULL, not both. workspace: bt_kl_lowrank_bwd_workspace(n, r) bytes, 8-byte aligned
 * (0: r above 4096). */
size_t bt_kl_lowrank_bwd_workspace(int64_t n, int32_t r);
int bt_kl_lowrank_bwd(const float *mu, const float *L, int64_t n, int32_t r, float d, const float *prior_mean, const float *prior_var,
                      const float *grad_kl, float *dmu, float *dL, int32_t *bad_pivots, void *workspace, size_t workspace_bytes,
                      bt_stream_t stream);

/* MC epilogue (examples/main_bayesian_cifar_dnn2bnn.py:551-557 and :402-412): from logits [S][B][C]
 * accumulate into packed[B*C + B + B*C] = [sum_s softmax | sum_s entropy | sum_s logits] (overwrites). */
int bt_mc_epilogue(int32_t S, int32_t B, int32_t C, const float *logits, float *packed, bt_stream_t stream);
/* MaxPool2d(kernel 3, stride 2, padding 1) over `planes` contiguous H x W planes (NCHW with planes = N * C): out holds planes x
 * ((H-1)/2+1) x ((W-1)/2+1). The pooling pass behind a stem whose fused launch returned BT_ERR_UNSUPPORTED for bt_epilogue.pool
 * (its tiles do not hold whole output images: the 112 x 112 ImageNet stem) -- `nn.MaxPool2d(3, 2, 1)` of the example models
 * (models/deterministic/resnet_large.py:120). Same comparisons as torch's max_pool2d (NaNs propagate): the same bits. */
int bt_maxpool_3x3s2(const float *in, float *out, int64_t planes, int32_t H, int32_t W, bt_stream_t stream);

/* The LSTM cell behind a time step's two Linear launches (layers LSTMReparameterization / LSTMFlipout): element-wise, memory-bound.
 * a, b: contiguous [rows][4H], the input-to-hidden and hidden-to-hidden maps' outputs, biases included; b may be null. Gate order over
 * the 4H columns: i, f, g, o (rnn_variational.py:107-153):
 *   i, f, o = sigmoid(z), g = tanh(z) over z = a + b;   c = f * c_prev + i * g;   h = o * tanh(c).
 * c_prev: c_rows rows of stride ld_c (floats); c_rows is rows or a divisor of it and row r reads row r % c_rows -- an initial state
 * shared by the MC samples of a sample-major batch. h_out, c_out: rows rows of stride ld_out, so a step can write its slab of a
 * sequence buffer. act: null for inference, else it receives the four activated gates as [rows][4H] for bt_lstm_cell_bwd.
 * The transcendentals are the hardware's exp2 / rcp, written so that an overflowing exponential lands on the limit (0, 1, -1).
 * Accesses are 16 bytes wide when H % 4 == 0, every pointer given is 16-byte aligned and ld_c, ld_out are multiples of 4, else 4
 * bytes wide with the same values. BT_ERR_BAD_ARG, before any launch: rows < 1, H < 1, a null a / c_prev / h_out / c_out, c_rows
 * not dividing rows, ld_c < H or ld_out < H. */
int bt_lstm_cell_fwd(int64_t rows, int64_t H, const float *a, const float *b, const float *c_prev, int64_t c_rows, int64_t ld_c,
                     float *h_out, float *c_out, int64_t ld_out, float *act, bt_stream_t stream);
/* Its backward, the closed form on the saved activations act = (i, f, g, o) [rows][4H], c_prev as given to the forward and the
 * forward's c_out as c_new (row stride ld_cn):
 *   dc = grad_c + grad_h o (1 - tanh^2 c_new);  di = dc g i (1 - i);  df = dc c_prev f (1 - f);  dg = dc i (1 - g^2);
 *   do = grad_h tanh(c_new) o (1 - o);  dc_prev = dc f.
 * grad_h, grad_c (row strides ld_gh, ld_gc) may each be null: zero. dz: contiguous [rows][4H] = (di, df, dg, do), the gradient of a
 * and of b alike. dc_prev: contiguous [rows][H], per row -- the gradient of a c_prev shared by the samples is its sum over them
 * (the caller's). Access widths and BT_ERR_BAD_ARG as bt_lstm_cell_fwd (null act / c_prev / c_new / dz / dc_prev; the stride of a
 * null gradient is not looked at). */
int bt_lstm_cell_bwd(int64_t rows, int64_t H, const float *act, const float *c_prev, int64_t c_rows, int64_t ld_c, const float *c_new,
                     int64_t ld_cn, const float *grad_h, int64_t ld_gh, const float *grad_c, int64_t ld_gc, float *dz, float *dc_prev,
                     bt_stream_t stream);

/* AvUC calibration losses (utils/avuc_loss.py: AvULoss with T = 1, AUAvULoss with T = 21). logits: contiguous [S][B][C], S >= 1 Monte
 * Carlo samples; labels: [B], 8-byte aligned, only compared with the prediction (an out-of-range label is "inaccurate"). Per row:
 *   p_s = softmax(z_s);  pbar = mean_s p_s;  c = max_k pbar_k;  pred = the first index of that maximum;  acc = (pred == label);
 *   H(p) = -sum p log(p + 1e-10);  u = H(pbar) (unc_type 0) or H(pbar) - mean_s H(p_s) (unc_type 1, S > 1);  t = tanh(u).
 * Thresholds, in double from the fp32 u: T = 1: *threshold, one fp32 value in DEVICE memory (never read on the host); T = 21:
 * th_0 = min u and th_20 = max u exactly, th_j = min u + x_j (max u - min u) between them, x = linspace(0, 1, 21). A row is certain at
 * j iff (double) u <= th_j. Per threshold the four soft sums sums[j] = (n_ac, n_au, n_ic, n_iu) = (sum c (1 - t), sum c t,
 * sum (1 - c)(1 - t), sum (1 - c) t) over the rows of each class, the four integer counts[j], and
 *   AvU_j = (n_ac + n_iu) / (n_ac + n_au + n_ic + n_iu + 1e-10);   *v = AvU_0 (T = 1) or the trapezoid of AvU_j over x_j (T = 21);
 *   *loss = -beta log(*v + 1e-10).
 * Two launches (one wave per row for C <= 64, one workgroup per row above; then one workgroup over the rows), sums in a fixed order,
 * no atomics, no host synchronisation: capturable, and the same bits from run to run. coef: [4][T + 1], what bt_avu_bwd needs of the
 * thresholds. workspace: bt_avu_workspace_bytes(S, B, C, T) bytes, 8-byte aligned, contents need not be initialised; afterwards it
 * holds float [3][B] = (c, u, t), int32 [3][B] = (pred, acc, the number of thresholds below u) and each sample row's softmax
 * max / denominator as float [S][B][2], and bt_avu_bwd reads it. thresholds: [T] doubles, 8-byte aligned.
 * BT_ERR_BAD_ARG before any launch: a null pointer (threshold may be null for T = 21), S, B or C <= 0, T not 1 or 21, unc_type not 0
 * or 1, unc_type 1 with S == 1, a misaligned labels / thresholds / workspace. BT_ERR_WORKSPACE: workspace_bytes too small. */
size_t bt_avu_workspace_bytes(int32_t S, int32_t B, int32_t C, int32_t T);
int bt_avu_fwd(int32_t S, int32_t B, int32_t C, const float *logits, const int64_t *labels, int32_t unc_type, int32_t T,
               const float *threshold, float beta, float *loss, float *v, float *sums, int32_t *counts, double *thresholds, float *coef,
               void *workspace, size_t workspace_bytes, bt_stream_t stream);
/* d loss / d logits as [S][B][C] times *grad_loss (one fp32 value in device memory), one launch of the row pass's shape, from the
 * logits, coef and the workspace of the bt_avu_fwd call. Thresholds and comparisons carry no gradient; the softmax is recomputed. */
int bt_avu_bwd(int32_t S, int32_t B, int32_t C, const float *logits, int32_t unc_type, int32_t T, const float *coef,
               const float *grad_loss, const void *workspace, size_t workspace_bytes, float *dlogits, bt_stream_t stream);

/* INT8 post-training-quantised Reparameterization layers (layers/variational_layers/quantize_linear_variational.py:115-224,
 * quantize_conv_variational.py:405-552) on v_mfma_i32_32x32x32_i8: one fused forward, bit for bit what torch's CPU quantised
 * operators give (integer accumulation has no order). With `1 / s` the fp32 reciprocal of the fp32 scale, every multiplication and
 * addition ONE fp32 rounding (but for the one fma of the output stage), rne = round to nearest even, and the quotient of scales of the
 * weight chain taken in double and rounded once; the output stage is fbgemm's, whose scales are rounded to fp32 FIRST:
 *   e   = clamp(rne(eps * (1 / s_eps)), -128, 127)
 *   p   = clamp(rne(float(q_sigma * e) * float(s_sigma * s_eps / s_mul)), -128, 127)
 *   w   = clamp(rne((float(p) * s_mul + float(q_mu) * s_mu) * (1 / s_add)), -128, 127)          the sampled int8 weight, never in HBM
 *   xq  = clamp(rne(x * (1 / s_in)) + z_in, 0, 255)                                             x is quantised where it is fetched
 *   acc = sum_k (xq - z_in) * w                                                                 int32; padding contributes 0
 *   b   = mu_b + sigma_b * eps_b          (mu_b NULL: no bias; sigma_b NULL: b = mu_b, a bias that came from BatchNorm folding)
 *   a   = float(s_in) * float(s_add),  m = a / float(s_out)                                     fp32 operations
 *   oq  = clamp(rne(fmaf(b, 1 / a, float(acc)) * m) + z_out, 0, 255)                            ONE rounding of b * (1 / a) + float(acc)
 *   out = float(oq - z_out) * s_out
 * The MFMA is signed x signed: the kernel feeds xq - 128 (padding: z_in - 128) and adds (128 - z_in) * sum_k w[s][co][k].
 * A (scale, zero point) pair; the five of a forward are the reference's eps, mul, add, in and out quantisers. */
typedef struct bt_q8_pair {
  double scale;       /* what q_scale() returns in the reference: a double */
  int32_t zero_point;
  int32_t reserved;
} bt_q8_pair;
typedef struct bt_q8_params {
  bt_q8_pair eps, mul, add, in, out;
  double s_mu, s_sigma;                   /* the scales of the two int8 parameter images */
  const int8_t *mu_packed, *sigma_packed; /* [Co][taps][Ci16] int8 (bt_q8_pack), Ci16 = Ci rounded up to a multiple of 16, padding 0 */
  const float *mu_b, *sigma_b;            /* fp32 [Co]; mu_b NULL: no bias (sigma_b is then ignored); sigma_b NULL: b = mu_b */
} bt_q8_params;
/* packed[(co * taps + t) * Ci16 + c] = natural[co][c][t] for both tensors (c >= Ci: 0). Once per conversion: the quantised
 * parameters are frozen. */
int bt_q8_pack(const int8_t *q_mu, const int8_t *q_sigma, int64_t Co, int64_t Ci, int64_t taps, int8_t *mu_packed, int8_t *sigma_packed,
               bt_stream_t stream);
/* The forward. x: fp32 [B][Ci][H][W] (sample s reads x + s * x_sample_stride; 0: one x for all samples). Draws: eps_w fp32
 * [S][Co][Ci][taps] (the weight's natural order) and eps_b [S][Co] are read, or eps_w NULL: both come from rng -- tensor 0 with
 * bt_rng_normal_fill's index rule e = (co * taps + t) * inner4 + c, tensor 1 for the bias, sample rng->sample0 + s -- so a launch fed
 * bt_rng_normal_fill's output gives the same bytes. out: fp32 [S][B][Co][Ho][Wo]; out_q: the u8 image oq in the same layout, or NULL.
 * BT_ERR_BAD_ARG before any launch: a null x / p / out / pack, a pack that is not 16-byte aligned, eps_w without eps_b when the bias
 * has a sigma, neither eps_w nor rng, a scale <= 0, an in or out zero point outside 0..255, an empty output. BT_ERR_UNSUPPORTED, nothing
 * launched: groups != 1, a nonzero eps, mul or add zero point, Ci * taps * 32640 >= 2^31 (the int32 accumulator's bound), S > 65535,
 * 2^31 or more output pixels, 2^40 or more elements of one sample's x, Co * taps * ceil(Ci / 4) > 2^32 (the draw stream's block index),
 * Co > 65535 * 64. */
int bt_q8_conv2d_fwd(const bt_conv2d_geom *g, int32_t S, const float *x, int64_t x_sample_stride, const bt_q8_params *p,
                     const float *eps_w, const float *eps_b, const bt_rng *rng, float *out, uint8_t *out_q, bt_stream_t stream);
/* Linear as the 1 x 1 map: x [B][In], out [S][B][Out], eps_w [S][Out][In]. */
int bt_q8_linear_fwd(int32_t B, int32_t In, int32_t Out, int32_t S, const float *x, int64_t x_sample_stride, const bt_q8_params *p,
                     const float *eps_w, const float *eps_b, const bt_rng *rng, float *out, uint8_t *out_q, bt_stream_t stream);

/* INT8 post-training-quantised Flipout layers (layers/flipout_layers/quantized_conv_flipout.py:257-514, quantized_linear_flipout.py
 * :119-261): both contractions of the Flipout estimator and the whole operator chain between them in ONE launch, bit for bit what the
 * chain of torch's CPU quantised operators gives. Ten (scale, zero point) pairs, in the order of the reference's ten-entry quant_dict:
 * eps, delta, in, mean, sign_in, sign_out, xp, pert, pert_signed, out. Conventions as above (one fp32 rounding per operation, rne);
 * requant is the output stage above (fbgemm's, ONE fma); sign_in / sign_out are +1 or -1:
 *   e    = clamp(rne(eps * (1 / s_eps)), -128, 127)
 *   d    = clamp(rne(float(q_sigma * e) * float(s_sigma * s_eps / s_delta)), -128, 127)        qint8 x qint8: the quotient in double
 *   xq   = clamp(rne(x * (1 / s_in)) + z_in, 0, 255)
 *   acc1 = sum_k (xq - z_in) * q_mu;   o1 = requant(acc1, mu_b; a = float(s_in) * float(s_mu)) -> (s_mean, z_mean)
 *   qsi  = clamp(rne(sign_in * (1 / s_si)) + z_si, 0, 255),   qso likewise from sign_out
 *   x'   = umul(xq, qsi -> xp)
 *   acc2 = sum_k (x' - z_xp) * d;      p  = requant(acc2, sigma_b * eps_b; a = float(s_xp) * float(s_delta)) -> (s_pert, z_pert)
 *   p'   = umul(p, qso -> pert_signed)
 *   oq   = uadd(o1, p' -> out),        out = float(oq - z_out) * s_out
 *   umul(a, b -> o) = clamp(rne(float((a - z_a) * (b - z_b)) * M) + z_o, 0, 255),  M = float(s_a) * float(s_b) * (1 / float(s_o)), fp32, left to right
 *   uadd(a, b -> o) = clamp(rne((fmaf(float(a), s_a, -(float(z_a) * s_a)) + fmaf(float(b), s_b, -(float(z_b) * s_b))) * (1 / s_o)) + z_o, 0, 255)
 * Padding contributes a real zero to both contractions. mu_b NULL: no bias on either path (sigma_b is then ignored); sigma_b NULL: the
 * perturbation path carries none (a bias that came from BatchNorm folding). */
typedef struct bt_q8_flip_params {
  bt_q8_pair eps, delta, in, mean, sign_in, sign_out, xp, pert, pert_signed, out;
  double s_mu, s_sigma;                   /* the scales of the two int8 parameter images */
  const int8_t *mu_packed, *sigma_packed; /* bt_q8_pack's */
  const float *mu_b, *sigma_b;            /* fp32 [Co] */
} bt_q8_flip_params;
/* The forward. x, x_sample_stride, out, out_q: as bt_q8_conv2d_fwd. A supplied draw is whole or absent: eps_w fp32 [S][Co][Ci][taps],
 * eps_b [S][Co] (needed when there is a sigma_b), sign_in fp32 [S][B][Ci][H][W] and sign_out fp32 [S][B][Co][Ho][Wo] -- a NEGATIVE value
 * means -1, anything else (+0, -0 and NaN included) +1 -- or all four NULL and rng: eps as above, the signs hash_sign of tensor 2's
 * (sign_in) and tensor 3's (sign_out) stream at the element's offset in ONE sample's tensor, sample rng->sample0 + s -- so a launch fed
 * bt_rng_normal_fill's and bt_rng_sign_fill's output gives the same bytes, and samples that share one x still get their own signs.
 * BT_ERR_BAD_ARG before any launch: a null x / p / out / pack, a pack that is not 16-byte aligned, neither eps_w nor rng, eps_w without
 * both sign tensors or a sign tensor without eps_w, eps_w without eps_b when the bias has a sigma, a scale <= 0, a zero point outside
 * 0..255 (all but eps and delta), a product of scales that underflows fp32, an empty output. BT_ERR_UNSUPPORTED, nothing launched:
 * groups != 1, a nonzero eps or delta zero point, Ci * taps * 32640 >= 2^31, 2^32 or more elements in one sample's x or output, and the
 * size limits of bt_q8_conv2d_fwd. */
int bt_q8_flip_conv2d_fwd(const bt_conv2d_geom *g, int32_t S, const float *x, int64_t x_sample_stride, const bt_q8_flip_params *p,
                          const float *eps_w, const float *eps_b, const float *sign_in, const float *sign_out, const bt_rng *rng,
                          float *out, uint8_t *out_q, bt_stream_t stream);
/* Linear as the 1 x 1 map: x [B][In], out [S][B][Out], eps_w [S][Out][In], sign_in [S][B][In], sign_out [S][B][Out]. */
int bt_q8_flip_linear_fwd(int32_t B, int32_t In, int32_t Out, int32_t S, const float *x, int64_t x_sample_stride,
                          const bt_q8_flip_params *p, const float *eps_w, const float *eps_b, const float *sign_in,
                          const float *sign_out, const bt_rng *rng, float *out, uint8_t *out_q, bt_stream_t stream);

/* Calibration of the INT8 layers: the seven MinMaxObservers of the reference's prepare() / calibrate / convert() flow
 * (conv_variational.py:331-337, :387-397), with the statistics kept on the device. A statistic is a (min, max) pair of fp32 values
 * that starts at (+inf, -inf); both calls MERGE into it (a call can only widen a pair), skip non-finite values and count them into
 * *nonfinite (uint32, device memory), write nothing else, allocate nothing and never synchronise with the host. The merge is one
 * integer vector atomic per statistic and workgroup on the value's bit pattern: the result does not depend on scheduling.
 *
 * bt_q8_observe_w, the weight side: mu, rho fp32 [rows][inner][taps] (the weight's natural order, n = rows * inner * taps elements, any
 * n, 4-byte alignment only), S samples of draws -- eps fp32 [S][n] in the same order, or eps NULL and rng: tensor 0's stream under
 * bt_rng_normal_fill's index rule, sample rng->sample0 + s --, coef fp32 [rows] or NULL (1): a per-output-channel factor, the folded
 * BatchNorm's weight / sqrt(running_var + eps). With sigma = log1p(exp(rho)) (the kernels' softplus) and every operation ONE fp32
 * rounding:  m = mu * coef,  q = sigma * coef,  t = q * eps,  w = m + t.  stats: fp32 [5][2], the ranges of q, m, eps, t, w -- the
 * reference's five qint8 stubs in its order (sigma, mu, eps, mul, add).
 * BT_ERR_BAD_ARG before any launch: a null mu / rho / stats / nonfinite, S < 1, rows / inner / taps < 1, both eps and rng or neither, a
 * pointer that is not 4-byte aligned. BT_ERR_UNSUPPORTED, nothing launched: S > 65535, n >= 2^40, inner * taps >= 2^31, rows * taps * ceil(inner / 4) > 2^32. */
int bt_q8_observe_w(const float *mu, const float *rho, const float *coef, int64_t rows, int64_t inner, int64_t taps, int32_t S,
                    const float *eps, const bt_rng *rng, float *stats, uint32_t *nonfinite, bt_stream_t stream);
/* The activation side: the ranges of up to BT_MINMAX_MAX_SEGS fp32 tensors (x, n elements, 4-byte alignment only), each merged into its
 * own pair dst[2], in one launch. BT_ERR_BAD_ARG before any launch: n_segs outside 1..4, a null segs / nonfinite / x / dst, n < 1, a
 * pointer that is not 4-byte aligned. */
#define BT_MINMAX_MAX_SEGS 4
typedef struct bt_minmax_seg {
  const float *x;
  int64_t n;
  float *dst; /* (min, max) */
} bt_minmax_seg;
int bt_minmax_update(int32_t n_segs, const bt_minmax_seg *segs, uint32_t *nonfinite, bt_stream_t stream);

/* Calibration of the INT8 Flipout layers: the activation-side observers of the reference's twelve-observer flow
 * (flipout_layers/conv_flipout.py:339-345, :419-434; linear_flipout.py:115-118, :178-191). The weight side (sigma, mu, eps, delta =
 * sigma * eps) is bt_q8_observe_w's rows 0..3 and the output bt_minmax_update's; the two launches below take the rest. Statistics,
 * merging, non-finite values, allocation and synchronisation: as above. Each statistic is its own (min, max) pair, fp32 [2].
 *
 * The observing two-contraction launch: bt_flipout_conv2d_fwd's / bt_flipout_linear_fwd's operands -- g, S, x, x_sample_stride, p (the
 * priors and the packed parameters are not read) and d: all draws supplied in the natural layouts (eps_w, eps_b when biased, sign_in,
 * sign_out; a NEGATIVE sign value means -1, anything else +1, and the +-1 that was used is what is observed) or none (eps from tensor
 * 0's stream, the bias draw from tensor 1's, the signs hash_sign of tensor 2's and 3's, exactly as the forward draws them) -- and an
 * optional per-output-channel coef[Co] / shift[Co], both or neither (absent: 1 and 0), the BatchNorm to be folded. For every output
 * element of all S samples, with sigma = log1p(exp(rho)), conv the layer's contraction (fp32 MFMA accumulation) and every other
 * operation ONE fp32 rounding:
 *   mean        = (conv(x, mu) + mu_b) * coef + shift
 *   pert        = (conv(x * sign_in, sigma * eps) + sigma_b * eps_b) * coef         (no bias: no bias terms)
 *   pert_signed = pert * sign_out
 * and the ranges of mean, pert, pert_signed and sign_out are merged into the four pairs. Nothing output-sized is written.
 * BT_ERR_BAD_ARG before any launch: what the Flipout forward refuses in these operands (null x / p / d / mu_w / rho_w, S < 1, a bad
 * geometry, some draws supplied and others not, coef without shift), a null pair or nonfinite, a pointer that is not 4-byte aligned,
 * bt_rng.flags != 0. BT_ERR_UNSUPPORTED, nothing launched: groups != 1, S > 65535, and the sizes the fp32 general kernel refuses (a
 * tensor of 2^30 elements or more, more than 128 taps). */
int bt_q8_flip_observe_conv2d(const bt_conv2d_geom *g, int32_t S, const float *x, int64_t x_sample_stride, const bt_params *p,
                              const bt_draws *d, const float *coef, const float *shift, float *mean_mm, float *pert_mm,
                              float *pert_signed_mm, float *sign_out_mm, uint32_t *nonfinite, bt_stream_t stream);
int bt_q8_flip_observe_linear(int32_t B, int32_t In, int32_t Out, int32_t S, const float *x, int64_t x_sample_stride,
                              const bt_params *p, const bt_draws *d, const float *coef, const float *shift, float *mean_mm,
                              float *pert_mm, float *pert_signed_mm, float *sign_out_mm, uint32_t *nonfinite, bt_stream_t stream);
/* The input-side sweep: x fp32, n elements per sample (sample s reads x + s * x_sample_stride; 0: one x for all samples, which still
 * get their own signs), 4-byte alignment only. sign_in fp32 [S][n] (negative: -1, anything else +1), or NULL and rng: hash_sign of
 * tensor 2's stream at the element's offset within ONE sample's tensor, sample rng->sample0 + s, as the forward indexes it. Merges the
 * ranges of x, sign_in and x * sign_in (one fp32 rounding). BT_ERR_BAD_ARG before any launch: a null x / pair / nonfinite, S < 1,
 * n < 1, a negative stride, both sign_in and rng or neither, a pointer that is not 4-byte aligned. BT_ERR_UNSUPPORTED, nothing
 * launched: S > 65535, n >= 2^32. */
int bt_q8_flip_observe_x(int64_t n, int32_t S, const float *x, int64_t x_sample_stride, const float *sign_in, const bt_rng *rng,
                         float *in_mm, float *sign_in_mm, float *xp_mm, uint32_t *nonfinite, bt_stream_t stream);

/* u8 activations between the INT8 layers. A quantised activation is a u8 image at one (scale, zero point)
 * pair in the CHANNEL-BLOCKED layout [N][CB][H][W][16], CB = ceil(C / 16): byte j of the 16-byte unit (n, cb, h, w) is channel 16 * cb + j
 * of pixel (h, w), and the bytes of channels >= C hold the zero point. [N][F] features are the same layout at H = W = 1 (rows padded to a
 * multiple of 16). Every blocked image must be 16-byte aligned.
 *
 * The forwards: bt_q8_conv2d_fwd / bt_q8_linear_fwd / bt_q8_flip_* with an x source and two destinations. x_kind BT_Q8_X_F32: x is fp32
 * [B][Ci][H][W], quantised at p->in where it is fetched, as there. BT_Q8_X_U8: x is the blocked image of [B][Ci][H][W] at the pair p->in
 * (the CALLER's pair of that image: nothing is requantised), x_sample_stride counts its bytes. out: fp32 [S][B][Co][Ho][Wo] or NULL;
 * out_blocked: the blocked image of [S * B][Co][Ho][Wo] at p->out, or NULL (then nothing u8 is written). The arithmetic, the draws and the
 * sign streams (indexed by the element's offset in the LOGICAL [B][Ci][H][W] / [B][Co][Ho][Wo]) are those of the entry points above,
 * bit for bit. BT_ERR_BAD_ARG before any launch, beside theirs: an x_kind that is neither, a null x, neither destination, a u8 x or an
 * out_blocked that is not 16-byte aligned, a u8 sample stride that is no multiple of 16. */
#define BT_Q8_X_F32 0
#define BT_Q8_X_U8 1
int bt_q8_conv2d_fwd_act(const bt_conv2d_geom *g, int32_t S, const void *x, int32_t x_kind, int64_t x_sample_stride, const bt_q8_params *p,
                         const float *eps_w, const float *eps_b, const bt_rng *rng, float *out, uint8_t *out_blocked, bt_stream_t stream);
int bt_q8_linear_fwd_act(int32_t B, int32_t In, int32_t Out, int32_t S, const void *x, int32_t x_kind, int64_t x_sample_stride,
                         const bt_q8_params *p, const float *eps_w, const float *eps_b, const bt_rng *rng, float *out, uint8_t *out_blocked,
                         bt_stream_t stream);
int bt_q8_flip_conv2d_fwd_act(const bt_conv2d_geom *g, int32_t S, const void *x, int32_t x_kind, int64_t x_sample_stride,
                              const bt_q8_flip_params *p, const float *eps_w, const float *eps_b, const float *sign_in,
                              const float *sign_out, const bt_rng *rng, float *out, uint8_t *out_blocked, bt_stream_t stream);
int bt_q8_flip_linear_fwd_act(int32_t B, int32_t In, int32_t Out, int32_t S, const void *x, int32_t x_kind, int64_t x_sample_stride,
                              const bt_q8_flip_params *p, const float *eps_w, const float *eps_b, const float *sign_in,
                              const float *sign_out, const bt_rng *rng, float *out, uint8_t *out_blocked, bt_stream_t stream);
/* The element-wise operators on blocked images: each ONE launch, no allocation, no host synchronisation; torch's CPU quantised
 * operators bit for bit (rne: round to nearest even; every operation one fp32 rounding but for the fma named). N, C, H, W: the logical
 * shape. BT_ERR_BAD_ARG before any launch: a null pointer, N / C / H / W < 1, a blocked image that is not 16-byte aligned, a scale <= 0
 * (or not finite), a zero point outside 0..255; BT_ERR_UNSUPPORTED: an image of 2^40 bytes or more.
 *   bt_q8_act_quantize    q = clamp(rne(x * (1 / s)) + z, 0, 255) of fp32 x [N][C][H][W] (quantize_per_tensor).
 *   bt_q8_act_dequantize  out fp32 [N][C][H][W] = float(q - z) * s.
 *   bt_q8_act_relu        out = max(q, z); out may be q (in place).
 *   bt_q8_act_add         quantized.add / add_relu of images a, b of ONE shape (the caller's shapes (N, C, H, W) of a and b are both
 *                         given: a mismatch is BT_ERR_BAD_ARG): clamp(rne((fmaf(float(a), s_a, -(float(z_a) * s_a)) + fmaf(float(b), s_b,
 *                         -(float(z_b) * s_b))) * (1 / s_o)) + z_o, 0, 255); relu != 0: the maximum of that and z_o.
 *   bt_q8_act_max_pool2d  the maximum of the levels over a kh x kw window (stride, padding; padding positions are ignored): out is the
 *                         blocked image of [N][C][Ho][Wo], Ho = (H + 2 ph - kh) / sh + 1. BT_ERR_BAD_ARG: kernel / stride < 1, padding < 0
 *                         or > half the kernel, an empty output.
 *   bt_q8_act_avg_pool    the global average pool to [N][C][1][1], at q's pair: clamp(rne(float(sum - z * n) * float(1 / n) + z), 0, 255),
 *                         n = H * W. BT_ERR_UNSUPPORTED: n >= 2^23.
 *   bt_q8_act_unblock     flatten: the blocked image of [N][C][H][W] -> the blocked image of [N][F], F = C * H * W in NCHW order (rows
 *                         padded with z to a multiple of 16). */
int bt_q8_act_quantize(const float *x, int64_t N, int64_t C, int64_t H, int64_t W, double scale, int32_t zero_point, uint8_t *q, bt_stream_t stream);
int bt_q8_act_dequantize(const uint8_t *q, int64_t N, int64_t C, int64_t H, int64_t W, double scale, int32_t zero_point, float *out,
                         bt_stream_t stream);
int bt_q8_act_relu(const uint8_t *q, int64_t N, int64_t C, int64_t H, int64_t W, int32_t zero_point, uint8_t *out, bt_stream_t stream);
int bt_q8_act_add(const uint8_t *a, const int64_t *a_shape, double s_a, int32_t z_a, const uint8_t *b, const int64_t *b_shape, double s_b,
                  int32_t z_b, double s_out, int32_t z_out, int32_t relu, uint8_t *out, bt_stream_t stream);
int bt_q8_act_max_pool2d(const uint8_t *q, int64_t N, int64_t C, int64_t H, int64_t W, int32_t kh, int32_t kw, int32_t sh, int32_t sw,
                         int32_t ph, int32_t pw, uint8_t *out, bt_stream_t stream);
int bt_q8_act_avg_pool(const uint8_t *q, int64_t N, int64_t C, int64_t H, int64_t W, int32_t zero_point, uint8_t *out, bt_stream_t stream);
int bt_q8_act_unblock(const uint8_t *q, int64_t N, int64_t C, int64_t H, int64_t W, int32_t zero_point, uint8_t *out, bt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BT_HIP_H */
