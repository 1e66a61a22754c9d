"""ctypes binding of libbtorch_hip.so (include/bt_hip.h).

The library is the product: there is NO Python/ATen fallback. If the shared
object is missing or a tensor is not on a HIP device, calls raise.
"""
import ctypes as C
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BT_LIB_PATH") or os.path.join(_HERE, "libbtorch_hip.so")   # BT_LIB_PATH: a diagnostic build (tools/stamps.py)
WORKSPACE_BYTES = 65536
KL_MAX_SEGMENTS = 64
PACK_MAX_SEGMENTS = 64
KL_RHO_IS_SIGMA = 1
KL_PRIOR_LAPLACE = 2
PRIOR_NORMAL, PRIOR_LAPLACE = 0, 1
DRAWS_EPS_PACKED = 1   # bt_rng.flags: eps_w holds [S] packed images (bt_pack_eps)
LOWRANK_MAX_R = 4      # BT_LOWRANK_MAX_R: ranks the fused forward multiplies in registers (above: the bt_lowrank_mean pre-pass)
DRAWS_SIGNS_PACKED = 2  # bt_rng.flags: sign_in / sign_out hold [S] byte images (bt_pack_signs); Flipout, with DRAWS_EPS_PACKED


def signs_packed_stride(n):
    """BT_SIGNS_PACKED_STRIDE: bytes of one sample's image of n signs."""
    return (int(n) + 15) // 16 * 16

_f32p = C.POINTER(C.c_float)
_vp = C.c_void_p


class bt_rng(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("call_base_dev", _vp), ("call", C.c_uint32), ("layer_id", C.c_uint32),
                ("sample0", C.c_uint32), ("flags", C.c_uint32)]


class bt_params(C.Structure):
    _fields_ = [(n, _vp) for n in ("mu_w", "rho_w", "mu_b", "rho_b", "prior_mu_w", "prior_sigma_w", "prior_mu_b", "prior_sigma_b", "mu_packed", "sigma_packed")] \
        + [("prior_kind", C.c_int32), ("reserved", C.c_int32)]


class bt_draws(C.Structure):
    _fields_ = [("eps_w", _vp), ("eps_b", _vp), ("sign_in", _vp), ("sign_out", _vp), ("rng", bt_rng)]


class bt_epilogue(C.Structure):
    _fields_ = [("scale", _vp), ("shift", _vp), ("residual", _vp), ("residual_sample_stride", C.c_int64), ("relu", C.c_int32),
                ("pool", C.c_int32)]


class bt_pack_seg(C.Structure):
    _fields_ = [(n, _vp) for n in ("mu_w", "rho_w", "src_mu", "src_rho", "mu_packed", "sigma_packed", "state")] \
        + [("Co", C.c_int64), ("Ci", C.c_int64), ("taps", C.c_int64), ("force", C.c_int32), ("reserved", C.c_int32)]


class bt_pack_kl(C.Structure):
    _fields_ = [(n, _vp) for n in ("prior_mu_w", "prior_sigma_w", "mu_b", "rho_b", "prior_mu_b", "prior_sigma_b", "kl_out")] \
        + [("n_bias", C.c_int64)]


class bt_conv2d_geom(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "Ci", "H", "W", "Co", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw", "groups")]


class bt_chain_member(C.Structure):
    _fields_ = [("g", C.POINTER(bt_conv2d_geom)), ("x", _vp), ("x_sample_stride", C.c_int64), ("p", C.POINTER(bt_params)), ("d", C.POINTER(bt_draws)),
                ("ep", C.POINTER(bt_epilogue)), ("out", _vp), ("kl_out", _vp)]


CHAIN_MAX = 4          # BT_CHAIN_MAX
CHAIN_DECLINED = 1     # BT_CHAIN_DECLINED: bt_reparam_conv2d_chain_fwd launched nothing -- the members are not a chain


class bt_updil(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("uh", "uw", "lo_h", "hi_h", "lo_w", "hi_w")]


class bt_dwin(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kd", "D", "sd", "dd", "pd")]


class bt_q8_pair(C.Structure):
    _fields_ = [("scale", C.c_double), ("zero_point", C.c_int32), ("reserved", C.c_int32)]


class bt_q8_params(C.Structure):
    _fields_ = [(n, bt_q8_pair) for n in ("eps", "mul", "add", "inp", "out")] + [("s_mu", C.c_double), ("s_sigma", C.c_double)] \
        + [(n, _vp) for n in ("mu_packed", "sigma_packed", "mu_b", "sigma_b")]


class bt_q8_flip_params(C.Structure):
    _fields_ = [(n, bt_q8_pair) for n in ("eps", "delta", "inp", "mean", "sign_in", "sign_out", "xp", "pert", "pert_signed", "out")] \
        + [("s_mu", C.c_double), ("s_sigma", C.c_double)] + [(n, _vp) for n in ("mu_packed", "sigma_packed", "mu_b", "sigma_b")]


class bt_minmax_seg(C.Structure):
    _fields_ = [("x", _vp), ("n", C.c_int64), ("dst", _vp)]


MINMAX_MAX_SEGS = 4    # BT_MINMAX_MAX_SEGS

_lib = None
_lock = threading.Lock()

_FWD_TAIL = [_vp, C.c_int64, C.POINTER(bt_params), C.POINTER(bt_draws), C.POINTER(bt_epilogue), _vp, _vp, _vp, C.c_size_t, _vp]
_PROTOS = {
    "bt_version": (C.c_int, []),
    "bt_last_error_string": (C.c_char_p, []),
    "bt_last_kernel_name": (C.c_char_p, []),
    "bt_last_launch_info": (C.c_int, [C.POINTER(C.c_int64), C.c_int32]),
    "bt_fused_scratch_bytes": (C.c_size_t, [C.POINTER(bt_conv2d_geom), C.c_int32]),
    "bt_set_contraction": (C.c_int, [C.c_int]),
    "bt_get_contraction": (C.c_int, []),
    "bt_conv2d_bwd_workspace": (C.c_size_t, [C.POINTER(bt_conv2d_geom), C.c_int32]),
    "bt_conv2d_bwd": (C.c_int, [C.POINTER(bt_conv2d_geom), C.c_int32, C.c_int32, _vp, C.c_int64, _vp, C.POINTER(bt_params), C.POINTER(bt_draws),
                                _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "bt_maxpool_3x3s2": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, _vp]),
    "bt_conv2d_bwd_kl": (C.c_int, [C.POINTER(bt_conv2d_geom), C.c_int32, C.c_int32, _vp, C.c_int64, _vp, C.POINTER(bt_params), C.POINTER(bt_draws), _vp,
                                   _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "bt_kl_normal_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_uint32, _vp, _vp, _vp]),
    "bt_kl_normal_bwd_segs": (C.c_int, [C.c_int32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int64), _vp, C.c_uint32,
                                        C.POINTER(_vp), C.POINTER(_vp), _vp]),
    "bt_reparam_linear_fwd": (C.c_int, [C.c_int32] * 4 + _FWD_TAIL),
    "bt_flipout_linear_fwd": (C.c_int, [C.c_int32] * 4 + _FWD_TAIL),
    "bt_reparam_conv2d_fwd": (C.c_int, [C.POINTER(bt_conv2d_geom), C.c_int32] + _FWD_TAIL),
    "bt_flipout_conv2d_fwd": (C.c_int, [C.POINTER(bt_conv2d_geom), C.c_int32] + _FWD_TAIL),
    "bt_reparam_conv2d_chain_fwd": (C.c_int, [C.c_int32, C.POINTER(bt_chain_member), C.c_int32, _vp]),
    "bt_reparam_conv2d_updil_fwd": (C.c_int, [C.POINTER(bt_conv2d_geom), C.POINTER(bt_updil), C.c_int32] + _FWD_TAIL),
    "bt_flipout_conv2d_updil_fwd": (C.c_int, [C.POINTER(bt_conv2d_geom), C.POINTER(bt_updil), C.c_int32] + _FWD_TAIL),
    "bt_reparam_conv2d_dwin_fwd": (C.c_int, [C.POINTER(bt_conv2d_geom), C.POINTER(bt_dwin), C.c_int32] + _FWD_TAIL),
    "bt_flipout_conv2d_dwin_fwd": (C.c_int, [C.POINTER(bt_conv2d_geom), C.POINTER(bt_dwin), C.c_int32] + _FWD_TAIL),
    "bt_kl_normal": (C.c_int, [C.c_int32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int64),
                               C.POINTER(C.c_int32), C.c_uint32, _vp, _vp, C.c_size_t, _vp]),
    "bt_pack_sync": (C.c_int, [C.c_int32, C.POINTER(bt_pack_seg), _vp, C.c_size_t, _vp]),
    "bt_pack_sync_kl": (C.c_int, [C.c_int32, C.POINTER(bt_pack_seg), C.POINTER(bt_pack_kl), _vp, C.c_size_t, _vp]),
    "bt_pack_params": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, _vp, _vp, _vp]),
    "bt_pack_eps": (C.c_int, [_vp, C.c_int32, C.c_int64, C.c_int64, C.c_int64, _vp, _vp]),
    "bt_pack_signs": (C.c_int, [_vp, C.c_int32, C.c_int64, _vp, _vp, _vp]),
    "bt_rng_normal_fill": (C.c_int, [C.POINTER(bt_rng), C.c_uint32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, _vp, _vp]),
    "bt_rng_sign_fill": (C.c_int, [C.POINTER(bt_rng), C.c_uint32, C.c_int32, C.c_int64, _vp, _vp]),
    "bt_rng_philox_raw": (C.c_int, [C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "bt_mc_epilogue": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "bt_lowrank_conv2d_fwd": (C.c_int, [C.POINTER(bt_conv2d_geom), C.c_int32, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int32, C.c_float, _vp, _vp, C.POINTER(bt_rng),
                                        C.POINTER(bt_epilogue), _vp, _vp]),
    "bt_lowrank_mean": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, _vp, C.POINTER(bt_rng), _vp, _vp]),
    "bt_kl_lowrank_workspace": (C.c_size_t, [C.c_int64, C.c_int32]),
    "bt_kl_lowrank": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.c_float, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "bt_lowrank_conv2d_bwd_workspace": (C.c_size_t, [C.POINTER(bt_conv2d_geom), C.c_int32, C.c_int32]),
    "bt_lowrank_conv2d_bwd": (C.c_int, [C.POINTER(bt_conv2d_geom), C.c_int32, _vp, C.c_int64, _vp, _vp, C.c_int64, _vp, C.c_int32, C.c_float, _vp, C.POINTER(bt_rng), _vp,
                                        _vp, _vp, _vp, C.c_size_t, _vp]),
    "bt_lowrank_conv2d_bwd_info": (C.c_int, [C.POINTER(C.c_int64), C.c_int32]),
    "bt_lowrank_wgrad_finish": (C.c_int, [_vp, C.c_int64, C.c_int32, C.c_int32, _vp, C.POINTER(bt_rng), _vp, _vp, _vp]),
    "bt_kl_lowrank_bwd_workspace": (C.c_size_t, [C.c_int64, C.c_int32]),
    "bt_kl_lowrank_bwd": (C.c_int, [_vp, _vp, C.c_int64, C.c_int32, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "bt_lstm_cell_fwd": (C.c_int, [C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, C.c_int64, _vp, _vp]),
    "bt_lstm_cell_bwd": (C.c_int, [C.c_int64, C.c_int64, _vp, _vp, C.c_int64, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int64, _vp, _vp, _vp]),
    "bt_avu_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "bt_avu_fwd": (C.c_int, [C.c_int32] * 3 + [_vp, _vp, C.c_int32, C.c_int32, _vp, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "bt_avu_bwd": (C.c_int, [C.c_int32] * 3 + [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "bt_kl_hier": (C.c_int, [C.c_int32] + [C.POINTER(_vp)] * 7 + [C.POINTER(C.c_int64), C.POINTER(C.c_int32), _vp, _vp, _vp, C.c_size_t, _vp]),
    "bt_kl_hier_bwd": (C.c_int, [C.c_int32] + [C.POINTER(_vp)] * 7 + [C.POINTER(C.c_int64), _vp] + [C.POINTER(_vp)] * 4 + [_vp]),
    "bt_special_eval": (C.c_int, [C.c_int32, _f32p, C.c_int64, _f32p]),
    "bt_q8_pack": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, _vp, _vp, _vp]),
    "bt_q8_conv2d_fwd": (C.c_int, [C.POINTER(bt_conv2d_geom), C.c_int32, _vp, C.c_int64, C.POINTER(bt_q8_params), _vp, _vp, C.POINTER(bt_rng), _vp, _vp, _vp]),
    "bt_q8_linear_fwd": (C.c_int, [C.c_int32] * 4 + [_vp, C.c_int64, C.POINTER(bt_q8_params), _vp, _vp, C.POINTER(bt_rng), _vp, _vp, _vp]),
    "bt_q8_flip_conv2d_fwd": (C.c_int, [C.POINTER(bt_conv2d_geom), C.c_int32, _vp, C.c_int64, C.POINTER(bt_q8_flip_params), _vp, _vp, _vp, _vp, C.POINTER(bt_rng), _vp, _vp,
                                       _vp]),
    "bt_q8_flip_linear_fwd": (C.c_int, [C.c_int32] * 4 + [_vp, C.c_int64, C.POINTER(bt_q8_flip_params), _vp, _vp, _vp, _vp, C.POINTER(bt_rng), _vp, _vp, _vp]),
    "bt_q8_observe_w": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _vp, C.POINTER(bt_rng), _vp, _vp, _vp]),
    "bt_minmax_update": (C.c_int, [C.c_int32, C.POINTER(bt_minmax_seg), _vp, _vp]),
    "bt_q8_flip_observe_conv2d": (C.c_int, [C.POINTER(bt_conv2d_geom), C.c_int32, _vp, C.c_int64, C.POINTER(bt_params), C.POINTER(bt_draws)] + [_vp] * 8),
    "bt_q8_flip_observe_linear": (C.c_int, [C.c_int32] * 4 + [_vp, C.c_int64, C.POINTER(bt_params), C.POINTER(bt_draws)] + [_vp] * 8),
    "bt_q8_flip_observe_x": (C.c_int, [C.c_int64, C.c_int32, _vp, C.c_int64, _vp, C.POINTER(bt_rng)] + [_vp] * 5),
    # u8 activations between the INT8 layers (csrc/bt_q8_act.hip and the *_act forwards): x, x_kind, x_sample_stride, ..., out, out_blocked
    "bt_q8_conv2d_fwd_act": (C.c_int, [C.POINTER(bt_conv2d_geom), C.c_int32, _vp, C.c_int32, C.c_int64, C.POINTER(bt_q8_params), _vp, _vp, C.POINTER(bt_rng), _vp, _vp,
                                      _vp]),
    "bt_q8_linear_fwd_act": (C.c_int, [C.c_int32] * 4 + [_vp, C.c_int32, C.c_int64, C.POINTER(bt_q8_params), _vp, _vp, C.POINTER(bt_rng), _vp, _vp, _vp]),
    "bt_q8_flip_conv2d_fwd_act": (C.c_int, [C.POINTER(bt_conv2d_geom), C.c_int32, _vp, C.c_int32, C.c_int64, C.POINTER(bt_q8_flip_params), _vp, _vp, _vp, _vp,
                                           C.POINTER(bt_rng), _vp, _vp, _vp]),
    "bt_q8_flip_linear_fwd_act": (C.c_int, [C.c_int32] * 4 + [_vp, C.c_int32, C.c_int64, C.POINTER(bt_q8_flip_params), _vp, _vp, _vp, _vp, C.POINTER(bt_rng), _vp, _vp,
                                           _vp]),
    "bt_q8_act_quantize": (C.c_int, [_vp] + [C.c_int64] * 4 + [C.c_double, C.c_int32, _vp, _vp]),
    "bt_q8_act_dequantize": (C.c_int, [_vp] + [C.c_int64] * 4 + [C.c_double, C.c_int32, _vp, _vp]),
    "bt_q8_act_relu": (C.c_int, [_vp] + [C.c_int64] * 4 + [C.c_int32, _vp, _vp]),
    "bt_q8_act_add": (C.c_int, [_vp, C.POINTER(C.c_int64), C.c_double, C.c_int32, _vp, C.POINTER(C.c_int64), C.c_double, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                               _vp, _vp]),
    "bt_q8_act_max_pool2d": (C.c_int, [_vp] + [C.c_int64] * 4 + [C.c_int32] * 6 + [_vp, _vp]),
    "bt_q8_act_avg_pool": (C.c_int, [_vp] + [C.c_int64] * 4 + [C.c_int32, _vp, _vp]),
    "bt_q8_act_unblock": (C.c_int, [_vp] + [C.c_int64] * 4 + [C.c_int32, _vp, _vp]),
}
EXPORTS = tuple(_PROTOS)
Q8_X_F32, Q8_X_U8 = 0, 1      # BT_Q8_X_F32, BT_Q8_X_U8


def lib():
    """The loaded library. Raises (loudly) when it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"{LIB_PATH} is missing: the HIP extension is the only implementation of this path "
                        "(no CPU/ATen fallback). Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "or `make -C bayesian_torch_amd/csrc`.")
                handle = C.CDLL(LIB_PATH)
                for name, (res, args) in _PROTOS.items():
                    fn = getattr(handle, name)
                    fn.restype, fn.argtypes = res, args
                _lib = handle
    return _lib


LAUNCH_INFO_FIELDS = ("workgroups", "m_tiles", "n_tiles", "S", "t_NI", "t_R", "t_Wt", "pixel_major", "row_tiles", "kl_slices", "groups", "n_bt", "n_rt", "n_ct", "fused_kl")


def last_launch_info():
    """Tile geometry of the calling thread's last fused-forward launch (bt_last_launch_info) as a dict."""
    v = (C.c_int64 * 16)()
    check(lib().bt_last_launch_info(v, 16))
    return dict(zip(LAUNCH_INFO_FIELDS, (int(x) for x in v)))


LOWRANK_BWD_INFO_FIELDS = ("dgrad_launches", "wgrad_launches", "dgrad_pieces", "wgrad_chunks", "dgrid_x", "dgrid_y", "dgrid_z", "wgrid_x", "wgrid_y", "wgrid_z")


def lowrank_bwd_info():
    """What the calling thread's last bt_lowrank_conv2d_bwd planned (bt_lowrank_conv2d_bwd_info) as a dict."""
    v = (C.c_int64 * 10)()
    check(lib().bt_lowrank_conv2d_bwd_info(v, 10))
    return dict(zip(LOWRANK_BWD_INFO_FIELDS, (int(x) for x in v)))


ERR_UNSUPPORTED = -2  # BT_ERR_UNSUPPORTED


def check(rc):
    if rc != 0:
        raise RuntimeError(f"libbtorch_hip error {rc}: {lib().bt_last_error_string().decode()}")


def ptr(t):
    return None if t is None else t.data_ptr()


def dev_f32(t, what):
    """Validate a tensor handed to the kernels: fp32, contiguous, on a HIP device."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{what} is on {t.device}: bayesian_torch_amd runs on a HIP (MI355X) device only; "
                           "there is no CPU implementation of this path")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def stream_ptr(device=None):
    """The current torch stream OF ``device`` (not of whatever device happens to be current)."""
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)     # the handle without a Stream object (the eager path asks twice per layer)
    if raw is not None and isinstance(device, torch.device) and device.index is not None:
        return raw(device.index)
    return torch.cuda.current_stream(device).cuda_stream


def on(device):
    """Context for a C-ABI launch on tensors of ``device``: the kernels launch on HIP's current device, so make the
    tensors' device current for the call (a model on cuda:1 while cuda:0 is current would otherwise run on GPU 0
    against GPU 1's memory, on a stream that orders nothing)."""
    return torch.cuda.device(device)


_ws = {}
_ws_retired = []


def workspace(key, device, scratch=0):
    """One zero-initialised BT_WORKSPACE_BYTES buffer per (owner, device); kernels leave it zeroed. ``scratch`` more bytes behind it
    (bt_fused_scratch_bytes: the split-K forwards' slabs; contents never matter) -- the buffer grows when a call asks for more."""
    k = (key, device.index if device.index is not None else torch.cuda.current_device())
    w = _ws.get(k)
    need = WORKSPACE_BYTES + ((int(scratch) + 255) // 256) * 256
    if w is None or w.numel() < need:
        if w is not None:
            _ws_retired.append(w)    # (a captured graph may still hold the smaller buffer's address)
        w = torch.zeros(need, dtype=torch.uint8, device=device)
        _ws[k] = w
    return w


def seg_chunks(segments, prepare, layer_ids=None):
    """What the segmented entry points take, per chunk of KL_MAX_SEGMENTS segments. prepare(index, segment) -> the segment's validated
    tensors in the C ABI's order (None: a null entry; the first one gives numel). Yields (index of the chunk's first segment, n, the
    prepared rows -- hold them until the call is made --, one pointer array per position, the numel array, the layer array or None)."""
    for c0 in range(0, len(segments), KL_MAX_SEGMENTS):
        rows = [prepare(c0 + i, seg) for i, seg in enumerate(segments[c0:c0 + KL_MAX_SEGMENTS])]
        n = len(rows)
        arrs = [(_vp * n)(*col) for col in zip(*[[None if t is None else t.data_ptr() for t in r] for r in rows])]
        numel = (C.c_int64 * n)(*[r[0].numel() for r in rows])
        lay = None if layer_ids is None else (C.c_int32 * n)(*layer_ids[c0:c0 + n])
        yield c0, n, rows, arrs, numel, lay


def _kl_segment(_, seg):
    ts = [dev_f32(t, "kl segment tensor") for t in seg]
    if not all(t.numel() == ts[0].numel() for t in ts):
        raise ValueError("kl segment tensors must have equal numel")
    return ts


def _kl_hier_segment(i, seg):
    if len(seg) != 7:
        raise ValueError("a hierarchical KL segment is (mu, rho, prior_mu, log_a, log_b, a0, b0)")
    return _kl_segment(i, seg)


def kl_normal(segments, layer_ids=None, rho_is_sigma=False, out=None, owner="kl", laplace=False):
    """segments: list of (mu, rho, prior_mu, prior_sigma) device tensors. Returns a 0-dim tensor:
    sum over layers of (sum over the layer's segments of the element mean).  laplace: kl_div's 'laplace' branch for
    every segment (the prior tensors are not read, as in the reference)."""
    L = lib()
    dev = segments[0][0].device
    total = None
    for _, n, keep, arrs, numel, lay in seg_chunks(segments, _kl_segment, layer_ids):
        res = torch.empty((), dtype=torch.float32, device=dev) if (out is None or total is not None) else out
        with on(dev):
            check(L.bt_kl_normal(n, arrs[0], arrs[1], arrs[2], arrs[3], numel, lay, (KL_RHO_IS_SIGMA if rho_is_sigma else 0) | (KL_PRIOR_LAPLACE if laplace else 0),
                                 res.data_ptr(), workspace(owner, dev).data_ptr(), WORKSPACE_BYTES, stream_ptr(dev)))
        total = res if total is None else total + res
    return total


def kl_hier(segs, layer_ids=None, owner="kl_hier", per_segment=False):
    """segs: list of (mu, rho, prior_mu, log_a, log_b, a0, b0) device tensors of equal numel: the hierarchical layers' kl_loss()
    (bt_kl_hier: the SUM over the elements). Returns a 0-dim tensor: sum over layers of (sum over the layer's segments), one launch
    per KL_MAX_SEGMENTS segments; per_segment: also a [len(segs)] tensor of every segment's own fp32 sum."""
    L = lib()
    dev = segs[0][0].device
    total = None
    seg_sums = torch.empty(len(segs), dtype=torch.float32, device=dev) if per_segment else None
    for c0, n, keep, arrs, numel, lay in seg_chunks(segs, _kl_hier_segment, layer_ids):
        res = torch.empty((), dtype=torch.float32, device=dev)
        so = None if seg_sums is None else seg_sums.data_ptr() + 4 * c0
        with on(dev):
            check(L.bt_kl_hier(n, *arrs, numel, lay, res.data_ptr(), so, workspace(owner, dev).data_ptr(), WORKSPACE_BYTES, stream_ptr(dev)))
        total = res if total is None else total + res
    return (total, seg_sums) if per_segment else total


SPECIAL_DIGAMMA, SPECIAL_TRIGAMMA, SPECIAL_LGAMMA, SPECIAL_X_TRIGAMMA_M1 = 0, 1, 2, 3


def special_eval(kind, x):
    """The kernels' fp32 special functions evaluated on the CPU (bt_special_eval): x a CPU float32 tensor of positive values."""
    x = x.detach().to(torch.float32).contiguous()
    if x.is_cuda:
        raise RuntimeError("special_eval is the host-side check of the special functions: it takes a CPU tensor")
    out = torch.empty_like(x)
    check(lib().bt_special_eval(int(kind), C.cast(x.data_ptr(), _f32p), x.numel(), C.cast(out.data_ptr(), _f32p)))
    return out
