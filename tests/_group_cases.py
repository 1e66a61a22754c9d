"""Grouped and depthwise convolution rows shared by test_grouped_plan_host.py (CPU) and test_gpu_grouped.py (GPU).  A plain module:
no fixtures, no pytest hooks.

Every launch with at most four input channels PER GROUP goes to the stem ("quad") kernel whatever ``groups`` is, so that kernel is
the depthwise path.  ROWS holds the smallest shapes that still reach each kernel named beside them (a quad tile must be at least
75 % full: M = B * Ho * Wo >= 384), with the kernel family the host dispatch plans for them in the automatic mode
(Reparameterization, Flipout) and in f32 mode (BT_QUAD_SPW=1, S in {1, 3}, per-sample x).  The inputs are built so that a value
taken from a neighbouring group or channel cannot pass unnoticed: channel c of x is scaled by 1 + c / 4, every output channel has a
bias, a BatchNorm scale and a shift of its own, some of the scales negative."""
import ctypes as C
import os

import torch

# id: Ci, Co, groups, (kh, kw), stride, padding, dilation, H, W, B, family under Reparameterization / Flipout / f32 mode
_T = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _row(Ci, Co, groups, k, st, pd, dl, H, W, B, reparam, flipout, f32="fast"):
    return dict(Ci=Ci, Co=Co, groups=groups, k=_T(k), st=_T(st), pd=_T(pd), dl=_T(dl), H=H, W=W, B=B, reparam=reparam, flipout=flipout, f32=f32)


ROWS = {
    "dw3": _row(12, 12, 12, 3, 1, 1, 1, 8, 8, 8, "quad512", "quad256f"),                      # Cig 1, Cog 1: ONE live row of a 64-row tile
    "dw3-b2": _row(12, 12, 12, 3, 1, 1, 1, 8, 8, 2, "fast", "fast"),                          # M = 128: too small for a quad tile
    "dwx2s2": _row(6, 12, 6, 3, 2, 1, 1, 16, 16, 8, "quad512", "quad256f"),                   # channel multiplier 2, stride 2
    "cig4": _row(16, 24, 4, 3, 1, 1, 1, 8, 8, 8, "quad512", "fast"),                          # Cig 4: no padding channel left for Flipout's sign bits
    "cig2k5": _row(6, 9, 3, 5, 1, 2, 1, 8, 8, 8, "quad512", "quad256f"),                      # Cig 2, 25 taps
    "cig3rect": _row(6, 10, 2, (3, 2), (2, 1), (1, 0), (1, 2), 16, 10, 8, "quad512", "quad256f"),
    "oct-g8": _row(64, 64, 8, 3, 1, 1, 1, 8, 8, 16, "split128", "split128f"),                 # whole octets per group: the general split kernel
    "cig12": _row(48, 40, 4, 3, 1, 1, 1, 8, 8, 16, "fast", "fast"),                           # Cig 12: neither quads nor octets
    "dw4x4": _row(12, 12, 12, 3, 1, 1, 1, 4, 4, 32, "quad512", "quad256f"),                   # 32 / 16 images per tile
    "dw2x2": _row(12, 12, 12, 3, 1, 1, 1, 2, 2, 128, "fast", "fast"),                         # pixel-major
    "dw1d": _row(8, 8, 8, (1, 5), 1, (0, 2), 1, 1, 64, 8, "quad512", "quad256f"),             # a depthwise Conv1d's launch
    "dw70": _row(70, 70, 70, 3, 1, 1, 1, 8, 8, 8, "quad512", "quad256f"),                     # 70 groups
    "dw7x7": _row(6, 6, 6, 7, 1, 3, 1, 16, 16, 2, "quad512", "quad256f"),                     # 49 taps
    "cog2": _row(64, 128, 64, 3, 1, 1, 1, 8, 8, 8, "quad512", "quad256f"),                    # Cig 1, Cog 2, 64 groups
    "cog70": _row(8, 140, 2, 3, 1, 1, 1, 8, 8, 8, "quad512", "fast"),                         # two channel tiles per group, the second with 6 live rows
}

_PREFIX = {
    "quad512": "fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=0",
    "quad256f": "fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=0",
    "split128": "fused_split_kernel<64,128,bf16x3,6 terms,",
    "split128f": "fused_split_kernel<64,128,bf16x3,2x6 terms,flip,",
    "fast": "fused_fast_kernel<",
    "fwd": "fused_fwd_kernel<",
}
GUARD_ROWS = ("dw3", "cog70", "dw70")       # one live row in 64, a partial second channel tile, 70 groups
GUARD_OFF1 = "fast"       # x, parameters and result 4 bytes past a 16-byte boundary: no vector access is left, the fp32 fast kernel takes every row
SPLIT_FAMILIES = ("quad512", "quad256f", "split128", "split128f")      # the bf16x3 kernels: held to the (K + 8) * 2^-24 bound


def family(name):
    """The family of ROWS' columns a kernel name belongs to (None: none of them).  The bf16 mode's twins (``bf16x1,1 terms``) count as
    the family of the tile they share."""
    n = name.replace("bf16x1,1 terms", "bf16x3,6 terms")
    for fam, pre in _PREFIX.items():
        if n.startswith(pre):
            return fam
    return None


def want_family(rid, flip, mode=0):
    """The table's cell: mode 0 automatic, 1 f32, 3 bf16 (Reparameterization: the automatic mode's tile; Flipout: untouched)."""
    r = ROWS[rid]
    return r["f32"] if mode == 1 else (r["flipout"] if flip else r["reparam"])


def conv_of(r):
    return dict(stride=r["st"], padding=r["pd"], dilation=r["dl"], groups=r["groups"])


def out_hw(r):
    Ho = (r["H"] + 2 * r["pd"][0] - r["dl"][0] * (r["k"][0] - 1) - 1) // r["st"][0] + 1
    Wo = (r["W"] + 2 * r["pd"][1] - r["dl"][1] * (r["k"][1] - 1) - 1) // r["st"][1] + 1
    return Ho, Wo


def k_len(r):
    """Products per output element: Cig * kh * kw."""
    return (r["Ci"] // r["groups"]) * r["k"][0] * r["k"][1]


_INPUTS = {}


def inputs(rid, S=3):
    """The row's CPU tensors, built once and never modified: mu, rho, mb, rb, x [S * B, ...] (x[:B] is the shared input), the
    BatchNorm constants sc / sh and a residual res [S * B, Co, Ho, Wo]."""
    key = (rid, S)
    if key in _INPUTS:
        return _INPUTS[key]
    r = ROWS[rid]
    g = torch.Generator().manual_seed(4000 + list(ROWS).index(rid))
    Ci, Co, Cig = r["Ci"], r["Co"], r["Ci"] // r["groups"]
    mu = torch.randn(Co, Cig, *r["k"], generator=g) * 0.1
    rho = torch.randn(Co, Cig, *r["k"], generator=g) * 0.1 - 3
    co = torch.arange(Co, dtype=torch.float32)
    mb = torch.randn(Co, generator=g) * 0.1 + 0.05 * (co % 11 - 5)          # a bias of its own per output channel
    rb = torch.randn(Co, generator=g) * 0.1 - 3
    x = torch.randn(S * r["B"], Ci, r["H"], r["W"], generator=g) * (1 + torch.arange(Ci, dtype=torch.float32) / 4).view(1, -1, 1, 1)
    sc = (0.5 + torch.rand(Co, generator=g)) * torch.where(co % 3 == 1, -1.0, 1.0)      # every third scale negative
    sh = torch.randn(Co, generator=g) * 0.3 + 0.02 * co
    Ho, Wo = out_hw(r)
    res = torch.randn(S * r["B"], Co, Ho, Wo, generator=g)
    _INPUTS[key] = dict(mu=mu, rho=rho, mb=mb, rb=rb, x=x.contiguous(), sc=sc, sh=sh, res=res, conv=conv_of(r), B=r["B"])
    return _INPUTS[key]


def oracle64(flip, t, xs, d, s, absolute=False):
    """Sample s of the fp64 oracle (oracle/bt_oracle.py on float64 tensors) on the draws ``d`` (eps_w, eps_b[, sign_in, sign_out], each
    [S, ...]).  ``absolute``: the magnitude conv(|x|, |W_s|) + |b_s| instead (Flipout: the sum over both contractions)."""
    from oracle import bt_oracle as O
    D = lambda v: None if v is None else v.double()
    mu, mb = D(t["mu"]), D(t["mb"])
    dw = O.softplus_ref(D(t["rho"])) * D(d["eps_w"][s])
    db = None if mb is None else O.softplus_ref(D(t["rb"])) * D(d["eps_b"][s])
    x = D(xs)
    if absolute:
        if flip:
            return O._contract(x.abs(), mu.abs() + dw.abs(), None if mb is None else mb.abs() + db.abs(), t["conv"])
        return O._contract(x.abs(), (mu + dw).abs(), None if mb is None else (mb + db).abs(), t["conv"])
    if flip:
        return O._contract(x, mu, mb, t["conv"]) + O._contract(x * D(d["sign_in"][s]), dw, db, t["conv"]) * D(d["sign_out"][s])
    return O._contract(x, mu + dw, None if mb is None else mb + db, t["conv"])


def host_draws(rid, flip, S=1, seed=9):
    """Seeded draws for the CPU tests (the GPU tests replay the on-chip ones)."""
    r, t = ROWS[rid], inputs(rid)
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_hw(r)
    d = dict(eps_w=torch.randn((S,) + tuple(t["mu"].shape), generator=g), eps_b=torch.randn(S, r["Co"], generator=g))
    if flip:
        sgn = lambda *s: torch.randint(0, 2, s, generator=g).float() * 2 - 1
        d.update(sign_in=sgn(S, r["B"], r["Ci"], r["H"], r["W"]), sign_out=sgn(S, r["B"], r["Co"], Ho, Wo))
    return d


# ------------------------------------------------------------------------------------------------------------------ the plan-only seam
P = 0x10000000          # any non-null, 16-byte aligned address: never dereferenced on the host


def plan(rid, flip, mode, S, per_sample=True, off=0):
    """The row's forward through ``bt_debug_plan_only`` (as tools/record_split_plans.py drives it) -> (return code, kernel name).
    ``off``: x, the parameters and the result start 4 * off bytes past a 16-byte boundary (the packs stay aligned)."""
    from bayesian_torch_amd import _lib
    m, L, h = _lib, _lib.lib(), C.CDLL(_lib.LIB_PATH)      # the bt_debug_* hooks are outside include/bt_hip.h
    r = ROWS[rid] if isinstance(rid, str) else rid      # (or a geometry of the same keys)
    geom = m.bt_conv2d_geom(r["B"], r["Ci"], r["H"], r["W"], r["Co"], r["k"][0], r["k"][1], r["st"][0], r["st"][1], r["pd"][0], r["pd"][1],
                            r["dl"][0], r["dl"][1], r["groups"])
    Q = P + 4 * off
    par = m.bt_params(Q, Q, Q, Q, P, P, P, P, P, P, 0, 0)
    draws = m.bt_draws(None, None, None, None, m.bt_rng(1, None, 0, 1, 0, 0))
    ws_bytes = m.WORKSPACE_BYTES + int(L.bt_fused_scratch_bytes(C.byref(geom), S))
    fn = L.bt_flipout_conv2d_fwd if flip else L.bt_reparam_conv2d_fwd
    before, spw = L.bt_get_contraction(), os.environ.get("BT_QUAD_SPW")
    os.environ["BT_QUAD_SPW"] = "1"     # the stems' sample walk is planned from the device's CU count: keep the one-sample path
    h.bt_debug_plan_only(1)
    try:
        assert L.bt_set_contraction(mode) == 0
        rc = fn(C.byref(geom), S, Q, r["B"] * r["Ci"] * r["H"] * r["W"] if per_sample else 0, C.byref(par), C.byref(draws), None, Q, P, P, ws_bytes, None)
    finally:
        h.bt_debug_plan_only(0)
        L.bt_set_contraction(before)
        if spw is None:
            del os.environ["BT_QUAD_SPW"]
        else:
            os.environ["BT_QUAD_SPW"] = spw
    return rc, (L.bt_last_kernel_name().decode() if rc == 0 else L.bt_last_error_string().decode())
