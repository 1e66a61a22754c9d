"""Functional form of the four fused forwards, of their backward and of the LSTM cell: tensors in, C-ABI calls, tensors out.  The layer modules
(layers/_fused.py, _family.py) add the MC frame, the call coordinates, the pack check and the KL wiring on top of ``fused_forward``."""
import ctypes as C
import math

import torch

from . import _lib, rng


def conv_out_hw(H, W, kh, kw, sh, sw, ph, pw, dh, dw):
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def fused_forward(x, mu_w, rho_w, mu_b=None, rho_b=None, *, pool=False, **kw):
    """See _fused_forward.  pool=True appends MaxPool2d(3, 2, 1) to the output stage (the ResNet stem): fused into the
    launch when its tiles hold whole output images, else run as a separate pooling pass on the launch's output."""
    if not pool:
        return _fused_forward(x, mu_w, rho_w, mu_b, rho_b, pool=False, **kw)
    r = _fused_forward(x, mu_w, rho_w, mu_b, rho_b, pool=True, **kw)
    if r is None:  # BT_ERR_UNSUPPORTED: nothing was launched
        out, kl = _fused_forward(x, mu_w, rho_w, mu_b, rho_b, pool=False, **kw)
        return maxpool_3x3s2(out), kl
    return r


def maxpool_3x3s2(x):
    """MaxPool2d(3, 2, 1) of an NCHW tensor on the HIP pooling pass (bt_maxpool_3x3s2): the same bits as torch's max_pool2d."""
    x = _lib.dev_f32(x, "input")
    N, Cc, H, W = x.shape
    out = torch.empty((N, Cc, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    with _lib.on(x.device):
        _lib.check(_lib.lib().bt_maxpool_3x3s2(x.data_ptr(), out.data_ptr(), N * Cc, H, W, _lib.stream_ptr(x.device)))
    return out


def _geometry(x, mu_w, conv, S, shared_x):
    """-> (B, the launch's bt_conv2d_geom -- Linear as the 1 x 1 convolution --, one sample's x elements, the contraction's output tail).
    An input-dilated conv (``conv["updil"]``): the geom holds x's own dims and no padding, the tail is the virtual image's output.
    A depth-window conv (``conv["dwin"]`` = (kd, D, sd, dd, pd)): x is the real [B, Ci * D, H, W]; B and the geom are the launch's over
    the virtual operand (B * Do images of Ci * kd channels), x elements the real ones."""
    per = 1 if shared_x else S
    if x.shape[0] % per:
        raise RuntimeError("stacked input rows are not a multiple of S")
    B, Co = x.shape[0] // per, mu_w.shape[0]
    if conv is None:
        In = mu_w.shape[1]
        if x.dim() != 2 or x.shape[1] != In:
            raise RuntimeError(f"expected [N, {In}] input, got {tuple(x.shape)}")
        return B, _lib.bt_conv2d_geom(B, In, 1, 1, Co, 1, 1, 1, 1, 0, 0, 1, 1, 1), x.numel() // per, (Co,)
    kh, kw = mu_w.shape[2], mu_w.shape[3]
    (sh, sw), (ph, pw), (dh, dw), groups = conv["stride"], conv["padding"], conv["dilation"], conv["groups"]
    Ci, H, W = x.shape[1], x.shape[2], x.shape[3]
    if conv.get("dwin") is not None:        # the virtual operand of bt_*_conv2d_dwin_fwd
        if conv.get("updil") is not None:
            raise RuntimeError("a conv takes a depth window or an input dilation, not both")
        dw_ = tuple(conv["dwin"])
        if len(dw_) != 5 or any(int(v) != v for v in dw_):
            raise RuntimeError("dwin is (kd, D, sd, dd, pd), five integers")
        kd, D, sd, dd, pd = dw_
        if min(kd, D, sd, dd) < 1 or pd < 0 or Ci % D:
            raise RuntimeError("a depth-window conv takes kd, D, sd, dd >= 1, pd >= 0 and x as [B, Ci * D, H, W]")
        Do = (D + 2 * pd - dd * (kd - 1) - 1) // sd + 1
        if D + 2 * pd - dd * (kd - 1) - 1 < 0 or Do < 1:
            raise RuntimeError("convolution output would be empty")
        B, Ci = B * Do, Ci // D * kd
    if Ci != mu_w.shape[1] * groups:
        raise RuntimeError(f"input has {Ci} channels, weight expects {mu_w.shape[1] * groups}")
    Hv, Wv = H, W
    if conv.get("updil") is not None:       # the virtual image of bt_*_conv2d_updil_fwd
        (uh, uw), (lo_h, hi_h, lo_w, hi_w) = conv["updil"], conv["pads"]
        if (ph, pw) != (0, 0) or min(uh, uw) < 1 or min(lo_h, hi_h, lo_w, hi_w) < 0:
            raise RuntimeError("an input-dilated conv takes dilation >= 1, explicit pads >= 0 and padding (0, 0)")
        Hv, Wv = (H - 1) * uh + 1 + lo_h + hi_h, (W - 1) * uw + 1 + lo_w + hi_w
    Ho, Wo = conv_out_hw(Hv, Wv, kh, kw, sh, sw, ph, pw, dh, dw)
    if Ho <= 0 or Wo <= 0:
        raise RuntimeError("convolution output would be empty")
    return B, _lib.bt_conv2d_geom(B, Ci, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, groups), x.numel() // per, (Co, Ho, Wo)


def _split_inject_wanted(tens, flip, S, x_elems, n_so, inject_path, state, geo_key):
    """Injected draws on the split-precision kernels: packed parameters and a whole draw (eps_b exactly when biased; Flipout: both sign
    tensors, Reparameterization: none), of a geometry the caller's state does not remember as declined."""
    ok = ((rng.get_inject_path() if inject_path is None else inject_path) == "split" and tens["eps_w"] is not None
          and tens["mu_packed"] is not None and tens["eps_w"].numel() == S * tens["mu_w"].numel()
          and (tens["mu_b"] is None) == (tens["eps_b"] is None))
    if ok and flip:
        ok = (tens["sign_in"] is not None and tens["sign_out"] is not None and tens["sign_in"].numel() == S * x_elems
              and tens["sign_out"].numel() == S * n_so)
    elif ok:
        ok = tens["sign_in"] is None and tens["sign_out"] is None
    return ok and not (state is not None and geo_key in state.setdefault("declined", set()))


def _pack_supplied_draw(tens, flip, S, x_elems, n_so, R, state):
    """Re-lay a whole supplied draw for the split-precision kernels (bt_pack_eps; Flipout: + two bt_pack_signs) -> the packed bt_draws.
    The buffers are the caller's state's ("buf", "sign_in_buf", "sign_out_buf", "sign_count"), made again only when too small."""
    L, mu_w = _lib.lib(), tens["mu_w"]
    dev, st = mu_w.device, {} if state is None else state

    def buffer(key, n, dtype):
        buf = st.get(key)
        if buf is None or buf.numel() < n or buf.device != dev:
            buf = st[key] = torch.empty(n, dtype=dtype, device=dev)
        return buf

    Co, Cig, taps = mu_w.shape[0], mu_w.shape[1], mu_w[0, 0].numel()
    eps_pk = buffer("buf", S * Co * taps * ((Cig + 3) // 4 * 4), torch.float32)
    with _lib.on(dev):
        _lib.check(L.bt_pack_eps(tens["eps_w"].data_ptr(), S, Co, Cig, taps, eps_pk.data_ptr(), _lib.stream_ptr(dev)))
    sg_pk = [None, None]
    if flip:      # the two sign tensors as byte images; the pass leaves its count of elements that are not +-1 in the state's counter
        cnt = st.get("sign_count")
        if cnt is None or cnt.device != dev:
            cnt = st["sign_count"] = torch.zeros(2, dtype=torch.int32, device=dev)
        for i, (key, n) in enumerate((("sign_in", x_elems), ("sign_out", n_so))):
            sg_pk[i] = buffer(key + "_buf", S * _lib.signs_packed_stride(n), torch.uint8)
            with _lib.on(dev):
                _lib.check(L.bt_pack_signs(tens[key].data_ptr(), S, n, sg_pk[i].data_ptr(), cnt.data_ptr() + 4 * i, _lib.stream_ptr(dev)))
    Rp = _lib.bt_rng(R.seed, R.call_base_dev, R.call, R.layer_id, R.sample0, _lib.DRAWS_EPS_PACKED | (_lib.DRAWS_SIGNS_PACKED if flip else 0))
    return _lib.bt_draws(eps_pk.data_ptr(), _lib.ptr(tens["eps_b"]), _lib.ptr(sg_pk[0]), _lib.ptr(sg_pk[1]), Rp)


def _epilogue(tens, out, S, relu, pool):
    """The fused output stage as a bt_epilogue reference, or None when the launch has none."""
    ep = _epilogue_struct(tens, out, S, relu, pool)
    return None if ep is None else C.byref(ep)


def _epilogue_struct(tens, out, S, relu, pool):
    scale, shift, res = tens["post_scale"], tens["post_shift"], tens["residual"]
    if scale is None and res is None and not relu and not pool:
        return None
    rstride, Co = 0, out.shape[1]
    if res is not None:
        if res.numel() == out.numel():
            rstride = out.numel() // S
        elif res.numel() * S != out.numel():
            raise RuntimeError(f"residual has {res.numel()} elements, out has {out.numel()} (S={S})")
    if scale is not None and (scale.numel() != Co or shift is None or shift.numel() != Co):
        raise RuntimeError("post_scale / post_shift must both have Co elements")
    return _lib.bt_epilogue(_lib.ptr(scale), _lib.ptr(shift), _lib.ptr(res), rstride, 1 if relu else 0, 1 if pool else 0)


def _f32_on(dev, tens):
    """Every tensor of the dict ``tens`` becomes contiguous fp32 (``_lib.dev_f32``; None stays None); one on another device than ``dev`` raises."""
    for k, t in tens.items():
        t = _lib.dev_f32(t, k)
        if t is not None and t.device != dev:
            raise RuntimeError(f"{k} on {t.device} but input on {dev}")
        tens[k] = t


def _fused_forward(x, mu_w, rho_w, mu_b=None, rho_b=None, *, flip=False, conv=None, S=1, shared_x=True,
                   priors=None, eps_w=None, eps_b=None, sign_in=None, sign_out=None,
                   seed=0, call=0, layer_id=0, sample0=0, call_base=None, want_kl=False, workspace_owner="functional",
                   post_scale=None, post_shift=None, residual=None, relu=False, packed=None, pool=False, prior_type="normal",
                   inject_path=None, eps_pack_state=None):
    """x: [B, In] (conv=None) or [B, Ci, H, W]; when ``shared_x`` is False x holds S stacked batches
    ([S*B, ...]).  conv: dict(stride=(sh,sw), padding=(ph,pw), dilation=(dh,dw), groups=g) for Conv2d.
    With ``updil=(uh, uw)`` and ``pads=(lo_h, hi_h, lo_w, hi_w)`` in it (padding (0, 0)), x is convolved as the input-dilated, explicitly
    padded image it stands for (bt_*_conv2d_updil_fwd: a transposed convolution without the upsampled copy); on-chip draws only, and a
    launch the library declines (BT_ERR_UNSUPPORTED, nothing launched) returns None instead of a result.
    With ``dwin=(kd, D, sd, dd, pd)`` in it, x is the real input of a Conv3d as [B, Ci * D, H, W] (a view of [B, Ci, D, H, W]) and mu_w
    the [Co, (Ci / g) * kd, kh, kw] kernel: the launch convolves the depth-unfolded operand without materialising it
    (bt_*_conv2d_dwin_fwd) and returns out [S * B * Do, Co, Ho, Wo]; on-chip draws only, None when the library declines.
    priors: (prior_mu_w, prior_sigma_w, prior_mu_b, prior_sigma_b) -- required when want_kl.
    eps_*/sign_*: injected draws with a leading S axis, or None for the on-chip generators.
    post_scale/post_shift [Co], residual ([S*B, ...] like out, or [B, ...] shared), relu: fused output stage
    (v*scale+shift, +residual, max(.,0)).  packed: (mu_packed, sigma_packed) from pack_params() -- selects the fast kernel.
    prior_type: "normal" | "laplace" (kl_div's branch; only matters when want_kl).
    inject_path: "general" | "split" | None (= rng.get_inject_path()): with "split", a whole injected draw (eps_w, eps_b exactly when
    biased, for Flipout both sign tensors of the right sizes; packed given) is re-laid by bt_pack_eps (Flipout: + two bt_pack_signs)
    and read by the split-precision kernels; a launch they decline (BT_ERR_UNSUPPORTED, nothing launched) runs as under "general".
    Supplied Flipout signs on this path are +1 / -1: an exact 0 is read as +1 and counted (include/bt_hip.h).
    eps_pack_state: a dict the caller owns (a layer keeps one: the buffers live and die with it) holding the packed-draw buffers
    ("buf", Flipout: "sign_in_buf" / "sign_out_buf"), the geometries that were declined, so that neither is made again on every
    call, and for Flipout "sign_count": an int32 device tensor [2] = the sign_in / sign_out elements of the last packed draw that were
    not exactly +1 or -1 (reading it synchronises; nothing here does).
    Returns (out [S*B, ...], kl or None)."""
    x = _lib.dev_f32(x, "input")
    dev = x.device
    tens = dict(mu_w=mu_w, rho_w=rho_w, mu_b=mu_b, rho_b=rho_b, eps_w=eps_w, eps_b=eps_b, sign_in=sign_in, sign_out=sign_out,
                post_scale=post_scale, post_shift=post_shift, residual=residual, mu_packed=None if packed is None else packed[0],
                sigma_packed=None if packed is None else packed[1])
    _f32_on(dev, tens)
    B, geom, x_elems, tail = _geometry(x, mu_w, conv, S, shared_x)
    n_so = B * math.prod(tail)      # one sample's contraction output, before any fused pooling
    if pool:
        if conv is None or residual is not None:
            raise RuntimeError("pool=True needs a Conv2d launch without residual")
        tail = (tail[0], (tail[1] - 1) // 2 + 1, (tail[2] - 1) // 2 + 1)
    out = torch.empty((S * B,) + tail, dtype=torch.float32, device=dev)
    kl = ws = None
    pr = [None] * 4
    L = _lib.lib()
    geo_key = (B, S, bool(shared_x), tuple(x.shape[1:]), None if conv is None else (*conv["stride"], *conv["padding"], *conv["dilation"], conv["groups"]),
               bool(pool), residual is not None)
    updil = None
    if conv is not None and conv.get("updil") is not None:
        updil = _lib.bt_updil(*conv["updil"], *conv["pads"])
        geo_key += (tuple(conv["updil"]), tuple(conv["pads"]))
    dwin = None
    if conv is not None and conv.get("dwin") is not None:
        dwin = _lib.bt_dwin(*(int(v) for v in conv["dwin"]))
        geo_key += (("dwin",) + tuple(conv["dwin"]),)
    split_inj = updil is None and dwin is None and _split_inject_wanted(tens, flip, S, x_elems, n_so, inject_path, eps_pack_state, geo_key)
    # layers whose output map is one pixel may run split over K-slices that meet in scratch behind the workspace (include/bt_hip.h)
    scratch = int(L.bt_fused_scratch_bytes(C.byref(geom), S)) if ((eps_w is None or split_inj) and not flip and packed is not None and updil is None and dwin is None) else 0
    if want_kl:
        if priors is None:
            raise ValueError("want_kl needs priors")
        pr = [_lib.dev_f32(t, "prior") for t in priors]
        kl = torch.empty((), dtype=torch.float32, device=dev)
    if scratch or want_kl:
        ws = _lib.workspace(workspace_owner, dev, scratch)
    P = _lib.bt_params(tens["mu_w"].data_ptr(), tens["rho_w"].data_ptr(), _lib.ptr(tens["mu_b"]), _lib.ptr(tens["rho_b"]),
                       _lib.ptr(pr[0]), _lib.ptr(pr[1]), _lib.ptr(pr[2]), _lib.ptr(pr[3]), _lib.ptr(tens["mu_packed"]), _lib.ptr(tens["sigma_packed"]),
                       _lib.PRIOR_LAPLACE if prior_type == "laplace" else _lib.PRIOR_NORMAL, 0)
    R = _rng(seed, call, layer_id, sample0, call_base)
    D = D_nat = _lib.bt_draws(_lib.ptr(tens["eps_w"]), _lib.ptr(tens["eps_b"]), _lib.ptr(tens["sign_in"]), _lib.ptr(tens["sign_out"]), R)
    if split_inj:
        D = _pack_supplied_draw(tens, flip, S, x_elems, n_so, R, eps_pack_state)
    E = _epilogue(tens, out, S, relu, pool)

    def launch(draws):
        tail_args = (x.data_ptr(), 0 if shared_x else x_elems, C.byref(P), C.byref(draws), E, out.data_ptr(), _lib.ptr(kl), _lib.ptr(ws),
                     ws.numel() if ws is not None else 0, _lib.stream_ptr(dev))
        if conv is None:
            fn = L.bt_flipout_linear_fwd if flip else L.bt_reparam_linear_fwd
            return fn(B, geom.Ci, geom.Co, S, *tail_args)
        if updil is not None:
            fn = L.bt_flipout_conv2d_updil_fwd if flip else L.bt_reparam_conv2d_updil_fwd
            return fn(C.byref(geom), C.byref(updil), S, *tail_args)
        if dwin is not None:
            fn = L.bt_flipout_conv2d_dwin_fwd if flip else L.bt_reparam_conv2d_dwin_fwd
            return fn(C.byref(geom), C.byref(dwin), S, *tail_args)
        fn = L.bt_flipout_conv2d_fwd if flip else L.bt_reparam_conv2d_fwd
        return fn(C.byref(geom), S, *tail_args)

    with _lib.on(dev):
        rc = launch(D)
        if split_inj and rc == _lib.ERR_UNSUPPORTED:      # nothing was launched: the natural layout on the general kernel, as under "general"
            if eps_pack_state is not None:
                eps_pack_state["declined"].add(geo_key)
            rc = launch(D_nat)
        if (pool or updil is not None or dwin is not None) and rc == _lib.ERR_UNSUPPORTED:
            return None
        _lib.check(rc)
    return out, kl


def fused_chain_forward(x, members, *, S=1, shared_x=True, outs=None):
    """A chain of Conv2dReparameterization layers of one shape as ONE launch (bt_reparam_conv2d_chain_fwd): member k + 1 convolves what
    member k wrote. x: the chain's input, [B, Ci, H, W] or S stacked batches (``shared_x`` False). members: dicts, in execution order, of
    what ``fused_forward`` takes per layer -- mu_w, rho_w, conv, packed=(mu_packed, sigma_packed), seed, call, layer_id, and optionally
    mu_b, rho_b, sample0, call_base, post_scale, post_shift, relu, residual. A member's residual is None, a tensor, the string "input"
    (the chain's input) or the index of an EARLIER member (that member's out). On-chip draws only; no KL (the pack check produces it).
    outs: the result tensors to write ([S * B, Co, Ho, Wo] each), else fresh ones.
    Returns the members' outs, bit for bit what the calls one by one give -- or None when the library declines (the shapes are not a
    chain it runs): nothing was launched, and the caller makes the calls."""
    x = _lib.dev_f32(x, "input")
    dev, L = x.device, _lib.lib()
    if not 1 <= len(members) <= _lib.CHAIN_MAX:
        return None
    # What the library's planner refuses from the shapes alone (split_chain_plan: one 64-channel tile, groups 1, stride 1, a window larger
    # than 1x1, whole images of at most 512 positions in a tile) is refused here, BEFORE any result is allocated: a stage of large maps
    # never holds n full activations for a chain that cannot be. What is left to the library -- the tile split_plan picks, alignment,
    # overlap -- is decided with the results allocated; forward_chain remembers a refusal, so that happens once.
    if outs is None:
        for m in members:
            w, cv = m["mu_w"], m["conv"]
            if (w.dim() != 4 or w.shape[0] > 64 or cv["groups"] != 1 or tuple(cv["stride"]) != (1, 1) or tuple(w.shape[2:]) == (1, 1) or x.dim() != 4
                    or math.prod(conv_out_hw(x.shape[2], x.shape[3], w.shape[2], w.shape[3], *cv["stride"], *cv["padding"], *cv["dilation"])) > 512):
                return None
    arr = (_lib.bt_chain_member * len(members))()
    keep, res_outs, cur, cur_shared = [], [], x, shared_x
    for k, m in enumerate(members):
        res = m.get("residual")
        if isinstance(res, str):
            if res != "input":
                raise ValueError("a member's residual is None, a tensor, \"input\" or an earlier member's index")
            res = x
        elif isinstance(res, int) and not isinstance(res, bool):
            if not 0 <= res < k:
                raise ValueError("a member's residual index names an EARLIER member")
            res = res_outs[res]
        tens = dict(mu_w=m["mu_w"], rho_w=m["rho_w"], mu_b=m.get("mu_b"), rho_b=m.get("rho_b"), post_scale=m.get("post_scale"), post_shift=m.get("post_shift"),
                    residual=res, mu_packed=m["packed"][0], sigma_packed=m["packed"][1])
        _f32_on(dev, tens)
        B, geom, x_elems, tail = _geometry(cur, tens["mu_w"], m["conv"], S, cur_shared)
        if m["conv"].get("updil") is not None or m["conv"].get("dwin") is not None:
            return None
        out = torch.empty((S * B,) + tail, dtype=torch.float32, device=dev) if outs is None else outs[k]
        P = _lib.bt_params(tens["mu_w"].data_ptr(), tens["rho_w"].data_ptr(), _lib.ptr(tens["mu_b"]), _lib.ptr(tens["rho_b"]), None, None, None, None,
                           tens["mu_packed"].data_ptr(), tens["sigma_packed"].data_ptr(), _lib.PRIOR_NORMAL, 0)
        D = _lib.bt_draws(None, None, None, None, _rng(m["seed"], m["call"], m["layer_id"], m.get("sample0", 0), m.get("call_base")))
        E = _epilogue_struct(tens, out, S, bool(m.get("relu")), False)
        ep = C.pointer(E) if E is not None else None
        arr[k] = _lib.bt_chain_member(C.pointer(geom), cur.data_ptr(), 0 if cur_shared else x_elems, C.pointer(P), C.pointer(D), ep, out.data_ptr(), None)
        keep.append((tens, geom, P, D, E, cur))
        res_outs.append(out)
        cur, cur_shared = out, False
    with _lib.on(dev):
        rc = L.bt_reparam_conv2d_chain_fwd(len(members), arr, S, _lib.stream_ptr(dev))
    if rc == _lib.CHAIN_DECLINED:
        return None
    _lib.check(rc)
    return res_outs


def _rng(seed, call, layer_id, sample0, call_base):
    return _lib.bt_rng(int(seed) & 0xFFFFFFFFFFFFFFFF, _lib.ptr(call_base), int(call) & 0xFFFFFFFF, int(layer_id), int(sample0), 0)


def rng_fill_normal(seed, call, layer_id, sample0, tensor_id, S, shape, device, call_base=None):
    """Materialise the on-chip eps stream of a weight ([Co, Ci/g, kh, kw] or [Out, In]) or bias ([Co]) tensor
    -> [S, *shape].  The stream is tap-major (include/bt_hip.h), the returned tensor is in natural order."""
    shape = tuple(shape)
    rows, inner = (shape[0], shape[1]) if len(shape) > 1 else (1, shape[0])   # a vector is one row (bias: block co >> 2)
    taps = 1
    for d in shape[2:]:
        taps *= d
    out = torch.empty((S,) + shape, dtype=torch.float32, device=device)
    R = _rng(seed, call, layer_id, sample0, call_base)
    with _lib.on(out.device):
        _lib.check(_lib.lib().bt_rng_normal_fill(C.byref(R), tensor_id, S, rows, inner, taps, out.data_ptr(), _lib.stream_ptr(out.device)))
    return out


def rng_fill_sign(seed, call, layer_id, sample0, tensor_id, S, shape, device, call_base=None):
    """Materialise the on-chip Flipout sign stream (tensor_id 2: sign_in over one sample's x, 3: sign_out) -> [S, *shape]."""
    shape = tuple(shape)
    n = 1
    for d in shape:
        n *= d
    out = torch.empty((S,) + shape, dtype=torch.float32, device=device)
    R = _rng(seed, call, layer_id, sample0, call_base)
    with _lib.on(out.device):
        _lib.check(_lib.lib().bt_rng_sign_fill(C.byref(R), tensor_id, S, n, out.data_ptr(), _lib.stream_ptr(out.device)))
    return out


def lowrank_mean(mu, L, S, z=None, *, seed=0, call=0, layer_id=0, sample0=0, call_base=None, out=None):
    """The mean pre-pass of a low-rank layer whose rank exceeds the fused forward's in-kernel bound (bt_lowrank_mean):
    m[s] = mu + L @ z_s as one fp32 chain per element, j ascending -> [S, n]. z: [S, r], or None for the on-chip stream (tensor 4 of
    the call's coordinates). out: a contiguous fp32 [S, n] device tensor to write into (a layer's workspace), made when None."""
    mu, L, z = _lib.dev_f32(mu, "mu"), _lib.dev_f32(L, "L"), _lib.dev_f32(z, "z")
    n, r = L.shape
    if mu.numel() != n or (z is not None and tuple(z.shape) != (S, r)):
        raise RuntimeError(f"lowrank_mean: mu [{mu.numel()}], L {tuple(L.shape)}, z {None if z is None else tuple(z.shape)} do not fit S={S}")
    if out is None:
        out = torch.empty((S, n), dtype=torch.float32, device=mu.device)
    elif tuple(out.shape) != (S, n) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != mu.device:
        raise RuntimeError("lowrank_mean: out must be a contiguous fp32 [S, n] tensor on mu's device")
    R = _rng(seed, call, layer_id, sample0, call_base)
    with _lib.on(mu.device):
        _lib.check(_lib.lib().bt_lowrank_mean(mu.data_ptr(), L.data_ptr(), n, r, S, _lib.ptr(z), C.byref(R), out.data_ptr(), _lib.stream_ptr(mu.device)))
    return out


def lowrank_conv2d(x, mean, L, d, wshape, conv, *, S=1, shared_x=True, z=None, eps_w=None, seed=0, call=0, layer_id=0, sample0=0, call_base=None):
    """The fused forward with a low-rank multivariate weight source (bt_lowrank_conv2d_fwd): sample s convolves x with
    w_s = mean_s + L @ z_s + sqrt(d) * eps_s, formed on chip. mean: [n] (one for all samples) or [S, n] (lowrank_mean's output);
    L: [n, R] with R <= _lib.LOWRANK_MAX_R, or None (R = 0); d: the constant diagonal (a float > 0); wshape = (Co, Ci, kh, kw), n its
    product; conv as in fused_forward (groups 1). z [S, R] and eps_w [S, n]: both supplied, or both None for the on-chip streams.
    -> out [S * B, Co, Ho, Wo]."""
    x, mean, L = _lib.dev_f32(x, "input"), _lib.dev_f32(mean, "mean"), _lib.dev_f32(L, "L")
    z, eps_w = _lib.dev_f32(z, "z"), _lib.dev_f32(eps_w, "eps_w")
    dev = x.device
    wshape = tuple(int(v) for v in wshape)
    n = math.prod(wshape)
    R = 0 if L is None else L.shape[1]
    if mean.numel() not in (n, S * n) or (L is not None and L.shape[0] != n):
        raise RuntimeError(f"lowrank_conv2d: mean [{mean.numel()}] / L do not fit a kernel of {n} weights and S={S}")
    if (eps_w is not None and R > 0 and z is None) or (eps_w is None and z is not None):
        raise RuntimeError("lowrank_conv2d: supply both draws (z, eps_w) or neither")
    if eps_w is not None and (eps_w.numel() != S * n or (R > 0 and tuple(z.shape) != (S, R))):
        raise RuntimeError(f"lowrank_conv2d: the supplied draws do not hold S={S} samples")
    B, geom, x_elems, tail = _geometry(x, _Shape(wshape), conv, S, shared_x)
    out = torch.empty((S * B,) + tail, dtype=torch.float32, device=dev)
    Rg = _rng(seed, call, layer_id, sample0, call_base)
    with _lib.on(dev):
        _lib.check(_lib.lib().bt_lowrank_conv2d_fwd(C.byref(geom), S, x.data_ptr(), 0 if shared_x else x_elems, mean.data_ptr(), n if mean.numel() == S * n and S > 1 else 0,
                                                    _lib.ptr(L), R, float(d), _lib.ptr(z) if R > 0 else None, _lib.ptr(eps_w), C.byref(Rg), None, out.data_ptr(),
                                                    _lib.stream_ptr(dev)))
    return out


class _Shape:
    """What ``_geometry`` reads of a weight tensor: its shape."""

    def __init__(self, shape):
        self.shape = tuple(shape)


def kl_lowrank(mu, L, d, prior_mean, prior_var, owner="kl_lowrank", bad_pivots=None):
    """KL( N(mu, L L^T + d I) || N(prior_mean, diag(prior_var)) ) on the HIP kernels (bt_kl_lowrank: an fp64 sweep and an r x r fp64
    Cholesky, two launches, nothing synchronised) -> fp32 device tensor [2] = (KL, KL / n). bad_pivots: an int32 device tensor [1]
    that counts the calls whose factorisation met a pivot that was not positive (their result is NaN), or None."""
    mu, L = _lib.dev_f32(mu, "mu"), _lib.dev_f32(L, "L")
    pm, pv = _lib.dev_f32(prior_mean, "prior_mean"), _lib.dev_f32(prior_var, "prior_var")
    n, r = L.shape
    if mu.numel() != n or pm.numel() != n or pv.numel() != n:
        raise RuntimeError("kl_lowrank: mu, prior_mean and prior_var must have L's row count")
    lib = _lib.lib()
    need = int(lib.bt_kl_lowrank_workspace(n, r))
    if need == 0:
        raise NotImplementedError(f"kl_lowrank: rank {r} is above the factorisation kernel's limit")
    ws = _lib.workspace((owner, "kl_lowrank"), mu.device, need)
    out = torch.empty((2,), dtype=torch.float32, device=mu.device)
    with _lib.on(mu.device):
        _lib.check(lib.bt_kl_lowrank(mu.data_ptr(), L.data_ptr(), n, r, float(d), pm.data_ptr(), pv.data_ptr(), out.data_ptr(), _lib.ptr(bad_pivots),
                                     ws.data_ptr() + _lib.WORKSPACE_BYTES, ws.numel() - _lib.WORKSPACE_BYTES, _lib.stream_ptr(mu.device)))
    return out


def lowrank_backward(x, grad_out, mean, L, d, wshape, conv, *, S=1, shared_x=True, need_x=True, need_w=True, z=None, eps_w=None, seed=0, call=0, layer_id=0,
                     sample0=0, call_base=None):
    """Gradients of ``lowrank_conv2d`` on the HIP backward kernels (bt_lowrank_conv2d_bwd): the data gradient regenerates
    w_s = mean_s + L @ z_s + sqrt(d) * eps_s per LDS stage from the forward's RNG coordinates (or reads the supplied draws); the weight
    gradient is kept per sample. The arguments are ``lowrank_conv2d``'s (mean [n] or [S, n], L [n, R] with R <= _lib.LOWRANK_MAX_R or
    None), x / grad_out as the forward saw / produced them. -> (dx like x or None -- summed over the samples for a shared x --,
    dW [S, n] or None: feed it to ``lowrank_wgrad_finish``, launch record of the call as a dict)."""
    x, g = _lib.dev_f32(x, "input"), _lib.dev_f32(grad_out, "grad_out")
    mean, L = _lib.dev_f32(mean, "mean"), _lib.dev_f32(L, "L")
    z, eps_w = _lib.dev_f32(z, "z"), _lib.dev_f32(eps_w, "eps_w")
    dev = x.device
    wshape = tuple(int(v) for v in wshape)
    n = math.prod(wshape)
    R = 0 if L is None else L.shape[1]
    if mean.numel() not in (n, S * n) or (L is not None and L.shape[0] != n):
        raise RuntimeError(f"lowrank_backward: mean [{mean.numel()}] / L do not fit a kernel of {n} weights and S={S}")
    if (eps_w is not None and R > 0 and z is None) or (eps_w is None and z is not None):
        raise RuntimeError("lowrank_backward: supply both draws (z, eps_w) or neither")
    if eps_w is not None and (eps_w.numel() != S * n or (R > 0 and tuple(z.shape) != (S, R))):
        raise RuntimeError(f"lowrank_backward: the supplied draws do not hold S={S} samples")
    B, geom, x_elems, tail = _geometry(x, _Shape(wshape), conv, S, shared_x)
    if g.numel() != S * B * math.prod(tail):
        raise RuntimeError(f"lowrank_backward: grad_out {tuple(g.shape)} is not the forward's output [{S * B}, {tail}]")
    lib = _lib.lib()
    dx = torch.empty((S, B) + tuple(x.shape[1:]), dtype=torch.float32, device=dev) if need_x else None
    dw = torch.empty((S, n), dtype=torch.float32, device=dev) if need_w else None
    # partials of wgrad's reduction chunks and of dgrad's output-channel pieces (contents need not be initialised)
    ws = torch.empty(max(16, lib.bt_lowrank_conv2d_bwd_workspace(C.byref(geom), S, R)), dtype=torch.uint8, device=dev)
    Rg = _rng(seed, call, layer_id, sample0, call_base)
    sd = C.c_float(math.sqrt(C.c_float(float(d)).value)).value      # the forward's sqrtf(d): a double root of a float rounds to the float root
    with _lib.on(dev):
        _lib.check(lib.bt_lowrank_conv2d_bwd(C.byref(geom), S, x.data_ptr(), 0 if shared_x else x_elems, g.data_ptr(), mean.data_ptr(),
                                             n if mean.numel() == S * n and S > 1 else 0, _lib.ptr(L), R, sd, _lib.ptr(z) if R > 0 else None, C.byref(Rg), _lib.ptr(eps_w),
                                             _lib.ptr(dx), _lib.ptr(dw), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
    info = _lib.lowrank_bwd_info()
    if need_x:
        dx = dx.sum(0) if shared_x else dx.reshape(x.shape)
    return dx, dw, info


def lowrank_wgrad_finish(dw, r, z=None, *, need_mu=True, need_L=True, seed=0, call=0, layer_id=0, sample0=0, call_base=None):
    """The chain rule over the per-sample weight gradients dw [S, n] of ``lowrank_backward`` (bt_lowrank_wgrad_finish):
    dmu[i] = sum_s dw[s, i], dL[i, j] = sum_s dw[s, i] * z_s[j], s ascending, for any rank r. z: [S, r], or None for the on-chip stream
    (tensor 4 of the call's coordinates). -> (dmu [n] or None, dL [n, r] or None)."""
    dw, z = _lib.dev_f32(dw, "dw"), _lib.dev_f32(z, "z")
    S, n = dw.shape
    if z is not None and tuple(z.shape) != (S, r):
        raise RuntimeError(f"lowrank_wgrad_finish: z {tuple(z.shape)} does not hold S={S} samples of rank {r}")
    dmu = torch.empty((n,), dtype=torch.float32, device=dw.device) if need_mu else None
    dL = torch.empty((n, r), dtype=torch.float32, device=dw.device) if need_L else None
    if dmu is None and dL is None:
        return None, None
    Rg = _rng(seed, call, layer_id, sample0, call_base)
    with _lib.on(dw.device):
        _lib.check(_lib.lib().bt_lowrank_wgrad_finish(dw.data_ptr(), n, int(r), S, _lib.ptr(z), C.byref(Rg), _lib.ptr(dmu), _lib.ptr(dL), _lib.stream_ptr(dw.device)))
    return dmu, dL


def kl_lowrank_backward(mu, L, d, prior_mean, prior_var, grad_kl, *, need_mu=True, need_L=True, bad_pivots=None):
    """Gradient of ``kl_lowrank``'s un-normalised KL times ``grad_kl`` (a device scalar) on the HIP kernels (bt_kl_lowrank_bwd: fp64, the
    forward's sweep, its Cholesky factor kept, an explicit r x r inverse; five launches, nothing synchronised)
    -> (dmu like mu or None, dL like L or None), fp32."""
    mu, L = _lib.dev_f32(mu, "mu"), _lib.dev_f32(L, "L")
    pm, pv = _lib.dev_f32(prior_mean, "prior_mean"), _lib.dev_f32(prior_var, "prior_var")
    g = _lib.dev_f32(grad_kl.reshape(1).contiguous(), "grad_kl")
    n, r = L.shape
    if mu.numel() != n or pm.numel() != n or pv.numel() != n:
        raise RuntimeError("kl_lowrank_backward: mu, prior_mean and prior_var must have L's row count")
    if not (need_mu or need_L):
        return None, None
    lib = _lib.lib()
    need = int(lib.bt_kl_lowrank_bwd_workspace(n, r))
    if need == 0:
        raise NotImplementedError(f"kl_lowrank_backward: rank {r} is above the factorisation kernel's limit")
    ws = torch.empty(need, dtype=torch.uint8, device=mu.device)
    dmu = torch.empty_like(mu) if need_mu else None
    dL = torch.empty_like(L) if need_L else None
    with _lib.on(mu.device):
        _lib.check(lib.bt_kl_lowrank_bwd(mu.data_ptr(), L.data_ptr(), n, r, float(d), pm.data_ptr(), pv.data_ptr(), g.data_ptr(), _lib.ptr(dmu), _lib.ptr(dL),
                                         _lib.ptr(bad_pivots), ws.data_ptr(), ws.numel(), _lib.stream_ptr(mu.device)))
    return dmu, dL


def pack_params(mu_w, rho_w):
    """Tap-major re-layout of a layer's (mu, softplus(rho)) -> (mu_packed, sigma_packed), each [Co, taps, Ci4]
    (include/bt_hip.h, bt_params). A cache of a pure function of the parameters; rebuild when they change."""
    mu_w, rho_w = _lib.dev_f32(mu_w, "mu_w"), _lib.dev_f32(rho_w, "rho_w")
    Co, Ci = mu_w.shape[0], mu_w.shape[1]
    taps = 1
    for d in mu_w.shape[2:]:
        taps *= d
    C4 = (Ci + 3) // 4 * 4
    mp = torch.empty((Co, taps, C4), dtype=torch.float32, device=mu_w.device)
    sp = torch.empty_like(mp)
    with _lib.on(mu_w.device):
        _lib.check(_lib.lib().bt_pack_params(mu_w.data_ptr(), rho_w.data_ptr(), Co, Ci, taps, mp.data_ptr(), sp.data_ptr(), _lib.stream_ptr(mu_w.device)))
    return mp, sp


def pack_buffers(Co, Ci, taps, device):
    """Persistent storage of one layer's pack: (mu_packed, sigma_packed, state) -- state = the 4 device words bt_pack_sync keeps
    (accumulator, fingerprint of the packed copy, dirty flag of the last call, rebuild count)."""
    C4 = (Ci + 3) // 4 * 4
    mp = torch.empty((Co, taps, C4), dtype=torch.float32, device=device)
    return mp, torch.empty_like(mp), torch.zeros(4, dtype=torch.int64, device=device)


def _kl_entry(kl):
    """kl = (prior_mu_w, prior_sigma_w, mu_b|None, rho_b|None, prior_mu_b|None, prior_sigma_b|None, kl_out) -> (bt_pack_kl, tensors kept)."""
    pm, ps = _lib.dev_f32(kl[0], "prior_mu_w"), _lib.dev_f32(kl[1], "prior_sigma_w")
    b = [None if t is None else _lib.dev_f32(t.detach(), "bias") for t in kl[2:6]]
    out = kl[6]
    n_bias = 0 if b[0] is None else b[0].numel()
    if any((t is None) != (b[0] is None) or (t is not None and t.numel() != n_bias) for t in b):
        raise RuntimeError("pack_sync: give all four bias tensors of a layer's KL, of one size, or none")
    return _lib.bt_pack_kl(pm.data_ptr(), ps.data_ptr(), *[_lib.ptr(t) for t in b], out.data_ptr(), n_bias), (pm, ps, b, out)


def _pack_sync_launch(arr, karr, owner, dev):
    """One bt_pack_sync call over the marshalled segments ``arr``; with ``karr`` (their bt_pack_kl entries) bt_pack_sync_kl."""
    L = _lib.lib()
    with _lib.on(dev):
        ws = _lib.workspace((owner, "pack"), dev).data_ptr()
        if karr is None:
            _lib.check(L.bt_pack_sync(len(arr), arr, ws, _lib.WORKSPACE_BYTES, _lib.stream_ptr(dev)))
        else:
            _lib.check(L.bt_pack_sync_kl(len(arr), arr, karr, ws, _lib.WORKSPACE_BYTES, _lib.stream_ptr(dev)))


def pack_sync(segments, owner="pack", kls=None):
    """segments: list of dict(mu, rho, src_mu|None, src_rho|None, mu_packed, sigma_packed, state, Co, Ci, taps, force) on ONE device.
    Re-packs, ON THE DEVICE and in the current stream, exactly the layers whose (mu, rho) no longer match the fingerprint their pack
    was built from (bt_pack_sync: two launches per 64 layers, no host synchronisation, graph-capturable).
    kls: None, or one entry per segment -- None or (prior_mu_w, prior_sigma_w, mu_b, rho_b, prior_mu_b, prior_sigma_b, kl_out): the
    sweep then also writes that layer's KL term ('normal' prior) into the 0-dim fp32 device tensor kl_out (bt_pack_sync_kl), and the
    layer's forward can go without its own KL sweep."""
    if not segments:
        return
    dev = segments[0]["mu"].device
    if kls is not None and all(k is None for k in kls):
        kls = None
    if len(segments) == 1 and "_c" in segments[0]:      # a layer checking itself again: its marshalled entry is still valid (same tensors, same buffers)
        arr = segments[0]["_c"][0]
        arr[0].force = 1 if segments[0].get("force") else 0
        return _pack_sync_launch(arr, None if kls is None else (_lib.bt_pack_kl * 1)(_kl_entry(kls[0])[0]), owner, dev)
    for c0 in range(0, len(segments), _lib.PACK_MAX_SEGMENTS):
        chunk = segments[c0:c0 + _lib.PACK_MAX_SEGMENTS]
        kchunk = None if kls is None else kls[c0:c0 + _lib.PACK_MAX_SEGMENTS]
        arr = (_lib.bt_pack_seg * len(chunk))()
        karr = None if kchunk is None else (_lib.bt_pack_kl * len(chunk))()
        keep = []
        for i, sg in enumerate(chunk):
            mu, rho = _lib.dev_f32(sg["mu"], "mu_w"), _lib.dev_f32(sg["rho"], "rho_w")
            smu = _lib.dev_f32(sg.get("src_mu"), "src_mu")
            srho = _lib.dev_f32(sg.get("src_rho"), "src_rho")
            if mu.device != dev:
                raise RuntimeError("pack_sync: all layers of one call must live on one device")
            keep.append((mu, rho, smu, srho))
            n_src = (smu if smu is not None else mu).numel()
            if n_src != sg["Co"] * sg["Ci"] * sg["taps"] or mu.numel() != n_src or rho.numel() != n_src:
                raise RuntimeError("pack_sync: geometry does not match the parameter tensors")
            arr[i] = _lib.bt_pack_seg(mu.data_ptr(), rho.data_ptr(), _lib.ptr(smu), _lib.ptr(srho), sg["mu_packed"].data_ptr(), sg["sigma_packed"].data_ptr(),
                                      sg["state"].data_ptr(), sg["Co"], sg["Ci"], sg["taps"], 1 if sg.get("force") else 0, 0)
            if kchunk is not None and kchunk[i] is not None:
                if kchunk[i][0].numel() != mu.numel():
                    raise RuntimeError("pack_sync: the weight priors do not have mu_w's size")
                karr[i], kept = _kl_entry(kchunk[i])
                keep.append(kept)
        if len(segments) == 1:
            segments[0]["_c"] = (arr, keep[:1])
        _pack_sync_launch(arr, karr, owner, dev)


def mc_epilogue(logits):
    """logits [S, B, C] -> packed [B*C + B + B*C] = [sum_s softmax | sum_s entropy | sum_s logits]."""
    logits = _lib.dev_f32(logits, "logits")
    S, B, Cc = logits.shape
    packed = torch.empty(B * Cc + B + B * Cc, dtype=torch.float32, device=logits.device)
    with _lib.on(logits.device):
        _lib.check(_lib.lib().bt_mc_epilogue(S, B, Cc, logits.data_ptr(), packed.data_ptr(), _lib.stream_ptr(logits.device)))
    return packed


def _cell_rows(t, H, what):
    """A [rows, H] operand the LSTM cell kernels address by row stride -> (tensor, rows, stride). A view whose rows are contiguous (one
    time slab of a [rows, T, H] buffer) stays a view; anything else is validated, and made contiguous, by ``_lib.dev_f32``."""
    if t is None:
        return None, 0, H
    if t.dim() != 2 or t.shape[1] != H:
        raise RuntimeError(f"{what}: expected [rows, {H}], got {tuple(t.shape)}")
    if t.is_contiguous() or t.stride(1) != 1 or t.stride(0) < H:
        return _lib.dev_f32(t, what), t.shape[0], H
    if not t.is_cuda:
        raise RuntimeError(f"{what} is on {t.device}: bayesian_torch_amd runs on a HIP (MI355X) device only; there is no CPU implementation of this path")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {t.dtype}")
    return t, t.shape[0], t.stride(0)


def _cell_out(t, rows, H, device, what):
    """A result of the cell forward: a fresh [rows, H] tensor, or the caller's row-strided view (written in place) -> (tensor, stride)."""
    if t is None:
        return torch.empty((rows, H), dtype=torch.float32, device=device), H
    if t.dim() != 2 or tuple(t.shape) != (rows, H) or t.dtype != torch.float32 or t.device != device or (H > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) < H):
        raise RuntimeError(f"{what}: expected a float32 [{rows}, {H}] view with contiguous rows on {device}, got {tuple(t.shape)} strides {tuple(t.stride())}")
    return t, (t.stride(0) if rows > 1 else H)


def lstm_cell_fwd(a, b, c_prev, h_out=None, c_out=None, want_act=False):
    """The LSTM cell of one time step on its HIP kernel (bt_lstm_cell_fwd): z = a + b ([rows, 4H], gate order i, f, g, o; b may be None),
    c = f * c_prev + i * g, h = o * tanh(c). c_prev: [c_rows, H] with c_rows = rows or a divisor of it (row r reads row r % c_rows: a
    state shared by the MC samples); rows may be strided. h_out / c_out: row-strided [rows, H] views to write into (a slab of a
    sequence buffer), made when None. want_act: also return the activated gates [rows, 4H] for ``lstm_cell_bwd``.
    -> (h, c, act or None)."""
    a, b = _lib.dev_f32(a, "a"), _lib.dev_f32(b, "b")
    if a.dim() != 2 or a.shape[1] % 4 or a.shape[1] == 0 or (b is not None and b.shape != a.shape):
        raise RuntimeError(f"lstm_cell_fwd: a and b are [rows, 4H], got {tuple(a.shape)} and {None if b is None else tuple(b.shape)}")
    rows, H = a.shape[0], a.shape[1] // 4
    dev = a.device
    c_prev, c_rows, ld_c = _cell_rows(c_prev, H, "c_prev")
    if c_prev is None or c_rows < 1 or rows % c_rows:
        raise RuntimeError(f"lstm_cell_fwd: c_prev has {c_rows} rows, the gates {rows}")
    h_out, ld_h = _cell_out(h_out, rows, H, dev, "h_out")
    c_out, ld_o = _cell_out(c_out, rows, H, dev, "c_out")
    if ld_h != ld_o:
        raise RuntimeError("lstm_cell_fwd: h_out and c_out must have one row stride")
    act = torch.empty((rows, 4 * H), dtype=torch.float32, device=dev) if want_act else None
    with _lib.on(dev):
        _lib.check(_lib.lib().bt_lstm_cell_fwd(rows, H, a.data_ptr(), _lib.ptr(b), c_prev.data_ptr(), c_rows, ld_c, h_out.data_ptr(), c_out.data_ptr(), ld_o,
                                               _lib.ptr(act), _lib.stream_ptr(dev)))
    return h_out, c_out, act


def lstm_cell_bwd(act, c_prev, c_new, grad_h, grad_c):
    """Gradients of ``lstm_cell_fwd`` on the HIP kernel (bt_lstm_cell_bwd), the closed form on the saved activations. grad_h / grad_c:
    [rows, H] (rows may be strided) or None for zero. -> (dz [rows, 4H], the gradient of a and of b alike; dc_prev [rows, H], per row:
    the caller sums a shared c_prev's over the samples)."""
    act = _lib.dev_f32(act, "act")
    rows, H = act.shape[0], act.shape[1] // 4
    dev = act.device
    c_prev, c_rows, ld_c = _cell_rows(c_prev, H, "c_prev")
    c_new, n_rows, ld_cn = _cell_rows(c_new, H, "c_new")
    grad_h, gh_rows, ld_gh = _cell_rows(grad_h, H, "grad_h")
    grad_c, gc_rows, ld_gc = _cell_rows(grad_c, H, "grad_c")
    if c_prev is None or c_new is None or c_rows < 1 or rows % c_rows or n_rows != rows or (grad_h is not None and gh_rows != rows) or (grad_c is not None and gc_rows != rows):
        raise RuntimeError("lstm_cell_bwd: c_new, grad_h and grad_c have the gates' rows, c_prev those or a divisor of them")
    dz = torch.empty((rows, 4 * H), dtype=torch.float32, device=dev)
    dc_prev = torch.empty((rows, H), dtype=torch.float32, device=dev)
    with _lib.on(dev):
        _lib.check(_lib.lib().bt_lstm_cell_bwd(rows, H, act.data_ptr(), c_prev.data_ptr(), c_rows, ld_c, c_new.data_ptr(), ld_cn, _lib.ptr(grad_h), ld_gh,
                                               _lib.ptr(grad_c), ld_gc, dz.data_ptr(), dc_prev.data_ptr(), _lib.stream_ptr(dev)))
    return dz, dc_prev


def fused_backward(x, grad_out, mu_w, rho_w, packed, *, flip=False, conv=None, S=1, shared_x=True, need_x=True, need_w=True,
                   eps_w=None, sign_in=None, sign_out=None, seed=0, call=0, layer_id=0, sample0=0, call_base=None, kl=None):
    """Gradients of ``fused_forward`` on the HIP backward kernels (bt_conv2d_bwd): the draws are regenerated on chip from the
    forward's RNG coordinates (or the injected ones are read).  x / grad_out as the forward saw / produced them.
    -> (dx like x or None, dmu_w, drho_w like mu_w or None).  Bias gradients are row sums of grad_out (caller).
    ``kl = (grad_kl device scalar, prior_mu_w, prior_sigma_w, prior kind)``: the layer's weight-KL term is differentiated in the same
    pass and added to dmu_w / drho_w (bt_conv2d_bwd_kl)."""
    x, g = _lib.dev_f32(x, "input"), _lib.dev_f32(grad_out, "grad_out")
    dev = x.device
    mu_w, rho_w = _lib.dev_f32(mu_w, "mu_w"), _lib.dev_f32(rho_w.detach(), "rho_w")
    B, geom, x_elems, _ = _geometry(x, mu_w, conv, S, shared_x)
    dx = torch.empty((S,) + (B,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev) if need_x else None
    dmu = torch.empty_like(mu_w) if need_w else None
    drho = torch.empty_like(mu_w) if need_w else None
    L = _lib.lib()
    # partials of wgrad's sample / reduction groups and of dgrad's output-channel pieces (contents need not be initialised)
    ws = torch.empty(max(16, L.bt_conv2d_bwd_workspace(C.byref(geom), S)), dtype=torch.uint8, device=dev)
    inj = [None if t is None else _lib.dev_f32(t, "draw") for t in (eps_w, sign_in, sign_out)]
    gkl = pm = ps = None
    lap = 0
    if kl is not None and need_w:
        gkl = _lib.dev_f32(kl[0].reshape(1), "grad_kl")
        lap = 1 if kl[3] == "laplace" else 0
        pm, ps = (None, None) if lap else (_lib.dev_f32(kl[1], "prior_mu"), _lib.dev_f32(kl[2], "prior_sigma"))
    P = _lib.bt_params(mu_w.data_ptr(), rho_w.data_ptr(), None, None, _lib.ptr(pm), _lib.ptr(ps), None, None, packed[0].data_ptr(), packed[1].data_ptr(), lap, 0)
    R = _rng(seed, call, layer_id, sample0, call_base)     # call_base: the device word of a captured training step (mc.TrainGraph)
    D = _lib.bt_draws(_lib.ptr(inj[0]), None, _lib.ptr(inj[1]), _lib.ptr(inj[2]), R)
    with _lib.on(dev):
        _lib.check(L.bt_conv2d_bwd_kl(C.byref(geom), S, 1 if flip else 0, x.data_ptr(), 0 if shared_x else x_elems, g.data_ptr(), C.byref(P), C.byref(D), _lib.ptr(gkl),
                                      _lib.ptr(dx), _lib.ptr(dmu), _lib.ptr(drho), _lib.ptr(ws), 0 if ws is None else ws.numel(), _lib.stream_ptr(dev)))
    if need_x:
        dx = dx.sum(0) if shared_x else dx.reshape(x.shape)
    return dx, dmu, drho


def kl_backward(mu, rho, prior_mu, prior_sigma, grad_kl, laplace=False):
    """(d kl / d mu, d kl / d rho) * grad_kl for one tensor of bt_kl_normal's mean (HIP kernel bt_kl_normal_bwd)."""
    mu, rho = _lib.dev_f32(mu.detach(), "mu"), _lib.dev_f32(rho.detach(), "rho")
    pm = None if laplace else _lib.dev_f32(prior_mu, "prior_mu")
    ps = None if laplace else _lib.dev_f32(prior_sigma, "prior_sigma")
    g = _lib.dev_f32(grad_kl.reshape(1).contiguous(), "grad_kl")
    dmu, drho = torch.empty_like(mu), torch.empty_like(mu)
    with _lib.on(mu.device):
        _lib.check(_lib.lib().bt_kl_normal_bwd(mu.data_ptr(), rho.data_ptr(), _lib.ptr(pm), _lib.ptr(ps), g.data_ptr(), mu.numel(),
                                               _lib.KL_PRIOR_LAPLACE if laplace else 0, dmu.data_ptr(), drho.data_ptr(), _lib.stream_ptr(mu.device)))
    return dmu, drho


def kl_backward_segs(segments, grad_kl, laplace=False):
    """[(d kl / d mu, d kl / d rho) * grad_kl] for every (mu, rho, prior_mu, prior_sigma) segment of bt_kl_normal's sum, ONE HIP
    launch per BT_KL_MAX_SEGMENTS tensors (bt_kl_normal_bwd_segs): the backward of a whole model's get_kl_loss."""
    L = _lib.lib()
    dev = segments[0][0].device
    g = _lib.dev_f32(grad_kl.reshape(1).contiguous(), "grad_kl")
    out = []

    def prepare(_, seg):
        mu, rho = _lib.dev_f32(seg[0].detach(), "mu"), _lib.dev_f32(seg[1].detach(), "rho")
        pm = None if laplace else _lib.dev_f32(seg[2], "prior_mu")
        ps = None if laplace else _lib.dev_f32(seg[3], "prior_sigma")
        out.append((torch.empty_like(mu), torch.empty_like(mu)))
        return (mu, rho, pm, ps) + out[-1]

    for _, n, keep, arrs, numel, _ in _lib.seg_chunks(segments, prepare):
        with _lib.on(dev):
            _lib.check(L.bt_kl_normal_bwd_segs(n, arrs[0], arrs[1], arrs[2] if not laplace else None, arrs[3] if not laplace else None, numel, g.data_ptr(),
                                               _lib.KL_PRIOR_LAPLACE if laplace else 0, arrs[4], arrs[5], _lib.stream_ptr(dev)))
    return out


def kl_hier_backward(segments, grad_kl, needs=None):
    """[(d kl / d mu, d rho, d log_a, d log_b) * grad_kl] for every (mu, rho, prior_mu, log_a, log_b, a0, b0) segment of bt_kl_hier's
    sum, ONE HIP launch per BT_KL_MAX_SEGMENTS tensors (bt_kl_hier_bwd). needs: per segment four booleans -- a gradient nobody asked
    for is neither allocated nor written (None in its place); default: all."""
    L = _lib.lib()
    dev = segments[0][0].device
    g = _lib.dev_f32(grad_kl.reshape(1).contiguous(), "grad_kl")
    out = []

    def prepare(j, seg):
        ts = [_lib.dev_f32(t.detach(), "kl segment tensor") for t in seg]
        if len(ts) != 7 or not all(t.numel() == ts[0].numel() for t in ts):
            raise ValueError("a hierarchical KL segment is (mu, rho, prior_mu, log_a, log_b, a0, b0) of equal numel")
        want = (True,) * 4 if needs is None else needs[j]
        out.append(tuple(torch.empty_like(ts[0]) if w else None for w in want))
        return tuple(ts) + out[-1]

    for c0, n, keep, arrs, numel, _ in _lib.seg_chunks(segments, prepare):
        if any(t is not None for grads in out[c0:c0 + n] for t in grads):
            with _lib.on(dev):
                _lib.check(L.bt_kl_hier_bwd(n, *arrs[:7], numel, g.data_ptr(), *arrs[7:], _lib.stream_ptr(dev)))
    return out


AVU_THRESHOLDS = 21   # AUAvULoss: np.linspace(0, 1, 21) between the batch's smallest and largest uncertainty


def avu_forward(logits, labels, unc_type=0, T=1, threshold=None, beta=1.0):
    """The AvUC loss of utils/avuc_loss.py on its HIP kernels (bt_avu_fwd: a row pass and a one-workgroup finish pass, no host
    read). logits: [S, B, C] (S Monte Carlo samples; the reference's [B, C] is S = 1); labels: [B] integers. T = 1: AvULoss against
    ``threshold``, a one-element device tensor; T = 21: AUAvULoss. -> dict: loss [1], v [1] (AvU, or the area under AvU), sums [T, 4]
    (n_ac, n_au, n_ic, n_iu), counts [T, 4] int32, thresholds [T] float64, coef (for ``avu_backward``), workspace, and views of the
    workspace: confidence, uncertainty, tanh_uncertainty [B], pred, acc, first_certain [B] int32 (a row is uncertain at the thresholds
    below index first_certain and certain from there on; T when it never is)."""
    logits = _lib.dev_f32(logits, "logits")
    if logits.dim() != 3:
        raise ValueError(f"avu_forward: logits are [S, B, C], got {tuple(logits.shape)}")
    S, B, Cc = logits.shape
    dev = logits.device
    if not labels.is_cuda:
        raise RuntimeError(f"labels are on {labels.device}: bayesian_torch_amd runs on a HIP (MI355X) device only; there is no CPU implementation of this path")
    if labels.dim() != 1 or labels.shape[0] != B or labels.dtype.is_floating_point:
        raise ValueError(f"avu_forward: labels are [B = {B}] integers, got {tuple(labels.shape)} {labels.dtype}")
    labels = labels.to(torch.int64).contiguous()
    if T == 1:
        threshold = _lib.dev_f32(threshold, "threshold")
        if threshold is None or threshold.numel() != 1:
            raise ValueError("avu_forward: T = 1 takes a one-element threshold tensor")
    L = _lib.lib()
    nbytes = L.bt_avu_workspace_bytes(S, B, Cc, T)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    v = torch.empty(1, dtype=torch.float32, device=dev)
    sums = torch.empty((T, 4), dtype=torch.float32, device=dev)
    counts = torch.empty((T, 4), dtype=torch.int32, device=dev)
    thr = torch.empty(T, dtype=torch.float64, device=dev)
    coef = torch.empty((4, T + 1), dtype=torch.float32, device=dev)
    with _lib.on(dev):
        _lib.check(L.bt_avu_fwd(S, B, Cc, logits.data_ptr(), labels.data_ptr(), int(unc_type), int(T), _lib.ptr(threshold), float(beta), loss.data_ptr(),
                                v.data_ptr(), sums.data_ptr(), counts.data_ptr(), thr.data_ptr(), coef.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr(dev)))
    rec_f = ws[:12 * B].view(torch.float32).view(3, B)
    rec_i = ws[12 * B:24 * B].view(torch.int32).view(3, B)
    return dict(loss=loss, v=v, sums=sums, counts=counts, thresholds=thr, coef=coef, workspace=ws, confidence=rec_f[0], uncertainty=rec_f[1],
                tanh_uncertainty=rec_f[2], pred=rec_i[0], acc=rec_i[1], first_certain=rec_i[2])


def avu_backward(logits, unc_type, T, coef, workspace, grad_loss):
    """d loss / d logits [S, B, C] of ``avu_forward`` times ``grad_loss`` (a one-element device tensor), one launch (bt_avu_bwd) from
    the forward's ``coef`` and ``workspace``; the softmax is recomputed from the logits."""
    logits = _lib.dev_f32(logits, "logits")
    S, B, Cc = logits.shape
    dev = logits.device
    g = _lib.dev_f32(grad_loss.reshape(1), "grad_loss")
    dlogits = torch.empty_like(logits)
    with _lib.on(dev):
        _lib.check(_lib.lib().bt_avu_bwd(S, B, Cc, logits.data_ptr(), int(unc_type), int(T), coef.data_ptr(), g.data_ptr(), workspace.data_ptr(),
                                         workspace.numel(), dlogits.data_ptr(), _lib.stream_ptr(dev)))
    return dlogits


def _dev_i8(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what} is on {t.device}: the INT8 forward runs on a HIP (MI355X) device only; there is no CPU implementation of this path")
    if t.dtype != torch.int8:
        raise TypeError(f"{what} must be int8, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def q8_pack(q_mu, q_sigma):
    """The [Co][taps][Ci16] int8 packs of a quantised layer's two parameter images (bt_q8_pack; Ci16: Ci rounded up to a multiple of
    16, padding 0). q_mu, q_sigma: int8 [Co, Ci, kh, kw] or [Out, In] -> (mu_packed, sigma_packed), each [Co, taps, Ci16]."""
    q_mu, q_sigma = _dev_i8(q_mu, "q_mu"), _dev_i8(q_sigma, "q_sigma")
    if q_mu.shape != q_sigma.shape or q_mu.dim() not in (2, 4):
        raise RuntimeError("q8_pack: q_mu and q_sigma must be two int8 tensors of one shape, [Co, Ci, kh, kw] or [Out, In]")
    Co, Ci = q_mu.shape[0], q_mu.shape[1]
    taps = math.prod(q_mu.shape[2:])
    Ci16 = (Ci + 15) // 16 * 16
    mp = torch.empty((Co, taps, Ci16), dtype=torch.int8, device=q_mu.device)
    sp = torch.empty_like(mp)
    with _lib.on(q_mu.device):
        _lib.check(_lib.lib().bt_q8_pack(q_mu.data_ptr(), q_sigma.data_ptr(), Co, Ci, taps, mp.data_ptr(), sp.data_ptr(), _lib.stream_ptr(q_mu.device)))
    return mp, sp


def _dev_u8(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what} is on {t.device}: the INT8 forward runs on a HIP (MI355X) device only; there is no CPU implementation of this path")
    if t.dtype != torch.uint8:
        raise TypeError(f"{what} must be uint8, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


class _XShape:
    """What ``_geometry`` reads of an input: the LOGICAL shape of a blocked u8 image."""

    def __init__(self, shape):
        self.shape = tuple(int(v) for v in shape)

    def dim(self):
        return len(self.shape)

    def numel(self):
        return math.prod(self.shape)


def q8_blocked_shape(shape):
    """The storage of a quantised activation of logical shape [N, C, H, W] or [N, F]: u8 [N, CB, H, W, 16] / [N, CB * 16], CB = ceil(C / 16)
    (include/bt_hip.h)."""
    shape = tuple(int(v) for v in shape)
    if len(shape) == 2:
        return (shape[0], (shape[1] + 15) // 16 * 16)
    if len(shape) != 4:
        raise RuntimeError(f"a quantised activation is [N, C, H, W] or [N, F], got {shape}")
    return (shape[0], (shape[1] + 15) // 16, shape[2], shape[3], 16)


def _q8_launch(who, x, packs, wshape, mu_b, sigma_b, conv, S, shared_x, eps_w, eps_b, rng, want_q, params, draws=None, x_shape=None, dest="f32"):
    """What the two INT8 forwards share: the operands, the draw sizes, the geometry, the outputs and the linear / conv2d call of
    ``bt_<who>_*_fwd``. params(mu_packed, sigma_packed, mu_b, sigma_b) -> the entry's params struct; draws(B, x_elems, tail) -> the
    pointers the entry takes between eps_b and rng (checked against the geometry there). x_shape: x is the u8 BLOCKED image of that
    logical shape; dest "f32" / "u8" / "both": what is written -- with either a ``bt_<who>_*_fwd_act`` call, whose u8 result is the
    blocked image (want_q does not apply)."""
    act = x_shape is not None or dest != "f32"
    if dest not in ("f32", "u8", "both"):
        raise ValueError(f"{who}_forward: dest must be 'f32', 'u8' or 'both', got {dest!r}")
    if x_shape is None:
        x = _lib.dev_f32(x, "input")
        xs = x
    else:
        x = _dev_u8(x, "input")
        xs = _XShape(x_shape)
        if x.numel() != math.prod(q8_blocked_shape(xs.shape)):
            raise RuntimeError(f"{who}_forward: the blocked image of {xs.shape} holds {math.prod(q8_blocked_shape(xs.shape))} bytes, got {x.numel()}")
    mu_b, sigma_b = _lib.dev_f32(mu_b, "mu_b"), _lib.dev_f32(sigma_b, "sigma_b")
    eps_w, eps_b = _lib.dev_f32(eps_w, "eps_w"), _lib.dev_f32(eps_b, "eps_b")
    mp, sp = _dev_i8(packs[0], "mu_packed"), _dev_i8(packs[1], "sigma_packed")
    wshape = tuple(int(v) for v in wshape)
    n = math.prod(wshape)
    if eps_w is not None and eps_w.numel() != S * n:
        raise RuntimeError(f"{who}_forward: eps_w holds {eps_w.numel()} elements, S={S} samples of {n} weights need {S * n}")
    if eps_b is not None and eps_b.numel() != S * wshape[0]:
        raise RuntimeError(f"{who}_forward: eps_b must be [S={S}, {wshape[0]}]")
    dev = x.device
    B, geom, x_elems, tail = _geometry(xs, _Shape(wshape), conv, S, shared_x)
    more = draws(B, x_elems, tail) if draws else ()
    out = torch.empty((S * B,) + tail, dtype=torch.float32, device=dev) if dest != "u8" else None
    if act:
        out_q = torch.empty(q8_blocked_shape((S * B,) + tail), dtype=torch.uint8, device=dev) if dest != "f32" else None
    else:
        out_q = torch.empty((S * B,) + tail, dtype=torch.uint8, device=dev) if want_q else None
    P = params(mp.data_ptr(), sp.data_ptr(), _lib.ptr(mu_b), _lib.ptr(sigma_b))
    Rg = _rng(*rng)
    stride = 0 if shared_x else (x_elems if x_shape is None else x.numel() // S)
    kind = (_lib.Q8_X_F32 if x_shape is None else _lib.Q8_X_U8,) if act else ()
    tail_args = (x.data_ptr(), *kind, stride, C.byref(P), _lib.ptr(eps_w), _lib.ptr(eps_b), *more, C.byref(Rg), _lib.ptr(out), _lib.ptr(out_q),
                 _lib.stream_ptr(dev))
    sfx = "_act" if act else ""
    with _lib.on(dev):
        if conv is None:
            _lib.check(getattr(_lib.lib(), f"bt_{who}_linear_fwd{sfx}")(B, wshape[1], wshape[0], S, *tail_args))
        else:
            _lib.check(getattr(_lib.lib(), f"bt_{who}_conv2d_fwd{sfx}")(C.byref(geom), S, *tail_args))
    return out, out_q


def q8_forward(x, packs, wshape, s_mu, s_sigma, pairs, mu_b=None, sigma_b=None, *, conv=None, S=1, shared_x=True, eps_w=None, eps_b=None,
               seed=0, call=0, layer_id=0, sample0=0, call_base=None, want_q=False, x_shape=None, dest="f32"):
    """The INT8 fused forward (bt_q8_conv2d_fwd / bt_q8_linear_fwd; the arithmetic is include/bt_hip.h's). x: fp32 [B, Ci, H, W]
    (conv: dict(stride, padding, dilation, groups)) or [B, In] (conv None); packs: q8_pack's; wshape: the weight's natural shape;
    pairs: five (scale, zero point) -- eps, mul, add, in, out; eps_w [S, *wshape] and eps_b [S, Co] supplied, or None for the on-chip
    streams. -> (out fp32 [S * B, Co, ...], the u8 image or None).
    u8 activations (bt_q8_*_fwd_act): x_shape -- x is the u8 BLOCKED image (``q8_blocked_shape``) of that
    logical shape at the pair ``pairs[in]``; dest "u8" / "both" -- the result is the blocked image at ``pairs[out]`` (and out is None
    for "u8": nothing fp32-sized is written). -> (out or None, the blocked image or None)."""
    pr = [_lib.bt_q8_pair(float(s), int(z), 0) for s, z in pairs]
    return _q8_launch("q8", x, packs, wshape, mu_b, sigma_b, conv, S, shared_x, eps_w, eps_b, (seed, call, layer_id, sample0, call_base), want_q,
                      lambda *ptrs: _lib.bt_q8_params(pr[0], pr[1], pr[2], pr[3], pr[4], float(s_mu), float(s_sigma), *ptrs), x_shape=x_shape, dest=dest)


Q8_FLIP_PAIRS = ("eps", "delta", "in", "mean", "sign_in", "sign_out", "xp", "pert", "pert_signed", "out")      # the order of a ten-entry quant_dict


def q8_flip_forward(x, packs, wshape, s_mu, s_sigma, pairs, mu_b=None, sigma_b=None, *, conv=None, S=1, shared_x=True, eps_w=None, eps_b=None,
                    sign_in=None, sign_out=None, seed=0, call=0, layer_id=0, sample0=0, call_base=None, want_q=False, x_shape=None, dest="f32"):
    """The INT8 Flipout forward (bt_q8_flip_conv2d_fwd / bt_q8_flip_linear_fwd; the arithmetic is include/bt_hip.h's): both
    contractions and the operator chain between them in one launch. Arguments as ``q8_forward``, but ``pairs`` holds TEN (scale, zero
    point) in the order ``Q8_FLIP_PAIRS``, and a supplied draw is whole or absent: eps_w [S, *wshape], eps_b [S, Co] (when there is a
    sigma_b), sign_in fp32 [S, B, *x.shape[1:]] and sign_out fp32 [S, B, Co, ...] (a negative value means -1, anything else +1), or
    all None for the on-chip streams (tensors 0 to 3). -> (out fp32 [S * B, Co, ...], the u8 image or None). ``x_shape`` / ``dest``: as
    ``q8_forward``; the sign tensors stay in the LOGICAL (natural) order."""
    sign_in, sign_out = _lib.dev_f32(sign_in, "sign_in"), _lib.dev_f32(sign_out, "sign_out")
    if len(pairs) != len(Q8_FLIP_PAIRS):
        raise ValueError(f"q8_flip_forward: pairs must hold ten (scale, zero point): {', '.join(Q8_FLIP_PAIRS)}")

    def signs(B, x_elems, tail):
        n_out = B * math.prod(tail)
        if sign_in is not None and sign_in.numel() != S * x_elems:
            raise RuntimeError(f"q8_flip_forward: sign_in holds {sign_in.numel()} elements, S={S} samples of x need {S * x_elems}")
        if sign_out is not None and sign_out.numel() != S * n_out:
            raise RuntimeError(f"q8_flip_forward: sign_out holds {sign_out.numel()} elements, S={S} samples of the output need {S * n_out}")
        return _lib.ptr(sign_in), _lib.ptr(sign_out)

    pr = [_lib.bt_q8_pair(float(s), int(z), 0) for s, z in pairs]
    return _q8_launch("q8_flip", x, packs, wshape, mu_b, sigma_b, conv, S, shared_x, eps_w, eps_b, (seed, call, layer_id, sample0, call_base), want_q,
                      lambda *ptrs: _lib.bt_q8_flip_params(*pr, float(s_mu), float(s_sigma), *ptrs), signs, x_shape=x_shape, dest=dest)


# ---------------------------------------------------------------------------- u8 activations between the INT8 layers (csrc/bt_q8_act.hip)
# The launches quantization/qact.py's carrier is built on: blocked u8 images (``q8_blocked_shape``) in, blocked u8 images out, each ONE
# launch on the current stream with no host synchronisation. ``shape`` is always the LOGICAL shape, [N, C, H, W] or [N, F].
def _nchw(shape):
    shape = tuple(int(v) for v in shape)
    if len(shape) == 2:
        return (shape[0], shape[1], 1, 1)
    if len(shape) != 4:
        raise RuntimeError(f"a quantised activation is [N, C, H, W] or [N, F], got {shape}")
    return shape


def _act_call(name, dev, *args):
    with _lib.on(dev):
        _lib.check(getattr(_lib.lib(), name)(*args, _lib.stream_ptr(dev)))


def _blocked(q, shape, what):
    q = _dev_u8(q, what)
    if q.numel() != math.prod(q8_blocked_shape(shape)):
        raise RuntimeError(f"{what}: the blocked image of {tuple(shape)} holds {math.prod(q8_blocked_shape(shape))} bytes, got {q.numel()}")
    return q


def q8_act_quantize(x, scale, zero_point):
    """fp32 [N, C, H, W] or [N, F] -> its blocked u8 image at (scale, zero_point) (bt_q8_act_quantize: quantize_per_tensor)."""
    x = _lib.dev_f32(x, "input")
    q = torch.empty(q8_blocked_shape(x.shape), dtype=torch.uint8, device=x.device)
    _act_call("bt_q8_act_quantize", x.device, x.data_ptr(), *_nchw(x.shape), float(scale), int(zero_point), q.data_ptr())
    return q


def q8_act_dequantize(q, shape, scale, zero_point):
    """The blocked image of ``shape`` -> fp32 in natural order, (q - z) * s (bt_q8_act_dequantize)."""
    q = _blocked(q, shape, "q8_act_dequantize")
    out = torch.empty(tuple(shape), dtype=torch.float32, device=q.device)
    _act_call("bt_q8_act_dequantize", q.device, q.data_ptr(), *_nchw(shape), float(scale), int(zero_point), out.data_ptr())
    return out


def q8_act_relu(q, shape, zero_point, inplace=False):
    """max(q, z) on a blocked image (bt_q8_act_relu); inplace: q itself is overwritten and returned."""
    q = _blocked(q, shape, "q8_act_relu")
    out = q if inplace else torch.empty_like(q)
    _act_call("bt_q8_act_relu", q.device, q.data_ptr(), *_nchw(shape), int(zero_point), out.data_ptr())
    return out


def q8_act_add(a, a_shape, a_pair, b, b_shape, b_pair, out_pair, relu=False):
    """torch.ops.quantized.add / add_relu of two blocked images of one shape -> the blocked image at out_pair (bt_q8_act_add)."""
    a, b = _blocked(a, a_shape, "q8_act_add"), _blocked(b, b_shape, "q8_act_add")
    out = torch.empty_like(a)
    sa, sb = (C.c_int64 * 4)(*_nchw(a_shape)), (C.c_int64 * 4)(*_nchw(b_shape))
    _act_call("bt_q8_act_add", a.device, a.data_ptr(), sa, float(a_pair[0]), int(a_pair[1]), b.data_ptr(), sb, float(b_pair[0]), int(b_pair[1]), float(out_pair[0]),
              int(out_pair[1]), int(bool(relu)), out.data_ptr())
    return out


def q8_act_max_pool2d(q, shape, kernel, stride, padding):
    """The maximum of the levels over kernel windows, padding ignored -> (blocked image, its logical shape) (bt_q8_act_max_pool2d)."""
    q = _blocked(q, shape, "q8_act_max_pool2d")
    N, Cc, H, W = _nchw(shape)
    (kh, kw), (sh, sw), (ph, pw) = kernel, stride, padding
    Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    if min(kh, kw, sh, sw) < 1 or Ho < 1 or Wo < 1:
        raise RuntimeError("q8_act_max_pool2d: pooling output would be empty")
    oshape = (N, Cc, Ho, Wo)
    out = torch.empty(q8_blocked_shape(oshape), dtype=torch.uint8, device=q.device)
    _act_call("bt_q8_act_max_pool2d", q.device, q.data_ptr(), N, Cc, H, W, kh, kw, sh, sw, ph, pw, out.data_ptr())
    return out, oshape


def q8_act_avg_pool(q, shape, zero_point):
    """The global average pool [N, C, H, W] -> (blocked image, [N, C, 1, 1]) at the same pair (bt_q8_act_avg_pool)."""
    q = _blocked(q, shape, "q8_act_avg_pool")
    N, Cc, H, W = _nchw(shape)
    oshape = (N, Cc, 1, 1)
    out = torch.empty(q8_blocked_shape(oshape), dtype=torch.uint8, device=q.device)
    _act_call("bt_q8_act_avg_pool", q.device, q.data_ptr(), N, Cc, H, W, int(zero_point), out.data_ptr())
    return out, oshape


def q8_act_unblock(q, shape, zero_point):
    """Flatten [N, C, H, W] to [N, C * H * W] in NCHW feature order -> (blocked image, its logical shape) (bt_q8_act_unblock)."""
    q = _blocked(q, shape, "q8_act_unblock")
    N, Cc, H, W = _nchw(shape)
    oshape = (N, Cc * H * W)
    out = torch.empty(q8_blocked_shape(oshape), dtype=torch.uint8, device=q.device)
    _act_call("bt_q8_act_unblock", q.device, q.data_ptr(), N, Cc, H, W, int(zero_point), out.data_ptr())
    return out, oshape


# ---------------------------------------------------------------------------- calibration of the INT8 layers (csrc/bt_q8_observe.hip)
CALIB_ROWS = ("sigma", "mu", "eps", "mul", "add", "in", "out")      # the rows of a layer's ``calib_minmax`` [7, 2]: (min, max) pairs
# ... and of a Flipout layer's [13, 2]: bt_q8_observe_w's five rows ("add" is a quantity Flipout never forms: conversion ignores it), then
# the reference's eight quint8 stubs. Which rows are symmetric and which a quant_dict takes: layers/_calibration.py's schemas, which refer to these tuples.
CALIB_FLIP_ROWS = ("sigma", "mu", "eps", "delta", "add", "in", "mean", "sign_in", "sign_out", "xp", "pert", "pert_signed", "out")


def calib_buffers(device=None, rows=len(CALIB_ROWS)):
    """-> (calib_minmax fp32 [rows, 2] of (+inf, -inf) pairs, calib_nonfinite int32 [1] of 0): empty statistics."""
    mm = torch.empty((rows, 2), dtype=torch.float32, device=device)
    mm[:, 0], mm[:, 1] = float("inf"), float("-inf")
    return mm, torch.zeros(1, dtype=torch.int32, device=device)


def _calib_dev(t, what, dtype):
    if not t.is_cuda:
        raise RuntimeError(f"{what} is on {t.device}: the observer kernels run on a HIP (MI355X) device only")
    if t.dtype != dtype or not t.is_contiguous():
        raise TypeError(f"{what} must be a contiguous {dtype} tensor")
    return t


def _no_capture(dev, what):
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{what}: calibration inside a graph capture is not supported; run the calibration batches eagerly")


def q8_observe_w(mu, rho, stats, nonfinite, *, S=1, coef=None, eps=None, seed=0, call=0, layer_id=0, sample0=0, call_base=None):
    """The weight-side observers (bt_q8_observe_w): merge the ranges of sigma * coef, mu * coef, eps, their product and the sampled
    weight over S samples into ``stats`` (fp32, >= 10 elements: rows 0..4 of a ``calib_minmax``), counting non-finite values into
    ``nonfinite`` (int32 [1]). mu, rho: [Co, Ci, ...]; eps: [S, *mu.shape] supplied, or None for the on-chip tensor 0 stream of the
    given coordinates; coef: [Co] or None. Nothing is returned and nothing is read back."""
    mu, rho = _lib.dev_f32(mu, "mu"), _lib.dev_f32(rho, "rho")
    coef, eps = _lib.dev_f32(coef, "coef"), _lib.dev_f32(eps, "eps")
    _calib_dev(stats, "stats", torch.float32), _calib_dev(nonfinite, "nonfinite", torch.int32)
    _no_capture(mu.device, "q8_observe_w")
    if mu.shape != rho.shape or mu.dim() < 2 or stats.numel() < 10:
        raise RuntimeError("q8_observe_w: mu and rho must be two tensors of one shape [Co, Ci, ...] and stats must hold 10 values")
    rows, inner = mu.shape[0], mu.shape[1]
    taps = math.prod(mu.shape[2:])
    if eps is not None and eps.numel() != S * mu.numel():
        raise RuntimeError(f"q8_observe_w: eps holds {eps.numel()} elements, S={S} samples of {mu.numel()} weights need {S * mu.numel()}")
    if coef is not None and coef.numel() != rows:
        raise RuntimeError(f"q8_observe_w: coef must hold {rows} values")
    R = _rng(seed, call, layer_id, sample0, call_base)
    with _lib.on(mu.device):
        _lib.check(_lib.lib().bt_q8_observe_w(mu.data_ptr(), rho.data_ptr(), _lib.ptr(coef), rows, inner, taps, S, _lib.ptr(eps), None if eps is not None else C.byref(R),
                                              stats.data_ptr(), nonfinite.data_ptr(), _lib.stream_ptr(mu.device)))


def minmax_update(segments, nonfinite):
    """The activation-side observers (bt_minmax_update): ``segments`` is a list of up to four (x, dst) -- x an fp32 device tensor,
    dst a 2-element fp32 view ((min, max), e.g. one row of a ``calib_minmax``) its range is merged into -- in ONE launch."""
    if not 1 <= len(segments) <= _lib.MINMAX_MAX_SEGS:
        raise RuntimeError(f"minmax_update: 1 to {_lib.MINMAX_MAX_SEGS} segments")
    _calib_dev(nonfinite, "nonfinite", torch.int32)
    keep = []
    for x, dst in segments:
        x = _lib.dev_f32(x, "x")
        _calib_dev(dst, "dst", torch.float32)
        if dst.numel() != 2 or x.numel() == 0 or x.device != nonfinite.device or dst.device != nonfinite.device:
            raise RuntimeError("minmax_update: x must be a non-empty tensor and dst a (min, max) pair, all on the counter's device")
        keep.append((x, dst))
    dev = nonfinite.device
    _no_capture(dev, "minmax_update")
    arr = (_lib.bt_minmax_seg * len(keep))(*[_lib.bt_minmax_seg(x.data_ptr(), x.numel(), dst.data_ptr()) for x, dst in keep])
    with _lib.on(dev):
        _lib.check(_lib.lib().bt_minmax_update(len(keep), arr, nonfinite.data_ptr(), _lib.stream_ptr(dev)))


def _pair(t, what):
    _calib_dev(t, what, torch.float32)
    if t.numel() != 2:
        raise RuntimeError(f"{what} must be a (min, max) pair")
    return t.data_ptr()


def q8_flip_observe_x(x, in_mm, sign_in_mm, xp_mm, nonfinite, *, S=1, shared_x=True, sign_in=None, seed=0, call=0, layer_id=0, sample0=0, call_base=None):
    """The input-side observers of a calibrating Flipout layer (bt_q8_flip_observe_x): merge the ranges of x, sign_in and x * sign_in
    over S samples into the three (min, max) pairs. x: one batch shared by the samples, or S stacked ones (``shared_x`` False);
    sign_in: fp32 [S, one sample's x] supplied (negative: -1, anything else +1), or None for the on-chip tensor 2 stream."""
    x, sign_in = _lib.dev_f32(x, "x"), _lib.dev_f32(sign_in, "sign_in")
    _calib_dev(nonfinite, "nonfinite", torch.int32)
    _no_capture(x.device, "q8_flip_observe_x")
    per = 1 if shared_x else S
    if x.numel() == 0 or x.numel() % per:
        raise RuntimeError("q8_flip_observe_x: x must be non-empty and hold S stacked batches when it is not shared")
    n = x.numel() // per
    if sign_in is not None and sign_in.numel() != S * n:
        raise RuntimeError(f"q8_flip_observe_x: sign_in holds {sign_in.numel()} elements, S={S} samples of x need {S * n}")
    R = _rng(seed, call, layer_id, sample0, call_base)
    with _lib.on(x.device):
        _lib.check(_lib.lib().bt_q8_flip_observe_x(n, S, x.data_ptr(), 0 if shared_x else n, _lib.ptr(sign_in), None if sign_in is not None else C.byref(R),
                                                   _pair(in_mm, "in_mm"), _pair(sign_in_mm, "sign_in_mm"), _pair(xp_mm, "xp_mm"), nonfinite.data_ptr(),
                                                   _lib.stream_ptr(x.device)))


def q8_flip_observe(x, mu_w, rho_w, mu_b, rho_b, mean_mm, pert_mm, pert_signed_mm, sign_out_mm, nonfinite, *, conv=None, S=1, shared_x=True, coef=None,
                    shift=None, eps_w=None, eps_b=None, sign_in=None, sign_out=None, seed=0, call=0, layer_id=0, sample0=0, call_base=None):
    """The observing two-contraction launch of a calibrating Flipout layer (bt_q8_flip_observe_conv2d / _linear; include/bt_hip.h):
    ``_fused_forward``'s operands of a Flipout call -- the draws all supplied or all None -- and an optional per-channel coef / shift
    (the BatchNorm to be folded). Merges the ranges of the mean output, the perturbation output, the perturbation output times sign_out
    and sign_out, over every output element of all S samples, into the four (min, max) pairs. Nothing output-sized is written."""
    x = _lib.dev_f32(x, "input")
    dev = x.device
    tens = dict(mu_w=mu_w, rho_w=rho_w, mu_b=mu_b, rho_b=rho_b, eps_w=eps_w, eps_b=eps_b, sign_in=sign_in, sign_out=sign_out, coef=coef, shift=shift)
    _f32_on(dev, tens)
    _calib_dev(nonfinite, "nonfinite", torch.int32)
    _no_capture(dev, "q8_flip_observe")
    B, geom, x_elems, tail = _geometry(x, mu_w, conv, S, shared_x)
    n_so, Co = B * math.prod(tail), mu_w.shape[0]
    for k, n in (("eps_w", S * mu_w.numel()), ("eps_b", S * Co), ("sign_in", S * x_elems), ("sign_out", S * n_so), ("coef", Co), ("shift", Co)):
        if tens[k] is not None and tens[k].numel() != n:
            raise RuntimeError(f"q8_flip_observe: {k} holds {tens[k].numel()} elements, this launch needs {n}")
    P = _lib.bt_params(tens["mu_w"].data_ptr(), tens["rho_w"].data_ptr(), _lib.ptr(tens["mu_b"]), _lib.ptr(tens["rho_b"]), None, None, None, None, None, None,
                       _lib.PRIOR_NORMAL, 0)
    D = _lib.bt_draws(_lib.ptr(tens["eps_w"]), _lib.ptr(tens["eps_b"]), _lib.ptr(tens["sign_in"]), _lib.ptr(tens["sign_out"]),
                      _rng(seed, call, layer_id, sample0, call_base))
    tail_args = (S, x.data_ptr(), 0 if shared_x else x_elems, C.byref(P), C.byref(D), _lib.ptr(tens["coef"]), _lib.ptr(tens["shift"]), _pair(mean_mm, "mean_mm"),
                 _pair(pert_mm, "pert_mm"), _pair(pert_signed_mm, "pert_signed_mm"), _pair(sign_out_mm, "sign_out_mm"), nonfinite.data_ptr(), _lib.stream_ptr(dev))
    L = _lib.lib()
    with _lib.on(dev):
        _lib.check(L.bt_q8_flip_observe_linear(B, geom.Ci, geom.Co, *tail_args) if conv is None else L.bt_q8_flip_observe_conv2d(C.byref(geom), *tail_args))
