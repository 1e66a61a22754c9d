"""The instantiation ledger (tests/golden/instantiation_cases.json, recorded by tools/find_instantiation_cases.py) as the tests read it,
and the one launch + fp64 reference a ledger case stands for. A plain module (no fixtures, no pytest hooks), shared by
test_instantiation_ledger_host.py (CPU: every row replans to its own name) and test_gpu_every_instantiation.py (GPU: every row runs).

``run_case`` builds the case's inputs from a seed taken from the kernel name (random x, mu, bias; rho spread over [-5.5, 0.5], so that
a wrong tap order, channel offset or sigma index changes the result), drives the launch through the public functional entry point with
the case's knobs (restored in ``finally``), holds the kernel name the real launch reports to the row's, the result buffer's guard
bands (tests/_guard.py), and every element of every sample to oracle/bt_oracle.py in float64 on the draws that were used -- at the
judgement the project already applies to the variant (``judge``)."""
import contextlib
import ctypes as C
import functools
import importlib.util
import json
import os
import zlib

import torch

import _guard as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-4, 1e-5      # test_gpu_split.py's, the project's output tolerance (conftest.assert_close)
SEED, CALL, LAYER, SAMPLE0 = 77, 2, 9, 5
TAGS = ("min", "ragged", "edge")


@functools.lru_cache(maxsize=None)
def finder():
    spec = importlib.util.spec_from_file_location("find_instantiation_cases", os.path.join(ROOT, "tools", "find_instantiation_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def ledger():
    with open(os.path.join(ROOT, "tests", "golden", "instantiation_cases.json")) as f:
        return json.load(f)


def cases_of(row):
    """[(tag, case)] of a ledger row: min, and ragged / edge where it has one."""
    return [(t, row[t]) for t in TAGS if row.get(t) is not None]


# ---------------------------------------------------------------------------------------------------------------- inputs
def _shapes(c):
    """-> (one sample's x shape, weight shape, the launch's output shape before any pooling, conv dict or None)."""
    fd = finder()
    B, Ci, Co, k, H = c["B"], c["Ci"], c["Co"], c["k"], c["H"]
    if c["entry"] == "linear" or k == 0:
        return (B, Ci), (Co, Ci), (B, Co), None
    Ho = fd.out_hw(c)
    conv = dict(stride=(c["st"],) * 2, padding=(c["pad"],) * 2, dilation=(1, 1), groups=1)
    if c["entry"] == "updil":
        conv.update(updil=tuple(fd.UPDIL[:2]), pads=tuple(fd.UPDIL[2:]))
    if c["dwin"] is not None:
        kd, D = c["dwin"][:2]
        conv.update(dwin=tuple(c["dwin"]))
        return (B, Ci * D, H, H), (Co, Ci * kd, k, k), (B * fd.depth_out(c), Co, Ho, Ho), conv
    return (B, Ci, H, H), (Co, Ci, k, k), (B, Co, Ho, Ho), conv


def make_inputs(name, tag, c):
    """Deterministic CPU tensors of a case, seeded from the kernel name."""
    g = torch.Generator().manual_seed(zlib.crc32(f"{name} {tag}".encode()) & 0x7FFFFFFF)
    rn = lambda *s: torch.randn(*s, generator=g)
    rho = lambda *s: torch.rand(*s, generator=g) * 6.0 - 5.5
    xs, ws, os_, conv = _shapes(c)
    S, Co = c["S"], c["Co"]
    t = dict(x=rn(*(((S if c["per_sample_x"] else 1) * xs[0],) + xs[1:])), mu_w=rn(*ws) * 0.1, rho_w=rho(*ws), mu_b=None, rho_b=None)
    if c["bias"]:
        t.update(mu_b=rn(Co) * 0.1, rho_b=rho(Co))
    d = None
    if c["draws"] != "chip":      # a supplied draw
        sg = lambda *s: torch.where(rn(*s) < 0, -1.0, 1.0)
        d = dict(eps_w=rn(S, *ws), eps_b=rn(S, Co) if c["bias"] else None, sign_in=sg(S, *xs) if c["flip"] else None, sign_out=sg(S, *os_) if c["flip"] else None)
    if c["entry"] == "lowrank":
        R = finder().LOWRANK_R
        n = t["mu_w"].numel()
        t.update(L=rn(n, R) * 0.05, d=0.01)
        if d is not None:
            d["z"] = rn(S, R)
    return t, d, (xs, ws, os_, conv)


@contextlib.contextmanager
def knobs(c):
    """The process-wide knobs of a case, every one restored on exit."""
    from bayesian_torch_amd import _lib
    L, h = _lib.lib(), C.CDLL(_lib.LIB_PATH)
    h.bt_debug_force_bn32.argtypes = [C.c_int]
    h.bt_debug_force_generic.argtypes = [C.c_int]
    mode, spw = L.bt_get_contraction(), os.environ.get("BT_QUAD_SPW")
    try:
        _lib.check(L.bt_set_contraction(c["mode"]))
        h.bt_debug_force_bn32(c["bn32"])
        h.bt_debug_force_generic(c["generic"])
        if c["spw"] is None:
            os.environ.pop("BT_QUAD_SPW", None)
        else:
            os.environ["BT_QUAD_SPW"] = str(c["spw"])
        yield
    finally:
        L.bt_set_contraction(mode)
        h.bt_debug_force_bn32(-1)
        h.bt_debug_force_generic(1 if os.environ.get("BT_FORCE_GENERIC") is not None else 0)
        if spw is None:
            os.environ.pop("BT_QUAD_SPW", None)
        else:
            os.environ["BT_QUAD_SPW"] = spw


# ---------------------------------------------------------------------------------------------------------------- the launch
def launch(c, t, d, shp, dev):
    """One launch of the case -> (out on the CPU or the observer's [4, 2] statistics, kernel name, the draws used, on the CPU)."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    xs, ws, os_, conv = shp
    S, flip, bias = c["S"], c["flip"], c["bias"]
    on = lambda v: None if v is None else v.to(dev).contiguous()
    x = G.place(t["x"].to(dev), c["x_off"] // 4) if c["x_off"] else on(t["x"])
    at = dict(seed=SEED, call=CALL, layer_id=LAYER, sample0=SAMPLE0)
    sup = {} if d is None else {k: on(v) for k, v in d.items()}
    stats = None
    with knobs(c), G.guarded_allocations(0) as log:
        if c["entry"] == "lowrank":
            out = F.lowrank_conv2d(x, on(t["mu_w"].reshape(-1)), on(t["L"]), t["d"], ws, conv, S=S, shared_x=not c["per_sample_x"], z=sup.get("z"), eps_w=sup.get("eps_w"), **at)
        elif c["entry"] == "obs":
            stats = G.place_result((4, 2), 0, device=dev, tag="stats")
            stats.view[:, 0], stats.view[:, 1] = float("inf"), -float("inf")
            bad = torch.zeros(1, dtype=torch.int32, device=dev)
            F.q8_flip_observe(x, on(t["mu_w"]), on(t["rho_w"]), on(t["mu_b"]), on(t["rho_b"]), *[stats.view[i] for i in range(4)], bad, conv=conv, S=S,
                              shared_x=not c["per_sample_x"], **sup, **at)
            out = None
        else:
            mu, rho = on(t["mu_w"]), on(t["rho_w"])
            r = F.fused_forward(x, mu, rho, on(t["mu_b"]), on(t["rho_b"]), flip=flip, conv=conv, S=S, shared_x=not c["per_sample_x"], pool=c["pool"],
                                packed=F.pack_params(mu, rho) if c["packs"] else None, inject_path={"packed": "split", "natural": "general"}.get(c["draws"]),
                                eps_pack_state={} if c["draws"] == "packed" else None, **sup, **at)
            assert r is not None, "the library declined the launch"
            out = r[0]
        name = _lib.lib().bt_last_kernel_name().decode()
        torch.cuda.synchronize()
        # nothing written outside any buffer the call allocated; every element of the result written
        G.check_all(log, body=lambda b: out is not None and b.view.data_ptr() == out.data_ptr())
        if stats is not None:
            G.check(stats, body=True)
            assert int(bad) == 0
    if d is None:      # the on-chip draws, regenerated from the launch's coordinates
        fill = lambda tid, shape: F.rng_fill_normal(SEED, CALL, LAYER, SAMPLE0, tid, S, shape, dev).cpu()
        sign = lambda tid, shape: F.rng_fill_sign(SEED, CALL, LAYER, SAMPLE0, tid, S, shape, dev).cpu()
        d = dict(eps_w=fill(0, ws), eps_b=fill(1, (c["Co"],)) if bias else None, sign_in=sign(2, xs) if flip else None, sign_out=sign(3, os_) if flip else None)
        if c["entry"] == "lowrank":
            d["z"] = fill(4, (t["L"].shape[1],))
    return (stats.view.cpu() if out is None else out.cpu()), name, d


# ---------------------------------------------------------------------------------------------------------------- the reference
def _materialise(c, x):
    """The image an input-dilated launch convolves."""
    if c["entry"] != "updil":
        return x
    uh, uw, lh, hh, lw, hw = finder().UPDIL
    H, W = x.shape[-2:]
    up = torch.zeros(x.shape[:-2] + ((H - 1) * uh + 1 + lh + hh, (W - 1) * uw + 1 + lw + hw), dtype=x.dtype)
    up[..., lh:lh + (H - 1) * uh + 1:uh, lw:lw + (W - 1) * uw + 1:uw] = x
    return up


def _volume(c, shp):
    """A depth-window case as the Conv3d it is: (x / sign_in -> [B, Ci, D, H, W], weight-shaped -> [Co, Ci, kd, kh, kw], the Conv3d's
    output -> the launch's [B * Do, Co, Ho, Wo], sign_out -> the Conv3d's layout, the conv3d dict)."""
    xs, ws, os_, _ = shp
    kd, D, sd, dd, pd = c["dwin"]
    B, Ci, Co, k, H = c["B"], c["Ci"], c["Co"], c["k"], c["H"]
    Do = os_[0] // B
    conv = dict(stride=(sd, c["st"], c["st"]), padding=(pd, c["pad"], c["pad"]), dilation=(dd, 1, 1), groups=1)
    return (lambda x: x.reshape(-1, Ci, D, H, H), lambda w: w.reshape(Co, Ci, kd, k, k), lambda o: o.permute(0, 2, 1, 3, 4).reshape(os_),
            lambda so: so.reshape(B, Do, Co, os_[2], os_[3]).permute(0, 2, 1, 3, 4), conv)


def references(c, t, d, shp, w_s=None):
    """fp64 oracle outputs of every sample, [S * B', ...] in the launch's layout. w_s [S, *w]: contract x with these weights instead of
    the sampled ones (the bf16 mode's rounded operands, the magnitude bound): no draw, and the bias only where ``w_s`` is a dict with it."""
    from oracle import bt_oracle as O
    xs, ws, os_, conv = shp
    S, B, flip = c["S"], xs[0], c["flip"]
    f = lambda v: None if v is None else v.double()
    oconv = None if conv is None else {k: conv[k] for k in ("stride", "padding", "dilation", "groups")}
    vx = vw = vo = vso = lambda v: v
    if c["dwin"] is not None:
        vx, vw, vo, vso, oconv = _volume(c, shp)
    outs = []
    for s in range(S):
        x = f(t["x"][s * B:(s + 1) * B] if c["per_sample_x"] else t["x"])
        eb = None if d is None or d.get("eps_b") is None else f(d["eps_b"][s])
        if w_s is not None:
            ref = O._contract(vx(_materialise(c, x)), vw(f(w_s["w"][s])), w_s.get("b", [None] * S)[s], oconv)
        elif flip:
            ref = O.flipout_fwd_ref(vx(_materialise(c, x)), vw(f(t["mu_w"])), vw(f(t["rho_w"])), vw(f(d["eps_w"][s])), vx(_materialise(c, f(d["sign_in"][s]))),
                                    vso(f(d["sign_out"][s])), f(t["mu_b"]), f(t["rho_b"]), eb, oconv)
        else:
            ref = O.reparam_fwd_ref(vx(_materialise(c, x)), vw(f(t["mu_w"])), vw(f(t["rho_w"])), vw(f(d["eps_w"][s])), f(t["mu_b"]), f(t["rho_b"]), eb, oconv)
        ref = vo(ref)
        if c["pool"]:
            ref = torch.nn.functional.max_pool2d(ref, 3, 2, 1)
        outs.append(ref)
    return torch.stack(outs)


# ---------------------------------------------------------------------------------------------------------------- the judgement
def judge(name, tag, c, t, d, shp, got, dev):
    """The project's judgement of the variant ``name`` states, on every sample and every element."""
    from conftest import assert_close
    from bayesian_torch_amd import functional as F
    xs, ws, os_, conv = shp
    S = c["S"]
    what = f"{name} [{tag}]"
    if c["entry"] == "obs":      # the calibration case module's reference and tolerances: the four activation rows of the launch
        import _q8cal_flip_cases as KF
        want, mags = KF.host_stats(t["x"], t["mu_w"], t["rho_w"], d["eps_w"], d["sign_in"], d["sign_out"], t["mu_b"], t["rho_b"], d["eps_b"], conv, None, None,
                                   not c["per_sample_x"])
        rows = ("mean", "pert", "pert_signed", "sign_out")
        stats = torch.zeros(len(KF.ROWS), 2, dtype=got.dtype)
        stats[[KF.ROWS.index(r) for r in rows]] = got
        KF.check_rows(stats, want, mags, what, rows=rows)
        return
    o = got.reshape((S, -1) + tuple(got.shape[1:]))
    if c["entry"] == "lowrank":      # tests/_lowrank_ref.py's reference at test_gpu_lowrank.py's tolerance
        import _lowrank_ref as R
        ctor = dict(out_channels=c["Co"], in_channels=c["Ci"], kernel_size=c["k"], stride=c["st"], padding=c["pad"])
        ref = R.forward(t["x"], t["mu_w"].reshape(-1), t["L"], torch.full((t["L"].shape[0],), t["d"]), d["z"], d["eps_w"].reshape(S, -1), ctor, not c["per_sample_x"])
        assert_close(got, ref, RTOL, ATOL, what)
        return
    exact = references(c, t, d, shp)
    assert o.shape == exact.shape, (what, tuple(o.shape), tuple(exact.shape))
    if "bf16x1" in name:
        # test_gpu_bf16_mode.py::_check_against_oracles, on every image: the oracle on operands rounded once to bf16 (w_s = mu + sigma * eps in
        # fp32, in the kernel's operation order, from the sigma the kernels read) at the unchanged tolerance, and the distance to the
        # unrounded oracle within 1.01 * 2^lg * (|x| conv |W_s|) + atol. That module's short-K rule: 2^-8 is the typical size of a
        # doubly rounded product and holds where the errors of >= 24 comparable products average; a row without that averaging is held to
        # the worst case (1 + 2^-8)^2 - 1 < 1.01 * 2^-7, which no correct kernel exceeds. The ledger's rows have no such averaging: their
        # rho spreads sigma over two and a half decades, so a handful of products carries an output, and padded borders and one-octet
        # layers meet fewer than 24 to begin with (MI355X, the 256-wide bf16x1 tiles xm=0 / 2 / 3 at 32 products per output: under 1e-7 of
        # max|ref| from the oracle on rounded operands, and 1, 2 and 3 elements past the 2^-8 form, by up to 5.3e-3). Every row is held to
        # the worst-case constant.
        bf = lambda v: v.bfloat16().float()
        Co, Ci = ws[0], ws[1]
        mu_d, rho_d = t["mu_w"].to(dev), t["rho_w"].to(dev)
        sig = F.pack_params(mu_d, rho_d)[1].cpu().reshape(Co, -1, (Ci + 3) // 4 * 4)[:, :, :Ci].permute(0, 2, 1).reshape(ws)
        host = torch.log1p(torch.exp(t["rho_w"]))
        assert float(((sig - host).abs() / host).max()) <= 5e-7, "packed sigma is not the fp32 softplus(rho)"
        w_s = t["mu_w"] + sig * d["eps_w"]
        b64 = None
        if c["bias"]:
            b64 = [t["mu_b"].double() + torch.log1p(torch.exp(t["rho_b"].double())) * d["eps_b"][s].double() for s in range(S)]
        rounded = references(dict(c), dict(t, x=bf(t["x"])), d, shp, w_s=dict(w=bf(w_s), **({} if b64 is None else {"b": b64})))
        mag = references(dict(c), dict(t, x=t["x"].abs()), d, shp, w_s=dict(w=w_s.abs()))
        lg = -7
        for s in range(S):
            print(f"{what}[s={s}]: max |out - rounded oracle| / max|ref| = {float((o[s].double() - rounded[s]).abs().max() / rounded[s].abs().max()):.3e}, "
                  f"max |out - exact oracle| / max|ref| = {float((o[s].double() - exact[s]).abs().max() / exact[s].abs().max()):.3e}")
            assert_close(o[s], rounded[s], RTOL, ATOL, f"{what}[s={s}] bf16 mode vs the oracle on rounded operands")
            over = (o[s].double() - exact[s]).abs() - (1.01 * 2.0 ** lg * mag[s] + ATOL * float(exact[s].abs().max()))
            assert float(over.max()) <= 0.0, f"{what}[s={s}]: {int((over > 0).sum())} elements past 1.01 * 2^{lg} * (|x| conv |W|) + atol, worst by {float(over.max()):.3e}"
    elif "bf16x2" in name:      # test_gpu_split.py::test_three_term_split_is_opt_in_and_coarser's documented window
        for s in range(S):
            err = float((o[s].double() - exact[s]).abs().max() / exact[s].abs().max())
            assert 1e-7 < err < 2e-4, (what, s, err)
    else:
        for s in range(S):
            assert_close(o[s], exact[s], RTOL, ATOL, f"{what}[s={s}]")


def run_case(name, tag, c, dev):
    """The whole check of one ledger case -> the kernel name the launch reported."""
    t, d, shp = make_inputs(name, tag, c)
    got, ran, used = launch(c, t, d, shp, dev)
    key = finder().base.lowrank_key(ran)
    assert key == name, f"[{tag}] planned for {name}, the launch ran {ran}"
    judge(name, tag, c, t, used, shp, got, dev)
    return ran
