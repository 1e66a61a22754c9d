"""Guard bands and misaligned operands on every launch path (tests/_guard.py, tests/_guard_rows.py).

Each launch here takes its operands as interior views of larger NaN-banded buffers, at 0, 4, 8 or 12 bytes past a 16-byte boundary,
and writes into pattern-filled result buffers handed out by the allocation proxy: a write outside a result, an element a launch
skips, and a read outside an operand that is used all fail, none of which a comparison of the result tensor alone can see.  Per
forward row: the guards, the plan (kernel name and launch info equal the plan-only seam's for the same displacement -- the names
themselves are pinned by test_guard_host.py), the fp64 C oracle on the replayed draws at the project's tolerances, and the aligned
launch's bits where the two names are one arithmetic family."""
import ctypes as C

import pytest
import torch

import _grad_cases as GC
import _guard as G
import _guard_rows as GR
from conftest import assert_close

pytestmark = pytest.mark.gpu
RTOL, ATOL, KL_TOL = 1e-4, 1e-5, 1e-5
SEED, CALL, LAYER, SAMPLE0 = 77, 2, 9, 5


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def same_family(a, b):
    """DESIGN's bit-identity promises, read off two kernel names: every tile / fetch mode / channel tile of the split general kernel
    and the direct kernel; the split-K kernel with itself; the fp32 fast and general kernels in one orientation and operand form."""
    def fam(n):
        head, _, args = n.partition("<")
        if head in ("fused_split_kernel", "fused_split_direct_kernel"):
            return ("split", "flip" in args, "bf16x1" in args)
        if head in ("fused_fast_kernel", "fused_fwd_kernel"):
            t = args.split(",")
            return ("fp32", t[3], t[4], t[5])
        return (head, args)
    return fam(a) == fam(b)


# ------------------------------------------------------------------------------------------------------------- forward rows
def _conv_desc(row):
    if row["kind"] == "linear":
        return None
    g = GR.geometry(row)
    conv = dict(stride=(g["st"],) * 2, padding=(g["pad"],) * 2, dilation=(1, 1), groups=1)
    if row["kind"] == "updil":
        conv.update(updil=GR.UPDIL[:2], pads=GR.UPDIL[2:])
    return conv


def _materialise(row, x):
    """The image an input-dilated launch convolves."""
    if row["kind"] != "updil":
        return x
    uh, uw, lh, hh, lw, hw = GR.UPDIL
    H, W = x.shape[-2:]
    up = torch.zeros(x.shape[:-2] + ((H - 1) * uh + 1 + lh + hh, (W - 1) * uw + 1 + lw + hw), dtype=x.dtype)
    up[..., lh:lh + (H - 1) * uh + 1:uh, lw:lw + (W - 1) * uw + 1:uw] = x
    return up


_CASES = {}


def _case(rid):
    """The row's CPU tensors, its replayed draws and its fp64-accumulated reference: computed once, shared, never modified."""
    if rid in _CASES:
        return _CASES[rid]
    from bayesian_torch_amd import functional as F
    from oracle import c_oracle as CO
    row, g = GR.ROWS[rid], GR.geometry(GR.ROWS[rid])
    S, B, flip, bias = row["S"], g["B"], row["flip"], row["bias"]
    gen = torch.Generator().manual_seed(1000 + sorted(GR.ROWS).index(rid))
    rn = lambda *s: torch.randn(*s, generator=gen)
    linear = row["kind"] == "linear"
    wshape = (g["Co"], g["Ci"]) if linear else (g["Co"], g["Ci"], g["k"], g["k"])
    xshape = (B, g["Ci"]) if linear else (B, g["Ci"], g["H"], g["W"])
    oshape = (B, g["Co"]) if linear else (B, g["Co"], g["Ho"], g["Wo"])
    t = dict(mu_w=rn(*wshape) * 0.1, rho_w=rn(*wshape) * 0.1 - 3, x=rn(*(((S if row["stacked"] else 1) * B,) + xshape[1:])))
    if bias:
        t.update(mu_b=rn(g["Co"]) * 0.1, rho_b=rn(g["Co"]) * 0.1 - 3)
    if row["kl"]:
        t.update(prior_mu_w=rn(*wshape) * 0.05, prior_sigma_w=torch.rand(wshape, generator=gen) + 0.5)
        if bias:
            t.update(prior_mu_b=rn(g["Co"]) * 0.05, prior_sigma_b=torch.rand(g["Co"], generator=gen) + 0.5)
    if row["res"]:
        t.update(residual=rn(*((S * B,) + oshape[1:])), post_scale=rn(g["Co"]) * 0.2 + 1, post_shift=rn(g["Co"]) * 0.1)
    dev = _dev()
    d = dict(eps_w=F.rng_fill_normal(SEED, CALL, LAYER, SAMPLE0, 0, S, wshape, dev).cpu())
    if bias:
        d["eps_b"] = F.rng_fill_normal(SEED, CALL, LAYER, SAMPLE0, 1, S, (g["Co"],), dev).cpu()
    if flip:
        d["sign_in"] = F.rng_fill_sign(SEED, CALL, LAYER, SAMPLE0, 2, S, xshape, dev).cpu()
        d["sign_out"] = F.rng_fill_sign(SEED, CALL, LAYER, SAMPLE0, 3, S, oshape, dev).cpu()
    conv = _conv_desc(row)
    oconv = None if conv is None else {k: conv[k] for k in ("stride", "padding", "dilation", "groups")}
    refs = []
    for s in range(S):
        xs = t["x"][s * B:(s + 1) * B] if row["stacked"] else t["x"]
        eb = d["eps_b"][s] if bias else None
        if flip:
            ref = CO.flipout_fwd(_materialise(row, xs), t["mu_w"], t["rho_w"], d["eps_w"][s], _materialise(row, d["sign_in"][s]), d["sign_out"][s],
                                 t.get("mu_b"), t.get("rho_b"), eb, oconv)
        elif row["mode"] == 3:
            # the bf16 mode is held to the oracle on ROUNDED operands (test_gpu_bf16_mode.py): x and w = mu + sigma * eps, the product
            # rounded, then the sum, sigma the packed fp32 softplus -- each rounded once to bf16, at the unchanged tolerance
            sig = F.pack_params(t["mu_w"].to(dev), t["rho_w"].to(dev))[1].cpu()[:, :, :g["Ci"]].permute(0, 2, 1).reshape(wshape)
            w_s = t["mu_w"] + sig * d["eps_w"][s]
            ref = CO.reparam_fwd(xs.bfloat16().float(), w_s.bfloat16().float(), t["rho_w"], torch.zeros_like(w_s), t.get("mu_b"), t.get("rho_b"), eb, oconv)
        else:
            ref = CO.reparam_fwd(_materialise(row, xs), t["mu_w"], t["rho_w"], d["eps_w"][s], t.get("mu_b"), t.get("rho_b"), eb, oconv)
        ref = ref.double()
        if row["res"]:
            sh = (1, -1) + (1,) * (ref.dim() - 2)
            ref = (ref * t["post_scale"].double().reshape(sh) + t["post_shift"].double().reshape(sh) + t["residual"][s * B:(s + 1) * B].double()).clamp_min(0)
        if row["pool"]:
            ref = torch.nn.functional.max_pool2d(ref, 3, 2, 1)
        refs.append(ref)
    kl = None
    if row["kl"]:
        kl = CO.kl_layer(t["mu_w"], t["rho_w"], t["prior_mu_w"], t["prior_sigma_w"], t.get("mu_b"), t.get("rho_b"), t.get("prior_mu_b"), t.get("prior_sigma_b"))
    _CASES[rid] = (t, d, torch.cat(refs), kl)
    return _CASES[rid]


def _launch(rid, off, which, inject="general"):
    """The row's launch with the operands ``which`` at ``off`` ("out": every buffer functional allocates) -> (out, kl, name, info).
    inject="split": the supplied draws are re-laid into packed images (1-d buffers: kept 16-byte aligned, as the library demands)."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    row = GR.ROWS[rid]
    t, d, _, _ = _case(rid)
    dev = _dev()
    put = lambda k, v: None if v is None else (G.place(v.to(dev), off) if k in which else v.to(dev).contiguous())
    a = {k: put(k, v) for k, v in t.items()}
    if row["nat"]:
        a.update({k: put(k, v) for k, v in d.items()})
    packed = None
    if row["packs"]:
        mp, sp = F.pack_params(t["mu_w"].to(dev), t["rho_w"].to(dev))
        packed = (put("mu_packed", mp), put("sigma_packed", sp))
    priors = (a.get("prior_mu_w"), a.get("prior_sigma_w"), a.get("prior_mu_b"), a.get("prior_sigma_b")) if row["kl"] else None
    geom = _lib.bt_conv2d_geom(*[GR.geometry(row)[k] for k in ("B", "Ci", "H", "W", "Co", "k", "k", "st", "st", "pad", "pad")], 1, 1, 1)
    scratch = int(_lib.lib().bt_fused_scratch_bytes(C.byref(geom), row["S"]))
    _off = off if "out" in which else 0
    if inject == "split":
        _off = lambda shape, dtype, o=_off: 0 if len(shape) == 1 else o
    _lib.check(_lib.lib().bt_set_contraction(row["mode"]))
    try:
        with G.seated_workspace("functional", dev, scratch) as ws, G.guarded_allocations(_off) as log:
            r = F.fused_forward(a["x"], a["mu_w"], a["rho_w"], a.get("mu_b"), a.get("rho_b"), flip=row["flip"], conv=_conv_desc(row), S=row["S"],
                                shared_x=not row["stacked"], priors=priors, eps_w=a.get("eps_w"), eps_b=a.get("eps_b"), sign_in=a.get("sign_in"),
                                sign_out=a.get("sign_out"), seed=SEED, call=CALL, layer_id=LAYER, sample0=SAMPLE0, want_kl=row["kl"],
                                post_scale=a.get("post_scale"), post_shift=a.get("post_shift"), residual=a.get("residual"), relu=row["res"],
                                packed=packed, pool=row["pool"], inject_path=inject, eps_pack_state={} if inject == "split" else None)
            assert r is not None, "the library declined the launch"
            name, info = _lib.lib().bt_last_kernel_name().decode(), _lib.last_launch_info()
            torch.cuda.synchronize()
            # (a fused pool the library declines leaves its pooled buffer behind: functional runs the launch again unpooled,
            # and is never written: its bands alone are held)
            declined = lambda b: row["pool"] and b.view.data_ptr() != r[0].data_ptr() and b.view.shape == r[0].shape
            G.check_all(log, body=lambda b: b.view.dtype == torch.float32 and not declined(b))
            # the launch used the seated workspace: _lib.workspace swaps in a fresh buffer when a call asks for more than was seated
            assert _lib._ws[("functional", dev.index)] is ws.view
            G.check_workspace(ws)
    finally:
        _lib.lib().bt_set_contraction(0)
    return r[0], r[1], name, info


def _variants(row):
    """(operands displaced, off): every operand alone and all together, at off 1, 2 and 3; the result buffers alone likewise."""
    ops = row["ops"]
    singles = [((op,), off) for op in ops + ("out",) for off in (1, 2, 3)]
    together = [(ops + ("out",), off) for off in (1, 2, 3)] if ops else []
    return singles + together


@pytest.mark.parametrize("rid", list(GR.ROWS))
def test_forward_row(rid):
    row = GR.ROWS[rid]
    t, d, ref, kl_ref = _case(rid)
    seam = GR.Seam()
    out0, kl0, name0, info0 = _launch(rid, 0, ())
    rc, pname, pinfo = seam.plan(row, 0, ())
    if row["walk"]:     # planned from the CU count: the seam (and the table) name its one-sample twin
        assert rc == 0 and "walk" in name0 and name0.startswith(row["aligned"].split(",pool=")[0]) and "pool=1" in name0, (rid, name0, pname)
    else:
        assert (rc, name0, info0) == (0, pname, pinfo) and (name0, GR.info_of(info0)) == (row["aligned"], row["info"]), (rid, name0, pname, info0)
    assert_close(out0, ref, RTOL, ATOL, f"{rid} aligned vs C oracle")
    if row["kl"]:
        assert abs(float(kl0) - kl_ref) <= KL_TOL * abs(kl_ref), (rid, float(kl0), kl_ref)
    for which, off in _variants(row):
        tag = f"{rid} {'+'.join(which)} @{off}"
        out, kl, name, info = _launch(rid, off, which)
        rc, pname, pinfo = seam.plan(row, off, which)
        if rc == 0 and row["walk"]:
            assert "walk" in name and "pool=1" in name, (tag, name)
        elif rc == 0:
            assert (name, info) == (pname, pinfo), (tag, name, pname, info, pinfo)
            if len(which) == 1:     # the table's own statement of this displaced launch
                assert (name, GR.info_of(info)) == (row["single"].get(which[0], row["aligned"]), row["single_info"].get(which[0], row["info"])), (tag, name, info)
        else:       # the fused pool declined (BT_ERR_UNSUPPORTED, nothing launched): the unpooled launch and the pooling pass
            assert row["pool"] and "fused max-pool" in pname, (tag, pname)
            rc, pname, pinfo = seam.plan(dict(row, pool=False), off, which)
            assert rc == 0 and name == pname, (tag, name, pname)
        assert_close(out, ref, RTOL, ATOL, tag + " vs C oracle")
        if row["kl"]:
            assert abs(float(kl) - kl_ref) <= KL_TOL * abs(kl_ref), (tag, float(kl), kl_ref)
        if same_family(name, name0):
            assert torch.equal(out, out0), f"{tag}: {name} differs from the aligned {name0} at {int((out != out0).sum())} of {out.numel()} elements"


@pytest.mark.parametrize("rid", ["n_r", "n_f"])
def test_packed_supplied_draws_with_guarded_pack_buffers(rid):
    """inject_path="split": bt_pack_eps / bt_pack_signs write the packed images into guarded buffers, the split kernel reads them and
    writes a guarded, displaced result: the oracle on the same draws, and the bits of the launch at off 0."""
    t, d, ref, _ = _case(rid)
    base = None
    for off in (0, 1, 2, 3):
        which = ("out", "eps_w", "x") if off else ()
        out, _, name, _ = _launch(rid, off, which, inject="split")
        assert name.startswith("fused_split_kernel<"), name
        assert_close(out, ref, RTOL, ATOL, f"{rid} packed draws @{off} vs C oracle")
        base = out if base is None else base
        assert torch.equal(out, base), (rid, off)


# ------------------------------------------------------------------------------------------------------------- backward rows
BWD_ROWS = ("A", "C", "E", "F", "G")


def _bwd_case(row_id):
    from bayesian_torch_amd import functional as F
    _, cls, ctor, xshape, S = GC.DRAW_ROW[row_id]
    flip, linear = "Flipout" in cls, cls.startswith("Linear")
    gen = torch.Generator().manual_seed(50 + ord(row_id))
    rn = lambda *s: torch.randn(*s, generator=gen)
    B = xshape[0]
    if linear:
        wshape, conv = (ctor["out_features"], ctor["in_features"]), None
    else:
        pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        k, grp = pair(ctor["kernel_size"]), ctor.get("groups", 1)
        wshape = (ctor["out_channels"], ctor["in_channels"] // grp) + k
        conv = dict(stride=pair(ctor.get("stride", 1)), padding=pair(ctor.get("padding", 0)), dilation=pair(ctor.get("dilation", 1)), groups=grp)
    mu, rho, x = rn(*wshape) * 0.1, rn(*wshape) * 0.1 - 3, rn(*xshape)
    if linear:
        oshape = (B, wshape[0])
    else:
        Ho, Wo = F.conv_out_hw(xshape[2], xshape[3], *wshape[2:], *conv["stride"], *conv["padding"], *conv["dilation"])
        oshape = (B, wshape[0], Ho, Wo)
    gout = rn(S * B, *oshape[1:])
    dev = _dev()
    d = dict(eps_w=F.rng_fill_normal(SEED, CALL, LAYER, SAMPLE0, 0, S, wshape, dev).cpu())
    if flip:
        d["sign_in"] = F.rng_fill_sign(SEED, CALL, LAYER, SAMPLE0, 2, S, xshape, dev).cpu()
        d["sign_out"] = F.rng_fill_sign(SEED, CALL, LAYER, SAMPLE0, 3, S, oshape, dev).cpu()
    _, gx, gp = GC.oracle_grads(flip, dict(mu_w=mu, rho_w=rho, mu_b=None, rho_b=None), x, d, conv, gout, S, True)
    return dict(flip=flip, conv=conv, S=S, mu=mu, rho=rho, x=x, gout=gout, draws=d, ref=(gx, gp["mu_w"], gp["rho_w"]))


def _bwd_launch(c, off, which, supplied, kl=None):
    from bayesian_torch_amd import functional as F
    dev = _dev()
    put = lambda k, v: G.place(v.to(dev), off) if k in which else v.to(dev).contiguous()
    mu, rho = c["mu"].to(dev), c["rho"].to(dev)
    packed = F.pack_params(mu, rho)
    dr = {k: put(k, v) for k, v in c["draws"].items()} if supplied else {}
    with G.guarded_allocations(off if "out" in which else 0) as log:
        got = F.fused_backward(put("x", c["x"]), put("grad_out", c["gout"]), mu, rho, packed, flip=c["flip"], conv=c["conv"], S=c["S"], shared_x=True,
                               eps_w=dr.get("eps_w"), sign_in=dr.get("sign_in"), sign_out=dr.get("sign_out"), seed=SEED, call=CALL, layer_id=LAYER,
                               sample0=SAMPLE0, kl=kl)
        torch.cuda.synchronize()
        # dx [S, B, ...], dmu, drho: every element written; the byte workspace ("contents need not be initialised"): its bands alone
        f32 = [b for b in log if b.view.dtype == torch.float32]
        assert sum(tuple(b.view.shape) == tuple(mu.shape) for b in f32) == 2 and sum(tuple(b.view.shape) == (c["S"],) + tuple(c["x"].shape) for b in f32) == 1
        assert len(f32) == 3 and [b.view.dtype for b in log if b not in f32] == [torch.uint8]
        G.check_all(log)
    return got


@pytest.mark.parametrize("row_id", BWD_ROWS)
def test_backward_row(row_id):
    c = _bwd_case(row_id)
    base = _bwd_launch(c, 0, (), False)
    names = ("dx", "dmu_w", "drho_w")
    for g, ref, nm in zip(base, c["ref"], names):
        assert_close(g, ref, *((1e-4, 1e-5) if nm == "dx" else (2e-4, 2e-5)), f"row {row_id} aligned {nm}")
    ops = ("x", "grad_out") + tuple(c["draws"])
    for which, off, supplied in [((op,), 1 + i % 3, op in c["draws"]) for i, op in enumerate(ops)] + [(("out",), o, False) for o in (1, 2, 3)] + \
            [(ops + ("out",), o, True) for o in (1, 2, 3)]:
        got = _bwd_launch(c, off, which, supplied)
        for g, b, ref, nm in zip(got, base, c["ref"], names):
            tag = f"row {row_id} {'+'.join(which)} @{off} {nm}"
            assert_close(g, ref, *((1e-4, 1e-5) if nm == "dx" else (2e-4, 2e-5)), tag)
            assert torch.equal(g, b), f"{tag}: differs from the aligned launch at {int((g != b).sum())} of {g.numel()} elements"


def test_backward_row_with_the_kl_term_and_misaligned_priors():
    c = _bwd_case("A")
    dev = _dev()
    gen = torch.Generator().manual_seed(5)
    pm, ps = torch.randn(c["mu"].shape, generator=gen) * 0.05, torch.rand(c["mu"].shape, generator=gen) + 0.5
    gk = torch.tensor(GC.KL_G, device=dev)
    kref = GC.kl_grad_ref("normal", c["mu"], c["rho"], pm, ps, torch.float64)
    base = _bwd_launch(c, 0, (), False, kl=(gk, pm.to(dev), ps.to(dev), "normal"))
    for off in (1, 2, 3):
        got = _bwd_launch(c, off, ("x", "grad_out", "out"), False, kl=(gk, G.place(pm.to(dev), off), G.place(ps.to(dev), off), "normal"))
        for g, b, ref, kr, nm in zip(got[1:], base[1:], c["ref"][1:], kref, ("dmu_w", "drho_w")):
            assert_close(g, ref + kr, 2e-4, 2e-5, f"kl row @{off} {nm}")
            assert torch.equal(g, b), (off, nm)


def test_backward_refuses_misaligned_packs():
    from bayesian_torch_amd import functional as F
    c = _bwd_case("A")
    dev = _dev()
    mu, rho = c["mu"].to(dev), c["rho"].to(dev)
    mp, sp = F.pack_params(mu, rho)
    with pytest.raises(RuntimeError, match="mu_packed / sigma_packed must be 16-byte aligned"):
        F.fused_backward(c["x"].to(dev), c["gout"].to(dev), mu, rho, (G.place(mp, 1), sp), flip=c["flip"], conv=c["conv"], S=c["S"])


@pytest.mark.parametrize("off", (0, 1, 2, 3))
def test_kl_backward_kernels_with_guarded_outputs(off):
    from bayesian_torch_amd import functional as F
    dev = _dev()
    t, ref = GC.kl_slice_ref(0, 3, 1029)
    a = {k: G.place(v.to(dev), off) for k, v in t.items()}
    gk = torch.tensor(GC.KL_G, device=dev)
    lim = GC.kl_limits(0)
    with G.guarded_allocations(off) as log:
        one = F.kl_backward(a["mu"], a["rho"], a["pmu"], a["psig"], gk)
        segs = F.kl_backward_segs([(a["mu"], a["rho"], a["pmu"], a["psig"]), (a["mu"][:5], a["rho"][:5], a["pmu"][:5], a["psig"][:5])], gk)
        torch.cuda.synchronize()
        G.check_all(log)
    for got in (one, segs[0]):
        err = GC.kl_errors("normal", t["mu"], t["rho"], t["psig"], got, ref)
        assert err["dmu"] <= lim["dmu"] and err["drho"] <= lim["drho"], (off, err, lim)
    assert torch.equal(one[0], segs[0][0]) and torch.equal(one[1], segs[0][1])


# ------------------------------------------------------------------------------------------------------------- helpers
@pytest.mark.parametrize("off", (0, 1, 2, 3))
def test_pack_params_and_pack_sync_with_displaced_parameters(off):
    from bayesian_torch_amd import functional as F
    dev = _dev()
    gen = torch.Generator().manual_seed(9)
    for Co, Ci, k in ((20, 6, 3), (16, 8, 1), (5, 3, 2)):      # Ci % 4 != 0: padded lanes
        mu, rho = torch.randn(Co, Ci, k, k, generator=gen) * 0.1, torch.randn(Co, Ci, k, k, generator=gen) * 0.1 - 3
        C4 = (Ci + 3) // 4 * 4
        want_mu = torch.zeros(Co, k * k, C4)
        want_mu[:, :, :Ci] = mu.reshape(Co, Ci, k * k).permute(0, 2, 1)
        plain_mu, plain_sig = F.pack_params(mu.to(dev), rho.to(dev))
        m, r = G.place(mu.to(dev), off), G.place(rho.to(dev), off)
        with G.guarded_allocations(off) as log:
            mp, sp = F.pack_params(m, r)
            torch.cuda.synchronize()
            G.check_all(log)
        assert torch.equal(mp.cpu(), want_mu) and torch.equal(mp, plain_mu) and torch.equal(sp, plain_sig)
        assert bool((sp[:, :, Ci:] == 0).all()) and bool((sp[:, :, :Ci] > 0).all())
        # pack_sync: both branches of its sweep's alignment test rebuild the same pack
        # with its KL term (bt_pack_sync_kl: the sweep reads the priors too -- displaced with the parameters), in a seated workspace
        from bayesian_torch_amd import _lib
        from oracle import c_oracle as CO
        pm, ps = torch.randn(mu.shape, generator=gen) * 0.05, torch.rand(mu.shape, generator=gen) + 0.5
        kl_ref = CO.kl_layer(mu, rho, pm, ps)
        for kls in (None, "kl"):
            with G.seated_workspace(("guard", "pack"), dev) as ws, G.guarded_allocations(0) as log:
                mp2, sp2, state = F.pack_buffers(Co, Ci, k * k, dev)
                kl_out = G.place_result((), off, device=dev, tag="kl_out")
                seg = dict(mu=m, rho=r, mu_packed=mp2, sigma_packed=sp2, state=state, Co=Co, Ci=Ci, taps=k * k, force=True)
                F.pack_sync([seg], owner="guard", kls=None if kls is None else [(G.place(pm.to(dev), off), G.place(ps.to(dev), off), None, None, None, None, kl_out.view)])
                torch.cuda.synchronize()
                G.check_all(log)
                assert _lib._ws[(("guard", "pack"), dev.index)] is ws.view
                G.check_workspace(ws)
                if kls is not None:
                    G.check(kl_out)
                    assert abs(float(kl_out.view) - kl_ref) <= KL_TOL * abs(kl_ref), (off, float(kl_out.view), kl_ref)
            assert torch.equal(mp2, mp) and torch.equal(sp2, sp)


@pytest.mark.parametrize("off", (0, 1, 2, 3))
def test_standalone_kl_kernel_leaves_its_seated_workspace_zeroed(off):
    """bt_kl_normal (both branches of its alignment test, normal and Laplace) in a guarded workspace of its own: the head reads zero
    after the call, the result matches the C oracle."""
    from bayesian_torch_amd import _lib
    from oracle import c_oracle as CO
    dev = _dev()
    gen = torch.Generator().manual_seed(21)
    n = 4001
    mu, rho = torch.randn(n, generator=gen) * 0.1, torch.randn(n, generator=gen) * 0.1 - 3
    pm, ps = torch.randn(n, generator=gen) * 0.05, torch.rand(n, generator=gen) + 0.5
    a = [G.place(v.to(dev), off) for v in (mu, rho, pm, ps)]
    for laplace, ref in ((False, CO.kl_normal(mu, rho, pm, ps)), (True, CO.kl_laplace(mu, rho))):
        with G.seated_workspace("guardkl", dev) as ws:
            out = G.place_result((), off, device=dev, tag="kl")
            got = _lib.kl_normal([tuple(a), tuple(v[:1023] for v in a)], layer_ids=[0, 1], out=out.view, owner="guardkl", laplace=laplace)
            one = _lib.kl_normal([tuple(a)], owner="guardkl", laplace=laplace)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.view.data_ptr() and _lib._ws[("guardkl", dev.index)] is ws.view
            G.check(out)
            G.check_workspace(ws)
        assert abs(float(one) - ref) <= KL_TOL * abs(ref), (off, laplace, float(one), ref)
        part = CO.kl_laplace(mu[:1023], rho[:1023]) if laplace else CO.kl_normal(mu[:1023], rho[:1023], pm[:1023], ps[:1023])
        assert abs(float(got) - (ref + part)) <= KL_TOL * abs(ref + part), (off, laplace, float(got), ref + part)


@pytest.mark.parametrize("off", (0, 1, 2, 3))
def test_rng_fills_with_guarded_outputs(off):
    from bayesian_torch_amd import functional as F
    dev = _dev()
    with G.guarded_allocations(off) as log:
        got = [F.rng_fill_normal(SEED, CALL, LAYER, SAMPLE0, 0, 2, shape, dev) for shape in ((5, 6, 3, 3), (7, 130), (9,), (3, 1))]
        got += [F.rng_fill_sign(SEED, CALL, LAYER, SAMPLE0, 2, 2, shape, dev) for shape in ((3, 5, 7, 7), (1,), (4, 129))]
        torch.cuda.synchronize()
        G.check_all(log)
    plain = [F.rng_fill_normal(SEED, CALL, LAYER, SAMPLE0, 0, 2, shape, dev) for shape in ((5, 6, 3, 3), (7, 130), (9,), (3, 1))]
    plain += [F.rng_fill_sign(SEED, CALL, LAYER, SAMPLE0, 2, 2, shape, dev) for shape in ((3, 5, 7, 7), (1,), (4, 129))]
    for a, b in zip(got, plain):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert all(bool((s.abs() == 1).all()) for s in got[4:])


MC_CASES = [(S, 5, 10) for S in (1, 64, 65, 129)] + [(3, 5, C) for C in (1, 64, 65, 257)] + [(3, B, 10) for B in (1, 4, 7)] + [(65, 1, 257), (2, 4, 65)]


@pytest.mark.parametrize("S,B,Cc", MC_CASES)
def test_mc_epilogue_edges_match_oracle(S, B, Cc):
    from bayesian_torch_amd import functional as F
    from oracle import bt_oracle as O
    logits = torch.randn(S, B, Cc, generator=torch.Generator().manual_seed(S * 1000 + B * 10 + Cc)) * 4
    if Cc > 1:
        logits[0, 0, 0] = logits[0, 0].max() - 200.0        # a softmax term that underflows to 0: the p > 0 guard of the entropy
    for off in (0, 1, 2, 3):
        with G.guarded_allocations(off) as log:
            packed = F.mc_epilogue(G.place(logits.to(_dev()), off))
            torch.cuda.synchronize()
            G.check_all(log)
        packed = packed.cpu()
        p, e, l = O.mc_epilogue_ref(logits)
        assert_close(packed[:B * Cc].reshape(B, Cc), p, 1e-5, 1e-6, "psum")
        assert_close(packed[B * Cc:B * Cc + B], e, 1e-5, 1e-6, "entropy")
        assert_close(packed[B * Cc + B:].reshape(B, Cc), l, 1e-5, 1e-6, "lsum")


@pytest.mark.parametrize("H,W", [(1, 1), (1, 8), (8, 1), (7, 7), (8, 8), (5, 6), (6, 5), (4, 12), (3, 16)])
def test_maxpool_pass_with_displaced_input_and_output(H, W):
    from bayesian_torch_amd import functional as F
    x = torch.randn(3, 5, H, W, generator=torch.Generator().manual_seed(H * 100 + W))
    want = torch.nn.functional.max_pool2d(x, 3, 2, 1)
    for off_in in (0, 1, 2, 3):
        for off_out in (0, 1, 2, 3):
            with G.guarded_allocations(off_out) as log:
                got = F.maxpool_3x3s2(G.place(x.to(_dev()), off_in))
                torch.cuda.synchronize()
                G.check_all(log)
            assert torch.equal(got.cpu(), want), (H, W, off_in, off_out)
