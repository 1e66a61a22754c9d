"""Two float64 oracles of the DISTRIBUTION of the on-chip draws as the forward kernels consume them, the statistics that hold a launch
to them, and the row table shared by test_draw_stats_host.py (CPU: the reference arithmetic with torch's own draws stays inside the
bound on every row's inputs, seeded faults fall outside it, every row plans the pinned kernel) and test_gpu_draw_distribution.py (GPU:
the same rows launched).  Nothing here calls rng_fill_* or materialize_last_draw: the parity tests ask "given these draws, is the output
f(x, params, draws)?", these ask "are the draws the kernel consumes one independent N(0,1) per weight and bias element, per sample, per
call and per layer, and do Flipout's signs decorrelate the examples of a batch?".

a. Impulse probe.  mu_w = 0 and every pixel an impulse reaches holds that single 1.0, so an output element is ONE sampled weight
   (plus, with a bias, the bias draw, which an all-zero example reads alone and which is subtracted): e = (out - bias part) / sigma is
   the kernel's standardised draw.  The map output element -> weight element comes from the float64 reference contraction on the same
   x with index-coded weights, and is asserted one-to-one.  Flipout reads s_out * s_in * eps: still N(0,1); every impulse is given to
   two examples, whose |e| must agree and whose signs must agree like a fair coin.  Its bias perturbation sits inside the sign_out
   product (out = mu_b + s_out * (s_in * sigma * eps + sigma_b * eps_b)), so a weight cannot be told from the bias draw in one output:
   the Flipout weight launches run without a bias and an all-zero launch with the bias reads the bias draw at the same coordinates.
b. Dense moments.  x = U(0.5, 1.5) > 0 (a shared draw inflates a variance, it cannot average out), B >= 2, mu != 0.  Reparameterization:
   mean contract(x, mu) + mu_b, covariance J diag(sigma^2) J^T + sigma_b^2 [same channel] over the chosen outputs, J the Jacobian of
   the float64 reference contraction (the rows ``unfold`` lists), cross-example entries included (eps is shared by the batch).  Flipout:
   the same mean, covariance diag(contract(x^2, sigma^2) + sigma_b^2), zero between examples, pixels and channels; its outputs are
   uncorrelated but not independent, so a zero entry's standard error carries the fourth-moment term Q (dense_moments).  At most 512 outputs
   of a launch are held (``choose_outputs``: first / last example, channels and pixels spread over the whole range).

Every statistic is in units of its own standard error over S samples, and the bound is 7.0 for all of them: 2 (1 - Phi(7)) = 2.6e-12
and no row makes more than 1e7 comparisons (corr_max: every pair of a probe's columns, or for the two rows with more than 4472 columns
the pairs that budget buys), a false alarm rate of at most 3e-5 per row; an aliased pair of draws gives sqrt(S) = 32 at
S = 1024.  Seeds are fixed."""
import math

import torch
import torch.nn.functional as TF

import _guard_rows as GR

BOUND = 7.0
CHUNK = 128            # samples per launch; S_total = 1024 is eight launches at sample0 = 0, 128, ...
SEED, CALL, LAYER = 4242, 11, 5
MAX_PAIRS = 10_000_000  # comparisons a row may make: the correlation entries of a probe (corr_max)
F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------- rows
def _row(base, forms, S_total=1024, **kw):
    r = dict(GR.ROWS[base]) if base else GR._row(False, "conv", None, CHUNK)
    r.update(S=CHUNK, bias=True, kl=False, res=False, pool=False, nat=False, stacked=False, walk=False, ops=(), groups=1, dwin=None, W=None, kw=None, padw=None,
             forms=tuple(forms), S_total=S_total)
    r.update(kw)
    return r


# id -> row (the keys of _guard_rows' rows + groups, dwin = (kd, D, sd, dd, pd), W when not H, kw / padw when not k / pad, forms, S_total).  geo = (Ci, Co, k, stride,
# pad, H, B).  The geometries are _guard_rows' own (B and H unchanged: a probe that needs more examples than B takes more launches at the
# same coordinates), f_3x3 is f_256 shrunk to 512 outputs per example, p_grp the [20, 6, 3, 2] groups-2 kernel with padding (1, 0) on 6 x 6 (test_gpu_grad_oracle's), w_a / w_f rows a / f1 of
# test_conv3d_native_host.py as the depth-window launch.
ROWS = {
    "g_packs": _row("g_packs", ("probe", "dense")),
    "g_rowtile": _row("g_rowtile", ("probe", "dense")),
    "g_xm1": _row("g_xm1", ("probe",)),
    "g_bn32": _row("g_bn32", ("probe",)),
    "b_xm1": _row("b_xm1", ("probe",)),
    "g_pchan": _row("g_pchan", ("dense",)),
    "q_r": _row("q_r", ("probe", "dense")),
    "q_f": _row("q_f", ("probe", "dense")),
    "f_xm1": _row("f_xm1", ("probe", "dense")),
    "f_3x3": _row("f_256", ("probe", "dense"), geo=(8, 32, 3, 1, 0, 6, 16)),
    "d_res": _row("d_res", ("probe",)),
    "d_str": _row("d_str", ("probe",), S_total=256),
    "s_64": _row("s_64", ("probe", "dense")),
    "s_128": _row("s_128", ("probe", "dense")),
    "p_rows": _row("p_rows", ("probe", "dense")),
    "p_general": _row("p_general", ("probe", "dense")),
    "p_lin130": _row("p_lin130", ("probe", "dense")),
    "p_grp": _row(None, ("probe", "dense"), geo=(12, 20, 3, 1, 1, 6, 4), kw=2, padw=0, groups=2, mode=1),
    "u_r": _row("u_r", ("dense",)),
    "u_f": _row("u_f", ("dense",)),
    "w_a": _row(None, ("dense",), kind="dwin", geo=(8, 24, 3, 1, 1, 6, 2), W=7, dwin=(3, 5, 1, 1, 2)),
    "w_f": _row(None, ("dense",), kind="dwin", flip=True, geo=(8, 20, 3, 1, 1, 10, 2), dwin=(2, 6, 2, 1, 0)),
}

# The launch every row plans, aligned, at S = CHUNK: (kernel name, _guard_rows.INFO_FIELDS).  The stem rows' GPU launch walks several
# samples per workgroup (planned from the CU count: ",walk" in its name); the table names the one-sample twin, as _guard_rows does.
PINS = {
    "g_packs": ("fused_split_kernel<64,512,bf16x3,6 terms,npw=4,xm=3>", (0, 8, 8, 8, 4, 1, 256)),
    "g_rowtile": ("fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=2>", (1, 64, 1, 2, 2, 1, 256)),
    "g_xm1": ("fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=1>", (0, 128, 1, 1, 1, 1, 128)),
    "g_bn32": ("fused_split_kernel<32,128,bf16x3,6 terms,npw=8,xm=1>", (0, 128, 1, 1, 1, 2, 256)),
    "b_xm1": ("fused_split_kernel<64,128,bf16x1,1 terms,npw=8,xm=1>", (0, 128, 1, 1, 1, 1, 128)),
    "g_pchan": ("fused_split_kernel<64,256,bf16x3,6 terms,npw=8,xm=3>", (0, 4, 8, 8, 2, 1, 256)),
    "q_r": ("fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=0>", (0, 32, 4, 4, 1, 1, 128)),
    "q_f": ("fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=0>", (0, 16, 4, 4, 2, 1, 256)),
    "f_xm1": ("fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=1>", (0, 128, 1, 1, 1, 1, 128)),
    "f_3x3": ("fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=0>", (0, 8, 4, 4, 2, 1, 256)),
    "d_res": ("fused_split_direct_kernel<64,8x64,bf16x3,6 terms,resident W>", (0, 2, 1, 64, 1, 1, 128)),
    "d_str": ("fused_split_direct_kernel<64,8x64,bf16x3,6 terms,streamed W>", (0, 64, 1, 64, 1, 1, 128)),
    "s_64": ("fused_split_skinny_kernel<64,4x32,bf16x3,6 terms,split-K 64>", (0, 128, 1, 1, 1, 1, 128)),
    "s_128": ("fused_split_skinny_kernel<64,4x32,bf16x3,6 terms,split-K 128>", (0, 128, 1, 1, 1, 1, 128)),
    "p_rows": ("fused_fast_kernel<32,128,1,reparam,conv,trans,inj=0,xmode=1,npw=8,pool=0>", (0, 2, 8, 8, 2, 1, 256)),
    "p_general": ("fused_fwd_kernel<32,128,1,reparam,conv,trans,inj=0>", (0, 0, 0, 0, 2, 1, 256)),
    "p_lin130": ("fused_fast_kernel<128,32,4,reparam,conv,trans,inj=0,xmode=0,npw=8,pool=0>", (0, 32, 1, 1, 1, 1, 128)),
    "p_grp": ("fused_fast_kernel<32,128,1,reparam,conv,notrans,inj=0,xmode=0,npw=8,pool=0>", (0, 4, 6, 5, 1, 1, 256)),
    "u_r": ("fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=5>", (0, 2, 8, 8, 2, 1, 256)),
    "u_f": ("fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=5>", (0, 2, 8, 8, 2, 1, 256)),
    "w_a": ("fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=6>", (0, 3, 6, 7, 5, 1, 256)),
    "w_f": ("fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=6>", (0, 1, 10, 10, 6, 1, 256)),
}


def geometry(row):
    """-> dict(B, Ci, H, W, Co, k, kw, st, pad, padw, Ho, Wo, G, and for a depth-window row the REAL x: D, Do; B is then the real batch)."""
    if row["kind"] != "dwin":
        g = GR.geometry(row)
        g["G"] = row["groups"]
        g["kw"], g["padw"] = row["kw"] or g["k"], g["pad"] if row["padw"] is None else row["padw"]
        if row["kind"] == "conv":
            g["Wo"] = (g["W"] + 2 * g["padw"] - g["kw"]) // g["st"] + 1
        return g
    Ci, Co, k, st, pad, H, B = row["geo"]
    W = row["W"] or H
    kd, D, sd, dd, pd = row["dwin"]
    return dict(B=B, Ci=Ci, H=H, W=W, Co=Co, k=k, kw=k, st=st, pad=pad, padw=pad, Ho=(H + 2 * pad - k) // st + 1, Wo=(W + 2 * pad - k) // st + 1, G=row["groups"],
                D=D, Do=(D + 2 * pd - dd * (kd - 1) - 1) // sd + 1)


def shapes(row):
    """-> (x shape as launched, weight shape as launched, one sample's output shape as launched)."""
    g = geometry(row)
    if row["kind"] == "linear":
        return (g["B"], g["Ci"]), (g["Co"], g["Ci"]), (g["B"], g["Co"])
    if row["kind"] == "dwin":
        return ((g["B"], g["Ci"] * g["D"], g["H"], g["W"]), (g["Co"], g["Ci"] // g["G"] * row["dwin"][0], g["k"], g["k"]),
                (g["B"] * g["Do"], g["Co"], g["Ho"], g["Wo"]))
    return (g["B"], g["Ci"], g["H"], g["W"]), (g["Co"], g["Ci"] // g["G"], g["k"], g["kw"]), (g["B"], g["Co"], g["Ho"], g["Wo"])


def conv_desc(row):
    """The ``conv`` argument of functional.fused_forward."""
    if row["kind"] == "linear":
        return None
    g = geometry(row)
    conv = dict(stride=(g["st"],) * 2, padding=(g["pad"], g["padw"]), dilation=(1, 1), groups=g["G"])
    if row["kind"] == "updil":
        conv.update(updil=GR.UPDIL[:2], pads=GR.UPDIL[2:])
    if row["kind"] == "dwin":
        conv.update(dwin=row["dwin"])
    return conv


def plan(seam, row):
    """The row's aligned launch through the plan-only seam -> (rc, kernel name, launch info).  Rows _guard_rows.Seam.plan cannot state
    (groups, a kernel that is not square, the depth window) take the same call chain with their own geometry: a second, small copy of
    that marshalling, kept here because _guard_rows.py and the tests that share it are left as they are."""
    import ctypes as C
    if row["groups"] == 1 and row["dwin"] is None and row["kw"] is None:
        return seam.plan(row, 0, ())
    m, L, g, P = seam.m, seam.L, geometry(row), GR.P
    par = m.bt_params(P, P, P, P, None, None, None, None, P if row["packs"] else None, P if row["packs"] else None, 0, 0)
    draws = m.bt_draws(None, None, None, None, m.bt_rng(1, None, 0, 1, 0, 0))
    tail = (row["S"], P, 0, C.byref(par), C.byref(draws), None, P, None, P, m.WORKSPACE_BYTES, None)
    before = L.bt_get_contraction()
    seam.h.bt_debug_plan_only(1)
    try:
        assert L.bt_set_contraction(row["mode"]) == 0
        if row["kind"] == "dwin":
            kd, D, sd, dd, pd = row["dwin"]
            geom = m.bt_conv2d_geom(g["B"] * g["Do"], g["Ci"] * kd, g["H"], g["W"], g["Co"], g["k"], g["k"], g["st"], g["st"], g["pad"], g["pad"], 1, 1, g["G"])
            dw = m.bt_dwin(kd, D, sd, dd, pd)
            rc = (L.bt_flipout_conv2d_dwin_fwd if row["flip"] else L.bt_reparam_conv2d_dwin_fwd)(C.byref(geom), C.byref(dw), *tail)
        else:
            geom = m.bt_conv2d_geom(g["B"], g["Ci"], g["H"], g["W"], g["Co"], g["k"], g["kw"], g["st"], g["st"], g["pad"], g["padw"], 1, 1, g["G"])
            rc = (L.bt_flipout_conv2d_fwd if row["flip"] else L.bt_reparam_conv2d_fwd)(C.byref(geom), *tail)
    finally:
        seam.h.bt_debug_plan_only(0)
        L.bt_set_contraction(before)
    if rc != 0:
        return rc, L.bt_last_error_string().decode(), None
    L.bt_last_launch_info(seam.info, 16)
    return rc, L.bt_last_kernel_name().decode(), dict(zip(m.LAUNCH_INFO_FIELDS, (int(v) for v in seam.info)))


# ------------------------------------------------------------------------------------------------------------- the reference contraction
def contract(row, x, w, fold=1):
    """The float64 reference contraction of the row's launch, output in the launch's layout.  fold > 1: x holds ``fold`` inputs stacked
    along its channels and w ``fold`` kernels stacked along its output channels (one grouped call for a chunk of samples)."""
    g = geometry(row)
    if row["kind"] == "linear":
        if fold == 1:
            return TF.linear(x, w)
        return torch.einsum("bfi,foi->bfo", x.reshape(x.shape[0], fold, -1), w.reshape(fold, -1, w.shape[1])).reshape(x.shape[0], -1)
    G = g["G"] * fold
    if row["kind"] == "dwin":
        kd, D, sd, dd, pd = row["dwin"]
        x5 = x.reshape(x.shape[0], -1, D, g["H"], g["W"])
        w5 = w.reshape(w.shape[0], -1, kd, g["k"], g["k"])
        o = TF.conv3d(x5, w5, None, (sd, g["st"], g["st"]), (pd, g["pad"], g["pad"]), (dd, 1, 1), G)
        return o.permute(0, 2, 1, 3, 4).reshape(-1, w.shape[0], g["Ho"], g["Wo"])
    if row["kind"] == "updil":
        uh, uw, lh, hh, lw, hw = GR.UPDIL
        H, W = x.shape[-2:]
        up = x.new_zeros(x.shape[:-2] + ((H - 1) * uh + 1 + lh + hh, (W - 1) * uw + 1 + lw + hw))
        up[..., lh:lh + (H - 1) * uh + 1:uh, lw:lw + (W - 1) * uw + 1:uw] = x
        x = up
    return TF.conv2d(x, w, None, g["st"], (g["pad"], g["padw"]), 1, G)


def contract_samples(row, x, w, sign_in=None):
    """x [B, ...] (shared) against w [S, Co, ...] -> [S, rows, Co, ...] in one grouped call; sign_in [S, B, ...]: x * sign_in per sample."""
    S, Co, G = w.shape[0], w.shape[1], geometry(row)["G"]
    if sign_in is not None:
        assert G == 1
        xs = (x.unsqueeze(0) * sign_in).transpose(0, 1)                     # [B, S, Ci, ...]
        o = contract(row, xs.reshape((x.shape[0], S * x.shape[1]) + tuple(x.shape[2:])), w.flatten(0, 1), fold=S)
        return o.reshape((o.shape[0], S, Co) + tuple(o.shape[2:])).transpose(0, 1)
    if G == 1:
        o = contract(row, x, w.flatten(0, 1))
        return o.reshape((o.shape[0], S, Co) + tuple(o.shape[2:])).transpose(0, 1)
    wg = w.reshape((S, G, Co // G) + tuple(w.shape[2:])).transpose(0, 1).flatten(0, 2)      # output channels ordered (group, sample, channel)
    o = contract(row, x, wg)
    o = o.reshape((o.shape[0], G, S, Co // G) + tuple(o.shape[2:]))
    return o.permute(2, 0, 1, 3, *range(4, o.dim())).reshape((S, o.shape[0], Co) + tuple(o.shape[4:]))


# ------------------------------------------------------------------------------------------------------------- parameters
def _gen(rid, salt):
    return torch.Generator().manual_seed(7000 + 10 * sorted(ROWS).index(rid) + salt)


def parameters(rid, form):
    """-> dict(mu_w, rho_w, mu_b, rho_b: fp32 as launched; sigma_w, sigma_b: float64 softplus).  sigma_w log-uniform over [0.007, 0.3],
    sigma_b uniform over [0.1, 0.6]; mu_w = 0 for the probe, N(0, 0.1^2) for the dense form."""
    row, gen = ROWS[rid], _gen(rid, 0 if form == "probe" else 1)
    _, wshape, _ = shapes(row)
    sig = torch.exp(torch.rand(wshape, generator=gen, dtype=F64) * (math.log(0.3) - math.log(0.007)) + math.log(0.007))
    sig_b = torch.rand(wshape[0], generator=gen, dtype=F64) * 0.5 + 0.1
    p = dict(mu_w=torch.zeros(wshape) if form == "probe" else torch.randn(wshape, generator=gen) * 0.1, rho_w=torch.log(torch.expm1(sig)).float(),
             mu_b=torch.randn(wshape[0], generator=gen) * 0.1, rho_b=torch.log(torch.expm1(sig_b)).float())
    p["sigma_w"], p["sigma_b"] = torch.log1p(torch.exp(p["rho_w"].double())), torch.log1p(torch.exp(p["rho_b"].double()))
    return p


# ------------------------------------------------------------------------------------------------------------- a. the impulse probe
_PROBES = {}


def probe(rid):
    """-> dict(xs: the impulse inputs, one [B, ...] fp32 tensor per launch; pos / wid: per launch, the flat indices into one sample's
    output and the weight elements (flat, natural order) they read; zero: per launch, the flat output index that reads channel co's
    bias alone, [Co]; mirror: the flat offset to the twin example (Flipout), K).  Built once per row and never modified."""
    if rid in _PROBES:
        return _PROBES[rid]
    row, g = ROWS[rid], geometry(ROWS[rid])
    assert row["kind"] in ("conv", "linear")
    xshape, wshape, oshape = shapes(row)
    flip, B, k, kw, st, pad, padw, G = row["flip"], g["B"], g["k"], g["kw"], g["st"], g["pad"], g["padw"], g["G"]
    Cig = g["Ci"] // G
    slots = B // 2 if flip else B - 1            # Flipout: example b + B // 2 repeats example b; Reparameterization: the last example stays zero
    per_out = math.prod(oshape[1:])

    def touched(h, w):     # the taps an impulse at pixel (h, w) reaches, and the output pixel of each
        res = {}
        for i in range(k):
            for j in range(kw):
                oh, ow = h + pad - i, w + padw - j
                if oh % st == 0 and ow % st == 0 and 0 <= oh // st < g["Ho"] and 0 <= ow // st < g["Wo"]:
                    res[(i, j)] = (oh // st, ow // st)
        return res

    # the impulses: per input channel, pixels until every tap of that channel is reached
    wanted = []
    for ci in range(g["Ci"]):
        seen = set()
        while len(seen) < k * kw:      # greedy cover: the pixel that reaches the most taps not yet reached
            h, w = max(((h, w) for h in range(g["H"]) for w in range(g["W"])), key=lambda hw: len(set(touched(*hw)) - seen))
            t = touched(h, w)
            assert set(t) - seen, (rid, ci)
            wanted.append((ci, h, w, t))
            seen |= set(t)
    # their seats: the first example of the current launch whose touched output pixels are all free (a 1 x 1 kernel seats one per pixel)
    launches, used = [[]], {}
    for ci, h, w, t in wanted:
        grp = ci // Cig
        for b in range(slots + 1):
            if b == slots:
                launches.append([])
                used, b = {}, 0
            if not any((b, grp, px) in used for px in t.values()):
                break
        used.update({(b, grp, px): 1 for px in t.values()})
        launches[-1].append((b, ci, h, w))
    xs = []
    for seats in launches:
        x = torch.zeros(xshape)
        for b, ci, h, w in seats:
            for bb in ((b, b + B // 2) if flip else (b,)):
                if row["kind"] == "linear":
                    x[bb, ci] = 1.0
                else:
                    x[bb, ci, h, w] = 1.0
        xs.append(x)
    # the map, from the reference contraction on index-coded weights: an output with exactly one contribution names its weight
    K = math.prod(wshape)
    w_idx, w_one = torch.arange(1, K + 1, dtype=F64).reshape(wshape), torch.ones(wshape, dtype=F64)
    pos, wid, have = [], [], torch.zeros(K, dtype=torch.bool)
    first = slice(0, (B // 2 if flip else B) * per_out)
    for x in xs:
        cnt, idx = contract(row, x.double(), w_one).reshape(-1)[first], contract(row, x.double(), w_idx).reshape(-1)[first]
        at = torch.nonzero(cnt == 1).reshape(-1)
        wd = idx[at].round().long() - 1
        keep, seen_here = [], set()
        for a, d in zip(at.tolist(), wd.tolist()):
            if not have[d] and d not in seen_here:
                seen_here.add(d)
                keep.append((a, d))
        have[[d for _, d in keep]] = True
        pos.append(torch.tensor([a for a, _ in keep], dtype=torch.long))
        wid.append(torch.tensor([d for _, d in keep], dtype=torch.long))
    allw, allp = torch.cat(wid), torch.cat([p + i * B * per_out for i, p in enumerate(pos)])
    assert bool(have.all()) and allw.numel() == K and allw.unique().numel() == K and allp.unique().numel() == K, (rid, int(have.sum()), K)
    pix = math.prod(oshape[2:])
    zero = (B - 1) * per_out + torch.arange(g["Co"]) * pix        # Reparameterization: example B - 1 is all zero in every launch
    _PROBES[rid] = dict(xs=xs, pos=pos, wid=wid, zero=zero, mirror=(B // 2) * per_out, K=K, per_out=per_out, pix=pix)
    return _PROBES[rid]


def probe_draws(rid, p, outs, bias_out=None):
    """The standardised draws an impulse run recovers.  outs: per launch [S, B * Co * Ho * Wo] float64 (Reparameterization: launched
    with the bias; Flipout: without); bias_out: Flipout's all-zero launch with the bias, [S, ...].
    -> E [S, K + Co] (weight columns in natural order, then the bias columns), and for Flipout E2 (the twin examples' columns)."""
    pr, row = probe(rid), ROWS[rid]
    S, Co = outs[0].shape[0], p["mu_b"].numel()
    sw, sb, mb = p["sigma_w"].reshape(-1), p["sigma_b"], p["mu_b"].double()
    E = torch.empty(S, pr["K"] + Co, dtype=F64)
    co_of = lambda wid: wid // (pr["K"] // Co)
    if not row["flip"]:
        for o, pos, wid in zip(outs, pr["pos"], pr["wid"]):
            E[:, wid] = (o[:, pos].double() - o[:, pr["zero"][co_of(wid)]].double()) / sw[wid]
        E[:, pr["K"]:] = (outs[0][:, pr["zero"]].double() - mb) / sb
        return E, None
    E2 = torch.empty_like(E)
    for o, pos, wid in zip(outs, pr["pos"], pr["wid"]):
        E[:, wid], E2[:, wid] = o[:, pos].double() / sw[wid], o[:, pos + pr["mirror"]].double() / sw[wid]
    z = torch.arange(Co) * pr["pix"]
    E[:, pr["K"]:], E2[:, pr["K"]:] = (bias_out[:, z].double() - mb) / sb, (bias_out[:, z + pr["mirror"]].double() - mb) / sb
    return E, E2


def corr_window(n, Co):
    """None when all n (n - 1) / 2 pairs of a probe's columns fit MAX_PAIRS, else the window w of corr_max's cover."""
    if Co is None or n * (n - 1) // 2 <= MAX_PAIRS:
        return None
    K = n - Co
    m = K // Co
    fixed = Co * m * (m - 1) // 2 + Co * K + Co * (Co - 1) // 2
    return max(0, min(m - 1, int(((MAX_PAIRS - fixed) / (Co * (Co - 1) // 2 * m) - 1) // 2)))


def corr_max(E, Co=None):
    """The largest |correlation| between two different columns of E [S, n] (C is the identity), in standard errors.  Every pair, in
    column blocks with a running maximum, while n (n - 1) / 2 <= MAX_PAIRS.  A probe with more columns (K weight columns as Co channels
    of m, then Co bias columns) takes the pairs MAX_PAIRS buys: every pair inside an output channel, every bias column against every
    column, and between two different channels every pair whose positions inside their channels differ by at most corr_window(n, Co)
    -- so every column meets every channel."""
    S, n = E.shape
    w = corr_window(n, Co)
    worst = 0.0
    if w is None:
        blk = 2048
        for a in range(0, n, blk):
            for b in range(a, n, blk):
                Cm = E[:, a:a + blk].T @ E[:, b:b + blk] / S
                if a == b:
                    Cm.fill_diagonal_(0)
                worst = max(worst, float(Cm.abs().max()))
        return worst * math.sqrt(S)
    K = n - Co
    m = K // Co
    E3 = E[:, :K].reshape(S, Co, m)
    for c in range(Co):
        Cm = E3[:, c].T @ E3[:, c] / S
        Cm.fill_diagonal_(0)
        worst = max(worst, float(Cm.abs().max()))
    Cb = E[:, K:].T @ E / S
    Cb[torch.arange(Co), K + torch.arange(Co)] = 0
    worst = max(worst, float(Cb.abs().max()))
    for off in range(w + 1):      # ordered channel pairs (c, d), c != d, positions (i, i + off): every unordered pair within the window
        A, B = E3[:, :, :m - off].permute(2, 1, 0), E3[:, :, off:].permute(2, 0, 1)
        Cx = torch.bmm(A, B) / S                  # [m - off, Co, Co]
        Cx[:, torch.arange(Co), torch.arange(Co)] = 0
        worst = max(worst, float(Cx.abs().max()))
    return worst * math.sqrt(S)


def probe_stats(E, Co=None, E2=None):
    """E [S, n] standardised draws -> {statistic: worst value in standard errors}.  C is the identity and the mean 0.  Co: the number of
    output channels of a probe row (its last Co columns are the bias draws), for corr_max."""
    S, n = E.shape
    st = dict(mean=float(E.mean(0).abs().max()) * math.sqrt(S), var=float(((E * E).mean(0) - 1).abs().max()) / math.sqrt(2.0 / S),
              lag1=float((E[1:] * E[:-1]).mean(0).abs().max()) * math.sqrt(S - 1),
              m3=abs(float((E ** 3).mean())) / math.sqrt(15.0 / (S * n)), m4=abs(float((E ** 4).mean()) - 3.0) / math.sqrt(96.0 / (S * n)))
    st["corr"] = corr_max(E, Co)
    if E2 is not None:      # Flipout: the twin example reads the same eps under its own signs
        # s_out * s_in hides a shared eps from the correlation above: |e| mapped back to N(0,1) (the probability transform of the half
        # normal, then the normal quantile) is exactly standard normal under the hypothesis and equal for two columns that share an eps
        Z = math.sqrt(2.0) * torch.special.erfinv((2 * torch.special.erf(E.abs() / math.sqrt(2.0)) - 1).clamp(-1 + 1e-15, 1 - 1e-15))
        st["corr_abs"] = corr_max(Z, Co)
        st["abs_gap"] = float(((E.abs() - E2.abs()).abs() / (1 + E.abs())).max())
        agree = ((E > 0) == (E2 > 0)).double().mean(0)
        st["sign"] = float((agree - 0.5).abs().max()) * 2 * math.sqrt(S)
    return st


def cross_stat(Ea, Eb):
    """The cross-correlation of matching columns of two runs, in standard errors."""
    return float((Ea * Eb).mean(0).abs().max()) * math.sqrt(Ea.shape[0])


# ------------------------------------------------------------------------------------------------------------- b. the dense moments
def choose_outputs(oshape, extra_channels=()):
    """At most 512 flat output indices of one sample's output [rows, Co, ...]: the first and the last example, channels and pixels spread
    over the whole range (first and last included)."""
    rows, Co, pix = oshape[0], oshape[1], math.prod(oshape[2:])
    spread = lambda n, m: sorted({round(i * (n - 1) / max(min(n, m) - 1, 1)) for i in range(min(n, m))})
    px = spread(pix, 32)
    ex = sorted({0, rows - 1})
    n_ch = max(1, 512 // (len(ex) * len(px)))
    extra = [c for c in extra_channels if c < Co]
    ch = sorted(set(spread(Co, max(1, min(Co, n_ch) - len(extra))) + extra))[:n_ch]
    idx = [(b * Co + c) * pix + q for b in ex for c in ch for q in px]
    assert len(idx) <= 512
    return torch.tensor(idx, dtype=torch.long)


def dense_x(rid):
    return (torch.rand(shapes(ROWS[rid])[0], generator=_gen(rid, 2), dtype=F64) + 0.5).float()


def dense_moments(contract_fn, x, p, flip, sel):
    """The analytic mean [N] and covariance [N, N] of the outputs ``sel`` (flat indices into contract_fn's output [rows, Co, ...]), and
    for Flipout Q [N, N] (below; None for Reparameterization, whose outputs are jointly Gaussian).
    contract_fn(x, w) is the float64 reference contraction; p holds mu_w, mu_b (fp32) and sigma_w, sigma_b (float64)."""
    x = x.double()
    mu = p["mu_w"].double()
    o = contract_fn(x, mu)
    Co, pix = o.shape[1], math.prod(o.shape[2:])
    co = (sel // pix) % Co
    has_b = p.get("mu_b") is not None
    mean = o.reshape(-1)[sel] + (p["mu_b"].double()[co] if has_b else 0)
    vb = p["sigma_b"][co] ** 2 if has_b else torch.zeros(sel.numel(), dtype=F64)
    s2 = p["sigma_w"] ** 2
    w = mu.clone().requires_grad_(True)
    flat = contract_fn(x, w).reshape(-1)
    J = torch.stack([torch.autograd.grad(flat[i], w, retain_graph=True)[0].reshape(-1) for i in sel.tolist()])
    same = (co[:, None] == co[None, :]).double()
    if flip:
        # the estimate of a zero covariance between two outputs that share eps under independent signs has the variance
        # (C_ii C_jj + 2 Q_ij) / S, Q_ij = sum_k J_ik^2 J_jk^2 sigma_k^4 + [same channel] sigma_b^4: the outputs are uncorrelated, not
        # independent (E[e^4] = 3), and with few terms per output the Gaussian formula alone would understate the standard error
        Q = ((J * J) * (s2 * s2).reshape(-1)) @ (J * J).T + same * vb[:, None] * vb[None, :]
        Q.fill_diagonal_(0)
        return mean, torch.diag(contract_fn(x * x, s2).reshape(-1)[sel] + vb), Q
    Cv = (J * s2.reshape(-1)) @ J.T
    return mean, Cv + same * vb[:, None], None      # eps_b[co] is shared by every output of channel co


_DENSE = {}


def dense_case(rid):
    """(x, parameters, chosen outputs, analytic mean, analytic covariance, Q or None) of a row's dense form: computed once, shared,
    never modified."""
    if rid not in _DENSE:
        row = ROWS[rid]
        x, p = dense_x(rid), parameters(rid, "dense")
        sel = choose_outputs(shapes(row)[2], extra_channels=(31, 32) if rid == "g_pchan" else ())
        _DENSE[rid] = (x, p, sel) + dense_moments(lambda a, w: contract(row, a, w), x, p, row["flip"], sel)
    return _DENSE[rid]


# The layer classes' dense rows: (id, class, constructor, x shape, the path switch the GPU test runs it under, every setting).  Conv1d has no
# switch; the transposed 2-d and the Conv3d geometries are rows of test_convt_native_host.py / test_conv3d_native_host.py that take the
# native launch.
R3 = dict(prior_mean=0.0, prior_variance=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0)
LAYER_ROWS = [
    ("c1r", "Conv1dReparameterization", dict(in_channels=16, out_channels=40, kernel_size=3, padding=1), (2, 16, 61), None),
    ("c1f", "Conv1dFlipout", dict(in_channels=8, out_channels=24, kernel_size=9, padding=4), (2, 8, 64), None),
    ("t2r", "ConvTranspose2dReparameterization", dict(in_channels=16, out_channels=24, kernel_size=3, stride=2, padding=1, output_padding=1), (2, 16, 5, 6), "convt"),
    ("t2f", "ConvTranspose2dFlipout", dict(in_channels=16, out_channels=16, kernel_size=3, stride=2, padding=1, output_padding=1, groups=2), (2, 16, 6, 5), "convt"),
    ("c3r", "Conv3dReparameterization", dict(in_channels=8, out_channels=24, kernel_size=3, padding=(2, 1, 1), **R3), (2, 8, 5, 6, 7), "conv3d"),
    ("c3f", "Conv3dFlipout", dict(in_channels=16, out_channels=16, kernel_size=3, padding=1, dilation=(2, 1, 1), groups=2), (2, 16, 6, 5, 5), "conv3d"),
    ("t3r", "ConvTranspose3dReparameterization", dict(in_channels=2, out_channels=4, kernel_size=(2, 3, 3), stride=(2, 1, 1), padding=(0, 1, 1)), (2, 2, 4, 8, 8), None),
    ("t3f", "ConvTranspose3dFlipout", dict(in_channels=4, out_channels=8, kernel_size=3, stride=(1, 2, 2), padding=1, output_padding=(0, 1, 1)), (2, 4, 3, 5, 5), None),
]
_LAYERS = {}


def layer_case(rid):
    """A layer row -> (a fresh CPU layer with the row's parameters, x, p, the reference layout's conv dict (oracle.bt_oracle._contract),
    chosen outputs, (analytic mean, analytic covariance, Q or None), one sample's output shape).  The moments are computed once."""
    import bayesian_torch_amd.layers as L
    from oracle import bt_oracle as O
    _, cls, ctor, xshape, _ = next(r for r in LAYER_ROWS if r[0] == rid)
    gen = torch.Generator().manual_seed(900 + [r[0] for r in LAYER_ROWS].index(rid))
    layer = getattr(L, cls)(**ctor)
    lo, hi = math.log(0.007), math.log(0.3)
    with torch.no_grad():
        layer.mu_kernel.copy_(torch.randn(layer.mu_kernel.shape, generator=gen) * 0.1)
        layer.rho_kernel.copy_(torch.log(torch.expm1(torch.exp(torch.rand(layer.rho_kernel.shape, generator=gen) * (hi - lo) + lo))))
        layer.mu_bias.copy_(torch.randn(layer.mu_bias.shape, generator=gen) * 0.1)
        layer.rho_bias.copy_(torch.log(torch.expm1(torch.rand(layer.rho_bias.shape, generator=gen) * 0.5 + 0.1)))
    x = torch.rand(xshape, generator=gen) + 0.5
    nd = len(xshape) - 2
    tup = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * nd
    conv = dict(stride=tup(layer.stride), padding=tup(layer.padding), dilation=tup(layer.dilation), groups=layer.groups)
    if "Transpose" in cls:
        conv.update(transposed=True, output_padding=tup(layer.output_padding))
    if rid not in _LAYERS:
        p = dict(mu_w=layer.mu_kernel.detach().clone(), mu_b=layer.mu_bias.detach().clone(), rho_w=layer.rho_kernel.detach().clone(), rho_b=layer.rho_bias.detach().clone(),
                 sigma_w=torch.log1p(torch.exp(layer.rho_kernel.detach().double())), sigma_b=torch.log1p(torch.exp(layer.rho_bias.detach().double())))
        fn = lambda a, w: O._contract(a, w, None, conv)
        oshape = tuple(fn(x.double(), p["mu_w"].double()).shape)
        sel = choose_outputs(oshape)
        _LAYERS[rid] = (p, sel) + dense_moments(fn, x, p, "Flipout" in cls, sel) + (oshape,)
    p, sel, mean, Cv, Q, oshape = _LAYERS[rid]
    return layer, x, p, conv, sel, (mean, Cv, Q), oshape


def dense_stats(Y, mean, Cv, Q=None):
    """Y [S, N] against the analytic mean and covariance -> {statistic: worst value in standard errors}.  Q: dense_moments' fourth-moment
    term of the Flipout rows' covariance entries."""
    S = Y.shape[0]
    d = Cv.diagonal()
    Z = Y - mean
    Ch = Z.T @ Z / S
    z = (Ch - Cv).abs() / torch.sqrt((d[:, None] * d[None, :] + Cv * Cv + (0 if Q is None else 2 * Q)) / S)
    off = z.clone()
    off.fill_diagonal_(0)
    U = Z / torch.sqrt(d)
    return dict(mean=float((Y.mean(0) - mean).abs().div(torch.sqrt(d / S)).max()), var=float(z.diagonal().max()), cov=float(off.max()),
                lag1=float((U[1:] * U[:-1]).mean(0).abs().max()) * math.sqrt(S - 1))


def worst(st):
    """The worst of the statistics that are held to BOUND (abs_gap is an equality, held on its own)."""
    return max(v for k, v in st.items() if k != "abs_gap")


ABS_GAP = 1e-5      # |e| of the two twin examples: one exact product each, a few fp32 ulp of (1 + |e|)
