"""CPU side of the draw-distribution tests (tests/_draw_stats.py): the reference arithmetic -- the float64 contraction on torch's own
normal_() and sign draws -- run through the impulse probe and the dense moments on the exact inputs of every GPU row stays inside the
7.0 bound; the same arithmetic with a seeded fault in the draws falls outside it (the test has teeth); every row plans the kernel its
pin names through the plan-only seam, and the pins reach every family test_gpu_draw_distribution.py is there for."""
import re

import pytest
import torch

import _draw_stats as DS
import _guard_rows as GR

F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------- the reference's draws
def _draw(rid, S, gen, fault=None):
    """One chunk of S samples drawn as the reference draws them (normal_(), uniform_(-1, 1).sign_()), with an optional seeded fault."""
    row = DS.ROWS[rid]
    xshape, wshape, oshape = DS.shapes(row)
    d = dict(eps_w=torch.empty((S,) + wshape, dtype=F64).normal_(generator=gen), eps_b=torch.empty(S, wshape[0], dtype=F64).normal_(generator=gen))
    if row["flip"]:
        d["sign_in"] = torch.empty((S,) + xshape, dtype=F64).uniform_(-1, 1, generator=gen).sign_()
        d["sign_out"] = torch.empty((S,) + oshape, dtype=F64).uniform_(-1, 1, generator=gen).sign_()
    if fault == "channel":          # one input channel's draws copied from another
        d["eps_w"][:, :, 1] = d["eps_w"][:, :, 0]
    elif fault == "pair":           # a single aliased pair of weight elements
        d["eps_w"].reshape(S, -1)[:, 5] = d["eps_w"].reshape(S, -1)[:, 3]
    elif fault == "pair_far":       # ... in the last output channel, the last columns of the probe
        d["eps_w"].reshape(S, -1)[:, -1] = d["eps_w"].reshape(S, -1)[:, -3]
    elif fault == "pair_cross":     # ... in two distant output channels, three positions apart inside their channels
        m = d["eps_w"][0, 0].numel()
        d["eps_w"].reshape(S, -1)[:, (wshape[0] - 1) * m + m - 12] = d["eps_w"].reshape(S, -1)[:, (wshape[0] // 4) * m + m - 15]
    elif fault == "bias":           # the bias draw equal to a weight draw
        d["eps_b"][:, :] = d["eps_w"].reshape(S, wshape[0], -1)[:, :, 0]
    elif fault == "repeat":         # odd samples repeat the previous sample's stream
        for v in d.values():
            v[1::2] = v[0::2]
    elif fault == "signs":          # Flipout signs shared by the examples of a batch
        d["sign_in"][:, 1:] = d["sign_in"][:, :1]
        d["sign_out"][:, 1:] = d["sign_out"][:, :1]
    else:
        assert fault is None, fault
    return d


def _bcast(v, o):
    return v.reshape(v.shape[:1] + (1, -1) + (1,) * (o.dim() - 3))


def host_probe(rid, S_total, seed, fault=None):
    """The probe's statistics of the reference arithmetic -> (stats, E)."""
    row, p, pr = DS.ROWS[rid], DS.parameters(rid, "probe"), DS.probe(rid)
    gen = torch.Generator().manual_seed(seed)
    Es, E2s = [], []
    for _ in range(S_total // DS.CHUNK):
        d = _draw(rid, DS.CHUNK, gen, fault)
        w = p["sigma_w"] * d["eps_w"]            # mu_w = 0
        outs, bias_out = [], None
        for x in pr["xs"]:
            if row["flip"]:
                o = DS.contract_samples(row, x.double(), w, d["sign_in"]) * d["sign_out"]
            else:
                o = DS.contract_samples(row, x.double(), w)
                o = o + _bcast(p["mu_b"].double() + p["sigma_b"] * d["eps_b"], o)
            outs.append(o.reshape(DS.CHUNK, -1))
        if row["flip"]:
            bias_out = (_bcast(p["mu_b"].double().expand(DS.CHUNK, -1), d["sign_out"]) + d["sign_out"] * _bcast(p["sigma_b"] * d["eps_b"], d["sign_out"])).reshape(DS.CHUNK, -1)
        E, E2 = DS.probe_draws(rid, p, outs, bias_out)
        Es.append(E)
        E2s.append(E2)
    E = torch.cat(Es)
    E2 = torch.cat(E2s) if row["flip"] else None
    return DS.probe_stats(E, DS.shapes(row)[1][0], E2), E


def host_dense(rid, S_total, seed, fault=None):
    row = DS.ROWS[rid]
    x, p, sel, mean, Cv, Q = DS.dense_case(rid)
    gen = torch.Generator().manual_seed(seed)
    Ys = []
    for _ in range(S_total // DS.CHUNK):
        d = _draw(rid, DS.CHUNK, gen, fault)
        w = p["mu_w"].double() + p["sigma_w"] * d["eps_w"]
        if row["flip"]:
            o = DS.contract_samples(row, x.double(), p["sigma_w"] * d["eps_w"], d["sign_in"])
            o = (o + _bcast(p["sigma_b"] * d["eps_b"], o)) * d["sign_out"] + (DS.contract(row, x.double(), p["mu_w"].double()) + _bcast(p["mu_b"].double()[None], o)[0])
        else:
            o = DS.contract_samples(row, x.double(), w)
            o = o + _bcast(p["mu_b"].double() + p["sigma_b"] * d["eps_b"], o)
        Ys.append(o.reshape(DS.CHUNK, -1)[:, sel])
    return DS.dense_stats(torch.cat(Ys), mean, Cv, Q)


def _show(tag, st):
    print(f"\n{tag}: worst {DS.worst(st):.2f}  " + "  ".join(f"{k} {v:.3g}" for k, v in st.items()))


# ------------------------------------------------------------------------------------------------------------- the reference stays inside
CASES = [(rid, form) for rid, row in DS.ROWS.items() for form in row["forms"]]


@pytest.mark.parametrize("rid,form", CASES, ids=[f"{r}-{f}" for r, f in CASES])
def test_reference_arithmetic_stays_inside_the_bound(rid, form):
    S = DS.ROWS[rid]["S_total"]
    st = host_probe(rid, S, 1)[0] if form == "probe" else host_dense(rid, S, 2)
    _show(f"{rid} {form} S={S} (reference arithmetic, torch draws)", st)
    assert DS.worst(st) < DS.BOUND, (rid, form, st)
    if form == "probe" and DS.ROWS[rid]["flip"]:
        assert st["abs_gap"] <= DS.ABS_GAP, st


@pytest.mark.parametrize("rid", [r[0] for r in DS.LAYER_ROWS])
def test_layer_rows_reference_arithmetic_stays_inside_the_bound(rid):
    """The layer-API rows of the GPU file: the layer's own float64 reference (oracle.bt_oracle) on torch's draws, sample by sample."""
    from oracle import bt_oracle as O
    layer, x, p, conv, sel, moments, oshape = DS.layer_case(rid)
    gen, S, x = torch.Generator().manual_seed(8), 1024, x.double()
    w64 = {k: p[k].double() for k in ("mu_w", "rho_w", "mu_b", "rho_b")}
    Y = torch.empty(S, sel.numel(), dtype=F64)
    for s in range(S):
        ew, eb = torch.empty(w64["mu_w"].shape, dtype=F64).normal_(generator=gen), torch.empty(w64["mu_b"].shape, dtype=F64).normal_(generator=gen)
        if layer._flip:
            si, so = (torch.empty(sh, dtype=F64).uniform_(-1, 1, generator=gen).sign_() for sh in (x.shape, oshape))
            o = O.flipout_fwd_ref(x, w64["mu_w"], w64["rho_w"], ew, si, so, w64["mu_b"], w64["rho_b"], eb, conv)
        else:
            o = O.reparam_fwd_ref(x, w64["mu_w"], w64["rho_w"], ew, w64["mu_b"], w64["rho_b"], eb, conv)
        Y[s] = o.reshape(-1)[sel]
    st = DS.dense_stats(Y, *moments)
    _show(f"{rid} {type(layer).__name__} dense S={S} N={sel.numel()} (reference arithmetic, torch draws)", st)
    assert DS.worst(st) < DS.BOUND, (rid, st)


def test_probe_maps_are_one_to_one_and_cover_every_weight_and_bias_element():
    for rid, row in DS.ROWS.items():
        if "probe" not in row["forms"]:
            continue
        pr, (xshape, wshape, oshape) = DS.probe(rid), DS.shapes(row)
        wid, pos = torch.cat(pr["wid"]), torch.cat([q + i * 10 ** 9 for i, q in enumerate(pr["pos"])])
        assert sorted(wid.tolist()) == list(range(pr["K"])) and pos.unique().numel() == pr["K"], rid
        for x in pr["xs"]:
            assert x.shape == xshape and bool(((x == 0) | (x == 1)).all())
            if not row["flip"]:
                assert float(x[-1].abs().sum()) == 0        # the example that reads the bias draw
            else:
                assert torch.equal(x[:xshape[0] // 2], x[xshape[0] // 2:2 * (xshape[0] // 2)])      # every impulse in two examples


# ------------------------------------------------------------------------------------------------------------- the test has teeth
# (row, form, fault, the statistic that must leave the bound)
FAULTS = [
    ("g_xm1", "probe", "channel", "corr"), ("g_xm1", "probe", "pair", "corr"), ("g_xm1", "probe", "bias", "corr"), ("g_xm1", "probe", "repeat", "lag1"),
    ("g_packs", "probe", "pair", "corr"), ("g_packs", "probe", "pair_far", "corr"), ("d_str", "probe", "pair_far", "corr"), ("d_str", "probe", "pair_cross", "corr"),
    ("s_128", "probe", "pair_far", "corr"), ("s_128", "probe", "pair_cross", "corr"), ("f_xm1", "probe", "signs", "sign"), ("f_xm1", "probe", "pair", "corr_abs"), ("f_3x3", "probe", "repeat", "lag1"),
    ("p_general", "dense", "channel", "cov"), ("p_general", "dense", "bias", "cov"), ("p_general", "dense", "repeat", "lag1"),
    ("f_3x3", "dense", "signs", "cov"), ("f_3x3", "dense", "repeat", "lag1"), ("s_128", "probe", "channel", "corr"), ("w_a", "dense", "repeat", "lag1"),
]


@pytest.mark.parametrize("rid,form,fault,stat", FAULTS, ids=[f"{r}-{f}-{x}" for r, f, x, _ in FAULTS])
def test_a_seeded_fault_in_the_draws_leaves_the_bound(rid, form, fault, stat):
    S = DS.ROWS[rid]["S_total"] if form == "probe" else 4096      # the probe at the GPU rows' S; the dense form at 4096, where a bias draw equal to a weight draw shows
    st = host_probe(rid, S, 3, fault)[0] if form == "probe" else host_dense(rid, S, 4, fault)
    _show(f"{rid} {form} fault={fault} S={S}", st)
    assert st[stat] > DS.BOUND and DS.worst(st) > DS.BOUND, (rid, form, fault, st)


def test_the_dense_form_misses_a_single_aliased_pair_and_the_probe_finds_it():
    """Why both oracles: one aliased pair of weight elements moves a dense variance by a fraction of its standard error, and the probe
    reads the pair as a correlation of sqrt(S) standard errors."""
    S = 1024
    dense, probe = host_dense("p_general", S, 5, "pair"), host_probe("p_general", S, 5, "pair")[0]
    _show("p_general dense fault=pair", dense)
    _show("p_general probe fault=pair", probe)
    assert DS.worst(dense) < DS.BOUND < probe["corr"] and probe["corr"] > 0.9 * S ** 0.5


def test_two_runs_at_coordinates_that_differ_are_uncorrelated_and_a_repeated_stream_is_not():
    """cross_stat, the statistic of the coordinate rows (call / call + 1, layer_id / layer_id + 1, eager / replay)."""
    a, b = host_probe("g_xm1", 1024, 6)[1], host_probe("g_xm1", 1024, 7)[1]
    print(f"\ncross-coordinate statistic, independent runs: {DS.cross_stat(a, b):.2f}; the same run twice: {DS.cross_stat(a, a):.1f}")
    assert DS.cross_stat(a, b) < DS.BOUND < DS.cross_stat(a, a)


# ------------------------------------------------------------------------------------------------------------- plan pins
@pytest.fixture(scope="module")
def seam():
    return GR.Seam()


@pytest.mark.parametrize("rid", list(DS.ROWS))
def test_row_plans_the_pinned_kernel(seam, rid):
    rc, name, info = DS.plan(seam, DS.ROWS[rid])
    assert (rc, name, GR.info_of(info)) == (0,) + DS.PINS[rid], (rid, name, info)


def test_rows_reach_every_family():
    names = {rid: DS.PINS[rid][0] for rid in DS.ROWS}
    assert set(DS.PINS) == set(DS.ROWS)
    hit = lambda pat, form: [rid for rid, n in names.items() if re.search(pat, n) and form in DS.ROWS[rid]["forms"]]
    g = lambda rid: DS.geometry(DS.ROWS[rid])
    for pat, form, more in (
            (r"^fused_split_kernel<64,\d+,bf16x3,6 terms,npw=\d,xm=[023]>", "probe", lambda r: g(r)["k"] == 3),       # split general, 3 x 3: taps in pairs + the ninth
            (r"^fused_split_kernel<64,\d+,bf16x3,6 terms,npw=\d,xm=[023]>", "dense", lambda r: g(r)["k"] == 3),
            (r"^fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=2>", "probe", lambda r: DS.PINS[r][1][0] == 1),       # the row tile
            (r"^fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=1>", "probe", None),                                  # one-pixel tile
            (r"^fused_split_kernel<32,128,bf16x3,6 terms", "probe", None),                                              # 32-channel tile
            (r"^fused_split_kernel<64,128,bf16x1,1 terms", "probe", None),                                              # bf16 mode
            (r"^fused_split_kernel<.*bf16x3,6 terms", "dense", lambda r: g(r)["Co"] % 32 and g(r)["Ci"] == 72),         # partial channel tile, 9 octets
            (r"^fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=0>", "probe", lambda r: g(r)["Ci"] == 3),            # stem quad, padded lane
            (r"^fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=0>", "dense", None),
            (r"^fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=0>", "probe", lambda r: g(r)["Ci"] == 3),
            (r"^fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=0>", "dense", None),
            (r"^fused_split_kernel<.*2x6 terms,flip,npw=\d,xm=1>", "probe", lambda r: g(r)["k"] == 1),                  # Flipout split, one tap
            (r"^fused_split_kernel<.*2x6 terms,flip,npw=\d,xm=1>", "dense", None),
            (r"^fused_split_kernel<.*2x6 terms,flip,npw=\d,xm=[023]>", "probe", lambda r: g(r)["k"] == 3),              # ... and 3 x 3
            (r"^fused_split_kernel<.*2x6 terms,flip,npw=\d,xm=[023]>", "dense", lambda r: g(r)["k"] == 3),
            (r"^fused_split_direct_kernel<.*resident W>", "probe", None), (r"^fused_split_direct_kernel<.*streamed W>", "probe", None),
            (r"^fused_split_skinny_kernel<.*split-K 64>", "probe", None), (r"^fused_split_skinny_kernel<.*split-K 64>", "dense", None),
            (r"^fused_split_skinny_kernel<.*split-K 128>", "probe", None), (r"^fused_split_skinny_kernel<.*split-K 128>", "dense", None),
            (r"^fused_fast_kernel<.*reparam,conv,trans,inj=0,xmode=1", "probe", lambda r: g(r)["G"] == 1),             # fp32 fast
            (r"^fused_fast_kernel<.*reparam,conv,trans,inj=0,xmode=1", "dense", lambda r: g(r)["G"] == 1),
            (r"^fused_fwd_kernel<.*reparam,conv,trans,inj=0>", "probe", lambda r: not DS.ROWS[r]["packs"]),             # fp32 general, without packs
            (r"^fused_fwd_kernel<.*reparam,conv,trans,inj=0>", "dense", None),
            (r"^fused_fast_kernel<128,32,4,", "probe", lambda r: DS.ROWS[r]["kind"] == "linear" and g(r)["Ci"] % 4),  # K % 4 != 0 Linear
            (r"^fused_fast_kernel<128,32,4,", "dense", lambda r: g(r)["Ci"] % 4),
            (r"^fused_f", "probe", lambda r: g(r)["G"] == 2 and g(r)["Ci"] // 2 == 6), (r"^fused_f", "dense", lambda r: g(r)["G"] == 2),      # groups 2, Cig = 6
            (r"^fused_split_kernel<.*6 terms,npw=8,xm=5>", "dense", lambda r: not DS.ROWS[r]["flip"]),                  # input-dilated fetch
            (r"^fused_split_kernel<.*flip,npw=8,xm=5>", "dense", None),
            (r"^fused_split_kernel<.*6 terms,npw=8,xm=6>", "dense", lambda r: not DS.ROWS[r]["flip"]),                  # depth-window fetch
            (r"^fused_split_kernel<.*flip,npw=8,xm=6>", "dense", None)):
        rows = [r for r in hit(pat, form) if more is None or more(r)]
        assert rows, (pat, form)
    for rid, row in DS.ROWS.items():      # shaped for seconds: eight launches of 128 samples (the streamed K = 512 row: two)
        assert row["S"] == DS.CHUNK and row["S_total"] == (256 if rid == "d_str" else 1024) and row["S_total"] % DS.CHUNK == 0
        if "dense" in row["forms"]:
            assert DS.geometry(row)["B"] >= 2
