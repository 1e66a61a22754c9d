"""CPU side of the guard-band tests: the helper tests itself on CPU tensors, every forward row of tests/_guard_rows.py plans the
kernel the table states -- aligned, with each operand alone displaced by 4, 8 and 12 bytes, and with all of them displaced -- through
the plan-only seam (made-up addresses, nothing launched), and the operands the library refuses to take misaligned are refused by
message.  This is the proof that a GPU row really takes another branch than its aligned twin."""
import ctypes as C
import re

import pytest
import torch

import _guard as G
import _guard_rows as GR


# ------------------------------------------------------------------------------------------------------------- the helper
@pytest.mark.parametrize("off", (0, 1, 2, 3))
def test_place_gives_the_offset_a_contiguous_view_and_the_values(off):
    t = torch.arange(2 * 3 * 5, dtype=torch.float32).reshape(2, 3, 5)
    v = G.place(t, off, band=8)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous() and v.shape == t.shape and torch.equal(v, t)
    base = v._base if v._base is not None else v
    flat = base.view(torch.float32) if base.dtype != torch.float32 else base
    start = (v.data_ptr() - flat.data_ptr()) // 4
    assert start >= 8 and flat.numel() - start - t.numel() >= 8
    assert bool(torch.isnan(flat[:start]).all()) and bool(torch.isnan(flat[start + t.numel():]).all())


@pytest.mark.parametrize("off", (0, 1, 2, 3))
@pytest.mark.parametrize("dtype", (torch.float32, torch.uint8))
def test_check_sees_band_writes_and_unwritten_elements(off, dtype):
    def fresh():
        g = G.place_result((3, 7), off, band=G.BAND, dtype=dtype, tag="t")
        assert g.view.data_ptr() % 16 == 4 * off and g.view.is_contiguous() and g.view.shape == (3, 7) and g.start >= G.BAND
        return g
    g = fresh()
    with pytest.raises(AssertionError, match="never written"):      # nothing written at all
        G.check(g)
    g.view.zero_()
    G.check(g)
    g = fresh()
    g.view.zero_()
    flat = g.view.reshape(-1)
    if dtype == torch.float32:
        flat.view(torch.int32)[11] = G._i32(G.PATTERN)             # one element left as it was
        with pytest.raises(AssertionError, match="word offset 11 was never written"):
            G.check(g)
        G.check(g, body=False)
        flat[11] = 0
    G.check(g)
    for where, rel in ((g.start - 1, -1), (g.start + g.n_words, g.n_words), (0, -g.start), (g.words.numel() - 1, g.words.numel() - 1 - g.start)):
        keep = int(g.words[where])
        g.words[where] = 0
        with pytest.raises(AssertionError, match=re.escape(f"word offset {rel} ")):
            G.check(g)
        g.words[where] = keep
        G.check(g)


def test_allocation_proxy_guards_and_restores():
    from bayesian_torch_amd import functional as F
    real = F.torch
    with G.guarded_allocations(lambda shape, dtype: 2 if len(shape) > 1 else 0, band=16) as log:
        a = F.torch.empty((2, 3), dtype=torch.float32, device="cpu")
        b = F.torch.empty_like(a)
        c = F.torch.empty(5, dtype=torch.uint8, device="cpu")
        k = F.torch.empty((), dtype=torch.float32, device="cpu")
        assert F.torch.float32 is torch.float32 and F.torch.zeros(2).sum() == 0
    assert F.torch is real and len(log) == 4
    assert [x.data_ptr() % 16 for x in (a, b, c, k)] == [8, 8, 0, 0] and k.dim() == 0 and c.dtype == torch.uint8
    for g in log[:2]:
        g.view.fill_(1.0)
    log[3].view.fill_(2.0)
    G.check_all(log)
    with pytest.raises(ZeroDivisionError):
        with G.guarded_allocations(1):
            1 / 0
    assert F.torch is real


# ------------------------------------------------------------------------------------------------------------- plan pins
@pytest.fixture(scope="module")
def seam():
    return GR.Seam()


@pytest.mark.parametrize("rid", list(GR.ROWS))
def test_row_plans_the_kernels_the_table_states(seam, rid):
    """Kernel name AND the stated launch-info fields, for the aligned plan and for every displaced one (a refusal: its text)."""
    row = GR.ROWS[rid]
    rc, name, info = seam.plan(row, 0, ())
    assert (rc, name, GR.info_of(info)) == (0, row["aligned"], row["info"]), (rid, name, info)
    assert set(row["single"]) <= set(row["ops"]) | {"out"} and set(row["single_info"]) <= set(row["ops"]) | {"out"}
    for off in (1, 2, 3):
        for op in row["ops"] + ("out",):
            want = row["single"].get(op, row["aligned"])
            rc1, got, info1 = seam.plan(row, off, (op,))
            assert got == want and (rc1 == 0) == want.startswith("fused_"), (rid, op, off, got)
            if rc1 == 0:
                assert GR.info_of(info1) == row["single_info"].get(op, row["info"]), (rid, op, off, info1)
                if want == row["aligned"] and op not in row["single_info"]:
                    assert info1 == info, (rid, op, off)
        if row["ops"]:
            rc2, got, info2 = seam.plan(row, off, row["ops"])
            assert got == row["together"] and (rc2 == 0) == got.startswith("fused_"), (rid, off, got)
            assert (None if rc2 else GR.info_of(info2)) == row["together_info"], (rid, off, info2)
    if row["pool"]:      # a displaced result takes the fused pool away (nothing launched): the unpooled launch plans
        assert seam.plan(dict(row, pool=False), 1, ("out",))[0] == 0


def test_rows_reach_every_family():
    """Every instantiation family and fetch mode the issue lists is the aligned launch of a row, and every row is run misaligned; the
    branches only the misaligned launches reach are among the displaced names."""
    aligned = {r["aligned"] for r in GR.ROWS.values()}
    displaced = {n for r in GR.ROWS.values() for n in list(r["single"].values()) + [r["together"]]}
    rx = lambda pat, names: any(re.search(pat, n) for n in names)
    for pat in ([r"^fused_split_kernel<64,128,bf16x3,6 terms,npw=8,xm=%d>" % m for m in (1, 2, 5)] +
                [r"^fused_split_kernel<64,(256|512),bf16x3,6 terms,npw=\d,xm=%d>" % m for m in (3, 4)] +
                [r"^fused_split_kernel<64,%d,bf16x3,6 terms" % w for w in (128, 256, 512)] +
                [r"^fused_split_kernel<32,128,bf16x3,6 terms", r"^fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=1>",
                 r"^fused_split_kernel<64,256,bf16x3,2x6 terms,flip,npw=4,xm=3>", r"^fused_split_kernel<64,128,bf16x3,2x6 terms,flip,npw=8,xm=5>",
                 r"^fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=0>", r"^fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=1>",
                 r"^fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=0>", r"^fused_split_quad_kernel<64,256,bf16x3,2x6 terms,flip,pool=1>",
                 r"^fused_split_direct_kernel<.*resident W>", r"^fused_split_direct_kernel<.*streamed W>",
                 r"^fused_split_skinny_kernel<.*split-K 64>", r"^fused_split_skinny_kernel<.*split-K 128>", r"^fused_split_kernel<64,128,bf16x1,1 terms",
                 r"^fused_fast_kernel<.*conv,trans,inj=0,xmode=2", r"^fused_fast_kernel<.*conv,trans,inj=0,xmode=1,npw=8,pool=0",
                 r"^fused_fast_kernel<.*pool=1>", r"^fused_fwd_kernel<.*reparam,conv,trans,inj=0>", r"^fused_fast_kernel<.*reparam,linear,trans",
                 r"^fused_fast_kernel<128,32,4,reparam,conv,trans", r"^fused_fwd_kernel<.*reparam,conv,trans,inj=1>", r"^fused_fwd_kernel<.*flip,conv,trans,inj=1>",
                 r"^fused_fwd_kernel<.*flip,linear,trans,inj=1>"]):
        assert rx(pat, aligned), pat
    for pat in (r"^fused_split_kernel<64,(128|256|512),bf16x3,6 terms,npw=\d,xm=0>", r"flip,npw=\d,xm=0>", r"bf16x1,1 terms,npw=8,xm=0>",
                r"^fused_fast_kernel<.*notrans.*xmode=1", r"^fused_fast_kernel<.*conv,trans,inj=0,xmode=0", r"^fused_fwd_kernel<.*notrans,inj=1>",
                r"^fused_fwd_kernel<32,128,1,reparam,conv,trans,inj=0>"):
        assert rx(pat, displaced), pat
    # what only the launch info shows: the row tile (the float2 output form), the whole four-pixel image tile (the float4 form), the
    # partial batch and channel tiles, the row-chunk staging's whole-image tiles, the fused KL's slices
    F = {k: i for i, k in enumerate(GR.INFO_FIELDS)}
    inf = lambda rid, k, which="info": GR.ROWS[rid][which][F[k]]
    for which in ("info", "together_info"):
        assert (inf("g_rowtile", "row_tiles", which), inf("g_rowtile", "t_R", which), inf("g_rowtile", "t_Wt", which)) == (1, 1, 2)
        assert GR.geometry(GR.ROWS["g_rowtile"])["Wo"] == 2
        g4 = GR.geometry(GR.ROWS["g_xm2_img4"])
        assert (inf("g_xm2_img4", "row_tiles", which), inf("g_xm2_img4", "t_R", which), inf("g_xm2_img4", "t_Wt", which)) == (0, g4["Ho"], g4["Wo"]) == (0, 2, 2)
        gb = GR.geometry(GR.ROWS["g_pbatch"])
        assert inf("g_pbatch", "t_NI", which) == gb["B"] == 120 and inf("g_pbatch", "m_tiles", which) == 1 and gb["Ho"] * gb["Wo"] == 1      # 120 of the tile's 128 columns
        gc = GR.geometry(GR.ROWS["g_pchan"])
        assert inf("g_pchan", "n_tiles", which) == 2 and gc["Co"] == 40                                                                   # 32 + 8 channels
        gr = GR.geometry(GR.ROWS["p_rows"])
        assert (inf("p_rows", "t_R", which), inf("p_rows", "t_Wt", which)) == (gr["Ho"], gr["Wo"])
    for rid in ("g_xm3_512", "g_xm3_256", "g_xm4", "g_flat", "f_256"):      # more than one tile of the wide widths
        assert inf(rid, "m_tiles") > 1, rid
    assert all(r["info"][F["kl_slices"]] >= 1 for r in GR.ROWS.values() if r["kl"])
    flat, walk, odd = GR.ROWS["g_flat"], GR.ROWS["q_walk"], GR.ROWS["p_oddx"]
    assert GR.geometry(flat)["W"] % 4 and flat["aligned"].endswith("xm=3>")          # xm 3 through x_flat
    assert walk["walk"] and walk["pool"] and walk["S"] >= 2 and not walk["stacked"]
    g = GR.geometry(odd)
    assert odd["stacked"] and (g["B"] * g["Ci"] * g["H"] * g["W"]) % 2 == 1             # an aligned x whose sample 1 is not
    for row in GR.ROWS.values():      # shaped for seconds
        g = GR.geometry(row)
        assert row["S"] <= 3 and (g["Ho"] * g["Wo"] <= 4096)


# ------------------------------------------------------------------------------------------------------------- refusals
def test_misaligned_packs_and_packed_draws_are_refused_before_any_launch():
    from bayesian_torch_amd import _lib
    L, P = _lib.lib(), GR.P
    geom = _lib.bt_conv2d_geom(2, 8, 4, 4, 16, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    draws = _lib.bt_draws(None, None, None, None, _lib.bt_rng(1, None, 0, 1, 0, 0))
    for mp, sp in ((P + 4, P), (P, P + 8), (P + 12, P + 12)):
        par = _lib.bt_params(P, P, None, None, None, None, None, None, mp, sp, 0, 0)
        rc = L.bt_conv2d_bwd_kl(C.byref(geom), 1, 0, P, 0, P, C.byref(par), C.byref(draws), None, P, P, P, P, 1 << 30, None)
        assert rc == -1 and L.bt_last_error_string().decode() == "bt_conv2d_bwd: mu_packed / sigma_packed must be 16-byte aligned"
    par = _lib.bt_params(P, P, None, None, None, None, None, None, P, P, 0, 0)
    for flip, fn in ((False, L.bt_reparam_conv2d_fwd), (True, L.bt_flipout_conv2d_fwd)):
        flags = _lib.DRAWS_EPS_PACKED | (_lib.DRAWS_SIGNS_PACKED if flip else 0)
        for eps, si, so, text in ((P + 4, P, P, "BT_DRAWS_EPS_PACKED: eps_w must be 16-byte aligned"),
                                  (P, P + 8, P, "BT_DRAWS_SIGNS_PACKED: sign_in / sign_out must be 16-byte aligned"),
                                  (P, P, P + 12, "BT_DRAWS_SIGNS_PACKED: sign_in / sign_out must be 16-byte aligned")):
            if not flip and "SIGNS" in text:
                continue
            d = _lib.bt_draws(eps, None, si if flip else None, so if flip else None, _lib.bt_rng(1, None, 0, 1, 0, flags))
            rc = fn(C.byref(geom), 1, P, 0, C.byref(par), C.byref(d), None, P, None, P, _lib.WORKSPACE_BYTES, None)
            assert rc == -1 and L.bt_last_error_string().decode().endswith(text), L.bt_last_error_string()
