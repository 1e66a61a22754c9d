"""CPU: the edge cases of tests/_q8_edges.py are worth running -- before any kernel sees them. Per case: the step-by-step model
(``E.run``, whose convolution walks the kernel's taps in the kernel's index arithmetic) equals ``M.forward``; the ties and clamp hits
the case was built for are there, counted on the model; and each subtly wrong variant of a step (``E.MUTANTS``) that the case is meant
to catch changes at least 1 % of its outputs. The counts of EVERY variant are printed for every case (pytest -s). No kernels are launched.

The 1 % is a condition on the inputs, not a tolerance on anything: a variant listed for a case below that stops changing its answer
means the case's inputs lost their point. Every variant is carried by some case."""
import pytest
import torch

import _q8_edges as E
import _q8_model as M

CASES = E.all_cases()
W_SATURATING = ("golden conv_c19x10k3s2p1_z0", "golden linear_33x10_z0", "gpu cases")      # decimal sets whose w passes either clamp end on > 1 % of the weights


def relevant(cid, c, args):
    """The variants case ``cid`` is built to catch."""
    if cid.startswith("chain["):
        name, pat = args
        if name == "dyadic 2^-k":
            return {"away_w", "wide_p"} | ({"away_e"} if pat != 1 else set())      # (pattern 1 trades half of its e ties for odd e)
        if name == "dyadic eps, multipliers 0.5":
            return {"wide_p"}                     # its ties at e and p are real but s_mul / s_add = 0.009 hides them from w
        if name == "decimal, dyadic ratios":
            return {"away_w", "fused_w", "div_eps", "div_add", "wide_p", "wide_w"} | ({"away_p"} if pat == 2 else set())
        return {"wide_e", "wide_p"} | ({"wide_w"} if name in W_SATURATING else set())
    if cid.startswith("near-"):                   # (the division and the two-rounding sum move 0.85 % and 1.0 % of the third case)
        return {"away_oq", "bias_after_m", "m_double"} | ({"unfused_oq", "div_out"} if args[0] < 2 else set())
    if cid.startswith("inq-"):
        return {"away_xq", "wide_xq"} | ({"div_in"} if args[0] == "decimal" else set())
    out = set()
    z_in = c["pairs"][3][1]
    if cid.startswith("requant-") and args[2] != "full":
        out |= {"away_oq", "wide_oq"} | ({"div_out"} if args[2] == "half_decimal" else set())
        if args[2] == "half_decimal" and args[0] == "linear" and args[1] < 2:
            out |= {"unfused_oq", "bias_after_m"}
    else:
        out |= {"wide_p", "wide_w"}
    if z_in == 0:
        out.add("wide_xq")
    conv = c["conv"]
    if conv is not None:
        if c["wshape"][2] != c["wshape"][3]:
            out.add("decode_kh")
        out |= {"swap_" + k for k in ("stride", "padding", "dilation") if conv[k][0] != conv[k][1]}
        if z_in != 0 and max(conv["padding"]) > 0:
            out.add("pad_xq0")
        if E.walked_taps(conv, c["wshape"], c["x"].shape, z_in)[1]:
            out.add("prune_shift")
    return out


def test_every_variant_is_carried_by_some_case():
    carried = set()
    for cid, (fn, args) in CASES.items():
        carried |= relevant(cid, fn(*args), args)
    assert carried == set(E.MUTANTS), sorted(set(E.MUTANTS) - carried)


@pytest.mark.parametrize("cid", list(CASES))
def test_case_is_the_models_and_its_variants_change_it(cid):
    fn, args = CASES[cid]
    c = fn(*args)
    base = E.run_oq(c)
    assert torch.equal(base, c["oq"].to(torch.int32)), "the step-by-step model differs from M.forward"
    assert torch.equal(torch.cat([E.run(c, s)["out"] for s in range(c["S"])], 0), c["out"])
    n, want = base.numel(), relevant(cid, c, args)
    counts = {}
    for m in E.MUTANTS:
        if c["conv"] is None and m in E.GEOMETRY_MUTANTS:
            continue
        counts[m] = int((E.run_oq(c, m) != base).sum())
    print(f"{cid}: {n} outputs, {len(torch.unique(base))} levels; changed by " + ", ".join(f"{m}{'*' if m in want else ''} {v}" for m, v in counts.items()))
    for m in sorted(want):
        assert counts[m] * 100 >= n, (cid, m, counts[m], n)


# ---------------------------------------------------------------------------- C. what the chain cases hold, per scale set
@pytest.mark.parametrize("name", sorted(E.scale_sets()))
def test_chain_cases_reach_ties_and_clamp_ends(name):
    s_mu, s_sigma, s_eps, s_mul, s_add = E.scale_sets()[name]
    st = [E.stats(E.chain_case(name, pat)) for pat in E.CHAIN_PATTERNS]
    print(f"chain[{name}] (ties, low end, high end, levels) per pattern: " + "; ".join(str({r: tuple(s[r].values()) for r in "epw"}) for s in st))
    for pat, s in enumerate(st):
        c = E.chain_case(name, pat)
        assert s["p"]["levels"] == 256
        w = torch.stack([M.sampled_weight(c["q_mu"], c["q_sigma"], c["eps_w"][i], s_mu, s_sigma, s_eps, s_mul, s_add) for i in range(2)])
        assert torch.equal(c["oq"].view(2, 256, 256).to(torch.int32) - 128, w.transpose(1, 2).to(torch.int32))      # the read-out: oq - 128 IS w
        assert not torch.equal(w[0], w[1])
    if name == "dyadic 2^-k":
        assert all(s[r]["ties"] >= 1000 for s in st for r in "epw")
    elif name == "dyadic eps, multipliers 0.5":      # (a half-step eps makes every e even: the odd products p ties on need pattern 1's second sample)
        assert all(s["e"]["ties"] >= 1000 for s in st) and st[1]["p"]["ties"] >= 1000
    elif name == "decimal, dyadic ratios":
        assert all(s[r]["ties"] >= 1000 for s in st for r in "epw")
    if not E.is_tie_set(name) or name == "decimal, dyadic ratios":
        a = torch.tensor([-128, 127], dtype=torch.int8)
        reach = M.qadd(a, a, s_mul, s_mu, s_add).tolist() == [-128, 127]      # w is monotone in (p, q_mu): no saturation at the corners, none anywhere
        for r in ("e", "p") + (("w",) if reach else ()):
            assert sum(s[r]["lo"] for s in st) >= 100 and sum(s[r]["hi"] for s in st) >= 100, (name, r)
        if not reach:
            assert all(s["w"]["lo"] == 0 and s["w"]["hi"] == 0 for s in st)


# ---------------------------------------------------------------------------- D. the input quantiser cases
@pytest.mark.parametrize("z", E.Z_INS)
@pytest.mark.parametrize("kind", list(E.INQ_KINDS))
def test_input_cases_reach_ties_and_both_clamp_ends(kind, z):
    c = E.inq_case(kind, z)
    s = E.stats(c)["xq"]
    print(f"inq {kind} z_in={z}: {c['oq'].numel()} inputs, {s['ties']} ties, {s['lo']} / {s['hi']} at the clamp ends, {s['levels']} levels")
    assert torch.equal(c["oq"], M.quant_in(c["x"], *c["pairs"][3]))      # the read-out: oq IS xq
    assert s["lo"] >= 100 and s["hi"] >= 100 and s["levels"] >= 255
    if kind == "dyadic":
        assert s["ties"] >= 1000


# ---------------------------------------------------------------------------- E. the requantisation cases
@pytest.mark.parametrize("bias", E.REQ_TIE_BIASES)
@pytest.mark.parametrize("shape", ["linear", "conv"])
def test_requant_cases_are_half_ties_and_reach_both_clamp_ends(shape, bias):
    lo = hi = 0
    for zi in range(len(E.ZPAIRS)):
        c = E.requant_case(shape, zi, bias)
        s = E.stats(c)["oq"]
        away = int((E.run_oq(c, "away_oq") != c["oq"].to(torch.int32)).sum())
        print(f"requant {shape} bias={bias} z={E.ZPAIRS[zi]}: {c['oq'].numel()} outputs, {s['ties']} ties, {s['lo']} / {s['hi']} at the clamp ends, half-away changes {away}")
        assert 4 * s["ties"] >= c["oq"].numel()
        lo, hi = lo + s["lo"], hi + s["hi"]
    assert lo >= 100 and hi >= 100


# ---------------------------------------------------------------------------- F. the geometries
@pytest.mark.parametrize("name", list(E.GEOMS))
def test_geometry_table(name):
    (KH, KW, H, W, sh, sw, ph, pw, dh, dw), Ci, Co, B, live = E.GEOMS[name]
    conv = E.geom_conv(name)
    wshape, xshape = (Co, Ci, KH, KW), (B, Ci, H, W)
    assert E.live_taps(conv, wshape, xshape) == live
    walked, pruned = E.walked_taps(conv, wshape, xshape, 128)
    assert pruned == (KH * KW <= 16 and len(live) < KH * KW) and not E.walked_taps(conv, wshape, xshape, 57)[1]
    c = E.geom_case(name, 128)
    Ho, Wo = E.conv_out(conv, wshape, xshape)
    assert tuple(c["oq"].shape) == (B, Co, Ho, Wo) and len(torch.unique(c["oq"])) > 16


def test_geometry_table_covers_what_it_claims():
    G = E.GEOMS
    maps = {n: E.conv_out(E.geom_conv(n), (v[2], v[1]) + v[0][:2], (v[3], v[1]) + v[0][2:4]) for n, v in G.items()}
    uneven_maps = [n for n, (Ho, Wo) in maps.items() if G[n][3] * Ho * Wo > 128 and Ho != Wo]
    assert len(uneven_maps) >= 2                                             # a pixel tile crosses an image boundary with Ho != Wo
    assert any(v[1] == 16 for v in G.values()) and any(v[2] > 64 for v in G.values())
    pruned = [n for n, v in G.items() if v[0][0] * v[0][1] <= 16 and len(v[4]) < v[0][0] * v[0][1]]
    assert any((len(G[n][4]) * 2) % 4 for n in pruned)                       # live taps * CB is no multiple of the four-unit stage
    assert any(G[n][0][0] * G[n][0][1] == 16 for n in pruned)                # the 16-tap limit of the live-tap word, pruned
    assert any(v[0][0] * v[0][1] > 16 and len(v[4]) < v[0][0] * v[0][1] for v in G.values())      # dead taps that pruning may not drop
