"""CPU: the references of tests/test_gpu_grad_oracle.py checked on their own -- a broken reference must not widen a limit or
feed draws in the wrong order without a test noticing."""
import pytest
import torch

import _grad_cases as GC
from conftest import assert_close, load_golden


@pytest.mark.parametrize("row", range(len(GC.KL_ROWS)), ids=GC.KL_ROW_IDS)
def test_fp32_reference_of_the_kl_gradient_is_finite_and_accurate(row):
    """The GPU limits are KL_FACTOR times these figures: the oracle's own fp32 autograd against its float64 autograd, on the fixed
    inputs, must be finite and within 1e-6 in the scaled measure (it prints 1.7e-7 to 5.1e-7; the Laplace rows move in the second digit
    with the host's libm)."""
    r = GC.kl_row(row)
    for a in r["ref64"] + r["ref32"]:
        assert a.shape == (GC.KL_N,) and bool(torch.isfinite(a).all())
    print(f"{GC.KL_ROW_IDS[row]}: fp32 reference worst dmu {r['ref32_err']['dmu']:.3e} drho {r['ref32_err']['drho']:.3e}")
    for k, v in r["ref32_err"].items():
        assert 0.0 < v < 1e-6, (k, v)


@pytest.mark.parametrize("row", [0, 2], ids=[GC.KL_ROW_IDS[0], GC.KL_ROW_IDS[2]])
def test_aten_checker_of_the_kl_gradient_meets_the_kernel_limit_on_the_cpu(row):
    """autograd._kl_grads_aten (the closed forms "HIP equals checker" tests compare with) in fp32 torch ops on the CPU."""
    from bayesian_torch_amd.autograd import _kl_grads_aten
    r = GC.kl_row(row)
    t = r["inputs"]
    got = _kl_grads_aten(t["mu"], t["rho"], t["pmu"], t["psig"], torch.tensor(GC.KL_G), r["kind"])
    err, lim = GC.kl_errors(r["kind"], t["mu"], t["rho"], t["psig"], got, r["ref64"]), GC.kl_limits(row)
    print(f"{GC.KL_ROW_IDS[row]}: _kl_grads_aten (CPU) worst dmu {err['dmu']:.3e} drho {err['drho']:.3e}; limits {lim['dmu']:.3e} {lim['drho']:.3e}")
    assert err["dmu"] <= lim["dmu"] and err["drho"] <= lim["drho"], (err, lim)


def test_kl_measure_sees_a_prior_sigma_that_is_not_squared():
    """The measure is not vacuous: the normal-prior closed form with 1 / sigma_p in place of 1 / sigma_p^2, evaluated in float64,
    misses both limits by orders of magnitude, and a slice's reference is the row's scaled by n / numel(slice)."""
    r = GC.kl_row(0)
    t = {k: v.double() for k, v in r["inputs"].items()}
    sig = torch.log1p(torch.exp(t["rho"]))
    gs = GC.KL_G / GC.KL_N
    bad = ((t["mu"] - t["pmu"]) / t["psig"] * gs, (sig / t["psig"] - 1 / sig) * torch.sigmoid(t["rho"]) * gs)
    err, lim = GC.kl_errors("normal", t["mu"], t["rho"], t["psig"], bad, r["ref64"]), GC.kl_limits(0)
    assert err["dmu"] > 1e4 * lim["dmu"] and err["drho"] > 1e4 * lim["drho"], (err, lim)
    ts, ref = GC.kl_slice_ref(0, 1000, 257)
    assert ts["mu"].numel() == 257
    for a, b in zip(ref, r["ref64"]):
        assert torch.allclose(a, b[1000:1257] * (GC.KL_N / 257), rtol=1e-12, atol=0)


def test_kl_segment_layout():
    segs = GC.kl_segments()
    lens = [n for _, n in segs]
    assert len(segs) == 70 and {1, 2, 255, 256, 257, 1023, 1024, 1025} <= set(lens) and max(lens) >= 3000
    covered = torch.zeros(GC.KL_N, dtype=torch.bool)
    for s, n in segs:
        covered[s:s + n] = True
    assert bool(covered.all())
    assert any(n > 1024 for n in lens[:64]) and any(n > 1024 for n in lens[64:])      # both launches hold a segment of several blocks
    t = torch.arange(GC.KL_N, dtype=torch.float32)
    views = GC.odd_offset_views(t, segs)
    for (s, n), v in zip(segs, views):
        assert v.storage_offset() % 2 == 1 and v.is_contiguous() and torch.equal(v, t[s:s + n])
        assert v.untyped_storage().data_ptr() == views[0].untyped_storage().data_ptr()


@pytest.mark.parametrize("name", ["lstm_reparam_7x5", "lstm_flipout_7x5"])
def test_lstm_gradient_helper_reproduces_the_golden_forward(name):
    """The helper the GPU gradient test differentiates, in fp32: the reference's own hidden_seq / c_ts, so it feeds step t's draws to
    step t; and its float64 form gives finite gradients to x and all eight parameters."""
    g = load_golden(name)
    with torch.no_grad():
        hs, cs, _, _ = GC.lstm_ref_run(name, torch.float32)
    assert_close(hs, g["hidden_seq"], rtol=1e-5, atol_scale=1e-6, what=name + ".hidden_seq")
    assert_close(cs, g["c_ts"], rtol=1e-5, atol_scale=1e-6, what=name + ".c_ts")
    hs, cs, x, p = GC.lstm_ref_run(name, torch.float64)
    assert hs.dtype == torch.float64 and len(p) == 8
    g1, g2 = GC.lstm_upstream(hs.shape)
    ((hs * g1).sum() + (cs * g2).sum()).backward()
    for k, v in dict(p, x=x).items():
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0, k


# row -> (wgrad's workgroups per tile = sample groups x reduction chunks, dgrad's output-channel pieces) the table of part B names
DRAW_ROW_PLANS = {"A": (2 * 2, 3), "B": (2, 1), "C": (2, 1), "D": (2, 3), "E": (2, 3), "F": (1, 1), "G": (3, 5)}


@pytest.mark.parametrize("row_id", sorted(DRAW_ROW_PLANS))
def test_supplied_draw_rows_reach_the_planned_splits(row_id):
    """The rows of part B are chosen for the splits wgrad_groups / dgrad_chunks make of them.  bt_conv2d_bwd_workspace is a function
    of both planners (no device needed): 2 * groups partial planes of [Co][T][Cig4], then dchunks copies of dx when there are several
    pieces -- so a planner that stops splitting a row the way the table says fails here instead of leaving the row green and blunt."""
    import ctypes as C
    from bayesian_torch_amd import _lib
    _, _, ctor, xs, S = GC.DRAW_ROW[row_id]
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if "in_features" in ctor:
        B, Ci, H, W, Co, G = xs[0], ctor["in_features"], 1, 1, ctor["out_features"], 1
        (kh, kw), (sh, sw), (ph, pw), (dh, dw) = (1, 1), (1, 1), (0, 0), (1, 1)
    else:
        B, Ci, H, W, Co, G = xs[0], ctor["in_channels"], xs[2], xs[3], ctor["out_channels"], ctor.get("groups", 1)
        (kh, kw), (sh, sw), (ph, pw), (dh, dw) = [pair(ctor.get(k, d)) for k, d in (("kernel_size", 1), ("stride", 1), ("padding", 0), ("dilation", 1))]
    geom = _lib.bt_conv2d_geom(B, Ci, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, G)
    groups, pieces = DRAW_ROW_PLANS[row_id]
    Cig4 = (Ci // G + 3) // 4 * 4
    want = 4 * (2 * groups * Co * kh * kw * Cig4 + (pieces * S * B * Ci * H * W if pieces > 1 else 0))
    assert int(_lib.lib().bt_conv2d_bwd_workspace(C.byref(geom), S)) == want


@pytest.mark.parametrize("row_id", ["A", "D", "E", "G"])
def test_rows_with_dgrad_pieces_pair_when_both_gradients_are_asked_for(row_id):
    """Through the plan-only record (no device): with dx and the weight gradients asked for, the rows whose dgrad runs in pieces launch
    twice -- wgrad + dgrad in one grid, then the two finishing passes in one grid of n_wfin + n_dfin blocks of 256 threads (at most
    4096 each) -- and four times with pairing off, the last launch being wgrad's finishing pass alone."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("record_bwd_launches", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "record_bwd_launches.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    case, geom, S = next(t for t in rec.draw_row_geoms() if t[0] == "row" + row_id)
    B, Ci, H, W, Co, kh, kw = geom[:7]
    assert DRAW_ROW_PLANS[row_id][1] > 1
    n_wfin = min(4096, (Co * (Ci // geom[13]) * kh * kw + 255) // 256)
    n_dfin = min(4096, (S * B * Ci * H * W + 255) // 256)
    r = rec.Recorder()
    r.h.bt_debug_plan_only(1)
    try:
        for pair, launches, last in ((1, 2, n_wfin + n_dfin), (0, 4, n_wfin)):
            r.h.bt_debug_bwd_pair(pair)
            r.call(case, geom, S, "both", flip="Flipout" in GC.DRAW_ROW[row_id][1])
            line = r.lines["bt_conv2d_bwd"][-1].split("|")
            assert line[2] == "0" and int(line[4]) == launches, line
            assert list(r.rec[:6]) == [last, 1, 1, 256, 1, 1], (pair, list(r.rec[:9]))
    finally:
        r.h.bt_debug_bwd_pair(1)
        r.h.bt_debug_plan_only(0)
