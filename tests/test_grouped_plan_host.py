"""Grouped and depthwise convolutions, the part that needs no GPU (tests/_group_cases.py holds the rows).

1. Through the plan-only seam every row reaches the kernel family its table cell names.  tests/test_gpu_grouped.py runs those
   rows on the device and asserts the same names: when the dispatch changes, THIS test says so first, and it is mended by moving the
   rows to shapes that reach the kernels again -- never by loosening what the GPU tests assert.
2. The rows can see a group bug: with x's channels rolled by one group (Cig) or the weight rows rolled by one group (Cog), the fp64
   oracle's output differs from the right one by more than 100 times the forward tolerance at 90 % or more of the output elements,
   so a kernel that reads a neighbouring group's activations or weights cannot pass the GPU comparison."""
import pytest
import torch

import _group_cases as GC

RTOL, ATOL = 1e-4, 1e-5


@pytest.mark.parametrize("rid", list(GC.ROWS))
def test_rows_reach_their_kernel_families(rid):
    for S in (1, 3):
        for what, flip, mode in (("Reparameterization auto", False, 0), ("Flipout auto", True, 0), ("Reparameterization f32", False, 1),
                                 ("Flipout f32", True, 1), ("Reparameterization bf16", False, 3), ("Flipout bf16", True, 3)):
            rc, name = GC.plan(rid, flip, mode, S)
            assert rc == 0, (rid, what, S, name)
            want = GC.want_family(rid, flip, mode)
            assert GC.family(name) == want, f"{rid} {what} S={S}: planned {name}, the table says {want}: move the row (tests/_group_cases.py)"
            if mode == 3 and not flip and want in GC.SPLIT_FAMILIES:
                assert "bf16x1,1 terms" in name, (rid, name)
            elif want in GC.SPLIT_FAMILIES:
                assert "bf16x3" in name, (rid, name)
            if mode == 0 and rid == "cog70" and not flip:
                from bayesian_torch_amd import _lib
                assert _lib.last_launch_info()["groups"] == 2 and _lib.last_launch_info()["n_tiles"] == 2, _lib.last_launch_info()


@pytest.mark.parametrize("rid", GC.GUARD_ROWS)
def test_displaced_operands_reach_the_family_the_guard_rows_assert(rid):
    for flip in (False, True):
        for S in (1, 3):
            rc, name = GC.plan(rid, flip, 0, S, off=1)
            assert rc == 0 and GC.family(name) == GC.GUARD_OFF1, (rid, flip, S, name)


def test_table_reaches_both_quad_kernels_and_the_general_split_kernel():
    cells = {(r["reparam"], r["flipout"]) for r in GC.ROWS.values()}
    assert {c[0] for c in cells} == {"quad512", "split128", "fast"} and {c[1] for c in cells} == {"quad256f", "split128f", "fast"}
    for rid, r in GC.ROWS.items():
        Ho, Wo = GC.out_hw(r)
        if r["reparam"] == "quad512":      # the quad tile is at least 75 % full
            assert r["B"] * Ho * Wo >= 384 and r["Ci"] // r["groups"] <= 4, rid


def _fraction_off(a, b):
    """Elements at which a differs from b by more than 100 times the forward tolerance, as a fraction."""
    tol = ATOL * float(b.abs().max()) + RTOL * b.abs()
    return float(((a - b).abs() > 100 * tol).double().mean())


@pytest.mark.parametrize("flip", [False, True], ids=["reparam", "flipout"])
@pytest.mark.parametrize("rid", list(GC.ROWS))
def test_rows_can_see_a_group_bug(rid, flip):
    r, t = GC.ROWS[rid], GC.inputs(rid)
    Cig, Cog = r["Ci"] // r["groups"], r["Co"] // r["groups"]
    d = GC.host_draws(rid, flip)
    xs = t["x"][:r["B"]]
    right = GC.oracle64(flip, t, xs, d, 0)
    # activations of the neighbouring group
    dx = dict(d, sign_in=d["sign_in"].roll(Cig, 2)) if flip else d
    wrong_x = GC.oracle64(flip, t, xs.roll(Cig, 1), dx, 0)
    # weights of the neighbouring group (the bias stays)
    tw = dict(t, mu=t["mu"].roll(Cog, 0), rho=t["rho"].roll(Cog, 0))
    wrong_w = GC.oracle64(flip, tw, xs, dict(d, eps_w=d["eps_w"].roll(Cog, 1)), 0)
    fx, fw = _fraction_off(wrong_x, right), _fraction_off(wrong_w, right)
    print(f"{rid} {'flipout' if flip else 'reparam'}: off by > 100 tol at {fx:.3f} (x rolled by Cig) and {fw:.3f} (weight rows rolled by Cog) of the outputs")
    assert fx >= 0.9 and fw >= 0.9, (rid, fx, fw)
