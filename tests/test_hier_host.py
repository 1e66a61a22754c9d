"""The hierarchical layers, host side (no launch): the drop-in surface against what the reference recorded
(tools/make_goldens_hier.py -> tests/golden/hier_*), the refusals, the C ABI's declarations and argument validation, the float64
oracle of tests/_hier_ref.py against the reference's recorded values, and the kernels' special functions evaluated on the CPU
(bt_special_eval) against torch.special in double."""
import ctypes
import inspect
import json
import math
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _hier_ref as R  # noqa: E402
from conftest import GOLD, load_golden  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bt_kl_hier", "bt_kl_hier_bwd", "bt_special_eval")
FIXTURES = R.FIXTURES


def _surface():
    with open(os.path.join(GOLD, "hier_surface.json")) as f:
        return json.load(f)


def _describe(cls, m, hypo):
    sig = inspect.signature(cls.__init__).parameters
    return dict(signature=list(sig)[1:], defaults={k: v.default for k, v in sig.items() if v.default is not inspect.Parameter.empty},
                state_dict={k: list(v.shape) for k, v in m.state_dict().items()}, parameters=[k for k, _ in m.named_parameters()],
                buffers=[k for k, _ in m.named_buffers() if not k.startswith("post_")], repr=repr(m),
                new_parameter_values=sorted({float(v) for k, p in m.named_parameters() if k.startswith("log_") for v in p.detach().reshape(-1)}),
                prior_type=m.prior_type,
                hypo={h: dict(shape=list(getattr(m, h).shape), values=sorted({float(v) for v in getattr(m, h).reshape(-1)}),
                              is_parameter=isinstance(getattr(m, h), torch.nn.Parameter), is_buffer=h in dict(m.named_buffers())) for h in hypo})


def test_surface_matches_the_reference():
    import bayesian_torch.layers.variational_layers.hiearchial_variational_layers as alias        # the reference's import path, spelling included
    import bayesian_torch_amd.layers as layers
    import bayesian_torch_amd.layers.variational_layers as vl
    import bayesian_torch_amd.layers.variational_layers.hiearchial_variational_layers as M
    want = _surface()
    L, Cv = M.LinearReparameterizationHierarchical_Weightwise, M.Conv2dReparameterizationHierarchical_Weightwise
    hl, hc = ("prior_hypo_a_weight", "prior_hypo_b_weight"), ("prior_variance_hypo_a", "prior_variance_hypo_b")
    for key, cls, m, hypo in (("linear", L, L(7, 5), hl), ("linear_nobias", L, L(7, 5, bias=False), hl), ("conv_nobias", Cv, Cv(4, 6, 3, bias=False), hc)):
        got, ref = _describe(cls, m, hypo), dict(want[key])
        fwd = ref.pop("forward")
        assert got == ref, (key, {k: (got[k], ref[k]) for k in ref if got[k] != ref[k]})
        assert list(inspect.signature(cls.forward).parameters)[1:1 + len(fwd)] == fwd
        assert inspect.signature(cls.forward).parameters["return_kl"].default is True
    assert sorted({float(v) for v in Cv(4, 6, 3, bias=False, prior_variance_hypo_a=2.0, prior_variance_hypo_b=3.0).prior_variance_hypo_a.reshape(-1)}) == want["conv_hypo_args"]
    assert float(Cv(4, 6, 3, bias=False, prior_variance_hypo_b=3.0).prior_variance_hypo_b[0, 0, 0, 0]) == 3.0
    for name, sig in want["not_weightwise_signatures"].items():
        assert list(inspect.signature(getattr(M, name).__init__).parameters)[1:] == sig
    assert dict(HYPO_A=M.HYPO_A, HYPO_B=M.HYPO_B) == want["constants"]
    for name, star in want["star_imported"].items():
        assert getattr(alias, name) is getattr(M, name)
        assert hasattr(vl, name) == star and hasattr(layers, name) == star      # reached by the module path only, as in the reference


def test_refusals():
    from bayesian_torch_amd import mc
    import bayesian_torch_amd.layers.variational_layers.hiearchial_variational_layers as M
    want = _surface()
    for name, e in want["not_weightwise"].items():
        args = (7, 5) if name.startswith("Linear") else (4, 6, 3)
        with pytest.raises(NotImplementedError) as ei:
            getattr(M, name)(*args)
        assert e["type"] == "NotImplementedError" and str(ei.value) == e["message"]
    assert want["conv_bias_forward_error"]["type"] == "RuntimeError"      # why: the reference's own forward cannot run with a bias
    with pytest.raises(NotImplementedError, match="reference's own forward cannot run"):
        M.Conv2dReparameterizationHierarchical_Weightwise(4, 6, 3)
    with pytest.raises(NotImplementedError, match="bias=False"):
        M.Conv2dReparameterizationHierarchical_Weightwise(4, 6, 3, bias=True)
    lin, conv = M.LinearReparameterizationHierarchical_Weightwise(7, 5), M.Conv2dReparameterizationHierarchical_Weightwise(4, 6, 3, bias=False)
    for layer, x in ((lin, torch.randn(3, 7)), (conv, torch.randn(2, 4, 5, 5))):
        with pytest.raises(RuntimeError, match="HIP"):
            layer(x)
        with pytest.raises(RuntimeError, match="HIP"):
            layer.kl_loss()
        with mc.mc_samples(1, x.shape[0]) as ctx:
            ctx.train_fused = True
            with pytest.raises(RuntimeError, match=r"TrainGraph\(fused=True\)"):
                layer(x)


def test_new_symbols_declared_exported_and_validated_on_the_host():
    from bayesian_torch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*\*?(bt_[a-z0-9_]+)\(", hdr, flags=re.M))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(handle, name), name
        decl = re.search(r"^int " + name + r"\((.*?)\);", hdr, flags=re.M | re.S).group(1)
        assert decl.count(",") + 1 == len(_lib._PROTOS[name][1]), name
    L = _lib.lib()
    assert L.bt_version() == 302
    buf = (ctypes.c_double * 64)()          # a host buffer: every call below must return before any launch
    p = ctypes.addressof(buf)
    vp = ctypes.c_void_p

    def arr(n, v=p):
        return (vp * max(n, 1))(*([v] * max(n, 1)))

    def fwd(n=2, null_array=None, null_entry=None, numel=5, out=p, ws=p, nbytes=_lib.WORKSPACE_BYTES, lay=None):
        a = [arr(n) for _ in range(7)]
        if null_entry is not None:
            a[null_entry][n - 1] = None
        if null_array is not None:
            a[null_array] = None
        ne = (ctypes.c_int64 * max(n, 1))(*([numel] * max(n, 1)))
        ly = None if lay is None else (ctypes.c_int32 * n)(*lay)
        return L.bt_kl_hier(n, *a, ne, ly, out, None, ws, nbytes, None)

    def bwd(n=2, null_array=None, null_entry=None, numel=5, g=p, outs=True):
        a = [arr(n) for _ in range(7)]
        if null_entry is not None:
            a[null_entry][n - 1] = None
        if null_array is not None:
            a[null_array] = None
        ne = (ctypes.c_int64 * max(n, 1))(*([numel] * max(n, 1)))
        o = [arr(n) if outs else None for _ in range(4)]
        return L.bt_kl_hier_bwd(n, *a, ne, g, *o, None)

    bad = [dict(n=0), dict(n=-1), dict(n=65), dict(numel=0), dict(numel=-3), dict(out=None), dict(ws=None), dict(nbytes=_lib.WORKSPACE_BYTES - 1), dict(lay=[1, 0])]
    bad += [dict(null_array=i) for i in range(7)] + [dict(null_entry=i) for i in range(7)]
    for kw in bad:
        assert fwd(**kw) == -1 and b"bt_kl_hier" in L.bt_last_error_string(), kw
    bad = [dict(n=0), dict(n=65), dict(numel=0), dict(g=None), dict(outs=False)] + [dict(null_array=i) for i in range(7)] + [dict(null_entry=i) for i in range(7)]
    for kw in bad:
        assert bwd(**kw) == -1 and b"bt_kl_hier_bwd" in L.bt_last_error_string(), kw
    x = (ctypes.c_float * 4)(1, 2, 3, 4)
    f32p = ctypes.POINTER(ctypes.c_float)
    for kind, xs, n, out in ((-1, x, 4, x), (4, x, 4, x), (0, None, 4, x), (0, x, 0, x), (0, x, 4, None)):
        assert L.bt_special_eval(kind, None if xs is None else ctypes.cast(xs, f32p), n, None if out is None else ctypes.cast(out, f32p)) == -1
        assert b"bt_special_eval" in L.bt_last_error_string()
    with pytest.raises(RuntimeError, match="HIP"):
        _lib.kl_hier([tuple(torch.ones(3) for _ in range(7))])


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_the_reference_recorded_kl(name):
    """The reference's fp32 kl_loss() and forward KL against the float64 oracle: within 4 units of 2^-23 (n + U) -- the fp32 formula
    reaches about 3 units of 2^-23 (1 + U_i) per element (printed below for the fixed rows), and its pairwise sum adds less than one."""
    g = load_golden(name)
    kl_loss, U, fwd = R.fixture_oracle(g)
    n = g["a0"].numel()
    tol = 4 * R.UNIT * (n + U)
    e1, e2 = abs(float(g["kl_loss"]) - kl_loss), abs(float(g["kl_forward"]) - fwd)
    print(f"{name}: oracle kl_loss {kl_loss:.12g} (recorded {float(g['kl_loss']):.9g}, off {e1:.3g}), forward {fwd:.12g} (off {e2:.3g}), tolerance {tol:.3g}")
    assert e1 <= tol and e2 <= tol
    assert (name == "hier_lin_bias") == (abs(fwd - kl_loss) > 0)


def test_fixed_rows_are_finite_and_the_fp32_yardstick_is_what_the_limits_say():
    for i in range(len(R.ROWS)):
        o, go = R.oracle(i), R.grad_oracle(i)
        print(f"row {R.ROW_IDS[i]}: fp32 formula worst per-element error {o['ref32_err']:.3f} units, sum error {R.sum_limit(i, torch.arange(R.N))[3]:.3f} units; "
              f"fp32 autograd worst errors {', '.join(f'{k} {v:.3f}' for k, v in go['ref32_err'].items())}")
        assert 0 < o["ref32_err"] < 64 and all(0 < v < 64 for v in go["ref32_err"].values())


# ----------------------------------------------------------------------------------------------------------- special functions
def _special_points():
    """1e5 fp32 points of [e^-20, e^20]: a geometric sweep, and dense linear sweeps around psi's root (1.4616) and around the
    recurrence threshold of csrc/bt_special.h (6), the threshold and its two neighbours included."""
    x = torch.cat([torch.exp(torch.linspace(-20, 20, 60000, dtype=torch.float64)), torch.linspace(1.36, 1.56, 20000, dtype=torch.float64),
                   torch.linspace(5.9, 6.1, 19997, dtype=torch.float64)]).float()
    six = torch.tensor(6.0)
    return torch.cat([x, torch.stack([six, torch.nextafter(six, torch.tensor(0.0)), torch.nextafter(six, torch.tensor(7.0))])])


def _ulp(v):
    """The fp32 ulp of |v| (float64 tensor, v > 0)."""
    return torch.exp2(torch.floor(torch.log2(v)) - 23)


def _special_cases(x):
    """kind -> (name, float64 reference, torch's own fp32 evaluation, uncancelled intermediate size S >= |f|).  digamma: the
    recurrence psi(x) = psi(x + N) - sum_{k<N} 1/(x + k) up to 10, as torch's fp32 digamma runs it, S = |psi(x + N)| + the sum;
    x psi' - 1: S = x psi' + 1; trigamma and lgamma are sums of one sign / library calls: S = |f|."""
    xd = x.double()
    N = torch.clamp(torch.ceil(10.0 - xd), min=0)
    rec = torch.zeros_like(xd)
    for k in range(10):
        rec = rec + torch.where(N > k, 1.0 / (xd + k), torch.zeros_like(xd))
    psi, psi1 = torch.special.digamma(xd), torch.special.polygamma(1, xd)
    return {0: ("digamma", psi, torch.digamma(x), torch.special.digamma(xd + N).abs() + rec),
            1: ("trigamma", psi1, torch.special.polygamma(1, x), psi1),
            2: ("lgamma", torch.special.gammaln(xd), torch.lgamma(x), torch.special.gammaln(xd).abs()),
            3: ("x*trigamma-1", xd * psi1 - 1.0, x * torch.special.polygamma(1, x) - 1.0, xd * psi1 + 1.0)}


def test_special_functions_on_the_cpu():
    """bt_special_eval (the kernels' source, compiled for the host) against torch.special in double: at most 8 x the worst error of
    torch's own fp32 evaluation at the same points, in ulps of max(|f|, S)."""
    from bayesian_torch_amd import _lib
    x = _special_points()
    assert x.numel() == 100000 and float(x.min()) < 2.1e-9 and float(x.max()) > 4.8e8
    for kind, (name, ref, t32, S) in _special_cases(x).items():
        got = _lib.special_eval(kind, x)
        assert bool(torch.isfinite(got).all()), name
        unit = _ulp(torch.maximum(ref.abs(), S).clamp_min(1e-300))
        e_got, e_t32 = (got.double() - ref).abs() / unit, (t32.double() - ref).abs() / unit
        i = int(e_got.argmax())
        print(f"{name}: worst error {float(e_got.max()):.3f} ulp at x = {float(x[i]):.9g} (torch fp32: {float(e_t32.max()):.3f} ulp, limit {8 * float(e_t32.max()):.3f})")
        assert float(e_got.max()) <= 8 * float(e_t32.max()), name
    # x psi'(x) - 1 keeps RELATIVE accuracy where the fp32 composition has cancelled to nothing
    big = x[x >= 6]
    ref = big.double() * torch.special.polygamma(1, big.double()) - 1.0
    rel = ((_lib.special_eval(3, big).double() - ref) / ref).abs()
    print(f"x*trigamma-1, x >= 6: worst relative error {float(rel.max()):.3g}")
    assert float(rel.max()) < 8 * R.UNIT
