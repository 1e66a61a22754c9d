"""AvUC losses, host side (no launch): the drop-in surface, the C ABI's argument validation, the numpy metrics and the float64 oracle
of tests/_avu_ref.py against what the reference recorded (tools/make_avu_goldens.py -> tests/golden/avu_*)."""
import ctypes
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _avu_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bt_avu_workspace_bytes", "bt_avu_fwd", "bt_avu_bwd")


def _sig(f):
    return [[p.name, None if p.default is inspect.Parameter.empty else p.default] for p in inspect.signature(f).parameters.values() if p.name != "self"]


def test_alias_import_and_reference_surface():
    from bayesian_torch.utils.avuc_loss import AvULoss, AUAvULoss                    # noqa: F401  (the reference's import path)
    import bayesian_torch.utils.avuc_loss as alias
    import bayesian_torch_amd.utils.avuc_loss as M
    with open(os.path.join(R.GOLD, "avu_surface.json")) as f:
        want = json.load(f)
    attrs = want.pop("attributes")
    for name, sig in want.items():
        obj = M
        for part in name.split("."):
            obj = getattr(obj, part)
        assert _sig(obj) == sig, (name, _sig(obj), sig)
        assert getattr(alias, name.split(".")[0]) is getattr(M, name.split(".")[0])
    m = M.AvULoss(beta=2)
    for k, v in attrs.items():
        assert getattr(m, k) == v, k
    assert "sklearn" not in open(M.__file__).read().replace("sklearn.metrics.auc", "")


def test_new_symbols_declared_exported_and_validated_on_the_host():
    from bayesian_torch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*\*?(bt_[a-z0-9_]+)\(", hdr, flags=re.M))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and name in _lib._PROTOS and hasattr(handle, name), name
    L = _lib.lib()
    assert L.bt_version() == 302
    assert L.bt_avu_workspace_bytes(3, 7, 5, 21) >= 4 * (6 * 7 + 2 * 3 * 7) and L.bt_avu_workspace_bytes(3, 7, 5, 2) == 0
    buf = (ctypes.c_double * 64)()          # a host buffer: every call below must return before any launch
    p = ctypes.addressof(buf)

    def fwd(S=1, B=4, C=3, logits=p, labels=p, ut=0, T=1, th=p, out=p, ws=p, nbytes=1 << 20):
        return L.bt_avu_fwd(S, B, C, logits, labels, ut, T, th, 1.0, out, out, out, out, out, out, ws, nbytes, None)

    def bwd(S=1, B=4, C=3, logits=p, ut=0, T=1, coef=p, g=p, ws=p, nbytes=1 << 20, dl=p):
        return L.bt_avu_bwd(S, B, C, logits, ut, T, coef, g, ws, nbytes, dl, None)
    bad = [dict(S=0), dict(B=0), dict(C=-1), dict(T=2), dict(T=0), dict(ut=2), dict(ut=-1), dict(ut=1, S=1), dict(logits=None), dict(labels=None),
           dict(th=None), dict(out=None), dict(ws=None), dict(ws=p + 4), dict(labels=p + 4)]
    for kw in bad:
        assert fwd(**kw) == -1 and b"bt_avu_fwd" in L.bt_last_error_string(), kw
    assert fwd(nbytes=8) == -3 and b"bt_avu_fwd" in L.bt_last_error_string()
    for kw in (dict(S=0), dict(B=-2), dict(C=0), dict(T=20), dict(ut=3), dict(ut=1, S=1), dict(logits=None), dict(coef=None), dict(g=None), dict(ws=None),
               dict(dl=None), dict(ws=p + 4)):
        assert bwd(**kw) == -1 and b"bt_avu_bwd" in L.bt_last_error_string(), kw
    assert bwd(nbytes=8) == -3 and b"bt_avu_bwd" in L.bt_last_error_string()


def test_cpu_tensors_and_type1_without_samples_are_refused():
    from bayesian_torch_amd import functional as F
    from bayesian_torch_amd.utils.avuc_loss import AvULoss, AUAvULoss
    z, y = torch.randn(4, 3), torch.tensor([0, 1, 2, 0])
    with pytest.raises(RuntimeError, match="HIP"):
        AvULoss()(z, y, 0.5)
    with pytest.raises(RuntimeError, match="HIP"):
        AUAvULoss()(z, y)
    with pytest.raises(RuntimeError, match="HIP"):
        F.avu_forward(z[None], y, 0, 21)
    for loss, args in ((AvULoss(), (0.5,)), (AUAvULoss(), ())):
        with pytest.raises(ValueError, match=r"\[S, B, C\]"):
            loss(z, y, *args, type=1)
        with pytest.raises(ValueError, match="S > 1"):
            loss(z[None], y, *args, type=1)
        with pytest.raises(ValueError):
            loss(z, y, *args, type=2)


def test_numpy_metrics_equal_the_reference():
    import bayesian_torch_amd.utils.avuc_loss as M
    with np.load(os.path.join(R.GOLD, "avu_numpy.npz")) as g:
        for f in ("entropy", "predictive_entropy", "mutual_information"):
            got = getattr(M, f)(g["mc_preds"])
            assert got.dtype == g[f].dtype and np.array_equal(got, g[f]), f
    for tag in R.BC_CASES:
        d = R.load(tag)
        avu, thr = M.eval_avu(d["pred"], d["y"], d["unc32"])
        assert avu.dtype == d["eval_avu_avu"].dtype and np.array_equal(avu, d["eval_avu_avu"]), tag
        assert thr.dtype == d["eval_avu_thr"].dtype and np.array_equal(thr, d["eval_avu_thr"]), tag
        got = M.accuracy_vs_uncertainty(d["pred"], d["y"], d["unc32"], float(d["th"]))
        assert isinstance(got, float) and got == float(d["acc_vs_unc"]), tag
        # the class method: the same metric in torch, nothing printed
        t = M.AvULoss().accuracy_vs_uncertainty(torch.from_numpy(d["pred"]), torch.from_numpy(d["y"]), torch.from_numpy(d["unc32"]), float(d["th"]))
        assert t.shape == (1,) and abs(float(t) - got) < 1e-6, tag


@pytest.mark.parametrize("tag", list(R.BC_CASES))
def test_oracle_reproduces_the_reference_within_its_recorded_error(tag):
    """The float64 oracle against the reference's recorded fp32 AvULoss value, its autograd gradient and auc_avu: each within the fp32
    error the generator recorded (it is that error by construction; a slack of 1e-6 of it for another machine's libm), and the oracle
    values themselves as recorded.  Also AUAvULoss.auc_avu of this project (torch ops, here on the CPU) against the reference's."""
    from _grad_cases import KL_FACTOR
    from bayesian_torch_amd.utils.avuc_loss import AUAvULoss
    assert R.FACTOR == KL_FACTOR
    d = R.load(tag)
    z, y, meta = torch.from_numpy(d["z"]), torch.from_numpy(d["y"]), d["meta"]
    z2, y2 = R.make_bc(tag, meta["seed"])
    assert torch.equal(z, z2) and torch.equal(y, y2)
    o1, o21 = R.evaluate(z, y, 0, 1, d["th"]), R.evaluate(z, y, 0, 21)
    for T, o, k in ((1, o1, "o1"), (21, o21, "o21")):
        ok, g, need = R.gap_ok(z, y, 0, T, d["th"])
        assert ok, (tag, T, g, need)
        for m in R.MEASURES:
            assert R.error(m, o[m], d[f"{k}_{m}"]) <= 1e-12, (tag, T, m)
        assert np.array_equal(o["counts"].numpy(), d[f"{k}_counts"])
    e1, e21 = meta["ref_err"][R.bc_group(tag, 1)], meta["ref_err"][R.bc_group(tag, 21)]
    slack = lambda e: e * (1 + 1e-6) + 1e-15   # noqa: E731
    assert R.error("loss", d["ref_loss"], o1["loss"]) <= slack(e1["loss"])
    assert R.error("grad", d["ref_grad"], o1["grad"]) <= slack(e1["grad"])
    assert R.error("v", d["ref_auc"], o21["v"]) <= slack(e21["v"])
    for grp, e in meta["ref_err"].items():
        for m in R.MEASURES:
            assert e[m] <= meta["pooled_ref_err"][grp][m]
    mine = AUAvULoss(beta=R.BETA).auc_avu(z, y, torch.from_numpy(d["unc32"]))
    # both form AvU_j in [0, 1] from fp32 sums of the SAME B fp32 terms (one softmax, one tanh), in different orders: a sum of n terms is
    # within n 2^-24 of exact, relative; numerator and denominator each, plus the quotient's and the trapezoid's few roundings
    assert mine.shape == (1,) and abs(float(mine) - float(d["ref_auc"])) <= (2 * meta["B"] + 8) * 2.0 ** -24
    if tag == "b1c3_inacc":
        assert float(o1["v"]) == 0.0 and abs(float(o1["loss"]) + R.BETA * np.log(1e-10)) < 1e-12 and torch.isfinite(o1["grad"]).all()


def test_mc_fixtures_hold_the_precondition_and_the_recorded_oracle():
    for tag in R.MC_CASES:
        d = R.load(f"mc_{tag}")
        z, y = torch.from_numpy(d["z"]), torch.from_numpy(d["y"])
        z2, y2 = R.make_mc(tag, d["meta"]["seed"])
        assert torch.equal(z, z2) and torch.equal(y, y2)
        for ut in (0, 1):
            for T in (1, 21):
                th = d[f"th_type{ut}"]
                ok, g, need = R.gap_ok(z, y, ut, T, th)
                assert ok, (tag, ut, T, g, need)
                o = R.evaluate(z, y, ut, T, th)
                for m in R.MEASURES:
                    assert R.error(m, o[m], d[f"o_type{ut}_T{T}_{m}"]) <= 1e-12, (tag, ut, T, m)
                e32 = R.errors(R.evaluate(z, y, ut, T, th, dtype=torch.float32), o)
                for m in R.MEASURES:
                    assert d["meta"]["ref_err"][f"mc_type{ut}/T{T}"][m] <= d["meta"]["pooled_ref_err"][f"mc_type{ut}"][m]
                    assert np.isfinite(e32[m])
