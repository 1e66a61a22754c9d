#!/usr/bin/env python3
"""Generate tests/golden/avu_*.npz by RUNNING the reference's utils/avuc_loss.py (read-only, beside the repository; ``--reference``).

Runs only in the build container, like tools/make_goldens.py: the reference is imported and fed the seeded cases of
tests/_avu_ref.py; nothing of it is copied.  Per [B, C] case (avu_<tag>.npz): the inputs (z, y, th); the reference's fp32 AvULoss
value and autograd gradient at threshold th (ref_loss, ref_grad); AUAvULoss.auc_avu on the reference's own entropy (ref_auc; its
forward raises); eval_avu and accuracy_vs_uncertainty of the module's numpy functions on (argmax, y, that entropy); the float64 oracle
of tests/_avu_ref.evaluate at T = 1 and T = 21 (o1_*, o21_*); and in ``meta`` the reference's fp32 errors against the oracle on
every measure of the tolerance rule, the precondition's gaps, and the errors pooled over the groups.  Per MC case (avu_mc_<tag>.npz)
the same with the fp32 evaluation of the oracle expression as the reference (the reference has no MC form).  avu_surface.json: the
reference's parameter names, defaults and attributes; avu_numpy.npz: its entropy / predictive_entropy / mutual_information.

Every case asserts (a) the classification precondition of _avu_ref at T = 1 and T = 21 and (b), for the [B, C] cases, that the
reference's OWN last threshold, umin + float64(1.0) * fp32(umax - umin), reaches umax -- in other batches the most uncertain row is
"uncertain" at the last threshold by a rounding accident and ref_auc is not the intended value.

    python tools/make_avu_goldens.py [--reference DIR] [--search TAG]     (--search: print the seeds 0..39 that satisfy (a) and (b))
"""
import argparse
import inspect
import json
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np
import torch

import _avu_ref as R

OUT = os.path.join(REPO, "tests", "golden")
torch.set_num_threads(1)


def reference(path):
    sys.path.insert(0, path)
    tc = types.ModuleType("termcolor")       # (the reference's package import pulls it in for a coloured print)
    tc.colored = lambda s, *a, **k: s
    sys.modules.setdefault("termcolor", tc)
    import bayesian_torch.utils.avuc_loss as ref
    assert os.path.realpath(ref.__file__).startswith(os.path.realpath(path)), ref.__file__
    return ref


def ref_last_threshold_reaches_umax(unc):
    umin, umax = torch.min(unc), torch.max(unc)
    return (umin + torch.tensor(np.float64(1.0)) * (umax - umin)).item() >= umax.item()


def bc_conditions(z, y):
    th = R.mid_threshold(z, y, 0)
    with torch.no_grad():
        p = torch.softmax(z, 1)
        unc = -1 * torch.sum(p * torch.log(p + 1e-10), dim=-1)
    ok1, g1, need = R.gap_ok(z, y, 0, 1, th)
    ok21, g21, _ = R.gap_ok(z, y, 0, 21)
    return ok1 and ok21 and ref_last_threshold_reaches_umax(unc), dict(gap_T1=g1, gap_T21=g21, gap_needed=need), th


def bc_case(ref, tag):
    B, C, seed, covers = R.BC_CASES[tag]
    z, y = R.make_bc(tag, seed)
    ok, gaps, th = bc_conditions(z, y)
    assert ok, (tag, seed, gaps)
    zr = z.clone().requires_grad_()
    loss = ref.AvULoss(beta=R.BETA)(zr, y, float(th))
    loss.backward()
    au = ref.AUAvULoss(beta=R.BETA)
    with torch.no_grad():
        unc = au.entropy(torch.softmax(z, dim=1))
        ref_auc = float(au.auc_avu(z, y, unc))
    pred = torch.softmax(z, 1).argmax(1).numpy()
    avu, thr = ref.eval_avu(pred, y.numpy(), unc.numpy())
    o1, o21 = R.evaluate(z, y, 0, 1, th), R.evaluate(z, y, 0, 21)
    e1, e21 = R.evaluate(z, y, 0, 1, th, dtype=torch.float32), R.evaluate(z, y, 0, 21, dtype=torch.float32)
    err1, err21 = R.errors(e1, o1), R.errors(e21, o21)
    err1["loss"], err1["grad"] = R.error("loss", loss, o1["loss"]), R.error("grad", zr.grad, o1["grad"])    # the reference itself
    err21["v"] = R.error("v", ref_auc, o21["v"])
    arrs = dict(z=z.numpy(), y=y.numpy(), th=np.float32(th), ref_loss=loss.detach().numpy(), ref_grad=zr.grad.numpy(), ref_auc=np.float64(ref_auc),
                unc32=unc.numpy(), pred=pred, eval_avu_avu=avu, eval_avu_thr=thr,
                acc_vs_unc=np.float64(ref.accuracy_vs_uncertainty(pred, y.numpy(), unc.numpy(), float(th))))
    for k, o in (("o1", o1), ("o21", o21)):
        arrs.update({f"{k}_{m}": o[m].numpy() for m in ("loss", "v", "grad", "sums", "counts", "thresholds", "u")})
    meta = dict(tag=tag, B=B, C=C, seed=seed, covers=covers, beta=R.BETA, ref_err={R.bc_group(tag, 1): err1, R.bc_group(tag, 21): err21}, **gaps,
                conditions="the reference's own last threshold reaches umax; no row's float64 u nearer to a threshold than gap_needed = "
                           "64 x max |u_fp32 - u_fp64| (T = 1: gap_T1, T = 21: gap_T21)",
                ref_err_source=dict(T1="loss, grad: the reference's AvULoss and its autograd; v, sums: fp32 evaluation of the oracle expression",
                                    T21="v: the reference's AUAvULoss.auc_avu; loss, grad, sums: fp32 evaluation of the oracle expression"))
    return f"avu_{tag}.npz", arrs, meta


def mc_case(tag):
    S, B, C, seed = R.MC_CASES[tag]
    z, y = R.make_mc(tag, seed)
    arrs, errs, gaps = dict(z=z.numpy(), y=y.numpy()), {}, {}
    for ut in (0, 1):
        th = R.mid_threshold(z, y, ut)
        arrs[f"th_type{ut}"] = np.float32(th)
        for T in (1, 21):
            ok, g, need = R.gap_ok(z, y, ut, T, th)
            assert ok, (tag, seed, ut, T, g, need)
            gaps[f"gap_type{ut}_T{T}"], gaps[f"gap_needed_type{ut}"] = g, need
            o, e = R.evaluate(z, y, ut, T, th), R.evaluate(z, y, ut, T, th, dtype=torch.float32)
            errs[f"mc_type{ut}/T{T}"] = R.errors(e, o)
            arrs.update({f"o_type{ut}_T{T}_{m}": o[m].numpy() for m in ("loss", "v", "grad", "sums", "counts", "thresholds", "u")})
    meta = dict(tag=tag, S=S, B=B, C=C, seed=seed, beta=R.BETA, ref_err=errs, **gaps,
                ref_err_source="fp32 evaluation of the oracle expression on the CPU (the reference has no MC form)")
    return f"avu_mc_{tag}.npz", arrs, meta


def surface(ref):
    """avu_surface.json: the reference's parameter names and defaults; avu_numpy.npz: its numpy metrics on seeded MC probabilities."""
    def sig(f):
        ps = list(inspect.signature(f).parameters.values())
        return [[p.name, None if p.default is inspect.Parameter.empty else p.default] for p in ps if p.name != "self"]
    s = {f"{c}.{m}": sig(getattr(getattr(ref, c), m)) for c in ("AvULoss", "AUAvULoss")
         for m in ("__init__", "forward", "entropy", "expected_entropy", "predictive_uncertainty", "model_uncertainty", "accuracy_vs_uncertainty")}
    s["AUAvULoss.auc_avu"] = sig(ref.AUAvULoss.auc_avu)
    s.update({f: sig(getattr(ref, f)) for f in ("entropy", "predictive_entropy", "mutual_information", "eval_avu", "accuracy_vs_uncertainty")})
    s["attributes"] = {k: v for k, v in vars(ref.AvULoss(beta=2)).items() if not k.startswith("_") and k != "training"}
    with open(os.path.join(OUT, "avu_surface.json"), "w") as f:
        json.dump(s, f, indent=1, sort_keys=True)
    torch.manual_seed(11)
    mc = torch.softmax(torch.randn(4, 6, 5) * 2, -1).numpy()
    np.savez_compressed(os.path.join(OUT, "avu_numpy.npz"), mc_preds=mc, entropy=ref.entropy(mc), predictive_entropy=ref.predictive_entropy(mc),
                        mutual_information=ref.mutual_information(mc), meta=np.array(json.dumps(dict(seed=11, what="the reference's numpy metrics"))))
    print("  avu_surface.json, avu_numpy.npz")


def search(tag):
    good = []
    for seed in range(40):
        if tag in R.BC_CASES:
            ok = bc_conditions(*R.make_bc(tag, seed))[0]
        else:
            z, y = R.make_mc(tag, seed)
            ok = all(R.gap_ok(z, y, ut, T, R.mid_threshold(z, y, ut))[0] for ut in (0, 1) for T in (1, 21))
        if ok:
            good.append(seed)
    print(tag, good)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("BT_REFERENCE_DIR", os.path.join(os.path.dirname(REPO), "reference")))
    ap.add_argument("--search", default=None)
    args = ap.parse_args()
    if args.search:
        return search(args.search)
    ref = reference(args.reference)
    files = [bc_case(ref, tag) for tag in R.BC_CASES] + [mc_case(tag) for tag in R.MC_CASES]
    pooled = {}
    for _, _, meta in files:
        for key, e in meta["ref_err"].items():
            grp = pooled.setdefault(key.split("/")[0], {m: 0.0 for m in R.MEASURES})
            for m in R.MEASURES:
                grp[m] = max(grp[m], e[m])
    for name, arrs, meta in files:
        meta["pooled_ref_err"] = pooled
        path = os.path.join(OUT, name)
        np.savez_compressed(path, meta=np.array(json.dumps(meta, sort_keys=True)), **arrs)
        print(f"  {name}  {os.path.getsize(path) / 1024:.1f} KiB")
    surface(ref)
    print(json.dumps(pooled, indent=1))


if __name__ == "__main__":
    main()
