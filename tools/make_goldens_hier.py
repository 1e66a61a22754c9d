#!/usr/bin/env python3
"""Generate tests/golden/hier_*.npz and hier_surface.json by RUNNING the reference's hierarchical layers
(layers/variational_layers/hiearchial_variational_layers.py; read-only at /root/reference).

Runs only in the build container, like tools/make_goldens_lowrank.py: the reference is imported (``termcolor`` stubbed), run on the
CPU, and what it holds and computes is recorded. Nothing of the reference is copied. Each fixture has the layer's parameters, the
hyper-prior and prior-mean tensors (all set to non-default seeded values), an input, the reference's fp32 ``kl_loss()`` and forward KL,
and torch's fp32 autograd gradients of the forward KL with respect to every parameter.

Usage:  python tools/make_goldens_hier.py
"""
import inspect
import json
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, "/root/reference")
_tc = types.ModuleType("termcolor")
_tc.colored = lambda s, *a, **k: s
sys.modules["termcolor"] = _tc

import numpy as np
import torch

import bayesian_torch.layers.variational_layers as ref_pkg                                               # the reference
from bayesian_torch.layers.variational_layers import hiearchial_variational_layers as R

OUT = os.path.join(REPO, "tests", "golden")
torch.set_num_threads(8)

# tag -> (class name, ctor kwargs, input shape, names of the hyper-prior attributes)
CASES = {
    "lin_bias": ("LinearReparameterizationHierarchical_Weightwise", dict(in_features=7, out_features=5, bias=True), (3, 7),
                 ("prior_hypo_a_weight", "prior_hypo_b_weight")),
    "lin_nobias": ("LinearReparameterizationHierarchical_Weightwise", dict(in_features=7, out_features=5, bias=False), (3, 7),
                   ("prior_hypo_a_weight", "prior_hypo_b_weight")),
    "conv": ("Conv2dReparameterizationHierarchical_Weightwise", dict(in_channels=4, out_channels=6, kernel_size=3, padding=1, bias=False), (2, 4, 6, 6),
             ("prior_variance_hypo_a", "prior_variance_hypo_b")),
}


def npf(t):
    return t.detach().cpu().numpy().astype(np.float32)


def run_case(tag, cls, ctor, xshape, hypo, seed):
    torch.manual_seed(seed)
    layer = getattr(R, cls)(**ctor)
    w = layer.mu_weight if hasattr(layer, "mu_weight") else layer.mu_kernel
    names = [k for k, _ in layer.named_parameters()]
    la, lb = [getattr(layer, k) for k in names if k.startswith("log_a_q")][0], [getattr(layer, k) for k in names if k.startswith("log_b_q")][0]
    la.data.copy_(0.7 * torch.randn_like(w))
    lb.data.copy_(0.7 * torch.randn_like(w))
    setattr(layer, hypo[0], 0.5 + 2.5 * torch.rand_like(w))
    setattr(layer, hypo[1], 0.5 + 2.5 * torch.rand_like(w))
    layer.prior_weight_mu = 0.1 * torch.randn_like(w)       # a DNN's weights, as the fork's scripts set it
    x = torch.randn(*xshape)
    kl_loss = layer.kl_loss()
    out, kl_fwd = layer(x)
    grads = torch.autograd.grad(kl_fwd, [p for _, p in layer.named_parameters()])
    arrs = {k: npf(p) for k, p in layer.named_parameters()}
    arrs.update({"grad_" + k: npf(g) for (k, _), g in zip(layer.named_parameters(), grads)})
    arrs.update(a0=npf(getattr(layer, hypo[0])), b0=npf(getattr(layer, hypo[1])), prior_weight_mu=npf(layer.prior_weight_mu), x=npf(x),
                kl_loss=npf(kl_loss), kl_forward=npf(kl_fwd), out_shape=np.array(out.shape))
    if ctor["bias"]:
        arrs.update(prior_bias_mu=npf(layer.prior_bias_mu), prior_bias_sigma=npf(layer.prior_bias_sigma))
    meta = dict(cls=cls, ctor=ctor, seed=seed, hypo=list(hypo), parameters=names)
    arrs["meta"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, f"hier_{tag}.npz")
    np.savez_compressed(path, **arrs)
    print(f"  hier_{tag}.npz  {os.path.getsize(path) / 1024:.1f} KiB   kl_loss {float(kl_loss.detach()):.9g}  forward kl {float(kl_fwd.detach()):.9g}")


def err(f):
    try:
        f()
    except Exception as e:      # noqa: BLE001
        return dict(type=type(e).__name__, message=str(e))
    return None


def describe(cls, m, hypo):
    sig = inspect.signature(cls.__init__).parameters
    return dict(signature=list(sig)[1:], defaults={k: v.default for k, v in sig.items() if v.default is not inspect.Parameter.empty},
                forward=list(inspect.signature(cls.forward).parameters)[1:], state_dict={k: list(v.shape) for k, v in m.state_dict().items()},
                parameters=[k for k, _ in m.named_parameters()], buffers=[k for k, _ in m.named_buffers()], repr=repr(m),
                new_parameter_values=sorted({float(v) for k, p in m.named_parameters() if k.startswith("log_") for v in p.detach().reshape(-1)}),
                prior_type=m.prior_type,
                hypo={h: dict(shape=list(getattr(m, h).shape), values=sorted({float(v) for v in getattr(m, h).reshape(-1)}),
                              is_parameter=isinstance(getattr(m, h), torch.nn.Parameter), is_buffer=h in dict(m.named_buffers())) for h in hypo})


def surface():
    L, Cv = R.LinearReparameterizationHierarchical_Weightwise, R.Conv2dReparameterizationHierarchical_Weightwise
    hl, hc = CASES["lin_bias"][3], CASES["conv"][3]
    cb = Cv(4, 6, 3, bias=True)
    s = dict(linear=describe(L, L(7, 5), hl), linear_nobias=describe(L, L(7, 5, bias=False), hl), conv_nobias=describe(Cv, Cv(4, 6, 3, bias=False), hc),
             conv_hypo_args=sorted({float(v) for v in Cv(4, 6, 3, bias=False, prior_variance_hypo_a=2.0, prior_variance_hypo_b=3.0).prior_variance_hypo_a.reshape(-1)}),
             conv_bias_forward_error=err(lambda: cb(torch.randn(1, 4, 5, 5))), conv_bias_kl_loss_error=err(cb.kl_loss),
             not_weightwise={"LinearReparameterizationHierarchical": err(lambda: R.LinearReparameterizationHierarchical(7, 5)),
                             "Conv2dReparameterizationHierarchical": err(lambda: R.Conv2dReparameterizationHierarchical(4, 6, 3))},
             not_weightwise_signatures={n: list(inspect.signature(getattr(R, n).__init__).parameters)[1:]
                                        for n in ("LinearReparameterizationHierarchical", "Conv2dReparameterizationHierarchical")},
             star_imported={n: hasattr(ref_pkg, n) for n in ("LinearReparameterizationHierarchical_Weightwise", "Conv2dReparameterizationHierarchical_Weightwise")},
             constants=dict(HYPO_A=R.HYPO_A, HYPO_B=R.HYPO_B))
    with open(os.path.join(OUT, "hier_surface.json"), "w") as f:
        json.dump(s, f, indent=1, sort_keys=True)
    print("  hier_surface.json")


if __name__ == "__main__":
    for i, (tag, (cls, ctor, xshape, hypo)) in enumerate(CASES.items()):
        run_case(tag, cls, ctor, xshape, hypo, 300 + i)
    surface()
