#!/usr/bin/env python3
"""Generate tests/golden/lowrank_*.npz and lowrank_surface.json by RUNNING the reference's
Conv2dReparameterization_Multivariate (layers/variational_layers/conv_variational.py:409-648; read-only at /root/reference).

Runs only in the build container, like tools/make_goldens.py: the reference is imported (``termcolor`` stubbed), fed seeded inputs,
and (inputs, parameters, the z and eps it drew, output, KL) are recorded. Nothing of the reference is copied. The draws are
recovered by replaying the generator from the state it had before the forward -- z (rank values), then eps (n values), the order of
LowRankMultivariateNormal.rsample -- and the generator asserts that mu + L z + sqrt(D) eps reproduces the layer's output.
``kl`` is the layer's fp32 value, ``kl64`` the same class run with every tensor cast to float64 (``D_param`` is a plain attribute and
is cast by hand). Both are the normalised KL / n the forward returns.

Usage:  python tools/make_goldens_lowrank.py
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
import torch.nn.functional as TF

from bayesian_torch.layers.variational_layers.conv_variational import Conv2dReparameterization_Multivariate as Ref   # the reference

OUT = os.path.join(REPO, "tests", "golden")
torch.set_num_threads(8)

# tag -> (ctor kwargs, input H = W, what it covers)
CASES = {
    "a_r1_c4x8k3p1": (dict(in_channels=4, out_channels=8, kernel_size=3, padding=1, rank=1), 6, "the base case"),
    "b_r3_c5x6k3s2p1": (dict(in_channels=5, out_channels=6, kernel_size=3, stride=2, padding=1, rank=3), 6, "odd rank below the bound; channels not a multiple of 4"),
    "c_r4_c5x6k3p1": (dict(in_channels=5, out_channels=6, kernel_size=3, padding=1, rank=4), 6, "the in-kernel bound"),
    "d_r5_c4x8k3p1": (dict(in_channels=4, out_channels=8, kernel_size=3, padding=1, rank=5), 6, "first pre-pass rank"),
    "e_r432_c3x16k3p1": (dict(in_channels=3, out_channels=16, kernel_size=3, padding=1, rank=432), 6, "the fork's full-rank stem"),
    "f_r1_c1x6k5": (dict(in_channels=1, out_channels=6, kernel_size=5, padding=0, rank=1), 8, "the LeNet layer"),
    "g_r2_c8x4k1": (dict(in_channels=8, out_channels=4, kernel_size=1, rank=2), 6, "1x1 kernel"),
    "h_r1_c4x8k3p1_moped": (dict(in_channels=4, out_channels=8, kernel_size=3, padding=1, rank=1), 6, "non-zero prior_mean, non-uniform prior_cov_D"),
}


def npf(t):
    return t.detach().cpu().numpy().astype(np.float32)


def run_case(tag, ctor, hw, covers, seed):
    torch.manual_seed(seed)
    layer = Ref(**ctor)
    n, r = layer.weight_size, ctor["rank"]
    if tag.startswith("h_"):      # what Multivariate_MOPED leaves behind: a prior centred on trained weights, per-weight variances
        layer.prior_mean.data.copy_(0.05 * torch.randn(n))
        layer.prior_cov_D.data.copy_(0.5 + torch.rand(n))
    x = torch.randn(2, ctor["in_channels"], hw, hw)
    state = torch.get_rng_state()
    with torch.no_grad():
        out, kl = layer(x)
    torch.set_rng_state(state)
    z, eps = torch.empty(r).normal_(), torch.empty(n).normal_()
    w = layer.mu_kernel + layer.L_param @ z + torch.sqrt(layer.D_param) * eps
    k = ctor["kernel_size"]
    chk = TF.conv2d(x, w.view(ctor["out_channels"], ctor["in_channels"], k, k), None, ctor.get("stride", 1), ctor.get("padding", 0))
    assert torch.allclose(chk, out, rtol=1e-5, atol=1e-6), (tag, float((chk - out).abs().max()))
    # the same class in float64
    l64 = Ref(**ctor).double()
    l64.load_state_dict({k_: v.double() for k_, v in layer.state_dict().items()})
    l64.D_param = layer.D_param.double()
    with torch.no_grad():
        _, kl64 = l64(x.double())
    meta = dict(cls="Conv2dReparameterization_Multivariate", ctor=ctor, covers=covers, seed=seed, input_hw=hw)
    arrs = dict(x=npf(x), mu_kernel=npf(layer.mu_kernel), L_param=npf(layer.L_param), prior_mean=npf(layer.prior_mean), prior_cov_L=npf(layer.prior_cov_L),
                prior_cov_D=npf(layer.prior_cov_D), D_param=npf(layer.D_param), z=npf(z), eps=npf(eps), out=npf(out), kl=npf(kl),
                kl64=kl64.detach().numpy().astype(np.float64), meta=np.array(json.dumps(meta)))
    path = os.path.join(OUT, f"lowrank_{tag}.npz")
    np.savez_compressed(path, **arrs)
    print(f"  lowrank_{tag}.npz  {os.path.getsize(path) / 1024:.1f} KiB   kl {float(kl):.9g}  kl64 {float(kl64):.15g}")


def surface():
    m = Ref(4, 8, 3, rank=2)

    def err(f):
        try:
            f()
        except Exception as e:      # noqa: BLE001
            return dict(type=type(e).__name__, message=str(e))
        return None

    torch.manual_seed(5)
    big = Ref(16, 32, 3, rank=4)
    s = dict(signature=list(inspect.signature(Ref.__init__).parameters)[1:],
             defaults={k: v.default for k, v in inspect.signature(Ref.__init__).parameters.items() if v.default is not inspect.Parameter.empty},
             forward=list(inspect.signature(Ref.forward).parameters)[1:], return_kl_default=inspect.signature(Ref.forward).parameters["return_kl"].default,
             state_dict={k: list(v.shape) for k, v in m.state_dict().items()}, parameters=[k for k, _ in m.named_parameters()],
             buffers=[k for k, _ in m.named_buffers()], repr=repr(m),
             attributes=dict(weight_size=m.weight_size, martern_prior=m.martern_prior, BLOCK_MAT_shape=list(m.BLOCK_MAT.shape),
                             D_param_shape=list(m.D_param.shape), D_param_dtype=str(m.D_param.dtype), D_param_value=float(m.D_param[0]),
                             D_param_is_parameter=isinstance(m.D_param, torch.nn.Parameter), in_channels=m.in_channels, out_channels=m.out_channels,
                             kernel_size=m.kernel_size, stride=m.stride, padding=m.padding, dilation=m.dilation, groups=m.groups, bias=m.bias),
             init=dict(std=0.1, mean=0.0, prior_mean=0.0, prior_cov_L=0.0, prior_cov_D=1.0, n=big.weight_size),
             errors={"in_channels % groups": err(lambda: Ref(3, 8, 3, groups=2)), "out_channels % groups": err(lambda: Ref(4, 6, 3, groups=4))},
             in_all="Conv2dReparameterization_Multivariate" in __import__("bayesian_torch.layers.variational_layers.conv_variational", fromlist=["__all__"]).__all__)
    with open(os.path.join(OUT, "lowrank_surface.json"), "w") as f:
        json.dump(s, f, indent=1, sort_keys=True)
    print("  lowrank_surface.json")


if __name__ == "__main__":
    for i, (tag, (ctor, hw, covers)) in enumerate(CASES.items()):
        run_case(tag, ctor, hw, covers, 100 + i)
    surface()
