"""A float64 CPU reference of the low-rank multivariate Conv2d layer, written for the tests (no kernels, nothing of the package under
test): the sampled weight w = mu + L z + sqrt(D) eps, F.conv2d in double, and the closed-form KL against a diagonal prior.  A plain
module, imported the way _grad_cases.py is."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as TF

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(f[len("lowrank_"):-4] for f in os.listdir(GOLD) if f.startswith("lowrank_") and f.endswith(".npz"))
MAX_R = 4      # ranks the forward kernel multiplies in registers
_cache = {}


def load(tag):
    """One fixture, loaded once and shared: tensors (fp32, ``kl64`` fp64) + ``meta``."""
    if tag not in _cache:
        d = np.load(os.path.join(GOLD, f"lowrank_{tag}.npz"))
        _cache[tag] = {k: (json.loads(str(d[k])) if k == "meta" else torch.from_numpy(d[k])) for k in d.files}
    return _cache[tag]


def case(letter):
    return next(t for t in CASES if t.startswith(letter + "_"))


def expected_path(rank):
    return "in_kernel" if rank <= MAX_R else "mean_prepass"


def two(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def weights(mu, L, D, z, eps):
    """[S, n] sampled weights in double: mu + z @ L^T + sqrt(D) * eps."""
    return mu.double() + z.double() @ L.double().t() + torch.sqrt(D.double()) * eps.double()


def forward(x, mu, L, D, z, eps, ctor, shared=True):
    """x [B, ...] (shared by the S samples) or [S * B, ...] -> out [S * B, Co, Ho, Wo] in double."""
    S = z.shape[0]
    w = weights(mu, L, D, z, eps)
    k = ctor["kernel_size"]
    xs = x.double()
    B = xs.shape[0] if shared else xs.shape[0] // S
    outs = []
    for s in range(S):
        xb = xs if shared else xs[s * B:(s + 1) * B]
        outs.append(TF.conv2d(xb, w[s].view(ctor["out_channels"], ctor["in_channels"], k, k), None, two(ctor.get("stride", 1)), two(ctor.get("padding", 0)),
                              two(ctor.get("dilation", 1)), 1))
    return torch.cat(outs, 0)


def kl_diag(mu, L, D, prior_mean, prior_var):
    """KL( N(mu, L L^T + diag D) || N(prior_mean, diag prior_var) ), un-normalised, double; differentiable."""
    mu, L, D, m, P = (t.double() for t in (mu, L, D, prior_mean, prior_var))
    n, r = L.shape
    G = torch.eye(r, dtype=torch.float64) + L.t() @ (L / D[:, None])
    return 0.5 * (torch.log(P).sum() - torch.log(D).sum() - torch.logdet(G) + ((D + (L * L).sum(1)) / P).sum() + ((mu - m) ** 2 / P).sum() - n)


def kl_general(mu, L, D, prior_mean, prior_L, prior_D):
    """The same against a low-rank prior, by torch.distributions in double (CPU)."""
    from torch.distributions import LowRankMultivariateNormal, kl_divergence
    q = LowRankMultivariateNormal(mu.double(), L.double(), D.double())
    p = LowRankMultivariateNormal(prior_mean.double(), prior_L.double(), prior_D.double())
    return kl_divergence(q, p)
