"""float64 CPU oracle of the hierarchical (inverse-gamma hyper-prior) KL, its fixed input rows and its error measure, shared by
test_hier_host.py (CPU) and test_gpu_hier.py (GPU).  A plain module: no fixtures, no pytest hooks.  It is written from the formula
alone -- torch.special in double -- and holds nothing of the package.

Per element, a = exp(log_a), b = exp(log_b), sigma = log1p(exp(rho)), m = prior_mu, (a0, b0) the hyper-prior:
    A = 1/2 [ ln b - psi(a) - ln sigma^2 + (a/b) sigma^2 + (a/b)(mu - m)^2 - 1 ]
    B = (a - a0) psi(a) - lnGamma(a) + lnGamma(a0) + a0 (ln b - ln b0) + (b0 - b)(a/b)
Eleven addends; kl = SUM (A + B).

Error measure (the one of _grad_cases.py): against the UNCANCELLED size U = sum of the addends' absolute values, in units of
2^-23 (1 + U).  A kernel may reach KL_FACTOR times the worst error the same formula evaluated with torch in fp32 on the CPU reaches
on the same inputs; on a sum never less than one unit (the result is one fp32 number).  Gradients: relative to the uncancelled size
of each closed form (``grad_scales``), in units of 2^-23 of it; the fp32 yardstick is described at ``grad_oracle``.
"""
import functools
import math

import torch

N = 4001
KL_FACTOR = 8.0          # the project's factor (tests/_grad_cases.py)
G_UP = 0.37              # upstream gradient of the backward tests
ROWS = ((-6.0, 6.0), (-20.0, 20.0))      # what log_a_q and log_b_q sweep
ROW_IDS = ["log_ab[-6,6]", "log_ab[-20,20]"]
NAMES = ("mu", "rho", "pm", "la", "lb", "a0", "b0")
UNIT = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def row(i):
    """The fixed fp32 inputs of row i, a dict of seven [N] CPU tensors: log_a / log_b sweep ROWS[i], rho sweeps [-8, 4], a0 / b0 sweep
    [0.1, 10] geometrically, all shuffled against each other; mu and the prior mean are 0.3 N(0, 1)."""
    lo, hi = ROWS[i]
    gen = lambda seed: torch.Generator().manual_seed(seed + 1000 * i)
    perm = lambda seed: torch.randperm(N, generator=gen(seed))
    hyp = torch.logspace(-1, 1, N)
    return dict(mu=0.3 * torch.randn(N, generator=gen(1)), rho=torch.linspace(-8, 4, N)[perm(2)].contiguous(), pm=0.3 * torch.randn(N, generator=gen(3)),
                la=torch.linspace(lo, hi, N)[perm(4)].contiguous(), lb=torch.linspace(lo, hi, N)[perm(5)].contiguous(),
                a0=hyp[perm(6)].contiguous(), b0=hyp[perm(7)].contiguous())


def addends(t, dtype=torch.float64):
    """[11, n]: the signed addends of A + B per element, evaluated in ``dtype`` from the tensors of t (any shape, flattened)."""
    mu, rho, pm, la, lb, a0, b0 = (t[k].detach().cpu().reshape(-1).to(dtype) for k in NAMES)
    a, b = torch.exp(la), torch.exp(lb)
    sig = torch.log1p(torch.exp(rho))
    r = a / b
    psi = torch.special.digamma(a)
    return torch.stack([0.5 * torch.log(b), -0.5 * psi, -0.5 * torch.log(sig * sig), 0.5 * r * sig * sig, 0.5 * r * (mu - pm) ** 2, torch.full_like(a, -0.5),
                        (a - a0) * psi, -torch.special.gammaln(a), torch.special.gammaln(a0), a0 * (torch.log(b) - torch.log(b0)), (b0 - b) * r])


def kl_elements(t):
    """-> (kl [n], U [n]) in float64: every element's A + B and its uncancelled size."""
    ad = addends(t)
    return ad.sum(0), ad.abs().sum(0)


def kl_fp32(t):
    """The formula in torch fp32 on the CPU, per element [n] (fp32): the yardstick's own evaluation.  Written as one would with torch
    ops: A and B as two expressions, added."""
    mu, rho, pm, la, lb, a0, b0 = (t[k].detach().cpu().reshape(-1).float() for k in NAMES)
    a, b = torch.exp(la), torch.exp(lb)
    s2 = torch.log1p(torch.exp(rho)) ** 2
    r = a / b
    psi = torch.digamma(a)
    A = 0.5 * (torch.log(b) - psi - torch.log(s2) + r * (s2 + (mu - pm) ** 2) - 1)
    B = (a - a0) * psi - torch.lgamma(a) + torch.lgamma(a0) + a0 * (torch.log(b) - torch.log(b0)) + (b0 - b) * r
    return A + B


def units(got, ref64, U):
    """|got - ref64| in units of 2^-23 (1 + U), float64 tensors (or floats)."""
    got = got.detach().double().cpu() if torch.is_tensor(got) else torch.tensor(float(got), dtype=torch.float64)
    return (got - ref64).abs() / (UNIT * (1.0 + U))


def worst(e):
    return math.nan if bool(torch.isnan(e).any()) else float(e.max())


@functools.lru_cache(maxsize=None)
def oracle(i):
    """Row i -> dict(kl [N], U [N], kl32 [N], elem_limit): the float64 values, the fp32 yardstick's values and KL_FACTOR times its
    worst per-element error.  Computed once."""
    t = row(i)
    kl, U = kl_elements(t)
    assert bool(torch.isfinite(kl).all()) and bool(torch.isfinite(U).all())
    kl32 = kl_fp32(t)
    e32 = worst(units(kl32, kl, U))
    return dict(kl=kl, U=U, kl32=kl32, ref32_err=e32, elem_limit=KL_FACTOR * e32)


def sum_limit(i, idx):
    """For the elements idx (a LongTensor, repeats allowed) of row i taken as one segment: (float64 sum, U of the sum, the limit in
    units: KL_FACTOR times the error of the fp32 yardstick's own sum, at least 1, and that fp32 error)."""
    o = oracle(i)
    ref, U = float(o["kl"][idx].sum()), float(o["U"][idx].sum())
    e32 = float(units(o["kl32"][idx].sum(), torch.tensor(ref, dtype=torch.float64), U))
    return ref, U, max(1.0, KL_FACTOR * e32), e32


# ------------------------------------------------------------------------------------------------------------------- gradients
GRADS = ("dmu", "drho", "dla", "dlb")


def grad_ref(t, dtype, g=G_UP):
    """(dmu, drho, dla, dlb) of g * SUM(A + B) by torch autograd in ``dtype`` (flattened)."""
    leaves = {k: t[k].detach().cpu().reshape(-1).to(dtype).clone().requires_grad_(k in ("mu", "rho", "la", "lb")) for k in NAMES}
    mu, rho, pm, la, lb, a0, b0 = (leaves[k] for k in NAMES)
    a, b = torch.exp(la), torch.exp(lb)
    s2 = torch.log1p(torch.exp(rho)) ** 2
    r = a / b
    psi = torch.special.digamma(a)
    A = 0.5 * (torch.log(b) - psi - torch.log(s2) + r * (s2 + (mu - pm) ** 2) - 1)
    B = (a - a0) * psi - torch.special.gammaln(a) + torch.special.gammaln(a0) + a0 * (torch.log(b) - torch.log(b0)) + (b0 - b) * r
    (g * (A + B).sum()).backward()
    return tuple(leaves[k].grad for k in ("mu", "rho", "la", "lb"))


def grad_scales(t, g=G_UP):
    """The uncancelled size of each gradient's closed form, float64 [n] each: sums of the absolute values of what the form adds.
      dmu = r (mu - m)                                   one product
      drho = (r sigma - 1/sigma) sigmoid(rho)            two terms
      dla = a [(a - a0 - 1/2) psi'(a) + (s/2 + b0)/b - 1]   three terms
      dlb = 1/2 + a0 - r (s/2 + b0)                      three terms"""
    mu, rho, pm, la, lb, a0, b0 = (t[k].detach().cpu().reshape(-1).double() for k in NAMES)
    a, b = torch.exp(la), torch.exp(lb)
    sig = torch.log1p(torch.exp(rho))
    r = a / b
    s = sig * sig + (mu - pm) ** 2
    q = r * (0.5 * s + b0)
    g = abs(g)
    return dict(dmu=g * r * (mu - pm).abs(), drho=g * (r * sig + 1.0 / sig) * torch.sigmoid(rho),
                dla=g * (a * (a - a0 - 0.5).abs() * torch.special.polygamma(1, a) + q + a), dlb=g * (0.5 + a0 + q))


def grad_errors(t, got, ref64, g=G_UP):
    """Worst per-element error of got = (dmu, drho, dla, dlb) against ref64 in units of 2^-23 of the gradient's uncancelled size ->
    dict.  Where that size is zero the gradient must be exactly zero.  A non-finite gradient gives nan or inf, which no limit admits."""
    sc = grad_scales(t, g)
    out = {}
    for k, gv, rv in zip(GRADS, got, ref64):
        e = (gv.detach().double().cpu().reshape(-1) - rv.reshape(-1)).abs()
        s = sc[k]
        out[k] = worst(torch.where(s > 0, e / (UNIT * s), torch.where(e == 0, torch.zeros_like(e), torch.full_like(e, math.inf))))
    return out


def grad_closed_fp32(t, g=G_UP):
    """The four closed forms of ``grad_scales`` evaluated with torch in fp32 on the CPU."""
    mu, rho, pm, la, lb, a0, b0 = (t[k].detach().cpu().reshape(-1).float() for k in NAMES)
    a, b = torch.exp(la), torch.exp(lb)
    sig = torch.log1p(torch.exp(rho))
    r = a / b
    s = sig * sig + (mu - pm) ** 2
    return (g * r * (mu - pm), g * (r * sig - 1 / sig) * torch.sigmoid(rho),
            g * a * ((a - a0 - 0.5) * torch.special.polygamma(1, a) + (0.5 * s + b0) / b - 1), g * (0.5 + a0 - a * (0.5 * s + b0) / b))


@functools.lru_cache(maxsize=None)
def grad_oracle(i):
    """Row i -> dict(ref64, ref32_err, limits): float64 autograd, the fp32 yardstick's worst errors and KL_FACTOR times them.  The
    yardstick is, per gradient, the better of the two fp32 evaluations a user could run on the CPU: torch's fp32 autograd of the formula
    and the closed forms in fp32 (autograd carries +a - a through log_b's gradient, which the closed form never forms: its error there is
    a hundred times the closed form's, and a limit taken from it would hold nothing)."""
    t = row(i)
    ref64 = grad_ref(t, torch.float64)
    assert all(bool(torch.isfinite(x).all()) for x in ref64)
    e_auto, e_closed = grad_errors(t, grad_ref(t, torch.float32), ref64), grad_errors(t, grad_closed_fp32(t), ref64)
    e32 = {k: min(e_auto[k], e_closed[k]) for k in GRADS}
    return dict(ref64=ref64, ref32_err=e32, ref32_autograd_err=e_auto, ref32_closed_err=e_closed, limits={k: KL_FACTOR * v for k, v in e32.items()})


# ------------------------------------------------------------------------------------------------------------------- segments
def segments():
    """70 (start, length) slices of a row read cyclically (index modulo N), in launch order: two launches of bt_kl_hier.  The lengths
    carry the edges of the forward kernel (256 threads; 1024 elements a pass; 4096 a block, so 4097 takes two blocks and 8193 three,
    each striding more than one pass) and of the backward kernel (1024 a block); the rest are small and odd."""
    edge = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193]
    small = [5 + (37 * i) % 97 for i in range(54)]
    lens = edge[:8] + small[:27] + edge[8:] + small[27:]
    segs, lo = [], 0
    for n in lens:
        segs.append((lo % N, n))
        lo += n + 13
    assert len(segs) == 70
    return segs


def seg_index(s, n):
    return (torch.arange(n) + s) % N


def packed_views(t, segs, device):
    """The slices ``segs`` of the 1-d CPU tensor t as views into ONE buffer on ``device``.  Even-numbered segments start 16-byte
    aligned (the kernel's float4 path, with its scalar tail), odd-numbered ones at an odd element offset (the scalar path)."""
    total = sum(n for _, n in segs) + 8 * len(segs) + 8
    buf = torch.full((total,), float("nan"), dtype=torch.float32, device=device)
    assert buf.data_ptr() % 16 == 0
    views, off = [], 0
    for j, (s, n) in enumerate(segs):
        off = (off + 3) // 4 * 4 + (j % 2)
        buf[off:off + n] = t[seg_index(s, n)].to(device)
        views.append(buf[off:off + n])
        off += n + 1
    return views


# ------------------------------------------------------------------------------------------------------------------- fixtures
FIXTURES = ("hier_lin_bias", "hier_lin_nobias", "hier_conv")      # tests/golden, written by tools/make_goldens_hier.py


def normal_kl_mean64(mu, rho, pm, ps):
    mu, rho, pm, ps = (t.double() for t in (mu, rho, pm, ps))
    sq = torch.log1p(torch.exp(rho))
    return float((torch.log(ps) - torch.log(sq) + (sq * sq + (mu - pm) ** 2) / (2 * ps * ps) - 0.5).mean())


def fixture_tensors(g):
    """A fixture's weight segment in the oracle's names."""
    w = "weight" if "mu_weight" in g else "kernel"
    return dict(mu=g["mu_" + w], rho=g["rho_" + w], pm=g["prior_weight_mu"], la=g["log_a_q_" + w], lb=g["log_b_q_" + w], a0=g["a0"], b0=g["b0"])


def fixture_oracle(g):
    """-> (kl_loss in float64, its U, forward KL in float64): the weights' sum, plus the bias's Gaussian mean KL where there is one."""
    kl, U = kl_elements(fixture_tensors(g))
    kl_loss, Us = float(kl.sum()), float(U.sum())
    fwd = kl_loss + (normal_kl_mean64(g["mu_bias"], g["rho_bias"], g["prior_bias_mu"], g["prior_bias_sigma"]) if "mu_bias" in g else 0.0)
    return kl_loss, Us, fwd
