"""Inputs and float64 references shared by test_grad_oracle_host.py (CPU) and test_gpu_grad_oracle.py (GPU).  A plain module:
no fixtures, no pytest hooks.  Every reference here is torch autograd of oracle/bt_oracle.py -- never the closed forms of
csrc/bt_bwd.hip or autograd._kl_grads_aten, which are what the tests hold to it."""
import functools
import math

import torch

from conftest import load_golden
from oracle import bt_oracle as O

# --------------------------------------------------------------------------------------------------------- A. KL gradient alone
KL_N = 4001
KL_G = 0.37          # upstream gradient of the KL term
# The kernels may be this many times worse than the oracle's own fp32 autograd (CPU libm): they chain the hardware's exp2, log and
# rcp, about 1 ulp each and up to about six per element.
KL_FACTOR = 8.0
KL_ROWS = (("normal", -30.0, 30.0), ("normal", -80.0, 80.0), ("laplace", -20.0, 30.0), ("laplace", -20.0, 80.0))
KL_ROW_IDS = [f"{k}[{int(lo)},{int(hi)}]" for k, lo, hi in KL_ROWS]


@functools.lru_cache(maxsize=None)
def kl_inputs(lo, hi):
    """The fixed fp32 inputs of one row: rho sweeps [lo, hi], mu and the per-element prior sigma are spread and shuffled against it."""
    n = KL_N
    perm = lambda seed: torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    return dict(mu=torch.linspace(-2, 2, n)[perm(101)].contiguous(), rho=torch.linspace(lo, hi, n), pmu=torch.full((n,), 0.3),
                psig=torch.linspace(0.05, 3, n)[perm(202)].contiguous())


def kl_grad_ref(kind, mu, rho, pmu, psig, dtype, g=KL_G):
    """(dmu, drho) of g * (the oracle's KL mean over this tensor), by torch autograd in ``dtype``."""
    m, r = mu.detach().to(dtype).clone().requires_grad_(True), rho.detach().to(dtype).clone().requires_grad_(True)
    if kind == "laplace":
        kl = O.kl_laplace_ref(m, O.softplus_ref(r))
    else:
        kl = O.kl_normal_ref(m, O.softplus_ref(r), pmu.detach().to(dtype), psig.detach().to(dtype))
    (g * kl).backward()
    return m.grad, r.grad


def kl_errors(kind, mu, rho, psig, got, ref64, g=KL_G):
    """Worst per-element scaled error of got = (dmu, drho) against ref64, all in float64 -> dict(dmu=, drho=).
    drho is measured against the UNCANCELLED size of the expression, (|t1| + |t2|) * sigmoid(rho) * g / n -- t1 - t2 crosses zero --
    with t2 = 1/sigma and t1 = sigma/sigma_p^2 (normal) or sqrt(2/pi) exp(-mu^2 / 2 sigma^2) (Laplace).  dmu: relative to |ref64|
    for the normal prior (an exact zero must be met exactly), in units of g / n for the Laplace prior (its 1 - 2 Phi form is only
    absolutely accurate at small mu / sigma).  A non-finite gradient gives nan or inf, which no limit admits."""
    mu, rho, psig = mu.detach().double().cpu(), rho.detach().double().cpu(), psig.detach().double().cpu()
    gs = g / mu.numel()
    sig = O.softplus_ref(rho)
    t1 = math.sqrt(2.0 / math.pi) * torch.exp(-mu * mu / (2 * sig * sig)) if kind == "laplace" else sig / (psig * psig)
    scale = (t1.abs() + 1.0 / sig) * torch.sigmoid(rho) * gs
    e_mu = (got[0].detach().double().cpu().reshape(-1) - ref64[0].reshape(-1)).abs()
    e_rho = (got[1].detach().double().cpu().reshape(-1) - ref64[1].reshape(-1)).abs() / scale
    if kind == "laplace":
        e_mu = e_mu / gs
    else:
        a = ref64[0].reshape(-1).abs()
        e_mu = torch.where(a > 0, e_mu / a, torch.where(e_mu == 0, torch.zeros_like(e_mu), torch.full_like(e_mu, math.inf)))
    worst = lambda e: math.nan if bool(torch.isnan(e).any()) else float(e.max())
    return dict(dmu=worst(e_mu), drho=worst(e_rho))


@functools.lru_cache(maxsize=None)
def kl_row(i):
    """Row i of KL_ROWS -> dict(kind, inputs, ref64, ref32, ref32_err): the float64 reference gradients of the whole 4001-element
    tensor, the oracle's own fp32 autograd on the same inputs, and that fp32 reference's worst scaled errors.  Computed once."""
    kind, lo, hi = KL_ROWS[i]
    t = kl_inputs(lo, hi)
    ref64 = kl_grad_ref(kind, t["mu"], t["rho"], t["pmu"], t["psig"], torch.float64)
    ref32 = kl_grad_ref(kind, t["mu"], t["rho"], t["pmu"], t["psig"], torch.float32)
    return dict(kind=kind, inputs=t, ref64=ref64, ref32=ref32, ref32_err=kl_errors(kind, t["mu"], t["rho"], t["psig"], ref32, ref64))


def kl_limits(i):
    """What a kernel may reach on row i: KL_FACTOR times the fp32 reference's own worst value of the same measure."""
    return {k: KL_FACTOR * v for k, v in kl_row(i)["ref32_err"].items()}


def kl_slice_ref(i, lo, n, g=KL_G):
    """float64 reference of elements [lo, lo + n) of row i taken as a tensor of their own: the mean is over these n elements."""
    r = kl_row(i)
    t = {k: v[lo:lo + n] for k, v in r["inputs"].items()}
    return t, kl_grad_ref(r["kind"], t["mu"], t["rho"], t["pmu"], t["psig"], torch.float64, g)


KL_FUSED_N = 24 * 16 * 3 * 3      # the [24, 16, 3, 3] weights of the fused-backward rows: the first 3456 elements of a row


def kl_segments():
    """70 (start, length) slices of a row's 4001 elements, in launch order.  61 of them tile the row; the other nine carry the block
    edges of the segmented kernel (1024 elements per block: 1023 / 1024 / 1025, and 255 / 256 / 257 around its 256 threads), 1, 2,
    and the first 3456 elements -- the fused rows' tensor -- as the one of several blocks.  They overlap the tiling: the lengths
    alone exceed 4001.  Segments 64..69 go to a second launch and hold a two-block segment too."""
    tile, lo = [], 0
    for i in range(60):
        tile.append((lo, 5 + (37 * i) % 97))
        lo += tile[-1][1]
    tile.append((lo, KL_N - lo))
    edge = {1: 4000, 2: 17, 255: 100, 256: KL_N - 256, 257: 1000, 1023: KL_N - 1023, 1024: 0, 1025: 1500, KL_FUSED_N: 0}
    e = lambda n: (edge[n], n)
    segs = [e(1024), e(1), e(1023)] + tile[:30] + [e(255), e(256), e(KL_FUSED_N)] + tile[30:] + [e(2), e(1025), e(257)]
    assert len(segs) == 70 and tile[-1][1] > 0 and all(0 <= s and s + n <= KL_N and n > 0 for s, n in segs)
    return segs


def odd_offset_views(t, segs):
    """Copies of the slices ``segs`` of the 1-d tensor t as views into ONE larger buffer on t's device, each starting at an odd
    element offset (a 4-byte-aligned address that is not 8-byte aligned)."""
    buf = torch.full((sum(n for _, n in segs) + 2 * len(segs) + 1,), float("nan"), dtype=t.dtype, device=t.device)
    views, off = [], 1
    for s, n in segs:
        buf[off:off + n] = t[s:s + n]
        views.append(buf[off:off + n])
        off += n + 1
        off += 1 - off % 2
    return views


# --------------------------------------------------------------------------------------------------------- B. supplied draws
# (id, layer class, constructor keywords, x shape of one sample batch, S) -- the smallest rows that reach the splitting logic of
# wgrad_groups / dgrad_chunks named beside them.
DRAW_ROWS = [
    ("A", "Conv2dReparameterization", dict(in_channels=64, out_channels=72, kernel_size=3, padding=1), (5, 64, 7, 7), 2),      # 2 reduction chunks (128 + 117 rows of M = 245); dgrad pieces 32 / 32 / 8
    ("B", "Conv2dReparameterization", dict(in_channels=12, out_channels=20, kernel_size=(3, 2), stride=(2, 1), padding=(1, 0), dilation=(1, 2), groups=2),
     (3, 12, 9, 8), 2),                                                                                                      # groups; Cig = 6, padded to 8
    ("C", "Conv2dFlipout", dict(in_channels=16, out_channels=24, kernel_size=3, stride=2, padding=1, groups=2), (4, 16, 7, 7), 2),    # supplied signs, strided dgrad taps
    ("D", "LinearReparameterization", dict(in_features=4096, out_features=130), (6, 4096), 3),      # sgroups = 2 < S = 3; 64 k-tiles; pieces 48 / 48 / 34
    ("E", "LinearFlipout", dict(in_features=130, out_features=70, bias=False), (9, 130), 2),         # Cig4 = 132; pieces 32 / 32 / 6
    ("F", "Conv2dReparameterization", dict(in_channels=3, out_channels=16, kernel_size=7, stride=2, padding=3), (2, 3, 16, 16), 1),   # stem, Cig = 3
    ("G", "Conv2dFlipout", dict(in_channels=70, out_channels=136, kernel_size=3, padding=1), (3, 70, 5, 5), 3),                # Cig4 = 72; 5 pieces; three channel tiles
]
DRAW_ROW = {r[0]: r for r in DRAW_ROWS}


def oracle_grads(flip, params, x, draws, conv, gout, S, shared, dtype=torch.float64):
    """out, dL/dx and the parameter gradients of L = (out * gout).sum() by torch autograd of the oracle's forward on ``draws``, in
    ``dtype`` on the CPU.  params: dict(mu_w, rho_w, mu_b, rho_b) (biases may be None); x: [B, ...] shared by the S samples or
    [S*B, ...] stacked sample-major; draws: materialize_last_draw()'s dict."""
    cv = lambda t: None if t is None else t.detach().cpu().to(dtype)
    p = {k: (None if v is None else cv(v).clone().requires_grad_(True)) for k, v in params.items()}
    xc = cv(x).clone().requires_grad_(True)
    d = {k: cv(v) for k, v in draws.items()}
    B = xc.shape[0] // (1 if shared else S)
    outs = []
    for s in range(S):
        xs = xc if shared else xc[s * B:(s + 1) * B]
        eb = d["eps_b"][s] if d.get("eps_b") is not None else None
        if flip:
            outs.append(O.flipout_fwd_ref(xs, p["mu_w"], p["rho_w"], d["eps_w"][s], d["sign_in"][s], d["sign_out"][s], p["mu_b"], p["rho_b"], eb, conv))
        else:
            outs.append(O.reparam_fwd_ref(xs, p["mu_w"], p["rho_w"], d["eps_w"][s], p["mu_b"], p["rho_b"], eb, conv))
    out = torch.cat(outs)
    (out * cv(gout)).sum().backward()
    return out.detach(), xc.grad, {k: (None if v is None else v.grad) for k, v in p.items()}


# --------------------------------------------------------------------------------------------------------- C. LSTM through time
LSTM_PARAMS = ("mu_w", "rho_w", "mu_b", "rho_b")


def lstm_inject_lists(g, nm, device):
    """The per-step ``inject_draw`` list of the cell's map ``nm`` ("ih" / "hh"), as the golden tests of the two LSTM layers build it."""
    T = g["meta"]["x_shape"][1]
    keys = [k for k in ("eps_w", "eps_b", "sign_in", "sign_out") if f"{nm}_{k}" in g]
    return [{k: g[f"{nm}_{k}"][t:t + 1].to(device) for k in keys} for t in range(T)]


def lstm_ref_run(name, dtype):
    """O.lstm_ref on the golden ``name`` in ``dtype``, step t of each map on step t's stored draws.
    -> (hidden_seq, c_ts, x leaf, {"ih_mu_w": leaf, ...}); the leaves require grad."""
    g = load_golden(name)
    flip = "flipout" in name
    leaf = lambda t: t.to(dtype).clone().requires_grad_(True)
    x = leaf(g["x"])
    p = {f"{nm}_{k}": leaf(g[f"{nm}_{k}"]) for nm in ("ih", "hh") for k in LSTM_PARAMS}

    def step(nm):
        def f(t, v):
            v = v.to(dtype)      # (lstm_ref starts from float32 zeros)
            a = (p[nm + "_mu_w"], p[nm + "_rho_w"], g[nm + "_eps_w"][t].to(dtype))
            b = (p[nm + "_mu_b"], p[nm + "_rho_b"], g[nm + "_eps_b"][t].to(dtype))
            if flip:
                return O.flipout_fwd_ref(v, *a, g[nm + "_sign_in"][t].to(dtype), g[nm + "_sign_out"][t].to(dtype), *b)
            return O.reparam_fwd_ref(v, *a, *b)
        return f
    hs, cs = O.lstm_ref(x, step("ih"), step("hh"), g["meta"]["out_features"])
    return hs, cs, x, p


def lstm_upstream(shape):
    gen = torch.Generator().manual_seed(17)
    return torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
