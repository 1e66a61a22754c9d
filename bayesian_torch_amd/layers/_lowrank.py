"""The engine behind ``Conv2dReparameterization_Multivariate`` (reference layers/variational_layers/conv_variational.py:409-648): a
Conv2d whose posterior is a low-rank multivariate normal over all n = Co * Ci * k * k weights,

    w_s = mu + L z_s + sqrt(d) o eps_s,      z_s ~ N(0, I_r),  eps_s ~ N(0, I_n),  d = 1e-10,

against a prior N(m, diag(P)) (what the constructor sets and ``Multivariate_MOPED`` installs).

Three paths (``choose_path``; ``layer._last["path"]``):

``"in_kernel"``     rank <= 4: the fp32 fused forward forms w_s in the producers' registers (bt_lowrank_conv2d_fwd); nothing
                    weight-sized is written.
``"mean_prepass"``  rank > 4: bt_lowrank_mean writes m_s = mu + L z_s ([S, n] floats, into the layer's workspace) and the same forward
                    kernel runs with rank 0 on it.
``"materialised"``  a call that needs gradients (unless ``set_lowrank_train_path("fused")``), or a ``D_param`` that is not one constant:
                    plain torch ops on the device, w = mu + z @ L^T + sqrt(D) * eps and F.conv2d per sample, with the draws the kernels
                    would have made.

Training (``set_lowrank_train_path``, environment default ``BT_LOWRANK_TRAIN_PATH``): under ``"materialised"`` (the default) a call that
needs gradients takes the torch composition and autograd differentiates it. Under ``"fused"`` it keeps its inference path and the HIP
backward of csrc/bt_lowrank_bwd.hip differentiates it (autograd.LowRankForward: the data gradient regenerates the sampled weights on
chip, the weight gradient stays per sample, one finishing launch gives dmu and dL); the KL of a diagonal prior is autograd.KLLowRank
(bt_kl_lowrank / bt_kl_lowrank_bwd). ``layer._last["backward"]`` says which: ``"fused"`` or ``"autograd"`` (None: no gradients asked for).

The KL of a diagonal prior comes from bt_kl_lowrank (an fp64 sweep and an r x r fp64 Cholesky; once per forward, whatever S); a prior
with a non-zero ``prior_cov_L``, or a call that needs gradients, takes it from torch ops in fp64 (``closed_form_kl``, or
torch.distributions for the general prior) -- the only factorisations there are r x r as well.

Deviations from the reference, all documented in DESIGN.md section 4.6d: ``kl_loss()`` works without a prior forward (the reference raises
AttributeError), ``groups != 1`` and a tuple ``kernel_size`` are refused at construction (the reference fails in ``view``), and
``martern_prior = True`` raises NotImplementedError (the reference's branch fails its own assert).
"""
import os

import torch
import torch.nn.functional as TF
from torch.nn import Parameter

from .. import _lib, autograd, mc, rng
from .. import functional as F
from ._fused import FusedBayesLayer
from .base_variational_layer import BaseVariationalLayer_

MAX_R = _lib.LOWRANK_MAX_R
D_INIT = 1e-10


TRAIN_PATHS = ("fused", "materialised")


def _check_train_path(name, what):
    if name not in TRAIN_PATHS:
        raise ValueError(f"{what}: expected one of {TRAIN_PATHS}, got {name!r}")
    return name


_train_path = [_check_train_path(os.environ.get("BT_LOWRANK_TRAIN_PATH", "materialised"), "BT_LOWRANK_TRAIN_PATH")]


def set_lowrank_train_path(name):
    """How a call of the low-rank multivariate layer that needs gradients runs: "materialised" (default) the torch composition under
    autograd, "fused" the inference launches with the HIP backward (module docstring). Process-wide; also the environment variable
    BT_LOWRANK_TRAIN_PATH, read at import. Returns the previous setting."""
    prev, _train_path[0] = _train_path[0], _check_train_path(name, "set_lowrank_train_path")
    return prev


def get_lowrank_train_path():
    return _train_path[0]


def choose_path(rank, d_uniform, prior_diagonal, needs_grad, train_path="materialised"):
    """-> (forward path, KL path, reason for leaving the kernels or None). A pure function of what the layer knows before it launches.
    train_path "fused": a call that needs gradients keeps the kernels' paths (a non-diagonal prior keeps the differentiable torch KL)."""
    if needs_grad and train_path != "fused":
        return "materialised", "materialised", "the call needs gradients"
    if not d_uniform:
        return "materialised", "materialised", "D_param is not one constant"
    fwd = "in_kernel" if rank <= MAX_R else "mean_prepass"
    if not prior_diagonal:
        return fwd, "materialised", "prior_cov_L is not zero"
    return fwd, "kernel", None


def _cholesky(A):
    """Lower Cholesky factor of a small fp64 matrix: on A's device, or on the host where the build has no device factorisation."""
    try:
        return torch.linalg.cholesky(A)
    except RuntimeError:
        return torch.linalg.cholesky(A.cpu()).to(A.device)


def closed_form_kl(mu, L, D, prior_mean, prior_var):
    """KL( N(mu, L L^T + diag(D)) || N(prior_mean, diag(prior_var)) ), un-normalised, in fp64 torch ops on the tensors' device:

        1/2 [ sum log P - sum log D - logdet(I_r + L^T diag(1/D) L) + sum (D + sum_j L_ij^2) / P + sum (mu - m)^2 / P - n ]

    D: a tensor [n] or a scalar. The only factorisation is the r x r one; differentiable in mu and L. -> 0-dim fp64 tensor."""
    mu, L = mu.double().reshape(-1), L.double()
    n, r = L.shape
    D = torch.as_tensor(D, dtype=torch.float64, device=mu.device).expand(n)
    m, P = prior_mean.double().reshape(-1), prior_var.double().reshape(-1)
    G = torch.eye(r, dtype=torch.float64, device=mu.device) + L.t() @ (L / D[:, None])
    logdet = 2.0 * torch.log(torch.diagonal(_cholesky(G))).sum()
    return 0.5 * (torch.log(P).sum() - torch.log(D).sum() - logdet + ((D + (L * L).sum(1)) / P).sum() + ((mu - m) ** 2 / P).sum() - n)


def general_kl(mu, L, D, prior_mean, prior_L, prior_D):
    """The same divergence against a low-rank prior N(m, prior_L prior_L^T + diag(prior_D)), by torch.distributions in fp64 (its
    factorisations are of the two capacitance matrices, r x r and 1 x 1 here: no n x n matrix is formed) -> 0-dim fp64 tensor."""
    from torch.distributions import LowRankMultivariateNormal, kl_divergence

    def run(dev):
        t = lambda v: v.double().to(dev)
        q = LowRankMultivariateNormal(t(mu).reshape(-1), t(L), t(D).reshape(-1))
        p = LowRankMultivariateNormal(t(prior_mean).reshape(-1), t(prior_L), t(prior_D).reshape(-1))
        return kl_divergence(q, p)

    try:
        return run(mu.device)
    except RuntimeError:
        if not mu.is_cuda:
            raise
        return run(torch.device("cpu")).to(mu.device)


class LowRankConv2dLayer(BaseVariationalLayer_):
    _kl_muted = False
    _rng_layer = True      # rng.assign_layer_ids numbers it with the other Bayesian layers
    _mc_frame = FusedBayesLayer._mc_frame
    _call_coords = FusedBayesLayer._call_coords
    _take_injected = FusedBayesLayer._take_injected

    def _build(self, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, rank, bias):
        if in_channels % groups != 0:
            raise ValueError('invalid in_channels size')
        if out_channels % groups != 0:
            raise ValueError('invalid in_channels size')      # sic: same message as the reference
        if groups != 1:
            raise ValueError(f"{type(self).__name__}: groups must be 1 (the reference views its weight as (Co, Ci, k, k) and fails for any other), got {groups}")
        if isinstance(kernel_size, bool) or not isinstance(kernel_size, int):
            raise ValueError(f"{type(self).__name__}: kernel_size must be an int (the reference views its weight as (Co, Ci, k, k)), got {kernel_size!r}")
        if isinstance(rank, bool) or not isinstance(rank, int) or rank < 1:
            raise ValueError(f"{type(self).__name__}: rank must be an int >= 1, got {rank!r}")
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.stride, self.padding, self.dilation, self.groups = stride, padding, dilation, groups
        self.bias = bias           # accepted and ignored, as in the reference: the layer has no bias parameters
        n = out_channels * in_channels * kernel_size * kernel_size
        self.weight_size = n
        self.mu_kernel = Parameter(torch.empty(n))
        self.L_param = Parameter(torch.empty(n, rank))
        self.D_param = torch.ones(n) * D_INIT      # a plain attribute, as in the reference: neither a parameter nor a buffer
        self.register_buffer("prior_mean", torch.empty(n), persistent=True)
        self.register_buffer("prior_cov_L", torch.empty(n, 1), persistent=True)
        self.register_buffer("prior_cov_D", torch.empty(n), persistent=True)
        self.init_parameters(n)
        self.martern_prior = False
        self.BLOCK_MAT = self.covariance_matrix_by_filter((kernel_size, kernel_size), sigma=1.0, lamb=1.0)
        self.rank = rank
        self._layer_id = rng.new_layer_id()
        self._last = None
        self._checks = None        # (key, d_uniform, d, prior_diagonal): one look at D_param / prior_cov_L per tensor version
        self._bad_pivots = None    # int32 device word: forwards whose KL factorisation met a pivot that was not positive
        self.inject_draw = None    # test hook: dict(z [S, rank], eps_w [S, n]) consumed instead of a fresh draw (or a list of them)
        self.force_path = None     # "materialised": every call takes the torch composition (the benchmark's baseline)

    def init_parameters(self, weight_size):
        self.prior_mean.data.copy_(torch.zeros(weight_size))          # prior N(0, I)
        self.prior_cov_L.data.copy_(torch.zeros((weight_size, 1)))
        self.prior_cov_D.data.copy_(torch.ones(weight_size))
        self.mu_kernel.data.normal_(mean=0, std=0.1)
        self.L_param.data.normal_(mean=0, std=0.1)

    def covariance_matrix_by_filter(self, filter_size, sigma=1.0, lamb=1.0):
        """The Matern-1/2 covariance of the filter's coordinates, [k*k, k*k] (the reference's BLOCK_MAT attribute; nothing here reads it)."""
        coords = torch.tensor([(float(i), float(j)) for i in range(filter_size[0]) for j in range(filter_size[1])])
        dist = torch.norm(coords.unsqueeze(1) - coords.unsqueeze(0), dim=2)
        return (sigma ** 2) * torch.exp(-dist / lamb)

    def get_covariance_param(self):
        return self.L_param, self.D_param

    def prepare(self):
        raise NotImplementedError("post-training quantisation (QuantStub observers) is outside the MI355X hot path")

    @property
    def _ws_id(self):
        return id(self)

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_checks"] = None
        return d

    # ------------------------------------------------------------------ what the tensors are
    def _wshape(self):
        return (self.out_channels, self.in_channels, self.kernel_size, self.kernel_size)

    def _conv_desc(self):
        two = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        if isinstance(self.padding, str):
            raise NotImplementedError("string padding modes are not supported")
        return dict(stride=two(self.stride), padding=two(self.padding), dilation=two(self.dilation), groups=1)

    def invalidate_checks(self):
        """Look at ``D_param`` / ``prior_cov_L`` again at the next call (writes through ``.data`` do not move a tensor's version)."""
        self._checks = None

    def _look(self, dev):
        """-> (D_param is one constant, that constant, prior_cov_L is zero, D_param on ``dev``). Looked at once per tensor version (it
        synchronises), and never inside a graph capture: a captured step runs its warm-up first."""
        D, pL = self.D_param, self.prior_cov_L
        key = (id(D), D._version, id(pL), pL._version, pL.device, dev)
        if self._checks is None or self._checks[0] != key:
            if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{type(self).__name__}: D_param / prior_cov_L changed since the last eager call; run one forward outside the capture")
            Dd = D.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
            lo, hi = float(Dd.min()), float(Dd.max())
            self._checks = (key, lo == hi and lo > 0.0, lo, not bool((pL != 0).any()), Dd)
        return self._checks[1:]

    # ------------------------------------------------------------------ KL
    def _kl(self, path, needs_grad):
        """(KL, KL / n) of the parameters as they are -> fp32 0-dim tensors."""
        mu, L = self.mu_kernel, self.L_param
        d_uniform, d, prior_diag, Dd = self._look(mu.device)
        if path == "kernel":
            if self._bad_pivots is None or self._bad_pivots.device != mu.device:
                self._bad_pivots = torch.zeros(1, dtype=torch.int32, device=mu.device)
            if needs_grad:      # the fused training path: the kernels' KL, differentiated by bt_kl_lowrank_bwd
                return autograd.KLLowRank.apply(mu, L, dict(d=d, prior_mean=self.prior_mean, prior_var=self.prior_cov_D, owner=("layer", self._ws_id),
                                                            bad_pivots=self._bad_pivots))
            out = F.kl_lowrank(mu.detach(), L.detach(), d, self.prior_mean, self.prior_cov_D, owner=("layer", self._ws_id), bad_pivots=self._bad_pivots)
            return out[0], out[1]
        if not needs_grad:
            mu, L = mu.detach(), L.detach()
        with torch.set_grad_enabled(needs_grad):
            if prior_diag:
                kl = closed_form_kl(mu, L, Dd, self.prior_mean, self.prior_cov_D)
            else:
                kl = general_kl(mu, L, Dd, self.prior_mean, self.prior_cov_L, self.prior_cov_D)
            return kl.float(), (kl / self.weight_size).float()

    def bad_pivots(self):
        """How many KL launches of this layer met a pivot that was not positive (their KL is NaN); synchronises."""
        return 0 if self._bad_pivots is None else int(self._bad_pivots.item())

    def _needs_grad(self, x=None):
        return torch.is_grad_enabled() and ((x is not None and x.requires_grad) or self.mu_kernel.requires_grad or self.L_param.requires_grad)

    def kl_loss(self):
        """The un-normalised KL of the layer's parameters. Unlike the reference's (which reads the distributions its last forward
        cached and raises AttributeError before one), it needs no forward."""
        if self.martern_prior:
            raise NotImplementedError(_MARTERN)
        mu = _lib.dev_f32(self.mu_kernel, "mu_kernel")
        needs_grad = self._needs_grad()
        d_uniform, _, prior_diag, _ = self._look(mu.device)
        _, kl_path, _ = choose_path(self.rank, d_uniform, prior_diag, needs_grad, train_path=get_lowrank_train_path())
        return self._kl(kl_path, needs_grad)[0]

    # ------------------------------------------------------------------ forward
    def _draws(self, S, coords, dev, inj, fused):
        """-> (z [S, r], eps_w [S, n]) as tensors, or (None, None) when the kernels draw on chip."""
        n, r = self.weight_size, self.rank
        if inj is not None:
            z, eps = inj["z"], inj["eps_w"]
            if z.shape[0] != S or eps.shape[0] != S:
                raise RuntimeError(f"inject_draw holds {z.shape[0]} / {eps.shape[0]} samples, this call computes {S}")
            return _lib.dev_f32(z.reshape(S, r), "z"), _lib.dev_f32(eps.reshape(S, n), "eps_w")
        if rng.get_mode() == "torch":      # z, then eps, per sample: the reference's draw order (rsample)
            z, eps = torch.empty((S, r), device=dev), torch.empty((S, n), device=dev)
            for s in range(S):
                z[s].normal_()
                eps[s].normal_()
            return z, eps
        if fused:
            return None, None
        return self._fill(coords, S, dev)

    def _fill(self, coords, S, dev):
        seed, call_base, call, lid, sample0 = coords
        z = F.rng_fill_normal(seed, call, lid, sample0, 4, S, (self.rank,), dev, call_base=call_base)
        eps = F.rng_fill_normal(seed, call, lid, sample0, 0, S, self._wshape(), dev, call_base=call_base)
        return z, eps.reshape(S, self.weight_size)

    def _mean_workspace(self, S, dev):
        """[S, n] floats behind the head of this layer's workspace (made, and grown, outside any capture: a captured step warms up)."""
        n = self.weight_size
        ws = _lib.workspace((("layer", self._ws_id), "lowrank_mean"), dev, 4 * S * n)
        return ws[_lib.WORKSPACE_BYTES:_lib.WORKSPACE_BYTES + 4 * S * n].view(torch.float32).view(S, n)

    def _forward(self, x, return_kl=True):
        if self.martern_prior:
            raise NotImplementedError(_MARTERN)
        ctx, collect, want_kl, return_kl = self._mc_frame(return_kl)
        x = _lib.dev_f32(x, "input")
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise RuntimeError(f"{type(self).__name__}: expected [N, {self.in_channels}, H, W], got {tuple(x.shape)}")
        if x.shape[0] == 0:
            raise RuntimeError("empty batch")
        mu, L = _lib.dev_f32(self.mu_kernel, "mu_kernel"), _lib.dev_f32(self.L_param, "L_param")
        dev = x.device
        conv = self._conv_desc()
        S, shared, coords = self._call_coords(ctx, x.shape[0])
        B = x.shape[0] // (1 if shared else S)
        needs_grad = self._needs_grad(x)
        d_uniform, d, prior_diag, Dd = self._look(dev)
        path, kl_path, reason = choose_path(self.rank, d_uniform, prior_diag, needs_grad, train_path=get_lowrank_train_path())
        if self.force_path == "materialised" and path != "materialised":
            path, kl_path, reason = "materialised", "materialised", "forced"
        z, eps = self._draws(S, coords, dev, self._take_injected(), path != "materialised")
        kw = dict(S=S, shared_x=shared, seed=coords.seed, call=coords.call, layer_id=coords.layer_id, sample0=coords.sample0, call_base=coords.call_base)
        if path == "materialised":
            Ld = L if needs_grad else L.detach()
            md = mu if needs_grad else mu.detach()
            with torch.set_grad_enabled(needs_grad):
                w = md + z @ Ld.t() + torch.sqrt(Dd) * eps                 # [S, n]: the only weight-sized tensor, never n x n
                xs = x.reshape((1 if shared else S, B) + tuple(x.shape[1:]))
                outs = [TF.conv2d(xs[0 if shared else s], w[s].view(self._wshape()), None, conv["stride"], conv["padding"], conv["dilation"], 1) for s in range(S)]
                out = outs[0] if S == 1 else torch.cat(outs, 0)
            kernel, launch = "torch: mu + z @ L^T + sqrt(D) * eps, conv2d", None
        elif needs_grad:      # the fused training path: the same launches, differentiated by the HIP backward
            bwd_rec = {}
            out = autograd.LowRankForward.apply(x, mu, L, dict(kw, d=d, wshape=self._wshape(), conv=conv, path=path, z=z, eps_w=eps, record=bwd_rec,
                                                               mean_out=self._mean_workspace(S, dev) if path == "mean_prepass" else None))
            kernel, launch = _lib.lib().bt_last_kernel_name().decode(), _lib.last_launch_info()
        else:
            if path == "in_kernel":
                out = F.lowrank_conv2d(x, mu.detach(), L.detach(), d, self._wshape(), conv, z=z, eps_w=eps, **kw)
            else:
                m = F.lowrank_mean(mu.detach(), L.detach(), S, z, seed=coords.seed, call=coords.call, layer_id=coords.layer_id, sample0=coords.sample0,
                                   call_base=coords.call_base, out=self._mean_workspace(S, dev))
                out = F.lowrank_conv2d(x, m, None, d, self._wshape(), conv, eps_w=eps, **kw)
            kernel, launch = _lib.lib().bt_last_kernel_name().decode(), _lib.last_launch_info()
        kl = self._kl(kl_path, needs_grad)[1] if want_kl else None      # once per forward, whatever S: the value does not depend on the sample
        fused_bwd = needs_grad and path != "materialised"
        self._last = dict(draw=None if z is None else dict(z=z, eps_w=eps), rng=coords, S=S, kernel=kernel, launch=launch, shared_x=shared, path=path,
                          kl_path=kl_path if want_kl else None, reason=reason, x_shape=(B,) + tuple(x.shape[1:]), out_shape=(B,) + tuple(out.shape[1:]),
                          backward=("fused" if fused_bwd else "autograd") if needs_grad else None, backward_launch=bwd_rec if fused_bwd else None)
        if collect:
            ctx.kls.append(kl)
        return (out, kl) if return_kl else out

    def materialize_last_draw(self):
        """The draw the last forward used: ``z`` [S, rank] and ``eps_w`` [S, n] -- the tensors that were read, or, after an on-chip
        draw, the streams regenerated from the call's coordinates (bt_rng_normal_fill, tensors 4 and 0)."""
        if self._last is None:
            raise RuntimeError("no forward has run yet")
        st = self._last
        if st["draw"] is not None:
            return dict(st["draw"])
        if st["rng"].call_base is not None:
            raise RuntimeError("draws made under a graph call_base cannot be replayed after the word advanced")
        z, eps = self._fill(st["rng"], st["S"], self.mu_kernel.device)
        return dict(z=z, eps_w=eps)


_MARTERN = ("the Matern prior is not implemented: the reference's martern_prior branch (conv_variational.py:530-538) hands martern_cov_kl_loss "
            "a vector d, gets a vector back and fails its own `assert not torch.isnan(kl_weight)`; it cannot run as written")
