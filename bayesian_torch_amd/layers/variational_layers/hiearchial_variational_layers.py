"""The hierarchical layers -- drop-in for reference ``layers/variational_layers/hiearchial_variational_layers.py`` (the file name's
spelling is the reference's: it is the import path; the module is not star-imported into ``layers``, there or here).

``LinearReparameterizationHierarchical_Weightwise`` (reference :293-430) and ``Conv2dReparameterizationHierarchical_Weightwise``
(:432-570) are the mean-field Reparameterization layers with one more level: every weight has its own prior variance with an
Inv-Gamma(a0, b0) hyper-prior and a variational Inv-Gamma(exp(log_a_q), exp(log_b_q)) posterior. The forward -- weights, draws, RNG
coordinates, kernels -- is exactly the parent's; what changes is the KL term, which here is a SUM over the weights (csrc/bt_kl_hier.hip:
one sweep forward, one element-wise launch backward, instead of the reference's ~40 ATen passes each way).

Deviations, all refusals:
  * ``Conv2dReparameterizationHierarchical_Weightwise(bias=True)`` raises at construction: the reference's own forward cannot run
    with a bias (its kl_loss() broadcasts the kernel-shaped hyper-prior against the [Co] bias, and where that happens to broadcast,
    kl_div is called without its prior_type). ``bias=False`` is the supported form.
  * inside ``mc.TrainGraph(fused=True)`` a forward raises: that step's fused sweep computes the Gaussian KL.
  * CPU tensors raise the usual RuntimeError: there is no CPU implementation.
The two non-weightwise classes raise NotImplementedError from their constructors, as in the reference.
"""
import torch
from torch.nn import Parameter

from ... import mc
from .conv_variational import Conv2dReparameterization
from .linear_variational import LinearReparameterization

HYPO_A = 1.0
HYPO_B = 1.0


class _HierarchicalKL:
    """What the two weightwise classes share: the seven-tensor KL segment, kl_loss(), and a forward that runs the parent's with its
    Gaussian KL off and attaches this KL once per call (whatever the number of MC samples)."""
    _sync_kl = False           # the pack check's sweep computes the Gaussian closed form: never for these layers
    _hier_kl = True            # get_kl_loss gathers these layers into bt_kl_hier launches
    _hypo_attrs = ("prior_hypo_a_weight", "prior_hypo_b_weight")

    def _hier_params(self):
        self.register_parameter("log_a_q_" + self._wname, Parameter(torch.full_like(self._w("mu"), 0.0)))
        self.register_parameter("log_b_q_" + self._wname, Parameter(torch.full_like(self._w("mu"), 0.0)))
        self._hier_cache = {}

    def __getstate__(self):      # (a copy's cache would be keyed by the original's tensors)
        d = super().__getstate__()
        d["_hier_cache"] = {}
        return d

    def _weight_shaped(self, name):
        """The attribute ``name`` -- read at every call: users overwrite the hyper-prior and prior_weight_mu -- on the weight's device,
        expanded to the weight's shape, contiguous fp32. A tensor that already is all that is passed through; anything else (a CPU
        tensor, a scalar, something broadcastable) is copied once per (data_ptr, _version) of what the attribute holds."""
        t, w = getattr(self, name), self._w("mu")
        if not torch.is_tensor(t):
            t = torch.as_tensor(float(t))
        if t.device == w.device and t.dtype == torch.float32 and t.shape == w.shape and t.is_contiguous():
            return t.detach()
        key = (t.data_ptr(), t._version, t.device, t.dtype, tuple(t.shape), w.device, tuple(w.shape))
        c = self._hier_cache.get(name)
        if c is None or c[0] != key:
            v = t.detach().to(device=w.device, dtype=torch.float32).expand(w.shape).contiguous()
            c = self._hier_cache[name] = (key, v, t)      # (t: kept alive, so that its address cannot come back with other contents)
        return c[1]

    def _hier_segment(self):
        """(mu, rho, prior_mu, log_a, log_b, a0, b0): this layer's entry of a bt_kl_hier call."""
        return (self._w("mu"), self._w("rho"), self._weight_shaped("prior_weight_mu"), self._w("log_a_q"), self._w("log_b_q"),
                self._weight_shaped(self._hypo_attrs[0]), self._weight_shaped(self._hypo_attrs[1]))

    def kl_loss(self):
        """The weights' hierarchical KL (a sum over the elements; the bias is not part of it, as in the reference)."""
        from ...autograd import kl_hier
        return kl_hier([self._hier_segment()], [0], ("layer", self._ws_id))

    def _bias_kl(self):
        """kl_div of the bias against its Gaussian (or Laplace) prior: the parent's mean KL, on the parent's kernels."""
        from ...autograd import kl_normal
        seg = (self.mu_bias, self.rho_bias, self.prior_bias_mu, self.prior_bias_sigma)
        return kl_normal([seg], [0], ("layer", self._ws_id), self._prior_kind())

    def _forward_kl(self):
        kl = self.kl_loss()
        return kl if self.mu_bias is None else kl + self._bias_kl()

    def forward(self, input, return_kl=True, residual=None):
        ctx, collect, want_kl, return_kl = self._mc_frame(return_kl)
        if ctx is not None and getattr(ctx, "train_fused", False):
            raise RuntimeError(f"{type(self).__name__} inside TrainGraph(fused=True): that step's fused sweep computes the Gaussian KL, "
                               "not this layer's hierarchical one; capture with fused=False or train eagerly")
        muted, self._kl_muted = self._kl_muted, True      # the parent's forward: same kernels, draws and coordinates, no Gaussian KL
        try:
            out = self._forward(input, False, residual)
        finally:
            self._kl_muted = muted
        kl = self._forward_kl() if want_kl else None
        if collect:
            ctx.kls.append(kl)
        return (out, kl) if return_kl else out


class LinearReparameterizationHierarchical(LinearReparameterization):
    def __init__(self, in_features, out_features, prior_mean=0.0, prior_variance=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0,
                 bias=True, prior_variance_hypo_a=HYPO_A, prior_variance_hypo_b=HYPO_B):
        raise NotImplementedError("Do Not Use this Class. Use LinearReparameterizationHierarchical_Weightwise instead.")


class Conv2dReparameterizationHierarchical(Conv2dReparameterization):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, prior_mean=0.0,
                 prior_variance=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, bias=True, prior_variance_hypo_a=HYPO_A,
                 prior_variance_hypo_b=HYPO_B):
        raise NotImplementedError("Do Not Use this Class. Use Conv2dReparameterizationHierarchical_Weightwise instead.")


class LinearReparameterizationHierarchical_Weightwise(_HierarchicalKL, LinearReparameterization):
    """Reference :293-430. ``prior_hypo_a_weight`` / ``prior_hypo_b_weight`` (plain attributes, ones) are the hyper-prior and
    ``prior_weight_mu`` the prior mean: overwrite them freely, with anything that broadcasts to the weight; they are read at every call.
    forward's KL = kl_loss() + the bias's ordinary mean KL."""

    def __init__(self, in_features, out_features, prior_mean=0.0, prior_variance=1.0, prior_type='normal', posterior_mu_init=0.0,
                 posterior_rho_init=-3.0, bias=True):
        super().__init__(in_features=in_features, out_features=out_features, prior_mean=prior_mean, prior_variance=prior_variance,
                         prior_type=prior_type, posterior_mu_init=posterior_mu_init, posterior_rho_init=posterior_rho_init, bias=bias)
        self._hier_params()
        self.prior_hypo_a_weight = torch.ones_like(self.mu_weight)
        self.prior_hypo_b_weight = torch.ones_like(self.mu_weight)


class Conv2dReparameterizationHierarchical_Weightwise(_HierarchicalKL, Conv2dReparameterization):
    """Reference :432-570, ``bias=False`` (see the module docstring). The hyper-prior is ``prior_variance_hypo_a`` /
    ``prior_variance_hypo_b``, kernel-shaped tensors filled with the constructor's values. forward's KL = kl_loss()."""
    _hypo_attrs = ("prior_variance_hypo_a", "prior_variance_hypo_b")

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, prior_mean=0.0,
                 prior_variance=1.0, posterior_mu_init=0.0, posterior_rho_init=-3.0, bias=True, prior_variance_hypo_a=1.0,
                 prior_variance_hypo_b=1.0):
        if bias:
            raise NotImplementedError(
                "Conv2dReparameterizationHierarchical_Weightwise(bias=True): the reference's own forward cannot run with a bias (its "
                "kl_loss() broadcasts the kernel-shaped hyper-prior against the bias, and kl_div is called without prior_type); "
                "construct it with bias=False")
        super().__init__(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size, stride=stride, padding=padding,
                         dilation=dilation, groups=groups, prior_mean=prior_mean, prior_variance=prior_variance,
                         posterior_mu_init=posterior_mu_init, posterior_rho_init=posterior_rho_init, bias=bias)
        self.prior_variance_hypo_a = torch.ones_like(self.mu_kernel) * prior_variance_hypo_a
        self.prior_variance_hypo_b = torch.ones_like(self.mu_kernel) * prior_variance_hypo_b
        self._hier_params()
