"""INT8 post-training-quantised Bayesian layers. Reparameterization -- ``QuantizedLinearReparameterization`` and
``QuantizedConv2dReparameterization`` of the reference (layers/variational_layers/quantize_linear_variational.py:44-224,
quantize_conv_variational.py:303-552) on the fused int8 MFMA forward (bt_q8_conv2d_fwd / bt_q8_linear_fwd, csrc/bt_q8.hip) -- and, at
the end of this file, Flipout: ``QuantizedLinearFlipout`` and ``QuantizedConv2dFlipout`` on the two-contraction forward
(bt_q8_flip_conv2d_fwd / bt_q8_flip_linear_fwd, csrc/bt_q8_flip.hip; ``_QuantizedFlipoutLayer`` says what differs).

The reference's forward is a chain of ``torch.ops.quantized.*`` calls, which exist on the CPU only. Here the chain -- quantise eps,
quantised mul and add (the sampled int8 weight), quantise x, the int8 contraction, requantise -- is ONE launch for all S Monte-Carlo
samples, and the result is the reference's bit for bit: integer accumulation has no order (tests/_q8_model.py
is the arithmetic in plain torch).

``quantize()`` is plain torch on the parameters' device (it also runs on CPU tensors); the forward needs a HIP device. Storage after
``quantize()``: int8 buffers ``quantized_mu_weight`` / ``quantized_sigma_weight`` with their scales as buffers
(``quantized_mu_scale`` / ``quantized_sigma_scale``), and the fp32 ``quantized_mu_bias`` / ``quantized_sigma_bias`` (the reference
does not quantise the bias either). ROCm tensors have no quantised dtype: ``get_quantized_tensor`` returns ``(int8 tensor, scale)``.

Deviations from the reference: BY DEFAULT the conv layer returns the DEQUANTISED fp32 output where the reference returns a quint8 tensor
(the Linear layer dequantises there too); ``_last["out_q"]`` holds the u8 image when ``want_q`` is set. A caller opts into the
reference's data path with a ``QActivation`` (quantization/qact.py): a layer handed one reads the u8 image as it
is, with the CARRIER's (scale, zero point) in place of the ``in`` pair, and a conv layer then returns a ``QActivation`` at its ``out``
pair (``return_quantized = True``: for an fp32 input as well -- the first layer of a u8 network); nothing fp32-sized is written. ``enable_int8_compute=False`` (the
reference's deprecated dequantise-and-run-fp32 branch) raises NotImplementedError -- with the reference's precedence: a layer that has a
``quant_dict`` takes the calibrated int8 branch whatever ``enable_int8_compute`` says, there and here -- and so does ``prepare()`` of a
quantised layer: calibration happens on the FLOAT layer (``quantization.prepare`` / ``convert``), and the
``quant_dict`` -- a list of five ``{'scale', 'zero_point'}`` entries (eps, mul, add, in, out) -- comes from there or from the caller. The layers are not
``FusedBayesLayer``s: ``fuse.py`` leaves them alone, and their KL is 0 as in the reference.
"""
import torch

from .. import _lib, rng
from .. import functional as F
from ..quantization.qact import QActivation
from ._calibration import FLIPOUT, REPARAM, _sqrt, bn_coef      # noqa: F401 -- (_sqrt: the tests' own bn_coef reads it here)
from ._fused import FusedBayesLayer
from .base_variational_layer import BaseVariationalLayer_, get_kernel_size


def _softplus(rho):
    return torch.log1p(torch.exp(rho))       # the reference's two fp32 operations (their last bit follows the host's exp / log1p)


class _QuantizedLayer(BaseVariationalLayer_):
    _kl_muted = True       # the KL of a quantised layer is 0: an mc_samples context collects nothing from it
    _rng_layer = True      # rng.assign_layer_ids numbers it with the other Bayesian layers
    _mc_frame = FusedBayesLayer._mc_frame
    _call_coords = FusedBayesLayer._call_coords
    _take_injected = FusedBayesLayer._take_injected
    _schema = REPARAM      # its ``pairs`` are what a quant_dict holds, in order
    _sign_keys = ()        # the sign tensors of a draw, beside eps_w and eps_b

    def _init_common(self, wshape, bias):
        self._wshape = tuple(wshape)
        self.bias = bias
        self.quant_prepare = False
        self.is_dequant = False
        self.quant_dict = None
        self.register_buffer("quantized_mu_weight", torch.zeros(self._wshape, dtype=torch.int8))
        self.register_buffer("quantized_sigma_weight", torch.zeros(self._wshape, dtype=torch.int8))
        self.register_buffer("quantized_mu_scale", torch.full((1,), 0.1))
        self.register_buffer("quantized_sigma_scale", torch.full((1,), 0.1))
        self.register_buffer("quantized_mu_bias", None)        # fp32 [Co] once quantize() gives the layer a bias
        self.register_buffer("quantized_sigma_bias", None)     # (None beside a mu: a bias that came from BatchNorm folding)
        self._layer_id = rng.new_layer_id()
        self._last = None
        self._cache = None         # (key, s_mu, s_sigma, packs): the scales as Python floats and the [Co][taps][Ci16] packs
        self.inject_draw = None    # test hook: dict(eps_w [S, *wshape], eps_b [S, Co] or None) consumed instead of a fresh draw (or a list)
        self.want_q = False        # keep the u8 output image of every forward in _last["out_q"]
        self.return_quantized = False      # a conv layer: return a QActivation for an fp32 input as well (the first layer of a u8 network)

    # ------------------------------------------------------------------ conversion
    def get_scale_and_zero_point(self, x, upper_bound=100, target_range=255):
        """Per-tensor symmetric quantiser of x: scale = clamp(max|x|, 0, upper_bound) * 2 / target_range, zero point 0 (tensors)."""
        zero_point = torch.zeros(1).to(x.device)
        xmax = torch.clamp(x.abs().max(), 0, upper_bound)
        return xmax * 2 / target_range, zero_point

    def get_quantized_tensor(self, x, default_scale=0.1):
        """-> (the int8 image of x, its scale as a 0-dim fp32 tensor); a zero scale is replaced by ``default_scale``."""
        scale, _ = self.get_scale_and_zero_point(x.detach())
        scale = scale.to(torch.float32)
        if scale == 0:
            scale = torch.tensor(default_scale, dtype=torch.float32, device=x.device)
        inv = torch.ones((), dtype=torch.float32, device=x.device) / scale      # quantize_per_tensor multiplies by the fp32 reciprocal
        q = torch.clamp(torch.round(x.detach().to(torch.float32) * inv), -128, 127).to(torch.int8)
        return q, scale

    def _store(self, mu_w, sigma_w, mu_b, sigma_b):
        """What quantize() leaves behind: the int8 images and scales of the two weight tensors, the fp32 bias tensors."""
        q, s = self.get_quantized_tensor(mu_w)
        self.quantized_mu_weight, self.quantized_mu_scale = q, s.reshape(1)
        q, s = self.get_quantized_tensor(sigma_w)
        self.quantized_sigma_weight, self.quantized_sigma_scale = q, s.reshape(1)
        self.quantized_mu_bias = None if mu_b is None else mu_b.detach().to(torch.float32).clone()
        self.quantized_sigma_bias = None if sigma_b is None else sigma_b.detach().to(torch.float32).clone()
        self._cache = None

    def _source(self, src):
        """The float layer quantize() reads: the argument, or what the converter left in ``_float`` (the reference copies the float
        layer's __dict__ into the new one; here the parameters are read from the float layer and never registered)."""
        src = self.__dict__.pop("_float", None) if src is None else src
        if src is None:
            raise RuntimeError(f"{type(self).__name__}.quantize(): no float layer to convert (use bnn_to_qbnn, or pass the layer)")
        return src

    def prepare(self):
        raise NotImplementedError("the observer / calibration pipeline (QuantStub observers) is not part of this package: supply quant_dict, "
                                  "a list of five {'scale', 'zero_point'} entries (eps, mul, add, in, out)")

    def dequantize(self):
        raise NotImplementedError("the dequantise-and-run-fp32 branch of the reference is deprecated there and not implemented here")

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        self._cache = None
        for name in ("quantized_mu_bias", "quantized_sigma_bias"):      # a bias exists exactly when the checkpoint has one
            t = state_dict.get(prefix + name)
            setattr(self, name, None if t is None else torch.empty_like(t, device=self.quantized_mu_weight.device))
        self.bias = self.quantized_mu_bias is not None
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self._cache = None
        return super()._apply(fn, *args, **kwargs)

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_cache"] = None
        return d

    # ------------------------------------------------------------------ forward
    def kl_loss(self):
        """0: the reference disables the KL of its quantised layers (their forward returns the literal 0)."""
        return torch.zeros((), dtype=torch.float32, device=self.quantized_mu_weight.device)

    def _frozen(self):
        """-> (s_mu, s_sigma as Python floats, the packs). Read once per conversion / load / move (it synchronises), never inside a
        graph capture: a captured step runs its warm-up first."""
        qm, qs = self.quantized_mu_weight, self.quantized_sigma_weight
        key = (qm.data_ptr(), qs.data_ptr(), qm.device)
        if self._cache is None or self._cache[0] != key:
            if qm.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{type(self).__name__}: converted, loaded or moved since the last eager call; run one forward outside the capture")
            packs = F.q8_pack(qm, qs)
            self._cache = (key, float(self.quantized_mu_scale.item()), float(self.quantized_sigma_scale.item()), packs)
        return self._cache[1:]

    def _pairs(self, *default_args):
        """The (scale, zero point) pairs of this call, in ``_schema.pairs``' order: the ``quant_dict``'s, or the class's defaults."""
        if self.quant_dict is None:
            return self._default_pairs(*default_args)
        names = self._schema.pairs
        if len(self.quant_dict) != len(names):
            raise ValueError(f"quant_dict must hold { {5: 'five', 10: 'ten'}[len(names)] } {{'scale', 'zero_point'}} entries: {', '.join(names)}")
        return [(float(d["scale"]), int(d["zero_point"])) for d in self.quant_dict]

    def _default_pairs(self, s_mu, s_sigma, normal_scale, default_scale, default_zero_point):
        s_mul = s_sigma * float(normal_scale)
        return [(float(normal_scale), 0), (s_mul, 0), (max(s_mul, s_mu), 0), (float(default_scale), int(default_zero_point)),
                (float(default_scale), int(default_zero_point))]

    def _conv(self):
        return None

    def _q8_forward(self, x, enable_int8_compute, normal_scale, default_scale, default_zero_point, return_kl):
        if not enable_int8_compute and self.quant_dict is None:
            raise NotImplementedError("enable_int8_compute=False (dequantise and run in fp32) is deprecated in the reference and not implemented here")
        ctx, _, _, return_kl = self._mc_frame(return_kl)
        qin = x if isinstance(x, QActivation) else None      # a quint8 input: read as it is, with ITS pair (the reference's quint8 branch)
        if qin is None:
            x = _lib.dev_f32(x, "input")
        elif not qin.is_cuda:
            raise RuntimeError(f"input is on {qin.device}: the INT8 forward runs on a HIP (MI355X) device only; there is no CPU implementation of this path")
        conv = self._conv()
        lead = None
        if conv is None:
            if x.shape[-1] != self._wshape[1]:
                raise RuntimeError(f"{type(self).__name__}: expected last dim {self._wshape[1]}, got {tuple(x.shape)}")
            if x.dim() != 2:
                if ctx is not None:
                    raise RuntimeError("MC batching needs [N, features] inputs for Linear layers")
                lead = tuple(x.shape[:-1])
                x = x.reshape(-1, self._wshape[1])
        elif x.dim() != 4 or x.shape[1] != self._wshape[1]:
            raise RuntimeError(f"{type(self).__name__}: expected [N, {self._wshape[1]}, H, W], got {tuple(x.shape)}")
        if x.shape[0] == 0:
            raise RuntimeError("empty batch")
        s_mu, s_sigma, packs = self._frozen()
        pairs = self._pairs(s_mu, s_sigma, normal_scale, default_scale, default_zero_point)
        i_in, i_out = self._schema.pairs.index("in"), self._schema.pairs.index("out")
        if qin is not None:
            pairs = list(pairs)
            pairs[i_in] = qin.pair
        S, shared, coords = self._call_coords(ctx, x.shape[0])
        draw = self._supplied_draw(self._take_injected(), S, x, shared)
        as_q = conv is not None and (qin is not None or self.return_quantized)      # (a Linear layer dequantises, as the reference's does)
        if qin is None and not as_q:
            out, out_q = self._launch(x, packs, s_mu, s_sigma, pairs, conv, S, shared, coords, draw)
        else:
            out, out_q = self._launch(x if qin is None else qin.data, packs, s_mu, s_sigma, pairs, conv, S, shared, coords, draw,
                                      x_shape=None if qin is None else tuple(x.shape), dest="u8" if as_q else "f32")
        B = x.shape[0] // (1 if shared else S)
        tail = self._out_tail(x)
        if as_q:
            out = QActivation(out_q, pairs[i_out][0], pairs[i_out][1], (S * B,) + tail)
        self._last = dict(draw=draw, rng=coords, S=S, shared_x=shared, pairs=pairs, out_q=out_q, x_shape=(B,) + tuple(x.shape[1:]),
                          out_shape=(B,) + tail, kernel=_lib.lib().bt_last_kernel_name().decode())
        if as_q:
            self._last["out"] = out      # the carrier this call returned
        if lead is not None:
            out = out.reshape(lead + (self._wshape[0],))
        return (out, 0) if return_kl else out

    def _out_tail(self, x):
        conv = self._conv()
        if conv is None:
            return (self._wshape[0],)
        return (self._wshape[0],) + F.conv_out_hw(x.shape[2], x.shape[3], self._wshape[2], self._wshape[3], *conv["stride"], *conv["padding"], *conv["dilation"])

    def _has_sampled_bias(self):
        return self.quantized_mu_bias is not None and self.quantized_sigma_bias is not None

    def _supplied_draw(self, inj, S, x, shared):
        """The draw this call reads instead of the on-chip streams -- the injected one, or in rng mode "torch" eps_w, eps_b, then the
        ``_sign_keys`` per sample, the reference's draw order -- as dict(eps_w, eps_b, *_sign_keys), or None."""
        if inj is not None:
            d = dict(eps_w=inj["eps_w"], eps_b=inj.get("eps_b"), **{k: inj[k] for k in self._sign_keys})
            if d["eps_w"].shape[0] != S:
                raise RuntimeError(f"inject_draw holds {d['eps_w'].shape[0]} samples, this call computes {S}")
            return d
        if rng.get_mode() != "torch":
            return None
        dev, B = x.device, x.shape[0] // (1 if shared else S)
        d = dict(eps_w=torch.empty((S,) + self._wshape, device=dev), eps_b=torch.empty((S, self._wshape[0]), device=dev) if self._has_sampled_bias() else None)
        d.update({k: torch.empty((S, B) + tail, device=dev) for k, tail in zip(self._sign_keys, (tuple(x.shape[1:]), self._out_tail(x)))})
        for s in range(S):
            d["eps_w"][s].normal_()
            if d["eps_b"] is not None:
                d["eps_b"][s].normal_()
            for k in self._sign_keys:
                d[k][s].uniform_(-1, 1).sign_()
        return d

    _forward_fn = staticmethod(F.q8_forward)      # the functional forward of the estimator: what _launch calls

    def _launch(self, x, packs, s_mu, s_sigma, pairs, conv, S, shared, coords, draw, **act):
        return self._forward_fn(x, packs, self._wshape, s_mu, s_sigma, pairs, self.quantized_mu_bias, self.quantized_sigma_bias, conv=conv, S=S, shared_x=shared,
                                seed=coords.seed, call=coords.call, layer_id=coords.layer_id, sample0=coords.sample0, call_base=coords.call_base,
                                want_q=self.want_q, **act, **(draw or {}))

    def materialize_last_draw(self):
        """The draw the last forward used: ``eps_w`` [S, *weight shape], ``eps_b`` [S, Co] (None without a sampled bias) and the
        ``_sign_keys`` -- the tensors that were read, or, after an on-chip draw, the streams regenerated from the call's coordinates
        (bt_rng_normal_fill, tensors 0 and 1; bt_rng_sign_fill, tensors 2 and 3)."""
        if self._last is None:
            raise RuntimeError("no forward has run yet")
        st = self._last
        if st["draw"] is not None:
            return dict(st["draw"])
        if st["rng"].call_base is not None:
            raise RuntimeError("draws made under a graph call_base cannot be replayed after the word advanced")
        seed, call_base, call, lid, sample0 = st["rng"]
        dev = self.quantized_mu_weight.device
        d = dict(eps_w=F.rng_fill_normal(seed, call, lid, sample0, 0, st["S"], self._wshape, dev),
                 eps_b=F.rng_fill_normal(seed, call, lid, sample0, 1, st["S"], (self._wshape[0],), dev) if self._has_sampled_bias() else None)
        for i, k in enumerate(self._sign_keys):
            d[k] = F.rng_fill_sign(seed, call, lid, sample0, 2 + i, st["S"], st[("x_shape", "out_shape")[i]], dev)
        return d


class _LinearShell:
    """Construction and conversion of a quantised Linear layer, Reparameterization or Flipout (the float twins name their parameters alike)."""

    def __init__(self, in_features, out_features):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self._init_common((out_features, in_features), True)

    def quantize(self, src=None):
        """Take over the parameters of ``src`` (the float Linear layer; default: the layer ``bnn_to_qbnn`` attached): int8 images of
        mu and log1p(exp(rho)), fp32 bias."""
        src = self._source(src)
        has_b = src.mu_bias is not None
        self.bias = has_b
        self._store(src.mu_weight, _softplus(src.rho_weight.detach()), src.mu_bias if has_b else None, _softplus(src.rho_bias.detach()) if has_b else None)


class QuantizedLinearReparameterization(_LinearShell, _QuantizedLayer):
    """Drop-in for reference ``quantize_linear_variational.py:44-224``. Build it with ``bnn_to_qbnn``."""

    def forward(self, input, enable_int8_compute=True, normal_scale=6 / 255, default_scale=0.2, default_zero_point=128, return_kl=True):
        return self._q8_forward(input, enable_int8_compute, normal_scale, default_scale, default_zero_point, return_kl)


class _Conv2dShell:
    """Construction and conversion of a quantised Conv2d layer, Reparameterization or Flipout. ``bn_*``: set by ``batch_norm_folding``
    before ``quantize()`` folds the BatchNorm into the int8 images and the bias."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=False):
        super().__init__()
        if in_channels % groups != 0 or out_channels % groups != 0:
            raise ValueError('invalid in_channels size')
        if groups != 1:
            raise NotImplementedError(f"{type(self).__name__}: groups must be 1 on the INT8 forward, got {groups}")
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.stride, self.padding, self.dilation, self.groups = stride, padding, dilation, groups
        self.bn_weight = self.bn_bias = self.bn_running_mean = self.bn_running_var = self.bn_eps = None
        kh, kw = get_kernel_size(kernel_size, 2)
        self._init_common((out_channels, in_channels, kh, kw), bias)

    def _conv(self):
        two = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        if isinstance(self.padding, str):
            raise NotImplementedError("string padding modes are not supported")
        return dict(stride=two(self.stride), padding=two(self.padding), dilation=two(self.dilation), groups=1)

    def quantize(self, src=None):
        """Take over the parameters of ``src`` (the float Conv2d layer; default: the layer ``bnn_to_qbnn`` attached), folding the
        BatchNorm given in ``bn_*`` if there is one: the expressions of quantize_conv_variational.py:405-435 in their order, with one
        difference -- the square root of ``running_var + eps`` is the IEEE (correctly rounded) fp32 value (``_sqrt``), where the
        reference takes whatever the host's fp32 ``torch.sqrt`` gives."""
        src = self._source(src)
        mu, sigma = src.mu_kernel.detach(), _softplus(src.rho_kernel.detach())
        has_b = src.mu_bias is not None
        mu_b = sigma_b = None
        if self.bn_weight is None:
            if has_b:
                mu_b, sigma_b = src.mu_bias.detach(), _softplus(src.rho_bias.detach())
        else:
            coef = bn_coef(self, "bn_")
            mu = mu * (coef.view(-1, 1, 1, 1).expand(mu.shape))
            sigma = sigma * (coef.view(-1, 1, 1, 1).expand(sigma.shape))
            if has_b:
                mu_b = (src.mu_bias.detach() - self.bn_running_mean) * coef + self.bn_bias.detach()
                sigma_b = _softplus(src.rho_bias.detach()) * coef
            else:
                mu_b = coef * (-self.bn_running_mean) + self.bn_bias.detach()
        self.bias = mu_b is not None
        self._store(mu, sigma, mu_b, sigma_b)
        self.bn_weight = self.bn_bias = self.bn_running_mean = self.bn_running_var = self.bn_eps = None


class QuantizedConv2dReparameterization(_Conv2dShell, _QuantizedLayer):
    """Drop-in for reference ``quantize_conv_variational.py:303-552``; returns the dequantised fp32 output (the reference: a quint8
    tensor)."""

    def forward(self, input, enable_int8_compute=True, normal_scale=6 / 255, default_scale=0.1, default_zero_point=128, return_kl=True):
        return self._q8_forward(input, enable_int8_compute, normal_scale, default_scale, default_zero_point, return_kl)


class _QuantizedFlipoutLayer(_QuantizedLayer):
    """What the two INT8 Flipout layers add to ``_QuantizedLayer``: ten (scale, zero point) pairs, a draw of four tensors, and the
    two-contraction forward (bt_q8_flip_conv2d_fwd / bt_q8_flip_linear_fwd, csrc/bt_q8_flip.hip).

    One chain for the default and the calibrated branch (the reference's two branches differ, and both are broken: section 4.6h):
    quantise x; o1 = qconv(x, q_mu, mu_b); quantise the two +-1 sign tensors; delta = quantized.mul(q_sigma, quantize(eps));
    x' = quantized.mul(x, sign_in); p = qconv(x', delta, sigma_b * eps_b); out = quantized.add(o1, quantized.mul(p, sign_out)). The
    signs are fair coins, as the float Flipout layers define them.

    ``quant_dict``: a list of TEN ``{'scale', 'zero_point'}`` entries in the reference's order -- eps, delta, in, mean, sign_in, sign_out,
    xp, pert, pert_signed, out -- supplied by the caller, or built by ``convert`` from the statistics of a FLOAT Flipout layer that was
    calibrated (``prepare(flipout=True)``, section 4.6i); ``prepare()`` of this converted layer raises. ``inject_draw``:
    dict(eps_w [S, *weight shape], eps_b [S, Co] or None, sign_in fp32 [S, B, *x.shape[1:]], sign_out fp32 [S, B, Co, ...]); in a sign
    tensor a negative value means -1 and anything else +1. rng mode "torch" draws eps_w, eps_b, sign_in, sign_out per sample."""

    _forward_fn = staticmethod(F.q8_flip_forward)
    _schema = FLIPOUT
    _sign_keys = ("sign_in", "sign_out")

    def prepare(self):
        raise NotImplementedError("calibration happens on the float Flipout layer (quantization.prepare(model, flipout=True), forwards, then "
                                  "convert(model, flipout=True)), not on the converted one; or supply quant_dict, a list of ten "
                                  f"{{'scale', 'zero_point'}} entries ({', '.join(F.Q8_FLIP_PAIRS)})")

    def _default_pairs(self, s_mu, s_sigma, normal_scale, default_scale, default_zero_point):
        dflt = (float(default_scale), int(default_zero_point))
        return [(float(normal_scale), 0), (s_sigma * float(normal_scale), 0)] + [dflt] * 8

class QuantizedLinearFlipout(_LinearShell, _QuantizedFlipoutLayer):
    """Drop-in for reference ``quantized_linear_flipout.py:44-261``. Build it with ``bnn_to_qbnn(flipout=True)``."""

    def forward(self, x, normal_scale=6 / 255, default_scale=0.1, default_zero_point=128, return_kl=True):
        return self._q8_forward(x, True, normal_scale, default_scale, default_zero_point, return_kl)


class QuantizedConv2dFlipout(_Conv2dShell, _QuantizedFlipoutLayer):
    """Drop-in for reference ``quantized_conv_flipout.py:257-514``; returns the dequantised fp32 output. BatchNorm folding as on
    ``QuantizedConv2dReparameterization`` (reference :350-386)."""

    def forward(self, x, normal_scale=6 / 255, default_scale=0.1, default_zero_point=128, return_kl=True):
        return self._q8_forward(x, True, normal_scale, default_scale, default_zero_point, return_kl)


__all__ = ["QuantizedLinearReparameterization", "QuantizedConv2dReparameterization"]      # (the Flipout pair: exported by layers/flipout_layers)
