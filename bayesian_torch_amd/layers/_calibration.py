"""Calibration of the INT8 layers in one place: which statistics a layer keeps (``CalibSchema``), how a ``quant_dict`` comes out of them
(``observer_qparams``, ``quant_dict_from_stats``), and the engine ``FusedBayesLayer`` inherits (``CalibrationMixin``). A leaf module: it
imports ``functional`` only; the layer classes, the converter and ``quantization`` import it."""
import collections

import torch

from .. import _lib
from .. import functional as F


class CalibSchema(collections.namedtuple("CalibSchema", "rows symmetric pairs")):
    """``rows``: the names of ``calib_minmax``'s (min, max) rows. ``symmetric``: the rows quantised with ``torch.qint8`` (per-tensor
    symmetric; every other row takes the affine ``torch.quint8``). ``pairs``: the rows a ``quant_dict`` takes, in its order."""
    __slots__ = ()

    def index(self, name):
        return self.rows.index(name)

    def row(self, mm, name):
        return mm[self.rows.index(name)]


# The reference's seven observers (conv_variational.py:331-337) and its ``quant_dict[2:]`` selection (models/bnn_to_qbnn.py:105-111); and
# bt_q8_observe_w's five rows ("add": Flipout never forms it, no pair takes it) before the eight quint8 stubs of conv_flipout.py:339-345
REPARAM = CalibSchema(F.CALIB_ROWS, ("sigma", "mu", "eps", "mul", "add"), ("eps", "mul", "add", "in", "out"))
FLIPOUT = CalibSchema(F.CALIB_FLIP_ROWS, ("sigma", "mu", "eps", "delta", "add"), F.Q8_FLIP_PAIRS)
_F32_EPS = torch.finfo(torch.float32).eps


def _f32(v):
    return v.detach().to(device="cpu", dtype=torch.float32) if isinstance(v, torch.Tensor) else torch.tensor(float(v), dtype=torch.float64).to(torch.float32)


def observer_qparams(min_val, max_val, dtype=torch.qint8):
    """``MinMaxObserver.calculate_qparams`` for a recorded range, in fp32 tensor arithmetic on the CPU -> (scale, zero point) as 0-dim
    fp32 / int64 tensors. ``torch.qint8``: the per-tensor symmetric quantiser of the five weight-side observers, scale =
    max(|min(min, 0)|, max(max, 0)) / 127.5, zero point 0. ``torch.quint8``: the affine quantiser of the input and output observers,
    scale = (max(max, 0) - min(min, 0)) / 255, zero point = clamp(0 - round(min(min, 0) / scale), 0, 255). Either scale is floored at
    the fp32 epsilon."""
    lo, hi = _f32(min_val), _f32(max_val)
    zero = torch.zeros_like(lo)
    min_neg, max_pos = torch.min(lo, zero), torch.max(hi, zero)
    eps = torch.tensor(_F32_EPS, dtype=torch.float32)
    if dtype == torch.qint8:
        max_pos = torch.max(-min_neg, max_pos)
        scale = torch.max(max_pos / (float(127 - (-128)) / 2), eps)
        return scale, torch.zeros_like(scale, dtype=torch.int64)
    if dtype == torch.quint8:
        scale = torch.max((max_pos - min_neg) / float(255 - 0), eps)
        zp = 0 - torch.round(min_neg / scale).to(torch.int64)
        return scale, torch.clamp(zp, 0, 255)
    raise ValueError(f"observer_qparams: dtype must be torch.qint8 (symmetric) or torch.quint8 (affine), got {dtype}")


def quant_dict_from_stats(schema, calib_minmax, calib_nonfinite, who):
    """The ``quant_dict`` of a calibrated layer (``who``, as the errors name it): one {'scale', 'zero_point'} per name of ``schema.pairs``
    from the statistics the observer kernels left on the device. ONE host read: the (min, max) pairs and whether a non-finite value was met."""
    host = torch.cat([calib_minmax.detach().reshape(-1).to(torch.float32), (calib_nonfinite.detach().reshape(-1) != 0).to(torch.float32)]).cpu()
    mm, bad = host[:-1].reshape(len(schema.rows), 2), bool(host[-1])
    if bad:
        raise RuntimeError(f"bnn_to_qbnn: {who} met non-finite values while calibrating (calib_nonfinite != 0): its ranges cannot be trusted")
    out = []
    for name in schema.pairs:
        lo, hi = schema.row(mm, name)
        if not bool(torch.isfinite(lo)) or not bool(torch.isfinite(hi)):
            raise RuntimeError(f"bnn_to_qbnn: {who} was prepared but its '{name}' statistics are still empty: run the calibration batches "
                               "(under torch.no_grad()) between prepare() and convert()")
        scale, zp = observer_qparams(lo, hi, torch.qint8 if name in schema.symmetric else torch.quint8)
        out.append({"scale": float(scale), "zero_point": int(zp)})
    return out


def _sqrt(t):
    """The IEEE (correctly rounded) fp32 square root: taken in double and rounded once. torch's CPU fp32 sqrt is not correctly rounded
    on every host: one ulp in one BatchNorm coefficient moved a folded layer's scale between two machines."""
    return torch.sqrt(t.double()).to(t.dtype)


def bn_coef(bn, prefix=""):
    """weight / sqrt(running_var + eps) of a BatchNorm -- or of the ``bn_*`` attributes a quantised conv shell was given (prefix "bn_")."""
    return getattr(bn, prefix + "weight").detach() / _sqrt(getattr(bn, prefix + "running_var") + getattr(bn, prefix + "eps"))


class _BnOutputObserver:
    """Forward hook of the BatchNorm a calibrating layer will be folded with: the layer's ``out`` statistic is the range of the
    BatchNorm's output. An object, not a closure: a deep copy of the model observes into the COPY's layer."""

    def __init__(self, layer):
        self.layer = layer

    def __call__(self, module, args, output):
        if self.layer.quant_prepare and not torch.is_grad_enabled():
            F.minmax_update([(output, self.layer._schema.row(self.layer.calib_minmax, "out"))], self.layer.calib_nonfinite)


class CalibrationMixin:
    """What ``prepare()`` and a calibrating forward of the four convertible classes (Linear / Conv2d, Reparameterization and Flipout) do."""
    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        cls._schema = FLIPOUT if cls._flip else REPARAM

    def _folded(self):
        return self.post_scale is not None or self.post_shift is not None or self.post_relu or self.post_pool

    def _calib_prepare(self, bn=None):
        """Reference conv_variational.py:331-337 (seven QuantStub observers; Flipout, conv_flipout.py:339-345: twelve): empty statistics
        in two persistent buffers, ``calib_minmax`` [len(self._schema.rows), 2] and ``calib_nonfinite`` [1], filled on the device by
        every no-grad forward from now on. ``bn``: the BatchNorm2d that ``bnn_to_qbnn(fuse_conv_bn=True)`` will fold into this layer:
        the weight rows are then those of mu * coef and sigma * coef (``calib_coef``), ``out`` is observed at the BatchNorm's output
        through a forward hook, and a Flipout layer's mean output takes the BatchNorm's shift (``calib_shift``)."""
        name = type(self).__name__
        if getattr(self, "groups", 1) != 1:
            raise NotImplementedError(f"{name}.prepare(): groups={self.groups} has no INT8 counterpart here (groups must be 1)")
        if self._folded():
            raise RuntimeError(f"{name}.prepare(): the layer carries a folded output stage (fuse.py); calibrate the unfolded model")
        if bn is not None and bn.training:
            raise RuntimeError(f"{name}.prepare(): the BatchNorm to fold is in training mode; call model.eval() first")
        self._calib_release()
        mm, bad = F.calib_buffers(self._w("mu").device, len(self._schema.rows))
        self.register_buffer("calib_minmax", mm)
        self.register_buffer("calib_nonfinite", bad)
        coef = shift = None
        if bn is not None:
            coef = bn_coef(bn).to(torch.float32).contiguous()
            if self._flip:
                shift = (bn.bias.detach() - coef * bn.running_mean).to(torch.float32).contiguous()      # quantize()'s folded bias, less mu_b * coef
            self._calib_hook = bn.register_forward_hook(_BnOutputObserver(self))
        self.register_buffer("calib_coef", coef, persistent=False)
        if self._flip:
            self.register_buffer("calib_shift", shift, persistent=False)
        self._calib_fused = bn is not None
        self.quant_prepare = True

    def _calib_release(self):
        """Take the BatchNorm's observer hook out again (``convert()``; a second ``prepare()``)."""
        hook = self.__dict__.pop("_calib_hook", None)
        if hook is not None:
            hook.remove()

    def _calib_observe(self, x, out, mu_t, rho_t, S, coords, draw, conv=None, shared=True):
        """The observer launches of a calibrating forward, on the call's own draws (supplied, or the forward's RNG coordinates): the
        weight sweep; Flipout: the input sweep (in, sign_in, xp) and the observing two-contraction launch (mean, pert, pert_signed,
        sign_out); then one ``minmax_update`` for whichever of ``in`` and ``out`` nobody else fills (a folded BatchNorm's hook: ``out``)."""
        if self._folded():
            raise RuntimeError(f"{type(self).__name__}: folded an output stage (fuse.py) after prepare(); calibrate the unfolded model")
        mm, bad, kernels = self.calib_minmax, self.calib_nonfinite, []
        row = lambda name: self._schema.row(mm, name)

        def run(launch, *a, **k):
            launch(*a, **k)
            kernels.append(_lib.lib().bt_last_kernel_name().decode())
        at = dict(S=S, seed=coords.seed, call=coords.call, layer_id=coords.layer_id, sample0=coords.sample0, call_base=coords.call_base)
        run(F.q8_observe_w, mu_t, rho_t, mm, bad, coef=self.calib_coef, eps=draw.get("eps_w"), **at)      # the schema's first five rows
        if self._flip:
            run(F.q8_flip_observe_x, x, row("in"), row("sign_in"), row("xp"), bad, shared_x=shared, sign_in=draw.get("sign_in"), **at)
            run(F.q8_flip_observe, x, mu_t, rho_t, self.mu_bias, self.rho_bias, row("mean"), row("pert"), row("pert_signed"), row("sign_out"), bad, conv=conv,
                shared_x=shared, coef=self.calib_coef, shift=self.calib_shift, eps_w=draw.get("eps_w"), eps_b=draw.get("eps_b"),
                sign_in=draw.get("sign_in"), sign_out=draw.get("sign_out"), **at)
        segs = ([] if self._flip else [(x, row("in"))]) + ([] if self._calib_fused else [(out, row("out"))])
        if segs:
            run(F.minmax_update, segs, bad)
        self._last.update(observed=True, observer_kernel=kernels[0], observer_kernels=tuple(kernels))
