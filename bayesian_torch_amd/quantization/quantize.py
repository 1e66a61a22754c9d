"""``prepare`` / ``convert`` -- the reference's post-training flow (``bayesian_torch/quantization/quantize.py``, which re-exports
``ao/quantization/quantize.py:135-172``) for the INT8 layers of this package:

    prepare(model)                      # every convertible Bayesian layer starts observing
    with torch.no_grad():
        for x in calibration_batches:
            model(x)                    # or mc_forward(model, x, S): all S samples' draws are observed
    convert(model)                      # bnn_to_qbnn: each calibrated layer gets its five-entry quant_dict

``prepare(model, flipout=True)`` ... ``convert(model, flipout=True)`` calibrates and converts ``LinearFlipout`` / ``Conv2dFlipout`` too:
thirteen statistics per layer (the reference's twelve Flipout observers and bt_q8_observe_w's fifth row), ten quant_dict entries.

The statistics are the reference's -- per layer the running (min, max) of sigma, mu, eps, sigma * eps, mu + sigma * eps, the input and
the output, seven ``MinMaxObserver``s there -- but they are taken on the device by two kernels behind each forward
(csrc/bt_q8_observe.hip): nothing weight-sized is written and nothing is read back before ``convert()``.

Deviations from the reference, on purpose: its ``prepare(model)`` rebuilds a hard-wired quantizable ResNet50 from ``model.module``'s
state dict and runs ``torch.quantization.prepare`` with the onednn qconfig on it -- a CPU flow for one architecture. Here ``prepare``
works IN PLACE on any model (it returns the same object), needs ``model.eval()``, inserts no torch observers and leaves the
deterministic layers alone. ``fuse_conv_bn=True`` calibrates the layers ``bnn_to_qbnn(fuse_conv_bn=True)`` builds -- weights scaled by
the BatchNorm's coefficient, output observed behind the BatchNorm -- which the reference's flow (``convert`` calls ``bnn_to_qbnn``
without it) cannot express.
"""
from ..layers._calibration import observer_qparams      # noqa: F401 -- (its home; re-exported here, where the reference has it)
from ..models import bnn_to_qbnn as _Q

class _Prepare:
    """What the converter's walk (models/bnn_to_qbnn.py: ``_walk``) does to a model that is being prepared: the layer at every site the
    converter would convert starts observing."""

    def __init__(self, flipout=False):
        self.done = []        # the prepared layers, in walk order
        self.flipout = flipout

    def _try(self, layer, **kw):
        prep = getattr(layer, "prepare", None)
        if not callable(prep) or layer in self.done:
            return
        if self.flipout and type(layer).__name__ in _Q._CONVERTIBLE_FLIPOUT:      # they calibrate on request only, like their conversion
            kw["flipout"] = True
        try:
            prep(**kw)
        except (NotImplementedError, RuntimeError):       # a layer without an INT8 counterpart: the converter is the one that says so
            return
        layer.dnn_to_bnn_flag = True                      # (the reference's enable_prepare does: the model's forward chains plain outputs)
        self.done.append(layer)

    def refuse(self, child):
        pass

    def conv(self, m, name):
        self._try(m._modules[name])

    linear = conv

    def pair(self, holder, c, b):
        conv, bn = holder._modules[c], holder._modules[b]
        if conv in self.done or getattr(conv, "quant_prepare", False) and getattr(conv, "_calib_fused", False):
            return
        if bn.training and callable(getattr(conv, "_calib_prepare", None)):
            raise RuntimeError(f"prepare(fuse_conv_bn=True): the BatchNorm '{b}' beside '{c}' is in training mode; call model.eval() first")
        self._try(conv, bn=bn)

    def left(self, m, name):
        pass              # a layer no folding rule names stays float in the converted model: nothing to calibrate


def enable_prepare(m, fuse_conv_bn=False, flipout=False):
    """Call ``prepare()`` on every layer ``bnn_to_qbnn(m, fuse_conv_bn, flipout)`` would convert, where it exists and does not raise, and
    set the layer's ``dnn_to_bnn_flag`` as the reference does (ao/quantization/quantize.py:135-143). With ``fuse_conv_bn`` the
    convolutions are paired with their BatchNorms by the converter's own rules (``bnn_to_qbnn.conv_bn_pairs``). ``flipout=True``:
    ``LinearFlipout`` / ``Conv2dFlipout`` are prepared too (``prepare(flipout=True)``: thirteen statistics each);
    by default they are left alone. -> the names of the prepared layers."""
    act = _Prepare(flipout)
    _Q._walk(m, fuse_conv_bn, act)
    names = {id(mod): n for n, mod in m.named_modules()}
    return [names.get(id(layer), "") for layer in act.done]


def prepare(model, fuse_conv_bn=False, flipout=False):
    """Start calibrating ``model`` (in place; the model is returned): see the module docstring for what differs from the reference's
    ``prepare``. The model must be in eval mode. ``flipout=True``: the Flipout layers ``convert(flipout=True)`` converts calibrate too."""
    if model.training:
        raise RuntimeError("prepare(): call model.eval() first -- calibration observes the inference forward (BatchNorm running statistics, no dropout)")
    enable_prepare(model, fuse_conv_bn, flipout)
    return model


def convert(model, fuse_conv_bn=False, flipout=False):
    """``bnn_to_qbnn(model, fuse_conv_bn, flipout)``: every calibrated layer becomes an INT8 layer with the ``quant_dict`` its statistics
    give (one host read per layer); ``fuse_conv_bn`` must be what ``prepare`` was given. ``flipout=True`` converts the Flipout layers too
    (calibrated ones -- ``prepare(flipout=True)`` -- get their ten-entry ``quant_dict``; the others the default pairs, or a
    ``quant_dict`` of the caller's). -> the model."""
    _Q.bnn_to_qbnn(model, fuse_conv_bn=fuse_conv_bn, flipout=flipout)
    return model


__all__ = ["prepare", "convert", "enable_prepare", "observer_qparams"]
