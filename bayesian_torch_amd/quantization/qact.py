"""u8 activations between the INT8 layers: what a quint8 tensor is in the reference's ``QResNet`` / ``QuantizableResNet`` (DESIGN.md
section 4.6k).

ROCm tensors have no quantised dtype, so ``QActivation`` carries one: a u8 device tensor in the CHANNEL-BLOCKED layout
``[N][ceil(C / 16)][H][W][16]`` (the unit the int8 walk kernel loads: the 16 channels of one pixel are 16 aligned bytes; bytes of
channels >= C hold the zero point; ``[N, F]`` is the same layout at H = W = 1), a scale (a Python float, what ``q_scale()`` returns), a
zero point in 0..255 and the logical shape. A quantised conv layer handed a ``QActivation`` reads it with ITS pair (as the reference's
``input.dtype == torch.quint8`` branch does) and returns one; the Linear layer dequantises.

The carrier implements ``__torch_function__`` as a non-Tensor class: ``nn.ReLU`` (in place or not), ``nn.MaxPool2d``,
``nn.AdaptiveAvgPool2d(1)`` / a global ``nn.AvgPool2d``, ``torch.flatten`` / ``nn.Flatten`` and ``nn.Identity`` of an unmodified model
reach the functions below; any other torch function raises TypeError naming itself. Every function is ONE launch on the current stream
(csrc/bt_q8_act.hip via ``functional.q8_act_*``), synchronises nothing and is graph-capturable; the arithmetic is torch's CPU quantised
operators' bit for bit (tests/test_q8_u8_model_host.py). A leading MC sample count is part of N, as on the fp32 path inside
``mc_samples``.
"""
import torch
import torch.nn as nn
import torch.nn.functional as TF

from .. import functional as F


def _check_pair(scale, zero_point):
    scale, zero_point = float(scale), int(zero_point)
    if not scale > 0.0:
        raise ValueError(f"a quantised activation needs a scale > 0, got {scale}")
    if not 0 <= zero_point <= 255:
        raise ValueError(f"a quint8 zero point lies in 0..255, got {zero_point}")
    return scale, zero_point


class QActivation:
    """A quint8 activation: ``data`` (u8, blocked: ``functional.q8_blocked_shape(shape)``), ``scale``, ``zero_point``, logical ``shape``."""

    def __init__(self, data, scale, zero_point, shape):
        self.scale, self.zero_point = _check_pair(scale, zero_point)
        self._shape = torch.Size(int(v) for v in shape)
        if data.dtype != torch.uint8 or tuple(data.shape) != F.q8_blocked_shape(self._shape):
            raise ValueError(f"the blocked u8 image of {tuple(self._shape)} is uint8 {F.q8_blocked_shape(self._shape)}, got {data.dtype} {tuple(data.shape)}")
        self.data = data

    # ---- the reference-shaped surface
    dtype = torch.quint8
    is_quantized = True

    def q_scale(self):
        return self.scale

    def q_zero_point(self):
        return self.zero_point

    @property
    def pair(self):
        return (self.scale, self.zero_point)

    @property
    def shape(self):
        return self._shape

    def size(self, dim=None):
        return self._shape if dim is None else self._shape[dim]

    def dim(self):
        return len(self._shape)

    @property
    def device(self):
        return self.data.device

    @property
    def is_cuda(self):
        return self.data.is_cuda

    def contiguous(self):
        return self

    def int_repr(self):
        """The u8 levels in natural order ([N, C, H, W] or [N, F]): a torch re-layout of the blocked image, mainly for tests."""
        if len(self._shape) == 2:
            return self.data[:, :self._shape[1]].contiguous()
        N, C, H, W = self._shape
        return self.data.permute(0, 1, 4, 2, 3).reshape(N, -1, H, W)[:, :C].contiguous()

    def dequantize(self):
        return dequantize(self)

    def flatten(self, start_dim=0, end_dim=-1):
        return flatten(self, start_dim, end_dim)

    def view(self, *shape):
        return _as_rows(self, shape, "view")

    def reshape(self, *shape):
        return _as_rows(self, shape, "reshape")

    def __repr__(self):
        return f"QActivation(shape={tuple(self._shape)}, scale={self.scale}, zero_point={self.zero_point}, device={self.device})"

    def _no_plus(self, other):
        raise TypeError("quantised activations are not added with '+' (torch cannot add quint8 tensors either): use "
                        "bayesian_torch_amd.quantization.qact.add / add_relu, or a QFunctional")

    __add__ = __radd__ = __iadd__ = _no_plus

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        handler = _DISPATCH.get(func)
        if handler is None:
            name = getattr(func, "__qualname__", None) or getattr(func, "__name__", None) or repr(func)
            raise TypeError(f"{getattr(func, '__module__', 'torch')}.{name} is not implemented for a QActivation (a quint8 activation): the quantised "
                            "path has relu, max_pool2d, adaptive_avg_pool2d(1) / a global avg_pool2d, flatten, add and add_relu; dequantize() first")
        return handler(*args, **(kwargs or {}))


def from_int_repr(levels, scale, zero_point):
    """The carrier of a u8 tensor in natural order ([N, C, H, W] or [N, F]): a torch re-layout, for tests and for data that arrives as
    levels (padding channels get the zero point)."""
    scale, zero_point = _check_pair(scale, zero_point)
    shape = tuple(levels.shape)
    store = F.q8_blocked_shape(shape)
    if len(shape) == 2:
        data = torch.full(store, zero_point, dtype=torch.uint8, device=levels.device)
        data[:, :shape[1]] = levels
    else:
        N, C, H, W = shape
        full = torch.full((N, store[1] * 16, H, W), zero_point, dtype=torch.uint8, device=levels.device)
        full[:, :C] = levels
        data = full.view(N, store[1], 16, H, W).permute(0, 1, 3, 4, 2).contiguous()
    return QActivation(data, scale, zero_point, shape)


def _q(x, what):
    if not isinstance(x, QActivation):
        raise TypeError(f"{what} takes a QActivation, got {type(x).__name__}")
    return x


def quantize_per_tensor(x, scale, zero_point, dtype=torch.quint8):
    """fp32 [N, C, H, W] or [N, F] -> QActivation: clamp(rne(x * (1 / s)) + z, 0, 255)."""
    if dtype != torch.quint8:
        raise NotImplementedError("activations are quint8")
    scale, zero_point = _check_pair(scale, zero_point)
    return QActivation(F.q8_act_quantize(x, scale, zero_point), scale, zero_point, x.shape)


def dequantize(q):
    """-> fp32 in natural order, (q - z) * s."""
    q = _q(q, "dequantize")
    return F.q8_act_dequantize(q.data, q.shape, q.scale, q.zero_point)


def relu(q, inplace=False):
    """max(q, z); ``inplace``: the carrier's own bytes are overwritten."""
    q = _q(q, "relu")
    data = F.q8_act_relu(q.data, q.shape, q.zero_point, inplace=bool(inplace))
    return q if inplace else QActivation(data, q.scale, q.zero_point, q.shape)


def _add(a, b, scale, zero_point, with_relu):
    a, b = _q(a, "add"), _q(b, "add")
    if tuple(a.shape) != tuple(b.shape):
        raise RuntimeError(f"add: shapes differ, {tuple(a.shape)} and {tuple(b.shape)}")
    po = _check_pair(max(a.scale, b.scale) if scale is None else scale, zero_point)
    return QActivation(F.q8_act_add(a.data, a.shape, a.pair, b.data, b.shape, b.pair, po, relu=with_relu), po[0], po[1], a.shape)


def add(a, b, scale=None, zero_point=0):
    """torch.ops.quantized.add(a, b, scale, zero_point); default: the reference QResNet's max(a.q_scale(), b.q_scale()) and 0."""
    return _add(a, b, scale, zero_point, False)


def add_relu(a, b, scale=None, zero_point=0):
    """torch.ops.quantized.add_relu: the sum clamped at 0 before it is requantised."""
    return _add(a, b, scale, zero_point, True)


def _two(v):
    return tuple(int(t) for t in v) if isinstance(v, (tuple, list)) else (int(v), int(v))


def max_pool2d(q, kernel_size, stride=None, padding=0, dilation=1, ceil_mode=False, return_indices=False):
    """The maximum of the levels over each window; padding positions are ignored."""
    q = _q(q, "max_pool2d")
    if _two(dilation) != (1, 1) or ceil_mode or return_indices or q.dim() != 4:
        raise NotImplementedError("quantised max_pool2d: [N, C, H, W] input, dilation 1, no ceil_mode, no indices")
    k = _two(kernel_size)
    data, shape = F.q8_act_max_pool2d(q.data, q.shape, k, k if stride is None or stride == [] else _two(stride), _two(padding))
    return QActivation(data, q.scale, q.zero_point, shape)


def adaptive_avg_pool2d(q, output_size):
    """The global average pool (output size 1): clamp(rne(float(sum - z * n) * float(1 / n) + z), 0, 255) at q's pair."""
    q = _q(q, "adaptive_avg_pool2d")
    if q.dim() != 4 or _two(output_size) != (1, 1):
        raise NotImplementedError("quantised adaptive_avg_pool2d: output size 1 of an [N, C, H, W] input (the global average pool)")
    data, shape = F.q8_act_avg_pool(q.data, q.shape, q.zero_point)
    return QActivation(data, q.scale, q.zero_point, shape)


def avg_pool2d(q, kernel_size, stride=None, padding=0, ceil_mode=False, count_include_pad=True, divisor_override=None):
    """The GLOBAL average pool: kernel_size equal to the map, no padding."""
    q = _q(q, "avg_pool2d")
    if q.dim() != 4 or _two(kernel_size) != tuple(q.shape[2:]) or _two(padding) != (0, 0) or divisor_override is not None:
        raise NotImplementedError("quantised avg_pool2d: only the global pool (kernel_size equal to the map, no padding, no divisor_override)")
    return adaptive_avg_pool2d(q, 1)


def flatten(q, start_dim=0, end_dim=-1):
    """flatten(1): free for a 1 x 1 map (the blocked layout of [N, C, 1, 1] IS that of [N, C]); a larger map is reordered to the NCHW
    feature order by one small launch."""
    q = _q(q, "flatten")
    nd = q.dim()
    start, end = start_dim % nd, end_dim % nd
    if nd == 2 and (start == end or (start, end) == (1, 1)):
        return q
    if nd != 4 or (start, end) != (1, 3):
        raise NotImplementedError("quantised flatten: start_dim=1 (to [N, features])")
    N, C, H, W = q.shape
    if H == 1 and W == 1:
        return QActivation(q.data.view(N, -1), q.scale, q.zero_point, (N, C))
    data, shape = F.q8_act_unblock(q.data, q.shape, q.zero_point)
    return QActivation(data, q.scale, q.zero_point, shape)


def _as_rows(q, shape, what):
    if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
        shape = tuple(shape[0])
    if len(shape) != 2 or int(shape[0]) != q.shape[0] or int(shape[1]) not in (-1, q.shape[1:].numel()):
        raise NotImplementedError(f"quantised {what}: only {what}(N, -1)")
    return flatten(q, 1) if q.dim() == 4 else q


def _identity(q, *args, **kwargs):
    return q


_DISPATCH = {
    TF.relu: relu, torch.relu: relu,
    TF.relu_: lambda q: relu(q, True), torch.relu_: lambda q: relu(q, True),
    TF.max_pool2d: max_pool2d,
    TF.adaptive_avg_pool2d: adaptive_avg_pool2d,
    TF.avg_pool2d: avg_pool2d,
    torch.flatten: flatten,
    torch.dequantize: dequantize,
}


class QuantStub(nn.Module):
    """``quantize_per_tensor`` as a module, for models written in the reference's style. (A first conv layer with
    ``return_quantized = True`` quantises in its own producer and needs none.)"""

    def __init__(self, scale=0.1, zero_point=128):
        super().__init__()
        self.scale, self.zero_point = _check_pair(scale, zero_point)

    def forward(self, x):
        return x if isinstance(x, QActivation) else quantize_per_tensor(x, self.scale, self.zero_point)


class DeQuantStub(nn.Module):
    def forward(self, x):
        return dequantize(x) if isinstance(x, QActivation) else x


class QFunctional(nn.Module):
    """``torch.ao.nn.quantized.QFunctional`` / ``FloatFunctional`` on carriers: ``add`` and ``add_relu`` at this module's output pair
    (scale None: the reference QResNet's max of the operands' scales)."""

    def __init__(self, scale=None, zero_point=0):
        super().__init__()
        self.scale, self.zero_point = (None if scale is None else float(scale)), int(zero_point)

    def add(self, a, b):
        return add(a, b, self.scale, self.zero_point)

    def add_relu(self, a, b):
        return add_relu(a, b, self.scale, self.zero_point)


__all__ = ["QActivation", "from_int_repr", "quantize_per_tensor", "dequantize", "relu", "add", "add_relu", "max_pool2d", "adaptive_avg_pool2d", "avg_pool2d",
           "flatten", "QuantStub", "DeQuantStub", "QFunctional"]
