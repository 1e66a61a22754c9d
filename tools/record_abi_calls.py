#!/usr/bin/env python
"""Records what the Python forward path HANDS to the C ABI, without a GPU and without the library.

Inside this process only (no seam in the product code) ``_lib.lib()`` becomes a stand-in whose every attribute is a function that records
``(name, args)`` and returns a scripted status, ``_lib.dev_f32`` becomes "contiguous or None", ``_lib.on`` a null context,
``_lib.stream_ptr`` 0 and ``torch.cuda.current_device`` 0. The whole chain -- layers, autograd bridge, functional, mc -- then runs on CPU
tensors, and a table of tiny cases walks its branches. One text record per C call: the function name, every scalar, every field of every
struct and struct array (the prototypes of ``_lib._PROTOS`` say which argument is what), the scripted return value. Pointers are
rendered by identity, never by value: ``name+offset`` for a pointer into a known tensor (the layers' parameters and buffers, their
packs, ``x``, supplied draws), ``#k+offset`` for the k-th other tensor of the case in order of first appearance. Per case also: output
shapes, ``_last`` with tensors replaced by their shapes, ``rng.peek_call()`` before and after, gradient shapes, or the exception.
While a case runs, every tensor that can reach the C ABI is kept alive (``torch.empty`` / ``zeros`` / ``empty_like`` and the
``dev_f32`` stand-in remember what they return), so no address is used twice and the first-appearance numbering is well defined.

``tests/test_abi_call_parity.py`` replays the table against ``tests/golden/abi_calls.txt`` (full text of the first and the last case
that reaches each C function) and ``tests/golden/abi_calls_sha256.json`` (one SHA-256 per case).

    python tools/record_abi_calls.py --dump FILE      # the whole text: diff two trees when a digest differs
    python tools/record_abi_calls.py --write-golden   # re-record tests/golden/ (only when a call is MEANT to change)
"""
import argparse
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN_TABLE = os.path.join(ROOT, "tests", "golden", "abi_calls.txt")
GOLDEN_SHA = os.path.join(ROOT, "tests", "golden", "abi_calls_sha256.json")

from bayesian_torch_amd import _lib, mc, rng                                    # noqa: E402
from bayesian_torch_amd import layers as BL                                     # noqa: E402
from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss                    # noqa: E402

OK, UNSUPPORTED = 0, _lib.ERR_UNSUPPORTED


class Env:
    """One case: the stand-in library, the known tensors, the tensors kept alive, the text."""

    def __init__(self):
        self.lines, self.calls = [], []
        self.script = {}            # C function name -> list of return values, consumed in order (then the default)
        self.keep = []              # every tensor that may reach the C ABI: alive until the case ends
        self.named = []             # (name, tensor) given by the case: x, supplied draws, call_base
        self.modules = []           # (prefix, module): parameters, buffers and packs are looked up when a pointer is rendered
        self.order = {}             # base address of an unnamed tensor -> first-appearance index

    # ---------------------------------------------------------------- pointers by identity
    def _known(self):
        for name, t in self.named:
            yield name, t
        for prefix, mod in self.modules:
            for n, t in list(mod.named_parameters()) + list(mod.named_buffers()):
                yield prefix + n, t
            for n, sub in mod.named_modules():
                pk = getattr(sub, "_pack", None)
                if pk is not None:
                    for label, t in zip(("mu_packed", "sigma_packed", "pack_state"), pk[1:]):
                        yield "%s%s%s%s" % (prefix, n, "." if n else "", label), t

    @staticmethod
    def _inside(p, t):
        base, nbytes = t.data_ptr(), t.numel() * t.element_size()
        return base != 0 and base <= p < base + max(nbytes, 1)

    def ptr(self, p):
        if isinstance(p, C.c_void_p):
            p = p.value
        if not p:
            return "null"
        for name, t in self._known():
            if self._inside(p, t):
                return "%s+%d" % (name, p - t.data_ptr())
        for t in self.keep:
            if self._inside(p, t):
                k = self.order.setdefault(t.data_ptr(), len(self.order))
                return "#%d+%d" % (k, p - t.data_ptr())
        return "?%d" % self.order.setdefault(p, len(self.order))

    # ---------------------------------------------------------------- rendering by prototype
    def struct(self, s):
        out = []
        for fname, ftype in s._fields_:
            v = getattr(s, fname)
            if ftype is C.c_void_p:
                out.append("%s=%s" % (fname, self.ptr(v)))
            elif isinstance(v, C.Structure):
                out.append("%s=%s" % (fname, self.struct(v)))
            elif ftype in (C.c_float, C.c_double):
                out.append("%s=%r" % (fname, v))
            else:
                out.append("%s=%d" % (fname, v))
        return "%s{%s}" % (type(s).__name__, " ".join(out))

    def arg(self, a, atype):
        if atype is C.c_void_p:
            return self.ptr(a)
        if isinstance(atype, type) and issubclass(atype, C._Pointer):
            if a is None:
                return "null"
            elem = atype._type_
            if hasattr(a, "_obj"):                     # byref(struct)
                return "&" + self.struct(a._obj)
            if isinstance(a, C.Structure):
                return "&" + self.struct(a)
            if issubclass(elem, C.Structure):
                return "[%s]" % ", ".join(self.struct(e) for e in a)
            if elem is C.c_void_p:
                return "[%s]" % ", ".join(self.ptr(e) for e in a)
            return "[%s]" % ", ".join(str(int(e)) for e in a)
        return repr(float(a)) if atype in (C.c_float, C.c_double) else str(int(a))

    # ---------------------------------------------------------------- the stand-in library
    def default(self, name):
        return {"bt_last_kernel_name": b"recorded_kernel", "bt_last_error_string": b"scripted error", "bt_conv2d_bwd_workspace": 256}.get(name, 0)

    def __getattr__(self, name):          # (only C function names reach this: everything else is a real attribute)
        if not name.startswith("bt_"):
            raise AttributeError(name)

        def fn(*args):
            rc = self.script[name].pop(0) if self.script.get(name) else self.default(name)
            types = _lib._PROTOS[name][1]
            assert len(types) == len(args), (name, len(types), len(args))
            shown = rc.decode() if isinstance(rc, bytes) else rc
            self.calls.append(name)
            self.lines.append("  %s(%s) -> %s" % (name, ", ".join(self.arg(a, t) for a, t in zip(args, types)), shown))
            return rc
        return fn

    # ---------------------------------------------------------------- what a case uses
    def tensor(self, name, *shape, grad=False, fill=None):
        t = torch.randn(*shape) if fill is None else torch.full(shape, float(fill))
        t.requires_grad_(grad)
        self.named.append((name, t))
        return t

    def layer(self, cls, prefix="", lid=7, freeze=False, **kw):
        m = getattr(BL, cls)(**kw) if isinstance(cls, str) else cls
        for i, sub in enumerate(s for s in m.modules() if hasattr(s, "_layer_id")):
            sub._layer_id = lid + i
        if freeze:
            for p in m.parameters():
                p.requires_grad_(False)
        self.modules.append((prefix, m))
        return m

    def note(self, what, value):
        self.lines.append("  %s: %s" % (what, shapes(value)))

    def last(self, m, what="_last"):
        self.note(what, m._last)

    def grads(self, m, *xs):
        g = {n: p.grad for n, p in m.named_parameters()}
        g.update({"x%d" % i: x.grad for i, x in enumerate(xs)})
        self.note("grads", g)


def shapes(v):
    if isinstance(v, torch.Tensor):
        return "T%s" % (tuple(v.shape),)
    if isinstance(v, dict):
        return "{%s}" % ", ".join("%s=%s" % (k, shapes(x)) for k, x in v.items())
    if isinstance(v, (tuple, list)):
        return ("(%s)" if isinstance(v, tuple) else "[%s]") % ", ".join(shapes(x) for x in v)
    return repr(v)


@contextlib.contextmanager
def stand_in(env, cuda_tensors=False):
    """The replacements, for the duration of one case. ``cuda_tensors``: tensors also claim ``is_cuda`` (mc.sync_model_packs only
    takes layers whose parameters do)."""
    saved = [(o, n, getattr(o, n)) for o, n in ((_lib, "lib"), (_lib, "dev_f32"), (_lib, "on"), (_lib, "stream_ptr"), (torch.cuda, "current_device"),
                                                 (torch.cuda, "is_current_stream_capturing"), (torch, "empty"), (torch, "zeros"), (torch, "empty_like"))]

    def keeping(fn):
        def wrapped(*a, **k):
            t = fn(*a, **k)
            env.keep.append(t)
            return t
        return wrapped

    def dev_f32(t, what):
        if t is None:
            return None
        t = t.contiguous()
        env.keep.append(t)
        return t

    _lib.lib, _lib.dev_f32, _lib.on, _lib.stream_ptr = (lambda: env), dev_f32, (lambda device: contextlib.nullcontext()), (lambda device=None: 0)
    torch.cuda.current_device = lambda: 0
    torch.cuda.is_current_stream_capturing = lambda: False      # (the real one raises without a GPU)
    torch.empty, torch.zeros, torch.empty_like = keeping(torch.empty), keeping(torch.zeros), keeping(torch.empty_like)
    if cuda_tensors:
        torch.Tensor.is_cuda = property(lambda self: True)
    ws, retired = dict(_lib._ws), list(_lib._ws_retired)
    _lib._ws.clear()                       # (keyed by id(layer): a dead layer's larger buffer must not be inherited)
    try:
        yield
    finally:
        for o, n, v in saved:
            setattr(o, n, v)
        if cuda_tensors:
            del torch.Tensor.is_cuda
        _lib._ws.clear()
        _lib._ws.update(ws)
        _lib._ws_retired[:] = retired


# ==================================================================== the case table
LAYERS = {      # class -> (constructor keywords, one batch's x shape at B = 2)
    "LinearReparameterization": (dict(in_features=5, out_features=3), (2, 5)),
    "LinearFlipout": (dict(in_features=5, out_features=3), (2, 5)),
    "Conv2dReparameterization": (dict(in_channels=3, out_channels=4, kernel_size=3, padding=1), (2, 3, 4, 4)),
    "Conv2dFlipout": (dict(in_channels=3, out_channels=4, kernel_size=3, padding=1), (2, 3, 4, 4)),
    "Conv1dReparameterization": (dict(in_channels=3, out_channels=4, kernel_size=3, stride=2, padding=1), (2, 3, 4)),
    "Conv1dFlipout": (dict(in_channels=3, out_channels=4, kernel_size=3, stride=2, padding=1), (2, 3, 4)),
    "Conv3dReparameterization": (dict(in_channels=2, out_channels=4, kernel_size=2, prior_mean=0, prior_variance=1, posterior_mu_init=0,
                                      posterior_rho_init=-3.0), (2, 2, 3, 4, 4)),
    "Conv3dFlipout": (dict(in_channels=2, out_channels=4, kernel_size=2, padding=1), (2, 2, 3, 4, 4)),
    "ConvTranspose1dFlipout": (dict(in_channels=3, out_channels=4, kernel_size=3, stride=2), (2, 3, 4)),
    "ConvTranspose2dReparameterization": (dict(in_channels=4, out_channels=6, kernel_size=3, stride=2, padding=1, output_padding=1, groups=2), (2, 4, 3, 3)),
}
FAMILY = ("Conv3dReparameterization", "Conv3dFlipout", "ConvTranspose1dFlipout", "ConvTranspose2dReparameterization")
CASES = []


def case(name, cuda_tensors=False):
    def deco(fn):
        CASES.append((name, fn, cuda_tensors))
        return fn
    return deco


def out_shape(cls, kw, S=1):
    """Shape of the layer's output for LAYERS' x at S samples (for the supplied Flipout sign_out)."""
    with torch.no_grad():
        x = torch.zeros(LAYERS[cls][1])
        if cls.startswith("Linear"):
            return (2, kw["out_features"])
        fn = {"Conv1d": torch.nn.functional.conv1d, "Conv2d": torch.nn.functional.conv2d, "Conv3d": torch.nn.functional.conv3d,
              "ConvTranspose1d": torch.nn.functional.conv_transpose1d, "ConvTranspose2d": torch.nn.functional.conv_transpose2d}[cls.split("R")[0].split("F")[0]]
        g = kw.get("groups", 1)
        ks = (kw["kernel_size"],) * (x.dim() - 2)
        w = torch.zeros((kw["in_channels"], kw["out_channels"] // g) + ks) if "Transpose" in cls else torch.zeros((kw["out_channels"], kw["in_channels"] // g) + ks)
        extra = dict(output_padding=kw.get("output_padding", 0)) if "Transpose" in cls else {}
        return tuple(fn(x, w, None, kw.get("stride", 1), kw.get("padding", 0), dilation=1, groups=g, **extra).shape)


def draw_for(env, m, cls, kw, S, tag="d"):
    """A supplied draw in the reference's layouts: eps_w [S, *w], eps_b [S, Co], Flipout: sign_in [S, *x], sign_out [S, *out]."""
    w = m._w("mu")
    d = dict(eps_w=env.tensor(tag + ".eps_w", S, *w.shape))
    if m.mu_bias is not None:
        d["eps_b"] = env.tensor(tag + ".eps_b", S, m.mu_bias.numel())
    if m._flip:
        d["sign_in"] = env.tensor(tag + ".sign_in", S, *LAYERS[cls][1], fill=1)
        d["sign_out"] = env.tensor(tag + ".sign_out", S, *out_shape(cls, kw), fill=-1)
    return d


def x_for(env, cls, S=1, grad=False, name="x"):
    shp = LAYERS[cls][1]
    return env.tensor(name, S * shp[0], *shp[1:], grad=grad)


def fwd(env, m, x, *a, **k):
    out = m(x, *a, **k)
    env.note("out", out)
    if hasattr(m, "_last"):
        env.last(m)
    return out


def _per_class():
    for cls, (kw, _) in LAYERS.items():
        for bias in (True, False):
            tag = "%s%s" % (cls, "" if bias else "-nobias")

            @case("bare/" + tag)
            def _(env, cls=cls, kw=kw, bias=bias):
                m = env.layer(cls, bias=bias, freeze=True, **kw)
                with torch.no_grad():
                    fwd(env, m, x_for(env, cls))
                    fwd(env, m, x_for(env, cls, name="x2"), return_kl=False)

            @case("mc-shared/" + tag)
            def _(env, cls=cls, kw=kw, bias=bias):
                m = env.layer(cls, bias=bias, **kw)
                with torch.no_grad(), mc.mc_samples(3, 2, sample0=5, collect_kl=True) as ctx:
                    fwd(env, m, x_for(env, cls), return_kl=False)
                    env.note("ctx.kls", ctx.kls)

            @case("mc-stacked/" + tag)
            def _(env, cls=cls, kw=kw, bias=bias):
                m = env.layer(cls, bias=bias, **kw)
                with torch.no_grad(), mc.mc_samples(3, 2, collect_kl=False, call_base=env.tensor("call_base", 1)) as ctx:
                    fwd(env, m, x_for(env, cls, S=3))
                    env.note("ctx.kls", ctx.kls)

            @case("inject-dict/" + tag)
            def _(env, cls=cls, kw=kw, bias=bias):
                m = env.layer(cls, bias=bias, **kw)
                with torch.no_grad(), mc.mc_samples(3, 2, collect_kl=True):
                    m.inject_draw = draw_for(env, m, cls, kw, 3)
                    fwd(env, m, x_for(env, cls))
                    env.note("materialize", m.materialize_last_draw())

            @case("train/" + tag)
            def _(env, cls=cls, kw=kw, bias=bias):
                m = env.layer(cls, bias=bias, **kw)
                x = x_for(env, cls, grad=bias)
                out, kl = fwd(env, m, x)
                (out.sum() + kl).backward()
                env.grads(m, x)

        @case("dnn-to-bnn-flag/" + cls)
        def _(env, cls=cls, kw=kw):
            m = env.layer(cls, **kw)
            m.dnn_to_bnn_flag = True
            with torch.no_grad():
                fwd(env, m, x_for(env, cls), return_kl=True)
            with torch.no_grad(), mc.mc_samples(2, 2, collect_kl=True) as ctx:
                fwd(env, m, x_for(env, cls, name="x2"))
                env.note("ctx.kls", ctx.kls)

        @case("inject-list/" + cls)
        def _(env, cls=cls, kw=kw):
            m = env.layer(cls, **kw)
            m.inject_draw = [draw_for(env, m, cls, kw, 1, "d0"), draw_for(env, m, cls, kw, 1, "d1")]
            with torch.no_grad():
                fwd(env, m, x_for(env, cls))
                fwd(env, m, x_for(env, cls, name="x2"), return_kl=False)
            env.note("left", m.inject_draw)

        @case("materialize/" + cls)
        def _(env, cls=cls, kw=kw):
            m = env.layer(cls, **kw)
            with torch.no_grad(), mc.mc_samples(2, 2):
                fwd(env, m, x_for(env, cls, S=2))
            env.note("materialize", m.materialize_last_draw())

        @case("train-mc/" + cls)
        def _(env, cls=cls, kw=kw):
            m = env.layer(cls, **kw)
            x = x_for(env, cls, S=2, grad=True)
            with mc.mc_samples(2, 2, sample0=3):
                out = fwd(env, m, x, return_kl=False)
            (out.sum() + m.kl_loss()).backward()
            env.grads(m, x)

        if cls not in FAMILY:
            @case("torch-mode/" + cls)
            def _(env, cls=cls, kw=kw):
                m = env.layer(cls, **kw)
                rng.set_mode("torch")
                with torch.no_grad():
                    fwd(env, m, x_for(env, cls))
                    with mc.mc_samples(2, 2):
                        fwd(env, m, x_for(env, cls, name="x2"))
                    env.note("materialize", m.materialize_last_draw())
                x = x_for(env, cls, name="x3")
                out, kl = fwd(env, m, x)
                (out.sum() + kl).backward()
                env.grads(m)


_per_class()


@case("lstm/two-steps")
def _(env):
    for bias in (True, False):
        m = env.layer("LSTMReparameterization", prefix="b%d." % bias, lid=3, in_features=4, out_features=3, bias=bias)
        x = env.tensor("x%d" % bias, 2, 2, 4)
        with torch.no_grad():
            env.note("out", m(x))
            env.last(m.ih, "ih._last")
            env.last(m.hh, "hh._last")
        hs, _, kl = m(x)
        (hs.sum() + kl).backward()
        env.grads(m)


@case("linear/extra-leading-dims")
def _(env):
    m = env.layer("LinearFlipout", in_features=5, out_features=3)
    with torch.no_grad():
        fwd(env, m, env.tensor("x", 2, 3, 5))
    x = env.tensor("x2", 2, 1, 2, 5, grad=True)
    out, kl = fwd(env, m, x)
    out.sum().backward()
    env.grads(m, x)


# ---------------------------------------------------------------- model level
@case("model/sync-model-packs", cuda_tensors=True)
def _(env):
    model = torch.nn.Sequential(BL.Conv2dReparameterization(3, 4, 3, padding=1), BL.Conv2dFlipout(4, 4, 1, bias=False), torch.nn.Flatten(),
                                BL.LinearReparameterization(64, 3, prior_type="laplace"))
    env.layer(model, lid=1)
    x = env.tensor("x", 2, 3, 4, 4)
    for collect in (True, True, False):
        env.lines.append("  -- collect_kl %s" % collect)
        with torch.no_grad(), mc.mc_samples(3, 2, collect_kl=collect) as ctx:
            mc.sync_model_packs(model, ctx, overlap=False)
            env.note("synced", len(ctx.synced))
            env.note("sync_kl", len(ctx.sync_kl))
            h, _ = model[0](x)
            h, _ = model[1](h)
            out, _ = model[3](model[2](h))
            env.note("out", out)
            env.note("ctx.kls", ctx.kls)
            for i in (0, 1, 3):
                env.last(model[i], "%d._last" % i)
    env.lines.append("  -- without a context, forced")
    with torch.no_grad():
        mc.sync_model_packs(model, force=True)


# ---------------------------------------------------------------- inject path "split"
def _split(cls):
    kw = LAYERS[cls][0]

    @case("split-path/" + cls)
    def _(env):
        m = env.layer(cls, **kw)
        rng.set_inject_path("split")
        env.script[_fwd_name(cls)] = [OK, UNSUPPORTED, OK, OK]
        with torch.no_grad():
            for i, (S, note) in enumerate(((2, "packed launch taken"), (3, "second geometry declined: natural-layout retry"),
                                           (3, "same geometry again: the memo skips the pack passes"))):
                env.lines.append("  -- %s" % note)
                with mc.mc_samples(S, 2, collect_kl=True):
                    m.inject_draw = draw_for(env, m, cls, kw, S, "d%d" % i)
                    fwd(env, m, x_for(env, cls, name="x%d" % i))
            env.note("eps_pack", {k: (sorted(map(repr, v)) if isinstance(v, set) else v) for k, v in m._eps_pack.items()})
            env.lines.append("  -- a draw without the bias part is not whole: general path")
            d = draw_for(env, m, cls, kw, 1, "d3")
            d.pop("eps_b")
            m.inject_draw = d
            fwd(env, m, x_for(env, cls, name="x3"))


def _fwd_name(cls):
    return "bt_%s_%s_fwd" % ("flipout" if "Flipout" in cls else "reparam", "linear" if cls.startswith("Linear") else "conv2d")


for _c in ("LinearReparameterization", "Conv2dReparameterization", "Conv2dFlipout", "LinearFlipout", "Conv1dFlipout", "Conv3dReparameterization"):
    _split(_c)


@case("split-path/torch-mode-and-stacked")
def _(env):
    cls = "Conv2dFlipout"
    kw = LAYERS[cls][0]
    m = env.layer(cls, **kw)
    rng.set_inject_path("split")
    rng.set_mode("torch")
    with torch.no_grad(), mc.mc_samples(2, 2):
        fwd(env, m, x_for(env, cls, S=2))
        fwd(env, m, x_for(env, cls, name="x2"))


@case("split-path/functional-without-state")
def _(env):
    from bayesian_torch_amd import functional as F
    m = env.layer("Conv2dFlipout", **LAYERS["Conv2dFlipout"][0])
    d = draw_for(env, m, "Conv2dFlipout", LAYERS["Conv2dFlipout"][0], 2)
    x = x_for(env, "Conv2dFlipout")
    with torch.no_grad():
        packed = F.pack_params(m.mu_kernel, m.rho_kernel)
        env.note("out", F.fused_forward(x, m.mu_kernel, m.rho_kernel, m.mu_bias, m.rho_bias, flip=True, S=2, packed=packed, inject_path="split",
                                        conv=dict(stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1), seed=9, call=4, layer_id=2, sample0=1, **d))


# ---------------------------------------------------------------- output stage
def _stage_layer(env, cls="Conv2dReparameterization"):
    return env.layer(cls, prefix=cls + ".", **LAYERS[cls][0])


@case("stage/scale-shift-relu")
def _(env):
    for cls in ("Conv2dReparameterization", "LinearFlipout"):
        m = _stage_layer(env, cls)
        n = m._w("mu").shape[0]
        m.post_scale, m.post_shift = torch.ones(n), torch.zeros(n)
        with torch.no_grad():
            fwd(env, m, x_for(env, cls, name="x." + cls))
            m.post_relu = True
            fwd(env, m, x_for(env, cls, name="x2." + cls), return_kl=False)
            m.post_scale = m.post_shift = None
            fwd(env, m, x_for(env, cls, name="x3." + cls), return_kl=False)


@case("stage/residual")
def _(env):
    m = _stage_layer(env)
    with torch.no_grad(), mc.mc_samples(3, 2):
        fwd(env, m, x_for(env, "Conv2dReparameterization"), residual=env.tensor("res_shared", 2, 4, 4, 4))
        fwd(env, m, x_for(env, "Conv2dReparameterization", S=3, name="x2"), residual=env.tensor("res_stacked", 6, 4, 4, 4))
        m.post_relu = True
        fwd(env, m, x_for(env, "Conv2dReparameterization", name="x3"), return_kl=False, residual=env.tensor("res3", 6, 4, 4, 4))


@case("stage/pool-accepted-and-declined")
def _(env):
    m = _stage_layer(env, "Conv2dFlipout")
    m.post_pool = m.post_relu = True
    env.script["bt_flipout_conv2d_fwd"] = [OK, UNSUPPORTED, OK]
    with torch.no_grad(), mc.mc_samples(2, 2, collect_kl=True):
        fwd(env, m, x_for(env, "Conv2dFlipout"))
        env.lines.append("  -- the fused launch declined: a second launch and the pooling pass")
        fwd(env, m, x_for(env, "Conv2dFlipout", name="x2"))


@case("stage/pool-with-split-draw")
def _(env):
    cls = "Conv2dReparameterization"
    m = _stage_layer(env)
    m.post_pool = True
    rng.set_inject_path("split")
    env.script["bt_reparam_conv2d_fwd"] = [UNSUPPORTED, UNSUPPORTED, UNSUPPORTED, OK]
    with torch.no_grad():
        m.inject_draw = draw_for(env, m, cls, LAYERS[cls][0], 1)
        fwd(env, m, x_for(env, cls))


# ---------------------------------------------------------------- other inference branches
@case("inference/laplace-prior")
def _(env):
    for cls in ("LinearReparameterization", "Conv2dReparameterization"):
        m = env.layer(cls, prefix=cls + ".", prior_type="laplace", **LAYERS[cls][0])
        with torch.no_grad():
            fwd(env, m, x_for(env, cls, name="x." + cls))
            env.note("kl_loss", m.kl_loss())
        out, kl = fwd(env, m, x_for(env, cls, name="x2." + cls))
        (out.sum() + kl).backward()
        env.grads(m)


@case("inference/scratch-bytes-0-and-4096")
def _(env):
    for cls in ("Conv2dReparameterization", "LinearReparameterization", "Conv2dFlipout"):
        m = env.layer(cls, prefix=cls + ".", **LAYERS[cls][0])
        env.script["bt_fused_scratch_bytes"] = [0, 4096, 4096, 0]
        with torch.no_grad():
            for i in range(3):
                fwd(env, m, x_for(env, cls, name="x%d.%s" % (i, cls)), return_kl=i != 1)


@case("inference/fused-kl-knob")
def _(env):
    from bayesian_torch_amd.layers import _fused
    m = env.layer("Conv2dReparameterization", **LAYERS["Conv2dReparameterization"][0])
    before, _fused.BT_FUSED_KL = _fused.BT_FUSED_KL, True
    try:
        with torch.no_grad():
            fwd(env, m, x_for(env, "Conv2dReparameterization"))
    finally:
        _fused.BT_FUSED_KL = before


@case("inference/forced-pack-and-cached-segment")
def _(env):
    m = env.layer("LinearReparameterization", **LAYERS["LinearReparameterization"][0])
    with torch.no_grad():
        fwd(env, m, x_for(env, "LinearReparameterization"))
        m.invalidate_pack()
        fwd(env, m, x_for(env, "LinearReparameterization", name="x2"), return_kl=False)
        fwd(env, m, x_for(env, "LinearReparameterization", name="x3"))


# ---------------------------------------------------------------- training
def _train_fused(stub):
    @case("train-fused/kl-stub-%s" % stub)
    def _(env):
        model = torch.nn.Sequential(BL.Conv2dReparameterization(3, 4, 3, padding=1), torch.nn.Flatten(), BL.LinearFlipout(64, 3, bias=False))
        env.layer(model, lid=1)
        for m in model:
            m.dnn_to_bnn_flag = stub
        x = env.tensor("x", 2, 3, 4, 4, grad=True)
        with mc.mc_samples(1, 2) as ctx:
            ctx.train_fused = True
            h = model[0](x)
            h = h if stub else h[0]
            out = model[2](model[1](h))
            out = out if stub else out[0]
        env.note("out", out)
        env.last(model[0], "0._last")
        env.last(model[2], "2._last")
        env.note("live", [m is model[0] or m is model[2] for m in ctx.live_layers])
        kl = get_kl_loss(model)
        env.note("kl", kl)
        (out.sum() + kl).backward()
        env.grads(model, x)
        env.lines.append("  -- the same step, every layer asked by itself (kl_loss)")
        with mc.mc_samples(1, 2) as ctx:
            ctx.train_fused = True
            h = model[0](x)
            out = model[2](model[1](h if stub else h[0]))
            out = out if stub else out[0]
        kl = model[0].kl_loss() + model[2].kl_loss()
        (out.sum() + kl).backward()
        env.grads(model, x)


_train_fused(False)
_train_fused(True)


@case("train/kl-loss-and-get-kl-loss")
def _(env):
    model = torch.nn.Sequential(BL.Conv2dFlipout(3, 4, 3), torch.nn.Flatten(), BL.LinearReparameterization(16, 3), BL.Conv3dFlipout(2, 2, 2))
    env.layer(model, lid=1)
    with torch.no_grad():
        env.note("kl_loss", model[0].kl_loss())
        env.note("get_kl_loss", get_kl_loss(model))
    kl = model[3].kl_loss() + get_kl_loss(model)
    env.note("kl", kl)
    kl.backward()
    env.grads(model)


@case("train/aten-checker")
def _(env):
    from bayesian_torch_amd import autograd
    before, autograd.BACKWARD_IMPL = autograd.BACKWARD_IMPL, "aten"
    try:
        for cls in ("Conv2dFlipout", "LinearReparameterization"):
            m = env.layer(cls, prefix=cls + ".", **LAYERS[cls][0])
            x = x_for(env, cls, S=2, grad=True, name="x." + cls)
            with mc.mc_samples(2, 2):
                out, kl = fwd(env, m, x)
            (out.sum() + kl).backward()
            env.grads(m, x)
    finally:
        autograd.BACKWARD_IMPL = before


@case("train/x-only-and-weights-only")
def _(env):
    m = env.layer("Conv2dReparameterization", freeze=True, **LAYERS["Conv2dReparameterization"][0])
    x = x_for(env, "Conv2dReparameterization", grad=True)
    out = fwd(env, m, x, return_kl=False)
    out.sum().backward()
    env.grads(m, x)
    m.mu_kernel.requires_grad_(True)
    out = fwd(env, m, x_for(env, "Conv2dReparameterization", name="x2"), return_kl=False)
    out.sum().backward()
    env.grads(m)


# ---------------------------------------------------------------- refusals
def refusal(name, cuda_tensors=False):
    def deco(fn):
        @case("refusal/" + name, cuda_tensors)
        def _(env):
            m, run = fn(env)
            try:
                run()
                env.lines.append("  did not raise")
            except Exception as e:      # noqa: BLE001 -- the type and the text ARE the record
                env.lines.append("  raises: %s: %s" % (type(e).__name__, e))
            env.note("_last", getattr(m, "_last", "-"))
        return fn
    return deco


def _nograd(m, x, **k):
    def run():
        with torch.no_grad():
            m(x, **k)
    return run


for _cls in ("Conv2dReparameterization", "LinearFlipout", "Conv1dFlipout", "Conv3dFlipout"):
    @refusal("wrong-channel-count/" + _cls)
    def _(env, cls=_cls):
        m = env.layer(cls, **LAYERS[cls][0])
        shp = list(LAYERS[cls][1])
        shp[-1 if cls.startswith("Linear") else 1] += 1
        return m, _nograd(m, env.tensor("x", *shp))

    @refusal("batch-mismatch/" + _cls)
    def _(env, cls=_cls):
        m = env.layer(cls, **LAYERS[cls][0])

        def run():
            with torch.no_grad(), mc.mc_samples(3, 4):
                m(x_for(env, cls))
        return m, run

    @refusal("inject-wrong-S/" + _cls)
    def _(env, cls=_cls):
        m = env.layer(cls, **LAYERS[cls][0])
        m.inject_draw = draw_for(env, m, cls, LAYERS[cls][0], 2)
        return m, _nograd(m, x_for(env, cls))


@refusal("empty-batch")
def _(env):
    m = env.layer("Conv2dReparameterization", **LAYERS["Conv2dReparameterization"][0])
    return m, _nograd(m, env.tensor("x", 0, 3, 4, 4))


@refusal("linear-extra-dims-inside-mc")
def _(env):
    m = env.layer("LinearReparameterization", **LAYERS["LinearReparameterization"][0])

    def run():
        with torch.no_grad(), mc.mc_samples(2, 2):
            m(env.tensor("x", 2, 2, 5))
    return m, run


@refusal("folded-stage-under-grad")
def _(env):
    m = env.layer("Conv2dReparameterization", **LAYERS["Conv2dReparameterization"][0])
    m.post_relu = True
    return m, lambda: m(x_for(env, "Conv2dReparameterization"))


@refusal("residual-under-grad")
def _(env):
    m = env.layer("Conv2dReparameterization", **LAYERS["Conv2dReparameterization"][0])
    return m, lambda: m(x_for(env, "Conv2dReparameterization"), residual=env.tensor("res", 2, 4, 4, 4))


@refusal("residual-of-wrong-size")
def _(env):
    m = env.layer("Conv2dReparameterization", **LAYERS["Conv2dReparameterization"][0])
    return m, _nograd(m, x_for(env, "Conv2dReparameterization"), residual=env.tensor("res", 3, 4, 4, 4))


@refusal("post-scale-without-shift")
def _(env):
    m = env.layer("Conv2dReparameterization", **LAYERS["Conv2dReparameterization"][0])
    m.post_scale = torch.ones(4)
    return m, _nograd(m, x_for(env, "Conv2dReparameterization"))


@refusal("pool-on-linear")
def _(env):
    m = env.layer("LinearReparameterization", **LAYERS["LinearReparameterization"][0])
    m.post_pool = True
    return m, _nograd(m, x_for(env, "LinearReparameterization"))


@refusal("empty-convolution-output")
def _(env):
    m = env.layer("Conv2dReparameterization", in_channels=3, out_channels=4, kernel_size=5)
    return m, _nograd(m, x_for(env, "Conv2dReparameterization"))


@refusal("family-torch-mode")
def _(env):
    m = env.layer("Conv3dFlipout", **LAYERS["Conv3dFlipout"][0])
    rng.set_mode("torch")
    return m, _nograd(m, x_for(env, "Conv3dFlipout"))


@refusal("family-post-relu")
def _(env):
    m = env.layer("ConvTranspose2dReparameterization", **LAYERS["ConvTranspose2dReparameterization"][0])
    m.post_relu = True
    return m, _nograd(m, x_for(env, "ConvTranspose2dReparameterization"))


@refusal("family-call-base-in-training")
def _(env):
    m = env.layer("ConvTranspose1dFlipout", **LAYERS["ConvTranspose1dFlipout"][0])

    def run():
        with mc.mc_samples(1, 2, call_base=env.tensor("call_base", 1)):
            m(x_for(env, "ConvTranspose1dFlipout"))
    return m, run


@refusal("launch-error")
def _(env):
    m = env.layer("LinearFlipout", **LAYERS["LinearFlipout"][0])
    env.script["bt_flipout_linear_fwd"] = [-1]
    return m, _nograd(m, x_for(env, "LinearFlipout"))


@refusal("materialize-before-forward")
def _(env):
    m = env.layer("Conv3dFlipout", **LAYERS["Conv3dFlipout"][0])
    return m, m.materialize_last_draw


@refusal("materialize-under-call-base")
def _(env):
    m = env.layer("LinearFlipout", **LAYERS["LinearFlipout"][0])
    with torch.no_grad(), mc.mc_samples(1, 2, call_base=env.tensor("call_base", 1)):
        m(x_for(env, "LinearFlipout"))
    return m, m.materialize_last_draw


# ---------------------------------------------------------------- INT8: calibration (prepare / convert) and the quantised layers
Q8_CLASSES = ("LinearReparameterization", "Conv2dReparameterization", "LinearFlipout", "Conv2dFlipout")


def _prepared(env, cls, bn=None):
    """A float layer of LAYERS' shape that observes from now on (the Flipout classes on request: ``prepare(flipout=True)``)."""
    m = env.layer(cls, **LAYERS[cls][0])
    kw = dict(flipout=True) if m._flip else {}
    if bn is not None:
        kw["bn"] = bn
    m.prepare(**kw)
    return m


def _q8_calib(cls):
    kw = LAYERS[cls][0]

    @case("q8-calib/bare/" + cls, cuda_tensors=True)
    def _(env):
        m = _prepared(env, cls)
        with torch.no_grad():
            fwd(env, m, x_for(env, cls))
            fwd(env, m, x_for(env, cls, name="x2"), return_kl=False)

    @case("q8-calib/inject/" + cls, cuda_tensors=True)
    def _(env):
        m = _prepared(env, cls)
        m.inject_draw = draw_for(env, m, cls, kw, 1)
        with torch.no_grad():
            fwd(env, m, x_for(env, cls))

    @case("q8-calib/torch-mode/" + cls, cuda_tensors=True)
    def _(env):
        m = _prepared(env, cls)
        rng.set_mode("torch")
        with torch.no_grad():
            fwd(env, m, x_for(env, cls))

    @case("q8-calib/mc/" + cls, cuda_tensors=True)
    def _(env):
        m = _prepared(env, cls)
        with torch.no_grad(), mc.mc_samples(2, 2, sample0=3):
            env.lines.append("  -- x shared")
            fwd(env, m, x_for(env, cls))
            env.lines.append("  -- x stacked")
            fwd(env, m, x_for(env, cls, S=2, name="x2"))

    if cls.startswith("Conv"):
        @case("q8-calib/batchnorm/" + cls, cuda_tensors=True)
        def _(env):
            bn = torch.nn.BatchNorm2d(kw["out_channels"]).eval()
            env.modules.append(("bn.", bn))
            m = _prepared(env, cls, bn)
            env.note("calib", {k: getattr(m, k, "-") for k in ("calib_coef", "calib_shift", "_calib_fused")})
            with torch.no_grad():
                out, _ = fwd(env, m, x_for(env, cls))
                env.lines.append("  -- the BatchNorm's hook: out is observed behind it")
                env.note("bn(out)", bn(out))
            m._calib_release()
            with torch.no_grad():
                env.lines.append("  -- released: the hook is gone")
                env.note("bn(out)", bn(out))


for _c in Q8_CLASSES:
    _q8_calib(_c)


def _quantised(env, cls, quant_dict=None):
    """-> (the float layer, its INT8 twin after ``bnn_to_qbnn`` of a one-layer model). The two weight scales are planted (exact binary
    fractions): everything the launch is handed is then the same on every host."""
    from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn
    f = getattr(BL, cls)(**LAYERS[cls][0])
    model = torch.nn.Sequential(f)
    env.layer(model, prefix="model.")
    bnn_to_qbnn(model, flipout=f._flip)
    q = model[0]
    q.quantized_mu_scale.fill_(0.5)
    q.quantized_sigma_scale.fill_(0.25)
    q.quant_dict, q._cache = quant_dict, None
    env.note("converted", type(q).__name__)
    return f, q


def _dict_of(n):
    return [{"scale": 0.5 ** (k + 1), "zero_point": 0 if k < 2 else 100 + k} for k in range(n)]


def _q8_layer(cls):
    kw = LAYERS[cls][0]
    n_pairs = 10 if "Flipout" in cls else 5

    @case("q8/bare/" + cls, cuda_tensors=True)
    def _(env):
        _, q = _quantised(env, cls)
        with torch.no_grad():
            fwd(env, q, x_for(env, cls))
            env.note("materialize", q.materialize_last_draw())
            env.lines.append("  -- the packs are kept: no second bt_q8_pack")
            fwd(env, q, x_for(env, cls, name="x2"), return_kl=False)

    @case("q8/mc/" + cls, cuda_tensors=True)
    def _(env):
        _, q = _quantised(env, cls)
        with torch.no_grad(), mc.mc_samples(2, 2, sample0=3):
            env.lines.append("  -- x shared")
            fwd(env, q, x_for(env, cls))
            env.lines.append("  -- x stacked")
            fwd(env, q, x_for(env, cls, S=2, name="x2"))

    @case("q8/inject/" + cls, cuda_tensors=True)
    def _(env):
        f, q = _quantised(env, cls)
        q.inject_draw = draw_for(env, f, cls, kw, 1)
        with torch.no_grad():
            fwd(env, q, x_for(env, cls))
            env.note("materialize", q.materialize_last_draw())

    @case("q8/torch-mode/" + cls, cuda_tensors=True)
    def _(env):
        _, q = _quantised(env, cls)
        rng.set_mode("torch")
        with torch.no_grad(), mc.mc_samples(2, 2):
            fwd(env, q, x_for(env, cls))
            env.note("materialize", q.materialize_last_draw())

    @case("q8/want-q-and-quant-dict/" + cls, cuda_tensors=True)
    def _(env):
        _, q = _quantised(env, cls, _dict_of(n_pairs))
        q.want_q = True
        with torch.no_grad():
            fwd(env, q, x_for(env, cls))

    @refusal("q8-quant-dict-of-wrong-length/" + cls, cuda_tensors=True)
    def _(env):
        _, q = _quantised(env, cls, _dict_of(n_pairs - 1))
        return q, _nograd(q, x_for(env, cls))


for _c in Q8_CLASSES:
    _q8_layer(_c)


def _planted(m):
    """Statistics as calibration batches would have left them, written on the host: row k is (-(k + 1) / 4, (k + 1) / 2)."""
    k = torch.arange(1, m.calib_minmax.shape[0] + 1, dtype=torch.float32)
    m.calib_minmax.copy_(torch.stack([-k / 4, k / 2], 1))
    return m


def _convert(env, m, **kw):
    from bayesian_torch_amd.quantization import convert
    model = torch.nn.Sequential()
    model.add_module("conv1" if type(m).__name__.startswith("Conv") else "fc", m)
    model.add_module("bn1", kw.pop("bn", torch.nn.Identity()))
    convert(model, flipout=m._flip, **kw)
    q = model[0]
    env.note("converted", type(q).__name__)
    env.note("quant_dict", q.quant_dict)
    return q


for _cls in Q8_CLASSES:
    @case("q8-convert/planted/" + _cls)
    def _(env, cls=_cls):
        m = _planted(_prepared(env, cls))
        _convert(env, m)

    @refusal("q8-convert/empty-row/" + _cls)
    def _(env, cls=_cls):
        m = _planted(_prepared(env, cls))
        m.calib_minmax[-1, 0] = float("inf")
        return m, lambda: _convert(env, m)

    @refusal("q8-convert/nonfinite/" + _cls)
    def _(env, cls=_cls):
        m = _planted(_prepared(env, cls))
        m.calib_nonfinite.fill_(3)
        return m, lambda: _convert(env, m)

for _cls in ("Conv2dReparameterization", "Conv2dFlipout"):
    @case("q8-convert/planted-with-batchnorm/" + _cls)
    def _(env, cls=_cls):
        bn = torch.nn.BatchNorm2d(LAYERS[cls][0]["out_channels"]).eval()
        m = _planted(_prepared(env, cls, bn))
        q = _convert(env, m, bn=bn, fuse_conv_bn=True)
        env.note("bias", q.quantized_mu_bias)
        env.note("hooks left on the BatchNorm", len(bn._forward_hooks))

    @refusal("q8-convert/fuse-mismatch/" + _cls)
    def _(env, cls=_cls):
        bn = torch.nn.BatchNorm2d(LAYERS[cls][0]["out_channels"]).eval()
        m = _planted(_prepared(env, cls, bn))
        return m, lambda: _convert(env, m, bn=bn)

    @refusal("q8-convert/fuse-mismatch-the-other-way/" + _cls)
    def _(env, cls=_cls):
        m = _planted(_prepared(env, cls))
        return m, lambda: _convert(env, m, bn=torch.nn.BatchNorm2d(LAYERS[cls][0]["out_channels"]).eval(), fuse_conv_bn=True)


for _cls in ("Conv2dReparameterization", "LinearFlipout"):
    @refusal("q8-calib/forward-that-needs-grad/" + _cls)
    def _(env, cls=_cls):
        m = _prepared(env, cls)
        return m, lambda: m(x_for(env, cls))

    @refusal("q8-calib/stage-folded-after-prepare/" + _cls)
    def _(env, cls=_cls):
        m = _prepared(env, cls)
        m.post_relu = True
        return m, _nograd(m, x_for(env, cls))

    @refusal("q8-calib/prepare-of-a-folded-layer/" + _cls)
    def _(env, cls=_cls):
        m = env.layer(cls, **LAYERS[cls][0])
        m.post_relu = True
        return m, lambda: m.prepare(flipout=True) if m._flip else m.prepare()


# ==================================================================== running
def run_case(name, fn, cuda_tensors=False):
    """-> (text of the case, the C function names it reached). Every case starts from the same state."""
    env = Env()
    mode, path, grad = rng.get_mode(), rng.get_inject_path(), torch.is_grad_enabled()
    rng.manual_seed(1234)
    rng.set_call(10)
    rng.set_mode("philox")
    rng.set_inject_path("general")
    torch.set_grad_enabled(True)
    try:
        with stand_in(env, cuda_tensors):
            fn(env)
            env.lines.append("  call: 10 -> %d" % rng.peek_call())
    finally:
        rng.set_mode(mode)
        rng.set_inject_path(path)
        torch.set_grad_enabled(grad)
        rng._state.pinned = False
    return "== %s\n%s\n" % (name, "\n".join(env.lines)), env.calls


def record():
    """-> {case name: (text, [C function names in call order])}, in table order."""
    return {name: run_case(name, fn, cu) for name, fn, cu in CASES}


def digests(rec):
    return {name: hashlib.sha256(text.encode()).hexdigest() for name, (text, _) in rec.items()}


def table(rec):
    """The committed full text: the first and the last case that reaches each C function."""
    first, last = {}, {}
    for name, (_, calls) in rec.items():
        for c in calls:
            first.setdefault(c, name)
            last[c] = name
    keep = set(first.values()) | set(last.values())
    return [name for name in rec if name in keep]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dump", metavar="FILE", help="write the whole table's text")
    ap.add_argument("--write-golden", action="store_true", help="re-record tests/golden/abi_calls.txt and abi_calls_sha256.json")
    args = ap.parse_args()
    rec = record()
    whole = "".join(text for text, _ in rec.values())
    names = sorted({c for _, calls in rec.values() for c in calls})
    print("%d cases, %d C calls, %d C functions, %d bytes of text" % (len(rec), sum(len(c) for _, c in rec.values()), len(names), len(whole)))
    print("sha256 of the whole text:", hashlib.sha256(whole.encode()).hexdigest())
    if args.dump:
        with open(args.dump, "w") as f:
            f.write(whole)
    if args.write_golden:
        with open(GOLDEN_TABLE, "w") as f:
            f.write("".join(rec[name][0] for name in table(rec)))
        with open(GOLDEN_SHA, "w") as f:
            json.dump(digests(rec), f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
