"""Conv3d and ConvTranspose{1,2,3}d (both flavours) on the fused kernels -- SURVEY.md section 8(f) rank 4.

Reference behaviour reproduced (paths under /root/reference/bayesian_torch/layers/):
  Conv3dReparameterization / Flipout            variational_layers/conv_variational.py:650-820, flipout_layers/conv_flipout.py:443-638
  ConvTranspose{1,2,3}dReparameterization       conv_variational.py:822-990, 992-1165, 1167-1340
  ConvTranspose{1,2,3}dFlipout                  conv_flipout.py:640-832, 834-1031, 1033-1230
(parameter names and shapes -- ConvTranspose kernels are [Ci][Co/groups][k...] --, constructor signatures, forward(input,
return_kl=True) -> (out, kl) | out, kl_loss()).

Every one of them is ONE launch of the fused Conv2d kernel (sampling, contraction, Flipout signs on chip) behind index
re-arrangements that are exact (no arithmetic):
  * transposed convolution = stride-1 convolution of the zero-upsampled input ((L-1)*s+1 samples, padded by d*(k-1)-p, plus
    output_padding on the far side) with the kernel transposed in its channel axes and flipped in space; sampling is
    element-wise, so transposing / flipping (mu, rho, eps) commutes with it;
  * Conv3d = Conv2d over B*Do images whose channels are (ci, kd): the depth window is unfolded into the channel axis, and the
    [Co][Ci/g][kd][kh][kw] kernel IS a [Co][(Ci/g)*kd][kh][kw] kernel in memory;
  * Conv1d-like = a 1 x k kernel over 1 x L images.
The re-arrangements of x are torch gathers (differentiable: training goes through the same autograd bridge as Conv2d) and cost
one extra pass over the activations. KL is taken by the standalone KL kernel on the parameters in their own layout.

ConvTranspose1d / ConvTranspose2d can skip that pass: ``set_transpose_path("native")`` (or ``BT_CONVT_PATH=native``) hands the
UN-upsampled x to the input-dilated entry points (bt_*_conv2d_updil_fwd), whose kernels resolve the virtual zero-upsampled, padded image
where they form their x addresses -- no tensor of the upsampled size is written or read. It applies to inference calls (no grad) that
draw on chip and crop nothing (d*(k-1) - p >= 0 in every axis); every other call, and any launch the library declines, takes the
materialising path. Reparameterization results are the same bits where both paths run the general split-precision kernel. Flipout
then draws one input sign per REAL element ([B][Ci][spatial], the reference's layout and distribution), so its samples differ from
the materialising path's, whose stream runs over the upsampled tensor. Under the "native" setting ``_last["x_path"]`` says which path
the call took ("native" | "upsample") and ``_last["x_shape"]`` is the shape of the x that was launched. The default is "upsample":
every launch, and the launch record, as before. ConvTranspose3d and the training path always materialise.

Conv3d can skip its pass in the same way: ``set_conv3d_path("native")`` (or ``BT_CONV3D_PATH=native``) hands the real x, as the view
[B][Ci * D][H][W], and a ``dwin=(kd, D, sd, dd, pd)`` entry to the depth-window entry points (bt_*_conv2d_dwin_fwd), whose kernels
resolve the depth window where they form their x addresses -- launch image b * Do + do, launch channel ci * kd + j reads depth plane
do * sd - pd + j * dd, a zero outside [0, D) -- so nothing of the unfolded size (kd / sd times the activations) is written or read.
It applies to calls without grad that draw on chip (no ``inject_draw``, rng mode not "torch") with integer padding; a call that needs
grad or supplies draws, and any launch the library declines, unfolds as before, with the same RNG coordinates. Reparameterization
results are the same bits where both paths run the general split-precision kernel. Flipout then draws ONE input sign per real element
of [B][Ci][D][H][W] -- the reference's layout and distribution; the unfolding path's stream runs over the unfolded tensor, one
independent sign per (element, depth window), which is not the reference's distribution where windows overlap.
Under the "native" setting ``_last["x_path"]`` is "native" | "unfold" and ``_last["x_shape"]`` the launched x's shape. The default
is "unfold": every launch and every ``_last`` key as before.
"""
import os

import torch
import torch.nn.functional as TF

from .. import _lib, rng
from .. import functional as F
from ._fused import FusedBayesLayer
from .base_variational_layer import get_kernel_size


def _tup(v, n):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * n


TRANSPOSE_PATHS = ("upsample", "native")


def _check_path(name, what):
    if name not in TRANSPOSE_PATHS:
        raise ValueError(f"{what}: expected one of {TRANSPOSE_PATHS}, got {name!r}")
    return name


_transpose_path = [_check_path(os.environ.get("BT_CONVT_PATH", "upsample"), "BT_CONVT_PATH")]


def set_transpose_path(name):
    """How ConvTranspose1d / ConvTranspose2d layers feed their launch: "upsample" (default) materialises the zero-upsampled, padded
    input; "native" lets the kernels read the real input through the input-dilated fetch where the call is eligible (module docstring).
    Process-wide; also the environment variable BT_CONVT_PATH, read at import. Returns the previous setting."""
    prev, _transpose_path[0] = _transpose_path[0], _check_path(name, "set_transpose_path")
    return prev


def get_transpose_path():
    return _transpose_path[0]


CONV3D_PATHS = ("unfold", "native")


def _check_conv3d_path(name, what):
    if name not in CONV3D_PATHS:
        raise ValueError(f"{what}: expected one of {CONV3D_PATHS}, got {name!r}")
    return name


_conv3d_path = [_check_conv3d_path(os.environ.get("BT_CONV3D_PATH", "unfold"), "BT_CONV3D_PATH")]


def set_conv3d_path(name):
    """How Conv3d layers feed their launch: "unfold" (default) materialises the depth-unfolded input; "native" lets the kernels read the
    real input through the depth-window fetch where the call is eligible (module docstring). Process-wide; also the environment variable
    BT_CONV3D_PATH, read at import. Returns the previous setting."""
    prev, _conv3d_path[0] = _conv3d_path[0], _check_conv3d_path(name, "set_conv3d_path")
    return prev


def get_conv3d_path():
    return _conv3d_path[0]


class FamilyConvLayer(FusedBayesLayer):
    _kind, _wname = "conv", "kernel"
    _nd, _transposed = 2, False
    _sync_kl = False     # (forward() takes the KL from kl_loss())
    _output_stage = False  # the launch's output is re-arranged afterwards: nothing folds into it (fuse.py skips these layers)

    def _setup(self, in_channels, out_channels, kernel_size, stride, padding, dilation, groups, output_padding, prior_mean, prior_variance,
               posterior_mu_init, posterior_rho_init, bias, tuple_inits):
        if in_channels % groups != 0 or out_channels % groups != 0:
            raise ValueError('invalid in_channels size')
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation, self.groups = kernel_size, stride, padding, dilation, groups
        if self._transposed:
            self.output_padding = output_padding
        self.prior_mean, self.prior_variance = prior_mean, prior_variance
        self.posterior_mu_init = (posterior_mu_init,) if tuple_inits else posterior_mu_init      # trailing commas of the Reparameterization classes
        self.posterior_rho_init = (posterior_rho_init,) if tuple_inits else posterior_rho_init
        self.bias = bias
        ks = get_kernel_size(kernel_size, self._nd)
        wshape = (in_channels, out_channels // groups) + ks if self._transposed else (out_channels, in_channels // groups) + ks
        self._build(wshape, bias, n_out=out_channels)

    # ------------------------------------------------------------------ exact re-arrangements
    def _w_eq(self, t, lead=0):
        """[lead...][kernel in this class's layout] -> the equivalent Conv2d kernel [lead...][Co][Cig'][kh][kw] (views / one copy)."""
        nd, g = self._nd, self.groups
        if self._transposed:                       # [Ci][Co/g][k...] -> [Co][Ci/g][k...], flipped in space
            L = t.shape[:lead]
            Ci, Cog = t.shape[lead], t.shape[lead + 1]
            ks = t.shape[lead + 2:]
            t = t.reshape(L + (g, Ci // g, Cog) + ks).transpose(lead + 1, lead + 2).reshape(L + (g * Cog, Ci // g) + ks)
            t = t.flip(tuple(range(lead + 2, lead + 2 + nd)))
        if nd == 1:
            t = t.unsqueeze(lead + 2)
        elif nd == 3:                              # (ci, kd) -> one channel axis: a view of the same memory when t is contiguous
            t = t.reshape(t.shape[:lead + 1] + (t.shape[lead + 1] * t.shape[lead + 2],) + t.shape[lead + 3:])
        return t.contiguous()

    def _geom(self):
        nd = self._nd
        s, p, d = _tup(self.stride, nd), _tup(self.padding, nd), _tup(self.dilation, nd)
        if any(isinstance(v, str) for v in p):
            raise NotImplementedError("string padding modes are not supported")
        op = _tup(getattr(self, "output_padding", 0), nd)
        ks = tuple(self._w("mu").shape[2:])
        return s, p, d, op, ks

    def _x_eq(self, x):
        """[N][C][spatial...] -> ([N'][C'][H][W] for the Conv2d launch, conv dict, function mapping the launch's output back)."""
        nd = self._nd
        s, p, d, op, ks = self._geom()
        if self._transposed:                       # zero-upsample, then pad by d*(k-1)-p (+ output_padding on the far side)
            up = tuple((n - 1) * si + 1 for n, si in zip(x.shape[2:], s))
            xu = x.new_zeros(x.shape[:2] + up)
            xu[(slice(None), slice(None)) + tuple(slice(None, None, si) for si in s)] = x
            pads = []
            for i in reversed(range(nd)):           # F.pad lists the last axis first; a negative amount crops
                lo = d[i] * (ks[i] - 1) - p[i]
                pads += [lo, lo + op[i]]
            x = TF.pad(xu, pads)
            s, p = (1,) * nd, (0,) * nd
        n0 = x.shape[0]
        if nd == 1:
            x = x.unsqueeze(2)
            conv = dict(stride=(1, s[0]), padding=(0, p[0]), dilation=(1, d[0]), groups=self.groups)
            back = lambda o: o.squeeze(2)
        elif nd == 2:
            conv = dict(stride=s, padding=p, dilation=d, groups=self.groups)
            back = lambda o: o
        else:                                       # unfold the depth window into the channel axis
            x = TF.pad(x, (0, 0, 0, 0, p[0], p[0]))
            win = (ks[0] - 1) * d[0] + 1
            xw = x.unfold(2, win, s[0])[..., ::d[0]]                        # [N][C][Do][H][W][kd]
            Do = xw.shape[2]
            x = xw.permute(0, 2, 1, 5, 3, 4).reshape(n0 * Do, x.shape[1] * ks[0], x.shape[3], x.shape[4])
            conv = dict(stride=s[1:], padding=p[1:], dilation=d[1:], groups=self.groups)
            # (the leading dimension comes from the launch's output: under mc_samples it holds S * n0 * Do rows even when x was shared)
            back = lambda o: o.reshape(-1, Do, o.shape[1], o.shape[2], o.shape[3]).permute(0, 2, 1, 3, 4)
        return x.contiguous(), conv, back

    def _native_pads(self):
        """Per spatial axis (lo, hi): the explicit padding of the dilated input -- exactly what _x_eq hands to F.pad."""
        s, p, d, op, ks = self._geom()
        return [(d[i] * (ks[i] - 1) - p[i], d[i] * (ks[i] - 1) - p[i] + op[i]) for i in range(self._nd)]

    def _native_setting(self):
        """Is this class's path switch on "native"? (Conv3d: set_conv3d_path; the transposed classes: set_transpose_path.) Then the launch
        record says which path the call took."""
        if self._transposed:
            return _transpose_path[0] == "native"
        return self._nd == 3 and _conv3d_path[0] == "native"

    def _native_eligible(self, needs_grad, supplied):
        """Does this call take the input-dilated launch? ConvTranspose1d / 2d under set_transpose_path("native"), no grad, on-chip draws,
        nothing cropped (a negative pad keeps the materialising path). Conv3d under set_conv3d_path("native"): the depth-window launch,
        no grad, on-chip draws (_geom has refused string padding)."""
        if not self._transposed:
            return self._nd == 3 and _conv3d_path[0] == "native" and not needs_grad and not supplied
        return (self._transposed and self._nd <= 2 and _transpose_path[0] == "native" and not needs_grad and not supplied
                and all(lo >= 0 for lo, _ in self._native_pads()))

    def _x_native(self, x):
        """[N][C][spatial...] of a ConvTranspose1d / 2d -> (the real input as [N][C][H][W], the input-dilated conv dict, back);
        of a Conv3d -> (the real input as the view [N][C * D][H][W], the depth-window conv dict, back)."""
        s, p, d, op, ks = self._geom()
        if self._nd == 3:       # Conv3d: the real x as [N][C * D][H][W] (a view), the depth window in the conv dict
            n0, D = x.shape[0], x.shape[2]
            Do = (D + 2 * p[0] - d[0] * (ks[0] - 1) - 1) // s[0] + 1
            conv = dict(stride=s[1:], padding=p[1:], dilation=d[1:], groups=self.groups, dwin=(ks[0], D, s[0], d[0], p[0]))
            back = lambda o: o.reshape(-1, Do, o.shape[1], o.shape[2], o.shape[3]).permute(0, 2, 1, 3, 4)
            xc = x.contiguous()
            return xc.reshape(n0, x.shape[1] * D, x.shape[3], x.shape[4]), conv, back
        pads = self._native_pads()
        if self._nd == 1:
            conv = dict(stride=(1, 1), padding=(0, 0), dilation=(1, d[0]), groups=self.groups, updil=(1, s[0]), pads=(0, 0) + pads[0])
            return x.unsqueeze(2).contiguous(), conv, lambda o: o.squeeze(2)
        conv = dict(stride=(1, 1), padding=(0, 0), dilation=d, groups=self.groups, updil=s, pads=pads[0] + pads[1])
        return x.contiguous(), conv, lambda o: o

    def _sign_out_eq(self, t):
        """[S][B][Co][spatial...] (the reference's layout) -> the Conv2d launch's [S][B'][Co][Ho][Wo]."""
        if self._nd == 1:
            return t.unsqueeze(3).contiguous()
        if self._nd == 3:
            S, B, Co, Do = t.shape[:4]
            return t.permute(0, 1, 3, 2, 4, 5).reshape(S, B * Do, Co, t.shape[4], t.shape[5]).contiguous()
        return t.contiguous()

    def _pack_source(self):
        return self._w_eq(self._w("mu").detach()), self._w_eq(self._w("rho").detach())

    def _w_nat(self, t, lead=0):
        """Inverse of _w_eq: [lead...][Co][Cig'][kh][kw] of the Conv2d launch -> this class's own kernel layout."""
        nd, g = self._nd, self.groups
        ks = tuple(self._w("mu").shape[2:])
        L = tuple(t.shape[:lead])
        if nd == 1:
            t = t.squeeze(lead + 2)
        elif nd == 3:
            t = t.reshape(L + (t.shape[lead], t.shape[lead + 1] // ks[0]) + ks)
        if self._transposed:
            t = t.flip(tuple(range(lead + 2, lead + 2 + nd)))
            Co, Cig = t.shape[lead], t.shape[lead + 1]
            t = t.reshape(L + (g, Co // g, Cig) + ks).transpose(lead + 1, lead + 2).reshape(L + (g * Cig, Co // g) + ks)
        return t.contiguous()

    _sign_keys = ("sign_in_eq", "sign_out_eq")

    def _supplied_draw(self, d, S):
        return dict(d, eps_w=self._w_nat(d["eps_w"], lead=1))

    def materialize_last_draw(self):
        """The last forward's draw in the REFERENCE's layouts where one exists: eps_w [S, *kernel], eps_b [S, Co]. The on-chip
        Flipout signs are defined over the Conv2d launch's operands (``sign_in_eq`` / ``sign_out_eq``: the re-arranged x and the
        launch's output): a transposed convolution's zero-upsampled x carries one sign per real element like the reference, Conv3d's
        depth-unfolded x one sign per (element, depth window) -- see DESIGN.md 4.6. A launch on the "native" path drew its input signs
        over the real x: they are reported as ``sign_in`` [S, B, Ci, spatial...] and ``sign_out`` [S, B, Co, spatial...], the reference's
        own layouts (``sign_out_eq`` stays: the same values in the launch's layout). For a native Conv3d launch that is ``sign_in``
        [S, B, Ci, D, H, W] (bt_rng_sign_fill over the real count) and ``sign_out`` [S, B, Co, Do, Ho, Wo]."""
        res = super().materialize_last_draw()
        if self._flip and self._last.get("x_path") == "native" and "sign_in_eq" in res:
            si, so = res.pop("sign_in_eq"), res["sign_out_eq"]
            if self._nd == 3:
                D = self._last["x_shape"][1] // self.in_channels
                res["sign_in"] = si.reshape(si.shape[:2] + (self.in_channels, D) + tuple(si.shape[3:]))
                Do = so.shape[1] // si.shape[1]
                res["sign_out"] = so.reshape((so.shape[0], si.shape[1], Do) + tuple(so.shape[2:])).permute(0, 1, 3, 2, 4, 5).contiguous()
                return res
            res["sign_in"], res["sign_out"] = (si.squeeze(3), so.squeeze(3)) if self._nd == 1 else (si, so)
        return res

    # ------------------------------------------------------------------ forward
    def forward(self, input, return_kl=True):
        if self.post_scale is not None or self.post_shift is not None or self.post_relu or self.post_pool:
            raise RuntimeError(f"{type(self).__name__} has no fused output stage: post_scale / post_shift / post_relu / post_pool must stay unset")
        ctx, collect, want_kl, return_kl = self._mc_frame(return_kl)
        x = _lib.dev_f32(input, "input")
        if x.dim() != self._nd + 2 or x.shape[1] != self.in_channels:
            raise RuntimeError(f"{type(self).__name__}: expected [N, {self.in_channels}, {self._nd} spatial dims], got {tuple(x.shape)}")
        S, shared, coords = self._call_coords(ctx, x.shape[0])
        mu_e, rho_e = self._w_eq(self._w("mu")), self._w_eq(self._w("rho"))
        needs_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))
        inj = self._take_injected()
        out, x_path = None, ("upsample" if self._transposed else "unfold")
        if self._native_eligible(needs_grad, inj is not None or rng.get_mode() == "torch"):
            xe, conv, back = self._x_native(x)      # the real x: the kernels resolve the upsampled / unfolded operand in their x fetch
            r = F.fused_forward(xe, mu_e, rho_e, self.mu_bias, self.rho_bias, **self._launch_kw(conv, S, shared, coords, {}, self._packed()))
            if r is not None:      # (None: the library declined, nothing was launched -> the materialising path, same coordinates)
                out, x_path = r[0], "native"
        draw = {}
        if out is None:
            xe, conv, back = self._x_eq(x)
            if inj is not None:           # draws in the reference's layouts (test hook), re-arranged like the operands
                draw["eps_w"] = self._w_eq(inj["eps_w"], lead=1)
                if inj.get("eps_b") is not None:
                    draw["eps_b"] = inj["eps_b"]
                if self._flip:
                    si = inj["sign_in"]
                    draw["sign_in"] = self._x_eq(si.reshape((-1,) + tuple(si.shape[2:])))[0].reshape((si.shape[0], -1) + tuple(xe.shape[1:]))
                    draw["sign_out"] = self._sign_out_eq(inj["sign_out"])
            elif rng.get_mode() == "torch":
                raise NotImplementedError("rng mode 'torch' covers Linear / Conv1d / Conv2d; the rest of the family draws on chip or takes inject_draw")
            if needs_grad:
                from ..autograd import FusedForward
                if coords.call_base is not None:
                    raise RuntimeError("graph-replayed draws (call_base) are not supported on the training path")
                out = FusedForward.apply(xe, mu_e, rho_e, self.mu_bias, self.rho_bias, self._launch_kw(conv, S, shared, coords, draw, self._packed()))
            else:
                out, _ = F.fused_forward(xe, mu_e, rho_e, self.mu_bias, self.rho_bias, **self._launch_kw(conv, S, shared, coords, draw, self._packed()))
        Be = xe.shape[0] // (1 if shared else S)
        self._last = dict(draw=draw or None, rng=coords, S=S, kernel=_lib.lib().bt_last_kernel_name().decode(),
                          w_eq_shape=tuple(mu_e.shape), x_shape=(Be,) + tuple(xe.shape[1:]), out_shape=(out.shape[0] // S,) + tuple(out.shape[1:]))
        if self._native_setting():      # (under the default setting the record stays what it was, key for key)
            self._last["x_path"] = x_path
        out = back(out).contiguous()
        kl = self.kl_loss() if want_kl else None
        if collect:
            ctx.kls.append(kl)
        return (out, kl) if return_kl else out


def _make(name, nd, transposed, flip, doc):
    tuple_inits = not flip

    if transposed:
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, output_padding=0,
                     prior_mean=0, prior_variance=1, posterior_mu_init=0, posterior_rho_init=-3.0, bias=True):
            FusedBayesLayer.__init__(self)
            self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, output_padding, prior_mean, prior_variance,
                        posterior_mu_init, posterior_rho_init, bias, tuple_inits)
    elif not flip:      # Conv3dReparameterization: the prior / posterior arguments are positional, without defaults (conv_variational.py:651-663)
        def __init__(self, in_channels, out_channels, kernel_size, prior_mean, prior_variance, posterior_mu_init, posterior_rho_init,
                     stride=1, padding=0, dilation=1, groups=1, bias=True):
            FusedBayesLayer.__init__(self)
            self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, 0, prior_mean, prior_variance,
                        posterior_mu_init, posterior_rho_init, bias, tuple_inits)
    else:
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                     prior_mean=0, prior_variance=1, posterior_mu_init=0, posterior_rho_init=-3.0, bias=True):
            FusedBayesLayer.__init__(self)
            self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, 0, prior_mean, prior_variance,
                        posterior_mu_init, posterior_rho_init, bias, tuple_inits)
    return type(name, (FamilyConvLayer,), dict(__init__=__init__, __doc__=doc, _nd=nd, _transposed=transposed, _flip=flip, __module__=__name__))


Conv3dReparameterization = _make("Conv3dReparameterization", 3, False, False, "Drop-in for reference conv_variational.py:650-820.")
ConvTranspose1dReparameterization = _make("ConvTranspose1dReparameterization", 1, True, False, "Drop-in for reference conv_variational.py:822-990.")
ConvTranspose2dReparameterization = _make("ConvTranspose2dReparameterization", 2, True, False, "Drop-in for reference conv_variational.py:992-1165.")
ConvTranspose3dReparameterization = _make("ConvTranspose3dReparameterization", 3, True, False, "Drop-in for reference conv_variational.py:1167-1340.")
Conv3dFlipout = _make("Conv3dFlipout", 3, False, True, "Drop-in for reference conv_flipout.py:443-638.")
ConvTranspose1dFlipout = _make("ConvTranspose1dFlipout", 1, True, True, "Drop-in for reference conv_flipout.py:640-832.")
ConvTranspose2dFlipout = _make("ConvTranspose2dFlipout", 2, True, True, "Drop-in for reference conv_flipout.py:834-1031.")
ConvTranspose3dFlipout = _make("ConvTranspose3dFlipout", 3, True, True, "Drop-in for reference conv_flipout.py:1033-1230.")

REPARAM = ["Conv3dReparameterization", "ConvTranspose1dReparameterization", "ConvTranspose2dReparameterization", "ConvTranspose3dReparameterization"]
FLIPOUT = ["Conv3dFlipout", "ConvTranspose1dFlipout", "ConvTranspose2dFlipout", "ConvTranspose3dFlipout"]
