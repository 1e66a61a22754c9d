"""CPU: the INT8 quantised Flipout layers without a GPU -- the class surface and signatures, quantize() against the Reparameterization
twin built from the same tensors (BatchNorm folding included), a state-dict round trip, bnn_to_qbnn(flipout=True) and the default
refusal, the C ABI's refusals (on the host, before any launch), and the model with a calibrated-style quant_dict against the float
Flipout formula. No kernels are launched."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch
import torch.nn as nn

import _q8_flip_cases as FC
import _q8_flip_model as FM
from conftest import ROOT


def test_class_surface_and_signatures():
    import bayesian_torch.layers as RL
    import bayesian_torch_amd.layers as L
    from bayesian_torch.layers.flipout_layers.quantized_conv_flipout import QuantizedConv2dFlipout
    from bayesian_torch.layers.flipout_layers.quantized_linear_flipout import QuantizedLinearFlipout
    from bayesian_torch_amd.layers.flipout_layers import QuantizedConv2dFlipout as C2, QuantizedLinearFlipout as L2
    from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn
    from bayesian_torch_amd.quantization import convert
    assert RL.QuantizedConv2dFlipout is L.QuantizedConv2dFlipout is QuantizedConv2dFlipout is C2
    assert RL.QuantizedLinearFlipout is L.QuantizedLinearFlipout is QuantizedLinearFlipout is L2
    sig = lambda f: list(inspect.signature(f).parameters)[1:]
    assert sig(L.QuantizedLinearFlipout.__init__) == ["in_features", "out_features"]
    assert sig(L.QuantizedConv2dFlipout.__init__) == ["in_channels", "out_channels", "kernel_size", "stride", "padding", "dilation", "groups", "bias"]
    for cls in (L.QuantizedLinearFlipout, L.QuantizedConv2dFlipout):
        assert sig(cls.forward) == ["x", "normal_scale", "default_scale", "default_zero_point", "return_kl"]
        p = inspect.signature(cls.forward).parameters
        assert (p["normal_scale"].default, p["default_scale"].default, p["default_zero_point"].default, p["return_kl"].default) == (6 / 255, 0.1, 128, True)
    assert list(inspect.signature(bnn_to_qbnn).parameters) == ["m", "fuse_conv_bn", "flipout"] and inspect.signature(bnn_to_qbnn).parameters["flipout"].default is False
    assert inspect.signature(convert).parameters["flipout"].default is False
    q = L.QuantizedLinearFlipout(3, 2)
    assert float(q.kl_loss()) == 0.0 and q.quant_dict is None and q.inject_draw is None and q.want_q is False
    assert q._pairs(0.01, 0.02, 6 / 255, 0.1, 128) == FM.scales_default(0.02) and len(FM.PAIRS) == 10
    from bayesian_torch_amd import functional as F
    assert F.Q8_FLIP_PAIRS == FM.PAIRS
    assert FM.quant_sign(torch.tensor([-1.0, 1.0]), 0.1, 128).tolist() == [118, 138]
    with pytest.raises(NotImplementedError, match="groups"):
        L.QuantizedConv2dFlipout(4, 4, 3, groups=2)
    with pytest.raises(NotImplementedError, match="ten"):
        q.prepare()
    with pytest.raises(RuntimeError, match="HIP"):      # no CPU forward
        q(torch.zeros(1, 3))
    with pytest.raises(RuntimeError, match="no float layer"):
        q.quantize()
    for n in (5, 9, 11):
        q.quant_dict = [dict(scale=0.1, zero_point=0)] * n
        with pytest.raises(ValueError, match="ten"):
            q._pairs(0.01, 0.02, 6 / 255, 0.1, 128)


def _fill(layer, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.5 if p.dim() > 1 else 1.0))
    return layer


def _bn(n, seed):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(n, eps=1e-4)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(n, generator=g) + 0.5), bn.bias.copy_(torch.randn(n, generator=g))
        bn.running_mean.copy_(torch.randn(n, generator=g)), bn.running_var.copy_(torch.rand(n, generator=g) + 0.25)
    return bn.eval()


@pytest.mark.parametrize("kind", ["linear", "conv", "conv_bias", "conv_bn", "conv_bias_bn"])
def test_quantize_equals_the_reparameterization_twin(kind):
    """The same parameter tensors in a Flipout and a Reparameterization float layer: every buffer quantize() leaves behind is equal,
    BatchNorm folding included; the state dict loads into a fresh shell."""
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd.models import bnn_to_qbnn as Q
    if kind == "linear":
        f, r = L.LinearFlipout(7, 5), L.LinearReparameterization(7, 5)
        names = ("mu_weight", "rho_weight", "mu_bias", "rho_bias")
    else:
        has_b = "bias" in kind
        f, r = L.Conv2dFlipout(5, 6, 3, stride=2, padding=1, bias=has_b), L.Conv2dReparameterization(5, 6, 3, stride=2, padding=1, bias=has_b)
        names = ("mu_kernel", "rho_kernel") + (("mu_bias", "rho_bias") if has_b else ())
    _fill(f, 3)
    with torch.no_grad():
        for n in names:
            getattr(r, n).copy_(getattr(f, n))
    bn = _bn(6, 4) if kind.endswith("bn") else None
    if kind == "linear":
        qf, qr = Q.qbnn_linear_layer(f, flipout=True), Q.qbnn_linear_layer(r)
    elif bn is None:
        qf, qr = Q.qbnn_conv_layer(f, flipout=True), Q.qbnn_conv_layer(r)
    else:
        qf, qr = Q.batch_norm_folding(f, bn, flipout=True), Q.batch_norm_folding(r, bn)
    assert type(qf).__name__ == ("QuantizedLinearFlipout" if kind == "linear" else "QuantizedConv2dFlipout") and qf._layer_id == f._layer_id
    sf, sr = qf.state_dict(), qr.state_dict()
    assert list(sf) == list(sr) and list(sf)[:4] == ["quantized_mu_weight", "quantized_sigma_weight", "quantized_mu_scale", "quantized_sigma_scale"]
    assert all(torch.equal(sf[k], sr[k]) for k in sf) and qf.bias == qr.bias
    assert sf["quantized_mu_weight"].dtype == torch.int8 and len(torch.unique(sf["quantized_mu_weight"])) > 32
    if kind == "conv_bn":
        assert qf.quantized_mu_bias is not None and qf.quantized_sigma_bias is None and qf.bn_weight is None      # the folded bias: mu only
    shell = type(qf)(*((7, 5) if kind == "linear" else (5, 6, 3, 2, 1)))
    shell.load_state_dict(sf)
    assert list(shell.state_dict()) == list(sf) and all(torch.equal(a, b) for a, b in zip(shell.state_dict().values(), sf.values())) and shell.bias == qf.bias


class _Block(nn.Module):
    def __init__(self, L):
        super().__init__()
        self.conv1 = L.Conv2dFlipout(3, 4, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(4)
        self.fc = L.LinearFlipout(4, 2)


def test_bnn_to_qbnn_converts_on_request_only():
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd.models.bnn_to_qbnn import bnn_to_qbnn
    from bayesian_torch_amd.quantization import convert, prepare
    kinds = lambda net: {n: type(m).__name__ for n, m in net.named_modules() if not m._modules and n}
    for mod, name in ((L.LinearFlipout(3, 2), "LinearFlipout"), (L.Conv2dFlipout(2, 2, 3), "Conv2dFlipout")):
        with pytest.raises(NotImplementedError, match=name + ".*flipout=True"):
            bnn_to_qbnn(nn.Sequential(mod))
    with pytest.raises(NotImplementedError, match="groups"):
        bnn_to_qbnn(nn.Sequential(L.Conv2dFlipout(4, 4, 3, groups=2)), flipout=True)
    with pytest.raises(NotImplementedError, match="Conv1dFlipout"):
        bnn_to_qbnn(nn.Sequential(L.Conv1dFlipout(2, 2, 3)), flipout=True)
    net = _Block(L).eval()
    ids = {n: m._layer_id for n, m in net.named_modules() if hasattr(m, "_layer_id")}
    assert bnn_to_qbnn(net, flipout=True) is None
    assert kinds(net) == {"conv1": "QuantizedConv2dFlipout", "bn1": "BatchNorm2d", "fc": "QuantizedLinearFlipout"}
    assert net.conv1.quantized_mu_bias is None and {n: m._layer_id for n, m in net.named_modules() if hasattr(m, "_layer_id")} == ids
    net = _Block(L).eval()
    bnn_to_qbnn(net, fuse_conv_bn=True, flipout=True)
    assert kinds(net) == {"conv1": "QuantizedConv2dFlipout", "bn1": "Identity", "fc": "QuantizedLinearFlipout"}
    assert net.conv1.quantized_mu_bias is not None and net.conv1.quantized_sigma_bias is None
    mixed = nn.Sequential(L.Conv2dReparameterization(2, 2, 3), L.Conv2dFlipout(2, 2, 3)).eval()      # a mixed model converts both families
    convert(mixed, flipout=True)
    assert kinds(mixed) == {"0": "QuantizedConv2dReparameterization", "1": "QuantizedConv2dFlipout"}
    with pytest.raises(NotImplementedError):       # calibration of a Flipout layer is out of scope: prepare() keeps raising
        L.Conv2dFlipout(2, 2, 3).prepare()
    net = _Block(L).eval()
    prepare(net)
    assert not net.conv1.quant_prepare and not net.fc.quant_prepare


# ---------------------------------------------------------------------------- the C ABI
OK = [(6 / 255, 0), (1e-4, 0)] + [(0.1, 128)] * 8


def _params(lib, pairs, s_mu=0.01, s_sigma=0.01, packs=(256, 512), mu_b=None, sigma_b=None):
    pr = [lib.bt_q8_pair(s, z, 0) for s, z in pairs]
    return lib.bt_q8_flip_params(*pr, s_mu, s_sigma, packs[0], packs[1], mu_b, sigma_b)     # (aligned non-null pack addresses: nothing is launched)


def test_c_abi_refuses_before_any_launch():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    err = lambda: L.bt_last_error_string()

    def lin(pairs=OK, In=8, S=1, rng=True, eps_w=None, eps_b=None, sign_in=None, sign_out=None, **kw):
        P = _params(_lib, pairs, **kw)
        R = _lib.bt_rng(1, None, 0, 1, 0, 0)
        return L.bt_q8_flip_linear_fwd(2, In, 4, S, 1024, 0, C.byref(P), eps_w, eps_b, sign_in, sign_out, C.byref(R) if rng else None, 2048, None, None)

    def conv(pairs, groups):
        P = _params(_lib, pairs)
        g = _lib.bt_conv2d_geom(1, 4, 5, 5, 4, 3, 3, 1, 1, 1, 1, 1, 1, groups)
        R = _lib.bt_rng(1, None, 0, 1, 0, 0)
        return L.bt_q8_flip_conv2d_fwd(C.byref(g), 1, 1024, 0, C.byref(P), None, None, None, None, C.byref(R), 2048, None, None)

    edit = lambda i, s=None, z=None: [(s if (j == i and s is not None) else p[0], z if (j == i and z is not None) else p[1]) for j, p in enumerate(OK)]
    assert lin(packs=(None, 512)) == -1 and b"packs are missing" in err()
    assert lin(packs=(256, 520)) == -1 and b"16-byte aligned" in err()
    for i in range(10):
        assert lin(edit(i, s=0.0)) == -1 and b"scale <= 0" in err()
        assert lin(edit(i, s=-0.1)) == -1
    assert lin(s_mu=0.0) == -1 and lin(s_sigma=-1.0) == -1
    for i in (0, 1):
        assert lin(edit(i, z=1)) == -2 and b"eps / delta zero point" in err()
    for i in range(2, 10):
        assert lin(edit(i, z=-1)) == -1 and b"zero point outside 0..255" in err()
        assert lin(edit(i, z=256)) == -1
        assert lin(edit(i, z=0)) == 0 and lin(edit(i, z=255)) == 0          # plan-only below: the ends of the range are accepted
    assert conv(OK, 2) == -2 and b"groups" in err()
    assert lin(In=65794) == -2 and b"2^31" in err()        # 65794 * 32640 >= 2^31
    assert lin(eps_w=4096) == -1 and b"whole or absent" in err()
    assert lin(eps_w=4096, sign_in=8192) == -1 and b"whole or absent" in err()
    assert lin(eps_w=4096, sign_out=8192) == -1
    assert lin(sign_in=8192) == -1 and b"sign tensor without eps_w" in err()
    assert lin(sign_out=8192) == -1 and lin(sign_in=8192, sign_out=8192) == -1
    assert lin(eps_w=4096, sign_in=8192, sign_out=8192, mu_b=64, sigma_b=128) == -1 and b"eps_w without eps_b" in err()
    assert lin(eps_w=4096, sign_in=8192, sign_out=8192, mu_b=64) == 0       # a folded bias has no sigma: no eps_b needed
    assert lin(edit(2, s=1e-30), s_mu=1e-30) == -1 and b"underflows" in err()      # s_in * s_mu
    assert lin(edit(6, s=1e-42)) == -1 and b"underflows" in err()                  # s_xp * s_delta
    tiny = edit(7, s=1e-25)
    tiny[5] = (1e-25, 128)
    assert lin(tiny) == -1 and b"underflows" in err()                             # s_pert * s_so
    assert lin(rng=False) == -1 and lin(S=0) == -1


@pytest.fixture(autouse=True)
def _plan_only():
    """Every call above that passes validation would launch: the library's plan-only seam records the launch instead. The records
    are drained afterwards (the count and the chain), so that a later test's own records start from nothing."""
    from bayesian_torch_amd import _lib
    h = C.CDLL(_lib.LIB_PATH)
    h.bt_debug_last_launch_record.argtypes = [C.POINTER(C.c_int64), C.c_int]
    h.bt_debug_plan_only(1)
    yield
    h.bt_debug_last_launch_record((C.c_int64 * 11)(), 11)
    h.bt_debug_plan_only(0)


def test_accepted_call_records_the_kernel_name():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    P = _params(_lib, OK)
    R = _lib.bt_rng(1, None, 0, 1, 0, 0)
    assert L.bt_q8_flip_linear_fwd(2, 8, 4, 1, 1024, 0, C.byref(P), None, None, None, None, C.byref(R), 2048, None, None) == 0
    assert L.bt_last_kernel_name().decode() == "q8_flip_fwd<i8 32x32x32,64x128,draws on chip>"
    assert L.bt_q8_flip_linear_fwd(2, 8, 4, 1, 1024, 0, C.byref(P), 4096, None, 8192, 8192, None, 2048, None, None) == 0
    assert L.bt_last_kernel_name().decode() == "q8_flip_fwd<i8 32x32x32,64x128,draws injected>"


def test_header_binding_and_library_agree():
    from bayesian_torch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in ("bt_q8_flip_linear_fwd", "bt_q8_flip_conv2d_fwd"):
        assert re.search(r"^int " + name + r"\(", hdr, flags=re.M), name
        assert name in _lib.EXPORTS and hasattr(handle, name), name
    assert C.sizeof(_lib.bt_q8_flip_params) == 10 * 16 + 2 * 8 + 4 * 8
    m = re.search(r"typedef struct bt_q8_flip_params \{\s*bt_q8_pair ([^;]+);", hdr)
    assert [n.strip() for n in m.group(1).split(",")] == list(FM.PAIRS)
    assert [n for n, _ in _lib.bt_q8_flip_params._fields_][:10] == ["inp" if n == "in" else n for n in FM.PAIRS]
    assert _lib.lib().bt_version() == 302
    mk = open(os.path.join(ROOT, "bayesian_torch_amd", "csrc", "Makefile")).read()
    assert "bt_q8_flip.hip" in mk and "bt_q8_common.h" in mk


# ---------------------------------------------------------------------------- a calibrated-style dict against the float formula
def test_observed_ranges_beat_the_default_pairs():
    """|x| up to 30 saturates the default pairs (0.1 at 128 spans +-12.8). A quant_dict built from the min and max of the float
    formula's intermediates on the same draws (observer_qparams: symmetric for eps and delta, affine for the other eight) brings the
    model closer to conv(x, mu) + b + (conv(x * s_in, sigma * eps) + sigma_b * eps_b) * s_out. A comparison: no threshold is set."""
    from bayesian_torch_amd.quantization.quantize import observer_qparams
    g = torch.Generator().manual_seed(11)
    conv = FC.C3(1, 1, 1)
    mu = torch.randn((6, 5, 3, 3), generator=g) * 0.2
    sigma = torch.rand((6, 5, 3, 3), generator=g) * 0.1 + 0.01
    mu_b, sigma_b = torch.randn(6, generator=g), torch.rand(6, generator=g) * 0.5
    x = (torch.rand((2, 5, 8, 8), generator=g) * 2 - 1) * 30.0
    eps_w, eps_b = torch.randn((6, 5, 3, 3), generator=g), torch.randn(6, generator=g)
    sign_in = torch.randint(0, 2, (2, 5, 8, 8), generator=g).float() * 2 - 1
    sign_out = torch.randint(0, 2, (2, 6, 8, 8), generator=g).float() * 2 - 1
    want, mid = FM.float_flipout(x, mu, sigma, eps_w, sign_in, sign_out, mu_b, sigma_b, eps_b, conv)
    import _q8_model as M
    s_mu, s_sigma = M.scale_of(mu), M.scale_of(sigma)
    q_mu, q_sigma = M.quantize_sym(mu, s_mu), M.quantize_sym(sigma, s_sigma)
    keys = ("eps", "delta", "inp", "mean", "sign_in", "sign_out", "xp", "pert", "pert_signed", "out")
    observed = []
    for i, k in enumerate(keys):
        sc, zp = observer_qparams(mid[k].min().float(), mid[k].max().float(), torch.qint8 if i < 2 else torch.quint8)
        observed.append((float(sc), int(zp)))
    err = {}
    for what, pairs in (("default", FM.scales_default(s_sigma)), ("observed", observed)):
        out = FM.forward(x, q_mu, q_sigma, s_mu, s_sigma, pairs, eps_w, sign_in, sign_out, mu_b, sigma_b, eps_b, conv)[1]
        err[what] = float((out.double() - want).abs().mean())
    print(f"mean |model - float Flipout| over {want.numel()} outputs (mean |float| {float(want.abs().mean()):.3f}): default pairs {err['default']:.4f}, observed ranges {err['observed']:.4f}")
    assert err["observed"] < err["default"]
