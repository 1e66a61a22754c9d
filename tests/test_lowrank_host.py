"""CPU: the drop-in surface of Conv2dReparameterization_Multivariate against what the reference's class showed
(tests/golden/lowrank_surface.json, tools/make_goldens_lowrank.py), the path decision, the closed-form KL helper against the
reference's float64 and float32 values, and the three new C-ABI entry points.  No kernels are launched."""
import ctypes
import inspect
import json
import math
import os
import re

import pytest
import torch

import _lowrank_ref as R
from conftest import GOLD, ROOT

SURF = json.load(open(os.path.join(GOLD, "lowrank_surface.json")))


def _cls():
    from bayesian_torch_amd.layers.variational_layers.conv_variational import Conv2dReparameterization_Multivariate
    return Conv2dReparameterization_Multivariate


def test_importable_by_both_module_paths_and_outside_all():
    import bayesian_torch.layers.variational_layers.conv_variational as alias
    import bayesian_torch_amd.layers.variational_layers.conv_variational as own
    assert alias.Conv2dReparameterization_Multivariate is own.Conv2dReparameterization_Multivariate is _cls()
    assert SURF["in_all"] is False and "Conv2dReparameterization_Multivariate" not in own.__all__
    from bayesian_torch_amd.layers._fused import FusedBayesLayer
    from bayesian_torch_amd.layers.base_variational_layer import BaseVariationalLayer_
    assert issubclass(_cls(), BaseVariationalLayer_) and not issubclass(_cls(), FusedBayesLayer)
    assert not hasattr(_cls(), "_pack_segment")          # mc.sync_model_packs skips it


def test_constructor_surface_matches_reference():
    M = _cls()
    params = inspect.signature(M.__init__).parameters
    assert list(params)[1:] == SURF["signature"]
    assert {k: v.default for k, v in params.items() if v.default is not inspect.Parameter.empty} == SURF["defaults"]
    assert list(inspect.signature(M.forward).parameters)[1:] == SURF["forward"]
    assert inspect.signature(M.forward).parameters["return_kl"].default is SURF["return_kl_default"]
    m = M(4, 8, 3, rank=2)
    assert list(m.state_dict()) == ["mu_kernel", "L_param", "prior_mean", "prior_cov_L", "prior_cov_D"] and set(m.state_dict()) == set(SURF["state_dict"])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == SURF["state_dict"]
    assert [k for k, _ in m.named_parameters()] == SURF["parameters"] and [k for k, _ in m.named_buffers()] == SURF["buffers"]
    assert repr(m) == SURF["repr"]
    a = SURF["attributes"]
    for k in ("weight_size", "martern_prior", "in_channels", "out_channels", "kernel_size", "stride", "padding", "dilation", "groups", "bias"):
        assert getattr(m, k) == a[k], k
    assert list(m.BLOCK_MAT.shape) == a["BLOCK_MAT_shape"] and m.rank == 2
    D = m.D_param
    assert list(D.shape) == a["D_param_shape"] and str(D.dtype) == a["D_param_dtype"] and float(D[0]) == a["D_param_value"]
    assert isinstance(D, torch.nn.Parameter) is a["D_param_is_parameter"] and "D_param" not in dict(m.named_buffers())
    L, D2 = m.get_covariance_param()
    assert L is m.L_param and D2 is m.D_param
    assert m.dnn_to_bnn_flag is False and hasattr(m, "_layer_id") and m._last is None


def test_init_statistics_and_prior_buffers():
    torch.manual_seed(5)
    m = _cls()(16, 32, 3, rank=4)
    i = SURF["init"]
    assert m.weight_size == i["n"]
    for t in (m.mu_kernel.detach(), m.L_param.detach()):       # N(0, 0.1^2): mean and std within 5 standard errors
        n = t.numel()
        assert abs(float(t.mean()) - i["mean"]) <= 5 * i["std"] / math.sqrt(n)
        assert abs(float(t.std()) - i["std"]) <= 5 * i["std"] / math.sqrt(2 * (n - 1))
    assert torch.equal(m.prior_mean, torch.full((i["n"],), i["prior_mean"])) and torch.equal(m.prior_cov_L, torch.full((i["n"], 1), i["prior_cov_L"]))
    assert torch.equal(m.prior_cov_D, torch.full((i["n"],), i["prior_cov_D"]))


def test_seeded_construction_matches_reference_draw_order():
    g = R.load(R.case("a"))
    torch.manual_seed(g["meta"]["seed"])
    m = _cls()(**g["meta"]["ctor"])
    assert torch.equal(m.mu_kernel.detach(), g["mu_kernel"]) and torch.equal(m.L_param.detach(), g["L_param"])
    assert torch.equal(m.D_param, g["D_param"])


def test_refusals():
    M = _cls()
    for name, f in (("in_channels % groups", lambda: M(3, 8, 3, groups=2)), ("out_channels % groups", lambda: M(4, 6, 3, groups=4))):
        e = SURF["errors"][name]
        assert e["type"] == "ValueError"
        with pytest.raises(ValueError, match=re.escape(e["message"])):
            f()
    with pytest.raises(ValueError, match="groups must be 1"):
        M(4, 8, 3, groups=2)
    with pytest.raises(ValueError, match="kernel_size must be an int"):
        M(4, 8, (3, 3))
    with pytest.raises(ValueError, match="rank must be an int >= 1"):
        M(4, 8, 3, rank=0)
    m = M(4, 8, 3)
    m.martern_prior = True
    with pytest.raises(NotImplementedError, match="assert not torch.isnan"):
        m(torch.zeros(1, 4, 5, 5))
    with pytest.raises(NotImplementedError, match="Matern"):
        m.kl_loss()
    with pytest.raises(NotImplementedError, match="quantisation"):
        m.prepare()
    m.martern_prior = False
    with pytest.raises(RuntimeError, match="HIP"):      # no CPU implementation of the forward
        m(torch.zeros(1, 4, 5, 5))


def test_layer_ids_are_assigned_by_position():
    import torch.nn as nn
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.layers import LinearReparameterization
    net = nn.Sequential(_cls()(3, 4, 3), nn.ReLU(), _cls()(4, 4, 3, rank=5), nn.Flatten(), LinearReparameterization(4, 2))
    assert rng.assign_layer_ids(net, first=7) == 3
    assert [net[0]._layer_id, net[2]._layer_id, net[4]._layer_id] == [7, 8, 9]


@pytest.mark.parametrize("rank,d_uniform,prior_diag,needs_grad,want", [
    (1, True, True, False, ("in_kernel", "kernel")), (4, True, True, False, ("in_kernel", "kernel")),
    (5, True, True, False, ("mean_prepass", "kernel")), (432, True, True, False, ("mean_prepass", "kernel")),
    (3, True, False, False, ("in_kernel", "materialised")), (7, True, False, False, ("mean_prepass", "materialised")),
    (2, False, True, False, ("materialised", "materialised")), (2, True, True, True, ("materialised", "materialised")),
    (9, False, False, True, ("materialised", "materialised")),
])
def test_path_decision(rank, d_uniform, prior_diag, needs_grad, want):
    from bayesian_torch_amd.layers._lowrank import MAX_R, choose_path
    assert MAX_R == R.MAX_R
    path, kl_path, reason = choose_path(rank, d_uniform, prior_diag, needs_grad)
    assert (path, kl_path) == want
    assert (reason is None) == (want == (R.expected_path(rank), "kernel"))


@pytest.mark.parametrize("tag", R.CASES)
def test_closed_form_kl_against_reference(tag):
    """fp64 on both sides: the helper on CPU tensors against the reference class run in float64 (rtol 1e-9), and against the
    reference's own fp32 value at the project's 1e-4."""
    from bayesian_torch_amd.layers._lowrank import closed_form_kl
    g = R.load(tag)
    n = g["mu_kernel"].numel()
    assert not bool((g["prior_cov_L"] != 0).any())
    kl = closed_form_kl(g["mu_kernel"], g["L_param"], g["D_param"], g["prior_mean"], g["prior_cov_D"])
    assert kl.dtype == torch.float64
    got, want64, want32 = float(kl) / n, float(g["kl64"]), float(g["kl"])
    print(f"{tag}: kl/n {got:.15g}  reference fp64 {want64:.15g} (rel {abs(got - want64) / abs(want64):.2e})  fp32 {want32:.9g} (rel {abs(got - want32) / abs(want32):.2e})")
    assert abs(got - want64) <= 1e-9 * abs(want64)
    assert abs(got - want32) <= 1e-4 * abs(want32)
    own = float(R.kl_diag(g["mu_kernel"], g["L_param"], g["D_param"], g["prior_mean"], g["prior_cov_D"])) / n     # the tests' own reference too
    assert abs(own - want64) <= 1e-9 * abs(want64)


def test_general_prior_kl_matches_distributions():
    from bayesian_torch_amd.layers._lowrank import general_kl
    g = R.load(R.case("b"))
    torch.manual_seed(3)
    pL = 0.1 * torch.randn(g["mu_kernel"].numel(), 1)
    got = general_kl(g["mu_kernel"], g["L_param"], g["D_param"], g["prior_mean"], pL, g["prior_cov_D"])
    want = R.kl_general(g["mu_kernel"], g["L_param"], g["D_param"], g["prior_mean"], pL, g["prior_cov_D"])
    assert abs(float(got) - float(want)) <= 1e-9 * abs(float(want))


def test_library_declares_and_exports_the_lowrank_entry_points():
    """include/bt_hip.h <-> _lib.EXPORTS <-> libbtorch_hip.so for the new entry points; argument validation is on the host."""
    from bayesian_torch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|const char \*)\s*\*?(bt_[a-z0-9_]+)\(", hdr, flags=re.M))
    new = {"bt_lowrank_conv2d_fwd", "bt_lowrank_mean", "bt_kl_lowrank", "bt_kl_lowrank_workspace"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(new):
        assert hasattr(handle, name), name
    assert re.search(r"#define BT_LOWRANK_MAX_R (\d+)", hdr).group(1) == str(_lib.LOWRANK_MAX_R)
    assert "4 = z" in hdr        # the z stream's tensor id is documented next to ids 0-3
    L = _lib.lib()
    geom = _lib.bt_conv2d_geom(2, 4, 6, 6, 8, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    rngc = _lib.bt_rng(0, None, 0, 1, 0, 0)
    one = ctypes.c_void_p(256)          # never dereferenced: every call below is refused before any launch
    fwd = lambda R_, Lp, d, ep=None: L.bt_lowrank_conv2d_fwd(ctypes.byref(geom), 1, one, 0, one, 0, Lp, R_, d, None, None, ctypes.byref(rngc), ep, one, None)
    assert fwd(5, one, 1e-10) == -1 and b"bt_lowrank_conv2d_fwd" in L.bt_last_error_string()
    assert fwd(-1, one, 1e-10) == -1 and fwd(2, None, 1e-10) == -1 and fwd(1, one, 0.0) == -1 and fwd(1, one, -1.0) == -1
    for ep in (_lib.bt_epilogue(None, None, None, 0, 1, 0), _lib.bt_epilogue(None, None, one, 0, 0, 0), _lib.bt_epilogue(None, None, None, 0, 0, 1)):
        assert fwd(1, one, 1e-10, ctypes.byref(ep)) == _lib.ERR_UNSUPPORTED
    assert L.bt_lowrank_mean(None, None, 1, 1, 1, None, None, None, None) == -1 and b"bt_lowrank_mean" in L.bt_last_error_string()
    assert L.bt_kl_lowrank(None, None, 1, 1, 1e-10, None, None, None, None, None, 0, None) == -1 and b"bt_kl_lowrank" in L.bt_last_error_string()
    assert L.bt_kl_lowrank(one, one, 10, 2, 1e-10, one, one, one, None, None, 0, None) == -3
    assert L.bt_kl_lowrank_workspace(432, 432) >= 8 * (432 * 432 * 2 + 4) and L.bt_kl_lowrank_workspace(10, 5000) == 0
    rf = lambda tid: L.bt_rng_normal_fill(ctypes.byref(rngc), tid, 1, 1, 4, 1, None, None)
    assert rf(5) == -1          # (ids 0..4 pass this check; the null output is refused either way, before any launch)
