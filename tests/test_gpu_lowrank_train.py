"""GPU: Conv2dReparameterization_Multivariate trained on the fused backward kernels (``set_lowrank_train_path("fused")``;
csrc/bt_lowrank_bwd.hip) against float64 autograd of tests/_lowrank_ref.py on the same draws, against the materialised path at the same
coordinates, and the KL gradient kernel against the CPU closed form (tests/_lowrank_train.py, itself held to autograd in
tests/test_lowrank_train_host.py)."""
import pytest
import torch
import torch.nn as nn

import _guard as G
import _lowrank_ref as R
import _lowrank_train as T
from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL, ATOL = 1e-4, 1e-5        # out and dx (tests/test_gpu_lowrank.py::test_training_path_against_fp64_autograd)
P_RTOL, P_ATOL = 2e-4, 2e-5    # the parameter gradients (the same test)


@pytest.fixture(autouse=True)
def _fused_train_path():
    import bayesian_torch_amd.layers as BL
    from bayesian_torch_amd import rng
    rng.set_mode("philox")
    prev = BL.set_lowrank_train_path("fused")
    try:
        yield
    finally:
        BL.set_lowrank_train_path(prev)


def _cls():
    from bayesian_torch_amd.layers.variational_layers.conv_variational import Conv2dReparameterization_Multivariate
    return Conv2dReparameterization_Multivariate


def _layer(tag):
    g = R.load(tag)
    m = _cls()(**g["meta"]["ctor"])
    m.load_state_dict({k: g[k] for k in ("mu_kernel", "L_param", "prior_mean", "prior_cov_L", "prior_cov_D")})
    return m.to(DEV), g


def _gy(shape, seed=1):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _grads(m, x):
    return dict(dx=None if x.grad is None else x.grad.clone(), dmu=m.mu_kernel.grad.clone(), dL=m.L_param.grad.clone())


def _zero(m, x):
    m.mu_kernel.grad = m.L_param.grad = None
    x.grad = None


def _hold(got, out, ref, what):
    assert_close(out, ref["out"], RTOL, ATOL, f"{what}: out")
    assert_close(got["dx"], ref["dx"], RTOL, ATOL, f"{what}: dL/dx")
    assert_close(got["dmu"], ref["dmu"], P_RTOL, P_ATOL, f"{what}: dL/dmu_kernel")
    assert_close(got["dL"], ref["dL"], P_RTOL, P_ATOL, f"{what}: dL/dL_param")


# ---------------------------------------------------------------------------- 1. all goldens, supplied draws, S = 1
@pytest.mark.parametrize("tag", R.CASES)
def test_goldens_with_supplied_draws(tag):
    m, g = _layer(tag)
    rank = g["meta"]["ctor"]["rank"]
    z, eps = g["z"][None].to(DEV), g["eps"][None].to(DEV)
    m.inject_draw = dict(z=z, eps_w=eps)
    x = g["x"].to(DEV).requires_grad_(True)
    out, kl = m(x)
    assert m._last["path"] == R.expected_path(rank) and m._last["backward"] == "fused"      # (fails without the feature: "materialised")
    assert m._last["kl_path"] == "kernel" and m._last["reason"] is None and "lowrank" in m._last["kernel"] and "inj=1" in m._last["kernel"]
    gy = _gy(out.shape)
    ((out * gy).sum() + kl).backward()
    torch.cuda.synchronize()
    ref = T.reference(g, x, z, eps, gy)
    _hold(_grads(m, x), out, ref, tag)
    assert abs(float(kl.detach()) - float(ref["kl"])) <= 1e-4 * abs(float(ref["kl"])) and m.bad_pivots() == 0
    rec = m._last["backward_launch"]
    assert rec["dgrad_launches"] >= 1 and rec["wgrad_launches"] >= 1 and rec["finish_launches"] == 1


# ---------------------------------------------------------------------------- 2. on-chip draws
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("letter", "bd")
def test_onchip_draws(letter, S, shared):
    from bayesian_torch_amd import mc, rng
    m, g = _layer(R.case(letter))
    B = g["x"].shape[0]
    xs = g["x"] if shared or S == 1 else torch.cat([g["x"], 0.5 * g["x"], -g["x"]])
    x = xs.to(DEV).requires_grad_(True)
    call0 = rng.peek_call()

    def step():
        _zero(m, x)
        rng.set_call(call0)
        with mc.mc_samples(S, B, sample0=5):
            out, kl = m(x)
        ((out * gy).sum() + kl).backward()
        return out.detach().clone(), _grads(m, x)

    gy = _gy((S * B,) + tuple(g["out"].shape[1:]))
    out, got = step()
    assert m._last["backward"] == "fused" and m._last["draw"] is None and "inj=0" in m._last["kernel"] and m._last["S"] == S
    assert m._last["shared_x"] is (shared or S == 1)
    draw = m.materialize_last_draw()
    torch.cuda.synchronize()
    ref = T.reference(g, x, draw["z"], draw["eps_w"], gy, shared=shared or S == 1)
    _hold(got, out, ref, f"{letter} S={S} shared={shared}")
    # a second run at the same coordinates: the same bits
    out2, got2 = step()
    assert torch.equal(out2, out) and all(torch.equal(got2[k], got[k]) for k in got)
    # the same draws supplied: the same bits
    m.inject_draw = dict(z=draw["z"].clone(), eps_w=draw["eps_w"].clone())
    out3, got3 = step()
    assert "inj=1" in m._last["kernel"] and m._last["backward"] == "fused"
    assert torch.equal(out3, out)
    for k in got:
        assert torch.equal(got3[k], got[k]), f"{k}: supplied draws against on-chip draws, max |diff| {float((got3[k] - got[k]).abs().max()):.3e}"


# ---------------------------------------------------------------------------- 3. fused against materialised
@pytest.mark.parametrize("letter", "bd")
def test_fused_and_materialised_agree_with_fp64(letter):
    import bayesian_torch_amd.layers as BL
    from bayesian_torch_amd import mc, rng
    m, g = _layer(R.case(letter))
    S, B = 2, g["x"].shape[0]
    x = g["x"].to(DEV).requires_grad_(True)
    gy = _gy((S * B,) + tuple(g["out"].shape[1:]))
    call0 = rng.peek_call()
    ref = None
    for path in ("fused", "materialised"):
        BL.set_lowrank_train_path(path)
        _zero(m, x)
        rng.set_call(call0)
        with mc.mc_samples(S, B, sample0=2):
            out, kl = m(x)
        ((out * gy).sum() + kl).backward()
        assert m._last["backward"] == ("fused" if path == "fused" else "autograd")
        assert m._last["path"] == (R.expected_path(g["meta"]["ctor"]["rank"]) if path == "fused" else "materialised")
        draw = m.materialize_last_draw()
        torch.cuda.synchronize()
        if ref is None:
            ref, z0 = T.reference(g, x, draw["z"], draw["eps_w"], gy), draw["z"].clone()
        else:
            assert torch.equal(draw["z"], z0)      # the same coordinates, the same draws
        _hold(_grads(m, x), out, ref, f"{letter} {path}")


# ---------------------------------------------------------------------------- 4. the KL gradient on its own
@pytest.mark.parametrize("tag", R.CASES)
def test_kl_gradient_against_the_closed_form(tag):
    """Un-normalised: |err| <= 1e-4 |ref| + 1e-6 max|ref| per element (the kernel is fp64 with an fp32 result)."""
    m, g = _layer(tag)
    kl = m.kl_loss()
    assert kl.requires_grad
    kl.backward()
    torch.cuda.synchronize()
    dmu, dL = T.kl_grad_closed_form(g["mu_kernel"], g["L_param"], g["D_param"], g["prior_mean"], g["prior_cov_D"])
    for name, got, want in (("dmu", m.mu_kernel.grad, dmu), ("dL", m.L_param.grad, dL)):
        err = (got.cpu().double() - want).abs()
        print(f"{tag} {name}: max |err| {float(err.max()):.3e}, max |ref| {float(want.abs().max()):.3e}")
        assert_close(got, want, 1e-4, 1e-6, f"{tag}: KL {name}")
    want = float(R.kl_diag(g["mu_kernel"], g["L_param"], g["D_param"], g["prior_mean"], g["prior_cov_D"]))
    assert abs(float(kl.detach()) - want) <= 1e-4 * abs(want) and m.bad_pivots() == 0
    # an upstream factor is a device scalar: the gradient scales with it
    m.mu_kernel.grad = m.L_param.grad = None
    (0.25 * m.kl_loss()).backward()
    assert_close(m.L_param.grad, 0.25 * dL, 1e-4, 1e-6, f"{tag}: 0.25 KL dL")
    assert_close(m.mu_kernel.grad, 0.25 * dmu, 1e-4, 1e-6, f"{tag}: 0.25 KL dmu")


def test_a_pivot_that_is_not_positive_gives_nan_gradients_and_is_counted():
    m, g = _layer(R.case("b"))
    with torch.no_grad():
        m.L_param[0, 0] = float("nan")      # I + L^T L / d is positive definite for any finite L: only a NaN reaches the refusal
    kl = m.kl_loss()
    kl.backward()
    torch.cuda.synchronize()
    assert bool(torch.isnan(kl)) and bool(torch.isnan(m.mu_kernel.grad).all()) and bool(torch.isnan(m.L_param.grad).all())
    assert m.bad_pivots() == 2      # the forward's factorisation and the backward's


# ---------------------------------------------------------------------------- 5. a tile-crossing geometry
def test_tile_crossing_geometry_against_fp64():
    """Ci = 68, Co = 70, 3 x 3, 10 x 10, B = 3: M = 300 (no multiple of 64 nor of the 16-step stage), two channel tiles with a tail on
    both axes, and by bwd_plan's rules three chunks of wgrad's reduction and three pieces of dgrad's output channels."""
    from bayesian_torch_amd import mc
    torch.manual_seed(5)
    ctor = dict(in_channels=68, out_channels=70, kernel_size=3, padding=1, rank=2)
    m = _cls()(**ctor).to(DEV)
    S, B = 2, 3
    x = torch.randn(B, 68, 10, 10).to(DEV).requires_grad_(True)
    gy = _gy((S * B, 70, 10, 10))
    with mc.mc_samples(S, B, sample0=1):
        out, kl = m(x)
    ((out * gy).sum() + kl).backward()
    rec = m._last["backward_launch"]
    assert m._last["path"] == "in_kernel" and m._last["backward"] == "fused"
    assert rec["wgrad_chunks"] > 1 and rec["dgrad_pieces"] > 1 and rec["wgrad_launches"] == 2 and rec["dgrad_launches"] == 2, rec
    assert (rec["dgrid_x"], rec["dgrid_y"], rec["wgrid_y"]) == (5, 2, 2) and rec["wgrid_z"] == S * rec["wgrad_chunks"] and rec["dgrid_z"] == S * rec["dgrad_pieces"]
    draw = m.materialize_last_draw()
    torch.cuda.synchronize()
    g = dict(mu_kernel=m.mu_kernel.detach().cpu(), L_param=m.L_param.detach().cpu(), D_param=m.D_param.cpu(), prior_mean=m.prior_mean.cpu(),
             prior_cov_D=m.prior_cov_D.cpu(), meta=dict(ctor=ctor))
    ref = T.reference(g, x, draw["z"], draw["eps_w"], gy)
    _hold(_grads(m, x), out, ref, "tile-crossing")


# ---------------------------------------------------------------------------- 6. selective gradients
def test_gradients_nobody_asked_for_are_not_computed():
    m, g = _layer(R.case("b"))
    gy = _gy(g["out"].shape)
    x = g["x"].to(DEV)                                       # a leaf input without grad: no dgrad launch
    out, kl = m(x)
    ((out * gy).sum() + kl).backward()
    rec = dict(m._last["backward_launch"])
    assert m._last["backward"] == "fused" and rec["dgrad_launches"] == 0 and rec["wgrad_launches"] >= 1 and rec["finish_launches"] == 1 and x.grad is None
    assert m.mu_kernel.grad is not None and m.L_param.grad is not None
    m.mu_kernel.grad = m.L_param.grad = None
    m.mu_kernel.requires_grad_(False), m.L_param.requires_grad_(False)      # frozen parameters: no wgrad launch, no finishing pass
    x = g["x"].to(DEV).requires_grad_(True)
    out, kl = m(x)
    ((out * gy).sum() + kl).backward()
    rec = dict(m._last["backward_launch"])
    assert m._last["backward"] == "fused" and rec["dgrad_launches"] >= 1 and rec["wgrad_launches"] == 0 and rec["finish_launches"] == 0
    assert x.grad is not None and m.mu_kernel.grad is None and m.L_param.grad is None


# ---------------------------------------------------------------------------- 7. guard bands
@pytest.mark.parametrize("letter", "be")
def test_guard_bands(letter):
    """Operands as interior views between NaN bands, 4 bytes off a 16-byte boundary; dx, the per-sample weight gradient, dmu, dL, the
    recomputed pre-pass and the workspaces inside pattern bands that must come back intact, every fp32 element written."""
    from bayesian_torch_amd import functional as F
    g = R.load(R.case(letter))
    ctor = g["meta"]["ctor"]
    rank, n, k = ctor["rank"], g["mu_kernel"].numel(), ctor["kernel_size"]
    wshape = (ctor["out_channels"], ctor["in_channels"], k, k)
    conv = dict(stride=R.two(ctor.get("stride", 1)), padding=R.two(ctor.get("padding", 0)), dilation=(1, 1), groups=1)
    x, mu, L = (G.place(g[key].to(DEV), 1) for key in ("x", "mu_kernel", "L_param"))
    pm, pv = G.place(g["prior_mean"].to(DEV), 1), G.place(g["prior_cov_D"].to(DEV), 1)
    z, eps = G.place(g["z"][None].to(DEV), 1), G.place(g["eps"][None].to(DEV), 1)
    gy = G.place(_gy(g["out"].shape), 1)
    c = G.place(torch.tensor([1.0 / n], device=DEV), 1)
    d = float(g["D_param"][0])
    with G.guarded_allocations(0) as log:
        if rank <= R.MAX_R:
            dx, dw, _ = F.lowrank_backward(x, gy, mu, L, d, wshape, conv, z=z, eps_w=eps)
        else:
            mean = F.lowrank_mean(mu, L, 1, z)
            dx, dw, _ = F.lowrank_backward(x, gy, mean, None, d, wshape, conv, eps_w=eps)
        dmu, dL = F.lowrank_wgrad_finish(dw, rank, z)
        kmu, kL = F.kl_lowrank_backward(mu, L, d, pm, pv, c)
    torch.cuda.synchronize()
    assert len(log) == (8 if rank <= R.MAX_R else 9)      # dx, dw, workspace, (mean,) dmu, dL, KL workspace, KL dmu, KL dL
    G.check_all(log)
    ref = T.reference(g, g["x"], g["z"][None], g["eps"][None], gy)
    assert_close(dx, ref["dx"], RTOL, ATOL, f"guarded {letter}: dx")
    assert_close(dmu + kmu, ref["dmu"], P_RTOL, P_ATOL, f"guarded {letter}: dmu")
    assert_close(dL + kL, ref["dL"], P_RTOL, P_ATOL, f"guarded {letter}: dL")


# ---------------------------------------------------------------------------- 8. a training smoke
class _Net(nn.Module):
    """tests/test_gpu_lowrank.py's small model: the full-rank stem (pre-pass), a rank-1 strided conv (in-kernel), a Linear head."""

    def __init__(self):
        super().__init__()
        from bayesian_torch_amd.layers import LinearReparameterization
        M = _cls()
        self.conv1 = M(3, 16, 3, padding=1, rank=432)
        self.conv2 = M(16, 16, 3, stride=2, padding=1, rank=1)
        self.fc = LinearReparameterization(16, 10)

    def forward(self, x):
        x, k1 = self.conv1(x)
        x, k2 = self.conv2(torch.relu(x))
        x, k3 = self.fc(torch.relu(x).mean((2, 3)))
        return x, k1 + k2 + k3


def test_three_sgd_steps_fused_against_materialised():
    import bayesian_torch_amd.layers as BL
    from bayesian_torch_amd import rng
    x = torch.randn(4, 3, 8, 8, generator=torch.Generator().manual_seed(3)).to(DEV)
    y = torch.tensor([1, 7, 3, 0], device=DEV)
    call0 = rng.peek_call()
    params = {}
    for path in ("fused", "materialised"):
        BL.set_lowrank_train_path(path)
        torch.manual_seed(21)
        net = _Net()
        rng.assign_layer_ids(net)
        net = net.to(DEV)
        opt = torch.optim.SGD(net.parameters(), lr=0.05)
        rng.set_call(call0)
        for _ in range(3):
            opt.zero_grad()
            logits, kl = net(x)
            (nn.functional.cross_entropy(logits, y) + kl / x.shape[0]).backward()
            opt.step()
        want = "fused" if path == "fused" else "autograd"
        assert net.conv1._last["backward"] == want and net.conv2._last["backward"] == want
        assert (net.conv1._last["path"], net.conv2._last["path"]) == (("mean_prepass", "in_kernel") if path == "fused" else ("materialised", "materialised"))
        params[path] = {k: v.detach().clone() for k, v in net.named_parameters()}
        assert all(bool(torch.isfinite(v).all()) for v in params[path].values())
    for k, v in params["fused"].items():
        assert_close(v, params["materialised"][k], P_RTOL, P_ATOL, f"after three steps: {k}")
