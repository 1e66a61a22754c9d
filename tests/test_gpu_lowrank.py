"""GPU: Conv2dReparameterization_Multivariate on the fused forward's low-rank weight source, the mean pre-pass and the KL kernels,
against the reference's recorded outputs (tests/golden/lowrank_*.npz) and a float64 CPU reference (tests/_lowrank_ref.py)."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

import _guard as G
import _lowrank_ref as R
from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL, ATOL = 1e-4, 1e-5       # the project's output tolerance (conftest.assert_close)
KL_RTOL = 1e-4


def _cls():
    from bayesian_torch_amd.layers.variational_layers.conv_variational import Conv2dReparameterization_Multivariate
    return Conv2dReparameterization_Multivariate


def _layer(tag):
    g = R.load(tag)
    m = _cls()(**g["meta"]["ctor"])
    m.load_state_dict({k: g[k] for k in ("mu_kernel", "L_param", "prior_mean", "prior_cov_L", "prior_cov_D")})
    return m.to(DEV), g


def _rel(a, b):
    a, b = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (a, b))
    return abs(a - b) / abs(b)


# ---------------------------------------------------------------------------- 1. goldens, injected draws
@pytest.mark.parametrize("tag", R.CASES)
def test_goldens_with_injected_draws(tag):
    m, g = _layer(tag)
    rank = g["meta"]["ctor"]["rank"]
    m.inject_draw = dict(z=g["z"][None].to(DEV), eps_w=g["eps"][None].to(DEV))
    with torch.no_grad():
        out, kl = m(g["x"].to(DEV))
    torch.cuda.synchronize()
    print(f"{tag}: kl {float(kl):.9g}  kl64 {float(g['kl64']):.15g} (rel {_rel(kl, g['kl64']):.2e})  reference fp32 {float(g['kl']):.9g} (rel {_rel(kl, g['kl']):.2e})  "
          f"max |out - golden| {float((out.cpu() - g['out']).abs().max()):.3e}  {m._last['kernel']}")
    assert m._last["path"] == R.expected_path(rank) and m._last["kl_path"] == "kernel" and m._last["reason"] is None
    assert "lowrank" in m._last["kernel"] and "inj=1" in m._last["kernel"] and m._last["S"] == 1
    assert m._last["kernel"].endswith(f"R={rank if rank <= R.MAX_R else 0}>")
    assert_close(out, g["out"], RTOL, ATOL, tag)
    assert kl.dim() == 0 and _rel(kl, g["kl64"]) <= KL_RTOL and _rel(kl, g["kl"]) <= KL_RTOL
    with torch.no_grad():
        total = m.kl_loss()      # un-normalised, from the parameters, on the KL kernels
    assert _rel(total, float(g["kl64"]) * m.weight_size) <= KL_RTOL and m.bad_pivots() == 0


def test_torch_mode_draws_z_then_eps_on_the_device():
    from bayesian_torch_amd import rng
    m, g = _layer(R.case("b"))
    rng.set_mode("torch")
    try:
        torch.manual_seed(17)
        with torch.no_grad():
            out, _ = m(g["x"].to(DEV))
        draw = m.materialize_last_draw()
    finally:
        rng.set_mode("philox")
    torch.manual_seed(17)
    z = torch.empty(3, device=DEV).normal_()
    eps = torch.empty(m.weight_size, device=DEV).normal_()
    assert torch.equal(draw["z"][0], z) and torch.equal(draw["eps_w"][0], eps) and "inj=1" in m._last["kernel"]
    ref = R.forward(g["x"], g["mu_kernel"], g["L_param"], g["D_param"], draw["z"].cpu(), draw["eps_w"].cpu(), g["meta"]["ctor"])
    assert_close(out, ref, RTOL, ATOL, "torch-mode draw")


# ---------------------------------------------------------------------------- 2. / 3. on-chip draws
@functools.lru_cache(maxsize=None)
def _onchip(tag, shared):
    """One S = 3 forward with on-chip draws, computed once and shared by the tests below: (layer, fixture, x, out, kl, draw, coords)."""
    from bayesian_torch_amd import mc, rng
    rng.set_mode("philox")
    torch.manual_seed(1234)
    m, g = _layer(tag)
    S, B = 3, g["x"].shape[0]
    x = g["x"].to(DEV) if shared else torch.cat([g["x"], 0.5 * g["x"], -g["x"]]).to(DEV)
    call0 = rng.peek_call()
    with torch.no_grad(), mc.mc_samples(S, B, sample0=5):
        out, kl = m(x)
    draw = m.materialize_last_draw()
    torch.cuda.synchronize()
    return m, g, x, out, kl, draw, call0, dict(m._last)


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("letter", "abcde")
def test_onchip_draws_against_fp64(letter, shared):
    from bayesian_torch_amd import mc
    m, g, x, out, kl, draw, call0, last = _onchip(R.case(letter), shared)
    rank = g["meta"]["ctor"]["rank"]
    assert last["path"] == R.expected_path(rank) and "inj=0" in last["kernel"] and last["S"] == 3 and last["shared_x"] is shared and last["draw"] is None
    assert tuple(draw["z"].shape) == (3, rank) and tuple(draw["eps_w"].shape) == (3, m.weight_size)
    z = draw["z"].cpu()
    for i in range(3):
        for j in range(i + 1, 3):
            assert not torch.equal(z[i], z[j])
    ref = R.forward(x.cpu(), g["mu_kernel"], g["L_param"], g["D_param"], z, draw["eps_w"].cpu(), g["meta"]["ctor"], shared)
    assert_close(out, ref, RTOL, ATOL, f"{letter} shared={shared}")
    want = float(R.kl_diag(g["mu_kernel"], g["L_param"], g["D_param"], g["prior_mean"], g["prior_cov_D"])) / m.weight_size
    assert _rel(kl, want) <= KL_RTOL and _rel(kl, g["kl64"]) <= KL_RTOL
    if shared:      # a second call draws afresh
        with torch.no_grad(), mc.mc_samples(3, x.shape[0], sample0=5):
            m(x)
        z2 = m.materialize_last_draw()["z"].cpu()
        assert not torch.equal(z2, z)


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("letter", "abcde")
def test_injected_equals_onchip_bit_for_bit(letter, shared):
    from bayesian_torch_amd import mc
    m, g, x, out, kl, draw, call0, last = _onchip(R.case(letter), shared)
    m.inject_draw = dict(z=draw["z"].clone(), eps_w=draw["eps_w"].clone())
    try:
        with torch.no_grad(), mc.mc_samples(3, g["x"].shape[0], sample0=5):
            out2, kl2 = m(x)
        assert "inj=1" in m._last["kernel"] and m._last["path"] == last["path"]
    finally:
        m.inject_draw = None
    assert torch.equal(out2, out) and torch.equal(kl2, kl)


@pytest.mark.parametrize("B,hw,S,why", [(2, 8, 1, "more than 32 output channels, more than 64 columns: the 64x128 tile"),
                                        (32, 16, 8, "a launch the planner gives a 256-column tile: planned again on 64x128")])
def test_wider_tiles_against_fp64(B, hw, S, why):
    """The third tile of the low-rank form, planned directly and through the re-plan; 40 output channels leave a partial channel tile."""
    from bayesian_torch_amd import mc, rng
    rng.set_mode("philox")
    torch.manual_seed(77)
    ctor = dict(in_channels=3, out_channels=40, kernel_size=3, padding=1, rank=2)
    m = _cls()(**ctor).to(DEV)
    x = torch.randn(B, 3, hw, hw, device=DEV)
    with torch.no_grad(), mc.mc_samples(S, B):
        out = m(x, return_kl=False)
    assert m._last["kernel"].startswith("fused_fwd_kernel<64,128,2,lowrank,conv,"), (why, m._last["kernel"])
    draw = m.materialize_last_draw()
    ref = R.forward(x.cpu(), m.mu_kernel.detach().cpu(), m.L_param.detach().cpu(), m.D_param, draw["z"].cpu(), draw["eps_w"].cpu(), ctor)
    assert_close(out, ref, RTOL, ATOL, why)


# ---------------------------------------------------------------------------- 4. pre-pass vs in-kernel
def test_prepass_matches_in_kernel_chain():
    """A rank-4 layer (in-kernel) and the same parameters as a rank-5 layer with a zero fifth column (pre-pass), z agreeing in its first
    four entries: the pre-pass runs the kernel's own chain (one rounding per operation, j ascending) and its fifth step adds a zero,
    so the outputs are the same bits."""
    m4, g = _layer(R.case("c"))
    ctor = dict(g["meta"]["ctor"], rank=5)
    m5 = _cls()(**ctor).to(DEV)
    with torch.no_grad():
        m5.mu_kernel.copy_(m4.mu_kernel)
        m5.L_param.zero_()
        m5.L_param[:, :4].copy_(m4.L_param)
    torch.manual_seed(7)
    S = 2
    z4, eps = torch.randn(S, 4, device=DEV), torch.randn(S, m4.weight_size, device=DEV)
    z5 = torch.cat([z4, torch.randn(S, 1, device=DEV)], 1)
    from bayesian_torch_amd import mc
    x = g["x"].to(DEV)
    outs = []
    for m, z in ((m4, z4), (m5, z5)):
        m.inject_draw = dict(z=z, eps_w=eps)
        with torch.no_grad(), mc.mc_samples(S, x.shape[0]):
            outs.append(m(x, return_kl=False))
    assert (m4._last["path"], m5._last["path"]) == ("in_kernel", "mean_prepass")
    assert_close(outs[1], outs[0], 1e-6, 1e-7, "pre-pass vs in-kernel")
    assert torch.equal(outs[1], outs[0])


# ---------------------------------------------------------------------------- 5. training path
def test_training_path_against_fp64_autograd():
    from bayesian_torch_amd import rng
    rng.set_mode("philox")
    torch.manual_seed(99)
    m, g = _layer(R.case("b"))
    ctor = g["meta"]["ctor"]
    x = g["x"].to(DEV).requires_grad_(True)
    call0 = rng.peek_call()
    out, kl = m(x)
    assert m._last["path"] == "materialised" and m._last["reason"] == "the call needs gradients"
    gy = torch.randn(out.shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    ((out * gy).sum() + kl).backward()
    draw = m.materialize_last_draw()
    # the fp64 CPU reference on the same draw
    xr = g["x"].double().requires_grad_(True)
    mur, Lr = g["mu_kernel"].double().requires_grad_(True), g["L_param"].double().requires_grad_(True)
    outr = R.forward(xr, mur, Lr, g["D_param"], draw["z"].cpu(), draw["eps_w"].cpu(), ctor)
    klr = R.kl_diag(mur, Lr, g["D_param"], g["prior_mean"], g["prior_cov_D"]) / m.weight_size
    ((outr * gy.cpu().double()).sum() + klr).backward()
    assert_close(out, outr, RTOL, ATOL, "out")
    assert_close(x.grad, xr.grad, 1e-4, 1e-5, "dL/dx")
    assert_close(m.mu_kernel.grad, mur.grad, 2e-4, 2e-5, "dL/dmu_kernel")
    assert_close(m.L_param.grad, Lr.grad, 2e-4, 2e-5, "dL/dL_param")
    assert _rel(kl, klr) <= KL_RTOL
    # the inference forward at the same coordinates makes the same draw on chip
    rng.set_call(call0)
    with torch.no_grad():
        out_inf, kl_inf = m(x.detach())
    assert m._last["path"] == "in_kernel"
    assert_close(out_inf, out, RTOL, ATOL, "inference forward at the training forward's coordinates")
    assert _rel(kl_inf, kl) <= KL_RTOL


# ---------------------------------------------------------------------------- 6. model level
class _Net(nn.Module):
    def __init__(self, bn=False):
        super().__init__()
        from bayesian_torch_amd.layers import LinearReparameterization
        M = _cls()
        self.conv1 = M(3, 16, 3, padding=1, rank=432)        # the full-rank stem: n = 432
        self.bn1 = nn.BatchNorm2d(16) if bn else nn.Identity()
        self.conv2 = M(16, 16, 3, stride=2, padding=1, rank=1)
        self.fc = LinearReparameterization(16, 10)

    def forward(self, x):
        x = torch.relu(self.bn1(self.conv1(x, return_kl=False)))
        x = torch.relu(self.conv2(x, return_kl=False))
        return self.fc(x.mean((2, 3)), return_kl=False)


def _net():
    from bayesian_torch_amd import rng
    rng.set_mode("philox")
    torch.manual_seed(21)
    net = _Net()
    rng.assign_layer_ids(net)
    return net.to(DEV).eval()


def test_model_mc_forward_equals_eager_samples_and_kl_sums():
    from bayesian_torch_amd import mc, rng
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    net = _net()
    x = torch.randn(4, 3, 8, 8, device=DEV)
    S = 3
    call0 = rng.peek_call()
    logits, kl = mc.mc_forward(net, x, S)
    assert rng.peek_call() - call0 == 3            # one call coordinate per layer forward
    assert net.conv1._last["path"] == "mean_prepass" and net.conv2._last["path"] == "in_kernel" and net.conv2._last["S"] == S
    for s in range(S):
        rng.set_call(call0)
        with torch.no_grad(), mc.mc_samples(1, x.shape[0], sample0=s):
            one = net(x)
        assert_close(logits[s], one, RTOL, ATOL, f"sample {s}")
    with torch.no_grad():
        h, k1 = net.conv1(x)
        h, k2 = net.conv2(torch.relu(h))
        _, k3 = net.fc(torch.relu(h).mean((2, 3)))
    assert _rel(kl, float(k1) + float(k2) + float(k3)) <= 1e-6
    with torch.no_grad():
        total = get_kl_loss(net)
        parts = float(net.conv1.kl_loss()) + float(net.conv2.kl_loss()) + float(net.fc.kl_loss())
    assert _rel(total, parts) <= 1e-6


def test_model_graph_replays_draw_afresh_and_keep_their_kl():
    from bayesian_torch_amd import mc
    net = _net()
    x = torch.randn(4, 3, 8, 8, device=DEV)
    graph = mc.McGraph(net, x, 3, epilogue=False)
    l1, k1, _ = graph.replay()
    l1, k1 = l1.clone(), k1.clone()
    l2, k2, _ = graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(l1, l2) and torch.equal(k1, k2) and bool(torch.isfinite(l2).all())
    _, kl = mc.mc_forward(net, x, 3)
    assert _rel(k2, kl) <= 1e-6


def test_fold_batchnorm_leaves_the_multivariate_layer_alone():
    from bayesian_torch_amd import fuse
    net = _Net(bn=True).eval()
    twin = copy.deepcopy(net)
    assert fuse.fold_batchnorm(twin) == 0 and fuse.fold_relu(twin) == 0
    assert isinstance(twin.bn1, nn.BatchNorm2d) and not hasattr(twin.conv1, "post_scale")
    assert list(twin.state_dict()) == list(net.state_dict())


# ---------------------------------------------------------------------------- 7. fallbacks
def test_nonuniform_d_takes_the_materialised_path():
    from bayesian_torch_amd import rng
    rng.set_mode("philox")
    torch.manual_seed(31)
    m, g = _layer(R.case("b"))
    D = 1e-4 * (1.0 + torch.rand(m.weight_size))
    m.D_param = D
    with torch.no_grad():
        out, kl = m(g["x"].to(DEV))
    assert m._last["path"] == "materialised" and m._last["kl_path"] == "materialised" and m._last["reason"] == "D_param is not one constant"
    draw = m.materialize_last_draw()
    ref = R.forward(g["x"], g["mu_kernel"], g["L_param"], D, draw["z"].cpu(), draw["eps_w"].cpu(), g["meta"]["ctor"])
    assert_close(out, ref, RTOL, ATOL, "non-uniform D")
    want = float(R.kl_diag(g["mu_kernel"], g["L_param"], D, g["prior_mean"], g["prior_cov_D"])) / m.weight_size
    assert _rel(kl, want) <= KL_RTOL


def test_lowrank_prior_takes_the_materialised_kl():
    from bayesian_torch_amd import rng
    rng.set_mode("philox")
    torch.manual_seed(32)
    m, g = _layer(R.case("b"))
    pL = 0.1 * torch.randn(m.weight_size, 1)
    m.prior_cov_L.copy_(pL.to(DEV))
    with torch.no_grad():
        out, kl = m(g["x"].to(DEV))
    assert m._last["path"] == "in_kernel" and m._last["kl_path"] == "materialised" and m._last["reason"] == "prior_cov_L is not zero"
    draw = m.materialize_last_draw()
    ref = R.forward(g["x"], g["mu_kernel"], g["L_param"], g["D_param"], draw["z"].cpu(), draw["eps_w"].cpu(), g["meta"]["ctor"])
    assert_close(out, ref, RTOL, ATOL, "low-rank prior: forward")
    want = float(R.kl_general(g["mu_kernel"], g["L_param"], g["D_param"], g["prior_mean"], pL, g["prior_cov_D"])) / m.weight_size
    assert _rel(kl, want) <= KL_RTOL


# ---------------------------------------------------------------------------- 8. guard bands
@pytest.mark.parametrize("letter", "cd")
def test_guard_bands(letter):
    """x, L, the mean and the draws as interior views between NaN bands, 4 bytes off a 16-byte boundary; the mean workspace of the pre-pass
    and the output inside pattern bands that must come back intact."""
    from bayesian_torch_amd import functional as F
    g = R.load(R.case(letter))
    ctor = g["meta"]["ctor"]
    rank, n = ctor["rank"], g["mu_kernel"].numel()
    k = ctor["kernel_size"]
    wshape = (ctor["out_channels"], ctor["in_channels"], k, k)
    conv = dict(stride=R.two(ctor.get("stride", 1)), padding=R.two(ctor.get("padding", 0)), dilation=(1, 1), groups=1)
    x, mu, L = (G.place(g[key].to(DEV), 1) for key in ("x", "mu_kernel", "L_param"))
    z, eps = G.place(g["z"][None].to(DEV), 1), G.place(g["eps"][None].to(DEV), 1)
    d = float(g["D_param"][0])
    with G.guarded_allocations(0) as log:
        if rank <= R.MAX_R:
            out = F.lowrank_conv2d(x, mu, L, d, wshape, conv, z=z, eps_w=eps)
        else:
            mean = F.lowrank_mean(mu, L, 1, z)
            out = F.lowrank_conv2d(x, mean, None, d, wshape, conv, eps_w=eps)
    torch.cuda.synchronize()
    assert len(log) == (1 if rank <= R.MAX_R else 2)
    G.check_all(log)
    assert_close(out, g["out"], RTOL, ATOL, f"guarded {letter}")
