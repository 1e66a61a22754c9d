"""GPU: the KL terms produced by the pack check (bt_pack_sync_kl) instead of the forward kernels' own sweep -- against the
reference goldens, against the fused sweep, after parameter writes a captured graph cannot see, and with forward outputs that
do not depend on where the KL was computed."""
import pytest
import torch

from conftest import assert_close, layer_tensors, load_golden

pytestmark = pytest.mark.gpu
PRIOR = {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "moped_enable": False, "moped_delta": 0.5}


def _cuda(t):
    return None if t is None else t.cuda()


def _sync_kl(g, force=True):
    """bt_pack_sync_kl on one fixture's parameters -> its KL term (0-dim device tensor)."""
    from bayesian_torch_amd import functional as F
    mu, rho = _cuda(g["mu_w"]), _cuda(g["rho_w"])
    Co, Ci = mu.shape[0], mu.shape[1]
    taps = mu[0, 0].numel()
    mp, sp, st = F.pack_buffers(Co, Ci, taps, mu.device)
    seg = dict(mu=mu, rho=rho, src_mu=None, src_rho=None, mu_packed=mp, sigma_packed=sp, state=st, Co=Co, Ci=Ci, taps=taps, force=force)
    out = torch.empty((), dtype=torch.float32, device=mu.device)
    kl = tuple(_cuda(g[k]) for k in ("prior_mu_w", "prior_sigma_w", "mu_b", "rho_b", "prior_mu_b", "prior_sigma_b")) + (out,)
    F.pack_sync([seg], owner="test_sync_kl", kls=[kl])
    return out


def _fused_kl(g):
    """The fixture's forward at one sample with its own draws (a leading sample axis of 1), KL swept by the forward kernel."""
    from bayesian_torch_amd import functional as F
    flip = "Flipout" in g["meta"]["cls"]
    st = lambda t: None if t is None else _cuda(t).unsqueeze(0)
    priors = tuple(_cuda(g[k]) for k in ("prior_mu_w", "prior_sigma_w", "prior_mu_b", "prior_sigma_b"))
    _, kl = F.fused_forward(_cuda(g["x"]), _cuda(g["mu_w"]), _cuda(g["rho_w"]), _cuda(g["mu_b"]), _cuda(g["rho_b"]), flip=flip, conv=g["conv"],
                            S=1, priors=priors, eps_w=st(g["eps_w"]), eps_b=st(g["eps_b"]), sign_in=st(g["sign_in"]) if flip else None,
                            sign_out=st(g["sign_out"]) if flip else None, want_kl=True)
    return kl


@pytest.mark.parametrize("name", ["linear_reparam_cfg1", "linear_reparam_k500", "linear_reparam_nobias", "linear_reparam_rprior",
                                  "linear_flipout_rprior", "linear_flipout_cfg1", "conv2d_reparam_c8x16k3s2", "conv2d_flipout_c3x8k3",
                                  "conv2d_reparam_c64x64k3hw1", "conv2d_reparam_c8x12g2"])
def test_sync_kl_matches_golden_and_fused_sweep(name):
    g = layer_tensors(load_golden(name))
    kl = _sync_kl(g)
    assert_close(kl.cpu(), g["kl"], 1e-5, 0, name + ".kl (pack check)")
    assert_close(kl.cpu(), _fused_kl(g).cpu(), 1e-6, 0, name + ".kl: pack check vs fused sweep")
    # deterministic: block partials summed in block order; clean parameters (no rebuild) give the same value
    assert torch.equal(_sync_kl(g, force=False), kl)


def _net(btype, width=64, seed=3):
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
    torch.manual_seed(seed)
    net = H.resnet18(10, width)
    dnn_to_bnn(net, dict(PRIOR, type=btype))
    H.fill_bayes_params(net, seed)
    return net.cuda().eval()


def test_model_sync_kl_matches_reference_golden():
    """Whole ResNet18 (Reparameterization) on on-chip draws: the summed KL of the layers equals the reference's get_kl_loss."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.mc import mc_forward
    g = load_golden("model_r18_reparam")
    meta = g["meta"]
    net = _net(meta["btype"], 64, meta["seed"])
    rng.set_mode("philox")
    x = torch.randn(*meta["x_shape"], generator=torch.Generator().manual_seed(meta["seed"] + 7)).cuda()
    _, kl = mc_forward(net, x, 2)
    assert_close(kl.cpu(), g["kl"], 1e-5, 0, "model_r18_reparam: kl from the pack check vs golden")
    assert not any(m._last["fused_kl"] for _, m in H.bayes_layers(net)), "every layer's KL should come from the pack check"


@pytest.mark.parametrize("btype", ["Reparameterization", "Flipout"])
def test_model_outputs_bit_identical_with_fused_kl(btype, monkeypatch):
    """The forward outputs do not depend on where the KL is computed; the KL agrees to double-accumulation rounding."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.layers import _fused
    from bayesian_torch_amd.mc import McGraph, mc_forward
    net = _net(btype, 16)
    rng.set_mode("philox")
    rng.manual_seed(11)
    x = torch.randn(8, 3, 32, 32, generator=torch.Generator().manual_seed(2)).cuda()
    c0 = rng.peek_call()
    logits, kl = mc_forward(net, x, 4)
    monkeypatch.setattr(_fused, "BT_FUSED_KL", True)
    rng.set_call(c0)
    logits_f, kl_f = mc_forward(net, x, 4)
    monkeypatch.setattr(_fused, "BT_FUSED_KL", False)
    assert torch.equal(logits, logits_f)
    assert_close(kl.cpu(), kl_f.cpu(), 1e-6, 0, btype + ": kl pack check vs fused sweep")
    # the captured graph carries the same KL
    g = McGraph(net, x, 4)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(g.kl, kl)


def test_graph_replay_kl_follows_data_writes():
    """A .data write the host cannot see: the next replay's KL is the KL of the new parameters (dirty path of the pack check)."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.mc import McGraph
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    net = _net("Reparameterization", 16)
    rng.set_mode("philox")
    x = torch.randn(8, 3, 32, 32, generator=torch.Generator().manual_seed(4)).cuda()
    g = McGraph(net, x, 2)
    g.replay()
    torch.cuda.synchronize()
    kl0 = g.kl.clone()
    with torch.no_grad():
        assert_close(kl0.cpu(), get_kl_loss(net).cpu(), 1e-6, 0, "replay kl vs get_kl_loss")
    layers = [m for _, m in H.bayes_layers(net)]
    layers[-2].mu_kernel.data.mul_(1.5)
    layers[-1].rho_bias.data.add_(0.25)
    g.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = get_kl_loss(net)
    assert not torch.equal(g.kl, kl0)
    assert_close(g.kl.cpu(), ref.cpu(), 1e-6, 0, "replay kl after .data writes vs get_kl_loss")


@pytest.mark.parametrize("cls", ["Conv2dReparameterization", "Conv2dFlipout", "LinearReparameterization"])
def test_layer_eager_sync_kl(cls, monkeypatch):
    """A layer called on its own checks its pack itself: the KL comes from that check, the output is the fused-sweep build's."""
    import bayesian_torch_amd.layers as L
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.layers import _fused
    torch.manual_seed(6)
    if cls.startswith("Conv"):
        m = getattr(L, cls)(16, 32, 3, padding=1).cuda()
        x = torch.randn(4, 16, 8, 8).cuda()
    else:
        m = getattr(L, cls)(96, 40).cuda()
        x = torch.randn(4, 96).cuda()
    m.prior_weight_mu.normal_(0, 0.1)
    rng.set_mode("philox")
    c0 = rng.peek_call()
    with torch.no_grad():
        out, kl = m(x)
        assert not m._last["fused_kl"]
        monkeypatch.setattr(_fused, "BT_FUSED_KL", True)
        rng.set_call(c0)
        out_f, kl_f = m(x)
        assert m._last["fused_kl"]
        monkeypatch.setattr(_fused, "BT_FUSED_KL", False)
        assert torch.equal(out, out_f)
        assert_close(kl.cpu(), kl_f.cpu(), 1e-6, 0, cls + ": kl pack check vs fused sweep")
        assert_close(kl.cpu(), m.kl_loss().cpu(), 1e-6, 0, cls + ": kl pack check vs kl_loss")
        m.mu_bias.data.add_(0.5)          # a write no version counter sees
        _, kl2 = m(x)
        assert_close(kl2.cpu(), m.kl_loss().cpu(), 1e-6, 0, cls + ": kl after a .data write")
        assert not torch.equal(kl2, kl)
