"""Chained same-shape 3x3 layers (bt_reparam_conv2d_chain_fwd, functional.fused_chain_forward, FusedBayesLayer.forward_chain): ONE launch
in which every workgroup walks the layers over its own images must give, bit for bit, what the same layers give one launch each at the
same call coordinates -- every member's output, not only the last.

Shapes. The chain needs the unchanged split_plan to give every member the 512-wide tile of whole images, and split_plan takes that
tile only when the launch has enough workgroups for a narrower tile to cost another round: with 8x8 maps and B = 13 / 16 (two 512-column
tiles per sample) that is S >= 73 for B = 16 and S >= 74 for B = 13 (its 128-wide tiles are 7 per sample: a third round from 74 on). So
the ragged-batch cases run twice: at S = 3, where the planner gives a narrower tile and the tests hold the DECLINE (nothing launched,
nothing returned) and, through the layer helper, the fallback's equality -- and at S = 74, the smallest S at which both batches chain,
where the test holds the equality and that the chain kernel really ran. C = 40 on 4x4 maps with B = 40 fills its two 512-column tiles to 62 %: split_plan
refuses that tile, the chain is declined, and the test holds the decline and the layers' one-by-one equality through the layer helper.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

CONV = dict(stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1)
S_CHAIN = 74      # see the module docstring


def _dev():
    return torch.device("cuda:0")


def _layers(n, C_, seed, bias=False):
    """n layers C_ -> C_ 3x3 with a folded BatchNorm (scale, shift) each; residuals as in basic blocks: the input, then member 1's out."""
    from bayesian_torch_amd import functional as F
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n):
        mu = (torch.randn(C_, C_, 3, 3, generator=g) * 0.05).to(_dev())
        rho = (torch.randn(C_, C_, 3, 3, generator=g) * 0.1 - 3.0).to(_dev())
        m = dict(mu_w=mu, rho_w=rho, conv=CONV, packed=F.pack_params(mu, rho), seed=1234, call=100 + k, layer_id=5 + k, sample0=0,
                 post_scale=(torch.rand(C_, generator=g) + 0.5).to(_dev()), post_shift=(torch.randn(C_, generator=g) * 0.1).to(_dev()), relu=True,
                 residual=[None, "input", None, 1][k % 4] if k < 4 else None)
        if bias:
            m["mu_b"], m["rho_b"] = (torch.randn(C_, generator=g) * 0.1).to(_dev()), (torch.randn(C_, generator=g) * 0.1 - 3.0).to(_dev())
        out.append(m)
    return out


def _one_by_one(x, members, S, shared_x):
    """The members as launches of their own at the same coordinates -> (outs, kernel names)."""
    from bayesian_torch_amd import _lib, functional as F
    outs, names, cur, sh = [], [], x, shared_x
    for m in members:
        res = m["residual"]
        res = x if res == "input" else outs[res] if isinstance(res, int) else res
        kw = {k: m[k] for k in ("conv", "packed", "seed", "call", "layer_id", "sample0", "post_scale", "post_shift", "relu")}
        out, _ = F.fused_forward(cur, m["mu_w"], m["rho_w"], m.get("mu_b"), m.get("rho_b"), S=S, shared_x=sh, residual=res, **kw)
        outs.append(out)
        names.append(_lib.lib().bt_last_kernel_name().decode())
        cur, sh = out, False
    return outs, names


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) and bool(torch.isfinite(p).all()) for p, q in zip(a, b))


_ref = {}


def _case(B, n=4, C_=64, H=8, S=S_CHAIN, shared=False, bias=False):
    """(x, members, the one-by-one outputs): computed once per shape and shared by the tests, never modified."""
    key = (B, n, C_, H, S, shared, bias)
    if key not in _ref:
        g = torch.Generator().manual_seed(B * 1000 + n)
        x = torch.randn((B if shared else S * B), C_, H, H, generator=g).to(_dev())
        members = _layers(n, C_, 11 * n + B, bias)
        outs, names = _one_by_one(x, members, S, shared)
        _ref[key] = (x, members, outs, names)
    return _ref[key]


def _chain_name(n, xm=3):
    return "fused_split_chain_kernel<64,512,bf16x3,6 terms,npw=4,xm=%d,n=%d>" % (xm, n)


@pytest.mark.parametrize("B", [13, 16])
def test_ragged_batch_chains_at_the_smallest_eligible_S(B):
    """B = 13: the second tile of every sample holds 5 images and 3 dead ones. Four members, residuals of two basic blocks."""
    from bayesian_torch_amd import _lib, functional as F
    x, members, want, names = _case(B)
    assert all(n_ == "fused_split_kernel<64,512,bf16x3,6 terms,npw=4,xm=3>" for n_ in names), names      # what the chain replaces
    got = F.fused_chain_forward(x, members, S=S_CHAIN, shared_x=False)
    assert got is not None, "the library declined an eligible chain"
    assert _lib.lib().bt_last_kernel_name().decode() == _chain_name(4)
    assert _lib.last_launch_info()["workgroups"] == 2 * S_CHAIN and _lib.last_launch_info()["t_NI"] == 8
    assert _same(got, want)


@pytest.mark.parametrize("B", [13, 16])
def test_ragged_batch_at_S_3_is_declined_with_nothing_launched(B):
    """S = 3: six workgroups of 512 columns -- split_plan takes a narrower tile, so there is no chain; the entry launches nothing."""
    from bayesian_torch_amd import _lib, functional as F
    x, members, want, names = _case(B, S=3)
    assert not any(",512," in n_ for n_ in names), names
    outs = [torch.full_like(w, float("nan")) for w in want]
    before = _lib.lib().bt_last_kernel_name().decode()
    assert F.fused_chain_forward(x, members, S=3, shared_x=False, outs=outs) is None
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs), "a declined chain wrote a result"
    assert _lib.lib().bt_last_kernel_name().decode() == before


def test_chain_of_two_and_a_shared_first_input_and_biases():
    from bayesian_torch_amd import _lib, functional as F
    x, members, want, _ = _case(16, n=2)
    got = F.fused_chain_forward(x, members, S=S_CHAIN, shared_x=False)
    assert got is not None and _lib.lib().bt_last_kernel_name().decode() == _chain_name(2) and _same(got, want)
    x, members, want, _ = _case(16, shared=True, bias=True)      # member 0 reads ONE batch for every sample; its residual user reads it too
    got = F.fused_chain_forward(x, members, S=S_CHAIN, shared_x=True)
    assert got is not None and _lib.lib().bt_last_kernel_name().decode() == _chain_name(4) and _same(got, want)


def test_external_residual_and_three_members():
    from bayesian_torch_amd import functional as F
    x, members, _, _ = _case(16)
    ext = torch.randn(S_CHAIN * 16, 64, 8, 8, generator=torch.Generator().manual_seed(3)).to(_dev())
    members = [dict(m) for m in members[:3]]
    members[2]["residual"] = ext
    want, _ = _one_by_one(x, members, S_CHAIN, False)
    got = F.fused_chain_forward(x, members, S=S_CHAIN, shared_x=False)
    assert got is not None and _same(got, want)


def test_chain_behind_dirty_lds():
    """LDS survives from kernel to kernel: the chain clears its weight buffers and zero pixels for EVERY member (the output staging of
    member k overwrites them), and reads nothing else it did not write."""
    from bayesian_torch_amd import _lib, functional as F
    L = _lib.lib()
    L.bt_debug_poison_lds.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.bt_debug_poison_lds.restype = ctypes.c_int
    word = torch.zeros(1, dtype=torch.int32, device=_dev())
    for B in (13, 16):
        x, members, want, _ = _case(B)
        assert L.bt_debug_poison_lds(word.data_ptr(), _lib.stream_ptr(word.device)) == 0
        got = F.fused_chain_forward(x, members, S=S_CHAIN, shared_x=False)
        assert got is not None and _same(got, want)


@pytest.mark.parametrize("off", [0, 1])
def test_guard_bands_around_every_out(off):
    """Every out inside NaN-pattern bands: nothing written outside, every element written. off = 1: input and outs 4 bytes past a 16-byte
    boundary -- the generic x fetch (xm 0) and the column read-out instead of the 16-byte forms, in the chain as in the single launches."""
    import _guard
    from bayesian_torch_amd import _lib, functional as F
    for B in (13, 16):
        x, members, want, _ = _case(B)
        xg = _guard.place(x, off)
        members = [dict(m) for m in members]
        if off:      # the members' own launches at the same misalignment
            with _guard.guarded_allocations(off):
                want, _ = _one_by_one(xg, members, S_CHAIN, False)
        with _guard.guarded_allocations(off) as log:
            got = F.fused_chain_forward(xg, members, S=S_CHAIN, shared_x=False)
        torch.cuda.synchronize()
        assert got is not None and _lib.lib().bt_last_kernel_name().decode() == _chain_name(4, 0 if off else 3)
        assert len(log) == 4
        _guard.check_all(log)
        assert _same(got, want)


# ---------------------------------------------------------------------------- the layer helper and the harness
class _Toy(torch.nn.Module):
    """A two-stage ResNet of basic blocks on 8x8 inputs: 3x3 stem, two identity blocks (the chain), a strided stage, the classifier."""

    def __init__(self, width):
        super().__init__()
        from bayesian_torch_amd.harness import resnet as H
        nn = torch.nn
        self.conv1, self.bn1 = nn.Conv2d(3, width, 3, 1, 1, bias=False), nn.BatchNorm2d(width)
        self.layer1 = nn.Sequential(H._Basic(width, width, 1, None), H._Basic(width, width, 1, None))
        short = nn.Sequential(nn.Conv2d(width, 2 * width, 1, 2, bias=False), nn.BatchNorm2d(2 * width))
        self.layer2 = nn.Sequential(H._Basic(width, 2 * width, 2, short), H._Basic(2 * width, 2 * width, 1, None))
        self.fc = nn.Linear(2 * width, 10)

    def forward(self, x):
        from bayesian_torch_amd.harness import resnet as H
        x = self.conv1(x)
        x = H.ResNet._run_stage(self.layer2, H.ResNet._run_stage(self.layer1, x))
        return self.fc(torch.flatten(x.mean((2, 3)), 1))


_models = {}


def _toy(width=64):
    if width not in _models:
        from bayesian_torch_amd import rng
        from bayesian_torch_amd.fuse import fold_pair
        from bayesian_torch_amd.harness import resnet as H
        from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn
        torch.manual_seed(0)
        net = _Toy(width)
        for m in net.modules():      # BatchNorms that do something
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1), m.running_var.uniform_(0.5, 1.5), m.weight.data.uniform_(0.5, 1.5), m.bias.data.normal_(0, 0.1)
        dnn_to_bnn(net, {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0, "type": "Reparameterization",
                         "moped_enable": False, "moped_delta": 0.5})
        H.fill_bayes_params(net, 3)
        net = net.to(_dev()).eval()
        fold_pair(net.conv1, net.bn1, relu=True)
        for stage in (net.layer1, net.layer2):
            for blk in stage:
                fold_pair(blk.conv1, blk.bn1, relu=True), fold_pair(blk.conv2, blk.bn2, relu=True)
                if blk.downsample is not None:
                    fold_pair(blk.downsample[0], blk.downsample[1], relu=False)
                    blk.downsample[1] = torch.nn.Identity()
                blk.fused = True
        rng.set_mode("philox")
        _models[width] = net
    return _models[width]


def _chain_convs(net):
    return [c for b in net.layer1 for c in (b.conv1, b.conv2)]


def _eager(net, x, S, call):
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.mc import mc_forward
    rng.set_call(call)
    logits, kl = mc_forward(net, x, S)
    return logits.clone(), kl.clone(), [dict(c._last) for c in _chain_convs(net)]


def test_model_chains_layer1_and_matches_the_unchained_model():
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.layers._fused import set_chain
    net = _toy()
    x = torch.randn(16, 3, 8, 8, generator=torch.Generator().manual_seed(1)).to(_dev())
    prev = set_chain(True)
    try:
        lo1, kl1, last1 = _eager(net, x, S_CHAIN, 5000)
        calls = rng.peek_call() - 5000
        draw1 = _chain_convs(net)[2].materialize_last_draw()
        set_chain(False)      # what BT_CHAIN=0 sets
        lo0, kl0, last0 = _eager(net, x, S_CHAIN, 5000)
        assert rng.peek_call() - 5000 == calls, "the chain consumed other call coordinates"
        draw0 = _chain_convs(net)[2].materialize_last_draw()
    finally:
        set_chain(prev)
    assert all(l["kernel"] == _chain_name(4) for l in last1), [l["kernel"] for l in last1]      # engaged: no silent fallback
    assert all(l["kernel"].startswith("fused_split_kernel<64,512,") for l in last0), [l["kernel"] for l in last0]
    assert torch.equal(lo1, lo0) and torch.equal(kl1, kl0) and bool(torch.isfinite(lo1).all())
    keys = {"rng", "S", "kernel", "launch", "shared_x", "residual", "fused_kl", "x_shape", "out_shape", "draw"}
    for a, b in zip(last1, last0):
        assert set(a) == keys == set(b)
        assert all(a[k] == b[k] for k in keys - {"kernel", "launch"}), (a, b)
        assert a["launch"]["workgroups"] == b["launch"]["workgroups"] and a["launch"]["t_NI"] == b["launch"]["t_NI"]
    assert torch.equal(draw1["eps_w"], draw0["eps_w"])


@pytest.mark.parametrize("B", [13, 16])
def test_ragged_batch_at_S_3_falls_back_through_the_helper(B):
    """The issue's shapes at S = 3 through the model: the helper asks, the library declines, the blocks run layer by layer -- the same
    coordinates, logits, KL and ``_last`` as with chaining off, and no chain kernel anywhere."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.layers._fused import set_chain
    net = _toy()
    x = torch.randn(B, 3, 8, 8, generator=torch.Generator().manual_seed(B)).to(_dev())
    prev = set_chain(True)
    try:
        got, klg, last = _eager(net, x, 3, 6000)
        calls = rng.peek_call() - 6000
        set_chain(False)
        ref, klr, last0 = _eager(net, x, 3, 6000)
        assert rng.peek_call() - 6000 == calls
    finally:
        set_chain(prev)
    assert not any("chain" in l["kernel"] for l in last), [l["kernel"] for l in last]
    assert torch.equal(got, ref) and torch.equal(klg, klr) and bool(torch.isfinite(got).all())
    assert all(a == b for a, b in zip(last, last0))


def test_member_with_a_forward_hook_falls_back():
    net = _toy()
    x = torch.randn(16, 3, 8, 8, generator=torch.Generator().manual_seed(1)).to(_dev())
    want, klw, _ = _eager(net, x, S_CHAIN, 5000)
    seen = []
    h = _chain_convs(net)[1].register_forward_hook(lambda mod, i, o: seen.append(tuple(o.shape)))
    try:
        got, klg, last = _eager(net, x, S_CHAIN, 5000)
    finally:
        h.remove()
    assert seen == [(S_CHAIN * 16, 64, 8, 8)]
    # the hooked member's block runs layer by layer (the hook saw its launch's output); the other block is still a run of its own: a chain of two
    assert [l["kernel"].split("<")[0] for l in last[:2]] == ["fused_split_kernel"] * 2, [l["kernel"] for l in last]
    assert all(l["kernel"] == _chain_name(2) for l in last[2:]), [l["kernel"] for l in last]
    assert torch.equal(got, want) and torch.equal(klg, klw)


def test_ragged_channels_are_declined_and_fall_back():
    """C = 40 on 4x4 maps, B = 40: two 512-column tiles filled to 62 % -- split_plan refuses the tile, so no chain; the helper passes, the
    blocks run one by one, and the model computes what it computes with chaining off."""
    from bayesian_torch_amd import functional as F
    from bayesian_torch_amd.layers._fused import set_chain
    x, members, want, names = _case(40, C_=40, H=4, S=3)
    assert not any("512" in n_ for n_ in names), names
    assert F.fused_chain_forward(x, members, S=3, shared_x=False) is None
    net = _toy(40)
    xi = torch.randn(40, 3, 4, 4, generator=torch.Generator().manual_seed(2)).to(_dev())
    got, klg, last = _eager(net, xi, 3, 7000)
    prev = set_chain(False)
    try:
        ref, klr, _ = _eager(net, xi, 3, 7000)
    finally:
        set_chain(prev)
    assert not any("chain" in l["kernel"] for l in last)
    assert torch.equal(got, ref) and torch.equal(klg, klr)


def test_graph_replays_equal_eager_at_the_same_coordinates():
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.mc import McGraph
    net = _toy()
    x = torch.randn(16, 3, 8, 8, generator=torch.Generator().manual_seed(4)).to(_dev())
    rng.set_call(9000)
    g = McGraph(net, x, S_CHAIN)
    assert all(c._last["kernel"] == _chain_name(4) for c in _chain_convs(net))
    for _ in range(3):
        c = rng.peek_call()
        logits, kl, _ = g.replay()
        logits, kl = logits.clone(), kl.clone()
        assert rng.peek_call() == c + g.calls_per_run
        want, klw, _ = _eager(net, x, S_CHAIN, c)
        assert rng.peek_call() == c + g.calls_per_run
        assert torch.equal(logits, want) and torch.equal(kl, klw)
