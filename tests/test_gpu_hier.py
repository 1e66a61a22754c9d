"""GPU: the hierarchical (inverse-gamma hyper-prior) KL kernels and layers against the float64 oracle of tests/_hier_ref.py.
A. bt_kl_hier per element (one-element segments), as sums (one segment, 70 segments in two launches, a segment beyond the block cap);
B. bt_kl_hier_bwd per element, and segmented against single-tensor bit for bit;
C. the two layer classes on the reference's fixtures: KL values, an untouched forward, gradients, overwritten hyper-priors;
D. a two-layer model: mc_forward, get_kl_loss, McGraph.
Every limit is KL_FACTOR times what the fp32 yardstick of _hier_ref reaches on the same inputs; each test prints both figures."""
import numpy as np
import pytest
import torch
from torch import nn

import _hier_ref as R
from conftest import assert_close, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = range(len(R.ROWS))


def _dev(t):
    return {k: v.to(DEV) for k, v in t.items()}


def _seg(t):
    return tuple(t[k] for k in R.NAMES)


def _seq_sum32(v, groups=None):
    """The kernel's fp32 order: segments of one layer added in order, layers added in order (groups: one id per segment)."""
    v = np.asarray(v, dtype=np.float32)
    groups = list(range(len(v))) if groups is None else groups
    total = layer = np.float32(0)
    for j, x in enumerate(v):
        if j == 0 or groups[j] != groups[j - 1]:
            if j:
                total = np.float32(total + layer)
            layer = x
        else:
            layer = np.float32(layer + x)
    return np.float32(total + layer)


# ------------------------------------------------------------------------------------------------------------------ A. the value
@pytest.mark.parametrize("row", ROWS, ids=R.ROW_IDS)
def test_kl_per_element_matches_the_oracle(row):
    """Every element of the row as a one-element segment at an odd element offset of one buffer, 64 segments a launch."""
    from bayesian_torch_amd import _lib
    t, o = R.row(row), R.oracle(row)
    bufs = {}
    for k in R.NAMES:
        b = torch.full((2 * R.N + 2,), float("nan"), device=DEV)
        b[1:2 * R.N + 1:2] = t[k].to(DEV)
        bufs[k] = b
    segs = [tuple(bufs[k][2 * j + 1:2 * j + 2] for k in R.NAMES) for j in range(R.N)]
    _, per = _lib.kl_hier(segs, per_segment=True, owner="test_hier")
    assert bool(torch.isfinite(per).all())
    e = R.units(per, o["kl"], o["U"])
    j = int(e.argmax())
    print(f"kl per element {R.ROW_IDS[row]}: kernel {float(e.max()):.3f} units (worst at log_a {float(t['la'][j]):.3f} log_b {float(t['lb'][j]):.3f} rho {float(t['rho'][j]):.3f}) "
          f"| fp32 formula {o['ref32_err']:.3f} | limit {o['elem_limit']:.3f}")
    assert R.worst(e) <= o["elem_limit"]


def _hold_sum(tag, got, row, idx):
    ref, U, lim, e32 = R.sum_limit(row, idx)
    e = float(R.units(got, torch.tensor(ref, dtype=torch.float64), U))
    print(f"{tag}: kernel {e:.3f} units | fp32 formula {e32:.3f} | limit {lim:.3f}   (sum {ref:.9g}, U {U:.4g})")
    assert e <= lim, f"{tag}: {e:.3f} units > {lim:.3f}"


def test_kl_one_segment_is_deterministic_and_leaves_the_workspace_zeroed():
    from bayesian_torch_amd import _lib
    seg = _seg(_dev(R.row(0)))
    k1, per = _lib.kl_hier([seg], per_segment=True, owner="test_hier")
    k2 = _lib.kl_hier([seg], owner="test_hier")
    torch.cuda.synchronize()
    _hold_sum("row 0 as one segment", k1, 0, torch.arange(R.N))
    assert torch.equal(k1, k2) and torch.equal(k1, per[0])
    assert int(_lib.workspace("test_hier", seg[0].device).count_nonzero()) == 0


def test_kl_70_segments_two_launches():
    """Lengths around the thread, pass and block sizes; even segments 16-byte aligned (float4 body + scalar tail), odd ones at odd
    element offsets. Every segment against the oracle; the total is the fp32 sum of seg_out in launch order, bit for bit."""
    from bayesian_torch_amd import _lib
    t, segs = R.row(0), R.segments()
    v = {k: R.packed_views(t[k], segs, DEV) for k in R.NAMES}
    assert all(v[k][0].data_ptr() % 16 == 0 and v[k][1].data_ptr() % 8 == 4 for k in R.NAMES)
    launch = [tuple(v[k][j] for k in R.NAMES) for j in range(len(segs))]
    total, per = _lib.kl_hier(launch, per_segment=True, owner="test_hier")
    total2, per2 = _lib.kl_hier(launch, per_segment=True, owner="test_hier")
    torch.cuda.synchronize()
    assert torch.equal(total, total2) and torch.equal(per, per2)
    assert int(_lib.workspace("test_hier", per.device).count_nonzero()) == 0
    for j, (s, n) in enumerate(segs):
        _hold_sum(f"segment {j} [{s}, +{n})", per[j], 0, R.seg_index(s, n))
    p = per.cpu().numpy()
    assert np.float32(total.item()) == np.float32(_seq_sum32(p[:64]) + _seq_sum32(p[64:]))
    lids = [j // 2 for j in range(len(segs))]      # pairs of segments form a layer (64 is even: no pair straddles the launches)
    grouped = _lib.kl_hier(launch, layer_ids=lids, owner="test_hier")
    assert np.float32(grouped.item()) == np.float32(_seq_sum32(p[:64], lids[:64]) + _seq_sum32(p[64:], lids[64:]))


def test_kl_segment_beyond_the_block_cap():
    """2048 blocks of 4096 elements is the cap: one segment of 2048 * 4096 + 4097 elements (row 0 repeated) makes its blocks stride."""
    from bayesian_torch_amd import _lib
    n = 2048 * 4096 + 4097
    reps = -(-n // R.N)
    seg = tuple(v.repeat(reps)[:n].contiguous() for v in _seg(_dev(R.row(0))))
    k1 = _lib.kl_hier([seg], owner="test_hier")
    k2 = _lib.kl_hier([seg], owner="test_hier")
    torch.cuda.synchronize()
    assert torch.equal(k1, k2)
    _hold_sum(f"one segment of {n} elements", k1, 0, torch.arange(n) % R.N)


# ------------------------------------------------------------------------------------------------------------------ B. the gradient
def _g():
    return torch.tensor(R.G_UP, device=DEV)


@pytest.mark.parametrize("row", ROWS, ids=R.ROW_IDS)
def test_kl_backward_matches_fp64_autograd(row):
    from bayesian_torch_amd import functional as F
    t, go = R.row(row), R.grad_oracle(row)
    got = F.kl_hier_backward([_seg(_dev(t))], _g())[0]
    err = R.grad_errors(t, got, go["ref64"])
    print(f"kl_hier_backward {R.ROW_IDS[row]}: kernel " + ", ".join(f"{k} {err[k]:.3f}" for k in R.GRADS) + " | fp32 yardstick "
          + ", ".join(f"{k} {go['ref32_err'][k]:.3f}" for k in R.GRADS) + " (units of 2^-23 of the uncancelled size)")
    assert all(bool(torch.isfinite(x).all()) for x in got), "non-finite gradient where the float64 reference is finite"
    for k in R.GRADS:
        assert err[k] <= go["limits"][k], f"{k}: {err[k]:.3f} > {go['limits'][k]:.3f}"


@pytest.mark.parametrize("row", ROWS, ids=R.ROW_IDS)
def test_kl_backward_segmented_equals_single_tensor_bit_for_bit(row):
    from bayesian_torch_amd import functional as F
    t, segs = R.row(row), R.segments()
    whole = F.kl_hier_backward([_seg(_dev(t))], _g())[0]
    v = {k: R.packed_views(t[k], segs, DEV) for k in R.NAMES}
    launch = [tuple(v[k][j] for k in R.NAMES) for j in range(len(segs))]
    out = F.kl_hier_backward(launch, _g())
    assert len(out) == len(segs)
    for j, ((s, n), got) in enumerate(zip(segs, out)):
        idx = R.seg_index(s, n).to(DEV)
        for k, a, b in zip(R.GRADS, got, whole):
            assert a.shape == (n,) and torch.equal(a, b[idx]), f"segment {j} [{s}, +{n}) {k}: bits differ from the single-tensor launch"
    some = F.kl_hier_backward(launch[:3], _g(), needs=[(False, False, True, True), (False,) * 4, (True, False, False, False)])
    assert some[0][0] is None and some[0][1] is None and torch.equal(some[0][2], out[0][2]) and torch.equal(some[0][3], out[0][3])
    assert some[1] == (None,) * 4 and torch.equal(some[2][0], out[2][0]) and some[2][1:] == (None,) * 3


# ------------------------------------------------------------------------------------------------------------------ C. the layers
def _layers(g, plain_too=True):
    """The fixture's hierarchical layer and a plain Reparameterization layer with the same (mu, rho, bias) parameters and layer id."""
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.layers import Conv2dReparameterization, LinearReparameterization
    import bayesian_torch_amd.layers.variational_layers.hiearchial_variational_layers as M
    rng.set_mode("philox")
    m = g["meta"]
    hier = getattr(M, m["cls"])(**m["ctor"])
    plain = (LinearReparameterization if "Linear" in m["cls"] else Conv2dReparameterization)(**m["ctor"])
    with torch.no_grad():
        for k in m["parameters"]:
            getattr(hier, k).copy_(g[k])
            if not k.startswith("log_"):
                getattr(plain, k).copy_(g[k])
    setattr(hier, m["hypo"][0], g["a0"].clone())
    setattr(hier, m["hypo"][1], g["b0"].clone())
    hier.prior_weight_mu = g["prior_weight_mu"].clone()
    plain._layer_id = hier._layer_id
    return hier.to(DEV), plain.to(DEV)


def _kl_limit(g):
    """(kl_loss in float64, forward KL in float64, U, limit in units): KL_FACTOR times the error of the reference's recorded fp32
    value, at least 1 unit."""
    kl_loss, U, fwd = R.fixture_oracle(g)
    e_rec = abs(float(g["kl_loss"]) - kl_loss) / (R.UNIT * (1 + U))
    return kl_loss, fwd, U, max(1.0, R.KL_FACTOR * e_rec), e_rec


@pytest.mark.parametrize("name", R.FIXTURES)
def test_layer_kl_matches_the_oracle_and_the_forward_is_the_parents(name):
    from bayesian_torch_amd import rng
    g = load_golden(name)
    hier, plain = _layers(g)
    x = g["x"].to(DEV)
    kl_loss, fwd, U, lim, e_rec = _kl_limit(g)
    rng.manual_seed(7)
    call0 = rng.peek_call()
    with torch.no_grad():
        got_loss = hier.kl_loss()
        out, kl = hier(x)
        rng.set_call(call0)
        want = plain(x, return_kl=False)
    e1, e2 = abs(float(got_loss) - kl_loss) / (R.UNIT * (1 + U)), abs(float(kl) - fwd) / (R.UNIT * (1 + U))
    print(f"{name}: kl_loss {e1:.3f} units, forward KL {e2:.3f} units | the reference's recorded fp32 value {e_rec:.3f} | limit {lim:.3f} (+2 with a bias)")
    assert e1 <= lim
    assert e2 <= lim + (2.0 if "mu_bias" in g else 0.0)      # the bias's mean KL (the parent's kernel) and one more fp32 addition
    assert "mu_bias" in g or torch.equal(kl, got_loss)
    assert tuple(out.shape) == tuple(int(v) for v in g["out_shape"]) and torch.equal(out, want), "the forward is not the parent's"


@pytest.mark.parametrize("name", R.FIXTURES)
def test_layer_gradients(name):
    """loss = out.sum() + kl: log_a_q / log_b_q gradients are the oracle's KL gradients (limits: row 0 of _hier_ref, whose sweeps span
    the fixtures' values); mu / rho gradients are the plain layer's contraction gradients plus the oracle's KL gradients."""
    from bayesian_torch_amd import rng
    g = load_golden(name)
    hier, plain = _layers(g)
    x = g["x"].to(DEV)
    t = R.fixture_tensors(g)
    ref64 = R.grad_ref(t, torch.float64, g=1.0)
    rng.manual_seed(7)
    call0 = rng.peek_call()
    out, kl = hier(x)
    (out.sum() + kl).backward()
    rng.set_call(call0)
    want = plain(x, return_kl=False)
    want.sum().backward()
    assert torch.equal(out, want)
    w = "weight" if "mu_weight" in g else "kernel"
    got = (hier._w("mu").grad, hier._w("rho").grad, getattr(hier, "log_a_q_" + w).grad, getattr(hier, "log_b_q_" + w).grad)
    err = R.grad_errors(t, (ref64[0], ref64[1], got[2], got[3]), ref64, g=1.0)
    lim = R.grad_oracle(0)["limits"]
    print(f"{name}: dla {err['dla']:.3f} dlb {err['dlb']:.3f} units (limits {lim['dla']:.3f}, {lim['dlb']:.3f})")
    assert err["dla"] <= lim["dla"] and err["dlb"] <= lim["dlb"]
    shape = got[0].shape
    assert_close(got[0], plain._w("mu").grad.double().cpu() + ref64[0].reshape(shape), 2e-4, 2e-5, "dmu")
    assert_close(got[1], plain._w("rho").grad.double().cpu() + ref64[1].reshape(shape), 2e-4, 2e-5, "drho")
    if "mu_bias" in g:
        assert hier.mu_bias.grad is not None and hier.rho_bias.grad is not None
    # only what requires a gradient gets one
    for p in hier.parameters():
        p.grad = None
    hier._w("mu").requires_grad_(False)
    getattr(hier, "log_b_q_" + w).requires_grad_(False)
    hier.kl_loss().backward()
    assert hier._w("mu").grad is None and getattr(hier, "log_b_q_" + w).grad is None
    assert torch.equal(getattr(hier, "log_a_q_" + w).grad, got[2])


def test_overwritten_hyper_priors_and_prior_mean_are_read_at_every_call():
    g = load_golden("hier_lin_nobias")
    hier, _ = _layers(g)
    t = R.fixture_tensors(g)

    def check(tag):
        kl, U = R.kl_elements(t)
        ref, Us = float(kl.sum()), float(U.sum())
        with torch.no_grad():
            got = float(hier.kl_loss())
        e = abs(got - ref) / (R.UNIT * (1 + Us))
        e32 = abs(float(R.kl_fp32(t).sum()) - ref) / (R.UNIT * (1 + Us))
        print(f"{tag}: {e:.3f} units (fp32 formula {e32:.3f})")
        assert e <= max(1.0, R.KL_FACTOR * e32), tag
        return got

    k0 = check("as loaded")
    t["a0"] = 0.3 + 3 * torch.rand(5, 7, generator=torch.Generator().manual_seed(1))
    hier.prior_hypo_a_weight = t["a0"].clone()                      # a CPU tensor, as the reference's scripts assign it
    k1 = check("prior_hypo_a_weight <- CPU tensor")
    hier.prior_hypo_a_weight.mul_(1.5)                              # in place (the version counter moves)
    t["a0"] = t["a0"] * 1.5
    k2 = check("prior_hypo_a_weight *= 1.5 in place")
    t["pm"] = 0.2 * torch.randn(5, 7, generator=torch.Generator().manual_seed(2))
    hier.prior_weight_mu = t["pm"].clone()                          # CPU again
    k3 = check("prior_weight_mu <- CPU tensor")
    hier.prior_weight_mu = t["pm"].to(DEV)
    assert check("prior_weight_mu <- device tensor") == k3
    hier.prior_hypo_b_weight = torch.tensor(2.5)                    # anything that broadcasts to the weight
    t["b0"] = torch.full((5, 7), 2.5)
    k4 = check("prior_hypo_b_weight <- scalar tensor")
    hier.prior_hypo_b_weight = torch.linspace(0.5, 2, 7, device=DEV)
    t["b0"] = torch.linspace(0.5, 2, 7).expand(5, 7).contiguous()
    k5 = check("prior_hypo_b_weight <- a row")
    assert len({k0, k1, k2, k3, k4, k5}) == 6


# ------------------------------------------------------------------------------------------------------------------ D. a model
class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        import bayesian_torch_amd.layers.variational_layers.hiearchial_variational_layers as M
        self.conv = M.Conv2dReparameterizationHierarchical_Weightwise(4, 6, 3, padding=1, bias=False, prior_variance_hypo_a=1.5, prior_variance_hypo_b=0.7)
        self.fc = M.LinearReparameterizationHierarchical_Weightwise(6, 5)

    def forward(self, x):
        return self.fc(torch.relu(self.conv(x, return_kl=False)).mean((2, 3)), return_kl=False)


def _net():
    from bayesian_torch_amd import rng
    rng.set_mode("philox")
    torch.manual_seed(33)
    net = _Net()
    with torch.no_grad():
        for m in (net.conv, net.fc):
            w = m._wname
            getattr(m, "log_a_q_" + w).normal_(0, 0.5)
            getattr(m, "log_b_q_" + w).normal_(0, 0.5)
    rng.assign_layer_ids(net)
    return net.to(DEV).eval()


def test_model_mc_forward_get_kl_loss_and_graph_replay():
    from bayesian_torch_amd import mc, rng
    from bayesian_torch_amd.models.dnn_to_bnn import get_kl_loss
    net = _net()
    x = torch.randn(4, 4, 6, 6, device=DEV)
    S = 3
    rng.manual_seed(11)
    with torch.no_grad(), mc.mc_samples(S, x.shape[0], collect_kl=True) as ctx:
        mc.sync_model_packs(net, ctx)
        net(x)
        mc.join_packs(ctx)
    assert len(ctx.kls) == 2      # one KL per layer, whatever S
    call0 = rng.peek_call()
    logits, kl = mc.mc_forward(net, x, S)
    assert rng.peek_call() - call0 == 2 and tuple(logits.shape) == (S, 4, 5)
    with torch.no_grad():
        total = get_kl_loss(net)
        parts = (net.conv.kl_loss(), net.fc.kl_loss(), net.fc._bias_kl())
    assert torch.equal(ctx.kls[0], parts[0]) and torch.equal(ctx.kls[1], parts[1] + parts[2])
    assert float(total) == float(_seq_sum32([parts[0].item(), parts[1].item()]))      # two layers in one launch, added in fp32 in order
    # the same terms in another fp32 order: three roundings of at most 2^-24 of a partial sum each (the terms are positive here)
    assert min(float(p) for p in parts) > 0
    assert abs(float(kl) - (float(total) + float(parts[2]))) <= 2.0 ** -21 * float(kl)
    # under autograd: one launch each way for the model, the same bits as layer by layer
    get_kl_loss(net).backward()
    ga = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    assert set(ga) == {"conv.mu_kernel", "conv.rho_kernel", "conv.log_a_q_kernel", "conv.log_b_q_kernel", "fc.mu_weight", "fc.rho_weight",
                       "fc.log_a_q_weight", "fc.log_b_q_weight"}      # the Linear's bias is not in get_kl_loss, as in the reference
    net.zero_grad(set_to_none=True)
    (net.conv.kl_loss() + net.fc.kl_loss()).backward()
    for n, gv in ga.items():
        assert torch.equal(gv, dict(net.named_parameters())[n].grad), n
    net.zero_grad(set_to_none=True)
    # a captured graph replays mc_forward bit for bit at the same call coordinates
    graph = mc.McGraph(net, x, S, epilogue=False)
    c = rng.peek_call()
    l1, k1, _ = graph.replay()
    l1, k1 = l1.clone(), k1.clone()
    rng.set_call(c)
    l2, k2 = mc.mc_forward(net, x, S)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and torch.equal(k1, k2) and torch.equal(k1, kl)
