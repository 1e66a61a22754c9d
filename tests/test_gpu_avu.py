"""GPU: the AvUC losses (csrc/bt_avu.hip behind bayesian_torch_amd/utils/avuc_loss.py) against the float64 oracle of tests/_avu_ref.py,
under its tolerance rule: every error against the oracle, a kernel may reach 8 x the fp32 reference's own error on the same measure,
pooled over the group (the fixtures' ``meta`` holds the figures; each test prints the kernel's beside them).  Every test first asserts
the rule's classification precondition on the CPU.
1. the [B, C] cases, T = 1 (AvULoss) and T = 21 (AUAvULoss): loss, v, sums, gradient; counts, pred exactly;  2. the MC form, both types;
3. a threshold equal to one row's u;  4. odd operand offsets inside guard bands, and the same bits from run to run;  5. forward and
backward captured in one graph and replayed on new logits and a new threshold tensor;  6. mc.TrainGraph with the loss in ``loss_fn``."""
import numpy as np
import pytest
import torch

import _avu_ref as R
import _guard as G

pytestmark = pytest.mark.gpu


def _precondition(z, y, ut, T, th):
    ok, g, need = R.gap_ok(z, y, ut, T, th)
    assert ok, f"precondition: a row lies {g:.3e} from a threshold, {need:.3e} needed"


def _through_module(z, y, ut, T, th):
    """The public classes with autograd -> (dict of the rule's measures, last_stats)."""
    from bayesian_torch_amd.utils.avuc_loss import AvULoss, AUAvULoss
    zg = z.cuda().requires_grad_()
    if T == 1:
        mod = AvULoss(beta=R.BETA)
        loss = mod(zg, y.cuda(), float(th), type=ut)
        v = None
    else:
        mod = AUAvULoss(beta=R.BETA)
        loss, v = mod(zg, y.cuda(), type=ut)
        assert v.shape == (1,) and not v.requires_grad
    assert loss.shape == (1,) and loss.requires_grad
    loss.backward()
    st = mod.last_stats
    assert all(t.is_cuda for t in st.values())
    sums = st["sums"]
    if v is None:     # AvULoss returns the loss alone: AvU from the sums it reports
        s = sums[0].double()
        v = (s[0] + s[3]) / (s.sum() + R.EPS)
    return dict(loss=loss.detach(), v=v, sums=sums, grad=zg.grad), st


def _hold(label, z, y, ut, T, th, meta, group):
    o = R.evaluate(z, y, ut, T, th)
    got, st = _through_module(z, y, ut, T, th)
    torch.cuda.synchronize()
    assert torch.isfinite(got["grad"]).all() and got["grad"].shape == z.shape
    assert np.array_equal(st["counts"].cpu().numpy(), o["counts"].numpy().astype(np.int32)), (label, st["counts"].cpu(), o["counts"])
    assert np.array_equal(st["pred"].cpu().numpy(), o["pred"].numpy().astype(np.int32)), label
    assert np.array_equal(st["acc"].cpu().numpy(), (o["pred"] == y).numpy().astype(np.int32)), label
    thr = st["thresholds"].cpu()
    assert thr.dtype == torch.float64 and thr.shape == (T,)
    if T == 21:       # the end thresholds are the batch's smallest and largest u exactly
        u = st["uncertainty"].cpu().double()
        assert float(thr[0]) == float(u.min()) and float(thr[-1]) == float(u.max()) and bool((thr[1:] >= thr[:-1]).all())
        assert int(st["counts"][-1, 1] + st["counts"][-1, 3]) == 0 and int(st["counts"][0, 0] + st["counts"][0, 2]) >= 1
    else:
        assert float(thr[0]) == float(np.float32(th))
    return R.hold(label, got, o, meta, group), got, o


@pytest.mark.parametrize("tag", list(R.BC_CASES))
def test_bc_cases_against_the_oracle(tag):
    d = R.load(tag)
    z, y, th = torch.from_numpy(d["z"]), torch.from_numpy(d["y"]), d["th"]
    for T in (1, 21):
        _precondition(z, y, 0, T, th)
    for T in (1, 21):
        _, got, o = _hold(f"{tag} T={T}", z, y, 0, T, th, d["meta"], R.bc_group(tag, T))
        if tag == "b1c3_inacc":      # inaccurate and certain: v = 0, the loss is -beta log(1e-10), the gradient finite
            assert float(got["v"]) == 0.0 and abs(float(got["loss"]) + R.BETA * np.log(1e-10)) <= R.limit(d["meta"], R.bc_group(tag, T), "loss")


@pytest.mark.parametrize("ut", [0, 1])
@pytest.mark.parametrize("tag", list(R.MC_CASES))
def test_mc_cases_against_the_oracle(tag, ut):
    d = R.load(f"mc_{tag}")
    z, y, th = torch.from_numpy(d["z"]), torch.from_numpy(d["y"]), d[f"th_type{ut}"]
    for T in (1, 21):
        _precondition(z, y, ut, T, th)
    for T in (1, 21):
        _hold(f"mc {tag} type={ut} T={T}", z, y, ut, T, th, d["meta"], f"mc_type{ut}")


def test_threshold_equal_to_a_rows_uncertainty_classifies_it_certain():
    """The threshold is the device value of one row's u from a first call's last_stats (never read on the host): that row, and every
    row below it, is certain; the rows above are not."""
    from bayesian_torch_amd.utils.avuc_loss import AvULoss
    d = R.load("b67c10")
    z, y = torch.from_numpy(d["z"]).cuda(), torch.from_numpy(d["y"]).cuda()
    _precondition(z, y, 0, 1, d["th"])
    mod = AvULoss()
    mod(z, y, d["th"])
    u = mod.last_stats["uncertainty"].clone()
    k = int(R.evaluate(z, y, 0, 1, d["th"])["u"].argsort()[30])      # a row of middle rank (from the CPU oracle)
    mod(z, y, u[k])
    st = mod.last_stats
    torch.cuda.synchronize()
    assert torch.equal(st["uncertainty"], u)
    fc = st["first_certain"].cpu()
    n = int((u <= u[k]).sum())
    assert int(fc[k]) == 0 and 1 < n < 67
    assert torch.equal(fc == 0, (u <= u[k]).cpu()) and torch.equal(fc == 1, (u > u[k]).cpu())
    assert int(st["counts"][0, 0] + st["counts"][0, 2]) == n and int(st["counts"].sum()) == 67
    assert float(st["thresholds"][0]) == float(u[k])


def _functional(z, y, ut, T, th, off=None):
    """avu_forward + avu_backward on [S, B, C] logits; ``off``: operands at that fp32 element offset, every allocation of the two
    calls (results and workspace) inside guard bands -> the results as CPU tensors."""
    from bayesian_torch_amd import functional as F
    z, y = z.cuda(), y.cuda()
    th = torch.tensor([float(th)], dtype=torch.float32, device="cuda")
    g = torch.tensor([0.75], dtype=torch.float32, device="cuda")
    if off is None:
        r = F.avu_forward(z, y, ut, T, th, R.BETA)
        r["grad"] = F.avu_backward(z, ut, T, r["coef"], r["workspace"], g)
        torch.cuda.synchronize()
    else:
        z, th, g = G.place(z, off), G.place(th, off), G.place(g, off)
        assert z.data_ptr() % 16 == 4 * off
        # fp32 results at the odd offset; the byte workspace and the float64 thresholds keep the 8-byte alignment the ABI asks for
        with G.guarded_allocations(lambda shape, dtype: off if dtype == torch.float32 else 2 * (off // 2)) as log:
            r = F.avu_forward(z, y, ut, T, th, R.BETA)
            r["grad"] = F.avu_backward(z, ut, T, r["coef"], r["workspace"], g)
        torch.cuda.synchronize()
        assert len(log) == 8, [b.tag for b in log]     # workspace, loss, v, sums, counts, thresholds, coef, dlogits
        G.check_all(log)                              # bands intact; every fp32 result written everywhere
    return {k: v.cpu().clone() for k, v in r.items()}


@pytest.mark.parametrize("case", ["b67c10", "b5c65", "mc_s3"])
def test_odd_offsets_inside_guard_bands_and_equal_bits(case):
    d = R.load(case)
    z, y = torch.from_numpy(d["z"]), torch.from_numpy(d["y"])
    ut = 1 if case.startswith("mc_") else 0
    th = d["th_type1"] if ut else d["th"]
    z3 = z if z.dim() == 3 else z[None]
    for T in (1, 21):
        _precondition(z, y, ut, T, th)
        base = _functional(z3, y, ut, T, th)
        again = _functional(z3, y, ut, T, th)
        o = R.evaluate(z, y, ut, T, th)
        assert R.error("grad", base["grad"].reshape(z.shape), 0.75 * o["grad"]) <= R.limit(d["meta"], f"mc_type{ut}" if ut else R.bc_group(case, T), "grad")
        for off in (1, 3):
            moved = _functional(z3, y, ut, T, th, off=off)
            for k in ("loss", "v", "sums", "counts", "thresholds", "coef", "grad", "pred", "acc", "first_certain", "uncertainty", "confidence"):
                assert torch.equal(base[k], again[k]), (k, "two runs differ")
                assert torch.equal(base[k], moved[k]), (k, off)


@pytest.mark.parametrize("T", [1, 21])
def test_forward_and_backward_captured_in_one_graph(T):
    """Capture loss + backward once; replay after copying new logits and a new threshold tensor into the static buffers: the bits of
    the eager call on those inputs."""
    from bayesian_torch_amd.utils.avuc_loss import AvULoss, AUAvULoss
    a, b = R.load("b7c5_s1"), R.load("b7c5_s3")
    for d in (a, b):
        _precondition(torch.from_numpy(d["z"]), torch.from_numpy(d["y"]), 0, T, d["th"])
    mod = AvULoss(beta=R.BETA) if T == 1 else AUAvULoss(beta=R.BETA)
    y = torch.from_numpy(a["y"]).cuda()

    def step(z, th):
        out = mod(z, y, th) if T == 1 else mod(z, y)[0]
        grad, = torch.autograd.grad(out.sum(), z)
        return out, grad
    zs = torch.from_numpy(a["z"]).cuda().requires_grad_()
    ths = torch.tensor([float(a["th"])], device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(zs, ths)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g, grad_g = step(zs, ths)
    # the labels stay (a's); new logits and a new threshold
    with torch.no_grad():
        zs.copy_(torch.from_numpy(b["z"]).cuda())
        ths.copy_(torch.tensor([float(b["th"])], device="cuda"))
    graph.replay()
    torch.cuda.synchronize()
    got_loss, got_grad = loss_g.clone(), grad_g.clone()
    ze = torch.from_numpy(b["z"]).cuda().requires_grad_()
    want_loss, want_grad = step(ze, torch.tensor([float(b["th"])], device="cuda"))
    torch.cuda.synchronize()
    assert torch.equal(got_loss, want_loss) and torch.equal(got_grad, want_grad)
    first = step(torch.from_numpy(a["z"]).cuda().requires_grad_(), float(a["th"]))
    assert not torch.equal(first[1], want_grad)      # (the replay did see the new inputs)


def test_train_graph_takes_the_loss_as_loss_fn():
    """mc.TrainGraph with cross-entropy + KL + AvULoss (threshold in a device tensor) as ``loss_fn``, against the same loop run eagerly
    from the same RNG position (the set-up of test_gpu_autograd.py's TrainGraph test): the same parameters bit for bit."""
    import copy
    from bayesian_torch_amd import rng
    from bayesian_torch_amd.harness import resnet as H
    from bayesian_torch_amd.mc import TrainGraph
    from bayesian_torch_amd.models.dnn_to_bnn import dnn_to_bnn, get_kl_loss
    from bayesian_torch_amd.utils.avuc_loss import AvULoss
    rng.set_mode("philox")
    torch.manual_seed(0)
    net = H.resnet18(10, width=8)
    dnn_to_bnn(net, {"prior_mu": 0.0, "prior_sigma": 1.0, "posterior_mu_init": 0.0, "posterior_rho_init": -3.0,
                     "type": "Reparameterization", "moped_enable": False, "moped_delta": 0.5})
    net = net.cuda().train()
    ref = copy.deepcopy(net)
    x = torch.randn(16, 3, 32, 32).cuda()
    y = torch.randint(0, 10, (16,)).cuda()
    avu, th = AvULoss(beta=3.0), torch.tensor([1.0], device="cuda")
    loss_fn = lambda m, out, yy: torch.nn.functional.cross_entropy(out, yy) + get_kl_loss(m) / 16 + avu(out, yy, th)   # noqa: E731
    n_warm, n_steps = 2, 2
    rng.manual_seed(11)
    opt_r = torch.optim.SGD(ref.parameters(), lr=0.01, momentum=0.9)
    eager = []
    for _ in range(n_warm + n_steps):
        opt_r.zero_grad(set_to_none=True)
        loss = loss_fn(ref, ref(x), y)
        loss.backward()
        opt_r.step()
        eager.append(float(loss))
    rng.manual_seed(11)
    opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9)
    tg = TrainGraph(net, opt, loss_fn, x, y, warmup=n_warm)
    got = [float(tg.step()) for _ in range(n_steps)]
    for a, b in zip(got, eager[n_warm:]):
        assert abs(a - b) <= 1e-6 * abs(b), (got, eager)      # (the fused wiring adds the KL means in another order: test_gpu_autograd.py)
    for (k, a), (_, b) in zip(net.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(a, b), k
    assert int(avu.last_stats["counts"].sum()) == 16
