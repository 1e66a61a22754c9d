"""CPU: tests/_q8_flip_model.py (the oracle of the q8 Flipout tests) held to torch's CPU quantised operators with exact equality:
quantized.mul and quantized.add of quint8 tensors over ALL 65 536 pairs of u8 values (the domain is finite: nothing is sampled), the
quantisation of the sign tensors at tie and saturating scales, and the whole chain against the literal operator chain
(quantize_per_tensor, quantized conv2d / linear, quantized.mul, quantized.add) on the layer cases the GPU test runs. The two readings
torch does not take (tests/_q8_flip_model.py) are shown to give other bytes. No kernels are launched."""
import math

import pytest
import torch

import _q8_edges as E
import _q8_flip_cases as FC
import _q8_flip_model as FM
import _q8_model as M

# (s_a, z_a, s_b, z_b, s_o, z_o): the default set, the set at which the unfused add differs, three more ...
NAMED_SETS = [(0.1, 128, 0.1, 128, 0.1, 128), (0.2, 3, 0.013, 250, 0.05, 100), (0.05, 120, 0.01, 100, 0.05, 131), (0.0437, 0, 0.4, 100, 0.03, 255),
              (0.153, 31, 2 / 3, 77, 0.0713, 57)]
TAIL = 13      # an odd tail behind the 65 536 pairs: torch's kernels have a vector body and a scalar tail


def _case_sets():
    """... and every set a layer case runs an operator at: (in, sign_in -> xp) and (pert, sign_out -> pert_signed) for mul, (mean,
    pert_signed -> out) for add."""
    mul, add = set(), set()
    for name, kind, bias, x_std in FC.LAYER_CASES + FC.EDGE_CASES:
        p = FC.case(name, kind, bias, 1, x_std)["pairs"]
        mul.add(p[FM.IN] + p[FM.SIGN_IN] + p[FM.XP])
        mul.add(p[FM.PERT] + p[FM.SIGN_OUT] + p[FM.PERT_SIGNED])
        add.add(p[FM.MEAN] + p[FM.PERT_SIGNED] + p[FM.OUT])
    return sorted(mul), sorted(add)


MUL_SETS = sorted(set(NAMED_SETS) | set(_case_sets()[0]))
ADD_SETS = sorted(set(NAMED_SETS) | set(_case_sets()[1]))


def _all_pairs():
    a = torch.arange(0, 256, dtype=torch.int32)
    a, b = a.repeat_interleave(256), a.repeat(256)
    return torch.cat([a, a[5::5041][:TAIL]]).to(torch.uint8), torch.cat([b, b[5::5041][:TAIL]]).to(torch.uint8)


def _qu(t, s, z):
    return torch._make_per_tensor_quantized_tensor(t, float(s), int(z))


PAD = 256      # what _body_add appends: more than the widest vector step (2 x 64 bytes), so every real position is in the vector body


def _body_add(qa, qb, s_o, z_o):
    """torch.ops.quantized.add with every position of qa / qb in the operator's VECTOR BODY -> int_repr of qa's shape. On this torch the
    operator is not a function of the pair alone: its vector body dequantises by one fused multiply-add, the scalar tail of each
    thread's chunk by (a - z) * s. So the operands are flattened, padded by PAD copies of their first
    element and added on one thread: one chunk, whose tail lies inside the padding."""
    n = qa.numel()
    flat = lambda q: torch._make_per_tensor_quantized_tensor(torch.cat([q.int_repr().reshape(-1), q.int_repr().reshape(-1)[:1].expand(PAD)]), q.q_scale(), q.q_zero_point())
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = torch.ops.quantized.add(flat(qa), flat(qb), s_o, z_o).int_repr()
    finally:
        torch.set_num_threads(threads)
    return out[:n].reshape(qa.shape)


def test_the_domain_is_whole():
    a, b = _all_pairs()
    assert a.numel() == 65536 + TAIL and len({(int(i), int(j)) for i, j in zip(a.tolist(), b.tolist())}) == 65536
    assert len(NAMED_SETS) >= 5 and NAMED_SETS[0] == (0.1, 128, 0.1, 128, 0.1, 128)


@pytest.mark.parametrize("st", MUL_SETS, ids=lambda s: "-".join(f"{v:g}" for v in s))
def test_umul_over_all_u8_pairs(st):
    s_a, z_a, s_b, z_b, s_o, z_o = st
    a, b = _all_pairs()
    ref = torch.ops.quantized.mul(_qu(a, s_a, z_a), _qu(b, s_b, z_b), s_o, z_o).int_repr()
    got = FM.umul(a, (s_a, z_a), b, (s_b, z_b), (s_o, z_o))
    bad = int((got != ref).sum())
    print(f"umul {st}: {a.numel()} positions compared (all 65536 pairs and a tail of {TAIL}), {bad} differ")
    assert torch.equal(got, ref), bad


@pytest.mark.parametrize("st", ADD_SETS, ids=lambda s: "-".join(f"{v:g}" for v in s))
def test_uadd_over_all_u8_pairs(st):
    s_a, z_a, s_b, z_b, s_o, z_o = st
    a, b = _all_pairs()
    a, b = a[:65536], b[:65536]
    ref = _body_add(_qu(a, s_a, z_a), _qu(b, s_b, z_b), s_o, z_o)
    got = FM.uadd(a, (s_a, z_a), b, (s_b, z_b), (s_o, z_o))
    bad = int((got != ref).sum())
    loose = torch.ops.quantized.add(_qu(a, s_a, z_a), _qu(b, s_b, z_b), s_o, z_o).int_repr()      # as the threads happen to split it: chunk tails inside
    print(f"uadd {st}: 65536 positions compared, all in the vector body (every pair of u8 values once), {bad} differ; "
          f"with the operator's own chunking {int((got != loose).sum())} positions (scalar tails) differ")
    assert torch.equal(got, ref), bad


def test_the_rejected_forms_differ_from_torch_somewhere():
    a, b = _all_pairs()
    st = NAMED_SETS[0]
    ref = torch.ops.quantized.mul(_qu(a, st[0], st[1]), _qu(b, st[2], st[3]), st[4], st[5]).int_repr()
    n_mul = int((FM.umul_double_quotient(a, st[0:2], b, st[2:4], st[4:6]) != ref).sum())
    st = NAMED_SETS[1]
    ref = _body_add(_qu(a, st[0], st[1]), _qu(b, st[2], st[3]), st[4], st[5])
    n_add = int((FM.uadd_unfused(a, st[0:2], b, st[2:4], st[4:6]) != ref).sum())
    print(f"double-quotient umul at {NAMED_SETS[0]}: {n_mul} mismatches; unfused uadd at {NAMED_SETS[1]}: {n_add} mismatches")
    assert n_mul > 0 and n_add > 0


@pytest.mark.parametrize("s,z,want", [(2 / 3, 77, (79, 75)), (0.4, 100, (102, 98)), (0.005, 128, (255, 0)), (0.1, 128, (138, 118)), (0.01, 100, (200, 0))])
def test_sign_quantisation_at_ties_and_saturation(s, z, want):
    """1 / f32(2 / 3) = 1.5 and 1 / f32(0.4) = 2.5 exactly: ties, rounded to even; s = 0.005 saturates both signs; 0.1 at 128: the default."""
    sign = torch.tensor([1.0, -1.0])
    if s in (2 / 3, 0.4):
        assert float(M.rcp32(s)) in (1.5, 2.5)
    ref = torch.quantize_per_tensor(sign, s, z, torch.quint8).int_repr()
    got = FM.quant_sign(sign, s, z)
    assert torch.equal(got, ref) and tuple(got.tolist()) == want


def _torch_chain(c, s):
    """The literal operator chain of the quantised Flipout layers on sample s of a case -> the quint8 output's int_repr."""
    qf = torch.nn.quantized.functional
    P, conv = c["pairs"], c["conv"]
    x = torch.quantize_per_tensor(c["x"][0], *P[FM.IN], torch.quint8)
    q_mu = torch._make_per_tensor_quantized_tensor(c["q_mu"], FC.S_MU, 0)
    q_sigma = torch._make_per_tensor_quantized_tensor(c["q_sigma"], FC.S_SIGMA, 0)
    op = (lambda a, w, b, pr: qf.linear(a, w, b, scale=pr[0], zero_point=pr[1])) if conv is None else \
        (lambda a, w, b, pr: qf.conv2d(a, w, b, conv["stride"], conv["padding"], conv["dilation"], 1, scale=pr[0], zero_point=pr[1]))
    o1 = op(x, q_mu, c["mu_b"], P[FM.MEAN])
    sign_in = torch.quantize_per_tensor(c["sign_in"][s], *P[FM.SIGN_IN], torch.quint8)
    sign_out = torch.quantize_per_tensor(c["sign_out"][s], *P[FM.SIGN_OUT], torch.quint8)
    e = torch.quantize_per_tensor(c["eps_w"][s], P[FM.EPS][0], 0, torch.qint8)
    delta = torch.ops.quantized.mul(q_sigma, e, P[FM.DELTA][0], 0)
    xp = torch.ops.quantized.mul(x, sign_in, *P[FM.XP])
    bp = None if (c["mu_b"] is None or c["sigma_b"] is None) else c["sigma_b"] * c["eps_b"][s]
    p = op(xp, delta, bp, P[FM.PERT])
    ps = torch.ops.quantized.mul(p, sign_out, *P[FM.PERT_SIGNED])
    out = torch._make_per_tensor_quantized_tensor(_body_add(o1, ps, *P[FM.OUT]), *P[FM.OUT])      # (quantized.add, every position in its vector body)
    return out.int_repr(), dict(o1=o1.int_repr(), xp=xp.int_repr(), p=p.int_repr(), ps=ps.int_repr())


@pytest.mark.parametrize("name,kind,bias,x_std", FC.LAYER_CASES + FC.EDGE_CASES + [FC.ON_CHIP_EDGE, FC.GUARD_EDGE])
def test_whole_chain_equals_the_operator_chain(name, kind, bias, x_std):
    """fbgemm: oneDNN's dilated quantised conv corrupts the heap in torch 2.10, and its requantisation ties are its own
    (tests/test_q8_model_host.py)."""
    c = FC.case(name, kind, bias, 1, x_std)
    oq, out, mid = FC.model(c)
    prev = torch.backends.quantized.engine
    torch.backends.quantized.engine = "fbgemm"
    try:
        ref, rmid = _torch_chain(c, 0)
    finally:
        torch.backends.quantized.engine = prev
    for k in ("o1", "xp", "p", "ps"):
        assert torch.equal(mid[0][k], rmid[k]), (k, int((mid[0][k] != rmid[k]).sum()))
    print(f"{name} {kind} {bias}: {ref.numel()} outputs, {len(torch.unique(ref))} levels, {int((oq != ref).sum())} differ")
    assert torch.equal(oq, ref)
    assert torch.equal(out, torch._make_per_tensor_quantized_tensor(ref, *c["pairs"][FM.OUT]).dequantize())


def test_cases_reach_what_they_are_for():
    """x' = 256 -> 255 under a negative sign at xq = 0; both clamp ends of o1, p, p' and oq; unsaturated cases elsewhere."""
    c = FC.case("conv_c37x70k3p1_9x7", "default", "mu_only", 1, 8.0)
    mid = FC.model(c)[2][0]
    hit = (mid["xq"] == 0) & (c["sign_in"][0] < 0)
    assert int(hit.sum()) > 10 and bool((mid["xp"][hit] == 255).all())
    for name, kind, bias, x_std in FC.LAYER_CASES:
        if kind != "clamps" or name != "conv_c37x70k3p1_9x7":
            continue
        c = FC.case(name, kind, bias, 1, x_std)
        oq, _, mid = FC.model(c)
        for k, t in (("o1", mid[0]["o1"]), ("p", mid[0]["p"]), ("ps", mid[0]["ps"]), ("oq", oq)):
            assert int((t == 0).sum()) > 0 and int((t == 255).sum()) > 0, (name, k)
            assert int(((t > 0) & (t < 255)).sum()) > t.numel() // 4, (name, k)
    c = FC.case("conv_c37x70k3p1_9x7", "dict", "full", 1, 1.5)
    oq, _, mid = FC.model(c)
    assert len(torch.unique(oq)) > 64 and len(torch.unique(mid[0]["p"])) > 64 and len(torch.unique(mid[0]["d"])) > 64


def test_edge_cases_reach_what_they_are_for():
    """The edge-geometry cases (FC.EDGE_CASES, FC.ON_CHIP_EDGE, FC.GUARD_EDGE): the model's u8 output has more than 16 distinct values
    (the bar of test_gpu_q8_edges.py's uneven-geometry test), the 'dict' cases' intermediates o1, p and p' are not constant, and each
    geometry is walked the way its case is for: pruned or not, a pixel tile that crosses images, two channel and two pixel tiles."""
    want_pruned = {("k3x5_2x7_uneven", "default"): True, ("k3x5_2x7_uneven", "dict"): False, ("k5x5_2x2_p2", "default"): False,
                   ("k2x8_3x2_p1x7", "dict"): False, ("k4x4_2x1_s2p3", "default"): True, ("k3x3_1x5", "default"): True}
    specs = [(c, 1) for c in FC.EDGE_CASES] + [(FC.ON_CHIP_EDGE, 2), (FC.GUARD_EDGE, 2)]
    assert {(s[0], s[1]) for s, _ in specs} == set(want_pruned) and {s[0] for s, _ in specs} == set(FC.EDGE_GEOMS)
    for (name, kind, bias, x_std), S in specs:
        c = FC.case(name, kind, bias, S, x_std)
        oq, _, mid = FC.model(c)
        levels = {k: len(torch.unique(torch.cat([m[k] for m in mid]))) for k in ("o1", "p", "ps")}
        print(f"{name} {kind} S={S}: {oq.numel()} outputs, {len(torch.unique(oq))} levels; o1 / p / p' levels {levels}; pruned: {FC.pruned(c)}")
        assert len(torch.unique(oq)) > 16, (name, kind)
        assert FC.pruned(c) is want_pruned[(name, kind)], (name, kind)
        if kind == "dict":
            assert all(p[1] != 128 for p in c["pairs"][2:]) and min(levels.values()) > 1, (name, levels)
        else:
            assert all(p[1] == 128 for p in c["pairs"][2:]), name
        if S == 2:
            assert not torch.equal(*oq.chunk(2, 0)), name
    wshape, xshape, conv = FC.GEOMS["k3x5_2x7_uneven"]
    assert wshape[0] > 64 and xshape[0] * math.prod(E.conv_out(conv, wshape, xshape)) > 128            # two channel tiles, two pixel tiles
    assert all(a != b for a, b in (wshape[2:], conv["stride"], conv["padding"], conv["dilation"]))
    wshape, xshape, conv = FC.GEOMS["k2x8_3x2_p1x7"]
    per = math.prod(E.conv_out(conv, wshape, xshape))
    assert per < 128 < xshape[0] * per and 128 % per                                                   # pixel 128 lies inside an image
    assert math.prod(FC.GEOMS["k4x4_2x1_s2p3"][0][2:]) == 16 and math.prod(FC.GEOMS["k5x5_2x2_p2"][0][2:]) == 25


def test_the_rejected_forms_change_the_layer_cases():
    """So that the GPU test, which compares with the model on these cases, can tell the forms apart."""
    n_mul = n_add = 0
    for name, kind, bias, x_std in FC.LAYER_CASES:
        c = FC.case(name, kind, bias, 1, x_std)
        oq = FC.model(c)[0]
        n_mul += int((FC.model(c, mul=FM.umul_double_quotient)[0] != oq).sum())
        n_add += int((FC.model(c, add=FM.uadd_unfused)[0] != oq).sum())
    print(f"over the layer cases: the double-quotient umul changes {n_mul} outputs, the unfused uadd {n_add}")
    assert n_mul > 0 and n_add > 0
