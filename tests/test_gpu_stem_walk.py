"""The stem's sample walk (bt_fused_split_quad.h, WALK): a workgroup runs a run of Monte-Carlo samples over one staged patch
and pools from its accumulators. Its results are those of the one-sample path, bit for bit: every sample equals a launch of
that sample alone (S = 1, matching sample0) and the launch with the walk switched off (BT_QUAD_SPW=1), at every walk length."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

CONV = dict(stride=(2, 2), padding=(3, 3), dilation=(1, 1), groups=1)


def _params(Co, bias, seed):
    g = torch.Generator().manual_seed(seed)
    mu, rho = torch.randn(Co, 3, 7, 7, generator=g) * 0.1, torch.randn(Co, 3, 7, 7, generator=g) * 0.1 - 3
    mb = torch.randn(Co, generator=g) * 0.1 if bias else None
    rb = torch.randn(Co, generator=g) * 0.1 - 3 if bias else None
    sc, sh = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.3
    c = lambda t: None if t is None else t.cuda()
    return c(mu), c(rho), c(mb), c(rb), c(sc), c(sh)


def _stem(x, p, S, sample0=3, spw=None, shared=True, pool=True, want_kl=False):
    """One launch of the stem (conv -> scale / shift -> ReLU [-> MaxPool2d(3, 2, 1)]); spw caps the walk (BT_QUAD_SPW)."""
    from bayesian_torch_amd import _lib
    from bayesian_torch_amd import functional as F
    mu, rho, mb, rb, sc, sh = p
    kw = dict(conv=CONV, S=S, shared_x=shared, seed=41, call=6, layer_id=2, sample0=sample0, packed=F.pack_params(mu, rho),
              post_scale=sc, post_shift=sh, relu=True, pool=pool)
    if want_kl:
        pr = (torch.zeros_like(mu), torch.full_like(mu, 0.1), None if mb is None else torch.zeros_like(mb),
              None if mb is None else torch.full_like(mb, 0.1))
        kw.update(priors=pr, want_kl=True)
    old = os.environ.get("BT_QUAD_SPW")
    if spw is not None:
        os.environ["BT_QUAD_SPW"] = str(spw)
    try:
        out, kl = F._fused_forward(x, mu, rho, mb, rb, **kw)
        torch.cuda.synchronize()
        kn = _lib.lib().bt_last_kernel_name().decode()
    finally:
        if spw is not None:
            if old is None:
                del os.environ["BT_QUAD_SPW"]
            else:
                os.environ["BT_QUAD_SPW"] = old
    return out, kl, kn


# B, Co, S, walk caps to try, bias
CASES = {
    "cfg3 stem, S = 32": (128, 64, 32, (8, 4, 2), True),
    "S = 33: ragged last sample group": (128, 64, 33, (8, 4), True),
    "S = 8": (128, 64, 8, (2,), False),
    "S = 3, odd batch (last tile holds one image)": (255, 64, 3, (2,), True),
    "24 channels (rows past Cog)": (256, 24, 4, (2,), True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_walk_equals_one_sample_path(name):
    B, Co, S, caps, bias = CASES[name]
    p = _params(Co, bias, 17)
    x = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(4)).cuda()
    ref, _, kn1 = _stem(x, p, S, spw=1)
    assert "pool=1" in kn1 and "walk" not in kn1, kn1
    assert tuple(ref.shape) == (S * B, Co, 8, 8)
    for cap in caps:
        out, _, kn = _stem(x, p, S, spw=cap)
        assert "fused_split_quad_kernel" in kn and "pool=1" in kn and "walk" in kn, (cap, kn)
        assert torch.equal(out, ref), (name, cap)
    ref = ref.reshape(S, B, Co, 8, 8)
    for s in sorted({0, 1, S // 2, S - 1}):
        one, _, _ = _stem(x, p, 1, sample0=3 + s)
        assert torch.equal(one, ref[s]), (name, s)


def test_walk_is_the_default_for_the_cifar_stem():
    p = _params(64, True, 3)
    x = torch.randn(128, 3, 32, 32, generator=torch.Generator().manual_seed(5)).cuda()
    _, _, kn = _stem(x, p, 32)
    assert "walk" in kn, kn
    _, _, kn = _stem(x, p, 1)    # one sample: the one-sample path
    assert "walk" not in kn and "pool=1" in kn, kn


def test_walk_fused_kl_matches():
    p = _params(64, True, 8)
    x = torch.randn(128, 3, 32, 32, generator=torch.Generator().manual_seed(6)).cuda()
    ref, kl_ref, kn1 = _stem(x, p, 16, spw=1, want_kl=True)
    out, kl, kn = _stem(x, p, 16, want_kl=True)
    assert "walk" in kn and "walk" not in kn1
    assert torch.equal(out, ref)
    assert torch.equal(kl, kl_ref), (float(kl), float(kl_ref))


def test_stacked_x_and_unpooled_stems_keep_the_one_sample_path():
    p = _params(64, True, 9)
    S, B = 8, 128
    xs = torch.randn(S * B, 3, 32, 32, generator=torch.Generator().manual_seed(7)).cuda()
    out, _, kn = _stem(xs, p, S, shared=False)
    assert "walk" not in kn and "pool=1" in kn, kn
    for s in (0, S - 1):
        one, _, _ = _stem(xs[s * B:(s + 1) * B], p, 1, sample0=3 + s)
        assert torch.equal(one, out[s * B:(s + 1) * B])
    x = xs[:B]
    full, _, kn = _stem(x, p, S, pool=False)
    assert "walk" not in kn and "pool=0" in kn, kn
    pooled, _, kn = _stem(x, p, S)
    assert "walk" in kn, kn
    assert torch.equal(pooled, torch.nn.functional.max_pool2d(full, 3, 2, 1))
