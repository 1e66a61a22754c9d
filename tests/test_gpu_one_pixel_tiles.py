"""GPU: the one-pixel tiles of the general split kernel (bt_fused_split.h, split_one_pixel_tile): launches whose input and output
planes are one pixel -- a padded 3x3 window over 1x1 maps, Linear -- on the ``xm=1`` instantiations, where the consumers load and
split x in registers and the producers stage weights alone.

The yardstick is the UNCHANGED ``xm=0`` instantiation of the same tile: an x buffer displaced by 4 bytes makes the planner choose the
generic fetch (tests/_guard_rows.py, row g_xm1), everything else about the launch stays.  Per case: the two launches are equal bit for
bit (both kernel names asserted), the injected twin on the materialised draws is equal bit for bit, S = 2 in one launch equals two
launches of one sample, and the result matches the fp64 C oracle on the replayed draws at test_gpu_split.py's tolerances.  The direct
and split-K flavours, which would take the K = 64 and the narrow launches first, are switched off through their test hooks.

B = 1: a launch of fewer than 112 columns is not planned on the split kernels at all (split_plan), aligned or not, so there is no
``xm=1`` launch to hold; those rows assert exactly that, and still hold the aligned launch to the displaced one and to the oracle."""
import ctypes

import pytest
import torch

from _guard import place
from conftest import assert_close

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 1e-5      # tests/test_gpu_split.py
SEED, CALL, LAYER, SAMPLE0, S = 41, 3, 6, 4, 2

# label: (kind, K, Co, B, bias, folded stage (scale / shift + residual + ReLU), shared x, 32-channel tiles, KL)
CASES = {
    "conv K=64 Co=128 B=128": ("conv", 64, 128, 128, False, False, False, False, False),
    "conv K=64 Co=40 B=120 bias stage shared": ("conv", 64, 40, 120, True, True, True, False, True),
    "conv K=72 Co=40 B=128 bias": ("conv", 72, 40, 128, True, False, False, False, False),
    "conv K=72 Co=128 B=120 stage bn32": ("conv", 72, 128, 120, False, True, False, True, False),
    "conv K=512 Co=128 B=128 bias stage": ("conv", 512, 128, 128, True, True, False, False, True),
    "conv K=512 Co=40 B=120 shared bn32": ("conv", 512, 40, 120, False, False, True, True, False),
    "conv K=520 Co=40 B=128 stage shared": ("conv", 520, 40, 128, False, True, True, False, False),
    "conv K=520 Co=128 B=120 bias bn32": ("conv", 520, 128, 120, True, False, False, True, True),
    "linear K=64 Co=40 B=128 bias bn32": ("linear", 64, 40, 128, True, False, False, True, False),
    "linear K=64 Co=128 B=120 stage": ("linear", 64, 128, 120, False, True, False, False, False),
    "linear K=72 Co=128 B=128 bias stage shared": ("linear", 72, 128, 128, True, True, True, False, False),
    "linear K=72 Co=40 B=120": ("linear", 72, 40, 120, False, False, False, False, True),
    "linear K=512 Co=40 B=128 bias stage": ("linear", 512, 40, 128, True, True, False, False, False),
    "linear K=512 Co=128 B=120 bias shared": ("linear", 512, 128, 120, True, False, True, False, False),
    "linear K=520 Co=128 B=128 stage bn32": ("linear", 520, 128, 128, False, True, False, True, True),
    "linear K=520 Co=40 B=120 bias shared bn32": ("linear", 520, 40, 120, True, False, True, True, False),
    "conv K=512 Co=128 B=1 bias stage": ("conv", 512, 128, 1, True, True, False, False, False),
    "linear K=72 Co=40 B=1 shared": ("linear", 72, 40, 1, False, False, True, False, False),
}


@pytest.fixture(autouse=True)
def _switches():
    """The general kernel for every row (the direct and split-K flavours off), and every process-wide knob back afterwards."""
    from bayesian_torch_amd import _lib, rng
    L = _lib.lib()
    L.bt_debug_disable_direct(1)
    L.bt_debug_disable_skinny(1)
    yield
    L.bt_debug_disable_direct(0)
    L.bt_debug_disable_skinny(0)
    L.bt_debug_force_bn32(-1)
    L.bt_set_contraction(0)
    rng.set_inject_path("general")


class Case:
    def __init__(self, label):
        from bayesian_torch_amd import functional as F
        self.label = label
        self.kind, self.K, self.Co, self.B, self.bias, self.stage, self.shared, self.bn32, self.kl = CASES[label]
        K, Co, B = self.K, self.Co, self.B
        g = torch.Generator().manual_seed(sum(map(ord, label)))
        wshape = (Co, K, 3, 3) if self.kind == "conv" else (Co, K)
        self.mu, self.rho = torch.randn(wshape, generator=g) * 0.1, torch.randn(wshape, generator=g) * 0.1 - 3
        self.mb = torch.randn(Co, generator=g) * 0.1 if self.bias else None
        self.rb = torch.randn(Co, generator=g) * 0.1 - 3 if self.bias else None
        rows = B if self.shared else S * B
        self.x = torch.randn((rows, K, 1, 1) if self.kind == "conv" else (rows, K), generator=g)
        oshape = (S * B, Co, 1, 1) if self.kind == "conv" else (S * B, Co)
        self.scale = torch.rand(Co, generator=g) + 0.5 if self.stage else None
        self.shift = torch.randn(Co, generator=g) if self.stage else None
        self.res = torch.randn(oshape, generator=g) if self.stage else None
        self.conv = dict(stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1) if self.kind == "conv" else None
        c = lambda t: None if t is None else t.cuda()
        self.d = {k: c(getattr(self, k)) for k in ("mu", "rho", "mb", "rb", "scale", "shift", "res")}
        self.pk = F.pack_params(self.d["mu"], self.d["rho"])
        self.pri = (torch.zeros_like(self.d["mu"]), torch.ones_like(self.d["mu"]),
                    None if self.mb is None else torch.zeros_like(self.d["mb"]), None if self.mb is None else torch.ones_like(self.d["mb"]))
        self.x_al, self.x_off = place(c(self.x), 0), place(c(self.x), 1)      # 16-byte aligned / displaced by 4 bytes, NaN bands around both
        assert self.x_al.data_ptr() % 16 == 0 and self.x_off.data_ptr() % 16 == 4

    def run(self, x, mode=0, samples=(0, S), draws=None, poison=None):
        """One launch of samples [s0, s1) -> (out, kl, kernel name)."""
        from bayesian_torch_amd import _lib
        from bayesian_torch_amd import functional as F
        L, d = _lib.lib(), self.d
        s0, s1 = samples
        n, B = s1 - s0, self.B
        xs = x if self.shared else x[s0 * B:s1 * B]
        kw = dict(conv=self.conv, S=n, shared_x=self.shared, seed=SEED, call=CALL, layer_id=LAYER, sample0=SAMPLE0 + s0, packed=self.pk)
        if self.stage:
            kw.update(post_scale=d["scale"], post_shift=d["shift"], residual=d["res"][s0 * B:s1 * B], relu=True)
        if self.kl:
            kw.update(priors=self.pri, want_kl=True, workspace_owner="t_one_pixel")
        if draws is not None:
            kw.update(eps_w=draws[0][s0:s1].contiguous(), eps_b=None if draws[1] is None else draws[1][s0:s1].contiguous(), inject_path="split")
        L.bt_debug_force_bn32(1 if self.bn32 else 0)
        _lib.check(L.bt_set_contraction(mode))
        try:
            if poison is not None:
                poison()
            out, kl = F.fused_forward(xs, d["mu"], d["rho"], d["mb"], d["rb"], **kw)
            return out, kl, L.bt_last_kernel_name().decode()
        finally:
            L.bt_set_contraction(0)

    def draws(self):
        from bayesian_torch_amd import functional as F
        dev = torch.device("cuda")
        eps_w = F.rng_fill_normal(SEED, CALL, LAYER, SAMPLE0, 0, S, self.mu.shape, dev)
        eps_b = F.rng_fill_normal(SEED, CALL, LAYER, SAMPLE0, 1, S, (self.Co,), dev) if self.bias else None
        return eps_w, eps_b

    def name(self, xm, np=3, inj=False):
        return "fused_split_kernel<%d,128,bf16x%d,%s terms,npw=8,xm=%d%s>" % (32 if self.bn32 else 64, np, "6" if np == 3 else "1", xm, ",inj" if inj else "")

    def oracle(self, eps_w, eps_b):
        """fp64 C oracle on the replayed draws, then the folded output stage in fp64 -> [S * B, ...]."""
        from oracle import c_oracle as CO
        B, outs = self.B, []
        for s in range(S):
            xs = self.x if self.shared else self.x[s * B:(s + 1) * B]
            ref = CO.reparam_fwd(xs, self.mu, self.rho, eps_w[s].cpu(), self.mb, self.rb, None if eps_b is None else eps_b[s].cpu(), self.conv).double()
            if self.stage:
                sh = (1, -1, 1, 1) if self.kind == "conv" else (1, -1)
                ref = ref * self.scale.double().view(sh) + self.shift.double().view(sh) + self.res[s * B:(s + 1) * B].double()
                ref = ref.clamp_min(0.0)
            outs.append(ref)
        return torch.cat(outs)


def _poison_hook():
    from bayesian_torch_amd import _lib
    L = _lib.lib()
    L.bt_debug_poison_lds.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.bt_debug_poison_lds.restype = ctypes.c_int
    word = torch.zeros(4, dtype=torch.int32, device="cuda")

    def poison():
        assert L.bt_debug_poison_lds(word.data_ptr(), _lib.stream_ptr(word.device)) == 0
    return poison


@pytest.mark.parametrize("label", list(CASES))
def test_one_pixel_tile_is_the_generic_fetch_bit_for_bit(label):
    c = Case(label)
    out, kl, kn = c.run(c.x_al)
    ref, klr, kn0 = c.run(c.x_off)
    eps_w, eps_b = c.draws()
    if c.B < 112:      # not a split-kernel launch, aligned or displaced (module docstring)
        assert "fused_split_kernel" not in kn and "fused_split_kernel" not in kn0, (kn, kn0)
    else:
        assert kn == c.name(1), kn
        assert kn0 == c.name(0), kn0
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref), f"{label}: {kn} differs from {kn0}: max abs {float((out - ref).abs().max()):.3e}"
    if c.kl:
        assert float(kl) == float(klr), (label, float(kl), float(klr))
    # the fp64 oracle on the replayed draws
    assert_close(out.cpu(), c.oracle(eps_w, eps_b), RTOL, ATOL, label + " vs C oracle")
    if c.B < 112:
        return
    # the injected twin reads the materialised draws: same bits
    inj, kli, kni = c.run(c.x_al, draws=(eps_w, eps_b))
    assert kni == c.name(1, inj=True), kni
    assert torch.equal(inj, out), f"{label}: {kni} differs from {kn}: max abs {float((inj - out).abs().max()):.3e}"
    # S = 2 in one launch against two launches of one sample each
    parts = [c.run(c.x_al, samples=(s, s + 1)) for s in range(S)]
    assert all("xm=1" in p[2] and "fused_split_kernel" in p[2] for p in parts), [p[2] for p in parts]
    assert torch.equal(torch.cat([p[0] for p in parts]), out), label + ": one launch of two samples vs two launches of one"


def test_one_pixel_tile_behind_poisoned_lds():
    """LDS survives from kernel to kernel: filled with NaN patterns right before the launch, the same bits come out -- the path clears
    nothing up front, so every weight slot it reads (the empty half of the last odd pair, the rows past the group's channels of a
    partial channel tile) has to be written by the launch itself."""
    poison = _poison_hook()
    for label in ("conv K=72 Co=40 B=128 bias", "linear K=520 Co=40 B=120 bias shared bn32"):
        c = Case(label)
        out, _, kn = c.run(c.x_al)
        assert kn == c.name(1), kn
        got, _, kn1 = c.run(c.x_al, poison=poison)
        assert kn1 == kn
        assert torch.isfinite(got).all() and torch.equal(got, out), label
        twin, _, kn0 = c.run(c.x_off, poison=poison)
        assert kn0 == c.name(0), kn0
        assert torch.equal(twin, out), label


@pytest.mark.parametrize("label", ["conv K=520 Co=128 B=120 bias bn32", "linear K=72 Co=128 B=128 bias stage shared"])
def test_one_pixel_tile_in_bf16_mode(label):
    """bt_set_contraction(3): one rounded piece per value, same tile, same plan -- against its xm=0 twin."""
    c = Case(label)
    out, _, kn = c.run(c.x_al, mode=3)
    ref, _, kn0 = c.run(c.x_off, mode=3)
    assert kn == c.name(1, np=1), kn
    assert kn0 == c.name(0, np=1), kn0
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref), f"{label}: {kn} differs from {kn0}: max abs {float((out - ref).abs().max()):.3e}"
