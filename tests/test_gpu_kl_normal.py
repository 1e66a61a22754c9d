"""GPU: bt_kl_normal over many segments, what test_gpu_hier.py holds bt_kl_hier to -- 70 segments in two launches against the 70
one-segment launches bit for bit and against float64, determinism, a zeroed workspace, a segment beyond the block cap."""
import math

import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
LENS = (1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193)   # thread, float4, pass and block edges
NSEG = 70
KINDS = ("normal", "laplace")
RTOL = 1e-5      # what test_gpu_layers.py holds this kernel to against fp64


def _kl64(mu, rho, pm, ps, kind):
    """kl_div's mean (base_variational_layer.py:68-97) in float64."""
    mu, rho, pm, ps = (t.double().cpu() for t in (mu, rho, pm, ps))
    sq = torch.log1p(torch.exp(rho))
    if kind == "laplace":      # against Laplace(0, 1): log 2 - 0.5 log(2 pi sq^2) - 0.5 + E|w|
        e_abs = sq * math.sqrt(2 / math.pi) * torch.exp(-mu ** 2 / (2 * sq ** 2)) + mu * torch.erf(mu / (sq * math.sqrt(2)))
        return (math.log(2) - 0.5 * torch.log(2 * math.pi * sq ** 2) - 0.5 + e_abs).mean()
    return (torch.log(ps) - torch.log(sq) + (sq ** 2 + (mu - pm) ** 2) / (2 * ps ** 2) - 0.5).mean()


def _tensors(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(n, generator=g), -3.0 + 0.1 * torch.randn(n, generator=g), torch.zeros(n), torch.ones(n))


@pytest.fixture(scope="module")
def packed():
    """70 segments as views into ONE buffer per tensor: even segments start 16-byte aligned (float4 body + scalar tail), odd ones at
    a byte offset of 4 modulo 8 (the scalar path)."""
    lens = [LENS[j % len(LENS)] for j in range(NSEG)]
    offs, off = [], 0
    for j, n in enumerate(lens):
        off = (off + 3) // 4 * 4 + (j % 2)
        offs.append(off)
        off += n + 1
    bufs = []
    for t in _tensors(off, 1234):
        b = t.to(DEV)
        assert b.data_ptr() % 16 == 0
        bufs.append(b)
    segs = [tuple(b[o:o + n] for b in bufs) for o, n in zip(offs, lens)]
    assert all(t.data_ptr() % 16 == 0 if j % 2 == 0 else t.data_ptr() % 8 == 4 for j, sg in enumerate(segs) for t in sg)
    return segs


def _layer_sum32(v, lids):
    """One launch's fp32 order: the segments of a layer added in order, then the layers in order."""
    total = layer = np.float32(0)
    for j, x in enumerate(np.asarray(v, dtype=np.float32)):
        if j == 0 or lids[j] != lids[j - 1]:
            if j:
                total = np.float32(total + layer)
            layer = x
        else:
            layer = np.float32(layer + x)
    return np.float32(total + layer)


@pytest.mark.parametrize("kind", KINDS)
def test_kl_70_segments_two_launches(packed, kind):
    from bayesian_torch_amd import _lib
    lap = kind == "laplace"
    lids = [j // 2 for j in range(NSEG)]      # pairs of segments form a layer (64 is even: no pair straddles the launches)
    single = [_lib.kl_normal([sg], owner="test_kl_normal", laplace=lap) for sg in packed]
    total = _lib.kl_normal(packed, layer_ids=lids, owner="test_kl_normal", laplace=lap)
    total2 = _lib.kl_normal(packed, layer_ids=lids, owner="test_kl_normal", laplace=lap)
    torch.cuda.synchronize()
    assert torch.equal(total, total2)
    assert int(_lib.workspace("test_kl_normal", total.device).count_nonzero()) == 0
    for j, (sg, v) in enumerate(zip(packed, single)):
        assert_close(v.cpu(), _kl64(*sg, kind).float(), RTOL, 0, f"{kind} segment {j} of {sg[0].numel()}")
    p = np.array([float(v) for v in single], dtype=np.float32)
    want = np.float32(_layer_sum32(p[:64], lids[:64]) + _layer_sum32(p[64:], lids[64:]))
    print(f"{kind}: total {float(total):.9g}, grouped single-segment launches {float(want):.9g}")
    assert np.float32(total.item()) == want


@pytest.mark.parametrize("kind", KINDS)
def test_kl_segment_beyond_the_block_cap(kind):
    """1024 blocks of 4096 elements is the cap: one segment of 1024 * 4096 + 4097 elements makes its blocks stride."""
    from bayesian_torch_amd import _lib
    seg = tuple(t.to(DEV) for t in _tensors(1024 * 4096 + 4097, 4321))
    k1 = _lib.kl_normal([seg], owner="test_kl_normal", laplace=kind == "laplace")
    k2 = _lib.kl_normal([seg], owner="test_kl_normal", laplace=kind == "laplace")
    torch.cuda.synchronize()
    assert torch.equal(k1, k2)
    assert int(_lib.workspace("test_kl_normal", k1.device).count_nonzero()) == 0
    assert_close(k1.cpu(), _kl64(*seg, kind).float(), RTOL, 0, f"{kind} one segment of {seg[0].numel()} elements")
