"""The chain planner of bt_reparam_conv2d_chain_fwd, without a GPU: with ``bt_debug_plan_only(1)`` launch_kernel records the launch and
returns before it touches the runtime (tools/record_split_plans.py reaches split_plan the same way), so calls with made-up, aligned
addresses -- never dereferenced on the host -- run validation, the members' split_plan and the chain's eligibility rule.

Shapes: cfg3's layer1 (ResNet18 / CIFAR, b128, S = 32: 64 -> 64 3x3 on 8x8 maps, four members, residuals as in two basic blocks) is
accepted; every way out of the rule is declined with BT_CHAIN_DECLINED and nothing recorded as launched."""
import ctypes as C

import pytest

from bayesian_torch_amd import _lib

P = 0x10000000            # any non-null, 16-byte aligned address
MB = 1 << 26              # spacing of the made-up buffers: more than any tensor here holds


class Chain:
    """n members of one shape over made-up addresses; the fields a case changes are plain attributes."""

    def __init__(self, n=4, C_=64, H=8, B=128, S=32, k=3, stride=1, pad=1):
        self.n, self.S = n, S
        self.geoms = [_lib.bt_conv2d_geom(B, C_, H, H, C_, k, k, stride, stride, pad, pad, 1, 1, 1) for _ in range(n)]
        self.x = [P + MB * i for i in range(n)]                      # member k reads buffer k ...
        self.out = [P + MB * (i + 1) for i in range(n)]              # ... and writes buffer k + 1
        self.res = [None, self.x[0], None, self.out[1]][:n] + [None] * max(0, n - 4)      # two basic blocks: the input, member 1's out
        self.kl = [None] * n
        self.shared = False

    def call(self):
        L = _lib.lib()
        keep, arr = [], (_lib.bt_chain_member * self.n)()
        for i, g in enumerate(self.geoms):
            out_elems = g.B * g.Co * g.H * g.W // (g.sh * g.sw)
            par = _lib.bt_params(P, P, None, None, None, None, None, None, P, P, 0, 0)
            dr = _lib.bt_draws(None, None, None, None, _lib.bt_rng(7, None, 10 + i, 1 + i, 0, 0))
            ep = _lib.bt_epilogue(P, P, self.res[i], out_elems if self.res[i] is not None else 0, 1, 0)
            xss = 0 if (i == 0 and self.shared) else g.B * g.Ci * g.H * g.W
            keep.append((par, dr, ep))
            arr[i] = _lib.bt_chain_member(C.pointer(g), self.x[i], xss, C.pointer(par), C.pointer(dr), C.pointer(ep), self.out[i], self.kl[i])
        return L.bt_reparam_conv2d_chain_fwd(self.n, arr, self.S, None)


@pytest.fixture()
def plan_only():
    h = C.CDLL(_lib.LIB_PATH)      # the bt_debug_* hooks are outside include/bt_hip.h
    _lib.lib()
    h.bt_debug_plan_only(1)
    try:
        yield
    finally:
        h.bt_debug_plan_only(0)


def test_accepts_cfg3_layer1(plan_only):
    c = Chain()
    assert c.call() == 0
    name = _lib.lib().bt_last_kernel_name().decode()
    assert name == "fused_split_chain_kernel<64,512,bf16x3,6 terms,npw=4,xm=3,n=4>", name
    info = _lib.last_launch_info()
    assert (info["workgroups"], info["m_tiles"], info["n_tiles"], info["S"], info["t_NI"], info["t_R"], info["t_Wt"]) == (512, 16, 1, 32, 8, 8, 8), info
    two = Chain(n=2)
    assert two.call() == 0 and _lib.lib().bt_last_kernel_name().decode().endswith("xm=3,n=2>")
    shared = Chain()
    shared.shared = True            # the first member's x shared by the samples
    assert shared.call() == 0


def _declined(c):
    L = _lib.lib()
    assert Chain(n=2).call() == 0 and L.bt_last_kernel_name().decode().endswith("n=2>")      # (a launch whose record a decline must leave alone)
    assert c.call() == _lib.CHAIN_DECLINED
    assert L.bt_last_kernel_name().decode().endswith("n=2>"), "a declined chain recorded a launch"


def test_declines_two_channel_tiles(plan_only):
    _declined(Chain(C_=128))


def test_declines_stride_2(plan_only):
    c = Chain(n=2)
    c.geoms[0] = _lib.bt_conv2d_geom(128, 64, 16, 16, 64, 3, 3, 2, 2, 1, 1, 1, 1, 1)      # 16x16 -> 8x8: member 1 reads 8x8
    _declined(c)


def test_declines_differing_H(plan_only):
    c = Chain(n=2)
    c.geoms[1] = _lib.bt_conv2d_geom(128, 64, 4, 4, 64, 3, 3, 1, 1, 1, 1, 1, 1, 1)
    _declined(c)


def test_declines_a_256_wide_plan(plan_only):
    _declined(Chain(B=16, S=3))      # six workgroups of 512 columns: split_plan takes the 256-wide tile


def test_declines_overlapping_buffers(plan_only):
    c = Chain()
    c.out[3] = c.out[1] + 64         # member 3's out inside member 1's
    _declined(c)
    c = Chain()
    c.out[2] = c.x[0]                # an out over the chain's input
    c.x[3] = c.out[2]
    _declined(c)
    c = Chain()
    c.res[1] = c.out[2]              # a residual that a LATER member writes
    _declined(c)
    c = Chain()
    c.x[2] = P + MB * 9              # member 2 does not read what member 1 wrote
    _declined(c)


def test_declines_a_kl_sweep(plan_only):
    c = Chain()
    c.kl[2] = P
    _declined(c)


def test_declines_more_than_four_members(plan_only):
    _declined(Chain(n=5))


def test_the_switch_reads_its_environment():
    """BT_CHAIN=0 -- what A/B runs set -- and the counter passes bench.py --full starts of itself (BT_BENCH_CHILD) switch the chained
    launches off at import; nothing set, they are on. A process of its own per setting: the variable is read once."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from bayesian_torch_amd.layers import _fused as f; a = f.chain_enabled(); b = f.set_chain(not a); print(a, b, f.chain_enabled())"
    for extra, want in (({}, "True True False"), ({"BT_CHAIN": "0"}, "False False True"), ({"BT_CHAIN": "1"}, "True True False"),
                        ({"BT_BENCH_CHILD": "1"}, "False False True")):
        env = {k: v for k, v in os.environ.items() if k not in ("BT_CHAIN", "BT_BENCH_CHILD")}
        env.update(extra)
        out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, check=True, capture_output=True, text=True).stdout
        assert out.strip().splitlines()[-1] == want, (extra, out)
