#!/usr/bin/env python
"""Records what the split-precision host dispatch PLANS, without a GPU.

With ``bt_debug_plan_only(1)`` the library's ``launch_kernel`` records the kernel name and returns before it touches the runtime, so a
forward call with made-up, 16-byte aligned addresses (never dereferenced on the host) runs eligibility, tile planner and
instantiation choice and leaves the plan in ``bt_last_kernel_name`` / ``bt_last_launch_info``. This tool sweeps the four conv2d /
linear entry points over a grid of layer shapes for every variant of the chain and writes one line per case::

    variant|case|return code|kernel name|the 16 launch-info integers

``tests/test_split_plan_parity.py`` replays it against ``tests/golden/split_plans.txt`` (full records: two cases per kernel name
reached, plus the boundary cases) and ``tests/golden/split_plans_sha256.json`` (one SHA-256 per variant over the whole sweep's text).

    python tools/record_split_plans.py --dump FILE      # the whole text: diff two trees when a digest differs
    python tools/record_split_plans.py --write-golden   # re-record tests/golden/ (only when a plan is MEANT to change)

BT_LIB_PATH selects another build of the library.
"""
import argparse
import ctypes as C
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN_TABLE = os.path.join(ROOT, "tests", "golden", "split_plans.txt")
GOLDEN_SHA = os.path.join(ROOT, "tests", "golden", "split_plans_sha256.json")

P = 0x10000000          # any non-null, 16-byte aligned address
MAX_ELEMS = 1 << 28
POOL_MAX_3x3_S2_P1 = 1

# (name, Flipout, contraction mode, packed draws)
VARIANTS = (("reparam", False, 0, False), ("reparam-bf16x2", False, 2, False), ("reparam-bf16", False, 3, False), ("reparam-packed", False, 0, True),
            ("flipout", True, 0, False), ("flipout-packed", True, 0, True))


def conv_cases():
    """The swept grid: (Ci, Co, k, stride, padding, H, B, S, pool, x_sample_stride != 0)."""
    for Ci, Co, k, st in itertools.product((3, 8, 64, 128, 256, 512), (32, 64, 256), (1, 3, 7), (1, 2)):
        for pad in sorted({0, k // 2}):
            for H, B, S in itertools.product((1, 2, 4, 8, 14, 16, 32, 56), (1, 4, 32, 128, 256), (1, 2, 16)):
                Ho = (H + 2 * pad - k) // st + 1
                if Ho <= 0 or max(B * Ci * H * H, B * Co * Ho * Ho) > MAX_ELEMS:
                    continue
                yield (Ci, Co, k, st, pad, H, B, S, 0, 0)
                if Ci == 3:   # the stems' fused pool epilogue, over a shared and a per-sample input
                    yield (Ci, Co, k, st, pad, H, B, S, 1, 0)
                    yield (Ci, Co, k, st, pad, H, B, S, 1, 1)


# Boundary cases, recorded in full: the 32-channel tiles forced off / on, the row tile (256 -> 256 3x3 on 2x2 maps, B 128), Linear.
BN32_CASES = [(Ci, Co, k, 1, k // 2, H, B, S, 0, 0) for Ci, Co, k, H, B, S in
              itertools.product((64, 256), (32, 64, 256), (1, 3), (1, 2, 4, 8), (32, 128), (1, 16))]
ROW_TILE_CASE = (256, 256, 3, 1, 1, 2, 128, 2, 0, 0)
LINEAR_CASES = [(B, In, Out, S) for B, In, Out, S in itertools.product((8, 128), (64, 512), (10, 256), (2,))]


class Recorder:
    def __init__(self):
        from bayesian_torch_amd import _lib
        self.L, self.m = _lib.lib(), _lib
        self.h = C.CDLL(_lib.LIB_PATH)      # the bt_debug_* hooks are outside include/bt_hip.h
        self.info = (C.c_int64 * 16)()
        self.lines = {}                     # variant -> [line]
        self.pool_ep = m_ep = self.m.bt_epilogue(None, None, None, 0, 1, POOL_MAX_3x3_S2_P1)
        self.pool_ref = C.byref(m_ep)

    def _draws(self, flip, packed, inject=False):
        """The draws of a call: on chip, packed images (``packed``) or the natural layout (``inject``)."""
        m = self.m
        if not (packed or inject):
            return m.bt_draws(None, None, None, None, m.bt_rng(1, None, 0, 1, 0, 0))
        flags = (m.DRAWS_EPS_PACKED | (m.DRAWS_SIGNS_PACKED if flip else 0)) if packed else 0
        return m.bt_draws(P, P, P if flip else None, P if flip else None, m.bt_rng(1, None, 0, 1, 0, flags))

    def _record(self, rc):
        """What follows ``variant|case|rc|`` in a line."""
        if rc != 0:
            return "-|-"
        self.L.bt_last_launch_info(self.info, 16)
        return "%s|%s" % (self.L.bt_last_kernel_name().decode(), ",".join(str(int(v)) for v in self.info))

    def _call(self, variant, key, fn, head, geom, S, flip, packed, pool, xss, inject=False, packs=True, x=P):
        m, L = self.m, self.L
        par = m.bt_params(P, P, P, P, P, P, P, P, P if packs else None, P if packs else None, 0, 0)
        draws = self._draws(flip, packed, inject)
        ws_bytes = m.WORKSPACE_BYTES + int(L.bt_fused_scratch_bytes(C.byref(geom), S))
        rc = fn(*head, S, x, xss, C.byref(par), C.byref(draws), self.pool_ref if pool else None, P, P, P, ws_bytes, None)
        self.lines[variant].append("%s|%s|%d|%s" % (variant, key, rc, self._record(rc)))

    def conv(self, variant, flip, packed, case, tag=""):
        Ci, Co, k, st, pad, H, B, S, pool, per_sample = case
        geom = self.m.bt_conv2d_geom(B, Ci, H, H, Co, k, k, st, st, pad, pad, 1, 1, 1)
        fn = self.L.bt_flipout_conv2d_fwd if flip else self.L.bt_reparam_conv2d_fwd
        key = "%sconv Ci%d Co%d k%d s%d p%d H%d B%d S%d pool%d xs%d" % (tag, Ci, Co, k, st, pad, H, B, S, pool, per_sample)
        self._call(variant, key, fn, (C.byref(geom),), geom, S, flip, packed, pool, B * Ci * H * H if per_sample else 0)

    def linear(self, variant, flip, packed, case):
        B, In, Out, S = case
        geom = self.m.bt_conv2d_geom(B, In, 1, 1, Out, 1, 1, 1, 1, 0, 0, 1, 1, 1)
        fn = self.L.bt_flipout_linear_fwd if flip else self.L.bt_reparam_linear_fwd
        self._call(variant, "linear B%d In%d Out%d S%d" % (B, In, Out, S), fn, (B, In, Out), geom, S, flip, packed, 0, 0)

    def sweep(self):
        L, h = self.L, self.h
        cases = list(conv_cases())
        before, spw = L.bt_get_contraction(), os.environ.get("BT_QUAD_SPW")
        # The stems' sample walk is planned from the device's CU count: BT_QUAD_SPW=1 (read at every launch) keeps every stem on the
        # one-sample path, which is what a machine without a device plans anyway -- the records do not depend on where they are made.
        os.environ["BT_QUAD_SPW"] = "1"
        h.bt_debug_plan_only(1)
        try:
            for variant, flip, mode, packed in VARIANTS:
                self.lines[variant] = []
                assert L.bt_set_contraction(mode) == 0
                for case in cases:
                    self.conv(variant, flip, packed, case)
                self.conv(variant, flip, packed, ROW_TILE_CASE, tag="rowtile ")
                for case in LINEAR_CASES:
                    self.linear(variant, flip, packed, case)
                for force in (0, 1):
                    h.bt_debug_force_bn32(force)
                    for case in BN32_CASES:
                        self.conv(variant, flip, packed, case, tag="bn32=%d " % force)
                    h.bt_debug_force_bn32(-1)
        finally:
            h.bt_debug_force_bn32(-1)
            h.bt_debug_plan_only(0)
            L.bt_set_contraction(before)
            if spw is None:
                del os.environ["BT_QUAD_SPW"]
            else:
                os.environ["BT_QUAD_SPW"] = spw
        return self.lines


def record():
    return Recorder().sweep()


def digests(lines):
    return {v: hashlib.sha256(("\n".join(ls) + "\n").encode()).hexdigest() for v, ls in lines.items()}


def name_of(line):
    return line.split("|")[3]


def table(lines):
    """The committed full records: the first and the last case of every kernel name a variant reaches, and the boundary cases."""
    rows = []
    for ls in lines.values():
        first, last = {}, {}
        for i, ln in enumerate(ls):
            first.setdefault(name_of(ln), i)
            last[name_of(ln)] = i
        keep = set(first.values()) | set(last.values())
        keys = [ln.split("|")[1] for ln in ls]
        keep |= {i for i, k in enumerate(keys) if k.startswith(("rowtile", "linear"))}
        keep |= set([i for i, k in enumerate(keys) if k.startswith("bn32=")][::16])
        rows += [ls[i] for i in sorted(keep)]
    return rows


FAMILIES = ("fused_fwd_kernel", "fused_fast_kernel", "fused_split_kernel", "fused_split_quad_kernel", "fused_split_direct_kernel", "fused_split_skinny_kernel")


def _terms(np_, flip):
    """split_terms of bt_fused_split_launch.h."""
    return "2x6" if flip else {3: "6", 2: "3", 1: "1"}[np_]


def library_names(lib_path):
    """family -> the set of names its instantiations run under, for the six forward-kernel families of the library: from the symbol
    table's host stubs, through the name builders of bt_fused_split_launch.h (split_kernel_names and its neighbours) and the
    snprintf calls of bt_fused_dispatch.h, bt_fused_lowrank.hip and bt_fused_flipout_obs.hip. A skinny stub runs under two names
    (split-K 64 and 128: both are entries); a low-rank name is keyed without its run-time ``,R=``. -> (names, number of stubs)."""
    import re
    import shutil
    import subprocess
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "nm (binutils) or llvm-nm is needed to list the library's kernels"
    out = subprocess.run([nm, "-C", lib_path], check=True, capture_output=True, text=True).stdout
    names = {f: set() for f in FAMILIES}
    word = {"true": 1, "false": 0}
    stubs = set(re.findall(r"__device_stub__(fused_[a-z_]+_kernel)<([^>]*)>", out))
    n_stubs = {f: 0 for f in FAMILIES}
    for kind, targs in stubs:
        if kind not in names:
            continue
        n_stubs[kind] += 1
        t = [word[v] if v in word else int(v) for v in (s.strip() for s in targs.split(","))]
        add = names[kind].add
        if kind in ("fused_fwd_kernel", "fused_fast_kernel"):
            # <BN, BM, CWN, FLIP, LINEAR, TRANS, INJ, then fwd: UPD, DWIN, LOWRANK, OBS; fast: XMODE, NPW, POOL>
            form = "%s,%s" % ("linear" if t[4] else "conv", "trans" if t[5] else "notrans")
            if kind == "fused_fast_kernel":
                add("fused_fast_kernel<%d,%d,%d,%s,%s,inj=%d,xmode=%d,npw=%d,pool=%d>" % (t[0], t[1], t[2], "flip" if t[3] else "reparam", form, t[6], t[7], t[8], t[9]))
            else:
                upd, dwin, lowrank, obs = (t[7:] + [0, 0, 0, 0])[:4]
                src = "lowrank" if lowrank else "flip" if t[3] else "reparam"
                add("fused_fwd_kernel<%d,%d,%d,%s,%s,inj=%d%s>" % (t[0], t[1], t[2], src, form, t[6], ",obs" if obs else ",dwin" if dwin else ",updil" if upd else ""))
        elif kind == "fused_split_kernel":      # <BN, BM, NP, NPW, XM, FLIP, INJ>
            add("fused_split_kernel<%d,%d,bf16x%d,%s terms%s,npw=%d,xm=%d%s>" % (t[0], t[1], t[2], _terms(t[2], t[5]), ",flip" if t[5] else "", t[3], t[4], ",inj" if t[6] else ""))
        elif kind == "fused_split_quad_kernel":      # <NP, POOL, FLIP, WALK, INJ>
            add("fused_split_quad_kernel<64,%d,bf16x%d,%s terms%s,pool=%d%s%s>" % (256 if t[2] else 512, t[0], _terms(t[0], t[2]), ",flip" if t[2] else "", t[1],
                                                                                    ",walk" if t[3] else "", ",inj" if t[4] else ""))
        elif kind == "fused_split_direct_kernel":      # <RESIDENT, INJ, NP>
            add("fused_split_direct_kernel<64,8x64,bf16x%d,%s terms,%s W%s>" % (t[2], _terms(t[2], 0), "resident" if t[0] else "streamed", ",inj" if t[1] else ""))
        else:      # fused_split_skinny_kernel<INJ>: the launch's K slice is an argument, the name says which
            for ks in (64, 128):
                add("fused_split_skinny_kernel<64,4x32,bf16x3,6 terms,split-K %d%s>" % (ks, ",inj" if t[0] else ""))
    return names, n_stubs


def lowrank_key(name):
    """A low-rank launch's name without its run-time rank: the key ``library_names`` lists it under."""
    import re
    return re.sub(r",R=\d+>$", ">", name)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dump", metavar="FILE", help="write the whole sweep's text")
    ap.add_argument("--write-golden", action="store_true", help="re-record tests/golden/split_plans.txt and split_plans_sha256.json")
    args = ap.parse_args()
    lines = record()
    names = sorted({name_of(ln) for ls in lines.values() for ln in ls} - {"-"})
    print("%d cases, %d kernel names (%d split-precision)" % (sum(map(len, lines.values())), len(names), sum(n.startswith("fused_split_") for n in names)))
    for v, d in digests(lines).items():
        print("%-16s %s" % (v, d))
    if args.dump:
        with open(args.dump, "w") as f:
            for ls in lines.values():
                f.write("\n".join(ls) + "\n")
    if args.write_golden:
        with open(GOLDEN_TABLE, "w") as f:
            f.write("\n".join(table(lines)) + "\n")
        with open(GOLDEN_SHA, "w") as f:
            json.dump(digests(lines), f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
