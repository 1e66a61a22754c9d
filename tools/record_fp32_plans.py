#!/usr/bin/env python
"""Records what the fp32-MFMA host dispatch PLANS, without a GPU: the sibling of ``record_split_plans.py`` for the launches the
split-precision chain does not take (``bt_set_contraction(1)``: fp32 everywhere; natural-layout injected draws; absent packs;
more than 9 taps; input-dilated launches; Linear).

A kernel name and the 16 launch-info integers do not pin an fp32 plan -- ``patch_ok``, ``mt_per_pixel``, ``x_rows``, ``x_cvec`` and the
alignment flags are read by the kernels and only some show in the name -- so with ``bt_debug_plan_only(1)`` ``launch_kernel`` also
leaves grid, block, LDS bytes, LDS limit and a 64-bit FNV-1a digest of the kernel's argument bytes (``bt_debug_last_launch_record``).
Same kernel, same grid / block / LDS, same argument bytes: the same launch. One line per call::

    variant|case|return code|kernel name|the 16 launch-info integers|grid,block,lds,lds_limit|argument digest

(a refusal: ``bt_last_error_string()`` in place of the name, ``-`` for the rest). ``tests/test_fp32_plan_parity.py`` replays it
against ``tests/golden/fp32_plans.txt`` (the first and the last case of every kernel name per variant, every refusal text once) and
``tests/golden/fp32_plans_sha256.json`` (one SHA-256 per variant over the whole text).

    python tools/record_fp32_plans.py --dump FILE      # the whole text: diff two trees when a digest differs
    python tools/record_fp32_plans.py --write-golden   # re-record tests/golden/ (only when a plan is MEANT to change)

BT_LIB_PATH selects another build of the library.
"""
import argparse
import ctypes as C
import hashlib
import itertools
import json
import os
import re
import shutil
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import record_split_plans as base   # noqa: E402
from record_split_plans import P, ROOT   # noqa: E402  (Recorder plumbing, name_of)

GOLDEN_TABLE = os.path.join(ROOT, "tests", "golden", "fp32_plans.txt")
GOLDEN_SHA = os.path.join(ROOT, "tests", "golden", "fp32_plans_sha256.json")
MAX_ELEMS = 1 << 26
VARIANTS = (("reparam", False), ("flipout", True))
# The four ways of a case: (tag, natural-layout injected draws, packs present, address of x)
WAYS = (("chip", False, True, P), ("inj", True, True, P), ("nopack", False, False, P), ("x+4", False, True, P + 4))


def conv_cases():
    """The swept grid: (Ci, Co, k, stride, dilation, groups, padding, H, B, S)."""
    for Ci, Co, k, st, dil, grp in itertools.product((3, 6, 8, 64, 256), (16, 32, 64, 256), (1, 2, 3, 7, 9, 12), (1, 2), (1, 2), (1, 2)):
        for pad in sorted({0, dil * (k // 2)}):
            for H, B, S in itertools.product((1, 2, 3, 4, 8, 16, 32, 56), (1, 2, 3, 4, 12, 32, 128, 200, 256), (1, 2, 16, 128)):
                Ho = (H + 2 * pad - dil * (k - 1) - 1) // st + 1
                if Ho <= 0 or max(B * Ci * H * H, B * Co * Ho * Ho) > MAX_ELEMS:
                    continue
                yield (Ci, Co, k, st, dil, grp, pad, H, B, S)


LINEAR_CASES = list(itertools.product((1, 8, 40, 128, 200, 300, 1024), (10, 64, 512), (10, 48, 256), (1, 2, 16, 32, 128)))
UPDIL = (2, 2, 1, 2, 1, 2)


class Sink:
    """One variant's lines, not kept (there are millions): the SHA-256 of the text, the first and the last record of every kernel
    name and the first of every refusal text (the committed table), the number of launches per kernel name."""

    def __init__(self, out=None):
        self.sha, self.first, self.last, self.count, self.n, self.out = hashlib.sha256(), {}, {}, {}, 0, out

    def append(self, line):
        self.sha.update(line.encode() + b"\n")
        f = line.split("|", 4)
        self.first.setdefault(f[3], (self.n, line))
        if f[2] == "0":
            self.last[f[3]] = (self.n, line)
            self.count[f[3]] = self.count.get(f[3], 0) + 1
        self.n += 1
        if self.out:
            self.out.write(line + "\n")

    def table(self):
        return [ln for _, ln in sorted(set(self.first.values()) | set(self.last.values()))]


class Fp32Recorder(base.Recorder):
    def __init__(self, out=None):
        super().__init__()
        self.out = out
        m = self.m
        self.rec = (C.c_int64 * 9)()
        self.h.bt_debug_last_launch_record.argtypes = [C.POINTER(C.c_int64), C.c_int]
        self.updil = m.bt_updil(*UPDIL)
        # the argument structs of every way, built once (the sweep makes some 4.6 million calls)
        self.keep = [m.bt_params(P, P, P, P, P, P, P, P, P if packs else None, P if packs else None, 0, 0) for packs in (False, True)]
        self.keep += [self._draws(flip, False, inj) for flip in (False, True) for inj in (False, True)]
        self.par = {packs: C.byref(self.keep[packs]) for packs in (False, True)}
        self.draws = {(flip, inj): C.byref(self.keep[2 + 2 * flip + inj]) for flip in (False, True) for inj in (False, True)}
        self.ws_bytes = m.WORKSPACE_BYTES
        self.fmt = "%s|" + ",".join(["%d"] * 16) + "|%d.%d.%d,%d.%d.%d,%d,%d|%016x"

    def _record(self, rc):
        if rc != 0:
            return "%s|-|-|-" % self.L.bt_last_error_string().decode()
        self.L.bt_last_launch_info(self.info, 16)
        self.h.bt_debug_last_launch_record(self.rec, 9)
        r = self.rec[:]
        r[8] &= 0xFFFFFFFFFFFFFFFF
        return self.fmt % (self.L.bt_last_kernel_name().decode(), *self.info[:], *r)

    def call(self, variant, key, fn, head, S, flip, way, pool=False, xss=0):
        tag, inj, packs, x = way
        rc = fn(*head, S, x, xss, self.par[packs], self.draws[flip, inj], self.pool_ref if pool else None, P, P, P, self.ws_bytes, None)
        self.lines[variant].append("%s|%s %s|%d|%s" % (variant, key, tag, rc, self._record(rc)))

    def conv(self, variant, flip, case, tag=""):
        Ci, Co, k, st, dil, grp, pad, H, B, S = case
        L = self.L
        geom = self.m.bt_conv2d_geom(B, Ci, H, H, Co, k, k, st, st, pad, pad, dil, dil, grp)
        fn, head = (L.bt_flipout_conv2d_fwd if flip else L.bt_reparam_conv2d_fwd), (C.byref(geom),)
        key = "%sconv Ci%d Co%d k%d s%d d%d g%d p%d H%d B%d S%d" % (tag, Ci, Co, k, st, dil, grp, pad, H, B, S)
        if tag:   # BT_FORCE_GENERIC: the on-chip way alone
            return self.call(variant, key, fn, head, S, flip, WAYS[0])
        for way in WAYS:
            self.call(variant, key, fn, head, S, flip, way)
        if Ci == 3:   # the stems' fused pool epilogue: a shared and a per-sample x, and the refusal with injected draws
            self.call(variant, key + " pool xs0", fn, head, S, flip, WAYS[0], pool=True)
            self.call(variant, key + " pool xs1", fn, head, S, flip, WAYS[0], pool=True, xss=B * Ci * H * H)
            self.call(variant, key + " pool xs0", fn, head, S, flip, WAYS[1], pool=True)
        if pad == 0 and k <= 3:   # the input-dilated entry points (on chip; injected draws and the pool are refused)
            fu, hu = (L.bt_flipout_conv2d_updil_fwd if flip else L.bt_reparam_conv2d_updil_fwd), (C.byref(geom), C.byref(self.updil))
            self.call(variant, key + " updil", fu, hu, S, flip, WAYS[0])
            if Ci == 3 and S == 1:
                self.call(variant, key + " updil", fu, hu, S, flip, WAYS[1])
                self.call(variant, key + " updil pool", fu, hu, S, flip, WAYS[0], pool=True)

    def linear(self, variant, flip, case):
        B, In, Out, S = case
        fn = self.L.bt_flipout_linear_fwd if flip else self.L.bt_reparam_linear_fwd
        for way in WAYS:
            self.call(variant, "linear B%d In%d Out%d S%d" % (B, In, Out, S), fn, (B, In, Out), S, flip, way)

    def sweep(self):
        L, h = self.L, self.h
        cases = list(conv_cases())
        before = L.bt_get_contraction()
        h.bt_debug_plan_only(1)
        h.bt_debug_force_generic(0)
        try:
            assert L.bt_set_contraction(1) == 0   # fp32 everywhere (mode 0's fp32 rows: record_split_plans.py)
            for variant, flip in VARIANTS:
                self.lines[variant] = Sink(self.out)
                for case in cases:
                    self.conv(variant, flip, case)
                for case in LINEAR_CASES:
                    self.linear(variant, flip, case)
                h.bt_debug_force_generic(1)
                for case in cases:
                    self.conv(variant, flip, case, tag="generic ")
                h.bt_debug_force_generic(0)
        finally:
            h.bt_debug_force_generic(1 if os.environ.get("BT_FORCE_GENERIC") is not None else 0)
            h.bt_debug_plan_only(0)
            L.bt_set_contraction(before)
        return self.lines


def record(out=None):
    """variant -> Sink. out: a text file that gets every line."""
    return Fp32Recorder(out).sweep()


def digests(sinks):
    return {v: s.sha.hexdigest() for v, s in sinks.items()}


def table(sinks):
    """The committed full records: the first and the last case of every kernel name a variant reaches, every refusal text once."""
    return [ln for s in sinks.values() for ln in s.table()]


def instantiated_names(lib_path):
    """The fp32 kernels the library holds, under the names the launchers give them: from the symbol table's host stubs."""
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "nm (binutils) or llvm-nm is needed to list the library's kernels"
    out = subprocess.run([nm, "-C", lib_path], check=True, capture_output=True, text=True).stdout
    names = set()
    word = {"true": 1, "false": 0}
    for kind, targs in re.findall(r"__device_stub__(fused_fwd_kernel|fused_fast_kernel)<([^>]*)>", out):
        t = [word[v] if v in word else int(v) for v in (s.strip() for s in targs.split(","))]
        head = "%d,%d,%d,%s,%s,%s" % (t[0], t[1], t[2], "flip" if t[3] else "reparam", "linear" if t[4] else "conv", "trans" if t[5] else "notrans")
        if kind == "fused_fwd_kernel":
            names.add("fused_fwd_kernel<%s,inj=%d%s>" % (head, t[6], ",updil" if t[7] else ""))
        else:
            names.add("fused_fast_kernel<%s,inj=%d,xmode=%d,npw=%d,pool=%d>" % (head, t[6], t[7], t[8], t[9]))
    return names


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dump", metavar="FILE", help="write the whole sweep's text")
    ap.add_argument("--write-golden", action="store_true", help="re-record tests/golden/fp32_plans.txt and fp32_plans_sha256.json")
    args = ap.parse_args()
    out = open(args.dump, "w") if args.dump else None
    t0 = time.perf_counter()
    sinks = record(out)
    dt = time.perf_counter() - t0
    if out:
        out.close()
    names = {n for s in sinks.values() for n in s.count}
    from bayesian_torch_amd import _lib
    have = instantiated_names(_lib.LIB_PATH)
    print("%d cases in %.2f s, %d kernel names, %d of the library's %d fp32 instantiations" %
          (sum(s.n for s in sinks.values()), dt, len(names), len(names & have), len(have)))
    for n in sorted(have - names):
        print("not reached:", n)
    for v, d in digests(sinks).items():
        print("%-16s %s" % (v, d))
    if args.write_golden:
        with open(GOLDEN_TABLE, "w") as f:
            f.write("\n".join(table(sinks)) + "\n")
        with open(GOLDEN_SHA, "w") as f:
            json.dump(digests(sinks), f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
