#!/usr/bin/env python
"""Records what the training backward PLANS, without a GPU: ``bt_conv2d_bwd`` / ``bt_conv2d_bwd_kl`` (the sibling of
``record_seg_launches.py`` for csrc/bt_bwd.hip and its host plan, csrc/bt_bwd_plan.h).

With ``bt_debug_plan_only(1)`` ``launch_kernel`` launches nothing and leaves grid, block, LDS and a digest of the kernel's arguments;
the backward's argument block is digested by what it means -- its pointers, then every scalar, in a fixed order -- not by its bytes.
``bt_debug_last_launch_record`` counts the plan-only launches of a call and chains their records (a backward launches one to four
times). The addresses are made up (never dereferenced on the host); ``bt_params`` / ``bt_draws`` are the real structs. One line per call::

    entry point|case|return code|error text|launches|chain digest|bt_conv2d_bwd_workspace (- where the geometry itself is refused)

``tests/test_bwd_launch_parity.py`` replays the sweep against ``tests/golden/bwd_launches.txt`` (every line) and
``tests/golden/bwd_launches_sha256.json`` (one SHA-256 per entry point).

    python tools/record_bwd_launches.py --dump FILE      # the whole text: diff two trees when a line differs
    python tools/record_bwd_launches.py --write-golden   # re-record tests/golden/ (only when a launch is MEANT to change)

BT_LIB_PATH selects another build of the library.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
GOLDEN_TABLE = os.path.join(ROOT, "tests", "golden", "bwd_launches.txt")
GOLDEN_SHA = os.path.join(ROOT, "tests", "golden", "bwd_launches_sha256.json")

ENTRIES = ("bt_conv2d_bwd", "bt_conv2d_bwd_kl")
P = 0x10000000
WANTS = ("dx", "w", "both")
TARGETS = ((128, 256), (256, 512), (512, 1024), (1, 1))


def addr(pos):
    """A non-null, 16-byte aligned address of its own for tensor position ``pos``."""
    return P + (pos << 24)


def conv(B, Ci, H, W, Co, k=1, s=1, p=0, d=1, G=1):
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = pair(k), pair(s), pair(p), pair(d)
    return (B, Ci, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, G)


def draw_row_geoms():
    """The seven DRAW_ROWS of tests/_grad_cases.py (their comments name the splits each one reaches)."""
    from _grad_cases import DRAW_ROWS as rows
    out = []
    for rid, _, ctor, xs, S in rows:
        if "in_features" in ctor:
            g = conv(xs[0], ctor["in_features"], 1, 1, ctor["out_features"])
        else:
            g = conv(xs[0], ctor["in_channels"], xs[2], xs[3], ctor["out_channels"], ctor.get("kernel_size", 1), ctor.get("stride", 1),
                     ctor.get("padding", 0), ctor.get("dilation", 1), ctor.get("groups", 1))
        out.append(("row" + rid, g, S))
    return out


def resnet18_cifar(B):
    """The 21 Bayesian layers of ResNet-18 on 32 x 32 inputs: the stem, four stages of two blocks (a 1x1 stride-2 shortcut from the second on), the head."""
    out, c, hw = [("stem", conv(B, 3, 32, 32, 64, 3, 1, 1))], 64, 32
    for stage, co in enumerate((64, 128, 256, 512), 1):
        for block in range(2):
            s = 2 if stage > 1 and block == 0 else 1
            out.append(("l%d.%d.conv1" % (stage, block), conv(B, c, hw, hw, co, 3, s, 1)))
            if s == 2:
                out.append(("l%d.%d.down" % (stage, block), conv(B, c, hw, hw, co, 1, 2, 0)))
            hw //= s
            out.append(("l%d.%d.conv2" % (stage, block), conv(B, co, hw, hw, co, 3, 1, 1)))
            c = co
    out.append(("fc", conv(B, 512, 1, 1, 10)))
    assert len(out) == 21
    return out


def geometries():
    """(case, geometry, S) of the sweep."""
    gs = draw_row_geoms()
    gs += [("r18 b128 " + n, g, 1) for n, g in resnet18_cifar(128)] + [("r18 b8 " + n, g, 4) for n, g in resnet18_cifar(8)]
    gs += [("linear 4096->130", conv(6, 4096, 1, 1, 130), 3)]
    gs += [("groups2", conv(4, 32, 8, 8, 64, 3, 1, 1, 1, 2), 2), ("groups4", conv(4, 32, 8, 8, 64, 3, 2, 1, 1, 4), 1)]
    gs += [("stride2", conv(4, 24, 9, 9, 40, 3, 2, 1), 2), ("dilation2", conv(4, 24, 9, 9, 40, 3, 1, 2, 2), 2),
           ("rect 1x5", conv(3, 20, 6, 11, 36, (1, 5), (1, 2), (0, 2)), 2), ("rect 5x2", conv(3, 20, 11, 6, 36, (5, 2), (2, 1), (2, 0), (1, 2)), 1)]
    gs += [("Cig%d" % c, conv(4, c, 6, 6, 40, 3, 1, 1), 2) for c in (1, 3, 4, 5, 130)]
    gs += [("Cog%d" % c, conv(2, 16, 4, 4, c, 3, 1, 1), 1) for c in (16, 31, 32, 33, 64, 65, 136)]
    gs += [("M%d" % m, conv(1, 16, 1, m, 24, 1), 1) for m in (15, 16, 17, 127, 128, 129)] + [("M245", conv(5, 16, 7, 7, 24, 3, 1, 1), 1)]
    return gs


class Recorder:
    def __init__(self):
        from bayesian_torch_amd import _lib
        self.m, self.L = _lib, _lib.lib()
        self.h = C.CDLL(_lib.LIB_PATH)      # the bt_debug_* hooks are outside include/bt_hip.h
        self.h.bt_debug_last_launch_record.argtypes = [C.POINTER(C.c_int64), C.c_int]
        self.rec = (C.c_int64 * 11)()
        self.lines = {e: [] for e in ENTRIES}

    def call(self, case, geom, S, want="both", flip=False, kl=False, inject=False, query=True, ws=None, edit=None, stride=None, null=()):
        """One backward call. want: the gradients asked for; kl: through bt_conv2d_bwd_kl with a grad_kl; inject: supplied draws;
        query False: the line does not hold bt_conv2d_bwd_workspace (a geometry the query itself refuses); ws: (pointer, bytes) in place
        of a workspace of exactly the queried size; edit(params, draws, args): the case's own change; null: arguments passed as NULL."""
        m = self.m
        g = m.bt_conv2d_geom(*geom)
        B, Ci, H, W = geom[:4]
        need = int(self.L.bt_conv2d_bwd_workspace(C.byref(g), S)) if query else 0
        p = m.bt_params()
        p.mu_w, p.rho_w, p.prior_mu_w, p.prior_sigma_w, p.mu_packed, p.sigma_packed = addr(1), addr(2), addr(3), addr(4), addr(5), addr(6)
        d = m.bt_draws()
        d.rng.seed, d.rng.call, d.rng.layer_id, d.rng.sample0, d.rng.call_base_dev = 0x1234567890ABCDEF, 7, 3, 2, addr(7)
        if inject:
            d.eps_w = addr(8)
            if flip:
                d.sign_in, d.sign_out = addr(9), addr(10)
        a = dict(x=addr(11), gout=addr(12), gkl=addr(13), dx=addr(14) if want in ("dx", "both") else None,
                 dmu=addr(15) if want in ("w", "both") else None, drho=addr(16) if want in ("w", "both") else None,
                 ws=addr(17), ws_bytes=need, stride=B * Ci * H * W if stride is None else stride, g=C.byref(g), p=C.byref(p), d=C.byref(d))
        if ws is not None:
            a["ws"], a["ws_bytes"] = ws
        for k in null:
            a[k] = None
        if edit:
            edit(p, d, a)
        entry = ENTRIES[1 if kl else 0]
        head = (a["g"], S, 1 if flip else 0, a["x"], a["stride"], a["gout"], a["p"], a["d"])
        tail = (a["dx"], a["dmu"], a["drho"], a["ws"], a["ws_bytes"], None)
        self.h.bt_debug_last_launch_record(self.rec, 11)      # (drains the count and the chain)
        rc = getattr(self.L, entry)(*head, *(((a["gkl"],) if kl else ()) + tail))
        self.h.bt_debug_last_launch_record(self.rec, 11)
        err = self.L.bt_last_error_string().decode() if rc else "-"
        self.lines[entry].append("%s|%s|%d|%s|%d|%016x|%s" % (entry, case, rc, err, self.rec[9], self.rec[10] & 0xFFFFFFFFFFFFFFFF, need if query else "-"))

    def sweep_geometries(self):
        for case, geom, S in geometries():
            for pair in (1, 0):
                self.h.bt_debug_bwd_pair(pair)
                for flip in (False, True):
                    for want in WANTS:
                        for kl in (False, True):
                            self.call("%s S%d %s %s %s" % (case, S, "flipout" if flip else "reparam", want, "paired" if pair else "unpaired"), geom, S, want, flip, kl)
        self.h.bt_debug_bwd_pair(1)

    def sweep_targets(self):
        some = [t for t in geometries() if t[0].startswith(("row", "r18 b128 l1.0", "r18 b128 l4.1", "r18 b8 l3.0", "r18 b128 fc", "Cog136", "M245", "groups2"))]
        for wt, dt in TARGETS:
            self.h.bt_debug_bwd_targets(wt, dt)
            for case, geom, S in some:
                for pair in (1, 0):
                    self.h.bt_debug_bwd_pair(pair)
                    for want in WANTS:
                        self.call("targets %d/%d %s S%d %s %s" % (wt, dt, case, S, want, "paired" if pair else "unpaired"), geom, S, want, flip=S > 1, kl=want != "dx")
        self.h.bt_debug_bwd_targets(0, 0)
        self.h.bt_debug_bwd_pair(1)

    def sweep_refusals(self):
        rowA, rowC = geometries()[0], geometries()[2]      # A: dgrad in three pieces (its own workspace check); C: one piece, Flipout
        for case, geom, S in (rowA, rowC):
            need = int(self.L.bt_conv2d_bwd_workspace(C.byref(self.m.bt_conv2d_geom(*geom)), S))
            for want in WANTS:
                for kl in (False, True):
                    self.call("%s %s null workspace" % (case, want), geom, S, want, kl=kl, ws=(None, need))
                    self.call("%s %s workspace one byte short" % (case, want), geom, S, want, kl=kl, ws=(addr(17), need - 1))
                    self.call("%s %s workspace one byte more" % (case, want), geom, S, want, kl=kl, ws=(addr(17), need + 1))
            for flip in (False, True):      # supplied draws; x shared by the samples
                for want in WANTS:
                    self.call("%s %s %s injected" % (case, "flipout" if flip else "reparam", want), geom, S, want, flip, kl=want == "w", inject=True)
                    self.call("%s %s %s shared x" % (case, "flipout" if flip else "reparam", want), geom, S, want, flip, stride=0)
        case, geom, S = rowC
        for kl in (False, True):
            for k in ("g", "x", "gout", "p", "d"):
                self.call("null %s" % k, geom, S, kl=kl, null=(k,))
            for f in ("mu_packed", "sigma_packed", "rho_w"):
                self.call("null %s" % f, geom, S, kl=kl, edit=lambda p, d, a, f=f: setattr(p, f, None))
            for f in ("mu_packed", "sigma_packed"):
                for off in (4, 8):
                    self.call("%s off by %d bytes" % (f, off), geom, S, kl=kl, edit=lambda p, d, a, f=f, off=off: setattr(p, f, getattr(p, f) + off))
            self.call("misaligned pack and bad groups", geom[:13] + (3,), S, kl=kl, query=False, edit=lambda p, d, a: setattr(p, "mu_packed", p.mu_packed + 4))
            self.call("dmu without drho", geom, S, kl=kl, null=("drho",))
            self.call("drho without dmu", geom, S, kl=kl, null=("dmu",))
            self.call("no gradient asked for", geom, S, kl=kl, null=("dx", "dmu", "drho"))
            for flip in (False, True):
                self.call("eps_w alone, flip %d" % flip, geom, S, flip=flip, kl=kl, edit=lambda p, d, a: setattr(d, "eps_w", addr(8)))
                self.call("signs alone, flip %d" % flip, geom, S, flip=flip, kl=kl, edit=lambda p, d, a: (setattr(d, "sign_in", addr(9)), setattr(d, "sign_out", addr(10))))
                self.call("eps_w and one sign, flip %d" % flip, geom, S, flip=flip, kl=kl, edit=lambda p, d, a: (setattr(d, "eps_w", addr(8)), setattr(d, "sign_in", addr(9))))
            self.call("groups not dividing Ci", geom[:13] + (3,), S, kl=kl, query=False)
            self.call("groups not dividing Co", conv(4, 16, 7, 7, 26, 3, 2, 1, 1, 4), S, kl=kl, query=False)
            self.call("S = 0", geom, 0, kl=kl, query=False)
            self.call("S = -1", geom, -1, kl=kl, query=False)
            self.call("groups = 0", geom[:13] + (0,), S, kl=kl, query=False)
            self.call("empty output", conv(2, 4, 1, 1, 4, 3), S, kl=kl, query=False)
            self.call("empty output, wide", conv(2, 4, 5, 2, 4, 3), S, kl=kl, query=False)
            self.call("x of 2^31 elements", conv(2, 1024, 1024, 1024, 4, 1), 1, kl=kl, query=False)
            self.call("x one row below 2^31 elements", conv(1, 2047, 1024, 1024, 4, 1), 1, "w", kl=kl)
            self.call("out of 2^31 elements", conv(2, 4, 1024, 1024, 1024, 1), 1, kl=kl, query=False)
            self.call("weights of 2^29 elements", conv(1, 32768, 1, 1, 16384, 1), 1, kl=kl, query=False)
        for f in ("mu_w", "prior_mu_w", "prior_sigma_w"):
            for lap in (0, 1):
                self.call("kl: null %s, prior_kind %d" % (f, lap), geom, S, kl=True, edit=lambda p, d, a, f=f, lap=lap: (setattr(p, f, None), setattr(p, "prior_kind", lap)))
        self.call("kl: laplace", geom, S, kl=True, edit=lambda p, d, a: setattr(p, "prior_kind", 1))
        self.call("kl: null grad_kl is the plain backward", geom, S, kl=True, null=("gkl",))
        self.call("kl: dx only", geom, S, "dx", kl=True)

    def sweep(self):
        self.h.bt_debug_plan_only(1)
        try:
            self.sweep_geometries()
            self.sweep_targets()
            self.sweep_refusals()
        finally:
            self.h.bt_debug_plan_only(0)
            self.h.bt_debug_bwd_targets(0, 0)
            self.h.bt_debug_bwd_pair(1)
        return self.lines


def record():
    """entry point -> its lines."""
    return Recorder().sweep()


def digests(lines):
    return {e: hashlib.sha256("".join(ln + "\n" for ln in ls).encode()).hexdigest() for e, ls in lines.items()}


def table(lines):
    return [ln for e in ENTRIES for ln in lines[e]]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dump", metavar="FILE", help="write the whole sweep's text")
    ap.add_argument("--write-golden", action="store_true", help="re-record tests/golden/bwd_launches.txt and bwd_launches_sha256.json")
    args = ap.parse_args()
    lines = record()
    text = "\n".join(table(lines)) + "\n"
    print("%d calls, %d refused" % (len(table(lines)), sum(ln.split("|")[2] != "0" for ln in table(lines))))
    for e, d in digests(lines).items():
        print("%-24s %s" % (e, d))
    if args.dump:
        with open(args.dump, "w") as f:
            f.write(text)
    if args.write_golden:
        with open(GOLDEN_TABLE, "w") as f:
            f.write(text)
        with open(GOLDEN_SHA, "w") as f:
            json.dump(digests(lines), f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
