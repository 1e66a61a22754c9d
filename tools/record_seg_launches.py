#!/usr/bin/env python
"""Records what the segmented launches PLAN, without a GPU: ``bt_kl_normal``, ``bt_kl_hier``, ``bt_kl_hier_bwd``,
``bt_kl_normal_bwd_segs`` and ``bt_pack_sync`` / ``bt_pack_sync_kl`` (the sibling of ``record_fp32_plans.py`` for the launches that
hand a list of tensors to one grid).

With ``bt_debug_plan_only(1)`` ``launch_kernel`` launches nothing and leaves grid, block, LDS and a digest of the kernel's arguments;
a segmented argument block is digested by what it means -- per segment its pointers, ``n`` and first block, then the table's tail
and the block's scalars -- not by its bytes, so the record does not depend on how the block is laid out. ``bt_debug_last_launch_record``
also counts the plan-only launches since it was last asked and chains their records (``bt_pack_sync_kl`` launches twice). The
addresses are made up (never dereferenced on the host), a different one for every tensor position and segment. One line per call::

    entry point|case|return code|error text|launches|chain digest

``tests/test_seg_launch_parity.py`` replays the sweep against ``tests/golden/seg_launches.txt`` (every line) and
``tests/golden/seg_launches_sha256.json`` (one SHA-256 per entry point).

    python tools/record_seg_launches.py --dump FILE      # the whole text: diff two trees when a line differs
    python tools/record_seg_launches.py --write-golden   # re-record tests/golden/ (only when a launch is MEANT to change)

BT_LIB_PATH selects another build of the library.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN_TABLE = os.path.join(ROOT, "tests", "golden", "seg_launches.txt")
GOLDEN_SHA = os.path.join(ROOT, "tests", "golden", "seg_launches_sha256.json")

P = 0x10000000
LENS = (1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
COUNTS = (1, 2, 3, 63, 64, 0, 65)
ENTRIES = ("bt_kl_normal", "bt_kl_hier", "bt_kl_hier_bwd", "bt_kl_normal_bwd_segs", "bt_pack_sync", "bt_pack_sync_kl")
MAX_SLOTS = 8000
VP = C.c_void_p


def addr(pos, seg):
    """A non-null, 16-byte aligned address of its own for tensor position ``pos`` of segment ``seg``."""
    return P + (pos << 24) + (seg << 12)


def lens_for(n, shift=0):
    return [LENS[(i + shift) % len(LENS)] for i in range(n)]


def layer_variants(n):
    yield "null", None
    yield "constant", [5] * n
    yield "pairs", [i // 2 for i in range(n)]
    if n > 1:
        yield "decreasing", [n - i for i in range(n)]


class Recorder:
    def __init__(self):
        from bayesian_torch_amd import _lib
        self.m, self.L = _lib, _lib.lib()
        self.h = C.CDLL(_lib.LIB_PATH)      # the bt_debug_* hooks are outside include/bt_hip.h
        self.h.bt_debug_last_launch_record.argtypes = [C.POINTER(C.c_int64), C.c_int]
        self.rec = (C.c_int64 * 11)()
        self.lines = {e: [] for e in ENTRIES}
        self.ws = _lib.WORKSPACE_BYTES

    def call(self, entry, case, *args):
        self.h.bt_debug_last_launch_record(self.rec, 11)      # (drains the count and the chain)
        rc = getattr(self.L, entry)(*args)
        self.h.bt_debug_last_launch_record(self.rec, 11)
        err = self.L.bt_last_error_string().decode() if rc else "-"
        self.lines[entry].append("%s|%s|%d|%s|%d|%016x" % (entry, case, rc, err, self.rec[9], self.rec[10] & 0xFFFFFFFFFFFFFFFF))

    # ------------------------------------------------------------------ the KL entry points
    def arrays(self, k, lens, null=None, first=0):
        """k pointer arrays over len(lens) segments (positions first..first+k) and the numel array. null: (position, segment) whose
        entry is NULL, or (position, None): the whole array is."""
        n = max(len(lens), 1)
        arrs = [(VP * n)(*[addr(first + p, i) for i in range(n)]) for p in range(k)]
        here = null is not None and first <= null[0] < first + k
        if here and null[1] is not None:
            arrs[null[0] - first][null[1]] = None
        out = [None if here and null[1] is None and null[0] - first == p else a for p, a in enumerate(arrs)]
        return out, (C.c_int64 * n)(*(list(lens) or [1]))

    def kl_call(self, entry, case, lens, lay=None, flags=0, null=None, nullarg=None, ws_bytes=None, priors=True, want=None):
        """One call of a KL entry point over segments of ``lens``. null: see arrays(); nullarg: a scalar argument passed as NULL
        ('numel', 'kl_out', 'seg_out', 'workspace', 'grad_kl'); priors False: the prior arrays are NULL (laplace gradients); want: the
        gradient arrays that are given (default: all)."""
        n = len(lens)
        nin = 7 if "hier" in entry else 4
        ins, numel = self.arrays(nin, lens, null)
        if not priors:
            ins[2] = ins[3] = None
        nm = None if nullarg == "numel" else numel
        layv = None if lay is None else (C.c_int32 * max(n, 1))(*lay)
        ws = None if nullarg == "workspace" else addr(30, 0)
        wsb = self.ws if ws_bytes is None else ws_bytes
        kl_out = None if nullarg == "kl_out" else addr(31, 0)
        g = None if nullarg == "grad_kl" else addr(32, 0)
        if entry == "bt_kl_normal":
            return self.call(entry, case, n, *ins, nm, layv, flags, kl_out, ws, wsb, None)
        if entry == "bt_kl_hier":
            return self.call(entry, case, n, *ins, nm, layv, kl_out, None if nullarg == "seg_out" else addr(33, 0), ws, wsb, None)
        outs, _ = self.arrays(4 if "hier" in entry else 2, lens, null, first=nin)
        if want is not None:
            outs = [a if p in want else None for p, a in enumerate(outs)]
        if entry == "bt_kl_hier_bwd":
            return self.call(entry, case, n, *ins, nm, g, *outs, None)
        return self.call(entry, case, n, *ins, nm, g, flags, *outs, None)

    def sweep_kl(self, entry, per_block, cap, slots):
        fwd, hier = "bwd" not in entry, "hier" in entry
        nin, nout = (7 if hier else 4), (0 if fwd else 4 if hier else 2)
        for n in COUNTS:
            for shift in (0, 5):
                self.kl_call(entry, "n%d shift%d" % (n, shift), lens_for(n, shift))
        for ln in LENS:
            self.kl_call(entry, "one len%d" % ln, [ln])
        if cap:     # the per-segment cap and one block past it; the workspace's slots and one segment past them
            for ln in (cap * per_block - 1, cap * per_block, cap * per_block + 1, cap * per_block + per_block + 1):
                self.kl_call(entry, "cap len%d" % ln, [ln, 5, ln])
            full = slots // cap
            for n in (full, full + 1):
                self.kl_call(entry, "slots %d segments at the cap" % n, [cap * per_block] * n)
            self.kl_call(entry, "slots overflow, then a null segment", [cap * per_block] * (full + 1) + [7], null=(1, full + 1))
            self.kl_call(entry, "slots overflow, decreasing layers", [cap * per_block] * (full + 1), lay=list(range(full + 1, 0, -1)))
        else:       # no cap: the grid's 2^31 - 1 blocks and one past them
            for ln in ((2 ** 31 - 1) * per_block, (2 ** 31 - 1) * per_block + 1):
                self.kl_call(entry, "grid len%d" % ln, [ln])
            self.kl_call(entry, "grid overflow in the second segment", [(2 ** 31 - 2) * per_block, 2 * per_block])
            self.kl_call(entry, "grid overflow, then a null segment", [(2 ** 31 - 1) * per_block + 1, 7], null=(1, 1))
        if fwd:
            for n in (1, 3, 64):
                for tag, lay in layer_variants(n):
                    self.kl_call(entry, "n%d layers %s" % (n, tag), lens_for(n), lay=lay)
        if not hier:
            for flags in (1, 2, 3):
                self.kl_call(entry, "flags%d" % flags, lens_for(3), flags=flags)
        if entry == "bt_kl_normal_bwd_segs":
            self.kl_call(entry, "laplace without priors", lens_for(3), flags=2, priors=False)
            self.kl_call(entry, "normal without priors", lens_for(3), flags=0, priors=False)
            self.kl_call(entry, "laplace, null prior entry", lens_for(3), flags=2, null=(2, 1))
        for pos in range(nin + nout):     # a null pointer in each argument position: the array, and one entry of it
            self.kl_call(entry, "null array %d" % pos, lens_for(3), null=(pos, None))
            self.kl_call(entry, "null entry %d of segment 1" % pos, lens_for(3), null=(pos, 1))
        if entry == "bt_kl_hier_bwd":
            for keep in range(4):        # one gradient asked for; none
                self.kl_call(entry, "only gradient %d" % keep, lens_for(3), want={keep})
            self.kl_call(entry, "no gradient", lens_for(3), want=())
        for what in ("numel",) + (("kl_out", "workspace") if fwd else ("grad_kl",)) + (("seg_out",) if entry == "bt_kl_hier" else ()):
            self.kl_call(entry, "null %s" % what, lens_for(3), nullarg=what)
        if fwd:
            self.kl_call(entry, "small workspace", lens_for(3), ws_bytes=self.ws - 1)
        self.kl_call(entry, "empty segment", [4, 0, 4])
        self.kl_call(entry, "negative segment", [4, -1, 4])

    # ------------------------------------------------------------------ the pack check
    def pack_call(self, entry, case, geoms, kl=None, bias=False, force=(), src=True, edit=None, ws_bytes=None, null_ws=False, null_segs=False):
        """geoms: [(Co, Ci, taps)]. kl: None, or the set of segments that ask for their KL (bias: with the bias tensors); force:
        segments with the force bit; src: src_mu / src_rho given; edit(segs, kls): the case's own change."""
        m, n = self.m, len(geoms)
        segs = (m.bt_pack_seg * max(n, 1))()
        kls = (m.bt_pack_kl * max(n, 1))()
        for i, (Co, Ci, taps) in enumerate(geoms):
            s = segs[i]
            s.mu_w, s.rho_w, s.mu_packed, s.sigma_packed, s.state = addr(0, i), addr(1, i), addr(4, i), addr(5, i), addr(6, i)
            if src:
                s.src_mu, s.src_rho = addr(2, i), addr(3, i)
            s.Co, s.Ci, s.taps, s.force = Co, Ci, taps, 1 if i in force else 0
            if kl is not None and i in kl:
                k = kls[i]
                k.prior_mu_w, k.prior_sigma_w, k.kl_out = addr(7, i), addr(8, i), addr(13, i)
                if bias:
                    k.mu_b, k.rho_b, k.prior_mu_b, k.prior_sigma_b, k.n_bias = addr(9, i), addr(10, i), addr(11, i), addr(12, i), Co
        if edit:
            edit(segs, kls)
        ws = None if null_ws else addr(30, 0)
        wsb = self.ws if ws_bytes is None else ws_bytes
        sp = None if null_segs else segs
        if entry == "bt_pack_sync":
            return self.call(entry, case, n, sp, ws, wsb, None)
        return self.call(entry, case, n, sp, None if kl is None else kls, ws, wsb, None)

    def sweep_pack(self, entry):
        with_kl = entry == "bt_pack_sync_kl"
        shapes = [(1, 1, 1), (1, 3, 1), (2, 2, 1), (5, 51, 1), (16, 16, 1), (257, 1, 1), (11, 93, 1), (16, 64, 1), (25, 41, 1), (45, 91, 1),
                  (64, 64, 1), (17, 241, 1), (3, 2731, 1)]      # Co * Ci: the swept lengths
        ways = [("", None, False)] + ([(" kl", "all", False), (" kl+bias", "all", True), (" kl even", "even", True)] if with_kl else [])
        for n in COUNTS:
            for tag, which, bias in ways:
                kl = None if which is None else set(range(0, n, 2 if which == "even" else 1))
                self.pack_call(entry, "n%d%s" % (n, tag), [shapes[i % len(shapes)] for i in range(n)], kl=kl, bias=bias)
        for shp in shapes:
            for tag, which, bias in ways:
                self.pack_call(entry, "one %dx%dx%d%s" % (*shp, tag), [shp], kl=None if which is None else {0}, bias=bias)
        for tag, which, bias in ways:
            kl3, kl64 = (None, None) if which is None else ({0, 1, 2}, set(range(64)))
            for shp in ((512, 1023, 1), (512, 1024, 1), (1, 524289, 1), (513, 1024, 1)):       # 128 fingerprint blocks and past them
                self.pack_call(entry, "fp cap %dx%dx%d%s" % (*shp, tag), [shp, (2, 2, 1), shp], kl=kl3, bias=bias)
            for shp in ((255, 64, 9), (256, 64, 9), (257, 64, 9), (128, 65, 9), (129, 65, 9)):   # 256 pack items and past them
                self.pack_call(entry, "item cap %dx%dx%d%s" % (*shp, tag), [shp, (2, 2, 1), shp], kl=kl3, bias=bias)
            # 64 x 128 fingerprint blocks: more than the workspace's slots, which only a KL needs
            self.pack_call(entry, "slots 64 segments of 128 blocks%s" % tag, [(512, 1024, 1)] * 64, kl=kl64, bias=bias)
            self.pack_call(entry, "slots 63 segments of 128 blocks%s" % tag, [(512, 1024, 1)] * 63, kl=None if which is None else set(range(63)), bias=bias)
            if which is not None:
                self.pack_call(entry, "slots 64 segments of 128 blocks, one KL%s" % tag, [(512, 1024, 1)] * 64, kl={40}, bias=bias)
            for Ci in (1, 2, 3, 5, 63, 65, 66, 130):
                self.pack_call(entry, "Ci%d%s" % (Ci, tag), [(7, Ci, 9), (4, 8, 3)], kl=None if which is None else {0, 1}, bias=bias)
            for taps in (1, 9, 128, 129):
                self.pack_call(entry, "taps%d%s" % (taps, tag), [(8, 16, 9), (8, 16, taps)], kl=None if which is None else {0, 1}, bias=bias)
            for force in ((0,), (1,), (0, 2), (63,)):
                self.pack_call(entry, "force %s%s" % (",".join(map(str, force)), tag), [(4, 8, 3)] * 64, kl=kl64, bias=bias, force=force)
            self.pack_call(entry, "no src%s" % tag, [(4, 8, 3)] * 3, kl=kl3, bias=bias, src=False)
        fields = ("mu_w", "rho_w", "src_mu", "src_rho", "mu_packed", "sigma_packed", "state")
        for f in fields:
            self.pack_call(entry, "null %s of segment 1" % f, [(4, 8, 3)] * 3, edit=lambda s, k, f=f: setattr(s[1], f, None))
        for f in ("Co", "Ci", "taps"):
            for v in (0, -1):
                self.pack_call(entry, "%s=%d in segment 1" % (f, v), [(4, 8, 3)] * 3, edit=lambda s, k, f=f, v=v: setattr(s[1], f, v))
        self.pack_call(entry, "null segs", [(4, 8, 3)] * 3, null_segs=True)
        self.pack_call(entry, "null workspace", [(4, 8, 3)] * 3, null_ws=True)
        self.pack_call(entry, "small workspace", [(4, 8, 3)] * 3, ws_bytes=self.ws - 1)
        if with_kl:
            for f in ("prior_mu_w", "prior_sigma_w", "mu_b", "rho_b", "prior_mu_b", "prior_sigma_b", "kl_out"):
                self.pack_call(entry, "kl: null %s of segment 1" % f, [(4, 8, 3)] * 3, kl={0, 1, 2}, bias=True, edit=lambda s, k, f=f: setattr(k[1], f, None))
            for v in (0, -1, 1 << 30, (1 << 30) - 1):
                self.pack_call(entry, "kl: n_bias=%d in segment 1" % v, [(4, 8, 3)] * 3, kl={0, 1, 2}, bias=True, edit=lambda s, k, v=v: setattr(k[1], "n_bias", v))
            self.pack_call(entry, "kl: taps 129 refused before any launch", [(8, 16, 129)], kl={0}, bias=True)

    def sweep(self):
        self.h.bt_debug_plan_only(1)
        try:
            self.sweep_kl("bt_kl_normal", 4096, 1024, MAX_SLOTS)
            self.sweep_kl("bt_kl_hier", 4096, 2048, MAX_SLOTS)
            self.sweep_kl("bt_kl_hier_bwd", 1024, 0, 0)
            self.sweep_kl("bt_kl_normal_bwd_segs", 1024, 0, 0)
            self.sweep_pack("bt_pack_sync")
            self.sweep_pack("bt_pack_sync_kl")
        finally:
            self.h.bt_debug_plan_only(0)
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
    ap.add_argument("--write-golden", action="store_true", help="re-record tests/golden/seg_launches.txt and seg_launches_sha256.json")
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
