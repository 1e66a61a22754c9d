#!/usr/bin/env python
"""Finds, without a GPU, a cheap launch for every forward-kernel instantiation the library holds: the ledger behind
``tests/test_instantiation_ledger_host.py`` and ``tests/test_gpu_every_instantiation.py``.

``record_split_plans.library_names`` lists the names the six families' instantiations run under. Under ``bt_debug_plan_only(1)`` (the
recorders' seam: a call plans, names its kernel and returns before it touches the runtime) this tool searches the entry points --
conv2d and linear, Reparameterization and Flipout, the input-dilated and the depth-window entry points, the low-rank forward and the
Flipout observer -- over a grid that is finer and far smaller than the recorders' (Ci 3, 8, 16, 24, ..., Co from 8, every k in 1..7
and 12, small maps, B x S just large enough to reach a tile) and over the knobs that select a variant: contraction modes 0..3,
packed / natural-layout supplied draws, absent packs, x displaced by 4 bytes, ``bt_debug_force_bn32`` / ``bt_debug_force_generic``,
``BT_QUAD_SPW``, the pool epilogue over a shared and over a per-sample x. Per name it keeps

- ``min``: the planned case with the fewest multiply-accumulates (ties: the smaller x);
- ``ragged``: the cheapest case of the same name in min's neighbourhood (Co +- 0..8, B - 0..3, Ci +- 0..4, H + 0..1) whose Co is no
  multiple of the channel tile, whose B * Ho * Wo is no multiple of the pixel tile and whose Ci is no multiple of 8 -- with a bias and
  S >= 2 where the name admits one -- or null.

A case is a flat dict: the entry point, the knobs, the geometry and the MAC count (``CASE_KEYS``). The sample walk's plan reads the
device's CU count, so its row is stated (the stem of tests/test_gpu_stem_walk.py) and flagged ``needs_device``.

    python tools/find_instantiation_cases.py            # search and report
    python tools/find_instantiation_cases.py --write    # re-record tests/golden/instantiation_cases.json

BT_LIB_PATH selects another build of the library.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import record_split_plans as base   # noqa: E402
from record_split_plans import P, ROOT   # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "instantiation_cases.json")
MAC_CAP = 1 << 28
UPDIL = (2, 2, 1, 2, 1, 2)
LOWRANK_R = 2

# entry: conv | linear | updil | dwin | lowrank | obs.  draws: chip | packed | natural.  spw: BT_QUAD_SPW's value, or None (unset).
# dwin: (kd, D, sd, dd, pd) of a depth-window launch, else None: then Ci is the REAL tensor's channels per depth plane (x is [B, Ci * D, H, H]).
CASE_KEYS = ("entry", "flip", "mode", "draws", "packs", "x_off", "bn32", "generic", "spw", "pool", "per_sample_x", "bias",
             "Ci", "Co", "k", "st", "pad", "H", "B", "S", "dwin", "macs")
DEFAULTS = dict(entry="conv", flip=False, mode=0, draws="chip", packs=True, x_off=0, bn32=-1, generic=0, spw=None, pool=False, per_sample_x=False, bias=False,
                dwin=None)


def out_hw(c):
    """Output height (= width) of a case's launch, or 0."""
    if c["entry"] == "linear" or (c["entry"] == "obs" and c["k"] == 0):
        return 1
    H = c["H"]
    if c["entry"] == "updil":
        H = (H - 1) * UPDIL[0] + 1 + UPDIL[2] + UPDIL[3]
    v = H + 2 * c["pad"] - c["k"]
    return v // c["st"] + 1 if v >= 0 else 0


def depth_out(c):
    if c["dwin"] is None:
        return 1
    kd, D, sd, dd, pd = c["dwin"]
    v = D + 2 * pd - dd * (kd - 1) - 1
    return v // sd + 1 if v >= 0 else 0


def macs_of(c):
    """Multiply-accumulates of the contraction (Flipout runs two)."""
    Ho = out_hw(c)
    kk = max(c["k"], 1) ** 2 * (c["dwin"][0] if c["dwin"] else 1)
    return c["S"] * c["B"] * depth_out(c) * c["Co"] * Ho * Ho * c["Ci"] * kk * (2 if c["flip"] else 1)


def x_elems(c):
    D = c["dwin"][1] if c["dwin"] else 1
    return c["B"] * c["Ci"] * D * (1 if c["entry"] == "linear" or c["k"] == 0 else c["H"] * c["H"])


def make_case(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    assert set(c) | {"macs"} == set(CASE_KEYS), sorted(set(c) ^ set(CASE_KEYS))
    c["macs"] = macs_of(c)
    return c


class Planner(base.Recorder):
    """Plans a case through the C ABI with made-up addresses (never dereferenced: bt_debug_plan_only)."""

    def __init__(self):
        super().__init__()
        self.h.bt_debug_force_bn32.argtypes = [C.c_int]
        self.h.bt_debug_force_generic.argtypes = [C.c_int]
        self.scratch = self.L.bt_fused_scratch_bytes

    # ------------------------------------------------------------------ knobs
    def knobs(self, c):
        """Sets the process-wide knobs of a case -> what ``restore`` needs."""
        before = (self.L.bt_get_contraction(), os.environ.get("BT_QUAD_SPW"))
        if c["spw"] is None:
            os.environ.pop("BT_QUAD_SPW", None)
        else:
            os.environ["BT_QUAD_SPW"] = str(c["spw"])
        self.h.bt_debug_plan_only(1)
        self.h.bt_debug_force_bn32(c["bn32"])
        self.h.bt_debug_force_generic(c["generic"])
        assert self.L.bt_set_contraction(c["mode"]) == 0
        return before

    def restore(self, before):
        self.h.bt_debug_force_generic(1 if os.environ.get("BT_FORCE_GENERIC") is not None else 0)
        self.h.bt_debug_force_bn32(-1)
        self.h.bt_debug_plan_only(0)
        self.L.bt_set_contraction(before[0])
        if before[1] is None:
            os.environ.pop("BT_QUAD_SPW", None)
        else:
            os.environ["BT_QUAD_SPW"] = before[1]

    # ------------------------------------------------------------------ one call, the knobs already set
    def call(self, c):
        """-> the kernel name the case plans (a low-rank name without its rank), or None when the library refuses it."""
        m, L = self.m, self.L
        entry, flip, S, B = c["entry"], c["flip"], c["S"], c["B"]
        x = P + c["x_off"]
        bias = P if c["bias"] else None
        if entry == "linear" or (entry == "obs" and c["k"] == 0):
            geom = m.bt_conv2d_geom(B, c["Ci"], 1, 1, c["Co"], 1, 1, 1, 1, 0, 0, 1, 1, 1)
        elif c["dwin"] is not None:      # the launch's geometry over the virtual operand: B * Do images of Ci * kd channels
            geom = m.bt_conv2d_geom(B * depth_out(c), c["Ci"] * c["dwin"][0], c["H"], c["H"], c["Co"], c["k"], c["k"], c["st"], c["st"], c["pad"], c["pad"], 1, 1, 1)
        else:
            geom = m.bt_conv2d_geom(B, c["Ci"], c["H"], c["H"], c["Co"], c["k"], c["k"], c["st"], c["st"], c["pad"], c["pad"], 1, 1, 1)
        xss = x_elems(c) if c["per_sample_x"] else 0
        if entry == "lowrank":
            inj = P if c["draws"] == "natural" else None
            R = m.bt_rng(1, None, 0, 1, 0, 0)
            rc = L.bt_lowrank_conv2d_fwd(C.byref(geom), S, x, xss, P, 0, P, LOWRANK_R, 0.01, inj, inj, C.byref(R), None, P, None)
        elif entry == "obs":
            inj = c["draws"] == "natural"
            par = m.bt_params(P, P, bias, bias, None, None, None, None, None, None, 0, 0)
            d = m.bt_draws(P if inj else None, bias if inj else None, P if inj else None, P if inj else None, m.bt_rng(1, None, 0, 1, 0, 0))
            tail = (S, x, xss, C.byref(par), C.byref(d), None, None, P, P, P, P, P, None)
            rc = L.bt_q8_flip_observe_linear(B, c["Ci"], c["Co"], *tail) if c["k"] == 0 else L.bt_q8_flip_observe_conv2d(C.byref(geom), *tail)
        else:
            packs = P if c["packs"] else None
            par = m.bt_params(P, P, bias, bias, None, None, None, None, packs, packs, 0, 0)
            if c["draws"] == "chip":
                d = m.bt_draws(None, None, None, None, m.bt_rng(1, None, 0, 1, 0, 0))
            else:
                flags = (m.DRAWS_EPS_PACKED | (m.DRAWS_SIGNS_PACKED if flip else 0)) if c["draws"] == "packed" else 0
                d = m.bt_draws(P, bias, P if flip else None, P if flip else None, m.bt_rng(1, None, 0, 1, 0, flags))
            # the workspace functional.fused_forward hands over: the split-K scratch where a launch may use it, else none
            scratch = 0
            if c["draws"] != "natural" and not flip and c["packs"] and entry in ("conv", "linear"):
                scratch = int(self.scratch(C.byref(geom), S))
            ws, ws_bytes = (P, m.WORKSPACE_BYTES + (scratch + 255) // 256 * 256) if scratch else (None, 0)
            tail = (S, x, xss, C.byref(par), C.byref(d), self.pool_ref if c["pool"] else None, P, None, ws, ws_bytes, None)
            if entry == "linear":
                rc = (L.bt_flipout_linear_fwd if flip else L.bt_reparam_linear_fwd)(B, c["Ci"], c["Co"], *tail)
            elif entry == "updil":
                u = m.bt_updil(*UPDIL)
                rc = (L.bt_flipout_conv2d_updil_fwd if flip else L.bt_reparam_conv2d_updil_fwd)(C.byref(geom), C.byref(u), *tail)
            elif entry == "dwin":
                w = m.bt_dwin(*c["dwin"])
                rc = (L.bt_flipout_conv2d_dwin_fwd if flip else L.bt_reparam_conv2d_dwin_fwd)(C.byref(geom), C.byref(w), *tail)
            else:
                rc = (L.bt_flipout_conv2d_fwd if flip else L.bt_reparam_conv2d_fwd)(C.byref(geom), *tail)
        if rc != 0:
            return None
        return base.lowrank_key(L.bt_last_kernel_name().decode())

    def plan(self, c):
        """A case's plan from a clean state (the replay of the host test)."""
        before = self.knobs(c)
        try:
            return self.call(c)
        finally:
            self.restore(before)


# ---------------------------------------------------------------------------------------------------------------- the grid
CI = (3, 8, 16, 24, 32, 64, 128, 256, 264, 512)
CO = (8, 16, 32, 40, 64, 72, 128, 256)
KS = (1, 2, 3, 4, 5, 6, 7, 12)
HS = (1, 2, 3, 4, 5, 7, 8, 14, 16, 32)
BS = ((1, 1), (2, 1), (3, 2), (4, 1), (8, 2), (16, 1), (16, 2), (32, 2), (64, 1), (64, 2), (128, 1), (128, 2), (256, 2), (8, 64), (32, 16), (64, 16), (128, 16), (256, 16),
      (512, 2), (1024, 2), (256, 64),
      # 65 <= B * Ho * Wo < 256 with S large: the 128 x 128 tiles, which want 256 workgroups of a launch too narrow for the wide tiles
      (5, 256), (8, 256), (12, 128), (17, 256), (32, 256), (100, 256), (128, 128), (200, 64))


def conv_geoms(ks=KS, cis=CI, cos=CO, hs=HS, bs=BS, cap=MAC_CAP):
    for Ci, Co, k, st in itertools.product(cis, cos, ks, (1, 2)):
        for pad in sorted({0, k // 2}):
            for H in hs:
                v = H + 2 * pad - k
                if v < 0:
                    continue
                Ho = v // st + 1
                per = Co * Ho * Ho * Ci * k * k
                for B, S in bs:
                    if per * B * S <= cap:
                        yield dict(Ci=Ci, Co=Co, k=k, st=st, pad=pad, H=H, B=B, S=S)


def conv_ways():
    """The knob settings of the conv2d / linear entry points."""
    for flip in (False, True):
        for mode in (0, 1, 2, 3):
            yield dict(flip=flip, mode=mode)
        yield dict(flip=flip, mode=0, draws="packed")
        yield dict(flip=flip, mode=1, draws="natural")
        yield dict(flip=flip, mode=1, packs=False)
        for mode in (0, 1, 3):
            yield dict(flip=flip, mode=mode, x_off=4)
        yield dict(flip=flip, mode=1, generic=1)
        for mode, bn32 in itertools.product((0, 2, 3), (0, 1)):
            yield dict(flip=flip, mode=mode, bn32=bn32)
        for bn32 in (0, 1):
            yield dict(flip=flip, mode=0, draws="packed", bn32=bn32)


def pool_ways():
    """The stems' pool epilogue: over a shared x (BT_QUAD_SPW=1 keeps a pooled stem on the one-sample kernel) and over a per-sample x."""
    for flip in (False, True):
        for mode, draws in ((0, "chip"), (1, "chip"), (3, "chip"), (0, "packed")):
            yield dict(flip=flip, mode=mode, draws=draws, pool=True, spw="1")
            yield dict(flip=flip, mode=mode, draws=draws, pool=True, per_sample_x=True)


def candidates():
    """(way, [geometry]) of the whole search."""
    geoms = list(conv_geoms())
    for w in conv_ways():
        yield dict(w, entry="conv"), geoms
    stems = list(conv_geoms(cis=(3, 4)))
    for w in pool_ways():
        yield dict(w, entry="conv"), stems
    lin = [dict(Ci=In, Co=Out, k=0, st=1, pad=0, H=1, B=B, S=S) for In, Out, (B, S) in
           itertools.product((8, 16, 24, 64, 128, 130, 256, 512, 1024), (8, 10, 32, 64, 72, 128, 256), BS + ((5, 2), (300, 2), (1024, 16), (4096, 16)))]
    for w in conv_ways():
        yield dict(w, entry="linear"), lin
    small = list(conv_geoms(ks=(1, 2, 3), cis=(3, 8, 16, 24, 64), hs=(1, 2, 3, 4, 8, 16)))
    for flip, mode in itertools.product((False, True), (0, 1, 3)):
        yield dict(entry="updil", flip=flip, mode=mode), [g for g in small if g["pad"] == 0]
        for dw, bn32 in itertools.product(((1, 1, 1, 1, 0), (2, 3, 1, 1, 0), (3, 4, 1, 1, 1), (3, 2, 2, 1, 1)), (-1, 1)):
            yield dict(entry="dwin", flip=flip, mode=mode, dwin=dw, bn32=bn32), [g for g in small if g["Ci"] != 3 or mode == 1]
    lr = list(conv_geoms(ks=(1, 3), cis=(3, 8, 16), cos=(8, 16, 32, 40, 64, 72, 128), hs=(1, 2, 3, 4, 5, 8, 16)))
    for draws in ("chip", "natural"):
        yield dict(entry="lowrank", draws=draws, mode=1), lr
        yield dict(entry="obs", flip=True, draws=draws), lr + [g for g in lin if g["Ci"] <= 130]
        yield dict(entry="obs", flip=True, draws=draws, x_off=4), [g for g in lin if g["Ci"] <= 130]


def tiles_of(name):
    """(channel tile, pixel tile) read off a kernel name: <BN,BM,...>, the direct kernel's <64,8x64 (64-pixel sub-tiles) and the
    split-K kernel's <64,4x32 (32 rows)."""
    m = re.match(r"\w+<(\d+),(?:\d+x)?(\d+)", name)
    return int(m.group(1)), int(m.group(2))


def is_ragged(name, c, strict=True):
    """Co off the channel tile, the launch's pixels off the pixel tile and (``strict``) the launch's input channels off 8."""
    bn, bm = tiles_of(name)
    Ho = out_hw(c)
    return c["Co"] % bn != 0 and (c["B"] * depth_out(c) * Ho * Ho) % bm != 0 and not (strict and (c["Ci"] * (c["dwin"][0] if c["dwin"] else 1)) % 8 == 0)


def better(a, b):
    return b is None or (a["macs"], x_elems(a)) < (b["macs"], x_elems(b))


def search(pl, log=print):
    """name -> the cheapest case found."""
    best, n = {}, 0
    for way, geoms in candidates():
        c0 = make_case(**way, **geoms[0])
        before = pl.knobs(c0)
        try:
            for g in geoms:
                c = dict(c0)
                c.update(g)
                c["macs"] = macs_of(c)
                if c["macs"] > MAC_CAP or c["macs"] == 0 or (c["pool"] and out_hw(c) < 1):
                    continue
                name = pl.call(c)
                n += 1
                if name is not None and better(c, best.get(name)):
                    best[name] = c
        finally:
            pl.restore(before)
    log("%d plans, %d names" % (n, len(best)))
    return best


def ragged_of(pl, name, mn, strict=True):
    """The cheapest ragged case of ``name`` in min's neighbourhood: with a bias and S >= 2 where one plans to it, else as min has them.
    strict=False: the ``edge`` case of a name without one -- the split-precision kernels take whole octets of input channels, so no case
    of theirs has Ci off 8: Co and the pixel count alone are off their tiles."""
    linear = mn["entry"] == "linear" or mn["k"] == 0
    before = pl.knobs(mn)
    try:
        for S, bias in ((max(mn["S"], 2), True), (mn["S"], mn["bias"])):
            if mn["entry"] == "lowrank" and bias:      # (the low-rank forward has no bias stage)
                bias = False
            found = None
            for dco, db, dci, dh in itertools.product(range(-8, 9), range(0, 4), range(-4, 5), (0,) if linear else (0, 1)):
                c = dict(mn, Co=mn["Co"] + dco, B=mn["B"] - db, Ci=mn["Ci"] + dci, H=mn["H"] + dh, S=S, bias=bias)
                if min(c["Co"], c["B"], c["Ci"]) < 1 or out_hw(c) < 1:
                    continue
                c["macs"] = macs_of(c)
                if c["macs"] > MAC_CAP or not is_ragged(name, c, strict) or not better(c, found):
                    continue
                if pl.call(c) == name:
                    found = c
            if found is not None:
                return found
    finally:
        pl.restore(before)
    return None


# The sample walk is planned from the device's CU count (quad_spw: at least one workgroup per CU): no plan without a device. Its rows are
# the stem of tests/test_gpu_stem_walk.py (3 -> Co, 7 x 7, stride 2, padding 3 on 32 x 32, pooled, x shared by the samples): that
# module's "24 channels" row, and its odd batch of 255 with those 24 channels.
WALK_ROWS = dict(min=dict(entry="conv", pool=True, bias=True, Ci=3, Co=24, k=7, st=2, pad=3, H=32, B=256, S=4),
                 ragged=dict(entry="conv", pool=True, bias=True, Ci=3, Co=24, k=7, st=2, pad=3, H=32, B=255, S=3))


def ledger(pl, names, log=print):
    """-> the fixture's dict for the library's ``names``."""
    best = search(pl, log)
    rows = {}
    for name in sorted(names):
        if ",walk" in name:
            rows[name] = dict(needs_device=True, min=make_case(**WALK_ROWS["min"]), ragged=make_case(**WALK_ROWS["ragged"]))
        elif name in best:
            rows[name] = dict(min=best[name], ragged=ragged_of(pl, name, best[name]))
            if rows[name]["ragged"] is None:
                rows[name]["edge"] = ragged_of(pl, name, best[name], strict=False)
    return dict(
        comment="Recorded by tools/find_instantiation_cases.py --write from a gfx950 build of the library, plan-only (no device). One row per name an "
                "instantiation of the six forward-kernel families runs under: 'min' the cheapest case found that plans to it, 'ragged' the cheapest one "
                "near it with Co, B*Ho*Wo and Ci off the tile sizes (null: none in the neighbourhood; 'edge' is then the cheapest one with Co and B*Ho*Wo "
                "off their tiles, or null). A case holds entry point, knobs, geometry and MACs.",
        mac_cap=MAC_CAP, updil=list(UPDIL), lowrank_rank=LOWRANK_R,
        over_budget=sorted(n for n, r in rows.items() if r["min"]["macs"] > MAC_CAP),
        no_ragged=sorted(n for n, r in rows.items() if r["ragged"] is None),
        rows=rows)


def dumps(led):
    """The fixture's text: one case per line."""
    one = lambda v: json.dumps(v, sort_keys=True)
    head = ",\n".join('"%s": %s' % (k, one(led[k])) for k in sorted(led) if k != "rows")
    rows = ",\n".join('%s: {\n%s}' % (one(n), ",\n".join(' "%s": %s' % (k, one(r[k])) for k in sorted(r))) for n, r in sorted(led["rows"].items()))
    return "{%s,\n\"rows\": {\n%s}}\n" % (head, rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", action="store_true", help="re-record tests/golden/instantiation_cases.json")
    args = ap.parse_args()
    from bayesian_torch_amd import _lib
    fam, stubs = base.library_names(_lib.LIB_PATH)
    names = set().union(*fam.values())
    t0 = time.perf_counter()
    led = ledger(Planner(), names)
    print("%.1f s; %d of the library's %d names (%d stubs) have a case" % (time.perf_counter() - t0, len(led["rows"]), len(names), sum(stubs.values())))
    for f in base.FAMILIES:
        print("%-28s %3d stubs %3d names %3d found" % (f, stubs[f], len(fam[f]), len(fam[f] & set(led["rows"]))))
    for n in sorted(names - set(led["rows"])):
        print("no case:", n)
    for n in sorted(set(led["rows"]) - names):
        print("not in the library:", n)
    print("over budget:", led["over_budget"])
    print("no ragged case: %d (%d of them without an edge case)" % (len(led["no_ragged"]), sum(led["rows"][n].get("edge") is None for n in led["no_ragged"])))
    for n in led["no_ragged"]:
        print("  ", n, {k: v for k, v in (led["rows"][n].get("edge") or {}).items() if v != DEFAULTS.get(k, "-")})
    print("largest min: %d MACs" % max(r["min"]["macs"] for r in led["rows"].values()))
    if args.write:
        with open(FIXTURE, "w") as f:
            f.write(dumps(led))


if __name__ == "__main__":
    main()
