"""The split-precision host dispatch plans what it planned when the fixtures were recorded (no GPU).

``bt_debug_plan_only(1)`` makes ``launch_kernel`` record the kernel name and return before it touches the runtime, so a forward call
with made-up aligned addresses runs the whole chain -- eligibility, tile planner, instantiation table, name builder -- on any machine.
``tools/record_split_plans.py`` sweeps ~150,000 such calls (Reparameterization in contraction modes 0 / 2 / 3 and with packed draws,
Flipout on chip and with packed draws and signs; conv2d and linear entry points; the stems' pool epilogue; 32-channel tiles forced
off / on; the row tile). This module replays the sweep against

- ``tests/golden/split_plans.txt``: full records (return code, kernel name, the 16 launch-info integers) of the first and the last
  case of every kernel name a variant reaches, and of the boundary cases;
- ``tests/golden/split_plans_sha256.json``: one SHA-256 per variant over the whole sweep's text.

Both were recorded from the commit before the launch templates and the planner were unified, built with the plan-only seam as its
only change. A digest that differs is diffed with ``python tools/record_split_plans.py --dump FILE`` on the two trees. The one
instantiation the sweep leaves out is the stems' sample walk (its plan reads the device's CU count; the recorder keeps the stems on
the one-sample path so that the records are the same with and without a device: tests/test_gpu_stem_walk.py pins the walk).
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_split_plans", os.path.join(ROOT, "tools", "record_split_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def sweep():
    rec = _recorder()
    return rec, rec.record()


@pytest.fixture(scope="module")
def golden_rows():
    rec = _recorder()
    with open(rec.GOLDEN_TABLE) as f:
        return [ln for ln in f.read().splitlines() if ln]


def test_table_records_replay(sweep, golden_rows):
    _, lines = sweep
    got = {tuple(ln.split("|")[:2]): ln for ls in lines.values() for ln in ls}
    assert len(golden_rows) >= 200
    for row in golden_rows:
        assert got.get(tuple(row.split("|")[:2])) == row


def test_whole_sweep_digests(sweep):
    rec, lines = sweep
    with open(rec.GOLDEN_SHA) as f:
        want = json.load(f)
    assert set(want) == {v[0] for v in rec.VARIANTS}
    assert rec.digests(lines) == want


def test_table_covers_every_kernel_name_the_sweep_reaches(sweep, golden_rows):
    rec, lines = sweep
    reached = {rec.name_of(ln) for ls in lines.values() for ln in ls} - {"-"}
    split = {n for n in reached if n.startswith("fused_split_")}
    # every name of the split-precision library but the stems' sample walk (needs a device): 68 kernels, the two skinny ones under two names each
    assert len(split) == 70
    assert not any("walk" in n for n in split)
    # the same statement from the library's own symbol table: the swept split names are the names its four split families' stubs run
    # under, minus exactly the input-dilated (xm=5), depth-window (xm=6) and sample-walk instantiations (other entry points / a device)
    from bayesian_torch_amd import _lib
    fam, _ = rec.library_names(_lib.LIB_PATH)
    have = set().union(*(names for f, names in fam.items() if f.startswith("fused_split_")))
    assert split == {n for n in have if "xm=5" not in n and "xm=6" not in n and "walk" not in n}
    assert not any(",flip," in n and "xm=2" in n for n in split)      # Flipout's 128-wide whole-plane fetch is not instantiated
    per_name = {}
    for row in golden_rows:
        per_name[rec.name_of(row)] = per_name.get(rec.name_of(row), 0) + 1
    assert reached <= set(per_name)
    assert all(per_name[n] >= 2 for n in split)
