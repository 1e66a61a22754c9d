"""The fp32-MFMA host dispatch plans what it planned when the fixtures were recorded (no GPU).

The sibling of ``test_split_plan_parity.py`` for the launches the split-precision chain does not take. With ``bt_debug_plan_only(1)``
``launch_kernel`` records the kernel name and -- ``bt_debug_last_launch_record`` -- grid, block, LDS bytes, LDS limit and a 64-bit
FNV-1a digest of the kernel's argument bytes, and launches nothing: same kernel, same grid / block / LDS, same argument bytes is the
same launch. ``tools/record_fp32_plans.py`` sweeps ~4.6 million such calls under ``bt_set_contraction(1)`` (conv2d over channels,
kernel sizes up to 12x12, stride, dilation, groups, padding, map sizes, batches and sample counts, each with on-chip draws, with
natural-layout injected draws, without packs and with a misaligned x; the stems' pool epilogue; the input-dilated entry points;
Linear; ``BT_FORCE_GENERIC``), for Reparameterization and Flipout. This module replays the sweep against

- ``tests/golden/fp32_plans.txt``: full records of the first and the last case of every kernel name per variant, and every refusal
  text once;
- ``tests/golden/fp32_plans_sha256.json``: one SHA-256 per variant over the whole sweep's text.

Both were recorded from the commit before the planner became a function (``fp32_plan``) and the launches one table
(``launch_fp32``), built with the plan-only seam as its only change. A digest that differs is diffed with
``python tools/record_fp32_plans.py --dump FILE`` on the two trees.
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_fp32_plans", os.path.join(ROOT, "tools", "record_fp32_plans.py"))
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
    """The sweep is not kept line by line (millions): its Sink keeps the rows the table is made of, chosen as when it was recorded."""
    rec, sinks = sweep
    assert len(golden_rows) >= 348      # two per instantiation, and the refusal texts
    got = rec.table(sinks)
    assert len(got) == len(golden_rows)
    for g, row in zip(got, golden_rows):
        assert g == row


def test_whole_sweep_digests(sweep):
    rec, sinks = sweep
    with open(rec.GOLDEN_SHA) as f:
        want = json.load(f)
    assert set(want) == {v[0] for v in rec.VARIANTS}
    assert rec.digests(sinks) == want


def test_every_fp32_instantiation_is_swept_twice(sweep, golden_rows):
    """Every fused_fwd_kernel / fused_fast_kernel instantiation in the built library (its symbol table, not a typed count) is named
    by at least two swept cases, and the table holds two records of it; the sweep names no kernel the library does not hold."""
    rec, sinks = sweep
    from bayesian_torch_amd import _lib
    have = rec.instantiated_names(_lib.LIB_PATH)
    assert len(have) > 100 and all(n.startswith(("fused_fwd_kernel<", "fused_fast_kernel<")) for n in have)
    count = {}
    for s in sinks.values():
        for n, c in s.count.items():
            count[n] = count.get(n, 0) + c
    assert set(count) == have
    assert all(count[n] >= 2 for n in have), sorted(n for n in have if count.get(n, 0) < 2)
    per_name = {}
    for row in golden_rows:
        per_name[rec.base.name_of(row)] = per_name.get(rec.base.name_of(row), 0) + 1
    assert all(per_name.get(n, 0) >= 2 for n in have)
