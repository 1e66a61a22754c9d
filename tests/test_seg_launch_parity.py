"""The segmented launches plan what they planned when the fixtures were recorded (no GPU).

``bt_kl_normal``, ``bt_kl_hier``, ``bt_kl_hier_bwd``, ``bt_kl_normal_bwd_segs`` and ``bt_pack_sync`` / ``bt_pack_sync_kl`` hand a list
of tensors to one grid through a per-segment table. With ``bt_debug_plan_only(1)`` each of their launches leaves grid, block, LDS and
a digest of what its argument block means (per segment: pointers, ``n``, first block; then the table's tail and the block's scalars),
and ``bt_debug_last_launch_record`` counts and chains the launches of a call. ``tools/record_seg_launches.py`` sweeps the segment
counts 1, 2, 3, 63, 64, 0, 65, the lengths around the float4, block and stride boundaries, every cap and one past it, the workspace's
slot limit with and without a KL, ``layer_of_segment`` as null, constant, in pairs and decreasing, the flag bits, the pack geometry
(``Ci`` off a multiple of 4, taps 1, 9, 128, 129, bias, ``force``) and a null pointer in every position. This module replays it against

- ``tests/golden/seg_launches.txt``: every call's entry point, case, return code, error text, launch count and chain digest;
- ``tests/golden/seg_launches_sha256.json``: one SHA-256 per entry point over its lines.

Both were recorded from the commit before the table became one struct (``SegTable``) with one host builder, built with the plan-only
seam -- these launches through ``launch_kernel``, the digests written for the argument blocks of that commit -- as its only change.
A line that differs is found with ``python tools/record_seg_launches.py --dump FILE``.
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sweep():
    spec = importlib.util.spec_from_file_location("record_seg_launches", os.path.join(ROOT, "tools", "record_seg_launches.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec, rec.record()


def test_every_call_replays(sweep):
    rec, lines = sweep
    with open(rec.GOLDEN_TABLE) as f:
        want = [ln for ln in f.read().splitlines() if ln]
    got = rec.table(lines)
    assert len(want) >= 500 and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_entry_point_digests(sweep):
    rec, lines = sweep
    with open(rec.GOLDEN_SHA) as f:
        want = json.load(f)
    assert set(want) == set(rec.ENTRIES)
    assert rec.digests(lines) == want


def test_the_sweep_reaches_what_it_claims(sweep):
    """Launch counts and refusals the sweep is there for: two launches per pack call, one per KL call, none for a refusal; every
    refusal text of the host builders at least once."""
    rec, lines = sweep
    for entry, ls in lines.items():
        for ln in ls:
            f = ln.split("|")
            assert f[4] == ("0" if f[2] != "0" else "2" if entry.startswith("bt_pack") else "1"), ln
    text = "\n".join(rec.table(lines))
    for msg in ("bt_kl_normal: too many blocks for the workspace; split the call", "bt_kl_hier: too many blocks for the workspace; split the call",
                "bt_kl_hier_bwd: too many elements for one launch", "bt_kl_normal_bwd_segs: too many elements for one launch",
                "bt_kl_normal: layer_of_segment must be non-decreasing", "bt_kl_hier: layer_of_segment must be non-decreasing",
                "bt_pack_sync: kernels larger than 128 taps are not supported"):
        assert msg in text, msg
