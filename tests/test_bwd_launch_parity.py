"""The training backward plans what it planned when the fixtures were recorded (no GPU).

``bt_conv2d_bwd`` / ``bt_conv2d_bwd_kl`` take everything they launch with from one host plan (``csrc/bt_bwd_plan.h``) and launch
through ``launch_kernel``. With ``bt_debug_plan_only(1)`` each launch leaves grid, block, LDS and a digest of what its argument block
means (the pointers, then every scalar, in a fixed order), and ``bt_debug_last_launch_record`` counts and chains the launches of a
call. ``tools/record_bwd_launches.py`` sweeps the seven ``DRAW_ROWS`` of ``_grad_cases.py``, the 21 ResNet-18 / CIFAR layers at
B 128 / S 1 and B 8 / S 4, Linear 4096 -> 130, groups, stride, dilation, rectangular kernels, ``Cig`` 1 ... 130, ``Cog`` 16 ... 136
(dgrad's piece cap), ``M`` 15 ... 245 (wgrad's chunk rounding) -- each for {dx, weights, both} x {Reparameterization, Flipout} x
{paired, unpaired} with and without ``grad_kl`` --, the workgroup targets (128, 256) ... (1, 1), the workspace null and one byte
short wherever it is checked, and every refusal. This module replays it against

- ``tests/golden/bwd_launches.txt``: every call's entry point, case, return code, error text, launch count, chain digest and the
  value of ``bt_conv2d_bwd_workspace``;
- ``tests/golden/bwd_launches_sha256.json``: one SHA-256 per entry point over its lines.

Both were recorded from the commit before the plan existed, built with the plan-only seam as its only change: the nine launches
through ``launch_kernel``, the digest written for that commit's ``BwdArgs``, and ``BT_WGRAD_WGS`` / ``BT_DGRAD_WGS`` /
``BT_NO_BWD_PAIR`` readable through ``bt_debug_bwd_targets`` / ``bt_debug_bwd_pair``. Only calls that commit survives are in the
sweep (it died of a division by zero on a zero stride, kernel size or channel count: ``test_bwd_host.py`` holds those).
A line that differs is found with ``python tools/record_bwd_launches.py --dump FILE``.
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sweep():
    spec = importlib.util.spec_from_file_location("record_bwd_launches", os.path.join(ROOT, "tools", "record_bwd_launches.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec, rec.record()


def test_every_call_replays(sweep):
    rec, lines = sweep
    with open(rec.GOLDEN_TABLE) as f:
        want = [ln for ln in f.read().splitlines() if ln]
    got = rec.table(lines)
    assert len(want) >= 2000 and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_entry_point_digests(sweep):
    rec, lines = sweep
    with open(rec.GOLDEN_SHA) as f:
        want = json.load(f)
    assert set(want) == set(rec.ENTRIES)
    assert rec.digests(lines) == want


def test_the_sweep_reaches_what_it_claims(sweep):
    """Launch counts: none for a refusal; paired 2; unpaired dgrad 1 or 2 (with a finishing pass), wgrad 2, both 3 or 4. Every
    refusal text of the backward at least once, and both workspace checks (dgrad's own only where it has pieces)."""
    rec, lines = sweep
    seen = set()
    for ls in lines.values():
        for ln in ls:
            f = ln.split("|")
            case, rc, n = f[1], int(f[2]), int(f[4])
            if rc:
                assert n == 0, ln
            elif case.endswith(" both paired"):
                assert n == 2, ln
            elif case.endswith(" both unpaired"):
                assert n in (3, 4), ln
            elif case.endswith((" w paired", " w unpaired")):
                assert n == 2, ln
            elif case.endswith((" dx paired", " dx unpaired")):
                assert n in (1, 2), ln
            seen.add(n)
    assert seen == {0, 1, 2, 3, 4}
    text = "\n".join(rec.table(lines))
    for msg in ("bt_conv2d_bwd: null argument", "bt_conv2d_bwd_kl: grad_kl needs dmu_w / drho_w", "bt_conv2d_bwd_kl: needs mu_w and the weight priors",
                "bt_conv2d_bwd: needs rho_w and the packed parameters (bt_pack_params)", "bt_conv2d_bwd: mu_packed / sigma_packed must be 16-byte aligned",
                "bt_conv2d_bwd: bad geometry", "bt_conv2d_bwd: dmu_w and drho_w go together", "bt_conv2d_bwd: inject all draws or none",
                "bt_conv2d_bwd: empty output", "bt_conv2d_bwd: tensor too large for the 32-bit sign / draw indices",
                "bt_conv2d_bwd: workspace smaller than bt_conv2d_bwd_workspace()"):
        assert msg in text, msg
    short = [ln for ln in lines["bt_conv2d_bwd"] if "workspace one byte short" in ln]
    assert {ln.split("|")[1].split(" workspace")[0]: int(ln.split("|")[2]) for ln in short} == {
        "rowA dx": -3, "rowA w": -3, "rowA both": -3, "rowC dx": 0, "rowC w": -3, "rowC both": -3}
