"""The Python forward path hands the C ABI what it handed it when the fixtures were recorded (no GPU, no library).

``tools/record_abi_calls.py`` replaces, inside the process only, ``_lib.lib()`` by a stand-in that records every C call and answers a
scripted status, and lets the layers, the autograd bridge, ``functional`` and ``mc`` run on CPU tensors over a table of tiny cases:
every layer class with and without bias, bare / ``mc_samples`` shared / stacked, on-chip / ``"torch"`` / ``inject_draw`` draws, the
``"split"`` inject path with its natural-layout retry and ``declined`` memo, the folded output stage (pool accepted and declined),
Laplace priors, the scratch answer, training (plain, ``train_fused`` with ``kl_stub`` both ways, the ATen checker), a model with
``mc.sync_model_packs``, ``materialize_last_draw`` and the refusals; and the INT8 side: the calibrating forwards of the four prepared
classes (on-chip / ``"torch"`` / ``inject_draw`` draws, ``mc_samples`` shared and stacked, a BatchNorm to fold), ``convert()`` of planted
statistics with its refusals, and the four quantised classes after ``bnn_to_qbnn``. A record holds the function name, every scalar, every field of
every struct and struct array, pointers by identity (tensor name + offset, or first-appearance index), and per case the output shapes,
``_last``, the call counter before and after, gradient shapes or the exception. This module replays the table against

- ``tests/golden/abi_calls.txt``: the full text of the first and the last case that reaches each C function;
- ``tests/golden/abi_calls_sha256.json``: one SHA-256 per case.

Both were recorded from the commit before the forward path was split into named helpers, with the recorder as its only addition; the
``q8`` cases likewise from the commit before calibration moved into ``layers/_calibration.py``. A
digest that differs is diffed with ``python tools/record_abi_calls.py --dump FILE`` on the two trees.
"""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorded():
    spec = importlib.util.spec_from_file_location("record_abi_calls", os.path.join(ROOT, "tools", "record_abi_calls.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec, rec.record()


@pytest.fixture(scope="module")
def golden_cases(recorded):
    with open(recorded[0].GOLDEN_TABLE) as f:
        chunks = f.read().split("== ")[1:]
    return {c.split("\n", 1)[0]: "== " + c for c in chunks}


def test_table_records_replay(recorded, golden_cases):
    _, rec = recorded
    assert len(golden_cases) >= 20
    for name, text in golden_cases.items():
        assert rec[name][0] == text, name


def test_every_case_digest(recorded):
    mod, rec = recorded
    with open(mod.GOLDEN_SHA) as f:
        want = json.load(f)
    assert len(want) >= 190 and set(want) == set(rec)
    got = mod.digests(rec)
    assert [n for n in want if got[n] != want[n]] == []


def test_table_covers_every_c_function_the_cases_reach(recorded, golden_cases):
    _, rec = recorded
    reached = {c for _, calls in rec.values() for c in calls}
    assert {"bt_pack_sync", "bt_pack_sync_kl", "bt_fused_scratch_bytes", "bt_reparam_linear_fwd", "bt_flipout_linear_fwd", "bt_reparam_conv2d_fwd",
            "bt_flipout_conv2d_fwd", "bt_last_kernel_name", "bt_last_launch_info", "bt_pack_eps", "bt_pack_signs", "bt_maxpool_3x3s2", "bt_kl_normal",
            "bt_kl_normal_bwd", "bt_kl_normal_bwd_segs", "bt_conv2d_bwd_workspace", "bt_conv2d_bwd_kl", "bt_rng_normal_fill", "bt_rng_sign_fill", "bt_q8_pack", "bt_q8_linear_fwd", "bt_q8_conv2d_fwd",
            "bt_q8_flip_linear_fwd", "bt_q8_flip_conv2d_fwd", "bt_q8_observe_w", "bt_minmax_update", "bt_q8_flip_observe_x", "bt_q8_flip_observe_linear",
            "bt_q8_flip_observe_conv2d"} <= reached
    in_table = {c for name in golden_cases for c in rec[name][1]}
    assert reached == in_table


def test_the_stand_in_is_gone_afterwards(recorded):
    import torch
    from bayesian_torch_amd import _lib
    assert _lib.lib.__module__ == _lib.__name__ and _lib.dev_f32.__module__ == _lib.__name__
    assert torch.empty.__module__ != recorded[0].__name__ and "is_cuda" not in vars(torch.Tensor)
