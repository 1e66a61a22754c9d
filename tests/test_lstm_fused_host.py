"""CPU: the LSTM cell entry points (bt_lstm_cell_fwd / bt_lstm_cell_bwd) and the host side of ``set_lstm_path("fused")``.

``bt_debug_plan_only(1)`` makes ``launch_kernel`` record the kernel name and return before it touches the runtime, so the argument checks
and the choice between the vector and the element-wise form run on any machine. The C-call sequence of the layers runs on the stand-in
library of tools/record_abi_calls.py with a case of this file's own (the recorder's table is pinned and gets none). The GPU side is
tests/test_gpu_lstm_fused.py; both files share tests/_lstm_cases.py."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import sys

import pytest
import torch

import _lstm_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 0x10000000          # any non-null, 16-byte aligned address


@pytest.fixture()
def plan_only():
    from bayesian_torch_amd import _lib
    L, h = _lib.lib(), C.CDLL(_lib.LIB_PATH)      # the bt_debug_* hooks are outside include/bt_hip.h
    h.bt_debug_plan_only(1)
    try:
        yield _lib, L
    finally:
        h.bt_debug_plan_only(0)


def _fwd(L, rows=8, H=64, a=P, b=P, c_prev=P, c_rows=None, ld_c=None, h_out=P, c_out=P, ld_out=None, act=None):
    rc = L.bt_lstm_cell_fwd(rows, H, a, b, c_prev, rows if c_rows is None else c_rows, H if ld_c is None else ld_c, h_out, c_out,
                            H if ld_out is None else ld_out, act, None)
    return rc, L.bt_last_kernel_name().decode()


def _bwd(L, rows=8, H=64, act=P, c_prev=P, c_rows=None, ld_c=None, c_new=P, ld_cn=None, grad_h=P, ld_gh=None, grad_c=P, ld_gc=None, dz=P, dc_prev=P):
    d = lambda v: H if v is None else v
    rc = L.bt_lstm_cell_bwd(rows, H, act, c_prev, rows if c_rows is None else c_rows, d(ld_c), c_new, d(ld_cn), grad_h, d(ld_gh), grad_c, d(ld_gc),
                            dz, dc_prev, None)
    return rc, L.bt_last_kernel_name().decode()


def test_entry_points_exist_and_agree_with_the_header():
    from bayesian_torch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bt_hip.h")).read()
    handle = C.CDLL(_lib.LIB_PATH)
    for name, n_args in (("bt_lstm_cell_fwd", 12), ("bt_lstm_cell_bwd", 15)):
        assert name in _lib.EXPORTS and hasattr(handle, name)
        decl = re.search(r"^int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
        assert decl.count(",") + 1 == len(_lib._PROTOS[name][1]) == n_args
    assert _lib.lib().bt_version() == 302


def test_bad_arguments_are_refused_before_any_launch(plan_only):
    _, L = plan_only
    assert _fwd(L)[0] == 0 and _bwd(L)[0] == 0
    bad_fwd = [dict(rows=0), dict(H=0), dict(rows=-3), dict(a=None), dict(c_prev=None), dict(h_out=None), dict(c_out=None), dict(c_rows=3), dict(c_rows=0),
               dict(c_rows=16), dict(ld_c=63), dict(ld_out=63)]
    for kw in bad_fwd:
        assert _fwd(L, **kw)[0] == -1, kw
        assert b"bt_lstm_cell_fwd" in L.bt_last_error_string()
    bad_bwd = [dict(rows=0), dict(H=0), dict(act=None), dict(c_prev=None), dict(c_new=None), dict(dz=None), dict(dc_prev=None), dict(c_rows=3), dict(c_rows=0),
               dict(ld_c=63), dict(ld_cn=63), dict(ld_gh=63), dict(ld_gc=63)]
    for kw in bad_bwd:
        assert _bwd(L, **kw)[0] == -1, kw
        assert b"bt_lstm_cell_bwd" in L.bt_last_error_string()
    # what is optional is accepted: no b, no act; either gradient missing (its stride is then not looked at); a shared c_prev
    assert _fwd(L, b=None)[0] == 0 and _fwd(L, c_rows=2)[0] == 0 and _fwd(L, c_rows=1)[0] == 0
    assert _bwd(L, grad_h=None, ld_gh=0)[0] == 0 and _bwd(L, grad_c=None, ld_gc=0)[0] == 0 and _bwd(L, grad_h=None, grad_c=None)[0] == 0


def test_the_planned_form_follows_the_vector_guard(plan_only):
    _, L = plan_only
    assert _fwd(L) == (0, "lstm_cell_fwd_kernel<vec4,act=0>")
    assert _fwd(L, act=P) == (0, "lstm_cell_fwd_kernel<vec4,act=1>")
    assert _fwd(L, ld_out=192, ld_c=68) == (0, "lstm_cell_fwd_kernel<vec4,act=0>")
    assert _bwd(L) == (0, "lstm_cell_bwd_kernel<vec4>")
    assert _bwd(L, grad_h=None, ld_gh=1, grad_c=None, ld_gc=3) == (0, "lstm_cell_bwd_kernel<vec4>")
    for H in (5, 130):
        assert _fwd(L, H=H) == (0, "lstm_cell_fwd_kernel<elem,act=0>")
        assert _fwd(L, H=H, act=P) == (0, "lstm_cell_fwd_kernel<elem,act=1>")
        assert _bwd(L, H=H) == (0, "lstm_cell_bwd_kernel<elem>")
    for op in ("a", "b", "c_prev", "h_out", "c_out", "act"):       # any one operand 4 bytes off
        assert _fwd(L, **{op: P + 4}) == (0, "lstm_cell_fwd_kernel<elem,act=%d>" % (op == "act")), op
    for op in ("act", "c_prev", "c_new", "grad_h", "grad_c", "dz", "dc_prev"):
        assert _bwd(L, **{op: P + 4}) == (0, "lstm_cell_bwd_kernel<elem>"), op
    for ld in (65, 66, 67, 193):
        assert _fwd(L, ld_out=ld) == (0, "lstm_cell_fwd_kernel<elem,act=0>")
        assert _fwd(L, ld_c=ld) == (0, "lstm_cell_fwd_kernel<elem,act=0>")
    for name in ("ld_c", "ld_cn", "ld_gh", "ld_gc"):
        assert _bwd(L, **{name: 65}) == (0, "lstm_cell_bwd_kernel<elem>"), name


def test_the_planned_grid_covers_rows_times_quads(plan_only):
    m, L = plan_only
    h = C.CDLL(m.LIB_PATH)
    rec = (C.c_int64 * 9)()
    for rows, H, blocks in ((257, 64, 17), (33, 130, 5), (3, 5, 1), (1, 1, 1), (256, 4, 1), (257, 4, 2)):      # ceil(rows * ceil(H / 4) / 256)
        assert _fwd(L, rows=rows, H=H)[0] == 0
        assert h.bt_debug_last_launch_record(rec, 9) == 0
        assert tuple(rec)[:8] == (blocks, 1, 1, 256, 1, 1, 0, 0), (rows, H, tuple(rec))
        assert _bwd(L, rows=rows, H=H)[0] == 0
        assert h.bt_debug_last_launch_record(rec, 9) == 0
        assert tuple(rec)[:8] == (blocks, 1, 1, 256, 1, 1, 0, 0), (rows, H, tuple(rec))


def test_switch_default_env_and_unknown_name():
    import bayesian_torch_amd.layers as BL
    assert BL.get_lstm_path() == os.environ.get("BT_LSTM_PATH", "torch")
    prev = BL.set_lstm_path("fused")
    try:
        assert BL.get_lstm_path() == "fused" and BL.set_lstm_path("torch") == "fused" and BL.get_lstm_path() == "torch"
        with pytest.raises(ValueError, match=r"set_lstm_path: expected one of \('torch', 'fused'\), got 'native'"):
            BL.set_lstm_path("native")
        assert BL.get_lstm_path() == "torch"
    finally:
        BL.set_lstm_path(prev)
    code = "import bayesian_torch_amd.layers as L; print(L.get_lstm_path())"
    env = {k: v for k, v in os.environ.items() if k != "BT_LSTM_PATH"}
    run = lambda e: subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True)
    assert run(env).stdout.strip() == "torch"
    assert run(dict(env, BT_LSTM_PATH="fused")).stdout.strip() == "fused"
    r = run(dict(env, BT_LSTM_PATH="cudnn"))
    assert r.returncode != 0 and "BT_LSTM_PATH: expected one of ('torch', 'fused'), got 'cudnn'" in r.stderr


# ------------------------------------------------------------------------------------------------ C calls on the recorder's stand-in
def _recorder():
    spec = importlib.util.spec_from_file_location("record_abi_calls", os.path.join(ROOT, "tools", "record_abi_calls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _record(R, path, fn, cuda_tensors=False):
    import bayesian_torch_amd.layers as BL
    prev = BL.set_lstm_path(path)
    try:
        return R.run_case("local", fn, cuda_tensors)
    finally:
        BL.set_lstm_path(prev)


def _want_kl(line):
    """A recorded bt_*_linear_fwd call asked for its KL term iff its kl_out pointer (argument 11 of 14) is not null."""
    args = re.match(r"\s*bt_\w+_linear_fwd\((.*)\) -> 0$", line).group(1)
    depth, parts, cur = 0, [], ""
    for ch in args:
        depth += ch in "{[" and 1 or (ch in "}]" and -1 or 0)
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    parts.append(cur.strip())
    assert len(parts) == 14, parts
    return parts[10] != "null"


@pytest.mark.parametrize("cls", ["LSTMReparameterization", "LSTMFlipout"])
def test_fused_no_grad_call_sequence_two_linears_and_one_cell_per_step(cls):
    R = _recorder()
    lin = "bt_flipout_linear_fwd" if "Flipout" in cls else "bt_reparam_linear_fwd"

    def case(env):
        m = env.layer(cls, lid=3, in_features=4, out_features=3)
        with torch.no_grad():
            env.note("out", m(env.tensor("x", 2, 3, 4)))

    text, calls = _record(R, "fused", case)
    assert "raises" not in text
    fwd = [c for c in calls if c in (lin, "bt_lstm_cell_fwd")]
    assert fwd == [lin, lin, "bt_lstm_cell_fwd"] * 3, calls
    assert set(calls) <= {lin, "bt_lstm_cell_fwd", "bt_pack_sync", "bt_pack_sync_kl", "bt_last_kernel_name", "bt_last_launch_info", "bt_fused_scratch_bytes"}, calls
    kl = [_want_kl(ln) for ln in text.splitlines() if "_linear_fwd(" in ln]
    syncs = [c for c in calls if c.startswith("bt_pack_sync")]
    # each map's KL once per forward: step 0's two calls take it (from their own pack check's sweep, or from the forward's), no later call does
    assert len(kl) == 6 and kl[2:] == [False] * 4
    assert syncs[:2] == ["bt_pack_sync_kl"] * 2 and syncs[2:] == ["bt_pack_sync"] * 4 and kl[:2] == [False, False]
    assert "out: (T(2, 3, 3), (T(2, 3, 3), T(2, 3, 3)), T())" in text
    cells = [ln for ln in text.splitlines() if "bt_lstm_cell_fwd(" in ln]
    # step t writes slab t of the time-major storage and reads slab t - 1 as c_prev; the next hh launch reads h from the same storage
    outs = [re.match(r"\s*bt_lstm_cell_fwd\(2, 3, (\S+), (\S+), (\S+), 2, 3, (\S+), (\S+), 3, null, null\)", ln).groups() for ln in cells]
    hbuf, cbuf = outs[0][3].split("+")[0], outs[0][4].split("+")[0]
    assert [o[3] for o in outs] == ["%s+%d" % (hbuf, 24 * t) for t in range(3)] and [o[4] for o in outs] == ["%s+%d" % (cbuf, 24 * t) for t in range(3)]
    assert [o[2] for o in outs[1:]] == [o[4] for o in outs[:2]]
    hh_x = [ln.split("(")[1].split(", ")[4] for ln in text.splitlines() if "_linear_fwd(" in ln][1::2]
    assert hh_x[1:] == [o[3] for o in outs[:2]], (hh_x, outs)


def test_torch_path_yields_todays_calls_and_fused_under_grad_adds_the_cell_pair():
    R = _recorder()

    def case(env):
        m = env.layer("LSTMReparameterization", lid=3, in_features=4, out_features=3)
        hs, _, kl = m(env.tensor("x", 2, 3, 4))
        (hs.sum() + kl).backward()
        env.grads(m)

    t_text, t_calls = _record(R, "torch", case)
    f_text, f_calls = _record(R, "fused", case)
    assert "raises" not in t_text + f_text
    lin = "bt_reparam_linear_fwd"
    assert "bt_lstm_cell_fwd" not in t_calls and "bt_lstm_cell_bwd" not in t_calls
    assert t_calls.count(lin) == f_calls.count(lin) == 6 and t_calls.count("bt_conv2d_bwd_kl") == f_calls.count("bt_conv2d_bwd_kl") == 6
    assert f_calls.count("bt_lstm_cell_fwd") == 3 and f_calls.count("bt_lstm_cell_bwd") == 3
    assert t_calls.count("bt_kl_normal") == 6 and f_calls.count("bt_kl_normal") == 2       # every step's two calls / step 0's two calls
    acts = [ln for ln in f_text.splitlines() if "bt_lstm_cell_fwd(" in ln]
    assert all(not ln.split(", ")[-2].startswith("null") for ln in acts)       # under grad the forward saves the activated gates
    # the pinned record of the default path is the recorder's own (tests/test_abi_call_parity.py): here only that this file's stand-in
    # run of it reproduces the recorder's digest for its LSTM case
    import json
    sha = json.load(open(R.GOLDEN_SHA))
    rec = R.run_case("lstm/two-steps", dict((n, f) for n, f, _ in R.CASES)["lstm/two-steps"])
    import hashlib
    assert hashlib.sha256(rec[0].encode()).hexdigest() == sha["lstm/two-steps"]


# ------------------------------------------------------------------------------------------------ the references themselves
@pytest.mark.parametrize("row", range(len(LC.CELL_ROWS)), ids=LC.CELL_IDS)
def test_float32_reference_is_finite_and_inside_its_bound(row):
    """The limit the GPU test applies is FACTOR x the float32 reference's own error: that error must be the 1e-7-size rounding noise the
    issue measured (0.3e-7 .. 8e-7 -- a reference that were off by more would hand the kernels a limit that checks nothing), and every
    output of both references finite, the +-90 rows included."""
    r = LC.cell_row(row)
    for k in LC.OUTPUTS + ("act",):
        assert torch.isfinite(r["ref64"][k]).all() and torch.isfinite(r["ref32"][k]).all(), k
    print(LC.CELL_IDS[row], {k: "%.2e" % v for k, v in r["ref32_err"].items()})
    for k, v in r["ref32_err"].items():
        assert 0 <= v <= 8e-7, (k, v)
    t = r["inputs"]
    if t["special"] == "pm90":
        H, act = t["H"], r["ref32"]["act"]
        assert torch.equal(act[0], torch.ones(4 * H)) and torch.equal(act[1, 2 * H:3 * H], -torch.ones(H))
        assert float(act[1, :2 * H].abs().max()) < 1e-38 and float(act[1, 3 * H:].abs().max()) < 1e-38


@pytest.mark.parametrize("row", range(len(LC.CELL_ROWS)), ids=LC.CELL_IDS)
def test_closed_form_backward_matches_fp64_autograd(row):
    """What bt_lstm_cell_bwd computes -- the closed form on the saved activations -- against float64 autograd of the gate arithmetic."""
    r = LC.cell_row(row)
    dz, dcp = LC.closed_form(r["inputs"], torch.float64)
    assert LC.metric(dz, r["ref64"]["dz"]) <= 1e-14 and LC.metric(dcp, r["ref64"]["dc_prev"]) <= 1e-14
    dz32, dcp32 = LC.closed_form(r["inputs"], torch.float32)
    assert LC.metric(dz32, r["ref64"]["dz"]) <= LC.FACTOR * max(r["ref32_err"]["dz"], 1e-7)
    assert LC.metric(dcp32, r["ref64"]["dc_prev"]) <= LC.FACTOR * max(r["ref32_err"]["dc_prev"], 1e-7)
