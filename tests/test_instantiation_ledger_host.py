"""Every forward-kernel instantiation the library holds has a row in the instantiation ledger, and every row still plans to its own
name (no GPU).

The library's side is ``record_split_plans.library_names``: the ``__device_stub__`` symbols of the six forward-kernel families
(fused_fwd / fused_fast / fused_split / fused_split_quad / fused_split_direct / fused_split_skinny) under the names their launchers
give them. The ledger's side is tests/golden/instantiation_cases.json (tools/find_instantiation_cases.py): per name a ``min`` case and,
where the neighbourhood holds one, a ``ragged`` case (else, where it holds one, an ``edge`` case: Co and the pixel count off their
tiles, Ci a whole number of octets). There is no exemption list: an instantiation without a row, or a row without an instantiation,
fails here, and so does a row whose geometry has drifted to another kernel. tests/test_gpu_every_instantiation.py runs the rows."""
import pytest

import _inst_cases as IC


@pytest.fixture(scope="module")
def library():
    from bayesian_torch_amd import _lib
    return IC.finder().base.library_names(_lib.LIB_PATH)


@pytest.fixture(scope="module")
def planner():
    return IC.finder().Planner()


def test_library_listing_counts_every_stub(library):
    names, stubs = library
    fd = IC.finder()
    assert set(names) == set(stubs) == set(fd.base.FAMILIES)
    assert all(stubs[f] > 0 for f in fd.base.FAMILIES)
    for f in fd.base.FAMILIES:      # one name per stub; the split-K kernel's two stubs run under two names each
        assert len(names[f]) == stubs[f] * (2 if f == "fused_split_skinny_kernel" else 1), (f, len(names[f]), stubs[f])
        assert all(n.startswith(f + "<") and n.endswith(">") for n in names[f])
    assert not any(",R=" in n for n in names["fused_fwd_kernel"]) and any(",lowrank," in n for n in names["fused_fwd_kernel"])
    # the fp32 recorder's listing is the same names without the depth-window, low-rank and observer forms
    from bayesian_torch_amd import _lib
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("record_fp32_plans", os.path.join(IC.ROOT, "tools", "record_fp32_plans.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    fp32 = names["fused_fwd_kernel"] | names["fused_fast_kernel"]
    assert rec.instantiated_names(_lib.LIB_PATH) == {n for n in fp32 if not n.endswith((",dwin>", ",obs>")) and ",lowrank," not in n}


def test_ledger_names_are_the_librarys(library):
    names, _ = library
    have = set().union(*names.values())
    rows = set(IC.ledger()["rows"])
    assert sorted(have - rows) == [], "instantiations without a ledger row (tools/find_instantiation_cases.py --write)"
    assert sorted(rows - have) == [], "ledger rows of kernels the library does not hold"


def test_rows_hold_cases_and_nothing_else():
    fd, led = IC.finder(), IC.ledger()
    assert led["mac_cap"] == fd.MAC_CAP == 1 << 28 and tuple(led["updil"]) == fd.UPDIL and led["lowrank_rank"] == fd.LOWRANK_R
    for name, row in led["rows"].items():
        assert set(row) <= {"min", "ragged", "edge", "needs_device"} and row.get("min") is not None and "ragged" in row, name
        assert ("edge" in row) == (row["ragged"] is None), name
        assert row.get("needs_device", False) == (",walk" in name), name      # the walk's plan reads the device's CU count: no other row may
        for tag, c in IC.cases_of(row):
            assert tuple(sorted(c)) == tuple(sorted(fd.CASE_KEYS)), (name, tag)
            assert c["macs"] == fd.macs_of(c) > 0, (name, tag)
            if tag != "min":
                assert fd.is_ragged(name, c, strict=tag == "ragged"), (name, tag)
            if c["pool"] and not c["per_sample_x"] and not row.get("needs_device"):      # a pooled stem that must stay on the one-sample kernel
                assert c["spw"] == "1", (name, tag)


def test_every_row_replans_to_its_own_name(planner):
    led = IC.ledger()
    wrong = []
    for name, row in led["rows"].items():
        if row.get("needs_device"):
            continue
        for tag, c in IC.cases_of(row):
            got = planner.plan(c)
            if got != name:
                wrong.append((name, tag, got))
    assert wrong == []


def test_cost_cap():
    """Every case is at most 2^28 multiply-accumulates; the names whose cheapest case exceeds that are the fixture's ``over_budget``, at
    most 5 % of the names."""
    led = IC.ledger()
    cap = 1 << 28
    over = sorted(n for n, r in led["rows"].items() if r["min"]["macs"] > cap)
    assert over == led["over_budget"] == ["fused_split_quad_kernel<64,512,bf16x3,6 terms,pool=1,walk>"]
    assert 20 * len(over) <= len(led["rows"])
    for name, row in led["rows"].items():
        if name not in over:
            assert all(c["macs"] <= cap for _, c in IC.cases_of(row)), name


def test_names_without_a_ragged_case():
    """A split-precision kernel takes whole octets of input channels, so none of its cases has Ci off 8; the other names listed are
    the forms that need Ci % 4 == 0 or whole tiles. They keep an ``edge`` case where the neighbourhood holds one."""
    led = IC.ledger()
    none = sorted(n for n, r in led["rows"].items() if r["ragged"] is None)
    assert none == led["no_ragged"]
    split = {n for n in led["rows"] if n.startswith("fused_split_kernel<") or n.startswith("fused_split_direct_kernel<") or n.startswith("fused_split_skinny_kernel<")}
    assert split <= set(none)


def test_a_drifted_row_a_missing_row_and_a_new_instantiation_fail(library, planner):
    """The three ways the ledger goes stale, each shown to be seen."""
    names, _ = library
    have = set().union(*names.values())
    rows = IC.ledger()["rows"]
    name = "fused_split_kernel<64,256,bf16x3,6 terms,npw=8,xm=3>"
    assert planner.plan(rows[name]["min"]) == name
    assert planner.plan(dict(rows[name]["min"], B=1, S=1)) != name                    # a geometry edited so that it plans elsewhere
    assert have - (set(rows) - {name}) == {name}                                       # a name deleted from the fixture
    assert (have | {"fused_split_kernel<64,1024,bf16x3,6 terms,npw=4,xm=0>"}) - set(rows) != set()      # an instantiation without a row
