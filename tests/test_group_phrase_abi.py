"""The ABI of fg_group_phrase_clauses: one new symbol --
FG_ABI_VERSION stays 6 and fg_query_batch keeps its layout.  Without a device: the
header, the Rust binding, the Python binding and INTEGRATION.md agree on the
symbol, the switch is off by default and asks / sets as fg_phrase_clauses does, and
fg_db's search of such a query over nothing committed plans nothing."""
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture()
def switches():
    """(group_clauses, group_phrase_clauses); the settings found are restored in teardown"""
    from fugu_amd import native
    fns = (native.group_clauses, native.group_phrase_clauses)
    was = [f() for f in fns]
    yield fns
    for f, w in zip(fns, was):
        f(w)


def test_header_rust_python_and_the_guide_agree():
    from fugu_amd import native
    h = open(os.path.join(ROOT, "include", "fugu.h")).read()
    rs = open(os.path.join(ROOT, "rust", "ffi.rs")).read()
    assert re.search(r"\nint fg_group_phrase_clauses\(int on\);", h)
    assert "unless\n * fg_group_phrase_clauses(1)" in h  # fg_group_clauses' list of refusals names the way out
    assert "pub fn fg_group_phrase_clauses(on: c_int) -> c_int;" in rs
    assert hasattr(native.lib(), "fg_group_phrase_clauses") and "fg_group_phrase_clauses" in native.EXPORTS
    assert re.search(r"#define FG_ABI_VERSION 6\b", h) and native.ABI_VERSION == 6 and native.lib().fg_abi_version() == 6
    assert [n for n, _ in native.QueryBatch._fields_] == ["n_queries", "q_off", "terms", "mode", "f_off", "f_terms",
                                                          "occur", "phrase_len", "phrase_pos"]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`fg_group_phrase_clauses`" in doc
    assert "k_gphrase" in native.Plan.seed_thresholds.__doc__


def test_the_switch_asks_and_sets(switches):
    from fugu_amd import native
    groups, gphrase = switches
    assert gphrase == native.group_phrase_clauses
    assert gphrase() == 0 and gphrase(-1) == 0  # off by default; < 0 only asks
    assert gphrase(1) == 0 and gphrase(-1) == 1
    assert gphrase(0) == 1 and gphrase() == 0
    assert gphrase(7) == 0 and gphrase(-5) == 1  # (any on != 0 turns it on)
    assert (groups(), native.phrase_clauses(), native.filter_clauses(), native.count_clauses()) == (0, 0, 0, 0)  # its own


def test_db_search_over_nothing_committed(switches):
    """no device: the parser yields these clause lists under fg_group_clauses alone; nothing committed, no plan"""
    from fugu_amd import db, native
    groups, gphrase = switches
    d = db.Database()
    queries = ["e-mail (server OR host)", '"new york" AND (pizza OR pasta)', "+(error failure) +disk-full",
               "state-of-the-art (gpu OR accelerator) -cpu"]
    for q in queries:  # fg_group_clauses off: the parser's answer of before
        with pytest.raises(native.Unsupported, match="query outside the device subset"):
            d.search(None, q)
    groups(1)
    assert db.parse_query_groups(queries[0]) == [(1, "phrase", ["e", "mail"]), (1, "any", ["server", "host"])]
    assert db.parse_query_groups(queries[2]) == [(0, "any", ["error", "failure"]), (0, "phrase", ["disk", "full"])]
    for on in (0, 1):
        gphrase(on)
        for q in queries:
            assert d.search(None, q) == []
    assert native.lib().fg_plan_create(None, None, 10, None) == native.FG_EINVAL
    d.close()
