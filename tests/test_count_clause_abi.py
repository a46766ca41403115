"""The ABI of phrase and group clauses in counts (fg_count_clauses):
two new symbols -- FG_ABI_VERSION stays 6 and fg_query_batch keeps its layout.
Without a device: the header, the Rust binding, the Python binding, INTEGRATION.md
and the library agree; the switch keeps the contract of fg_phrase_clauses; with it
on the host's count entry points take phrase and group queries, with it off they
refuse them as before."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture()
def switch():
    """sets fg_count_clauses; the setting found is restored in teardown"""
    from fugu_amd import native
    was = native.count_clauses()
    yield native.count_clauses
    native.count_clauses(was)


@pytest.fixture()
def groups():
    from fugu_amd import native
    was = native.group_clauses()
    yield native.group_clauses
    native.group_clauses(was)


def test_header_rust_python_doc_and_library_agree():
    from fugu_amd import native
    h = open(os.path.join(ROOT, "include", "fugu.h")).read()
    rs = open(os.path.join(ROOT, "rust", "ffi.rs")).read()
    assert re.search(r"\nint fg_count_clauses\(int on\);", h)
    assert re.search(r"\nint fg_count_clause_trace\(int enable, double\* ms_out, uint32_t\* calls\);", h)
    assert "pub fn fg_count_clauses(on: c_int) -> c_int;" in rs
    assert "pub fn fg_count_clause_trace(enable: c_int, ms_out: *mut f64, calls: *mut u32) -> c_int;" in rs
    assert re.search(r"#define FG_ABI_VERSION 6\b", h) and native.ABI_VERSION == 6
    assert native.lib().fg_abi_version() == 6
    assert [n for n, _ in native.QueryBatch._fields_] == ["n_queries", "q_off", "terms", "mode", "f_off", "f_terms",
                                                          "occur", "phrase_len", "phrase_pos"]
    assert "fg_count_clauses" in native.EXPORTS and "fg_count_clause_trace" in native.EXPORTS
    lib = ctypes.CDLL(native.LIB_PATH)  # the symbols themselves, not the binding's wrappers
    assert lib.fg_count_clauses is not None and lib.fg_count_clause_trace is not None
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "fg_count_clauses" in open(os.path.join(ROOT, doc)).read(), doc
    assert "`fg_count_clause_trace`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_switch_contract(switch):
    from fugu_amd import native
    assert switch() == 0  # off by default
    assert switch(1) == 0 and switch(-1) == 1 and switch(-7) == 1  # returns the previous setting; < 0 only asks
    assert (native.phrase_clauses(), native.group_clauses(), native.filter_clauses()) == (0, 0, 0)  # switches of their own
    assert switch(5) == 1 and switch(0) == 1 and switch() == 0
    was = native.phrase_clauses(1)
    try:
        assert switch() == 0
    finally:
        native.phrase_clauses(was)


def test_clause_trace_contract():
    from fugu_amd import native
    ms, calls = native.count_clause_trace(1)
    assert sorted(ms) == ["k_cjoin", "k_crow"] and calls == 0
    ms, calls = native.count_clause_trace(0)
    assert ms == {"k_crow": 0.0, "k_cjoin": 0.0} and calls == 0
    assert native.lib().fg_count_clause_trace(-1, None, None) == native.FG_OK


def test_host_counts_take_phrases_and_groups_when_on(switch, groups):
    from fugu_amd import db
    switch(1)
    d = db.Database()
    try:
        assert d.facet_counts(None, "/", '"new york"') == ([], 0)
        assert d.facet_counts(None, "/", 'alpha "new york"') == ([], 0)
        with pytest.raises(db.native.Unsupported):  # the parser is unchanged: a group needs fg_group_clauses to parse
            d.facet_counts(None, "/", "(a b) c")
        groups(1)
        assert d.facet_counts(None, "/", "(a b) c") == ([], 0)
        assert d.facet_counts(None, "/", '(a AND b) "new york"', filters=["/org/1"]) == ([], 0)
    finally:
        d.close()


def test_host_counts_refuse_them_when_off(switch, groups):
    from fugu_amd import db
    assert switch() == 0
    d = db.Database()
    try:
        for q in ('"new york"', 'alpha "new york"'):
            with pytest.raises(db.native.Unsupported) as e:
                d.facet_counts(None, "/", q)
            assert "query outside the device subset: phrase clause in a count query" in str(e.value)
        groups(1)
        with pytest.raises(db.native.Unsupported) as e:
            d.facet_counts(None, "/", "(a b) c")
        assert "query outside the device subset: group clause in a count query" in str(e.value)
        assert d.facet_counts(None, "/", "alpha beta") == ([], 0)
    finally:
        d.close()


def test_null_arguments_still_fail_cleanly(switch):
    from fugu_amd import native
    switch(1)
    assert native.lib().fg_count_batch(None, 0, None, None, 0, None, None) == native.FG_EINVAL
