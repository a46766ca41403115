"""The ABI of group clauses (fg_group_clauses): new symbols and
flag values only -- FG_ABI_VERSION stays 6 and fg_query_batch keeps its layout.
Without a device: the header, the Rust binding and the Python binding agree, and
the host refuses what it must with the switch on.  With one (marked gpu): the
phrase_len flag values get TODAY'S answer while the switch is off -- FG_EINVAL
"bad phrase_len at term N" from the planner (the flags make the member count
larger than the terms the query has left), "phrase clause in a count query" from
fg_count_batch (any value >= 2) and "the model does not cover phrase queries"
from fg_model_batch (any value != 1)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture()
def switch():
    """sets fg_group_clauses; the setting found is restored in teardown"""
    from fugu_amd import native
    was = native.group_clauses()
    yield native.group_clauses
    native.group_clauses(was)


def test_header_rust_and_python_agree():
    from fugu_amd import native
    h = open(os.path.join(ROOT, "include", "fugu.h")).read()
    rs = open(os.path.join(ROOT, "rust", "ffi.rs")).read()
    assert re.search(r"#define FG_CLAUSE_ANY 0x80000000u", h) and re.search(r"#define FG_CLAUSE_ALL 0x40000000u", h)
    assert re.search(r"\nint fg_group_clauses\(int on\);", h)
    assert "pub const FG_CLAUSE_ANY: u32 = 0x8000_0000;" in rs and "pub const FG_CLAUSE_ALL: u32 = 0x4000_0000;" in rs
    assert "pub fn fg_group_clauses(on: c_int) -> c_int;" in rs
    assert (native.CLAUSE_ANY, native.CLAUSE_ALL) == (0x80000000, 0x40000000)
    assert re.search(r"#define FG_ABI_VERSION 6\b", h) and native.ABI_VERSION == 6
    assert [n for n, _ in native.QueryBatch._fields_] == ["n_queries", "q_off", "terms", "mode", "f_off", "f_terms",
                                                          "occur", "phrase_len", "phrase_pos"]
    assert hasattr(native.lib(), "fg_group_clauses") and "fg_group_clauses" in native.EXPORTS
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`fg_group_clauses`" in doc and "FG_CLAUSE_ANY" in doc


def test_host_refusals_with_the_switch_on(switch):
    """no device: the parser and the count path of fg_db"""
    from fugu_amd import db, native
    d = db.Database()
    switch(1)
    for q in ("(a b) c", "a AND b OR c", "+(a AND b) c"):
        with pytest.raises(native.Unsupported, match="group clause in a count query"):
            d.facet_counts(None, "/", q)
        for f in (db.parse_query, db.parse_query_occur):
            with pytest.raises(native.Unsupported, match="group clause"):
                f(q)
    assert d.facet_counts(None, "/", "(a)") == ([], 0)  # a one-word group is that word
    assert d.search(None, "(a b) c") == []               # nothing committed: no hits, no plan
    switch(0)
    for q in ("(a b) c", "a AND b OR c"):  # off: the parser's answers of before
        with pytest.raises(native.Unsupported, match="query outside the device subset"):
            d.facet_counts(None, "/", q)
        with pytest.raises(native.Unsupported, match="query outside the device subset"):
            d.search(None, q)
    d.close()


def test_null_arguments_still_fail_cleanly(switch):
    from fugu_amd import native
    switch(1)
    assert native.lib().fg_plan_create(None, None, 10, None) == native.FG_EINVAL


@pytest.mark.gpu
def test_flag_values_with_the_switch_off_get_todays_answer(switch):
    from fugu_amd import native
    if native.device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    ctx = native.Context((0,))
    docs = [[0, 1, 2], [1, 2], [0, 2, 2], [1]]
    off = np.cumsum([0] + [len(x) for x in docs]).astype(np.uint64)
    ix = native.Index.from_docs(ctx, off, np.concatenate(docs).astype(np.uint32), 3)
    assert switch() == 0
    S = native.OCCUR_SHOULD
    for flag in (native.CLAUSE_ANY, native.CLAUSE_ALL, native.CLAUSE_ANY | native.CLAUSE_ALL):
        kw = dict(occur=[S, S, S], phrase_len=[2 | flag, 0, 1], phrase_pos=[0, 0, 0])
        with pytest.raises(native.FuguError, match=r"query 0: bad phrase_len at term 0") as e:
            ix.search_batch([0, 3], [0, 1, 2], 10, **kw)
        assert e.value.code == native.FG_EINVAL
        with pytest.raises(native.FuguError, match=r"query 0: bad phrase_len at term 0"):
            native.Plan([ix, ix], [0, 3], [0, 1, 2], 10, **kw)
        with pytest.raises(native.Unsupported, match="query 0: phrase clause in a count query"):
            native.count_batch([ix], [0, 3], [0, 1, 2], **kw)
        with pytest.raises(native.FuguError, match="the model does not cover phrase queries") as e:
            ix.model([0, 3], [0, 1, 2], 10, phrase_len=kw["phrase_len"], phrase_pos=kw["phrase_pos"])
        assert e.value.code == native.FG_EINVAL
    switch(1)  # on: the same arrays are a group query
    s, d, n = ix.search_batch([0, 3], [0, 1, 2], 10, occur=[S, S, S], phrase_len=[2 | native.CLAUSE_ANY, 0, 1],
                              phrase_pos=[0, 0, 0])
    assert int(n[0]) == 4
