"""The ABI of field-qualified term clauses (fg_field_clauses): new
symbols and flag values only -- FG_ABI_VERSION stays 6 and fg_query_batch keeps its
layout.  Without a device: the header, the Rust binding, the Python binding and
INTEGRATION.md agree; the switch asks, sets and leaves the other six alone; the
host parser answers as today while it is off and parses `text:WORD` / `name:WORD`
with every refusal's message while it is on."""
import os
import re

import pytest

from conftest import ROOT

OTHERS = ("phrase_clauses", "group_clauses", "filter_clauses", "count_clauses", "group_phrase_clauses",
          "group_member_phrases")
TODAY = "query syntax beyond bare/\\+/-/AND/OR terms"


@pytest.fixture()
def switch():
    """sets fg_field_clauses; the setting found is restored in teardown"""
    from fugu_amd import native
    was = native.field_clauses()
    yield native.field_clauses
    native.field_clauses(was)


@pytest.fixture()
def groups():
    """sets fg_group_clauses; the setting found is restored in teardown"""
    from fugu_amd import native
    was = native.group_clauses()
    yield native.group_clauses
    native.group_clauses(was)


def test_header_rust_python_and_doc_agree():
    from fugu_amd import native
    h = open(os.path.join(ROOT, "include", "fugu.h")).read()
    rs = open(os.path.join(ROOT, "rust", "ffi.rs")).read()
    assert re.search(r"#define FG_CLAUSE_TEXT 0x20000000u", h) and re.search(r"#define FG_CLAUSE_NAME 0x10000000u", h)
    assert re.search(r"\nint fg_field_clauses\(int on\);", h)
    assert "pub const FG_CLAUSE_TEXT: u32 = 0x2000_0000;" in rs and "pub const FG_CLAUSE_NAME: u32 = 0x1000_0000;" in rs
    assert "pub fn fg_field_clauses(on: c_int) -> c_int;" in rs
    assert (native.CLAUSE_TEXT, native.CLAUSE_NAME) == (0x20000000, 0x10000000)
    # beside the group flags, no bit shared
    assert not (native.CLAUSE_TEXT | native.CLAUSE_NAME) & (native.CLAUSE_ANY | native.CLAUSE_ALL)
    assert re.search(r"#define FG_ABI_VERSION 6\b", h) and native.ABI_VERSION == 6 and native.lib().fg_abi_version() == 6
    assert [n for n, _ in native.QueryBatch._fields_] == ["n_queries", "q_off", "terms", "mode", "f_off", "f_terms",
                                                          "occur", "phrase_len", "phrase_pos"]
    assert hasattr(native.lib(), "fg_field_clauses") and "fg_field_clauses" in native.EXPORTS
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`fg_field_clauses`" in doc and "FG_CLAUSE_TEXT" in doc and "FG_CLAUSE_NAME" in doc
    import field_ref as fr
    assert (fr.FLAG[fr.TEXT], fr.FLAG[fr.NAME]) == (native.CLAUSE_TEXT, native.CLAUSE_NAME)


def test_the_switch_asks_sets_and_leaves_the_others_alone(switch):
    from fugu_amd import native
    others = [getattr(native, n) for n in OTHERS]
    before = [f() for f in others]
    assert switch == native.field_clauses
    assert switch() == 0 and switch(-1) == 0  # off by default; < 0 only asks
    assert switch(1) == 0 and switch(-1) == 1
    assert [f() for f in others] == before
    assert switch(0) == 1 and switch() == 0
    assert switch(7) == 0 and switch(-5) == 1  # (any on != 0 turns it on)
    assert [f() for f in others] == before
    for f, was in zip(others, before):  # and none of them sets it
        assert f(1) == was
        assert switch() == 1
        f(was)
    assert switch(0) == 1


def test_parser_off_answers_as_today(switch):
    from fugu_amd import db, native
    assert switch() == 0
    d = db.Database()
    for q in ("name:report", "+name:report +quarterly", "text:a OR name:b"):
        for f in (db.parse_query_groups, db.parse_query_clauses, db.parse_query, db.parse_query_occur):
            with pytest.raises(native.Unsupported, match="^libfugu error -5: " + TODAY + "$"):
                f(q)
        with pytest.raises(native.Unsupported, match="query outside the device subset: " + TODAY + "$"):
            d.search(None, q)
        with pytest.raises(native.Unsupported, match="query outside the device subset: " + TODAY + "$"):
            d.facet_counts(None, "/", q)
    d.close()


M, S, X = 0, 1, 2
ACCEPTED = [
    ("name:report", [(S, "report", "name")]),
    ("text:error", [(S, "error", "text")]),
    ("+name:report +quarterly", [(M, "report", "name"), (M, "quarterly", None)]),
    ("text:a OR name:b", [(S, "a", "text"), (S, "b", "name")]),
    ("text:a AND name:b AND c", [(M, "a", "text"), (M, "b", "name"), (M, "c", None)]),
    ("a -name:b", [(S, "a", None), (X, "b", "name")]),
    ("+text:a name:b c", [(M, "a", "text"), (S, "b", "name"), (S, "c", None)]),
    ("name:a text:a", [(S, "a", "name"), (S, "a", "text")]),
    ("  name:Report   TEXT ", [(S, "report", "name"), (S, "text", None)]),  # WORD is analyzed, the field is not
    ("name:name text:text", [(S, "name", "name"), (S, "text", "text")]),
]
REFUSED = [
    ("name:e-mail", "field-qualified phrase"),         # WORD analyzes to several tokens
    ("text:user@example.com", "field-qualified phrase"),
    ('name:"quarterly report"', "field-qualified phrase"),
    ('+name:"report"', "field-qualified phrase"),        # a quoted literal, whatever it holds
    ("name:(a b)", "field-qualified group"),
    ("+name:(a OR b) c", "field-qualified group"),
    ("(name:a b)", "field-qualified group"),             # a field word inside parentheses
    ("(b name:a) c", "field-qualified group"),
    ("id:x", r"field outside \[text, name\]"),
    ("namespace:prod report", r"field outside \[text, name\]"),
    ("+organization:acme", r"field outside \[text, name\]"),
    ("Name:report", r"field outside \[text, name\]"),    # the field name exactly as the schema writes it
    ("TEXT:a", r"field outside \[text, name\]"),
    ("name:", "a term analyzes to no token"),
    ("name:...", "a term analyzes to no token"),
    ("name:a^2", TODAY),                                  # boosts, ranges and the rest: as before
    ("name:[a TO b]", TODAY),
    (":a", TODAY),
    ("-name:a", "MustNot clauses only"),
    ("name:a AND", "operator outside the supported forms"),
]


def test_parser_on(switch, groups):
    from fugu_amd import db, native
    switch(1)
    for q, want in ACCEPTED:
        assert db.parse_query_fields(q) == want, q
        kinds = [(oc, f or "term", [t]) for oc, t, f in want]
        assert db.parse_query_groups(q) == kinds, q
        if any(f for _, _, f in want):  # the term-per-clause parsers cannot express a field
            for f in (db.parse_query, db.parse_query_occur):
                with pytest.raises(native.Unsupported, match="a field-qualified term"):
                    f(q)
    assert db.parse_query_clause_lines("+name:report quarterly") == ["0:name:report@0", "1:quarterly@0"]
    assert db.parse_query_occur("a -b") == [(S, "a"), (X, "b")]  # a query without a field: as before
    for g in (0, 1):  # the refusals, whatever fg_group_clauses says
        groups(g)
        for q, why in REFUSED:
            with pytest.raises(native.Unsupported, match="^libfugu error -5: " + why + "$"):
                db.parse_query_groups(q)
    groups(1)  # a field word inside a mixed-infix AND-run; alone beside one it stands as it is
    with pytest.raises(native.Unsupported, match="field-qualified group"):
        db.parse_query_groups("name:a AND b OR c")
    with pytest.raises(native.Unsupported, match="field-qualified group"):
        db.parse_query_groups("c OR b AND text:a")
    assert db.parse_query_groups("name:a OR b AND c") == [(S, "name", ["a"]), (S, "all", ["b", "c"])]
    groups(0)
    d = db.Database()
    assert d.search(None, "+name:report +quarterly") == []  # nothing committed: no hits, no plan
    with pytest.raises(native.Unsupported, match="field clause in a count query"):
        d.facet_counts(None, "/", "name:report")
    with pytest.raises(native.Unsupported, match="query outside the device subset: field-qualified phrase"):
        d.search(None, "name:e-mail")
    d.close()
    switch(0)
    with pytest.raises(native.Unsupported, match=TODAY):  # the same process, off again
        db.parse_query_groups("name:report")


def test_null_arguments_still_fail_cleanly(switch):
    from fugu_amd import native
    switch(1)
    assert native.lib().fg_plan_create(None, None, 10, None) == native.FG_EINVAL
