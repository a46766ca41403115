"""The ABI of field-qualified phrase clauses (fg_field_phrases): one new
symbol, no new flag value -- FG_ABI_VERSION stays 6 and fg_query_batch keeps its
layout.  Without a device: the header, the Rust binding, the Python binding and
INTEGRATION.md agree; the switch asks, sets and leaves the other seven alone; the
host parser answers as today while it is off -- "field-qualified phrase" included,
with fg_field_clauses on -- and parses `name:"..."` / `name:e-mail` with every
remaining refusal's message while both are on."""
import os
import re

import pytest

from conftest import ROOT

OTHERS = ("phrase_clauses", "group_clauses", "filter_clauses", "count_clauses", "group_phrase_clauses",
          "group_member_phrases", "field_clauses")
TODAY = "query syntax beyond bare/\\+/-/AND/OR terms"
QUOTED = TODAY + r" and plain quoted phrases \(slop, prefix, boost\)"


def _switch(name):
    from fugu_amd import native
    f = getattr(native, name)
    was = f()
    yield f
    f(was)


@pytest.fixture()
def switch():
    """sets fg_field_phrases; the setting found is restored in teardown"""
    yield from _switch("field_phrases")


@pytest.fixture()
def fields():
    yield from _switch("field_clauses")


@pytest.fixture()
def groups():
    yield from _switch("group_clauses")


def test_header_rust_python_and_doc_agree():
    from fugu_amd import native
    h = open(os.path.join(ROOT, "include", "fugu.h")).read()
    rs = open(os.path.join(ROOT, "rust", "ffi.rs")).read()
    assert re.search(r"\nint fg_field_phrases\(int on\);", h)
    assert "pub fn fg_field_phrases(on: c_int) -> c_int;" in rs
    assert hasattr(native.lib(), "fg_field_phrases") and "fg_field_phrases" in native.EXPORTS
    # no new flag value, the version and the batch layout stay
    assert re.search(r"#define FG_CLAUSE_TEXT 0x20000000u", h) and re.search(r"#define FG_CLAUSE_NAME 0x10000000u", h)
    assert re.search(r"#define FG_ABI_VERSION 6\b", h) and native.ABI_VERSION == 6 and native.lib().fg_abi_version() == 6
    assert [n for n, _ in native.QueryBatch._fields_] == ["n_queries", "q_off", "terms", "mode", "f_off", "f_terms",
                                                          "occur", "phrase_len", "phrase_pos"]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`fg_field_phrases`" in doc
    import field_phrase_ref as fp
    assert (fp.FLAG[fp.TEXT], fp.FLAG[fp.NAME]) == (native.CLAUSE_TEXT, native.CLAUSE_NAME)
    b = fp.batch([[fp.P([3, 4], fp.MUST, fp.NAME), fp.T(5, fp.SHOULD, fp.TEXT), fp.P([6, 7, 8], fp.SHOULD, None, [0, 1, 3])]])
    assert b[3].tolist() == [2 | native.CLAUSE_NAME, 0, 1 | native.CLAUSE_TEXT, 3, 0, 0]
    assert b[4].tolist() == [0, 1, 0, 0, 1, 3] and b[2].tolist() == [0, 0, 1, 1, 1, 1] and b[0].tolist() == [0, 6]


def test_the_switch_asks_sets_and_leaves_the_others_alone(switch):
    from fugu_amd import native
    others = [getattr(native, n) for n in OTHERS]
    before = [f() for f in others]
    assert switch == native.field_phrases
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


PHRASES = ('name:"annual report"', "name:e-mail", "text:user@example.com", '+name:"q3 report" +budget')


def test_parser_off_answers_as_today(switch, fields):
    from fugu_amd import db, native
    assert switch() == 0 and fields() == 0
    d = db.Database()
    for on in (0, 1):  # the new switch alone changes nothing: fg_field_clauses is off
        switch(on)
        for q in PHRASES + ("name:report e-mail",):
            for f in (db.parse_query_groups, db.parse_query_clauses):
                with pytest.raises(native.Unsupported, match="^libfugu error -5: " + TODAY + "$"):
                    f(q)
            with pytest.raises(native.Unsupported, match="query outside the device subset: " + TODAY + "$"):
                d.search(None, q)
    switch(0)
    fields(1)  # fg_field_clauses on, the new switch off: today's refusals
    for q in PHRASES + ('+name:"report"',):
        with pytest.raises(native.Unsupported, match="^libfugu error -5: field-qualified phrase$"):
            db.parse_query_groups(q)
        with pytest.raises(native.Unsupported, match="query outside the device subset: field-qualified phrase$"):
            d.search(None, q)
    assert db.parse_query_groups("name:report e-mail") == [(1, "name", ["report"]), (1, "phrase", ["e", "mail"])]
    assert db.parse_query_fields("+name:report +quarterly") == [(0, "report", "name"), (0, "quarterly", None)]
    with pytest.raises(native.Unsupported, match="a phrase clause"):
        db.parse_query_fields("name:report e-mail")
    d.close()


M, S, X = 0, 1, 2
ACCEPTED = [  # (query, parse_query_groups, parse_query_clause_lines)
    ('name:"annual report"', [(S, "name", ["annual", "report"])], ["1:name:annual@0 report@1"]),
    ("name:e-mail", [(S, "name", ["e", "mail"])], ["1:name:e@0 mail@1"]),
    ("text:user@example.com", [(S, "text", ["user", "example", "com"])], ["1:text:user@0 example@1 com@2"]),
    ('+name:"q3 report" +budget', [(M, "name", ["q3", "report"]), (M, "term", ["budget"])],
     ["0:name:q3@0 report@1", "0:budget@0"]),
    ("name:report e-mail", [(S, "name", ["report"]), (S, "phrase", ["e", "mail"])], ["1:name:report@0", "1:e@0 mail@1"]),
    ('budget -text:"draft copy"', [(S, "term", ["budget"]), (X, "text", ["draft", "copy"])],
     ["1:budget@0", "2:text:draft@0 copy@1"]),
    ('name:"a b" AND text:c-d AND e', [(M, "name", ["a", "b"]), (M, "text", ["c", "d"]), (M, "term", ["e"])],
     ["0:name:a@0 b@1", "0:text:c@0 d@1", "0:e@0"]),
    ('name:"a b" OR "c d" OR text:e', [(S, "name", ["a", "b"]), (S, "phrase", ["c", "d"]), (S, "text", ["e"])],
     ["1:name:a@0 b@1", "1:c@0 d@1", "1:text:e@0"]),
    ('+name:"report"', [(M, "name", ["report"])], ["0:name:report@0"]),  # a quoted literal of one token: a field term
    ('name:"Annual  (Report)"', [(S, "name", ["annual", "report"])], ["1:name:annual@0 report@1"]),  # analyzed, literal
    ('name:"a b" text:"a b"', [(S, "name", ["a", "b"]), (S, "text", ["a", "b"])], ["1:name:a@0 b@1", "1:text:a@0 b@1"]),
]
REFUSED = [
    ('name:"a b"~2', QUOTED),                             # slop / prefix / boost suffixes
    ('name:"a b"*', QUOTED),
    ('name:"a b"^2', QUOTED),
    ('+text:"a b"~1 c', QUOTED),
    (r'name:"a \" b"', "unterminated quoted literal"),    # an escape inside the literal: the quote ends early
    (r'name:"a\"b"c"', QUOTED),
    (r'name:"a \\ b"', "escape inside a quoted literal"),
    ('name:"..."', "a term analyzes to no token"),
    ('name:""', "a term analyzes to no token"),
    ("name:(a b)", "field-qualified group"),
    ('+name:("a b" OR c) d', "field-qualified group"),
    ("(name:e-mail b)", "field-qualified group"),         # a field word inside parentheses
    ('id:"a b"', r"field outside \[text, name\]"),
    ("namespace:e-mail", r"field outside \[text, name\]"),
    ('Name:"a b"', r"field outside \[text, name\]"),
    ("name:e-mail^2", TODAY),
    ("name:e-mail~1", TODAY),
    ('-name:"a b"', "MustNot clauses only"),
    ('name:"a b', "unterminated quoted literal"),
]


def test_parser_on(switch, fields, groups):
    from fugu_amd import db, native
    fields(1)
    switch(1)
    for q, kinds, lines in ACCEPTED:
        assert db.parse_query_groups(q) == kinds, q
        assert db.parse_query_clause_lines(q) == lines, q
        want = [(oc, toks[0] if len(toks) == 1 else toks, None if kind in ("term", "phrase") else kind)
                for oc, kind, toks in kinds]
        assert db.parse_query_fields(q) == want, q
        for f in (db.parse_query, db.parse_query_occur):  # the term-per-clause parsers cannot express them
            with pytest.raises(native.Unsupported):
                f(q)
    # the analyzer's offsets ride along: a dropped token leaves a hole
    assert db.parse_query_clause_lines("name:e-mail") == ["1:name:e@0 mail@1"]
    assert db.parse_query_occur("a -b") == [(S, "a"), (X, "b")]  # a query without a field: as before
    assert db.parse_query_groups("e-mail") == [(S, "phrase", ["e", "mail"])]
    for g in (0, 1):  # the refusals that stay, whatever fg_group_clauses says
        groups(g)
        for q, why in REFUSED:
            with pytest.raises(native.Unsupported, match="^libfugu error -5: " + why + "$"):
                db.parse_query_groups(q)
    groups(1)  # a field phrase inside a mixed-infix AND-run
    with pytest.raises(native.Unsupported, match="field-qualified group"):
        db.parse_query_groups('name:"a b" AND c OR d')
    assert db.parse_query_groups('name:"a b" OR c AND d') == [(S, "name", ["a", "b"]), (S, "all", ["c", "d"])]
    groups(0)
    d = db.Database()
    assert d.search(None, '+name:"q3 report" +budget') == []  # nothing committed: no hits, no plan
    assert d.search(None, "name:report e-mail") == []
    with pytest.raises(native.Unsupported, match="field clause in a count query"):
        d.facet_counts(None, "/", 'name:"annual report"')
    with pytest.raises(native.Unsupported, match="field clause in a count query"):
        d.facet_counts(None, "/", "name:e-mail")
    d.close()
    switch(0)
    with pytest.raises(native.Unsupported, match="field-qualified phrase"):  # the same process, off again
        db.parse_query_groups('name:"annual report"')
    fields(0)
    with pytest.raises(native.Unsupported, match=TODAY):
        db.parse_query_groups('name:"annual report"')


def test_null_arguments_still_fail_cleanly(switch, fields):
    from fugu_amd import native
    fields(1)
    switch(1)
    assert native.lib().fg_plan_create(None, None, 10, None) == native.FG_EINVAL
