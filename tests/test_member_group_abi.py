"""The ABI of fg_group_member_phrases: one new symbol --
FG_ABI_VERSION stays 6 and fg_query_batch keeps its layout.  Without a device: the
header, the Rust binding, the Python binding and INTEGRATION.md agree on the
symbol, the switch is off by default, asks / sets as fg_group_phrase_clauses does
and leaves the other five switches alone."""
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture()
def switches():
    """(group_clauses, group_member_phrases); the settings found are restored in teardown"""
    from fugu_amd import native
    fns = (native.group_clauses, native.group_member_phrases)
    was = [f() for f in fns]
    yield fns
    for f, w in zip(fns, was):
        f(w)


def test_header_rust_python_and_the_guide_agree():
    from fugu_amd import native
    h = open(os.path.join(ROOT, "include", "fugu.h")).read()
    rs = open(os.path.join(ROOT, "rust", "ffi.rs")).read()
    assert re.search(r"\nint fg_group_member_phrases\(int on\);", h)
    assert "pub fn fg_group_member_phrases(on: c_int) -> c_int;" in rs
    assert hasattr(native.lib(), "fg_group_member_phrases") and "fg_group_member_phrases" in native.EXPORTS
    assert re.search(r"#define FG_ABI_VERSION 6\b", h) and native.ABI_VERSION == 6 and native.lib().fg_abi_version() == 6
    assert [n for n, _ in native.QueryBatch._fields_] == ["n_queries", "q_off", "terms", "mode", "f_off", "f_terms",
                                                          "occur", "phrase_len", "phrase_pos"]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`fg_group_member_phrases`" in doc
    assert "k_mgroup" in native.Plan.seed_thresholds.__doc__


def test_the_switch_asks_and_sets(switches):
    from fugu_amd import native
    groups, members = switches
    assert members == native.group_member_phrases
    assert members() == 0 and members(-1) == 0  # off by default; < 0 only asks
    assert members(1) == 0 and members(-1) == 1
    assert members(0) == 1 and members() == 0
    assert members(7) == 0 and members(-5) == 1  # (any on != 0 turns it on)
    others = (groups, native.phrase_clauses, native.filter_clauses, native.count_clauses, native.group_phrase_clauses)
    assert [f() for f in others] == [0] * 5  # its own: the other five are untouched
    assert native.lib().fg_plan_create(None, None, 10, None) == native.FG_EINVAL


QUERIES = ["(e-mail OR email) server", '("new york" OR boston) pizza', "+(disk-full enospc) +error",
           "e-mail AND server OR host"]


def test_parser_off_gets_todays_refusals(switches):
    """fg_group_clauses alone: each query is refused as before, message included"""
    from fugu_amd import db, native
    groups, members = switches
    groups(1)
    today = ["a group member analyzes to several tokens", "a quoted literal inside a group",
             "a group member analyzes to several tokens", "a group member analyzes to several tokens"]
    for q, why in zip(QUERIES, today):
        with pytest.raises(native.Unsupported, match=why):
            db.parse_query_groups(q)
    for q in ('("a) b" OR c)', '("new york")'):
        with pytest.raises(native.Unsupported, match="a quoted literal inside a group"):
            db.parse_query_groups(q)
    assert members(1) == 0 and groups(0) == 1  # the new switch without fg_group_clauses: no parentheses at all
    with pytest.raises(native.Unsupported):
        db.parse_query_groups(QUERIES[0])


def test_parser_on(switches):
    from fugu_amd import db, native
    groups, members = switches
    groups(1)
    members(1)
    want = [
        ([(1, "any", [["e", "mail"], "email"]), (1, "term", ["server"])], ["1:(e@0 mail@1 | email)", "1:server@0"]),
        ([(1, "any", [["new", "york"], "boston"]), (1, "term", ["pizza"])], ["1:(new@0 york@1 | boston)", "1:pizza@0"]),
        ([(0, "any", [["disk", "full"], "enospc"]), (0, "term", ["error"])], ["0:(disk@0 full@1 | enospc)", "0:error@0"]),
        ([(1, "all", [["e", "mail"], "server"]), (1, "term", ["host"])], ["1:(e@0 mail@1 & server)", "1:host@0"]),
    ]
    for q, (clauses, lines) in zip(QUERIES, want):
        assert db.parse_query_groups(q) == clauses, q
        assert db.parse_query_clause_lines(q) == lines, q
    assert db.parse_query_groups('("a) b" OR c)') == [(1, "any", [["a", "b"], "c"])]  # a parenthesis inside quotes is literal
    assert db.parse_query_groups('("new york")') == [(1, "phrase", ["new", "york"])]   # one literal is that literal
    assert db.parse_query_clause_lines('("new york")') == ["1:new@0 york@1"]
    assert db.parse_query_groups("(e-mail)") == [(1, "phrase", ["e", "mail"])]
    # every existing answer is unchanged
    assert db.parse_query_groups("(a OR b) c") == [(1, "any", ["a", "b"]), (1, "term", ["c"])]
    assert db.parse_query_clause_lines("+(a b) -c") == ["0:(a | b)", "2:c@0"]
    assert db.parse_query_groups("a AND b OR c") == [(1, "all", ["a", "b"]), (1, "term", ["c"])]
    assert db.parse_query_groups('"new york" AND pizza OR "los angeles"') == [
        (1, "all", [["new", "york"], "pizza"]), (1, "phrase", ["los", "angeles"])]
    for q, why in (('("new york"~2 OR b)', "slop, prefix, boost"), ('("a\\\\b c" OR d)', "escape inside a quoted literal"),
                   ('("new york OR b)', "unterminated quoted literal"), ("((a b) OR c)", "a group inside a group"),
                   ('("..." OR b)', "a term analyzes to no token"), ("(a OR b", "unterminated group")):
        with pytest.raises(native.Unsupported, match=why):
            db.parse_query_groups(q)


def test_db_search_over_nothing_committed(switches):
    """no device: nothing committed, no plan"""
    from fugu_amd import db, native
    groups, members = switches
    d = db.Database()
    for q in QUERIES:  # fg_group_clauses off: the parser's answer of before
        with pytest.raises(native.Unsupported, match="query outside the device subset"):
            d.search(None, q)
    groups(1)
    for q in QUERIES:
        with pytest.raises(native.Unsupported, match="query outside the device subset"):
            d.search(None, q)
    members(1)
    for q in QUERIES + ['("a) b" OR c)', '("new york")']:
        assert d.search(None, q) == []
    d.close()


def test_counts_refuse_the_shape_as_unsupported(switches):
    """counts on this shape are out of scope: with fg_count_clauses on too, a query the parser accepts is still
    FG_EUNSUPPORTED (the answer a host falls back on), never FG_EINVAL from the count ABI; other shapes go on"""
    from fugu_amd import db, native
    groups, members = switches
    was = native.count_clauses()
    d = db.Database()
    try:
        groups(1), members(1), native.count_clauses(1)
        for q in QUERIES + ['("a) b" OR c)']:
            with pytest.raises(native.Unsupported, match="group with phrase members in a count query"):
                d.facet_counts(None, "/", query=q)
        assert d.facet_counts(None, "/", query="(server OR host) mail") == ([], 0)   # a plain group still counts
        assert d.facet_counts(None, "/", query='("new york")') == ([], 0)            # one literal: a phrase clause
        native.count_clauses(0)
        with pytest.raises(native.Unsupported, match="group clause in a count query"):  # as before
            d.facet_counts(None, "/", query=QUERIES[0])
    finally:
        native.count_clauses(was)
        d.close()
