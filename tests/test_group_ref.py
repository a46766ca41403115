"""Group clauses without a GPU: the switch, the parser, the
reference's identities, and the conditions of the generator whose queries
test_gpu_group.py runs -- that every kind is there, that the grouping decides
which docs hit, and that the nested f32 sum really differs from the flat one.
Every test that sets the switch does so through the `switch` fixture, which
restores the setting it found."""
import numpy as np
import pytest

import bool_ref as br
import group_ref as gr

M, S, X = gr.MUST, gr.SHOULD, gr.MUST_NOT
ANY, ALL = gr.ANY, gr.ALL
F = np.float32


@pytest.fixture()
def switch():
    """sets fg_group_clauses; the setting found is restored in teardown"""
    from fugu_amd import native
    was = native.group_clauses()
    yield native.group_clauses
    native.group_clauses(was)


@pytest.fixture()
def on(switch):
    switch(1)


# ------------------------------------------------------------------ the switch
def test_native_binds_the_switch(switch):
    from fugu_amd import native
    assert "fg_group_clauses" in native.EXPORTS and switch == native.group_clauses
    assert switch() == 0 and switch(-1) == 0  # off by default; < 0 only asks
    assert switch(1) == 0 and switch(-1) == 1
    assert switch(0) == 1 and switch() == 0
    assert switch(7) == 0 and switch(-5) == 1  # (any on != 0 turns it on)
    assert native.phrase_clauses() == 0        # (a switch of its own)
    assert (native.CLAUSE_ANY, native.CLAUSE_ALL) == (1 << 31, 1 << 30) == (gr.FLAG[ANY], gr.FLAG[ALL])
    assert native.ABI_VERSION == 6 and native.lib().fg_abi_version() == 6


# ------------------------------------------------------------------ the parser
ACCEPTED = [
    ("(rust OR golang) AND tutorial", ["0:(rust | golang)", "0:tutorial@0"]),
    ("+(error failure) +disk", ["0:(error | failure)", "0:disk@0"]),
    ("a AND b OR c", ["1:(a & b)", "1:c@0"]),
    ("(a b c)", ["1:(a | b | c)"]),
    ("(a OR b)", ["1:(a | b)"]),
    ("(a AND b)", ["1:(a & b)"]),
    ("(+a +b)", ["1:(a & b)"]),
    ("-(a b) c", ["2:(a | b)", "1:c@0"]),
    ("a -(b c)", ["1:a@0", "2:(b | c)"]),
    ("+(a AND b) -(c AND d) e", ["0:(a & b)", "2:(c & d)", "1:e@0"]),
    ("(a b) OR (c AND d) OR e", ["1:(a | b)", "1:(c & d)", "1:e@0"]),
    ("(a b) AND (c d)", ["0:(a | b)", "0:(c | d)"]),
    ("a AND b OR c AND d", ["1:(a & b)", "1:(c & d)"]),
    ("a OR b AND c AND d OR e", ["1:a@0", "1:(b & c & d)", "1:e@0"]),
    ("(a b) OR c AND d", ["1:(a | b)", "1:(c & d)"]),
    ("e-mail OR a AND b", ["1:e@0 mail@1", "1:(a & b)"]),
    ("(a)", ["1:a@0"]),                  # a one-word group is that word
    ("+(a) -( b )", ["0:a@0", "2:b@0"]),
    ("(  Rust   GoLang )", ["1:(rust | golang)"]),
    ("(a a)", ["1:(a | a)"]),
]
REFUSED = [
    ("(a -b)", "MustNot member inside a group"),
    ("(-a -b)", "MustNot member inside a group"),
    ("(+a b)", "mixed prefixes inside a group"),
    ("(a AND b OR c)", "mixed AND / OR inside a group"),
    ("(+a AND +b)", "prefix beside AND / OR inside a group"),
    ("((a b) c)", "group inside a group"),
    ("(a (b c))", "group inside a group"),
    ('(a "b c")', "quoted literal inside a group"),
    ("(e-mail b)", "group member analyzes to several tokens"),
    ("()", "empty group"),
    ("(  )", "empty group"),
    ("(a b", "unterminated group"),
    ("(a b)^2", "after a group"),
    ("(a b) AND c OR d", "group inside a group"),   # AND binds tighter: ((a b) AND c) OR d nests two levels
    ('"x y" AND b OR c', "quoted literal inside a group"),
    ("e-mail AND b OR c", "group member analyzes to several tokens"),
    ("+a AND b OR c", "beyond bare"),
    ("-(a b)", "MustNot clauses only"),
    ("(a AND)", "operator outside the supported forms"),
    ("(... b)", "analyzes to no token"),
]
NEW_FORMS = [q for q, _ in ACCEPTED + REFUSED]


@pytest.mark.parametrize("q,want", ACCEPTED)
def test_parser_accepts(on, q, want):
    from fugu_amd import db
    assert db.parse_query_clause_lines(q) == want


@pytest.mark.parametrize("q,why", REFUSED)
def test_parser_refuses_with_its_reason(on, q, why):
    from fugu_amd import db, native
    with pytest.raises(native.Unsupported, match=why.replace("(", r"\(")):
        db.parse_query_clause_lines(q)


@pytest.mark.parametrize("q", NEW_FORMS)
def test_switch_off_refuses_every_new_form(switch, q):
    from fugu_amd import db, native
    assert switch() == 0
    with pytest.raises(native.Unsupported):
        db.parse_query_clauses(q)
    with pytest.raises(native.Unsupported):
        db.parse_query(q)


def test_parser_helpers_and_the_term_per_clause_forms(on):
    from fugu_amd import db, native
    assert db.parse_query_groups("+(a b) -(c AND d) e-mail f") == [
        (M, "any", ["a", "b"]), (X, "all", ["c", "d"]), (S, "phrase", ["e", "mail"]), (S, "term", ["f"])]
    for f in (db.parse_query, db.parse_query_occur):  # their outputs cannot express a group
        with pytest.raises(native.Unsupported, match="group clause"):
            f("(a b) c")
        with pytest.raises(native.Unsupported, match="group clause"):
            f("a AND b OR c")
    # the forms of before parse as before with the switch on
    assert db.parse_query_occur("a -b +c") == [(S, "a"), (X, "b"), (M, "c")]
    assert db.parse_query_clauses("a AND e-mail") == [(M, [("a", 0)]), (M, [("e", 0), ("mail", 1)])]
    assert db.parse_query_occur("(a)") == [(S, "a")]


# ------------------------------------------------------------------ the reference's identities
@pytest.fixture(scope="module")
def gen():
    c = gr.synth()
    ref = gr.Ref(c.corpus)
    qs = gr.queries()
    return c, ref, qs


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_identities(gen):
    c, ref, _ = gen
    cor = c.corpus
    for a, b, d in ((6, 7, 8), (gr.T_2047, 9, gr.T_LONG), (48, 7, 49), (gr.T_FEW, gr.T_EVERY, 6)):
        for bounds in (None, gr.SEG_CUTS):
            kw = dict(seg_bounds=bounds)
            # one any-of group = the flat Should query; one all-of group = the flat Must query, bit for bit
            assert same_bits(ref.hits([gr.G(S, ANY, [a, b, d])], **kw), cor._hits([a, b, d], [S] * 3, None, bounds, None))
            assert same_bits(ref.hits([gr.G(M, ANY, [a, b, d])], **kw), cor._hits([a, b, d], [S] * 3, None, bounds, None))
            assert same_bits(ref.hits([gr.G(S, ALL, [a, b, d])], **kw), cor._hits([a, b, d], [M] * 3, None, bounds, None))
            assert same_bits(ref.hits([gr.G(M, ALL, [b, a])], **kw), cor._hits([b, a], [M] * 2, None, bounds, None))
            # a -(b c) = a -b -c
            assert same_bits(ref.hits([gr.T(S, a), gr.G(X, ANY, [b, d])], **kw),
                             cor._hits([a, b, d], [S, X, X], None, bounds, None))
    assert len(ref.hits([gr.G(S, ALL, [6, 7, 8])])[0]) > 0


def test_costs_and_the_must_order(gen):
    """any-of: the sum of the members' costs; all-of: the smallest; the Musts join in (cost, position) order"""
    c, ref, _ = gen
    st = c.corpus.own
    cost = lambda t, lo=0, hi=gr.N: ref._clause(t, lo, hi, st)[1]  # noqa: E731
    a, b, d = 6, 7, gr.T_2047
    assert cost((ANY, [a, b])) == cost(a) + cost(b) and cost((ALL, [a, b])) == min(cost(a), cost(b))
    assert cost((ALL, [a, gr.T_FEW]), 0, 3000) == 0 and cost((ANY, [a, gr.T_FEW]), 0, 3000) == cost(a, 0, 3000)
    sa, sb, sd = (c.corpus.clause(t, st)[0] for t in (a, b, d))
    both = np.flatnonzero((sa >= 0) & (sb >= 0) & (sd >= 0) & c.corpus.alive)
    assert len(both) > 10
    docs, sc = ref.hits([gr.G(M, ANY, [a, b]), gr.T(M, d)])
    got = dict(zip(docs.tolist(), sc))
    z = F(0.0)
    for x in both[:10]:  # the term is the cheaper clause: (0.0 + (s_d + ((0.0 + s_a) + s_b)))
        assert cost(d) < cost((ANY, [a, b]))
        assert got[int(x)] == F(z + (sd[x] + ((z + sa[x]) + sb[x])))
    docs, sc = ref.hits([gr.G(M, ALL, [a, b]), gr.T(M, gr.T_LONG)])
    sl = c.corpus.clause(gr.T_LONG, st)[0]
    lo, hi = sorted((a, b), key=cost)
    s_lo, s_hi = (c.corpus.clause(t, st)[0] for t in (lo, hi))
    x = int(docs[0])
    assert F(sc[0]) == F(z + ((z + ((s_lo[x] + s_hi[x]) + z)) + sl[x]))  # (the group's cost, its smallest member's, is lower)


# ------------------------------------------------------------------ the generator
def test_corpus_has_the_edge_lists(gen):
    c, _, _ = gen
    assert c.corpus.n == gr.N <= 12000 and gr.V <= 64
    for t, n in gr.EDGE_LEN.items():
        assert c.merged_len(t) == n, t
    assert sorted(gr.EDGE_LEN.values()) == [40, 2047, 2048, 2049, 8193]  # kChunk's edges, past 4 chunks, < 64
    assert c.merged_len(gr.T_ABSENT) == 0 and c.merged_len(gr.T_EVERY) == gr.N
    assert c.corpus.docs(gr.T_FEW).min() >= gr.SEG_CUTS[2] and c.corpus.docs(gr.T_LOW).max() < gr.SEG_CUTS[1]
    assert all(len(c.corpus.docs(t, 0)) == 0 and len(c.corpus.docs(t, 1)) > 0 for t in gr.NAME_ONLY)
    assert all(0 < len(c.corpus.docs(t, 1)) < len(c.corpus.docs(t, 0)) for t in gr.NAME_TOO)
    assert 0 < c.deleted.sum() < gr.N // 10
    tf = np.bincount(c.text_tok[int(c.text_off[c.corpus.docs(gr.T_2047)[7]]):
                                int(c.text_off[c.corpus.docs(gr.T_2047)[7] + 1])], minlength=2)[gr.T_2047]
    assert tf == 300  # an escaped tf byte


def test_generator_conditions(gen):
    c, ref, qs = gen
    assert set(qs) == set(gr.KINDS) and set(gr.MUST_KINDS) <= set(gr.DECIDING)
    gone = lambda t: t in gr.GONE or t == gr.T_ABSENT  # noqa: E731
    n_hit = 0
    for kind in gr.KINDS:
        assert len(qs[kind]) >= 12, kind
        bits_differ = 0
        for q in qs[kind]:
            assert gr.n_terms_of(q) <= 16 and any(gr.is_group(b) for _, b in q)
            assert all(len(b[1]) >= 2 for _, b in q if gr.is_group(b))
            d, s = ref.hits(q)
            fd, fs = ref.hits(gr.flatten(q))
            n_hit += len(d) > 0
            must_gone = any(oc == M and gr.is_group(b) and b[0] == ALL and any(gone(t) for t in b[1]) for oc, b in q)
            if kind in gr.DECIDING and not must_gone:
                assert set(d.tolist()) != set(fd.tolist()), (kind, q)
            if must_gone:  # an all-of Must group with a missing member empties the query, nested or flat
                assert len(d) == 0 and len(fd) == 0
            if kind in ("sgrp_must", "xany"):
                assert set(d.tolist()) == set(fd.tolist()), (kind, q)
            both, i, j = np.intersect1d(d, fd, return_indices=True)
            bits_differ += bool((s[i].view(np.uint32) != fs[j].view(np.uint32)).any())
        print(kind, "queries whose nested sum differs bitwise from the flat one on a shared doc:", bits_differ)
        if kind in gr.MUST_KINDS:
            assert bits_differ >= 1, kind
    assert n_hit >= 0.9 * sum(len(v) for v in qs.values())
    # what each kind is
    for q in qs["many_mt"]:
        assert [(oc, gr.is_group(b) and b[0]) for oc, b in q] == [(M, ANY), (M, False)]
    for q in qs["many_many"]:
        assert [(oc, b[0]) for oc, b in q if gr.is_group(b)] == [(M, ANY)] * 2 and all(oc != M or gr.is_group(b) for oc, b in q)
    for q in qs["sall_sall"]:
        assert all(oc == S for oc, _ in q) and sum(gr.is_group(b) and b[0] == ALL for _, b in q) == 2
    for q in qs["sgrp_must"]:
        assert {oc for oc, _ in q} == {M, S} and all(gr.is_group(b) for oc, b in q if oc == S)
    assert all(any(oc == X and b[0] == ANY for oc, b in q if gr.is_group(b)) for q in qs["xany"])
    assert all(any(oc == X and b[0] == ALL for oc, b in q if gr.is_group(b)) for q in qs["xall"])
    for kind, k in (("miss_any", ANY), ("miss_all", ALL)):
        assert all(any(gr.is_group(b) and b[0] == k and any(gone(t) for t in b[1]) for _, b in q) for q in qs[kind])
        assert {t for q in qs[kind] for _, b in q if gr.is_group(b) for t in b[1] if gone(t)} == set(gr.GONE) | {gr.T_ABSENT}
    assert {oc for q in qs["miss_all"] for oc, b in q if gr.is_group(b) and any(gone(t) for t in b[1])} == {M, S, X}
    for q in qs["repeat"]:
        flat = [t for _, t in gr.flatten(q)]
        assert len(set(flat)) < len(flat)
    for q in qs["t16"]:
        assert gr.n_terms_of(q) == 16 and len(q) == 4 and all(gr.is_group(b) and len(b[1]) == 4 for _, b in q)
    for q in qs["name"]:
        assert any(t in gr.NAME_ONLY for _, t in gr.flatten(q)) and any(t in gr.NAME_TOO for _, t in gr.flatten(q))
    # a query whose k-th and (k + 1)-th hits tie on score, at a k of the GPU test
    ties = set()
    for q in qs["tie"]:
        s, _ = ref.search(q, 1001)
        ties |= {k for k in gr.KS if len(s) > k and s[k - 1] == s[k]}
    assert ties >= {10, 100}, ties
    # every edge list is some pass's lead: a Must term beside an any-of group, and a Should all-of group's member
    assert {q[1][1] for q in qs["many_mt"]} == set(gr.EDGE_LEN)
    assert {q[0][1][1][0] for q in qs["sall_sall"]} == set(gr.EDGE_LEN)


def test_chunk_bound_fires_on_the_long_list(gen):
    """k_group's skip rule in the reference's numbers: a `tie` query leads from T_LONG's list (one pass: its other
    member is absent, the second Must group is T_EVERY alone); after the first 2048-posting chunk the k-th best
    key (k = 1, 10, 100) lies above every later chunk's bound -- the chunk's largest T_LONG score plus T_EVERY's
    largest score -- so those chunks are skipped, and no hit of theirs belongs to the top k"""
    c, ref, qs = gen
    q = [gr.G(M, ANY, [gr.T_LONG, gr.T_ABSENT]), gr.G(M, ANY, [gr.T_EVERY, gr.GONE[0]])]
    assert q in qs["tie"]
    st = c.corpus.own
    s_long, s_every = c.corpus.clause(gr.T_LONG, st)[0], c.corpus.clause(gr.T_EVERY, st)[0]
    docs = np.flatnonzero(s_long >= 0)
    assert len(docs) == 8193
    total = (F(0.0) + ((F(0.0) + s_long[docs]) + (F(0.0) + s_every[docs]))).astype(F)
    first = np.sort(total[:2048][c.corpus.alive[docs[:2048]]])[::-1]
    for k in (1, 10, 100):
        for ch in range(1, 5):
            bound = F(F(s_long[docs[ch * 2048:(ch + 1) * 2048]].max() + s_every.max()) * F(1.00000762939453125))
            assert bound < first[k - 1], (k, ch)
        assert set(ref.search(q, k)[1].tolist()) <= set(docs[:2048].tolist())


def test_batch_encoding():
    q_off, terms, occur, plen, ppos = gr.batch([[gr.G(M, ANY, [3, 4, 5]), gr.T(S, 9)], [gr.G(X, ALL, [1, 2])]])
    assert q_off.tolist() == [0, 4, 6] and terms.tolist() == [3, 4, 5, 9, 1, 2]
    assert occur.tolist() == [M, M, M, S, X, X] and not ppos.any()
    assert plen.tolist() == [3 | 1 << 31, 0, 0, 1, 2 | 1 << 30, 0]
