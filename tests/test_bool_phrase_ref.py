"""Phrase clauses beside other clauses, the parts that need no GPU: the binding
of the switch, the reference (tests/bool_phrase_ref.py) against a hand-derived
known answer, and the conditions the GPU tests' queries must meet so they
cannot pass vacuously.

Known answer on phrase_ref.kat_corpus(): d0 = `a b c`, d1 = `a a b`,
d2 = `b c d e`, d3 = `a a a` (text only; a=0 b=1 c=2 d=3 e=4).  By hand:
  "a b" is in d0 (position 0) and d1 (position 1); "b c" in d0 and d2; "a a" in
  d1 (once) and d3 (twice); c is in d0 and d2; d in d2; b in d0, d1, d2.
  "a b" c    (Should, Should): {d0, d1} | {d0, d2} = {0, 1, 2}; d0 sums both
  +"a b" +c  : {d0, d1} & {d0, d2} = {0}
  +"b c" -d  : {d0, d2} - {d2} = {0}
  c -"a b"   : {d0, d2} - {d0, d1} = {2}
  +"a a" b   : {d1, d3}; b is in d1 alone, so d1 = (0.0 + "a a"(d1)) + (0.0 + b(d1))
               and d3 = 0.0 + "a a"(d3)
The clause scores themselves are phrase_ref's and bool_ref's (each pinned by its
own known answer in test_phrase_ref.py / test_bool_ref.py).

  +b +"a b" +c, +"a b" +b +c, +a +b +"b c": {d0} each; three Musts, so the (cost,
               position) order shows in the sum's bits (test_must_order_... below)

Generator conditions (conditions, not measurements).  Every kind has >= 16
queries and >= 75% of the queries of every kind have a hit.  For >= 50% of the
queries of every kind the hit SET differs from the same query with each phrase
replaced by the conjunction of its terms -- with ONE exception, mt_sp: a Should
phrase beside a Must term never changes which docs hit (it only adds score), so
there the condition is that for >= 50% the phrase matches some hit.  Each kind
is also held to what it is for: `name` phrases hold a name-only id, `missing`
has the missing term as Must, Should and MustNot (a missing Must: no hits),
`repeat` holds its phrase's repeated term as a clause, `t16` has 16 terms.
"""
import numpy as np
import pytest

import bool_phrase_ref as bp
import bool_ref as br
import phrase_ref as pr

M, S, X = bp.MUST, bp.SHOULD, bp.MUST_NOT
F = np.float32

KAT = [
    ("sp_sc", [bp.P([0, 1], S), bp.T(2, S)], {0, 1, 2}),
    ("mp_mc", [bp.P([0, 1], M), bp.T(2, M)], {0}),
    ("mp_xd", [bp.P([1, 2], M), bp.T(3, X)], {0}),
    ("sc_xp", [bp.T(2, S), bp.P([0, 1], X)], {2}),
    ("mp_sb", [bp.P([0, 0], M), bp.T(1, S)], {1, 3}),
    # three Musts: costs b 3, "a b" 3, c 2 -> c, b, "a b" / c, "a b", b; a 3, b 3, "b c" min(3, 2) = 2 -> "b c", a, b
    ("mb_mp_mc", [bp.T(1, M), bp.P([0, 1], M), bp.T(2, M)], {0}),
    ("mp_mb_mc", [bp.P([0, 1], M), bp.T(1, M), bp.T(2, M)], {0}),
    ("ma_mb_mp", [bp.T(0, M), bp.T(1, M), bp.P([1, 2], M)], {0}),
]


@pytest.fixture()
def switch():
    """sets fg_phrase_clauses; the setting found is restored in teardown"""
    from fugu_amd import native
    was = native.phrase_clauses()
    yield native.phrase_clauses
    native.phrase_clauses(was)


def test_native_binds_the_switch(switch):
    from fugu_amd import native
    assert "fg_phrase_clauses" in native.EXPORTS and switch == native.phrase_clauses
    assert switch() == 0 and switch(-1) == 0  # off by default; < 0 only asks
    assert switch(1) == 0 and switch(-1) == 1
    assert switch(0) == 1 and switch() == 0
    assert switch(7) == 0 and switch(-5) == 1  # (any on != 0 turns it on)


def test_known_answer():
    docs = pr.kat_corpus()
    ref = bp.Ref(5, docs)
    text = pr.Field(docs)
    st = pr.Stats.of(text, None, 5)
    got = {}
    for tag, q, want in KAT:
        s, d = ref.search(q, 10)
        assert set(d.tolist()) == want, (tag, d)
        assert len(set(d.tolist())) == len(d) and (np.diff(s) <= 0).all()
        got[tag] = dict(zip(d.tolist(), s.tolist()))

    def phrase(terms):
        s, d, _ = pr.search(text, None, st, terms, [0, 1], 4)
        return dict(zip(d.tolist(), s))

    cor = br.Corpus(5, np.cumsum([0] + [len(x) for x in docs]), np.concatenate(docs))
    term = lambda t: cor.clause(t, cor.own)[0]  # noqa: E731
    ab, aa, bc = phrase([0, 1]), phrase([0, 0]), phrase([1, 2])
    z = F(0.0)
    assert got["mp_sb"][1] == F((z + aa[1]) + (z + term(1)[1])) and got["mp_sb"][3] == F(z + aa[3])
    assert got["mp_sb"][1] > aa[1]  # (d1 carries the added Should score)
    assert got["sp_sc"][0] == F((z + ab[0]) + term(2)[0]) and got["sp_sc"][1] == F(z + ab[1])
    assert got["sp_sc"][2] == F(z + term(2)[2])
    assert got["mp_mc"][0] == F(z + (ab[0] + term(2)[0]))
    assert got["mp_xd"][0] == F(z + bc[0]) and got["sc_xp"][2] == F(z + term(2)[2])
    a, b, c = term(0)[0], term(1)[0], term(2)[0]
    assert got["mb_mp_mc"][0] == F(z + ((c + b) + (z + ab[0])))
    assert got["mp_mb_mc"][0] == F(z + ((c + ab[0]) + (z + b)))
    assert got["ma_mb_mp"][0] == F(z + ((bc[0] + a) + (z + b)))


def test_must_order_follows_the_segment_cost():
    """three Musts: (s0 + s1) + (0.0 + s2) in (cost, position) order, a phrase's cost the sum
    over the fields of its terms' smallest list there"""
    docs = pr.kat_corpus()
    ref = bp.Ref(5, docs)
    q = [bp.T(1, M), bp.P([0, 1], M), bp.T(2, M)]  # costs: b 3, "a b" min(3, 3) = 3, c 2 -> c, b, "a b"
    s, d = ref.search(q, 10)
    assert d.tolist() == [0]
    cl = [ref.clause(t, o, ref.pstats) for t, o, _ in q]
    assert [c[1](0, 4) for c in cl] == [3, 3, 2]
    assert s[0] == F(F(0.0) + ((cl[2][0][0] + cl[0][0][0]) + (F(0.0) + cl[1][0][0])))
    # inside docs [1, 4) the phrase's cost is min(a: d1 d3, b: d1 d2) = 2, b's 2, c's 1
    assert [c[1](1, 4) for c in cl] == [2, 2, 1]


@pytest.fixture(scope="module")
def gen():
    c = pr.Synth()
    ref = bp.of_synth(c)
    qs = bp.queries(c)
    hits = {k: [ref.hits(q)[0] for q in v] for k, v in qs.items()}
    return c, ref, qs, hits


def test_references_agree_on_the_statistics(gen):
    c, ref, _, _ = gen
    own, st = ref.corpus.own, ref.pstats
    assert (own.n_docs, tuple(own.tot_tokens)) == (st.n, st.tot)
    assert np.array_equal(own.df_text, st.df_text) and np.array_equal(own.df_name, st.df_name)


def test_generator_conditions(gen):
    c, ref, qs, hits = gen
    assert set(qs) == set(bp.KINDS)
    for kind, v in qs.items():
        assert len(v) >= 16, kind
        for q in v:
            assert sum(len(t) for t, _, _ in q) <= 16 and any(len(t) > 1 for t, _, _ in q) and len(q) >= 2
    frac = lambda xs: sum(bool(x) for x in xs) / len(xs)  # noqa: E731
    assert set(bp.KINDS) - set(bp.DECIDING) == {"mt_sp"}
    for kind in bp.KINDS:
        assert frac([len(h) > 0 for h in hits[kind]]) >= 0.75, kind
        differ = [set(h.tolist()) != set(ref.hits(q, as_conj=True)[0].tolist()) for q, h in zip(qs[kind], hits[kind])]
        print(kind, "hit", frac([len(h) > 0 for h in hits[kind]]), "differ", frac(differ))
        if kind in bp.DECIDING:
            assert frac(differ) >= 0.5, (kind, frac(differ))
        else:
            assert frac(differ) == 0.0, kind  # (mt_sp: the Should phrase cannot change the hit set)
    adds = [len(ref.hits([(q[0][0], q[0][1], M), (q[1][0], q[1][1], M)])[0]) > 0 for q in qs["mt_sp"]]
    assert frac(adds) >= 0.5
    assert all(max(q[0][0]) >= pr.V_TEXT for q in qs["name"])
    assert all(sum(len(t) for t, _, _ in q) == 16 for q in qs["t16"])
    for q in qs["repeat"]:
        (ph,), (tm,) = [t for t, _, _ in q if len(t) > 1], [t for t, _, _ in q if len(t) == 1]
        assert tm[0] in ph and ph.count(tm[0]) >= 2
    assert {tuple(oc for _, _, oc in q) for q in qs["repeat"]} == {(M, S), (M, M), (M, X), (S, S)}
    gone = lambda t: t == bp.MISSING or t >= pr.V  # noqa: E731
    must_gone = [any(oc == M and any(gone(t) for t in ts) for ts, _, oc in q) for q in qs["missing"]]
    assert all(any(gone(t) for ts, _, _ in q for t in ts) for q in qs["missing"])
    assert {oc for q in qs["missing"] for ts, _, oc in q if any(gone(t) for t in ts)} == {M, S, X}
    assert any(must_gone) and all(len(h) == 0 for h, g in zip(hits["missing"], must_gone) if g)


def test_long_lists_cross_a_full_item():
    """Synth(n=10000): term 0's merged list exceeds kPhraseMaxGroup * kChunk = 8192 postings"""
    c = pr.Synth(n=10000)
    ref = bp.of_synth(c)
    assert len(np.union1d(ref.corpus.docs(0, 0), ref.corpus.docs(0, 1))) > 8192
