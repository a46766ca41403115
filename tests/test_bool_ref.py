"""bool_ref (the vectorised brute-force reference) against the committed fixtures
and against the C oracle on the 6-16 clause edges corpus of clause_edges.py;
and that corpus's claims about itself.  Bit-exact: doc ids and f32 score bits.
"""
import numpy as np
import pytest

import bool_ref as br
import clause_edges as ce
from conftest import golden_corpus, golden_facets, load_golden

OCC = {"must": br.MUST, "should": br.SHOULD, "must_not": br.MUST_NOT}
FACET_QUERIES = ("should16", "must16", "must4_not2_should10")


def test_occur_fixture():
    fx = load_golden("occur_2k.json")
    n, nt, off, tok, no, ntk, dl = golden_corpus(fx, use_c_synth=False)
    c = br.Corpus(nt, off, tok, no, ntk, dl)
    bad = [q for q in fx["queries"]
           if br.hits_of(*c.search(q["terms"], [OCC[o] for o in q["occur"]], q["k"])) != q["hits"]]
    assert not bad, bad[:3]
    assert sum(len(q["hits"]) for q in fx["queries"]) > 2000


def test_names_fixture():
    fx = load_golden("synth_names_2k.json")
    n, nt, off, tok, no, ntk, dl = golden_corpus(fx, use_c_synth=False)
    c = br.Corpus(nt, off, tok, no, ntk, dl)
    for q in fx["queries"]:
        o = [br.MUST if q["mode"] == "and" else br.SHOULD] * len(q["terms"])
        assert br.hits_of(*c.search(q["terms"], o, q["k"])) == q["hits"], q


def test_facets_fixture():
    fx = load_golden("facets_2k.json")
    n, nt, off, tok, no, ntk, dl = golden_corpus(fx, use_c_synth=False)
    c = br.Corpus(nt, off, tok, no, ntk, dl, golden_facets(fx))
    assert c.own.tot_facet_tokens == sum(len(t) for t in fx["facet_tokens"])
    for q in fx["queries"]:
        o = [br.MUST if q["mode"] == "and" else br.SHOULD] * len(q["terms"])
        assert br.hits_of(*c.search(q["terms"], o, q["k"], q["fterms"])) == q["hits"], (q["terms"], q["fterms"])


@pytest.fixture(scope="module")
def case():
    return ce.edges_case()


@pytest.fixture(scope="module")
def oracle(case):
    from oracle import oracle as orc
    assert (orc.MUST, orc.SHOULD, orc.MUST_NOT) == (br.MUST, br.SHOULD, br.MUST_NOT)
    c = case
    ix = orc.OracleIndex(c["V"], c["off"], c["tok"], c["name_off"], c["name_tok"], c["deleted"], threads=8,
                         facet_off=c["facets"][0], facet_tok=c["facets"][1], n_fterms=c["facets"][2])
    yield ix
    ix.close()


def same(ref_hits, s, d, k, what):
    rs, rd = ref_hits
    assert len(d) == min(k, len(rd)), what
    assert np.array_equal(d.astype(np.int64), rd[:k]), what
    assert np.array_equal(s.view(np.uint32), rs[:k].view(np.uint32)), what


def test_classes(case):
    """The hand-made terms are in the density classes the docstring derives."""
    c = case
    ref, n = c["ref"], c["N"]
    for j, t in enumerate(c["H"]):
        df = int(ref.own.df_text[t])
        assert df == len(c["hand"][j][0]) and ref.own.df_name[t] == 0
        assert np.isin(ce.E, ref.docs(t)).all()
        if j < 4:
            assert n // 5 <= df <= n // 2 + 10
        elif j < 8:
            assert n // 200 <= df <= n // 100 + 10
        elif j < 12:
            assert 25 <= df <= 70 and ce.dir_shift(df, n) <= 12
            assert j == 11 or len(np.unique(ref.docs(t) >> 12)) <= 6  # (of 13 tiles: most are empty)
        else:
            assert 12 <= df <= 24 and ce.dir_shift(df, n) >= 13
    assert ce.dir_shift(24, n) == 13 and ce.dir_shift(25, n) == 12
    assert (n - 1) % 32 != 0 and n - ((n - 1) >> 12 << 12) == 848  # the last rank word and the last tile are partial
    esc = ref.fld[0]
    d, tf = ref._list(esc, c["T"]["esc"])
    assert sorted(d[tf >= 255].tolist()) == [4095, 4096] and (tf[tf < 255] == 1).all() and 90 <= len(d) <= 110
    dn = ref.docs(c["T"]["name"], 1)
    assert 0 < len(dn) and abs(3 * len(dn) - len(ref.docs(c["T"]["name"]))) <= 3
    assert [len(x) for x in c["fdocs"]] == [8191, 8192, 8193] and all(x[-1] == n - 1 for x in c["fdocs"])
    assert [int(np.isin(ce.E, x).sum()) for x in c["fdocs"]] == [10, 10, 6]
    assert ref.own.df_facet.tolist() == [8191, 8192, 8193]
    assert c["deleted"][8191] == 1 and c["deleted"][[e for e in ce.E if e != 8191]].sum() == 0
    assert 0.1 < c["deleted"].mean() < 0.2


def test_claims(case):
    """The queries are what they claim to be (from the reference alone)."""
    c = case
    ref, Q, qs, occ = c["ref"], c["Q"], c["qs"], c["occ"]
    alive_e = sorted(e for e in ce.E if e != 8191)
    run = lambda name, k, r=ref: r.search(qs[Q[name]], occ[Q[name]], k)  # noqa: E731
    # all-Should: the edge docs lead.  Nine of the ten are alive, so the top 10 are those nine and one more
    # doc; without the deletion doc 8191 is in the top 10, which then holds edge docs only
    s, d = run("should16", 1000)
    assert sorted(d[:9].tolist()) == alive_e and len(d) == 1000
    assert s[999] < s[8] and d[999] not in ce.E
    s0, d0 = run("should16", 10, c["ref_nodel"])
    assert sorted(d0.tolist()) == sorted(ce.E)
    assert sorted(run("should16_rev", 10)[1][:9].tolist()) == alive_e
    assert sorted(run("must16", 1000)[1].tolist()) == alive_e
    for child, parent in (("should15_not1", "should15"), ("should8_not8", "should8")):
        a, b = run(child, 10)[1], run(parent, 10)[1]
        assert len(a) == len(b) == 10 and a.tolist() != b.tolist(), child
        assert 0 in b and 0 not in a  # (doc 0 is in the excluded dense term)
    # Must-driven queries with hits whose Should part matches only on some
    s, d = run("must4_not2_should10", 1000)
    assert 100 < len(d) < 1000 and 0 not in d and np.isin(alive_e, d).any()
    nd = len(ref.search(qs[Q["must4_not2_should10"]][:4], [br.MUST] * 4, 1000)[1])
    assert len(d) < nd - 100  # (the MustNots remove many)
    assert len(run("must12_should4", 10)[1]) == 9
    # the fill: every clause count 6..16 occurs, and each third has hits
    hits = [len(ref.search(qs[i], occ[i], 10)[1]) for i in range(len(Q), 64)]
    third = len(hits) // 3
    assert all(h == 10 for h in hits[:len(hits) - 2 * third])
    assert sum(h > 0 for h in hits[-2 * third:-third]) >= third // 2 and sum(h > 0 for h in hits[-third:]) >= third // 2


def test_edges_vs_oracle(case, oracle):
    """bool_ref == the C oracle, bit for bit, on the whole batch: plain and segmented."""
    c = case
    ref = c["ref"]
    for sb in (None, ce.SEG_BOUNDS):
        for i in range(64):
            want = ref.search(c["qs"][i], c["occ"][i], max(ce.KS), seg_bounds=sb)
            for k in ce.KS:
                s, d = oracle.search(c["qs"][i], k, occur=c["occ"][i], seg_bounds=sb)
                same(want, s, d, k, (i, k, sb is not None))


def test_edges_facets_vs_oracle(case, oracle):
    c = case
    ref, Q = c["ref"], c["Q"]
    texts = [(c["qs"][Q[n]], c["occ"][Q[n]]) for n in FACET_QUERIES] + [([], [])]
    for fterms in ([0], [1], [2], [2, br.MISSING], [0, 2], []):
        for terms, occ in texts:
            if not terms and not fterms:
                continue  # (AllQuery: below)
            for sb in (None, ce.SEG_BOUNDS):
                want = ref.search(terms, occ, max(ce.KS), fterms, seg_bounds=sb)
                for k in ce.KS:
                    s, d = oracle.search(terms, k, fterms=fterms if fterms else None, occur=occ, seg_bounds=sb)
                    same(want, s, d, k, (terms[:2], fterms, k, sb is not None))
    want = ref.search([], [], 1024, [])
    s, d = oracle.search([], 1024, fterms=[])
    same(want, s, d, 1024, "AllQuery")
    assert (s == 1.0).all() and d.tolist() == np.flatnonzero(c["deleted"] == 0)[:1024].tolist()


def test_wide_case():
    """The second corpus (test_gpu_clause_edges.py's widest work items): its classes at
    140,000 docs, and its hand-made terms span all 35 tiles of the first segment only."""
    w = ce.wide_case()
    ref, n0 = w["ref"], ce.N_WIDE0
    assert ce.dir_shift(68, n0) == 13 and ce.dir_shift(69, n0) == 12
    assert ((n0 - 1) >> 12) + 1 == 35 and n0 - (34 << 12) == 736
    for j, t in enumerate(w["H"]):
        d = ref.docs(t)
        df = len(d)
        assert d[0] == 0 and d[-1] == n0 - 1 and np.isin(ce.E_WIDE, d).all()
        if 8 <= j < 12:
            assert ce.dir_shift(df, n0) <= 12
        elif j >= 12:
            assert ce.dir_shift(df, n0) >= 13
    assert sorted({len(q) for q in w["qs"]}) == [2, 8, 9, 16] and len(w["qs"]) == 256
