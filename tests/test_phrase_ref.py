"""Phrase queries, the parts that need no GPU: the host parser's clauses, the
numpy reference (tests/phrase_ref.py) against a hand-derived known answer, and
the conditions the GPU tests' corpus must meet so they cannot pass vacuously.

Known answer (SURVEY Appendix A.4 arithmetic, f32).  Corpus: Appendix C's
d0 = `a b c`, d1 = `a a b`, d2 = `b c d e`, plus d3 = `a a a`; text only.
  N = 4, total tokens = 13, avgdl = 3.25
  df(a) = 3, df(b) = 3, df(c) = 2
  idf(df=3) = ln(1 + (4 - 3 + 0.5) / (3 + 0.5)) = ln(1.4285715) = 0.35667497
  idf(df=2) = ln(1 + 2.5 / 2.5) = ln 2 = 0.6931472
  cache[3] = 1.2 * (0.25 + 0.75 * 3 / 3.25) = 1.1307693
  cache[4] = 1.2 * (0.25 + 0.75 * 4 / 3.25) = 1.4076923
  "a b": weight = (0.35667497 + 0.35667497) * 2.2 = 1.5693699
         d0 (position 0) and d1 (position 1), count 1, length 3:
         1.5693699 * (1 / (1 + 1.1307693)) = 0.7365275 each -> [d0, d1] (doc ascending)
  "b c": weight = (0.35667497 + 0.6931472) * 2.2 = 2.3096089
         d0: 2.3096089 * (1 / 2.1307693) = 1.0839320
         d2: length 4, 2.3096089 * (1 / 2.4076923) = 0.9592625 -> [d0, d2]
  "a a": weight = 1.5693699; d3 `a a a` holds it twice (overlapping), d1 once:
         d3: 1.5693699 * (2 / (2 + 1.1307693)) = 1.0025460
         d1: 0.7365275 -> [d3, d1]
"""
import numpy as np
import pytest

import phrase_ref as pr

M, S, X = 0, 1, 2


@pytest.fixture(scope="module")
def db():
    from fugu_amd import db as d
    return d


# ------------------------------------------------------------------ parser
def test_parser_clauses(db):
    pc = db.parse_query_clauses
    assert pc("e-mail") == [(S, [("e", 0), ("mail", 1)])]
    assert pc("+foo-bar") == [(M, [("foo", 0), ("bar", 1)])]
    assert pc('"New York"') == [(S, [("new", 0), ("york", 1)])]
    assert pc('"rust"') == [(S, [("rust", 0)])]
    assert pc("user@example.com") == [(S, [("user", 0), ("example", 1), ("com", 2)])]
    assert pc('"alpha ' + "x" * 45 + ' beta"') == [(S, [("alpha", 0), ("beta", 2)])]
    assert pc("a b") == [(S, [("a", 0)]), (S, [("b", 0)])]
    assert pc("+a -b") == [(M, [("a", 0)]), (X, [("b", 0)])]
    assert pc("state-of-the-art") == [(S, [("state", 0), ("of", 1), ("the", 2), ("art", 3)])]
    assert pc("3.14 foo_bar") == [(S, [("3", 0), ("14", 1)]), (S, [("foo", 0), ("bar", 1)])]
    assert pc('-"a b" c') == [(X, [("a", 0), ("b", 1)]), (S, [("c", 0)])]
    assert pc("a AND b-c") == [(M, [("a", 0)]), (M, [("b", 0), ("c", 1)])]


@pytest.mark.parametrize("q", ['"a b"~2', '"a b"*', "--a", "a OR -b", '"a \\" b"', '"a b', 'x"a b"', '"a b"^2', '""',
                               '-"a b"'])
def test_parser_clauses_reject(db, q):
    from fugu_amd import native
    with pytest.raises(native.Unsupported):
        db.parse_query_clauses(q)


@pytest.mark.parametrize("q", ['"a b"', "foo-bar", "user@example.com"])
def test_term_parsers_still_refuse_phrases(db, q):
    from fugu_amd import native
    with pytest.raises(native.Unsupported):
        db.parse_query(q)
    with pytest.raises(native.Unsupported):
        db.parse_query_occur(q)


def test_abi_revision():
    from fugu_amd import native
    assert native.ABI_VERSION == 6 and native.lib().fg_abi_version() == 6
    assert [n for n, _ in native.QueryBatch._fields_][-2:] == ["phrase_len", "phrase_pos"]
    assert [n for n, _ in native.DocsInput._fields_][-5:] == ["keep_positions", "text_gap", "n_text_gap", "name_gap",
                                                             "n_name_gap"]


# ------------------------------------------------------------------ reference known answer
def kat():
    text = pr.Field(pr.kat_corpus())
    return text, pr.Stats.of(text, None, 5)


@pytest.mark.parametrize("terms,docs,counts,scores", [
    ([0, 1], [0, 1], [1, 1], [0.7365275, 0.7365275]),
    ([1, 2], [0, 2], [1, 1], [1.0839320, 0.9592625]),
    ([0, 0], [3, 1], [2, 1], [1.0025460, 0.7365275]),
])
def test_reference_known_answer(terms, docs, counts, scores):
    text, st = kat()
    assert (st.n, st.tot[0]) == (4, 13) and st.df_text[:3].tolist() == [3, 3, 2]
    s, d, (ct, _) = pr.search(text, None, st, terms, [0, 1], 10)
    assert d.tolist() == docs and ct[d].tolist() == counts
    assert s.dtype == np.float32 and np.allclose(s, scores, rtol=1e-6, atol=0)


def test_reference_gaps_and_deletes():
    # `alpha <dropped> beta` does not hold "alpha beta" but holds alpha@0 beta@2
    text = pr.Field([[0, 1], [0, 1], [1, 0]], [None, [1], None])
    st = pr.Stats.of(text, None, 2)
    assert text.len.tolist() == [2, 2, 2]  # gaps count nowhere
    assert pr.search(text, None, st, [0, 1], [0, 1], 10)[1].tolist() == [0]
    assert pr.search(text, None, st, [0, 1], [0, 2], 10)[1].tolist() == [1]
    assert pr.search(text, None, st, [0, 1], [0, 1], 10, deleted=[1, 0, 0])[1].tolist() == []
    # a phrase never spans two docs
    assert pr.search(text, None, st, [1, 0], [0, 1], 10)[1].tolist() == [2]


# ------------------------------------------------------------------ the GPU tests' corpus
def test_corpus_conditions():
    c = pr.Synth()
    assert c.n == 6000 and len(c.queries) == 256
    assert 200 < c.deleted.sum() < 400 and 60 < sum(g is not None for g in c.text_gaps) < 200
    assert sum(len(x) > 0 for x in c.name) == 2000
    text, name = pr.Field(c.text, c.text_gaps), pr.Field(c.name, c.name_gaps)
    st = pr.Stats.of(text, name, pr.V)
    hits, lead, name_only, kinds = [], [], 0, set()
    merged = np.maximum(st.df_text, 0) + 0
    for t in range(pr.V):  # merged (text U name) list lengths
        merged[t] = len(set(text.owner[text.flat == t]) | set(name.owner[name.flat == t]))
    for terms, offs in c.queries:
        _, d, (ct, cn) = pr.search(text, name, st, terms, offs, 6000, deleted=c.deleted)
        hits.append(len(d))
        known = [t for t in terms if t < pr.V]
        lead.append(min(merged[t] for t in known) if len(known) == len(terms) else 0)
        name_only += int(len(d) > 0 and not (ct[d] > 0).any())
        kinds.add((len(set(terms)) < len(terms), offs != list(range(len(offs))), len(known) < len(terms)))
    hits = np.array(hits)
    assert (hits[:192] >= 1).all()  # the spans cut from alive docs
    assert (hits > 0).mean() >= 0.75
    assert (hits > 10).sum() >= 32
    assert (hits > 1000).sum() >= 4
    assert max(l for l, h in zip(lead, hits) if h > 0) > 4096  # a lead list of more than 2 * kChunk postings
    assert name_only >= 4
    assert {(True, False, False), (False, True, False), (False, False, True)} <= kinds
    assert all(2 <= len(t) <= 5 for t, _ in c.queries)
