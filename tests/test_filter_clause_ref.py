"""Facet filters on phrase, phrase-beside and group queries without a GPU
(DESIGN.md §16): the switch, and -- in the reference's numbers alone -- that the
cases test_gpu_filter_clauses.py runs can catch each mistake a kernel could make.
These are conditions on the inputs (tests/filter_clause_ref.py), not on the code
under test.  Per kernel family, at least 8 cases each where
 (a) the filter removes a doc of the unfiltered top k (a kernel ignoring the
     filter fails),
 (b) the filtered top k differs from the filtered hits ordered by text score (a
     kernel forgetting the facet score fails),
 (c) at k = 1 and k = 10 there are more than k filtered hits and a doc of the
     filtered top k has a text-only score below the k-th filtered total (a bound
     without the facet part may drop it),
 (d) k_group: a chunk after the first of the 8193-posting lead list holds a doc
     of the filtered top 10 while the chunk's text-only bound is below the 10th
     filtered total (a chunk bound without f_max skips it),
 (e) k_phrase: one case whose lead list is longer than 4 x kChunk postings.
The facet score itself (bool_ref.Corpus._facet_union) is pinned to the C oracle
bit for bit on textless filtered queries of the same corpora.
"""
import numpy as np
import pytest

import filter_clause_ref as fc
import group_ref as gr
import phrase_ref as pr

F = np.float32
FAMILIES = {"phrase": fc.phrase_family, "bphrase": fc.bphrase_family, "group": fc.group_family}


@pytest.fixture()
def switch():
    """sets fg_filter_clauses; the setting found is restored in teardown"""
    from fugu_amd import native
    was = native.filter_clauses()
    yield native.filter_clauses
    native.filter_clauses(was)


def test_native_binds_the_switch(switch):
    from fugu_amd import native
    assert "fg_filter_clauses" in native.EXPORTS and switch == native.filter_clauses
    assert switch() == 0 and switch(-1) == 0  # off by default; < 0 only asks
    assert switch(1) == 0 and switch(-1) == 1
    assert switch(0) == 1 and switch() == 0
    assert switch(7) == 0 and switch(-5) == 1  # (any on != 0 turns it on)
    assert native.phrase_clauses() == 0 and native.group_clauses() == 0  # (switches of their own)
    assert native.ABI_VERSION == 6 and native.lib().fg_abi_version() == 6


def test_generator_holds_what_it_promises():
    for fam in (f() for f in FAMILIES.values()):
        off, tok, nf = fam.fac
        assert nf == fc.N_FTERMS and len(off) == fam.n + 1 and int(off[-1]) == len(tok)
        df = fam.facets.df
        assert df[fc.A] > fam.n // 2 and df[fc.RARE] == fc.N_RARE < 10 and df[fc.NODOC] == 0
        assert all(fc.N_RARE < df[t] < fam.n // 2 for t in (fc.AX, fc.AY, fc.B, fc.BZ, fc.E, fc.EW, fc.HOT, fc.SEG))
        per_doc = np.diff(off.astype(np.int64))
        assert (per_doc == 0).mean() > 0.05 and (per_doc >= 2).mean() > 0.2  # docs with none, docs with several
        has = np.zeros((fam.n, nf), bool)
        has[np.repeat(np.arange(fam.n), per_doc), tok] = True
        for child, parent in ((fc.AX, fc.A), (fc.AY, fc.A), (fc.BZ, fc.B), (fc.EW, fc.E)):  # ancestors included
            assert not (has[:, child] & ~has[:, parent]).any()
        assert (has[:, fc.B] & has[:, fc.A]).sum() > 100  # two facets of different branches
        seg_docs = np.flatnonzero(has[:, fc.SEG])
        assert seg_docs.min() >= fam.cuts[-2]  # present in the last segment only
        # every clause count, the all-missing lists, a missing term beside present ones, a shared list
        assert {len(f) for _, f in fam.cases} == set(fc.CLAUSE_COUNTS)
        lists = [tuple(f) for _, f in fam.cases]
        assert all(lists.count(tuple(f)) >= 2 for f in fc.ALL_MISSING)
        assert any(fc.MISSING in f and len(set(f) - {fc.MISSING, fc.NODOC}) for f in lists)
        assert (fc.A,) in lists and (fc.RARE,) in lists


@pytest.mark.parametrize("name", list(FAMILIES))
def test_cases_can_catch_each_mistake(name):
    fam = FAMILIES[name]()
    n = {key: 0 for key in ("a", "b", "c1", "c10", "zero")}
    for case in fam.cases:
        i, ft = case
        d, s = fam.hits[i]
        _, any_f = fam.facets.union(ft, fam.fst)
        ws, wd = fam.want(case, len(d) + 1)  # every filtered hit, ordered
        n["zero"] += len(wd) == 0
        text = np.full(fam.n, F(-1.0))
        text[d] = s
        top = d[np.lexsort((d, -s))[:10]]
        n["a"] += bool((~any_f[top]).any())
        dd, ss = d[any_f[d]], s[any_f[d]]
        n["b"] += dd[np.lexsort((dd, -ss))[:10]].tolist() != wd[:10].tolist()
        for k in (1, 10):
            n[f"c{k}"] += len(wd) > k and bool((text[wd[:k]] < ws[k - 1]).any())
    assert min(n["a"], n["b"], n["c1"], n["c10"]) >= 8, n
    assert n["zero"] <= 0.25 * len(fam.cases), n
    for f in fc.ALL_MISSING:  # the all-missing lists are meant to have no hits
        assert all(len(fam.want(c, 10)[1]) == 0 for c in fam.cases if c[1] == f)


def test_group_chunk_bound_needs_the_facet_part():
    """(d): the pass leads from T_LONG's 8193 postings alone; a chunk's text-only bound, as k_group forms it (the
    chunk's largest lead score plus T_EVERY's largest, inflated), restated over per-chunk maxima in numpy"""
    fam = fc.group_family()
    c = gr.synth()
    st = c.corpus.own
    qi = fam.queries.index(fc.LONG_LEAD_QUERY)
    s_long, s_every = c.corpus.clause(gr.T_LONG, st)[0], c.corpus.clause(gr.T_EVERY, st)[0]
    lead = np.flatnonzero(s_long >= 0)
    assert len(lead) == 8193
    found = []
    for case in fam.cases:
        if case[0] != qi:
            continue
        ws, wd = fam.want(case, 10)
        if len(wd) < 10:
            continue
        for ch in range(1, 5):
            docs = lead[ch * 2048:(ch + 1) * 2048]
            bound = F(F(s_long[docs].max() + s_every.max()) * F(1.00000762939453125))
            if bound < ws[9] and np.isin(wd, docs).any():
                found.append((case[1], ch))
    assert found, "no seed of the generator yields such a chunk"


def test_phrase_case_with_a_long_lead_list():
    """(e): the lead list (the phrase's distinct term with the fewest docs in either field) exceeds 4 x kChunk"""
    fam = fc.big_phrase_family()
    c = fam.synth
    lens = []
    for t in set(fc.BIG_QUERY[0]):
        lens.append(sum(1 for i in range(c.n) if (c.text[i] == t).any() or (c.name[i] == t).any()))
    assert min(lens) > 4 * 2048, lens
    assert len(fam.cases) >= 256  # so many queries: a query's items hold several chunks each
    d, s = fam.hits[0]
    text = np.full(fam.n, F(-1.0))
    text[d] = s
    lead = np.sort(d)  # (every hit holds the lead term; its position among the hits orders the chunks as the list's)
    for flt in fc.BIG_FILTERS:
        for k in (1, 10):
            ws, wd = fam.want((0, list(flt)), k + 1)
            assert len(wd) > k and (text[wd[:k]] < ws[k - 1]).any()  # (c) holds here too
        # the k-th filtered total lies above EVERY text-only score, and the top 10 is spread over the doc range
        ws, wd = fam.want((0, list(flt)), 10)
        assert ws[9] > s.max() and len(np.unique(np.searchsorted(lead, wd) * 10 // len(lead))) >= 4, flt


def oracle_union(n_terms, off, tok, deleted, fam, fterms, k):
    from oracle import oracle as orc
    ix = orc.OracleIndex(n_terms, off, tok, deleted=deleted, facet_off=fam.fac[0], facet_tok=fam.fac[1],
                         n_fterms=fam.fac[2])
    try:
        return [ix.search([], k, fterms=f) for f in fterms]
    finally:
        ix.close()


@pytest.mark.parametrize("name", ["phrase", "group"])
def test_facet_union_equals_the_oracle_bit_for_bit(name):
    """textless filtered queries: the facet union alone, (doc, score bits) of the top 1000"""
    fam = FAMILIES[name]()
    if name == "group":
        c = gr.synth()
        n_terms, off, tok, dele = gr.V, c.text_off, c.text_tok, c.deleted
    else:
        c = fc.phrase_synth()
        off, tok, _ = c.csr(c.text, c.text_gaps)
        n_terms, dele = pr.V, c.deleted.astype(np.uint8)
    lists = sorted({tuple(f) for _, f in fam.cases})
    alive = np.flatnonzero(np.asarray(dele) == 0)
    got = oracle_union(n_terms, off, tok, dele, fam, [list(f) for f in lists], 1000)
    for f, (os_, od) in zip(lists, got):
        fs, any_f = fam.facets.union(f, fam.fst)
        d = alive[any_f[alive]]
        o = np.lexsort((d, -fs[d]))[:1000]
        assert od.astype(np.int64).tolist() == d[o].tolist(), f
        assert os_.view(np.uint32).tolist() == fs[d[o]].view(np.uint32).tolist(), f
