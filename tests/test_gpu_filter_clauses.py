"""Facet filters on phrase, phrase-beside and group queries on the device
(k_phrase, k_bphrase, k_group behind fg_filter_clauses) against
the numpy reference tests/filter_clause_ref.py: doc ids and order exact, scores
within 1e-5 relative (the known-answer corpus bit for bit).  Every test that
turns a switch on does so through the `on` / `switches` fixtures, which restore
the settings they found in teardown.

- the known-answer corpus with a facet on some docs;
- per family, every query with filters of 1, 2, 3, 5 and 8 clauses (the dense
  term alone, the rare term alone, missing terms beside present ones, only
  missing terms, lists shared by several queries) at k = 1, 10, 1000;
- a ~20,000-doc corpus whose phrase leads from more than 8192 postings;
- the corpora as 3 segments under global statistics, the middle one built under
  its own and rescored with changed deletions, the last one alone holding SEG:
  single-snapshot plans merged, a multi-snapshot plan, fg_search_sharded;
- plans executed in parts (fg_plan_execute_part), one snapshot and two;
- one batch mixing the shapes; empty and partly missing filters; the switch off
  (the three refusals, word for word) and on without filters (byte-equal);
- fg_db_search and the JSON handler with filters.
test_filter_clause_ref.py checks, without a GPU, that these cases can catch a
kernel that ignores the filter, forgets the facet score, or bounds without it.
"""
import json

import numpy as np
import pytest

import bool_phrase_ref as bpr
import filter_clause_ref as fc
import group_ref as gr
import phrase_ref as pr
from shard_ref import merge_topk_numpy

pytestmark = pytest.mark.gpu
RTOL = 1e-5
FAMILIES = ("phrase", "bphrase", "group")
F = np.float32


@pytest.fixture(scope="module")
def native():
    from fugu_amd import native as nat
    if nat.device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    return nat


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context((0,))


@pytest.fixture()
def switches(native):
    """(phrase_clauses, group_clauses, filter_clauses); the settings found are restored in teardown"""
    fns = (native.phrase_clauses, native.group_clauses, native.filter_clauses)
    was = [f() for f in fns]
    yield fns
    for f, w in zip(fns, was):
        f(w)


@pytest.fixture()
def on(switches):
    for f in switches:
        f(1)


def check(s, d, n, want, k, tag=""):
    """device rows (s, d, n) against the reference lists `want` [(scores, docs)] cut at k"""
    for i, (rs, rd) in enumerate(want):
        rs, rd = rs[:k], rd[:k]
        m = int(n[i])
        assert m == len(rd), (tag, i, m, len(rd))
        assert np.array_equal(np.asarray(d[i, :m], np.int64), np.asarray(rd, np.int64)), (tag, i)
        assert np.allclose(s[i, :m], rs, rtol=RTOL, atol=0), (tag, i)


def batch_of(name, queries, flists):
    """the keyword arguments of search_batch / Plan / search_sharded after k, and (q_off, terms)"""
    if name == "phrase":
        q_off, terms, plen, ppos = fc.phrase_synth().batch(queries)
        kw = dict(phrase_len=plen, phrase_pos=ppos)
    else:
        q_off, terms, occur, plen, ppos = (bpr if name == "bphrase" else gr).batch(queries)
        kw = dict(occur=occur, phrase_len=plen, phrase_pos=ppos)
    if flists is not None:
        kw["f_off"], kw["f_terms"] = fc.filter_arrays(flists)
    return q_off, terms, kw


def case_batch(name, fam, cases=None):
    cases = fam.cases if cases is None else cases
    return batch_of(name, [fam.queries[i] for i, _ in cases], [f for _, f in cases])


# ------------------------------------------------------------------ known answer
def test_known_answer_bit_for_bit(native, ctx, on):
    docs = pr.kat_corpus()
    off = np.cumsum([0] + [len(x) for x in docs]).astype(np.uint64)
    tok = np.concatenate(docs).astype(np.uint32)
    fac = (np.array([0, 1, 3, 3, 4], np.uint64), np.array([0, 0, 1, 1], np.uint32), 2)  # facet ids per doc: 0: [0]; 1: [0, 1]; 2: none; 3: [1]
    ix = native.Index.from_docs(ctx, off, tok, 5, positions=True, facets=fac)
    text = pr.Field(docs)
    st = pr.Stats.of(text, None, 5)
    facets = fc.Facets(4, fac)
    fst = facets.stats()
    qs = [[0, 1], [1, 2], [0, 0]]
    seen = 0
    for flt in ([0], [1], [0, 1], [1, fc.MISSING, 0]):
        s, d, n = ix.search_batch([0, 2, 4, 6], [t for q in qs for t in q], 10, phrase_len=[2, 0] * 3,
                                  phrase_pos=[0, 1] * 3, f_off=np.arange(4) * len(flt), f_terms=flt * 3)
        for i, q in enumerate(qs):
            rs, rd, _ = pr.search(text, None, st, q, [0, 1], 10)
            ws, wd = facets.filtered((rd, rs), flt, fst, 10)
            m = int(n[i])
            assert d[i, :m].tolist() == wd.tolist(), (flt, q, d[i, :m], wd)
            assert s[i, :m].view(np.uint32).tolist() == ws.view(np.uint32).tolist(), (flt, q, s[i, :m], ws)
            seen += m
    assert seen >= 10  # [0, 1] hits docs 0 and 1, [1, 2] doc 0 (doc 2 has no facet), [0, 0] docs 1 and 3


# ------------------------------------------------------------------ single snapshots
@pytest.fixture(scope="module")
def world(native, ctx):
    """per family: (Family, index, the reference's top 1000 of every case) -- computed once, shared, never changed"""
    c = fc.phrase_synth()
    to, tt, tg = c.csr(c.text, c.text_gaps)
    no, nt, ng = c.csr(c.name, c.name_gaps)
    pf = fc.phrase_family()
    ix_p = native.Index.from_docs(ctx, to, tt, pr.V, no, nt, deleted=c.deleted, positions=True, text_gaps=tg,
                                  name_gaps=ng, facets=pf.fac)
    g = gr.synth()
    gf = fc.group_family()
    ix_g = native.Index.from_docs(ctx, g.text_off, g.text_tok, gr.V, g.name_off, g.name_tok, deleted=g.deleted,
                                  facets=gf.fac)
    out = {}
    for name, fam, ix in (("phrase", pf, ix_p), ("bphrase", fc.bphrase_family(), ix_p), ("group", gf, ix_g)):
        out[name] = (fam, ix, [fam.want(case, 1000) for case in fam.cases])
    return out


@pytest.mark.parametrize("k", [1, 10, 1000])
@pytest.mark.parametrize("name", FAMILIES)
def test_cases_match_reference(native, world, on, name, k):
    fam, ix, want = world[name]
    q_off, terms, kw = case_batch(name, fam)
    s, d, n = ix.search_batch(q_off, terms, k, **kw)
    check(s, d, n, want, k, f"{name} k={k}")
    assert (n > 0).mean() >= 0.75


def test_long_lead_list_shares_a_threshold(native, ctx, on):
    """(e): the phrase's lead list spans several work items of several chunks each, which prune on one
    threshold word: a bound without the facet part drops the later chunks' top-k docs"""
    fam = fc.big_phrase_family()
    c = fam.synth
    to, tt, tg = c.csr(c.text, c.text_gaps)
    no, nt, ng = c.csr(c.name, c.name_gaps)
    ix = native.Index.from_docs(ctx, to, tt, pr.V, no, nt, deleted=c.deleted, positions=True, text_gaps=tg,
                                name_gaps=ng, facets=fam.fac)
    q_off, terms, plen, ppos = c.batch([fam.queries[i] for i, _ in fam.cases])
    f_off, f_terms = fc.filter_arrays([f for _, f in fam.cases])
    assert len(fam.cases) >= 256
    want = {tuple(f): fam.want((0, list(f)), 10) for f in fc.BIG_FILTERS}  # computed once per distinct filter
    for k in (1, 10):
        s, d, n = ix.search_batch(q_off, terms, k, phrase_len=plen, phrase_pos=ppos, f_off=f_off, f_terms=f_terms)
        check(s, d, n, [want[tuple(f)] for _, f in fam.cases], k, f"long lead k={k}")
        assert (n == k).all()


# ------------------------------------------------------------------ segments
def build_segments(native, ctx, name, fam, dele):
    """3 snapshots under global statistics (facet ones included); the middle one built under its OWN
    statistics and the old deletions, then rescored: query-time scores"""
    cuts = list(fam.cuts)
    parts, g = [], None
    for lo, hi in zip(cuts, cuts[1:]):
        if name == "group":
            c = gr.synth()
            to, tt, no, nt = c.segment(lo, hi)
            kw = {}
            old = c.deleted[lo:hi]
        else:
            c = fc.phrase_synth()
            to, tt, tg = c.csr(c.text, c.text_gaps, lo, hi)
            no, nt, ng = c.csr(c.name, c.name_gaps, lo, hi)
            kw = dict(positions=True, text_gaps=tg, name_gaps=ng)
            old = c.deleted[lo:hi]
        kw["facets"] = fc.segment(fam.fac, lo, hi)
        parts.append(((to, tt, (gr.V if name == "group" else pr.V), no, nt), kw, old))
        x = native.docs_stats(to, tt, parts[-1][0][2], no, nt, facets=kw["facets"])
        g = x if g is None else g + x
    assert np.array_equal(np.asarray(g.df_facet, np.int64), fam.facets.df) and g.tot_facet_tokens == fam.facets.tot
    ixs = []
    for s_, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        args, kw, old = parts[s_]
        if s_ == 1:
            own = native.Index.from_docs(ctx, *args, deleted=old, **kw)
            ixs.append(own.rescore(g, deleted=dele[lo:hi]))
        else:
            ixs.append(native.Index.from_docs(ctx, *args, deleted=dele[lo:hi], global_stats=g, **kw))
    return ixs, np.array(cuts[:-1], np.int64)


@pytest.mark.parametrize("name", FAMILIES)
def test_segments_equal_the_reference(native, ctx, on, name):
    fam = {"phrase": fc.phrase_family, "bphrase": fc.bphrase_family, "group": fc.group_family}[name]()
    cuts = list(fam.cuts)
    if name == "group":
        c = gr.synth()
        dele = c.deleted.copy()
        dele[cuts[1]:cuts[2]:7] ^= 1  # the middle segment's deletions change after its build
        ref = gr.Ref(c.corpus)
        hits = [ref.hits(q, seg_bounds=cuts, deleted=dele) for q in fam.queries]
    else:
        c = fc.phrase_synth()
        dele = c.deleted.copy()
        dele[cuts[1]:cuts[2]:7] = ~dele[cuts[1]:cuts[2]:7]
        if name == "phrase":
            hits = fc.phrase_hits(c, fam.queries, deleted=dele)
        else:
            ref = bpr.of_synth(c)
            hits = [ref.hits(q, seg_bounds=cuts, deleted=dele) for q in fam.queries]
    ixs, base = build_segments(native, ctx, name, fam, dele)
    cases = fam.cases[::3] + [c_ for c_ in fam.cases if fc.SEG in c_[1]][:40]  # a third, and SEG's: two segments lack it
    want = [fam.want(case, 1000, hits=hits) for case in cases]
    q_off, terms, kw = case_batch(name, fam, cases)
    for k in (10, 1000):
        s, d, sh, n = native.search_sharded(ixs, q_off, terms, k, ctx=ctx, **kw)
        check(s, d.astype(np.int64) + base[sh], n, want, k, f"{name} sharded k={k}")
    k = 10  # (the host merge is a Python loop)
    per = [ix.search_batch(q_off, terms, k, **kw) for ix in ixs]
    es, ed, esh, en = merge_topk_numpy(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]),
                                       np.stack([p[2] for p in per]), k)
    check(es, ed.astype(np.int64) + base[esh], en, want, k, f"{name} single plans")
    seg_only = [i for i, c_ in enumerate(cases) if c_[1] == [fc.SEG]]
    assert seg_only and not per[0][2][seg_only].any() and not per[1][2][seg_only].any() and per[2][2][seg_only].any()
    plan = native.Plan(ixs, q_off, terms, k, **kw)
    plan.execute()
    ps, pd, pn = plan.results()
    nq, S = len(q_off) - 1, len(ixs)
    es, ed, esh, en = merge_topk_numpy(ps.reshape(S, nq, k), pd.reshape(S, nq, k), pn.reshape(S, nq), k)
    check(es, ed.astype(np.int64) + base[esh], en, want, k, f"{name} multi-snapshot plan")


@pytest.mark.parametrize("name", FAMILIES)
def test_plan_executed_in_parts(native, world, on, name):
    """fg_plan_execute_part: the first part builds the masks, the last runs the filtered kernels; one snapshot,
    and the same snapshot twice as a multi-snapshot plan (every slot carries its own q_filter)"""
    fam, ix, want = world[name]
    cases = fam.cases[:120]
    q_off, terms, kw = case_batch(name, fam, cases)
    k = 10
    for target in (ix, [ix, ix]):
        plan = native.Plan(target, q_off, terms, k, **kw)
        plan.execute()
        whole = plan.results()
        plan.execute_part(None, 0.0, 0.5)
        plan.execute_part(None, 0.5, 1.0)
        parts = plan.results()
        if target is ix:
            assert np.array_equal(whole[2], parts[2])
            for i in range(len(cases)):  # (a row's first n entries: the rest is not written)
                m = int(whole[2][i])
                assert np.array_equal(whole[1][i, :m], parts[1][i, :m]), i
                assert np.array_equal(whole[0][i, :m].view(np.uint32), parts[0][i, :m].view(np.uint32)), i
            check(*parts, want[:len(cases)], k, f"{name} in parts")
            continue
        # (a query's slots share its threshold, so a slot may keep fewer than k: the merge is what is defined)
        nq = len(cases)
        for tag, (ps, pd, pn) in (("whole", whole), ("parts", parts)):
            es, ed, esh, en = merge_topk_numpy(ps.reshape(2, nq, k), pd.reshape(2, nq, k), pn.reshape(2, nq), k)
            for i, (rs, rd) in enumerate(want[:nq]):
                both = sorted((-float(s), sh, int(d)) for sh in (0, 1) for s, d in zip(rs[:k], rd[:k]))[:k]
                m = int(en[i])
                assert m == len(both), (name, tag, i)
                assert [(int(sh), int(d)) for sh, d in zip(esh[i, :m], ed[i, :m])] == [(sh, d) for _, sh, d in both], (tag, i)
                assert np.allclose(es[i, :m], [-s for s, _, _ in both], rtol=RTOL, atol=0), (name, tag, i)


# ------------------------------------------------------------------ one mixed batch
def test_batch_mixes_the_shapes(native, world, on):
    """a filtered phrase, an unfiltered phrase, a filtered term AND, a textless filtered query, an AllQuery
    and two filtered group queries sharing one mask, on the phrase corpus"""
    fam, ix, _ = world["phrase"]
    c = fc.phrase_synth()
    bref = bpr.of_synth(c)
    gref = gr.Ref(bref.corpus)
    M, S = gr.MUST, gr.SHOULD
    alive = np.flatnonzero(~c.deleted)
    phrase = fam.queries[0]
    flt = [fc.A, fc.HOT, fc.B]
    groups = [[gr.G(M, gr.ANY, [5, 9]), gr.T(M, 2)], [gr.G(S, gr.ALL, [3, 7]), gr.T(S, 41)]]
    # (terms, occur, phrase_len, phrase_pos, filter)
    rows = [(phrase[0], [M] * len(phrase[0]), [len(phrase[0])] + [0] * (len(phrase[0]) - 1), phrase[1], flt),
            (phrase[0], [M] * len(phrase[0]), [len(phrase[0])] + [0] * (len(phrase[0]) - 1), phrase[1], []),
            ([4, 11], [M, M], [1, 1], [0, 0], flt),
            ([], [], [], [], flt),
            ([], [], [], [], [])]
    for q in groups:
        _, t, oc, pl, pp = gr.batch([q])
        rows.append((t.tolist(), oc.tolist(), pl.tolist(), pp.tolist(), [fc.AX, fc.E]))
    q_off = np.cumsum([0] + [len(r[0]) for r in rows]).astype(np.uint32)
    cat = lambda j, t: np.array([x for r in rows for x in r[j]], t)  # noqa: E731
    f_off, f_terms = fc.filter_arrays([r[4] for r in rows])
    k = 50
    s, d, n = ix.search_batch(q_off, cat(0, np.uint32), k, occur=cat(1, np.uint8), phrase_len=cat(2, np.uint32),
                              phrase_pos=cat(3, np.uint32), f_off=f_off, f_terms=f_terms)
    dele = c.deleted
    fs, any_f = fam.facets.union(flt, fam.fst)
    td, ts = bref.corpus._hits([4, 11], [M, M], None, None, None)
    td, ts = td[~dele[td]], ts[~dele[td]]  # (both indexed by the unfiltered td: the right side is evaluated first)
    fd = alive[any_f[alive]]
    want = [fam.facets.filtered(fam.hits[0], flt, fam.fst, k),
            fam.facets.filtered(fam.hits[0], None, fam.fst, k),
            fam.facets.filtered((td, ts), flt, fam.fst, k),
            fam.facets.filtered((fd, np.zeros(len(fd), F)), flt, fam.fst, k),  # the union alone: 0.0 + fs
            (np.ones(min(k, len(alive)), F), alive[:k])]
    want += [fam.facets.filtered(gref.hits(q, deleted=dele), [fc.AX, fc.E], fam.fst, k) for q in groups]
    check(s, d, n, want, k, "mixed")
    assert all(int(x) > 0 for x in n)


# ------------------------------------------------------------------ empty and partly missing filters
@pytest.mark.parametrize("name", FAMILIES)
def test_empty_and_partly_missing_filters(native, world, on, name):
    fam, ix, _ = world[name]
    qs = fam.queries[:24]
    k = 100
    rows = {}
    for tag, flt in (("gone", [fc.MISSING, fc.MISSING]), ("nodoc", [fc.NODOC]), ("part", [fc.MISSING, fc.B, fc.NODOC, fc.E]),
                     ("present", [fc.B, fc.E])):
        q_off, terms, kw = batch_of(name, qs, [flt] * len(qs))
        rows[tag] = ix.search_batch(q_off, terms, k, **kw)
    assert not rows["gone"][2].any() and not rows["nodoc"][2].any()
    check(*rows["part"], [fam.facets.filtered(fam.hits[i], [fc.B, fc.E], fam.fst, k) for i in range(len(qs))], k, "part")
    assert rows["part"][2].sum() > 0 and np.array_equal(rows["part"][2], rows["present"][2])
    for i in range(len(qs)):  # a missing clause adds nothing: the present ones' union, bit for bit
        m = int(rows["part"][2][i])
        assert np.array_equal(rows["part"][1][i, :m], rows["present"][1][i, :m])
        assert np.array_equal(rows["part"][0][i, :m].view(np.uint32), rows["present"][0][i, :m].view(np.uint32))


# ------------------------------------------------------------------ the switch
def test_switch_off_keeps_the_refusals(native, world, switches):
    phrase_on, group_on, filter_on = switches
    assert filter_on() == 0  # off by default
    phrase_on(1)
    group_on(1)
    for name, text in (("phrase", "query 0: phrase with facet filters"), ("bphrase", "query 0: phrase with facet filters"),
                       ("group", "query 0: group with facet filters")):
        fam, ix, _ = world[name]
        q_off, terms, kw = batch_of(name, fam.queries[:1], [[fc.A]])
        with pytest.raises(native.Unsupported) as e:
            ix.search_batch(q_off, terms, 10, **kw)
        assert str(e.value).endswith(text), str(e.value)
        with pytest.raises(native.Unsupported, match=text[9:]):
            native.Plan([ix, ix], q_off, terms, 10, **kw)
    assert filter_on(1) == 0 and filter_on(-1) == 1
    fam, ix, _ = world["phrase"]
    q_off, terms, kw = batch_of("phrase", fam.queries[:1], [[fc.A]])
    assert int(ix.search_batch(q_off, terms, 10, **kw)[2][0]) > 0
    # fg_count_batch keeps refusing phrase clauses, filters or not
    with pytest.raises(native.Unsupported, match="phrase clause in a count query"):
        native.count_batch([ix], q_off, terms, **kw)
    assert filter_on(0) == 1
    with pytest.raises(native.Unsupported, match="phrase with facet filters"):
        ix.search_batch(q_off, terms, 10, **kw)


@pytest.mark.parametrize("name", FAMILIES)
def test_switch_on_without_filters_changes_nothing(native, world, switches, name):
    phrase_on, group_on, filter_on = switches
    phrase_on(1)
    group_on(1)
    fam, ix, _ = world[name]
    k = 100
    q_off, terms, kw = batch_of(name, fam.queries, None)
    assert filter_on(0) == 0
    off = ix.search_batch(q_off, terms, k, **kw)
    filter_on(1)
    on_ = ix.search_batch(q_off, terms, k, **kw)
    kw["f_off"], kw["f_terms"] = fc.filter_arrays([[]] * len(fam.queries))  # f_off given, every list empty
    empty = ix.search_batch(q_off, terms, k, **kw)
    for got in (on_, empty):
        assert np.array_equal(got[2], off[2])
        for i in range(len(fam.queries)):  # (a row's first n entries: the rest is not written)
            m = int(off[2][i])
            assert np.array_equal(got[1][i, :m], off[1][i, :m]), i
            assert np.array_equal(got[0][i, :m].view(np.uint32), off[0][i, :m].view(np.uint32)), i
    check(*off, [fam.facets.filtered(h, None, fam.fst, k) for h in fam.hits], k, f"{name} unfiltered")


# ------------------------------------------------------------------ fg_db
DB_DOCS = [
    ("d0", "send me an e-mail about the e-mail server", ["/topic/x"]),
    ("d1", "mail e then nothing", ["/topic/x"]),
    ("d2", "an e-mail once", ["/topic/y", "/kind/a"]),
    ("d3", "e mail e mail e mail", None),
    ("d4", "the e-mail of the day", ["/topic/x/deep", "/kind/a"]),
    ("d5", "nothing here", ["/topic/x"]),
    ("d6", "one more e-mail server and an e-mail", ["/kind/a"]),
    ("d7", "last e-mail", ["/topic/y"]),
]


def test_db_search_and_json_with_filters(native, ctx, switches):
    """The text side is phrase_ref's; the facet side of a doc is its score in the TEXTLESS filtered search
    of the same filters (k_scan, pinned to the oracle by test_host.py): score = f32(text + facet)."""
    from fugu_amd import db
    phrase_on, group_on, filter_on = switches
    d = db.Database(ctx)
    ns = "flt"
    d.create_namespace(ns)
    for i, (rid, text, fl) in enumerate(DB_DOCS):
        d.upsert(db.ObjectRecord(rid, text, facets=fl), ns)
        if i in (2, 5, 7):  # three commits: three segments (until the merger joins them)
            d.commit(ns)
    d.merge_wait(ns)
    vocab = {}
    toks = [[vocab.setdefault(w, len(vocab)) for w in text.replace("-", " ").split()] for _, text, _ in DB_DOCS]
    text = pr.Field(toks)
    st = pr.Stats.of(text, None, len(vocab))
    info = d.merge_info(ns)
    assert st.n == info["n_docs_stats"]
    st.tot = tuple(info["tot_tokens"])
    rs, rd, _ = pr.search(text, None, st, [vocab["e"], vocab["mail"]], [0, 1], 20)
    assert set(rd.tolist()) == {0, 2, 3, 4, 6, 7}
    assert filter_on() == 0
    for filters, docs in ((["/topic/x"], {0, 4}), (["/kind/a", "/topic/y"], {2, 4, 6, 7}), (["/topic/*"], {0, 2, 4, 7}),
                          (["/nope"], set())):
        filter_on(0)
        with pytest.raises(native.Unsupported, match="phrase with facet filters"):
            d.search(ns, "e-mail", filters=filters)
        with pytest.raises(native.Unsupported):
            d.search_json(ns, "e-mail", filters=filters, shape=db.SHAPE_POST_SEARCH)
        facet = {g: F(s) for s, g in d.search(ns, "", per_page=20, filters=filters)}  # the union alone
        filter_on(1)
        got = d.search(ns, "e-mail", per_page=20, filters=filters)
        want = sorted(((F(F(s) + facet[int(g)]), int(g)) for s, g in zip(rs, rd) if int(g) in facet),
                      key=lambda x: (-x[0], x[1]))
        assert {g for _, g in got} == docs == {g for _, g in want}, (filters, got)
        assert [g for _, g in got] == [g for _, g in want], (filters, got, want)
        assert [F(s).view(np.uint32) for s, _ in got] == [s.view(np.uint32) for s, _ in want], (filters, got, want)
        js = json.loads(d.search_json(ns, "e-mail", per_page=20, filters=filters, shape=db.SHAPE_POST_SEARCH))
        assert [x["id"] for x in js["results"]] == [DB_DOCS[g][0] for _, g in got]
        assert np.allclose([x["score"] for x in js["results"]], [s for s, _ in got], rtol=1e-6, atol=0)
    # a phrase beside a term, and a group, with filters: the other two switches decide as before
    with pytest.raises(native.Unsupported, match="phrase clause beside other clauses"):
        d.search(ns, "e-mail server", filters=["/topic/x"])
    phrase_on(1)
    assert {g for _, g in d.search(ns, "+e-mail +server", filters=["/topic/x"])} == {0}
    assert {g for _, g in d.search(ns, "+e-mail +server", filters=["/kind/a", "/topic/x"])} == {0, 6}
    with pytest.raises(native.Unsupported):
        d.search(ns, "(server OR day) AND mail", filters=["/kind/a"])
    group_on(1)
    assert {g for _, g in d.search(ns, "(server OR day) AND mail", filters=["/kind/a"])} == {4, 6}
    filter_on(0)
    with pytest.raises(native.Unsupported, match="group with facet filters"):
        d.search(ns, "(server OR day) AND mail", filters=["/kind/a"])
    d.close()
