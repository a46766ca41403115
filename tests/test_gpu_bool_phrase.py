"""Phrase clauses beside other clauses on the device (k_bphrase, DESIGN.md §14,
behind fg_phrase_clauses) against the numpy reference tests/bool_phrase_ref.py:
doc ids and order exact, scores within 1e-5 relative (the known-answer corpus bit
for bit).  Every test that sets the switch does so through the `switch` fixture
(`on`: it, turned on), which restores the setting it found in teardown: the
refusal tests of test_gpu_phrase.py run in the same process.

- the known-answer queries of test_bool_phrase_ref.py, those with three Musts
  (the planner's cost order shows in the sum's bits) among them;
- phrase_ref.Synth() (6000 docs, names, deletions, gaps) x 16 queries of each of
  bool_phrase_ref.KINDS at k = 1, 10, 1000; some of them as batches of one (their
  lead chunks spread over several items); Synth(n=10000) with lead and pass lists
  past kPhraseMaxGroup * kChunk = 8192 postings; an escaped tf byte (tf >= 255) in
  a term clause beside a phrase;
- the corpus as 3 segments under global statistics, the middle one rescored with
  changed deletions: fg_search_sharded, a multi-snapshot plan's slots and single
  plans merged on the host;
- a batch mixing them with plain AND / OR term queries and single-phrase queries;
- the switch itself, and fg_db through search and search_json.
test_bool_phrase_ref.py checks, without a GPU, that the queries decide something.
"""
import json

import numpy as np
import pytest

import bool_phrase_ref as bp
import phrase_ref as pr
from shard_ref import merge_topk_numpy

pytestmark = pytest.mark.gpu
RTOL = 1e-5
M, S, X = bp.MUST, bp.SHOULD, bp.MUST_NOT


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
def switch(native):
    """sets fg_phrase_clauses; the setting found is restored in teardown"""
    was = native.phrase_clauses()
    yield native.phrase_clauses
    native.phrase_clauses(was)


@pytest.fixture()
def on(switch):
    switch(1)


def check(s, d, n, want, k, tag="", bits=False):
    """device rows (s, d, n) against the reference lists `want` [(scores, docs)] cut at k"""
    for i, (rs, rd) in enumerate(want):
        rs, rd = rs[:k], rd[:k]
        m = int(n[i])
        assert m == len(rd), (tag, i, m, len(rd))
        assert np.array_equal(d[i, :m].astype(np.int64), rd.astype(np.int64)), (tag, i, d[i, :m], rd)
        if bits:
            assert s[i, :m].view(np.uint32).tolist() == rs.view(np.uint32).tolist(), (tag, i, s[i, :m], rs)
        else:
            assert np.allclose(s[i, :m], rs, rtol=RTOL, atol=0), (tag, i)


def run(ix, queries, k):
    q_off, terms, occur, plen, ppos = bp.batch(queries)
    return ix.search_batch(q_off, terms, k, occur=occur, phrase_len=plen, phrase_pos=ppos)


def build(native, ctx, c, lo=0, hi=None, **kw):
    to, tt, tg = c.csr(c.text, c.text_gaps, lo, hi)
    no, nt, ng = c.csr(c.name, c.name_gaps, lo, hi)
    return native.Index.from_docs(ctx, to, tt, pr.V, no, nt, positions=True, text_gaps=tg, name_gaps=ng, **kw)


# ------------------------------------------------------------------ known answer
def test_known_answer_bit_for_bit(native, ctx, on):
    from test_bool_phrase_ref import KAT
    docs = pr.kat_corpus()
    off = np.cumsum([0] + [len(x) for x in docs]).astype(np.uint64)
    ix = native.Index.from_docs(ctx, off, np.concatenate(docs).astype(np.uint32), 5, positions=True)
    ref = bp.Ref(5, docs)
    qs = [q for _, q, _ in KAT]
    s, d, n = run(ix, qs, 10)
    check(s, d, n, [ref.search(q, 10) for q in qs], 10, "kat", bits=True)
    assert [set(d[i, :int(n[i])].tolist()) for i in range(len(qs))] == [w for _, _, w in KAT]


# ------------------------------------------------------------------ 6000 docs
@pytest.fixture(scope="module")
def corpus(native, ctx):
    c = pr.Synth()
    ref = bp.of_synth(c)
    ix = build(native, ctx, c, deleted=c.deleted)
    kinds = bp.queries(c)
    qs = [q for kind in bp.KINDS for q in kinds[kind]]
    want = [ref.search(q, 1000) for q in qs]
    return c, ix, ref, qs, want


@pytest.mark.parametrize("k", [1, 10, 1000])
def test_corpus_matches_reference(native, corpus, on, k):
    c, ix, ref, qs, want = corpus
    assert len(qs) == 16 * len(bp.KINDS)
    s, d, n = run(ix, qs, k)
    check(s, d, n, want, k, f"k={k}")
    assert (n > 0).mean() >= 0.75


def test_batches_of_one_spread_the_lead_chunks(native, corpus, on):
    c, ix, ref, qs, want = corpus
    for i in range(0, len(qs), 16 * 2 + 1):  # a query of every other kind, alone: up to 64 items per pass
        s, d, n = run(ix, [qs[i]], 10)
        check(s, d, n, [want[i]], 10, f"alone {i}")


def test_lists_past_a_full_item(native, ctx, on):
    """lead (Must-driven) and pass (Should-driven) lists of > kPhraseMaxGroup * kChunk = 8192 postings"""
    c = pr.Synth(n=10000)
    ref = bp.of_synth(c)
    ix = build(native, ctx, c, deleted=c.deleted)
    assert ix.stats().n_docs == 10000
    r = np.random.default_rng(5)
    plain = [i for i in range(c.n) if not c.deleted[i] and c.text_gaps[i] is None and len(c.text[i]) >= 6]
    qs = []
    for i in range(32):
        t = c.text[plain[int(r.integers(0, len(plain)))]]
        a = int(r.integers(0, len(t) - 2))
        ph = [int(x) for x in t[a:a + 2]]
        if i % 2:
            qs.append([bp.T(0, S), bp.P(ph, S)])            # pass 0 sweeps term 0's list
        else:
            qs.append([bp.P([0, 0], M), bp.T(0, M if i % 4 else S), bp.P(ph, S)])  # every Must list is term 0's
    for k in (10, 1000):
        s, d, n = run(ix, qs, k)
        check(s, d, n, [ref.search(q, k) for q in qs], k, f"long k={k}")
    assert (n > 0).all()


def test_escaped_tf_in_a_term_clause_beside_a_phrase(native, ctx, on):
    docs = [[7] * 300 + [1, 2], [1, 2, 7], [7, 7, 1], [3, 4], [2, 1, 2] + [7] * 260]
    off = np.cumsum([0] + [len(x) for x in docs]).astype(np.uint64)
    ix = native.Index.from_docs(ctx, off, np.concatenate(docs).astype(np.uint32), 8, positions=True)
    ref = bp.Ref(8, docs)
    qs = [[bp.T(7, S), bp.P([1, 2], S)], [bp.T(7, M), bp.P([1, 2], M)], [bp.P([7, 7], M), bp.T(1, S)],
          [bp.P([1, 2], M), bp.T(7, S), bp.T(3, X)], [bp.P([2, 7], S), bp.T(7, S)]]
    s, d, n = run(ix, qs, 10)
    check(s, d, n, [ref.search(q, 10) for q in qs], 10, "escaped tf")
    assert n.tolist() == [4, 3, 3, 3, 4]


# ------------------------------------------------------------------ segments
@pytest.fixture(scope="module")
def segments(native, ctx, corpus):
    c, _, ref, qs, _ = corpus
    cuts = [0, 1700, 4300, c.n]
    g = None
    for lo, hi in zip(cuts, cuts[1:]):
        to, tt, _ = c.csr(c.text, c.text_gaps, lo, hi)
        no, nt, _ = c.csr(c.name, c.name_gaps, lo, hi)
        x = native.docs_stats(to, tt, pr.V, no, nt)
        g = x if g is None else g + x
    dele = c.deleted.copy()
    dele[cuts[1]:cuts[2]:7] = ~dele[cuts[1]:cuts[2]:7]  # the middle segment's deletions change after its build
    ixs = []
    for s_, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        if s_ == 1:  # built under its OWN statistics and the old deletions, then rescored: query-time statistics
            ixs.append(build(native, ctx, c, lo, hi, deleted=c.deleted[lo:hi]).rescore(g, deleted=dele[lo:hi]))
        else:
            ixs.append(build(native, ctx, c, lo, hi, deleted=dele[lo:hi], global_stats=g))
    want = [ref.search(q, 1000, seg_bounds=cuts, deleted=dele) for q in qs]
    return ixs, np.array(cuts[:-1], np.int64), want


@pytest.mark.parametrize("k", [10, 1000])
def test_segments_equal_the_reference(native, ctx, corpus, segments, on, k):
    qs = corpus[3]
    ixs, base, want = segments
    q_off, terms, occur, plen, ppos = bp.batch(qs)
    kw = dict(occur=occur, phrase_len=plen, phrase_pos=ppos)
    s, d, sh, n = native.search_sharded(ixs, q_off, terms, k, ctx=ctx, **kw)
    check(s, d.astype(np.int64) + base[sh], n, want, k, "sharded")
    if k != 10:  # (the host merges below are Python loops)
        return
    per = [ix.search_batch(q_off, terms, k, **kw) for ix in ixs]
    es, ed, esh, en = merge_topk_numpy(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]),
                                       np.stack([p[2] for p in per]), k)
    check(es, ed.astype(np.int64) + base[esh], en, want, k, "single plans")
    plan = native.Plan(ixs, q_off, terms, k, **kw)
    plan.execute()
    ps, pd, pn = plan.results()
    nq, S_ = len(q_off) - 1, len(ixs)
    es, ed, esh, en = merge_topk_numpy(ps.reshape(S_, nq, k), pd.reshape(S_, nq, k), pn.reshape(S_, nq), k)
    check(es, ed.astype(np.int64) + base[esh], en, want, k, "multi-snapshot plan")
    assert np.array_equal(np.minimum(pn.reshape(S_, nq).sum(0), k), n)


# ------------------------------------------------------------------ mixed batches
def test_batch_mixes_the_shapes(native, ctx, corpus, segments, switch):
    c, ix, ref, qs, want = corpus
    ixs, base, swant = segments
    r = np.random.default_rng(3)
    mixed, kind = [], []  # kind: the index in qs, or -1 (a plain row)
    for i in range(96):
        if i % 3 == 0:
            kind.append((i * 7) % len(qs))
            mixed.append(qs[kind[-1]])
            continue
        kind.append(-1)
        if i % 3 == 1:  # a single phrase
            t, o = c.queries[(i * 5) % 256]
            mixed.append([(list(t), list(o), M if i % 2 else S)])
        else:  # AND / OR term queries, some with an exclusion
            m = int(r.integers(1, 5))
            oc = [M if i % 2 else S] * m
            if m > 2 and i % 4 == 0:
                oc[-1] = X
            mixed.append([bp.T(int(r.integers(0, pr.V_TEXT)), o) for o in oc])
    plain = [q for q, kd in zip(mixed, kind) if kd < 0]
    rows = [i for i, kd in enumerate(kind) if kd < 0]
    new = [i for i, kd in enumerate(kind) if kd >= 0]
    k = 100

    def one(queries):
        return run(ix, queries, k)

    def sharded(queries):
        q_off, terms, occur, plen, ppos = bp.batch(queries)
        s, d, sh, n = native.search_sharded(ixs, q_off, terms, k, ctx=ctx, occur=occur, phrase_len=plen, phrase_pos=ppos)
        return s, d.astype(np.int64) + base[sh], n

    for tag, go, rf in (("one index", one, want), ("segments", sharded, swant)):
        assert switch(0) == 0  # (off by default, and after the first round)
        off = go(plain)
        with pytest.raises(native.Unsupported, match="phrase clause beside other clauses"):
            go(mixed)
        switch(1)
        alone, both = go(plain), go(mixed)
        switch(0)
        check(both[0][new], both[1][new], both[2][new], [rf[kind[i]] for i in new], k, tag)
        for a in (alone, off):  # the plain rows: byte-identical without the new queries, and with the switch off
            assert np.array_equal(both[2][rows], a[2])
            for j, i in enumerate(rows):  # (a row's first n entries: the rest is not written)
                m = int(a[2][j])
                assert np.array_equal(both[1][i, :m], a[1][j, :m]), (tag, i)
                assert np.array_equal(both[0][i, :m].view(np.uint32), a[0][j, :m].view(np.uint32)), (tag, i)
        assert (off[2] > 0).mean() > 0.5


# ------------------------------------------------------------------ the switch
def test_switch(native, ctx, corpus, switch):
    c, ix, ref, qs, want = corpus
    assert switch() == 0
    with pytest.raises(native.Unsupported, match="phrase clause beside other clauses"):
        run(ix, qs[:1], 10)
    assert switch(1) == 0 and switch(-1) == 1
    s, d, n = run(ix, qs[:4], 10)
    check(s, d, n, want[:4], 10, "on")
    to, tt, _ = c.csr(c.text, c.text_gaps, 0, 200)
    fo = np.arange(201, dtype=np.uint64)
    fx = native.Index.from_docs(ctx, to, tt, pr.V, positions=True, facets=(fo, np.zeros(200, np.uint32), 1))
    q_off, terms, occur, plen, ppos = bp.batch([[bp.P([0, 1], S), bp.T(2, S)]])
    kw = dict(occur=occur, phrase_len=plen, phrase_pos=ppos)
    with pytest.raises(native.Unsupported, match="phrase with facet filters"):
        fx.search_batch(q_off, terms, 10, f_off=[0, 1], f_terms=[0], **kw)
    assert int(fx.search_batch(q_off, terms, 10, **kw)[2][0]) > 0
    nopos = native.Index.from_docs(ctx, to, tt, pr.V)
    with pytest.raises(native.Unsupported, match="snapshot built without positions"):
        nopos.search_batch(q_off, terms, 10, **kw)
    with pytest.raises(native.Unsupported, match="snapshot built without positions"):
        native.search_sharded([fx, nopos], q_off, terms, 10, **kw)
    with pytest.raises(native.Unsupported, match="terms"):  # 17 terms: the existing check and message
        run(ix, [[bp.P(list(range(9)), S), bp.P(list(range(8)), S)]], 10)
    assert switch(0) == 1
    with pytest.raises(native.Unsupported, match="phrase clause beside other clauses"):
        run(ix, qs[:1], 10)


# ------------------------------------------------------------------ fg_db
DB_QUERIES = [("e-mail server", [(["e", "mail"], [0, 1], S), (["server"], [0], S)]),
              ("+e-mail -server", [(["e", "mail"], [0, 1], M), (["server"], [0], X)]),
              ('"new york" guide', [(["new", "york"], [0, 1], S), (["guide"], [0], S)]),
              ('+"e-mail server" alpha', [(["e", "mail", "server"], [0, 1, 2], M), (["alpha"], [0], S)])]


def db_reference(d, ns, docs):
    """the reference's hit lists [(score, global doc)] of DB_QUERIES over the namespace's current segments"""
    from test_gpu_phrase import py_tokens
    segs = d.segments(ns)
    keep = [g for seg in segs for g in seg]
    info = d.merge_info(ns)
    vocab = {}
    tt, tg, nt, ng = [], [], [], []
    for g in keep:
        for src, dst, dg in ((docs[g][1], tt, tg), (docs[g][2] or "", nt, ng)):
            toks, gaps = py_tokens(src)
            dst.append([vocab.setdefault(w, len(vocab)) for w in toks])
            dg.append(gaps or None)
    ref = bp.Ref(len(vocab), tt, tg, nt, ng)
    assert ref.pstats.n == info["n_docs_stats"]
    ref.pstats.tot = tuple(info["tot_tokens"])
    bounds = np.cumsum([0] + [len(s) for s in segs])
    out = []
    for _, cl in DB_QUERIES:
        q = [([vocab.get(w, bp.MISSING) for w in ws], o, oc) for ws, o, oc in cl]
        s, dd = ref.search(q, 20, seg_bounds=bounds)
        out.append([(float(x), keep[int(y)]) for x, y in zip(s, dd)])
    return out


def test_db_clauses_beside_phrases(native, ctx, switch):
    from fugu_amd import db
    from test_gpu_phrase import DOCS, same
    d = db.Database(ctx)
    ns = "bphr"
    d.create_namespace(ns)
    switch(1)
    for i, (rid, text, nm) in enumerate(DOCS):  # 9 commits, one segment each: the merger runs
        d.upsert(db.ObjectRecord(rid, text, metadata={"name": nm} if nm else None), ns)
        d.commit(ns)
        if i == 5:
            same([d.search(ns, q, per_page=20) for q, _ in DB_QUERIES], db_reference(d, ns, DOCS))
    d.merge_wait(ns)
    assert d.merge_info(ns)["merges"] >= 1
    got = [d.search(ns, q, per_page=20) for q, _ in DB_QUERIES]
    same(got, db_reference(d, ns, DOCS))
    docs_of = lambda r: [g for _, g in r]  # noqa: E731
    assert set(docs_of(got[0])) == {0, 6, 8} and set(docs_of(got[1])) == {6, 8}
    assert set(docs_of(got[2])) == {2, 6} and docs_of(got[3]) == [0]
    for q, r in zip(DB_QUERIES, got):
        js = json.loads(d.search_json(ns, q[0], per_page=20))
        assert [x["id"] for x in js["results"]] == [DOCS[g][0] for g in docs_of(r)]
        assert np.allclose([x["score"] for x in js["results"]], [x for x, _ in r], rtol=RTOL, atol=0)
    switch(0)
    with pytest.raises(native.Unsupported, match="phrase clause beside other clauses"):
        d.search(ns, "e-mail server")
