"""Group clauses on the device (k_group, DESIGN.md §15, behind fg_group_clauses)
against the numpy reference tests/group_ref.py on (doc, score bits), every query
compared.  Every test that sets the switch does so through the `switch` fixture
(`on`: it, turned on), which restores the setting it found in teardown.

- group_ref.synth() (12,000 docs, 64 terms, names, deletions, lead lists of 2047 /
  2048 / 2049 / 8193 postings, a term in 40 docs, an absent term) x 12 queries of
  each of group_ref.KINDS at k = 1, 10, 100, 1000: the small k make thresholds
  rise inside an item, so the chunk bound fires; the `tie` kind holds queries
  whose k-th and (k+1)-th hits tie on score;
- the corpus as three segments of unequal size (one lacks T_FEW, two lack T_LOW):
  fg_search_sharded and a multi-snapshot plan's slots merged on the host;
- a rescored snapshot: changed statistics and deletions, bounds scaled by q_rup;
- fg_db_search and the JSON handler over a small committed namespace;
- a batch mixing them with plain AND / OR / single-term queries;
- the refusals, and the switch itself.
test_group_ref.py checks, without a GPU, that the queries decide something.
"""
import json

import numpy as np
import pytest

import bool_ref as br
import group_ref as gr
from shard_ref import merge_topk_numpy

pytestmark = pytest.mark.gpu
M, S, X = gr.MUST, gr.SHOULD, gr.MUST_NOT
ANY, ALL = gr.ANY, gr.ALL


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
    """sets fg_group_clauses; the setting found is restored in teardown"""
    was = native.group_clauses()
    yield native.group_clauses
    native.group_clauses(was)


@pytest.fixture()
def on(switch):
    switch(1)


def check(s, d, n, want, k, tag=""):
    """device rows (s, d, n) against the reference lists `want` [(scores, docs)] cut at k: (doc, score bits)"""
    for i, (rs, rd) in enumerate(want):
        m = int(n[i])
        got, ref = gr.hits_of(s[i, :m], d[i, :m]), gr.hits_of(rs[:k], rd[:k])
        assert got == ref, (tag, i, m, len(ref), [x for x in zip(got, ref) if x[0] != x[1]][:3])


def run(ix, queries, k):
    q_off, terms, occur, plen, ppos = gr.batch(queries)
    return ix.search_batch(q_off, terms, k, occur=occur, phrase_len=plen, phrase_pos=ppos)


@pytest.fixture(scope="module")
def corpus(native, ctx):
    c = gr.synth()
    ref = gr.Ref(c.corpus)
    ix = native.Index.from_docs(ctx, c.text_off, c.text_tok, gr.V, c.name_off, c.name_tok, deleted=c.deleted)
    kinds = gr.queries()
    qs = [q for kind in gr.KINDS for q in kinds[kind]]
    want = [ref.search(q, 1000) for q in qs]  # computed once, shared, never changed
    return c, ix, ref, qs, want


# ------------------------------------------------------------------ every query, every k
@pytest.mark.parametrize("k", gr.KS)
def test_corpus_matches_reference(native, corpus, on, k):
    c, ix, ref, qs, want = corpus
    assert len(qs) == gr.PER_KIND * len(gr.KINDS) >= 144
    s, d, n = run(ix, qs, k)
    check(s, d, n, want, k, f"k={k}")
    assert (n > 0).mean() >= 0.9
    if k in (10, 100):  # a query whose k-th and (k+1)-th hits tie on score is among them
        assert any(len(rs) > k and rs[k - 1] == rs[k] for rs, _ in want)


def test_batches_of_one_spread_the_lead_chunks(native, corpus, on):
    c, ix, ref, qs, want = corpus
    for i in range(0, len(qs), gr.PER_KIND + 1):  # a query of every kind, alone: up to 64 items per pass
        s, d, n = run(ix, [qs[i]], 10)
        check(s, d, n, [want[i]], 10, f"alone {i}")


# ------------------------------------------------------------------ segments, rescored snapshots
@pytest.fixture(scope="module")
def segments(native, ctx, corpus):
    c, _, ref, qs, want = corpus
    cuts = list(gr.SEG_CUTS)
    g = None
    for lo, hi in zip(cuts, cuts[1:]):
        x = native.docs_stats(*c.segment(lo, hi)[:2], gr.V, *c.segment(lo, hi)[2:])
        g = x if g is None else g + x
    ixs = []
    for lo, hi in zip(cuts, cuts[1:]):
        to, tt, no, nt = c.segment(lo, hi)
        ixs.append(native.Index.from_docs(ctx, to, tt, gr.V, no, nt, deleted=c.deleted[lo:hi], global_stats=g))
    swant = [ref.search(q, 1000, seg_bounds=cuts) for q in qs]
    return ixs, np.array(cuts[:-1], np.int64), swant


@pytest.mark.parametrize("k", [10, 1000])
def test_segments_equal_the_reference(native, ctx, corpus, segments, on, k):
    c, _, ref, qs, want = corpus
    ixs, base, swant = segments
    # the segments order their Musts by their own costs: some sums differ from the one-snapshot ones
    q_off, terms, occur, plen, ppos = gr.batch(qs)
    kw = dict(occur=occur, phrase_len=plen, phrase_pos=ppos)
    s, d, sh, n = native.search_sharded(ixs, q_off, terms, k, ctx=ctx, **kw)
    check(s, d.astype(np.int64) + base[sh], n, swant, k, "sharded")
    if k != 10:  # (the host merge below is a Python loop)
        return
    plan = native.Plan(ixs, q_off, terms, k, **kw)
    plan.execute()
    ps, pd, pn = plan.results()
    nq, S_ = len(q_off) - 1, len(ixs)
    es, ed, esh, en = merge_topk_numpy(ps.reshape(S_, nq, k), pd.reshape(S_, nq, k), pn.reshape(S_, nq), k)
    check(es, ed.astype(np.int64) + base[esh], en, swant, k, "multi-snapshot plan")


@pytest.mark.parametrize("k", [10, 1000])
def test_rescored_snapshot(native, ctx, corpus, on, k):
    """statistics changed after the build: query-time scores, the chunk and term bounds scaled by q_rup"""
    c, ix, ref, qs, _ = corpus
    r = np.random.default_rng(9)
    own = native.docs_stats(c.text_off, c.text_tok, gr.V, c.name_off, c.name_tok)
    other = native.ShardStats(7000, (90000, 5000), r.integers(0, 3000, gr.V).astype(np.uint32),
                              r.integers(0, 900, gr.V).astype(np.uint32))
    g = own + other
    dele = c.deleted.copy()
    dele[::11] ^= 1
    rx = ix.rescore(g, deleted=dele)
    st = br.Stats(int(g.n_docs), tuple(int(x) for x in g.tot_tokens), np.asarray(g.df_text, np.int64),
                  np.asarray(g.df_name, np.int64))
    s, d, n = run(rx, qs, k)
    check(s, d, n, [ref.search(q, k, stats=st, deleted=dele) for q in qs], k, f"rescored k={k}")


# ------------------------------------------------------------------ mixed batches
def test_batch_mixes_the_shapes(native, ctx, corpus, switch):
    c, ix, ref, qs, want = corpus
    r = np.random.default_rng(3)
    mixed, kind = [], []  # kind: the index in qs, or -1 (a plain row)
    for i in range(96):
        if i % 3 == 0:
            kind.append((i * 7) % len(qs))
            mixed.append(qs[kind[-1]])
            continue
        kind.append(-1)
        m = 1 if i % 9 == 1 else int(r.integers(2, 5))  # single-term, AND and OR queries, some with an exclusion
        oc = [M if i % 2 else S] * m
        if m > 2 and i % 4 == 0:
            oc[-1] = X
        mixed.append([gr.T(o, int(r.integers(0, 48))) for o in oc])
    plain = [q for q, kd in zip(mixed, kind) if kd < 0]
    rows = [i for i, kd in enumerate(kind) if kd < 0]
    new = [i for i, kd in enumerate(kind) if kd >= 0]
    k = 100

    def plain_only(queries):  # without phrase_len: the call of before
        q_off, terms, occur, _, _ = gr.batch(queries)
        return ix.search_batch(q_off, terms, k, occur=occur)

    assert switch(0) == 0
    off = plain_only(plain)
    with pytest.raises(native.FuguError, match="bad phrase_len"):
        run(ix, mixed, k)
    switch(1)
    alone, both = run(ix, plain, k), run(ix, mixed, k)
    switch(0)
    check(both[0][new], both[1][new], both[2][new], [want[kind[i]] for i in new], k, "mixed")
    for a in (alone, off):  # the plain rows: byte-identical without the group queries, and with the switch off
        assert np.array_equal(both[2][rows], a[2])
        for j, i in enumerate(rows):  # (a row's first n entries: the rest is not written)
            m = int(a[2][j])
            assert np.array_equal(both[1][i, :m], a[1][j, :m]), i
            assert np.array_equal(both[0][i, :m].view(np.uint32), a[0][j, :m].view(np.uint32)), i
    # the plain rows against the reference too
    for j, q in enumerate(plain):
        rs, rd = ref.search(q, k)
        assert gr.hits_of(off[0][j, :int(off[2][j])], off[1][j, :int(off[2][j])]) == gr.hits_of(rs, rd), j
    assert (off[2] > 0).mean() > 0.5


# ------------------------------------------------------------------ the switch and the refusals
def test_switch_and_refusals(native, ctx, corpus, switch):
    c, ix, ref, qs, want = corpus
    assert switch() == 0
    for q in (qs[0], [gr.G(S, ALL, [6, 7])], [gr.G(M, ANY, [6, 7]), gr.T(M, 8)]):
        with pytest.raises(native.FuguError, match="bad phrase_len at term 0") as e:  # today's answer, FG_EINVAL
            run(ix, [q], 10)
        assert e.value.code == native.FG_EINVAL and not isinstance(e.value, native.Unsupported)
    assert switch(1) == 0 and switch(-1) == 1
    s, d, n = run(ix, qs[:4], 10)
    check(s, d, n, want[:4], 10, "on")
    bad = lambda plen, terms=(6, 7, 8): ix.search_batch(  # noqa: E731
        [0, len(terms)], list(terms), 10, occur=[S] * len(terms), phrase_len=plen, phrase_pos=[0] * len(terms))
    for plen in ([3 | native.CLAUSE_ANY | native.CLAUSE_ALL, 0, 0], [1 | native.CLAUSE_ANY, 1, 1],
                 [4 | native.CLAUSE_ALL, 0, 0], [2 | native.CLAUSE_ANY, 1, 1][:2] + [0]):
        with pytest.raises(native.FuguError, match="phrase_len"):
            bad(plen)
    with pytest.raises(native.FuguError, match="group member's offset must be 0"):
        ix.search_batch([0, 2], [6, 7], 10, occur=[S, S], phrase_len=[2 | native.CLAUSE_ANY, 0], phrase_pos=[0, 1])
    q_off, terms, occur, plen, ppos = gr.batch([[gr.G(S, ANY, [6, 7]), gr.T(S, 8)]])
    kw = dict(occur=occur, phrase_len=plen, phrase_pos=ppos)
    with pytest.raises(native.Unsupported, match="group clause beside a phrase clause"):
        ix.search_batch([0, 4], [6, 7, 8, 9], 10, occur=[S] * 4, phrase_len=[2 | native.CLAUSE_ANY, 0, 2, 0],
                        phrase_pos=[0, 0, 0, 1])
    fo = np.arange(201, dtype=np.uint64)
    to, tt, no, nt = c.segment(0, 200)
    fx = native.Index.from_docs(ctx, to, tt, gr.V, facets=(fo, np.zeros(200, np.uint32), 1))
    with pytest.raises(native.Unsupported, match="group with facet filters"):
        fx.search_batch(q_off, terms, 10, f_off=[0, 1], f_terms=[0], **kw)
    assert int(fx.search_batch(q_off, terms, 10, **kw)[2][0]) > 0
    with pytest.raises(native.Unsupported, match="group clause in a count query"):
        native.count_batch([ix], q_off, terms, **kw)
    with pytest.raises(native.Unsupported, match="does not cover group clauses"):
        ix.model(q_off, terms, 10, phrase_len=plen, phrase_pos=ppos)
    with pytest.raises(native.Unsupported, match="terms"):  # 17 terms: the existing check and message
        run(ix, [[gr.G(S, ANY, list(range(6, 15))), gr.G(S, ALL, list(range(15, 23)))]], 10)
    assert switch(0) == 1
    with pytest.raises(native.Unsupported, match="phrase clause in a count query"):  # today's answers again
        native.count_batch([ix], q_off, terms, **kw)
    with pytest.raises(native.FuguError, match="does not cover phrase queries"):
        ix.model(q_off, terms, 10, phrase_len=plen, phrase_pos=ppos)
    with pytest.raises(native.FuguError, match="bad phrase_len"):
        run(ix, qs[:1], 10)


# ------------------------------------------------------------------ fg_db
DB_DOCS = [
    ("d0", "a b c", None), ("d1", "a c c d", "b"), ("d2", "b d", None), ("d3", "a a b", "c a"),
    ("d4", "c d e", None), ("d5", "b c e e", None), ("d6", "a d", "c"), ("d7", "e f", None),
    ("d8", "a b c d e f", "a b"), ("d9", "c", None), ("d10", "b b a f", None), ("d11", "a c", "d"),
    ("d12", "a f e", None),
]
DB_QUERIES = [  # (query, its clauses as group_ref's, over words)
    ("(a OR b) AND c", [(M, (ANY, ["a", "b"])), (M, "c")]),
    ("+(a b) +c", [(M, (ANY, ["a", "b"])), (M, "c")]),
    ("a AND b OR c", [(S, (ALL, ["a", "b"])), (S, "c")]),
    ("a -(b c)", [(S, "a"), (X, (ANY, ["b", "c"]))]),
]


def db_reference(d, ns):
    """the reference's hit lists [(score, global doc)] of DB_QUERIES over the namespace's current segments"""
    segs = d.segments(ns)
    keep = [g for seg in segs for g in seg]
    info = d.merge_info(ns)
    vocab = {}
    ids = lambda text: [vocab.setdefault(w, len(vocab)) for w in (text or "").split()]  # noqa: E731
    tt, nt = [ids(DB_DOCS[g][1]) for g in keep], [ids(DB_DOCS[g][2]) for g in keep]
    csr = lambda rows: (np.cumsum([0] + [len(x) for x in rows]).astype(np.uint64),  # noqa: E731
                        np.array([t for x in rows for t in x], np.uint32))
    cor = br.Corpus(len(vocab), *csr(tt), *csr(nt))
    assert cor.own.n_docs == info["n_docs_stats"]
    st = br.Stats(cor.own.n_docs, tuple(info["tot_tokens"]), cor.own.df_text, cor.own.df_name)  # the namespace's totals
    ref = gr.Ref(cor)
    bounds = np.cumsum([0] + [len(s) for s in segs])
    out = []
    for _, q in DB_QUERIES:
        q = [(oc, (b[0], [vocab.get(w, gr.MISSING) for w in b[1]]) if gr.is_group(b) else vocab.get(b, gr.MISSING))
             for oc, b in q]
        s, dd = ref.search(q, 20, seg_bounds=bounds, stats=st)
        out.append([(np.float32(x), keep[int(y)]) for x, y in zip(s, dd)])
    return out


def test_db_search_and_json(native, ctx, switch):
    from fugu_amd import db
    d = db.Database(ctx)
    ns = "grp"
    d.create_namespace(ns)
    for i, (rid, text, nm) in enumerate(DB_DOCS):
        d.upsert(db.ObjectRecord(rid, text, metadata={"name": nm} if nm else None), ns)
        if i in (3, 7, 12):  # three commits: three segments (until the merger joins them)
            d.commit(ns)
    d.merge_wait(ns)
    assert switch() == 0
    for q, _ in DB_QUERIES:  # refused with the switch off
        with pytest.raises(native.Unsupported, match="query outside the device subset"):
            d.search(ns, q)
        with pytest.raises(native.Unsupported):
            d.search_json(ns, q)
    switch(1)
    got = [d.search(ns, q, per_page=20) for q, _ in DB_QUERIES]
    want = db_reference(d, ns)
    for q, g, w in zip(DB_QUERIES, got, want):
        assert [x for _, x in g] == [x for _, x in w], (q[0], g, w)
        assert [np.float32(s).view(np.uint32) for s, _ in g] == [s.view(np.uint32) for s, _ in w], (q[0], g, w)
    docs_of = lambda r: {g for _, g in r}  # noqa: E731
    assert docs_of(got[0]) == docs_of(got[1]) == {0, 1, 3, 5, 6, 8, 11}  # (a or b, text or name) and c
    assert docs_of(got[2]) == {0, 1, 3, 4, 5, 6, 8, 9, 10, 11} and docs_of(got[3]) == {12}
    for (q, _), r in zip(DB_QUERIES, got):
        js = json.loads(d.search_json(ns, q, per_page=20))
        assert [x["id"] for x in js["results"]] == [DB_DOCS[g][0] for _, g in r]
        assert np.allclose([x["score"] for x in js["results"]], [x for x, _ in r], rtol=1e-6, atol=0)
    with pytest.raises(native.Unsupported, match="group clause in a count query"):
        d.facet_counts(ns, "/", "(a b) c")
    switch(0)
    with pytest.raises(native.Unsupported, match="query outside the device subset"):  # the same process, off again
        d.search(ns, "(a OR b) AND c")
