"""Phrases as group members on the device (k_mgroup, DESIGN.md §19, behind
fg_group_member_phrases with fg_group_clauses) against the numpy reference
tests/member_group_ref.py on (doc, score bits), every query compared.  Every test
sets the switches through the `switches` fixture, which restores what it found.

- corpus A and corpus B (group_phrase_ref's worlds) x every query of every kind of
  member_group_ref.KINDS at k = 1, 10, 100, 1000; batches of one;
- corpus A as three unequal segments, the first lacking terms of the queries:
  fg_search_sharded and a multi-snapshot plan's slots merged on the host;
- a rescored snapshot: changed statistics and deletions;
- one batch of a plain AND, a plain OR, a single phrase, a phrase beside a term, a
  group query, a group beside a phrase, a facet-only query (k_scan) and the new shape
  with every switch on, each row against its own reference;
- fg_db_search and the JSON handler over a small committed namespace;
- a 16-row query runs, a 17-row query is refused;
- the switch and the refusals: off, the ABI answers FG_EINVAL "a group member's
  offset must be 0" as before (the test that fails without the feature).
test_member_group_ref.py checks, without a GPU, that the queries decide something.
"""
import json

import numpy as np
import pytest

import bool_ref as br
import member_group_ref as mg
import phrase_ref as pr
from shard_ref import merge_topk_numpy

pytestmark = pytest.mark.gpu
M, S, X = mg.M, mg.S, mg.X
ANY, ALL = mg.ANY, mg.ALL


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
    """(group_clauses, group_member_phrases, group_phrase_clauses, phrase_clauses, filter_clauses); restored after"""
    fns = (native.group_clauses, native.group_member_phrases, native.group_phrase_clauses, native.phrase_clauses,
           native.filter_clauses)
    was = [f() for f in fns]
    yield fns
    for f, w in zip(fns, was):
        f(w)


@pytest.fixture()
def on(switches):
    switches[0](1)
    switches[1](1)


def check(s, d, n, want, k, tag=""):
    """device rows (s, d, n) against the reference lists `want` [(scores, docs)] cut at k: (doc, score bits)"""
    for i, (rs, rd) in enumerate(want):
        m = int(n[i])
        got, ref = mg.hits_of(s[i, :m], d[i, :m]), mg.hits_of(rs[:k], rd[:k])
        assert got == ref, (tag, i, m, len(ref), [x for x in zip(got, ref) if x[0] != x[1]][:3])


def run(ix, queries, k):
    q_off, terms, occur, plen, ppos = mg.batch(queries)
    return ix.search_batch(q_off, terms, k, occur=occur, phrase_len=plen, phrase_pos=ppos)


def build(native, ctx, w, lo=0, hi=None, deleted=None, **kw):
    args, gaps = w.csr(lo, hi)
    dele = w.deleted[lo:hi] if deleted is None else deleted
    return native.Index.from_docs(ctx, *args, positions=True, deleted=dele.astype(np.uint8), **gaps, **kw)


@pytest.fixture(scope="module", params=["A", "B"])
def corpus(request, native, ctx):
    w = mg.world(request.param)
    ix = build(native, ctx, w)
    qs = mg.all_queries(w.name)
    ref = mg.ref_of(w.name)
    want = [ref.search(q, 1000) for q in qs]  # computed once, shared, never changed
    return w, ix, qs, want


# ------------------------------------------------------------------ every query, every k
@pytest.mark.parametrize("k", mg.KS)
def test_corpus_matches_reference(native, corpus, on, k):
    w, ix, qs, want = corpus
    assert len(qs) == mg.PER_KIND * len(mg.kinds_of(w.name)) >= 15 * 8
    s, d, n = run(ix, qs, k)
    check(s, d, n, want, k, f"{w.name} k={k}")
    assert (n > 0).mean() >= 0.9


def test_batches_of_one_spread_the_lead_chunks(native, corpus, on):
    w, ix, qs, want = corpus
    for i in range(0, len(qs), mg.PER_KIND + 1):  # a query of every kind, alone: up to 64 items per pass
        s, d, n = run(ix, [qs[i]], 10)
        check(s, d, n, [want[i]], 10, f"{w.name} alone {i}")


# ------------------------------------------------------------------ segments, rescored snapshots
@pytest.mark.parametrize("k", [10, 1000])
def test_segments_equal_the_reference(native, ctx, on, k):
    w = mg.world("A")
    qs = mg.all_queries("A")
    ref = mg.ref_of("A")
    cuts = list(w.cuts)
    g = None
    for lo, hi in zip(cuts, cuts[1:]):
        x = native.docs_stats(*w.csr(lo, hi)[0])
        g = x if g is None else g + x
    ixs = [build(native, ctx, w, lo, hi, global_stats=g) for lo, hi in zip(cuts, cuts[1:])]
    base = np.array(cuts[:-1], np.int64)
    swant = [ref.search(q, k, seg_bounds=cuts) for q in qs]
    q_off, terms, occur, plen, ppos = mg.batch(qs)
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
    w, ix, qs, _ = corpus
    r = np.random.default_rng(9)
    own = native.docs_stats(*w.csr()[0])
    other = native.ShardStats(7000, (90000, 5000), r.integers(0, 3000, w.V).astype(np.uint32),
                              r.integers(0, 900, w.V).astype(np.uint32))
    g = own + other
    dele = w.deleted.copy()
    dele[::11] ^= True
    rx = ix.rescore(g, deleted=dele.astype(np.uint8))
    st = pr.Stats(int(g.n_docs), tuple(int(x) for x in g.tot_tokens), np.asarray(g.df_text, np.int64),
                  np.asarray(g.df_name, np.int64))
    ref = mg.ref_of(w.name)
    s, d, n = run(rx, qs, k)
    check(s, d, n, [ref.search(q, k, stats=st, deleted=dele) for q in qs], k, f"{w.name} rescored k={k}")


# ------------------------------------------------------------------ one batch of every shape
def test_batch_mixes_the_shapes(native, ctx, corpus, switches):
    """k_conj, k_disj, k_scan, k_phrase, k_bphrase, k_group, k_gphrase and k_mgroup rows in one plan: each kernel finds
    its own work-item range, k_mgroup's last.  The snapshot carries one facet term per doc (doc % 3) for the scan rows."""
    w, _, qs, want = corpus
    for f in switches:
        f(1)
    args, gaps = w.csr()
    fo, ft = np.arange(w.n + 1, dtype=np.uint64), (np.arange(w.n) % 3).astype(np.uint32)
    ix = native.Index.from_docs(ctx, *args, positions=True, deleted=w.deleted.astype(np.uint8), facets=(fo, ft, 3), **gaps)
    fc = br.Corpus(w.V, args[0], args[1], args[3], args[4], deleted=w.deleted.astype(np.uint8), facets=(fo, ft, 3))
    r = np.random.default_rng(3)
    mid, rare = w.pools["mid"], w.pools["rare"]
    pick = lambda pool, n: [int(x) for x in r.choice(pool, n, replace=False)]  # noqa: E731
    phrases = [mg.phrase_members(q)[0] for q in qs[:12]]
    mixed, new = [], []
    scan = {}  # row -> its facet term
    for i in range(96):
        a, b, c = pick(mid + rare, 3)
        ph = phrases[i % len(phrases)]
        shape = i % 8
        if shape == 7:
            scan[len(mixed)] = i % 3
            mixed.append([])                                             # no text clause, a facet filter: k_scan
        elif shape == 0:
            mixed.append([mg.T(M, a), mg.T(M, b)])                       # a plain AND
        elif shape == 1:
            mixed.append([mg.T(S, a), mg.T(S, b), mg.T(S, c)])           # a plain OR
        elif shape == 2:
            mixed.append([(M if i % 16 < 8 else S, ph)])                 # a single phrase
        elif shape == 3:
            mixed.append([(S, ph), mg.T(S, a)])                          # a phrase beside a term
        elif shape == 4:
            mixed.append([mg.G(M, ANY, [a, b]), mg.T(M, c)])             # a group query
        elif shape == 5:
            mixed.append([(S, ph), mg.G(S, ANY, [a, b])])                # a group beside a phrase
        else:
            new.append(len(mixed))
            mixed.append(qs[(i * 5) % len(qs)])                          # the new shape
    k = 100
    ref = mg.ref_of(w.name)
    q_off, terms, occur, plen, ppos = mg.batch(mixed)
    f_off = np.cumsum([0] + [int(r_ in scan) for r_ in range(len(mixed))]).astype(np.uint32)
    f_terms = np.array([scan[r_] for r_ in sorted(scan)], np.uint32)
    s, d, n = ix.search_batch(q_off, terms, k, occur=occur, phrase_len=plen, phrase_pos=ppos, f_off=f_off, f_terms=f_terms)
    expect = [fc.search([], None, k, fterms=[scan[r_]]) if r_ in scan else ref.search(q, k) for r_, q in enumerate(mixed)]
    check(s, d, n, expect, k, f"{w.name} mixed")
    assert (n > 0).mean() > 0.8 and (n[new] > 0).mean() > 0.8 and (n[sorted(scan)] == k).all()


# ------------------------------------------------------------------ the row limit
def test_sixteen_rows_run_and_seventeen_are_refused(native, corpus, on):
    w, ix, qs, want = corpus
    i = next(i for i, q in enumerate(qs) if mg.n_rows_of(q) == 16)
    s, d, n = run(ix, [qs[i]], 100)
    check(s, d, n, [want[i]], 100, f"{w.name} 16 rows")
    with pytest.raises(native.Unsupported, match="terms"):  # 17 rows: the existing check and message
        run(ix, [[mg.G(S, ANY, [mg.Ph(list(range(9))), mg.Ph(list(range(9, 17)))])]], 10)


# ------------------------------------------------------------------ the switch and the refusals
def test_switch_and_refusals(native, ctx, corpus, switches):
    w, ix, qs, want = corpus
    groups, members, gphrase, beside, filters = switches
    assert (groups(), members(), gphrase(), beside(), filters()) == (0, 0, 0, 0, 0)
    assert members(1) == 0  # the new switch alone: the flags do not parse
    with pytest.raises(native.FuguError, match="bad phrase_len"):
        run(ix, qs[:1], 10)
    assert members(0) == 1 and groups(1) == 0
    with pytest.raises(native.FuguError, match="query 0: a group member's offset must be 0") as e:  # today's answer
        run(ix, qs[:1], 10)
    assert not isinstance(e.value, native.Unsupported)  # FG_EINVAL
    gphrase(1), beside(1), filters(1)
    with pytest.raises(native.FuguError, match="a group member's offset must be 0"):  # (not consulted)
        run(ix, qs[:1], 10)
    gphrase(0), beside(0), filters(0)
    assert members(1) == 0 and members(-1) == 1
    s, d, n = run(ix, qs[:4], 10)
    check(s, d, n, want[:4], 10, "on")
    q_off, terms, occur, plen, ppos = mg.batch(qs[:1])
    kw = dict(occur=occur, phrase_len=plen, phrase_pos=ppos)
    args, gaps = w.csr(0, 200)
    fo = np.arange(201, dtype=np.uint64)
    fx = native.Index.from_docs(ctx, *args, positions=True, facets=(fo, np.zeros(200, np.uint32), 1), **gaps)
    for f in (0, 1):  # whatever fg_filter_clauses says
        filters(f)
        with pytest.raises(native.Unsupported, match="group with phrase members and facet filters"):
            fx.search_batch(q_off, terms, 10, f_off=[0, 1], f_terms=[0], **kw)
    filters(0)
    fx.search_batch(q_off, terms, 10, **kw)
    nopos = native.Index.from_docs(ctx, *args)
    with pytest.raises(native.Unsupported, match="snapshot built without positions"):
        nopos.search_batch(q_off, terms, 10, **kw)
    with pytest.raises(native.Unsupported, match="snapshot built without positions"):
        native.search_sharded([fx, nopos], q_off, terms, 10, **kw)
    with pytest.raises(native.FuguError, match="the model does not cover"):
        ix.model(q_off, terms, 10, phrase_len=plen, phrase_pos=ppos)
    # the ABI's checks with the switch on
    bad = lambda plen, ppos: ix.search_batch([0, 3], [1, 2, 3], 10, occur=np.full(3, S, np.uint8),  # noqa: E731
                                             phrase_len=np.array(plen, np.uint32), phrase_pos=np.array(ppos, np.uint32))
    any3 = 3 | 0x80000000
    with pytest.raises(native.FuguError, match="a group member's offset must be 0"):  # the group's first offset
        bad([any3, 0, 0], [1, 0, 0])
    with pytest.raises(native.FuguError, match="phrase offsets must increase"):
        bad([any3, 0, 0], [0, 2, 2])
    with pytest.raises(native.FuguError, match="phrase offset too large"):
        bad([any3, 0, 0], [0, 1 << 30, 0])
    with pytest.raises(native.FuguError, match="a group needs two members"):
        bad([any3, 0, 0], [0, 1, 2])
    assert members(0) == 1
    with pytest.raises(native.FuguError, match="a group member's offset must be 0"):
        run(ix, qs[:1], 10)


# ------------------------------------------------------------------ fg_db
PHR = mg.PHR
DB_DOCS = [
    ("d0", "send an e-mail to the server admin", None),
    ("d1", "the host got mail e then nothing", None),
    ("d2", "new york pizza and a boston pizza", "New York guide"),
    ("d3", "york new pasta and the art of boston", None),
    ("d4", "disk-full error on the e-mail host", "error log"),
    ("d5", "an enospc error of the full disk", None),
    ("d6", "e mail server e mail host email", "new york pasta"),
    ("d7", "the server sent email to boston", "pizza"),
    ("d8", "the error was disk-full again", None),
    ("d9", "pizza in new york", "e-mail"),
    ("d10", "a full disk is no error", None),
]
DB_QUERIES = [  # (query, its clauses over words)
    ("(e-mail OR email) server", [(S, (ANY, [(PHR, ["e", "mail"], [0, 1]), "email"])), (S, "server")]),
    ('("new york" OR boston) pizza', [(S, (ANY, [(PHR, ["new", "york"], [0, 1]), "boston"])), (S, "pizza")]),
    ("+(disk-full enospc) +error", [(M, (ANY, [(PHR, ["disk", "full"], [0, 1]), "enospc"])), (M, "error")]),
    ("e-mail AND server OR host", [(S, (ALL, [(PHR, ["e", "mail"], [0, 1]), "server"])), (S, "host")]),
]


def db_reference(d, ns):
    """the reference's hit lists [(score, global doc)] of DB_QUERIES over the namespace's current segments"""
    import bool_phrase_ref as bp
    from test_gpu_phrase import py_tokens
    segs = d.segments(ns)
    keep = [g for seg in segs for g in seg]
    info = d.merge_info(ns)
    vocab = {}
    tt, tg, nt, ng = [], [], [], []
    for g in keep:
        for src, dst, dg in ((DB_DOCS[g][1], tt, tg), (DB_DOCS[g][2] or "", nt, ng)):
            toks, gaps = py_tokens(src)
            dst.append([vocab.setdefault(x, len(vocab)) for x in toks])
            dg.append(gaps or None)
    base = bp.Ref(len(vocab), tt, tg, nt, ng)
    assert base.pstats.n == info["n_docs_stats"]
    base.pstats.tot = tuple(info["tot_tokens"])
    ref = mg.Ref(base)
    bounds = np.cumsum([0] + [len(s) for s in segs])
    wid = lambda x: vocab.get(x, mg.MISSING)  # noqa: E731

    def conv(b):
        if isinstance(b, str):
            return wid(b)
        if b[0] == PHR:
            return (PHR, [wid(x) for x in b[1]], list(b[2]))
        return (b[0], [conv(m) for m in b[1]])

    out = []
    for _, cl in DB_QUERIES:
        s, dd = ref.search([(oc, conv(b)) for oc, b in cl], 20, seg_bounds=bounds)
        out.append([(np.float32(x), keep[int(y)]) for x, y in zip(s, dd)])
    return out


def test_db_search_and_json(native, ctx, switches):
    from fugu_amd import db
    groups, members = switches[:2]
    d = db.Database(ctx)
    ns = "mgrp"
    d.create_namespace(ns)
    for i, (rid, text, nm) in enumerate(DB_DOCS):
        d.upsert(db.ObjectRecord(rid, text, metadata={"name": nm} if nm else None), ns)
        if i in (3, 7, 10):  # three commits: three segments (until the merger joins them)
            d.commit(ns)
    d.merge_wait(ns)
    groups(1)
    for q, _ in DB_QUERIES:  # the new switch off: Unsupported, as now
        with pytest.raises(native.Unsupported, match="query outside the device subset"):
            d.search(ns, q)
        with pytest.raises(native.Unsupported):
            d.search_json(ns, q)
    members(1)
    got = [d.search(ns, q, per_page=20) for q, _ in DB_QUERIES]
    want = db_reference(d, ns)
    for q, g, w in zip(DB_QUERIES, got, want):
        assert [x for _, x in g] == [x for _, x in w], (q[0], g, w)
        assert [np.float32(s).view(np.uint32) for s, _ in g] == [s.view(np.uint32) for s, _ in w], (q[0], g, w)
    docs_of = lambda r: {g for _, g in r}  # noqa: E731
    assert docs_of(got[0]) == {0, 4, 6, 7, 9} and docs_of(got[1]) == {2, 3, 6, 7, 9}
    assert docs_of(got[2]) == {4, 5, 8} and docs_of(got[3]) == {0, 1, 4, 6}
    for (q, _), r in zip(DB_QUERIES, got):
        js = json.loads(d.search_json(ns, q, per_page=20))
        assert [x["id"] for x in js["results"]] == [DB_DOCS[g][0] for _, g in r]
        assert np.allclose([x["score"] for x in js["results"]], [x for x, _ in r], rtol=1e-6, atol=0)
    was = native.count_clauses(1)  # counts on this shape are out of scope: Unsupported, not the count ABI's FG_EINVAL
    try:
        for q, _ in DB_QUERIES:
            with pytest.raises(native.Unsupported, match="group with phrase members in a count query"):
                d.facet_counts(ns, "/", query=q)
        plain = "(server OR host) mail"  # a plain group is counted as before
        assert d.facet_counts(ns, "/", query=plain)[1] == len(d.search(ns, plain, per_page=20)) >= 5
    finally:
        native.count_clauses(was)
    members(0)
    with pytest.raises(native.Unsupported, match="query outside the device subset"):  # the same process, off again
        d.search(ns, DB_QUERIES[0][0])
