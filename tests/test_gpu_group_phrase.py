"""A group clause beside a phrase clause on the device (k_gphrase, DESIGN.md §18,
behind fg_group_phrase_clauses with fg_group_clauses) against the numpy reference
tests/group_phrase_ref.py on (doc, score bits), every query compared.  Every test
sets the switches through the `switches` fixture (`on`: the two, turned on), which
restores what it found in teardown.

- corpus A (phrase_ref.Synth(): 6000 docs of 1 to 300 tokens, names, gaps,
  deletions) and corpus B (group_ref.synth() with positions: lead lists of 2047 /
  2048 / 2049 / 8193 postings, an escaped tf) x every query of every kind of
  group_phrase_ref.KINDS at k = 1, 10, 100, 1000; batches of one;
- corpus A as three unequal segments, the first lacking terms of the queries:
  fg_search_sharded and a multi-snapshot plan's slots merged on the host;
- a rescored snapshot: changed statistics and deletions;
- one batch of a plain AND, a plain OR, a single phrase, a phrase beside a term, a
  group query and the new shape with every switch on, each row against its own
  reference: the kernels' work-item ranges;
- fg_db_search and the JSON handler over a small committed namespace with
  hyphenated words;
- the switch and the refusals.
test_group_phrase_ref.py checks, without a GPU, that the queries decide something.
"""
import json

import numpy as np
import pytest

import group_phrase_ref as gp
import phrase_ref as pr
from shard_ref import merge_topk_numpy

pytestmark = pytest.mark.gpu
M, S, X = gp.M, gp.S, gp.X
ANY, ALL = gp.ANY, gp.ALL


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
    """(group_clauses, group_phrase_clauses, phrase_clauses, filter_clauses); the settings found are restored"""
    fns = (native.group_clauses, native.group_phrase_clauses, native.phrase_clauses, native.filter_clauses)
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
        got, ref = gp.hits_of(s[i, :m], d[i, :m]), gp.hits_of(rs[:k], rd[:k])
        assert got == ref, (tag, i, m, len(ref), [x for x in zip(got, ref) if x[0] != x[1]][:3])


def run(ix, queries, k):
    q_off, terms, occur, plen, ppos = gp.batch(queries)
    return ix.search_batch(q_off, terms, k, occur=occur, phrase_len=plen, phrase_pos=ppos)


def build(native, ctx, w, lo=0, hi=None, deleted=None, **kw):
    args, gaps = w.csr(lo, hi)
    dele = w.deleted[lo:hi] if deleted is None else deleted
    return native.Index.from_docs(ctx, *args, positions=True, deleted=dele.astype(np.uint8), **gaps, **kw)


@pytest.fixture(scope="module", params=["A", "B"])
def corpus(request, native, ctx):
    w = gp.world(request.param)
    ix = build(native, ctx, w)
    kinds = gp.queries(w.name)
    qs = [q for kind in gp.kinds_of(w.name) for q in kinds[kind]]
    want = [w.ref.search(q, 1000) for q in qs]  # computed once, shared, never changed
    return w, ix, qs, want


# ------------------------------------------------------------------ every query, every k
@pytest.mark.parametrize("k", gp.KS)
def test_corpus_matches_reference(native, corpus, on, k):
    w, ix, qs, want = corpus
    assert len(qs) == gp.PER_KIND * len(gp.kinds_of(w.name)) >= 15 * 4
    s, d, n = run(ix, qs, k)
    check(s, d, n, want, k, f"{w.name} k={k}")
    assert (n > 0).mean() >= 0.9
    if k in (10, 100):  # a query whose k-th and (k+1)-th hits tie on score is among them
        assert any(len(rs) > k and rs[k - 1] == rs[k] for rs, _ in want)


def test_batches_of_one_spread_the_lead_chunks(native, corpus, on):
    w, ix, qs, want = corpus
    for i in range(0, len(qs), gp.PER_KIND + 1):  # a query of every kind, alone: up to 64 items per pass
        s, d, n = run(ix, [qs[i]], 10)
        check(s, d, n, [want[i]], 10, f"{w.name} alone {i}")


# ------------------------------------------------------------------ segments, rescored snapshots
@pytest.fixture(scope="module")
def world_a(native, ctx):
    w = gp.world("A")
    kinds = gp.queries("A")
    qs = [q for kind in gp.kinds_of("A") for q in kinds[kind]]
    return w, qs


@pytest.mark.parametrize("k", [10, 1000])
def test_segments_equal_the_reference(native, ctx, world_a, on, k):
    w, qs = world_a
    cuts = list(gp.SEG_CUTS_A)
    g = None
    for lo, hi in zip(cuts, cuts[1:]):
        x = native.docs_stats(*w.csr(lo, hi)[0])
        g = x if g is None else g + x
    ixs = [build(native, ctx, w, lo, hi, global_stats=g) for lo, hi in zip(cuts, cuts[1:])]
    base = np.array(cuts[:-1], np.int64)
    swant = [w.ref.search(q, k, seg_bounds=cuts) for q in qs]
    q_off, terms, occur, plen, ppos = gp.batch(qs)
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
    s, d, n = run(rx, qs, k)
    check(s, d, n, [w.ref.search(q, k, stats=st, deleted=dele) for q in qs], k, f"{w.name} rescored k={k}")


# ------------------------------------------------------------------ one batch of every shape
def test_batch_mixes_the_shapes(native, ctx, corpus, switches):
    """k_conj, k_disj, k_phrase, k_bphrase, k_group and k_gphrase rows in one plan: each kernel finds its own items"""
    w, ix, qs, want = corpus
    for f in switches:
        f(1)
    r = np.random.default_rng(3)
    mid, rare = w.pools["mid"], w.pools["rare"]
    pick = lambda pool, n: [int(x) for x in r.choice(pool, n, replace=False)]  # noqa: E731
    phrases = [next(b for _, b in q if gp.is_phrase(b)) for q in qs[:12]]
    mixed, new = [], []
    for i in range(72):
        a, b, c = pick(mid + rare, 3)
        ph = phrases[i % len(phrases)]
        shape = i % 6
        if shape == 0:
            mixed.append([gp.T(M, a), gp.T(M, b)])                       # a plain AND
        elif shape == 1:
            mixed.append([gp.T(S, a), gp.T(S, b), gp.T(S, c)])           # a plain OR
        elif shape == 2:
            mixed.append([(M if i % 12 < 6 else S, ph)])                 # a single phrase
        elif shape == 3:
            mixed.append([(S, ph), gp.T(S, a)])                          # a phrase beside a term
        elif shape == 4:
            mixed.append([gp.G(M, ANY, [a, b]), gp.T(M, c)])             # a group query
        else:
            new.append(len(mixed))
            mixed.append(qs[(i * 7) % len(qs)])                          # the new shape
    k = 100
    s, d, n = run(ix, mixed, k)
    check(s, d, n, [w.ref.search(q, k) for q in mixed], k, f"{w.name} mixed")
    assert (n > 0).mean() > 0.8 and (n[new] > 0).mean() > 0.8


# ------------------------------------------------------------------ the switch and the refusals
def test_switch_and_refusals(native, ctx, corpus, switches):
    w, ix, qs, want = corpus
    groups, gphrase, beside, filters = switches
    assert (groups(), gphrase(), beside(), filters()) == (0, 0, 0, 0)
    assert gphrase(1) == 0  # the new switch alone: the flags do not parse
    with pytest.raises(native.FuguError, match="bad phrase_len"):
        run(ix, qs[:1], 10)
    assert gphrase(0) == 1 and groups(1) == 0
    with pytest.raises(native.Unsupported, match="query 0: group clause beside a phrase clause"):  # today's message
        run(ix, qs[:1], 10)
    beside(1)
    with pytest.raises(native.Unsupported, match="group clause beside a phrase clause"):  # (not consulted)
        run(ix, qs[:1], 10)
    beside(0)
    assert gphrase(1) == 0 and gphrase(-1) == 1
    s, d, n = run(ix, qs[:4], 10)
    check(s, d, n, want[:4], 10, "on")
    q_off, terms, occur, plen, ppos = gp.batch(qs[:1])
    kw = dict(occur=occur, phrase_len=plen, phrase_pos=ppos)
    args, gaps = w.csr(0, 200)
    fo = np.arange(201, dtype=np.uint64)
    fx = native.Index.from_docs(ctx, *args, positions=True, facets=(fo, np.zeros(200, np.uint32), 1), **gaps)
    for f in (0, 1):  # whatever fg_filter_clauses says
        filters(f)
        with pytest.raises(native.Unsupported, match="group and phrase clauses with facet filters"):
            fx.search_batch(q_off, terms, 10, f_off=[0, 1], f_terms=[0], **kw)
    filters(0)
    fx.search_batch(q_off, terms, 10, **kw)
    nopos = native.Index.from_docs(ctx, *args)
    with pytest.raises(native.Unsupported, match="snapshot built without positions"):
        nopos.search_batch(q_off, terms, 10, **kw)
    with pytest.raises(native.Unsupported, match="snapshot built without positions"):
        native.search_sharded([fx, nopos], q_off, terms, 10, **kw)
    with pytest.raises(native.FuguError, match="the model does not cover"):  # (phrase or group: whichever stands first)
        ix.model(q_off, terms, 10, phrase_len=plen, phrase_pos=ppos)
    with pytest.raises(native.Unsupported, match="terms"):  # 17 terms: the existing check and message
        run(ix, [[gp.P(S, list(range(9))), gp.G(S, ANY, list(range(9, 17)))]], 10)
    assert gphrase(0) == 1
    with pytest.raises(native.Unsupported, match="group clause beside a phrase clause"):
        run(ix, qs[:1], 10)


# ------------------------------------------------------------------ fg_db
DB_DOCS = [
    ("d0", "send an e-mail to the server admin", None),
    ("d1", "the host got mail e then nothing", None),
    ("d2", "new york pizza and a state-of-the-art gpu", "New York guide"),
    ("d3", "york new pasta and the art of state", None),
    ("d4", "disk-full error on the e-mail host", "error log"),
    ("d5", "a failure of the full disk of pasta", None),
    ("d6", "e mail server e mail host", "new york pasta"),
    ("d7", "state of the art accelerator beside a cpu", "state of the art"),
    ("d8", "the failure was disk-full again", None),
    ("d9", "pizza in new york", "e-mail"),
    ("d10", "an accelerator is no gpu", None),
]
DB_QUERIES = [  # (query, its clauses over words)
    ("e-mail (server OR host)", [(S, (gp.PHR, ["e", "mail"], [0, 1])), (S, (ANY, ["server", "host"]))]),
    ('"new york" AND (pizza OR pasta)', [(M, (gp.PHR, ["new", "york"], [0, 1])), (M, (ANY, ["pizza", "pasta"]))]),
    ("+(error failure) +disk-full", [(M, (ANY, ["error", "failure"])), (M, (gp.PHR, ["disk", "full"], [0, 1]))]),
    ("state-of-the-art (gpu OR accelerator) -cpu",
     [(S, (gp.PHR, ["state", "of", "the", "art"], [0, 1, 2, 3])), (S, (ANY, ["gpu", "accelerator"])), (X, "cpu")]),
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
    ref = gp.Ref(base)
    bounds = np.cumsum([0] + [len(s) for s in segs])
    wid = lambda x: vocab.get(x, gp.MISSING)  # noqa: E731
    out = []
    for _, cl in DB_QUERIES:
        q = [(oc, wid(b)) if isinstance(b, str) else (oc, (b[0], [wid(x) for x in b[1]]) + tuple(b[2:])) for oc, b in cl]
        s, dd = ref.search(q, 20, seg_bounds=bounds)
        out.append([(np.float32(x), keep[int(y)]) for x, y in zip(s, dd)])
    return out


def test_db_search_and_json(native, ctx, switches):
    from fugu_amd import db
    groups, gphrase = switches[:2]
    d = db.Database(ctx)
    ns = "gphr"
    d.create_namespace(ns)
    for i, (rid, text, nm) in enumerate(DB_DOCS):
        d.upsert(db.ObjectRecord(rid, text, metadata={"name": nm} if nm else None), ns)
        if i in (3, 7, 10):  # three commits: three segments (until the merger joins them)
            d.commit(ns)
    d.merge_wait(ns)
    groups(1)
    for q, _ in DB_QUERIES:  # the new switch off: refused as now
        with pytest.raises(native.Unsupported, match="group clause beside a phrase clause"):
            d.search(ns, q)
        with pytest.raises(native.Unsupported):
            d.search_json(ns, q)
    gphrase(1)
    got = [d.search(ns, q, per_page=20) for q, _ in DB_QUERIES]
    want = db_reference(d, ns)
    for q, g, w in zip(DB_QUERIES, got, want):
        assert [x for _, x in g] == [x for _, x in w], (q[0], g, w)
        assert [np.float32(s).view(np.uint32) for s, _ in g] == [s.view(np.uint32) for s, _ in w], (q[0], g, w)
    docs_of = lambda r: {g for _, g in r}  # noqa: E731
    assert docs_of(got[0]) == {0, 1, 4, 6, 9} and docs_of(got[1]) == {2, 6, 9}
    assert docs_of(got[2]) == {4, 8} and docs_of(got[3]) == {2, 10}
    for (q, _), r in zip(DB_QUERIES, got):
        js = json.loads(d.search_json(ns, q, per_page=20))
        assert [x["id"] for x in js["results"]] == [DB_DOCS[g][0] for _, g in r]
        assert np.allclose([x["score"] for x in js["results"]], [x for x, _ in r], rtol=1e-6, atol=0)
    gphrase(0)
    with pytest.raises(native.Unsupported, match="group clause beside a phrase clause"):  # the same process, off again
        d.search(ns, DB_QUERIES[0][0])
