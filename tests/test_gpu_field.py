"""Field-qualified term clauses on the device (k_field, DESIGN.md §20, behind
fg_field_clauses) against the numpy reference tests/field_ref.py on (doc, score
bits), every query compared.  Every test that sets the switch does so through the
`switch` fixture (`on`: it, turned on), which restores the setting it found in
teardown.

- field_ref.synth() (12,000 docs, 64 terms in two fields, deletions, merged lead
  lists of 2047 / 2048 / 2049 / 8193 postings, a term in 40 docs, terms in one
  field only and in both, escaped tfs in either field, an absent term) x 12
  queries of each of field_ref.KINDS at k = 1, 10, 100, 1000: the small k make
  thresholds rise inside an item, so the chunk bound fires; the `tie` kind holds
  queries whose k-th and (k+1)-th hits tie on score;
- the corpus as three segments of unequal size (the second has no name postings
  at all, only the last holds T_FEW): fg_search_sharded and a multi-snapshot
  plan's slots merged on the host;
- a rescored snapshot: changed statistics and deletions, bounds scaled by q_rup;
- fg_db_search and the JSON handler over a small committed namespace;
- a batch mixing them with plain AND / OR / single-term queries;
- the refusals, and the switch itself.
test_field_ref.py checks, without a GPU, that the queries decide something.
"""
import json

import numpy as np
import pytest

import bool_ref as br
import field_ref as fr
from shard_ref import merge_topk_numpy

pytestmark = pytest.mark.gpu
M, S, X = fr.MUST, fr.SHOULD, fr.MUST_NOT
TEXT, NAME = fr.TEXT, fr.NAME


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
    """sets fg_field_clauses; the setting found is restored in teardown"""
    was = native.field_clauses()
    yield native.field_clauses
    native.field_clauses(was)


@pytest.fixture()
def on(switch):
    switch(1)


@pytest.fixture()
def others(native):
    """the other six switches, as a setter of all of them; the settings found are restored in teardown"""
    fs = [native.phrase_clauses, native.group_clauses, native.filter_clauses, native.count_clauses,
          native.group_phrase_clauses, native.group_member_phrases]
    was = [f() for f in fs]
    yield lambda v: [f(v) for f in fs]
    for f, w in zip(fs, was):
        f(w)


def check(s, d, n, want, k, tag=""):
    """device rows (s, d, n) against the reference lists `want` [(scores, docs)] cut at k: (doc, score bits)"""
    for i, (rs, rd) in enumerate(want):
        m = int(n[i])
        got, ref = fr.hits_of(s[i, :m], d[i, :m]), fr.hits_of(rs[:k], rd[:k])
        assert got == ref, (tag, i, m, len(ref), [x for x in zip(got, ref) if x[0] != x[1]][:3])


def run(ix, queries, k):
    q_off, terms, occur, plen, ppos = fr.batch(queries)
    return ix.search_batch(q_off, terms, k, occur=occur, phrase_len=plen, phrase_pos=ppos)


@pytest.fixture(scope="module")
def corpus(native, ctx):
    c = fr.synth()
    ref = fr.Ref(c.corpus)
    ix = native.Index.from_docs(ctx, c.text_off, c.text_tok, fr.V, c.name_off, c.name_tok, deleted=c.deleted)
    kinds = fr.queries()
    qs = [q for kind in fr.KINDS for q in kinds[kind]]
    want = [ref.search(q, 1000) for q in qs]  # computed once, shared, never changed
    return c, ix, ref, qs, want


# ------------------------------------------------------------------ every query, every k
@pytest.mark.parametrize("k", fr.KS)
def test_corpus_matches_reference(native, corpus, on, k):
    c, ix, ref, qs, want = corpus
    assert len(qs) == fr.PER_KIND * len(fr.KINDS) >= 108
    s, d, n = run(ix, qs, k)
    check(s, d, n, want, k, f"k={k}")
    assert (n > 0).mean() >= 0.9
    if k in (10, 100):  # a query whose k-th and (k+1)-th hits tie on score is among them
        assert any(len(rs) > k and rs[k - 1] == rs[k] for rs, _ in want)
    if k == 10:  # the escaped tfs are in some top 10
        esc = {x for docs in fr.ESC_DOCS.values() for x in docs}
        assert esc & {int(x) for i in range(len(qs)) for x in d[i, :int(n[i])]}


def test_batches_of_one_spread_the_lead_chunks(native, corpus, on):
    c, ix, ref, qs, want = corpus
    for i in range(0, len(qs), fr.PER_KIND + 1):  # a query of every kind, alone: up to 64 items per pass
        s, d, n = run(ix, [qs[i]], 10)
        check(s, d, n, [want[i]], 10, f"alone {i}")


def test_same_term_in_both_fields_is_the_unqualified_term(native, corpus, on):
    """`name:a text:a` on k_field against the plain `a` on the kernels of before: docs and score bits"""
    c, ix, ref, qs, want = corpus
    two = fr.queries()[fr.EQUAL]
    q_off, terms, occur, _, _ = fr.batch([[fr.C(S, q[0][1])] for q in two])
    for k in (10, 1000):
        a, b = run(ix, two, k), ix.search_batch(q_off, terms, k, occur=occur)
        assert np.array_equal(a[2], b[2]) and (b[2] > 0).all()
        for i in range(len(two)):
            m = int(a[2][i])
            assert fr.hits_of(a[0][i, :m], a[1][i, :m]) == fr.hits_of(b[0][i, :m], b[1][i, :m]), (k, i)


# ------------------------------------------------------------------ segments, rescored snapshots
@pytest.fixture(scope="module")
def segments(native, ctx, corpus):
    c, _, ref, qs, want = corpus
    cuts = list(fr.SEG_CUTS)
    g = None
    for lo, hi in zip(cuts, cuts[1:]):
        x = native.docs_stats(*c.segment(lo, hi)[:2], fr.V, *c.segment(lo, hi)[2:])
        g = x if g is None else g + x
    ixs = []
    for lo, hi in zip(cuts, cuts[1:]):
        to, tt, no, nt = c.segment(lo, hi)
        ixs.append(native.Index.from_docs(ctx, to, tt, fr.V, no, nt, deleted=c.deleted[lo:hi], global_stats=g))
    assert [x.stats().has_name for x in ixs] == [True, False, True]  # the second: no name postings at all
    swant = [ref.search(q, 1000, seg_bounds=cuts) for q in qs]
    return ixs, np.array(cuts[:-1], np.int64), swant


@pytest.mark.parametrize("k", [10, 1000])
def test_segments_equal_the_reference(native, ctx, corpus, segments, on, k):
    c, _, ref, qs, want = corpus
    ixs, base, swant = segments
    # the segments order their Musts by their own costs: some sums differ from the one-snapshot ones
    q_off, terms, occur, plen, ppos = fr.batch(qs)
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
    # a `name:` Must has no hit in the nameless segment, T_FEW none outside the last
    q = [[fr.C(M, fr.T_LONG, NAME)], [fr.C(S, fr.T_FEW, TEXT), fr.C(S, fr.T_FEW, NAME)]]
    b = fr.batch(q)
    s, d, sh, n = native.search_sharded(ixs, b[0], b[1], 1000, ctx=ctx, occur=b[2], phrase_len=b[3], phrase_pos=b[4])
    assert int(n[0]) == 1000 and 1 not in set(sh[0].tolist())
    assert int(n[1]) > 0 and set(sh[1, :int(n[1])].tolist()) == {2}
    check(s, d.astype(np.int64) + base[sh], n, [ref.search(x, 1000, seg_bounds=list(fr.SEG_CUTS)) for x in q], 1000, "absent")


@pytest.mark.parametrize("k", [10, 1000])
def test_rescored_snapshot(native, ctx, corpus, on, k):
    """statistics changed after the build: query-time scores, the chunk and term bounds scaled by q_rup"""
    c, ix, ref, qs, _ = corpus
    r = np.random.default_rng(9)
    own = native.docs_stats(c.text_off, c.text_tok, fr.V, c.name_off, c.name_tok)
    other = native.ShardStats(7000, (90000, 5000), r.integers(0, 3000, fr.V).astype(np.uint32),
                              r.integers(0, 900, fr.V).astype(np.uint32))
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
        mixed.append([fr.C(o, int(r.integers(0, 56))) for o in oc])
    plain = [q for q, kd in zip(mixed, kind) if kd < 0]
    rows = [i for i, kd in enumerate(kind) if kd < 0]
    new = [i for i, kd in enumerate(kind) if kd >= 0]
    k = 100

    def plain_only(queries):  # without phrase_len: the call of before
        q_off, terms, occur, _, _ = fr.batch(queries)
        return ix.search_batch(q_off, terms, k, occur=occur)

    assert switch(0) == 0
    off = plain_only(plain)
    with pytest.raises(native.FuguError, match="bad phrase_len"):
        run(ix, mixed, k)
    switch(1)
    alone, both = run(ix, plain, k), run(ix, mixed, k)
    switch(0)
    check(both[0][new], both[1][new], both[2][new], [want[kind[i]] for i in new], k, "mixed")
    for a in (alone, off):  # the plain rows: byte-identical without the field queries, and with the switch off
        assert np.array_equal(both[2][rows], a[2])
        for j, i in enumerate(rows):  # (a row's first n entries: the rest is not written)
            m = int(a[2][j])
            assert np.array_equal(both[1][i, :m], a[1][j, :m]), i
            assert np.array_equal(both[0][i, :m].view(np.uint32), a[0][j, :m].view(np.uint32)), i
    # the plain rows against the reference too
    for j, q in enumerate(plain):
        rs, rd = ref.search(q, k)
        assert fr.hits_of(off[0][j, :int(off[2][j])], off[1][j, :int(off[2][j])]) == fr.hits_of(rs, rd), j
    assert (off[2] > 0).mean() > 0.5


# ------------------------------------------------------------------ the switch and the refusals
def test_switch_off_answers_as_today(native, corpus, switch):
    c, ix, ref, qs, want = corpus
    assert switch() == 0
    for q in (qs[0], [fr.C(M, 6, NAME), fr.C(M, 7)], [fr.C(S, 6, TEXT)]):
        with pytest.raises(native.FuguError, match="query 0: bad phrase_len at term 0") as e:  # today's answer, FG_EINVAL
            run(ix, [q], 10)
        assert e.value.code == native.FG_EINVAL and not isinstance(e.value, native.Unsupported)
    with pytest.raises(native.FuguError, match="query 0: bad phrase_len at term 1") as e:
        run(ix, [[fr.C(M, 7), fr.C(M, 6, NAME)]], 10)
    assert e.value.code == native.FG_EINVAL
    b = fr.batch([[fr.C(S, 6, NAME)]])
    kw = dict(occur=b[2], phrase_len=b[3], phrase_pos=b[4])
    with pytest.raises(native.FuguError, match="bad phrase_len at term 0"):
        native.Plan([ix, ix], b[0], b[1], 10, **kw)
    with pytest.raises(native.Unsupported, match="phrase clause in a count query"):
        native.count_batch([ix], b[0], b[1], **kw)
    with pytest.raises(native.FuguError, match="does not cover phrase queries"):
        ix.model(b[0], b[1], 10, phrase_len=b[3], phrase_pos=b[4])


def test_switch_and_refusals(native, ctx, corpus, switch, others):
    c, ix, ref, qs, want = corpus
    assert switch(1) == 0 and switch(-1) == 1
    s, d, n = run(ix, qs[:4], 10)
    check(s, d, n, want[:4], 10, "on")
    T_, N_, ANY, ALL = native.CLAUSE_TEXT, native.CLAUSE_NAME, native.CLAUSE_ANY, native.CLAUSE_ALL
    bad = lambda plen, ppos=None, terms=(6, 7, 8): ix.search_batch(  # noqa: E731
        [0, len(terms)], list(terms), 10, occur=[S] * len(terms), phrase_len=plen,
        phrase_pos=ppos or [0] * len(terms))
    q_off, terms, occur, plen, ppos = fr.batch([[fr.C(S, 6, NAME), fr.C(S, 8)]])
    kw = dict(occur=occur, phrase_len=plen, phrase_pos=ppos)
    fo = np.arange(201, dtype=np.uint64)
    to, tt, no, nt = c.segment(0, 200)
    fx = native.Index.from_docs(ctx, to, tt, fr.V, no, nt, facets=(fo, np.zeros(200, np.uint32), 1))
    for v in (0, 1):  # whatever the other six switches say
        others(v)
        with pytest.raises(native.FuguError, match="query 0: bad phrase_len at term 1") as e:  # both flags on one entry
            bad([1, 1 | T_ | N_, 1])
        assert e.value.code == native.FG_EINVAL and not isinstance(e.value, native.Unsupported)
        for plen_ in ([2 | N_, 0, 1], [3 | T_, 0, 0], [0 | N_, 1, 1], [1, 1, 2 | T_]):  # a count that is not 1
            with pytest.raises(native.Unsupported, match="field-qualified phrase"):
                bad(plen_)
        for plen_ in ([2 | ANY | N_, 0, 1], [1, 2 | ALL | T_, 0], [1 | ANY | T_, 1, 1]):  # together with ANY / ALL
            with pytest.raises(native.Unsupported, match="field-qualified group"):
                bad(plen_)
        with pytest.raises(native.Unsupported, match="field clause beside a phrase clause"):
            bad([1 | N_, 2, 0], [0, 0, 1])
        with pytest.raises(native.Unsupported, match="field clause beside a phrase clause"):
            bad([2, 0, 1 | T_], [0, 1, 0])
        with pytest.raises(native.Unsupported, match="field clause with facet filters"):
            fx.search_batch(q_off, terms, 10, f_off=[0, 1], f_terms=[0], **kw)
        assert int(fx.search_batch(q_off, terms, 10, **kw)[2][0]) > 0
        with pytest.raises(native.Unsupported, match="field clause in a count query"):
            native.count_batch([ix], q_off, terms, **kw)
        with pytest.raises(native.Unsupported, match="does not cover field clauses"):
            ix.model(q_off, terms, 10, phrase_len=plen, phrase_pos=ppos)
    # with fg_group_clauses on (the flags parse): a field flag on a group's member row, a field clause beside a group
    with pytest.raises(native.Unsupported, match="field-qualified group"):
        bad([2 | ANY, N_, 1])
    with pytest.raises(native.Unsupported, match="field-qualified group"):
        bad([3 | ALL, 0, 1 | T_])
    with pytest.raises(native.Unsupported, match="field clause beside a group clause"):
        bad([1 | N_, 2 | ANY, 0])
    with pytest.raises(native.Unsupported, match="field clause beside a group clause"):
        bad([2 | ALL, 0, 1 | T_])
    others(0)
    with pytest.raises(native.Unsupported, match="terms"):  # 17 terms: the existing check and message
        run(ix, [[fr.C(S, t, NAME) for t in range(6, 23)]], 10)
    s, d, n = run(ix, [[fr.C(S, t, (NAME, TEXT, None)[t % 3]) for t in range(6, 22)]], 10)  # 16: within FG_MAX_TERMS
    check(s, d, n, [ref.search([fr.C(S, t, (NAME, TEXT, None)[t % 3]) for t in range(6, 22)], 10)], 10, "16 clauses")
    assert switch(0) == 1
    with pytest.raises(native.FuguError, match="bad phrase_len"):  # today's answer again
        run(ix, qs[:1], 10)


# ------------------------------------------------------------------ fg_db
DB_DOCS = [
    ("d0", "a b c", None), ("d1", "a c c d", "b"), ("d2", "b d", None), ("d3", "a a b", "c a"),
    ("d4", "c d e", None), ("d5", "b c e e", "report"), ("d6", "a d", "c"), ("d7", "e f", None),
    ("d8", "a b c d e f", "a b"), ("d9", "c report", None), ("d10", "b b a f", "quarterly report"), ("d11", "a c", "d"),
    ("d12", "a f e", None),
]
DB_QUERIES = [  # (query, its clauses as field_ref's, over words)
    ("name:report", [(S, "report", NAME)]),
    ("text:report", [(S, "report", TEXT)]),
    ("+name:a +b", [(M, "a", NAME), (M, "b", None)]),
    ("+name:c +text:a", [(M, "c", NAME), (M, "a", TEXT)]),
    ("name:a text:a", [(S, "a", NAME), (S, "a", TEXT)]),
    ("text:c OR name:b OR d", [(S, "c", TEXT), (S, "b", NAME), (S, "d", None)]),
    ("a -name:c", [(S, "a", None), (X, "c", NAME)]),
    ("+text:a name:b", [(M, "a", TEXT), (S, "b", NAME)]),
    ("+name:f a", [(M, "f", NAME), (S, "a", None)]),  # no doc names f
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
    ref = fr.Ref(cor)
    bounds = np.cumsum([0] + [len(s) for s in segs])
    out = []
    for _, q in DB_QUERIES:
        q = [(oc, vocab.get(w, fr.V * 1000), f) for oc, w, f in q]
        s, dd = ref.search(q, 20, seg_bounds=bounds, stats=st)
        out.append([(np.float32(x), keep[int(y)]) for x, y in zip(s, dd)])
    return out


def test_db_search_and_json(native, ctx, switch):
    from fugu_amd import db
    d = db.Database(ctx)
    ns = "fld"
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
    assert docs_of(got[0]) == {5, 10} and docs_of(got[1]) == {9}           # the title, not the body; and the reverse
    assert docs_of(got[2]) == {3, 8} and docs_of(got[3]) == {3, 6}
    assert docs_of(got[4]) == {0, 1, 3, 6, 8, 10, 11, 12} == docs_of(d.search(ns, "a", per_page=20))
    assert [np.float32(s).view(np.uint32) for s, _ in got[4]] == \
        [np.float32(s).view(np.uint32) for s, _ in d.search(ns, "a", per_page=20)]
    assert docs_of(got[6]) == {0, 1, 8, 10, 11, 12} and docs_of(got[8]) == set()
    for (q, _), r in zip(DB_QUERIES, got):
        js = json.loads(d.search_json(ns, q, per_page=20))
        assert [x["id"] for x in js["results"]] == [DB_DOCS[g][0] for _, g in r]
        assert np.allclose([x["score"] for x in js["results"]], [x for x, _ in r], rtol=1e-6, atol=0)
    with pytest.raises(native.Unsupported, match="field clause in a count query"):
        d.facet_counts(ns, "/", "name:report")
    with pytest.raises(native.Unsupported, match="field-qualified phrase"):
        d.search(ns, 'name:"quarterly report"')
    with pytest.raises(native.Unsupported, match=r"field outside \[text, name\]"):
        d.search(ns, "id:d5")
    switch(0)
    with pytest.raises(native.Unsupported, match="query outside the device subset"):  # the same process, off again
        d.search(ns, "name:report")
