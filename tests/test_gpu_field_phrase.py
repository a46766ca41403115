"""Field-qualified phrase clauses on the device (k_fphrase, DESIGN.md §21, behind
fg_field_phrases on top of fg_field_clauses) against the numpy reference
tests/field_phrase_ref.py on (doc, score bits), every query compared.  Every test
that sets a switch does so through the `switch` / `fields` fixtures, which restore
the settings they found in teardown.

- field_phrase_ref.synth() (12,000 docs as token streams in two fields, deletions,
  lead lists of 2047 / 2048 / 2049 merged postings whose docs are text only, both
  and name only, tf >= 255 in either field, a gap inside a name, a repeated-term
  phrase, absent terms) x 12 queries of each of field_phrase_ref.KINDS at k = 1,
  10, 100, 1000; one of every kind alone, as a batch of one;
- `name:"a b" text:"a b"` against the plain phrase on k_phrase;
- the corpus as three segments of unequal size (the second has no name tokens at
  all, only the last holds X_A / X_T): fg_search_sharded and a multi-snapshot plan;
- a rescored snapshot;
- fg_db_search and the JSON handler over a small committed namespace;
- a batch mixing them with plain AND / OR / phrase / field-term queries;
- the refusals that stay, and the switch itself.
test_field_phrase_ref.py checks, without a GPU, that the queries decide something.
"""
import json

import numpy as np
import pytest

import field_phrase_ref as fp
import phrase_ref as pr
from shard_ref import merge_topk_numpy

pytestmark = pytest.mark.gpu
M, S, X = fp.MUST, fp.SHOULD, fp.MUST_NOT
TEXT, NAME = fp.TEXT, fp.NAME


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
def fields(native):
    """sets fg_field_clauses; the setting found is restored in teardown"""
    was = native.field_clauses()
    yield native.field_clauses
    native.field_clauses(was)


@pytest.fixture()
def switch(native):
    """sets fg_field_phrases; the setting found is restored in teardown"""
    was = native.field_phrases()
    yield native.field_phrases
    native.field_phrases(was)


@pytest.fixture()
def on(fields, switch):
    fields(1)
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
        got, ref = fp.hits_of(s[i, :m], d[i, :m]), fp.hits_of(rs[:k], rd[:k])
        assert got == ref, (tag, i, m, len(ref), [x for x in zip(got, ref) if x[0] != x[1]][:3])


def run(ix, queries, k):
    q_off, terms, occur, plen, ppos = fp.batch(queries)
    return ix.search_batch(q_off, terms, k, occur=occur, phrase_len=plen, phrase_pos=ppos)


def build(native, ctx, c, lo=0, hi=None, **kw):
    to, tt, tg = c.csr(c.text, c.text_gaps, lo, hi)
    no, nt, ng = c.csr(c.name, c.name_gaps, lo, hi)
    return native.Index.from_docs(ctx, to, tt, fp.V_ALL, no, nt, positions=True, text_gaps=tg, name_gaps=ng, **kw)


@pytest.fixture(scope="module")
def corpus(native, ctx):
    c = fp.synth()
    ref = c.ref()
    ix = build(native, ctx, c, deleted=c.deleted.astype(np.uint8))
    kinds = fp.queries()
    qs = [q for kind in fp.KINDS for q in kinds[kind]]
    want = [ref.search(q, 1000) for q in qs]  # computed once, shared, never changed
    return c, ix, ref, qs, want


# ------------------------------------------------------------------ every query, every k
@pytest.mark.parametrize("k", fp.KS)
def test_corpus_matches_reference(native, corpus, on, k):
    c, ix, ref, qs, want = corpus
    assert len(qs) == fp.PER_KIND * len(fp.KINDS) >= 132
    s, d, n = run(ix, qs, k)
    check(s, d, n, want, k, f"k={k}")
    assert (n > 0).mean() >= 0.83  # (11 of 12 in ten kinds; the `lacking` kind has no hits)
    if k in (10, 100):  # a query whose k-th and (k+1)-th hits tie on score is among them
        assert any(len(rs) > k and rs[k - 1] == rs[k] for rs, _ in want)
    if k == 10:  # the escaped tfs are in some top 10
        esc = set(fp.ESC_NAME_DOCS) | set(fp.ESC_TEXT_DOCS)
        assert esc <= {int(x) for i in range(len(qs)) for x in d[i, :int(n[i])]}


def test_batches_of_one_spread_the_lead_chunks(native, corpus, on):
    c, ix, ref, qs, want = corpus
    for i in range(0, len(qs), fp.PER_KIND + 1):  # a query of every kind, alone: up to 64 items per pass
        s, d, n = run(ix, [qs[i]], 10)
        check(s, d, n, [want[i]], 10, f"alone {i}")


def test_both_fields_are_the_plain_phrase(native, corpus, on):
    """`name:"a b" text:"a b"` on k_fphrase against the plain `"a b"` on k_phrase: docs and score bits"""
    c, ix, ref, qs, want = corpus
    two = fp.queries()[fp.EQUAL]
    plain = [[fp.P(q[0][0], S)] for q in two]
    for k in (10, 1000):
        a, b = run(ix, two, k), run(ix, plain, k)
        assert np.array_equal(a[2], b[2]) and (b[2] > 0).all()
        for i in range(len(two)):
            m = int(a[2][i])
            assert fp.hits_of(a[0][i, :m], a[1][i, :m]) == fp.hits_of(b[0][i, :m], b[1][i, :m]), (k, i)


# ------------------------------------------------------------------ segments, rescored snapshots
@pytest.fixture(scope="module")
def segments(native, ctx, corpus):
    c, _, ref, qs, want = corpus
    cuts = list(fp.SEG_CUTS)
    g = None
    for lo, hi in zip(cuts, cuts[1:]):
        to, tt, _ = c.csr(c.text, c.text_gaps, lo, hi)
        no, nt, _ = c.csr(c.name, c.name_gaps, lo, hi)
        x = native.docs_stats(to, tt, fp.V_ALL, no, nt)
        g = x if g is None else g + x
    dele = c.deleted.astype(np.uint8)
    ixs = [build(native, ctx, c, lo, hi, deleted=dele[lo:hi], global_stats=g) for lo, hi in zip(cuts, cuts[1:])]
    assert [x.stats().has_name for x in ixs] == [True, False, True]  # the second: no name tokens at all
    swant = [ref.search(q, 1000, seg_bounds=cuts) for q in qs]
    return ixs, np.array(cuts[:-1], np.int64), swant


@pytest.mark.parametrize("k", [10, 1000])
def test_segments_equal_the_reference(native, ctx, corpus, segments, on, k):
    c, _, ref, qs, want = corpus
    ixs, base, swant = segments
    q_off, terms, occur, plen, ppos = fp.batch(qs)
    kw = dict(occur=occur, phrase_len=plen, phrase_pos=ppos)
    s, d, sh, n = native.search_sharded(ixs, q_off, terms, k, ctx=ctx, **kw)
    check(s, d.astype(np.int64) + base[sh], n, swant, k, "sharded")


def test_segments_as_a_multi_snapshot_plan(native, ctx, corpus, segments, on):
    c, _, ref, qs, want = corpus
    ixs, base, swant = segments
    k = 10  # (the host merge below is a Python loop)
    q_off, terms, occur, plen, ppos = fp.batch(qs)
    kw = dict(occur=occur, phrase_len=plen, phrase_pos=ppos)
    plan = native.Plan(ixs, q_off, terms, k, **kw)
    plan.execute()
    ps, pd, pn = plan.results()
    nq, S_ = len(q_off) - 1, len(ixs)
    es, ed, esh, en = merge_topk_numpy(ps.reshape(S_, nq, k), pd.reshape(S_, nq, k), pn.reshape(S_, nq), k)
    check(es, ed.astype(np.int64) + base[esh], en, swant, k, "multi-snapshot plan")


def test_clauses_absent_in_a_segment(native, ctx, corpus, segments, on):
    c, _, ref, qs, want = corpus
    ixs, base, swant = segments
    # a `name:` Must has no hit in the nameless segment; X_A is only in the last: the phrase is absent elsewhere
    q = [[fp.P([fp.E_2049, fp.E_B], M, NAME)], [fp.P([fp.X_A, fp.X_B], S, NAME), fp.P([fp.X_T, fp.X_B], S, TEXT)],
         [fp.P([fp.X_A, fp.X_B], M, NAME), fp.T(0, S)]]
    b = fp.batch(q)
    s, d, sh, n = native.search_sharded(ixs, b[0], b[1], 1000, ctx=ctx, occur=b[2], phrase_len=b[3], phrase_pos=b[4])
    assert int(n[0]) > 100 and 1 not in set(sh[0, :int(n[0])].tolist())
    assert int(n[1]) > 0 and set(sh[1, :int(n[1])].tolist()) == {2} == set(sh[2, :int(n[2])].tolist())
    check(s, d.astype(np.int64) + base[sh], n, [ref.search(x, 1000, seg_bounds=list(fp.SEG_CUTS)) for x in q], 1000, "absent")


@pytest.mark.parametrize("k", [10, 1000])
def test_rescored_snapshot(native, ctx, corpus, on, k):
    """statistics changed after the build: the weights and the tf caches are the new ones"""
    c, ix, ref, qs, _ = corpus
    r = np.random.default_rng(9)
    to, tt, _ = c.csr(c.text, c.text_gaps)
    no, nt, _ = c.csr(c.name, c.name_gaps)
    own = native.docs_stats(to, tt, fp.V_ALL, no, nt)
    other = native.ShardStats(7000, (90000, 5000), r.integers(0, 3000, fp.V_ALL).astype(np.uint32),
                              r.integers(0, 900, fp.V_ALL).astype(np.uint32))
    g = own + other
    dele = c.deleted.copy()
    dele[::11] ^= True
    rx = ix.rescore(g, deleted=dele.astype(np.uint8))
    st = pr.Stats(int(g.n_docs), tuple(int(x) for x in g.tot_tokens), np.asarray(g.df_text, np.int64),
                  np.asarray(g.df_name, np.int64))
    s, d, n = run(rx, qs, k)
    check(s, d, n, [ref.search(q, k, stats=st, deleted=dele) for q in qs], k, f"rescored k={k}")


# ------------------------------------------------------------------ mixed batches
def test_batch_mixes_the_shapes(native, ctx, corpus, fields, switch):
    c, ix, ref, qs, want = corpus
    r = np.random.default_rng(3)
    mixed, kind = [], []  # kind: the index in qs, or -1 (a row of a shape of before)
    for i in range(96):
        if i % 3 == 0:
            kind.append((i * 7) % len(qs))
            mixed.append(qs[kind[-1]])
            continue
        kind.append(-1)
        if i % 12 == 1:    # a lone plain phrase (k_phrase)
            mixed.append([fp.P([int(r.integers(0, 6)), int(r.integers(0, 6))], S)])
        elif i % 12 == 2:  # field-term queries (k_field)
            mixed.append([fp.T(int(r.integers(0, 56)), M, NAME), fp.T(int(r.integers(0, 56)), M, (TEXT, None)[i % 2])])
        else:              # single-term, AND and OR queries, some with an exclusion
            m = 1 if i % 9 == 1 else int(r.integers(2, 5))
            oc = [M if i % 2 else S] * m
            if m > 2 and i % 4 == 0:
                oc[-1] = X
            mixed.append([fp.T(int(r.integers(0, 56)), o) for o in oc])
    plain = [q for q, kd in zip(mixed, kind) if kd < 0]
    rows = [i for i, kd in enumerate(kind) if kd < 0]
    new = [i for i, kd in enumerate(kind) if kd >= 0]
    k = 100
    fields(1)
    assert switch(0) == 0
    off = run(ix, plain, k)
    with pytest.raises(native.Unsupported, match="field-qualified phrase|field clause beside a phrase clause"):
        run(ix, mixed, k)
    switch(1)
    alone, both = run(ix, plain, k), run(ix, mixed, k)
    switch(0)
    check(both[0][new], both[1][new], both[2][new], [want[kind[i]] for i in new], k, "mixed")
    for a in (alone, off):  # the rows of before: byte-identical without the new queries, and with the switch off
        assert np.array_equal(both[2][rows], a[2])
        for j, i in enumerate(rows):  # (a row's first n entries: the rest is not written)
            m = int(a[2][j])
            assert np.array_equal(both[1][i, :m], a[1][j, :m]), i
            assert np.array_equal(both[0][i, :m].view(np.uint32), a[0][j, :m].view(np.uint32)), i
    for j, q in enumerate(plain):  # and against the reference too
        rs, rd = ref.search(q, k)
        assert fp.hits_of(off[0][j, :int(off[2][j])], off[1][j, :int(off[2][j])]) == fp.hits_of(rs, rd), j
    assert (off[2] > 0).mean() > 0.5


# ------------------------------------------------------------------ the switch and the refusals
def test_switch_off_answers_as_today(native, corpus, fields, switch):
    c, ix, ref, qs, want = corpus
    assert switch() == 0 and fields() == 0
    q1, q2 = [fp.P([0, 1], S, NAME)], [fp.T(0, S, NAME), fp.P([0, 1], S)]
    for v in (0, 1):  # the new switch alone changes nothing
        switch(v)
        for q in (q1, q2):
            with pytest.raises(native.FuguError, match="query 0: bad phrase_len at term 0") as e:  # FG_EINVAL
                run(ix, [q], 10)
            assert e.value.code == native.FG_EINVAL and not isinstance(e.value, native.Unsupported)
    switch(0)
    fields(1)  # fg_field_clauses alone: the refusals of today
    with pytest.raises(native.Unsupported, match="query 0: field-qualified phrase"):
        run(ix, [q1], 10)
    with pytest.raises(native.Unsupported, match="query 0: field clause beside a phrase clause"):
        run(ix, [q2], 10)
    with pytest.raises(native.Unsupported, match="query 1: field-qualified phrase"):
        run(ix, [[fp.T(0, S)], [fp.P([0, 1, 2], M, TEXT), fp.T(3, M)]], 10)
    b = fp.batch([q1])
    kw = dict(occur=b[2], phrase_len=b[3], phrase_pos=b[4])
    with pytest.raises(native.Unsupported, match="field-qualified phrase"):
        native.Plan([ix, ix], b[0], b[1], 10, **kw)
    with pytest.raises(native.Unsupported, match="field clause in a count query"):
        native.count_batch([ix], b[0], b[1], **kw)
    with pytest.raises(native.Unsupported, match="does not cover field clauses"):
        ix.model(b[0], b[1], 10, phrase_len=b[3], phrase_pos=b[4])


def test_switch_and_refusals(native, ctx, corpus, fields, switch, others):
    c, ix, ref, qs, want = corpus
    fields(1)
    assert switch(1) == 0 and switch(-1) == 1
    s, d, n = run(ix, qs[:4], 10)
    check(s, d, n, want[:4], 10, "on")
    T_, N_, ANY, ALL = native.CLAUSE_TEXT, native.CLAUSE_NAME, native.CLAUSE_ANY, native.CLAUSE_ALL
    bad = lambda plen, ppos=None, terms=(6, 7, 8, 9): ix.search_batch(  # noqa: E731
        [0, len(terms)], list(terms), 10, occur=[S] * len(terms), phrase_len=plen,
        phrase_pos=ppos or [0, 1, 0, 0])
    q_off, terms, occur, plen, ppos = fp.batch([[fp.P([0, 1], S, NAME), fp.T(2, S)]])
    kw = dict(occur=occur, phrase_len=plen, phrase_pos=ppos)
    fo = np.arange(201, dtype=np.uint64)
    to, tt, _ = c.csr(c.text, c.text_gaps, 0, 200)
    no, nt, _ = c.csr(c.name, c.name_gaps, 0, 200)
    fx = native.Index.from_docs(ctx, to, tt, fp.V_ALL, no, nt, positions=True,
                                facets=(fo, np.zeros(200, np.uint32), 1))
    nopos = native.Index.from_docs(ctx, to, tt, fp.V_ALL, no, nt)
    for v in (0, 1):  # whatever the other six switches say
        others(v)
        with pytest.raises(native.FuguError, match="query 0: bad phrase_len at term 0") as e:  # both flags on one entry
            bad([2 | T_ | N_, 0, 1, 1])
        assert e.value.code == native.FG_EINVAL and not isinstance(e.value, native.Unsupported)
        with pytest.raises(native.FuguError, match="query 0: bad phrase_len at term 2") as e:  # past the query's end
            bad([1, 1, 3 | N_, 0], [0, 0, 0, 1])
        assert e.value.code == native.FG_EINVAL
        with pytest.raises(native.FuguError, match="phrase_len inside a phrase must be 0"):
            bad([3 | N_, 0, 1, 1], [0, 1, 2, 0])
        with pytest.raises(native.FuguError, match="a phrase's first offset must be 0"):
            bad([1, 2 | T_, 0, 1], [0, 1, 2, 0])
        with pytest.raises(native.FuguError, match="phrase offsets must increase"):
            bad([2 | T_, 0, 1, 1], [0, 0, 0, 0])
        for plen_ in ([2 | ANY | N_, 0, 1, 1], [1, 1, 2 | ALL | T_, 0]):  # together with ANY / ALL
            with pytest.raises(native.Unsupported, match="field-qualified group"):
                bad(plen_)
        with pytest.raises(native.Unsupported, match="field clause with facet filters"):
            fx.search_batch(q_off, terms, 10, f_off=[0, 1], f_terms=[0], **kw)
        assert int(fx.search_batch(q_off, terms, 10, **kw)[2][0]) > 0
        with pytest.raises(native.Unsupported, match="snapshot built without positions"):
            nopos.search_batch(q_off, terms, 10, **kw)
        with pytest.raises(native.Unsupported, match="snapshot built without positions"):
            native.search_sharded([fx, nopos], q_off, terms, 10, **kw)
        with pytest.raises(native.Unsupported, match="field clause in a count query"):
            native.count_batch([ix], q_off, terms, **kw)
        with pytest.raises(native.Unsupported, match="does not cover field clauses"):
            ix.model(q_off, terms, 10, phrase_len=plen, phrase_pos=ppos)
    # with fg_group_clauses on (the flags parse): a field flag on a group's member row, a group anywhere in such a query
    with pytest.raises(native.Unsupported, match="field-qualified group"):
        bad([2 | ANY, N_, 1, 1], [0, 0, 0, 0])
    with pytest.raises(native.Unsupported, match="field-qualified phrase beside a group clause"):
        bad([2 | N_, 0, 2 | ANY, 0], [0, 1, 0, 0])
    with pytest.raises(native.Unsupported, match="field clause beside a group clause"):
        bad([2 | ALL, 0, 1 | T_, 1], [0, 0, 0, 0], terms=(6, 7, 8, 9))
    with pytest.raises(native.Unsupported, match="field clause beside a group clause"):
        ix.search_batch([0, 5], [6, 7, 8, 9, 10], 10, occur=[S] * 5, phrase_len=[1 | N_, 2, 0, 2 | ANY, 0],
                        phrase_pos=[0, 0, 1, 0, 0])
    others(0)
    with pytest.raises(native.Unsupported, match="terms"):  # 17 terms: the existing check and message
        run(ix, [[fp.P([0, 1], S, NAME)] + [fp.T(t, S) for t in range(6, 21)]], 10)
    q16 = [fp.P([0, 1], S, NAME), fp.P([1, 2, 0], S, TEXT)] + [fp.T(t, S, (NAME, TEXT, None)[t % 3]) for t in range(6, 17)]
    s, d, n = run(ix, [q16], 10)  # 16: within FG_MAX_TERMS
    check(s, d, n, [ref.search(q16, 10)], 10, "16 terms")
    assert switch(0) == 1
    with pytest.raises(native.Unsupported, match="field-qualified phrase"):  # today's answer again
        run(ix, qs[:1], 10)


# ------------------------------------------------------------------ fg_db
DB_DOCS = [
    ("d0", "the annual report is out", "Annual Report 2024"), ("d1", "annual budget and report", "budget annual"),
    ("d2", "send an e-mail to user@example.com", "e-mail policy"), ("d3", "q3 report budget", "Q3 Report"),
    ("d4", "budget only", "q3 report draft"), ("d5", "mail e reversed", "mail e"),
    ("d6", "annual report annual report", None), ("d7", "report e-mail", "report"),
    ("d8", "user example com", "user@example.com"), ("d9", "nothing", "annual report annual report"),
    ("d10", "budget q3", None), ("d11", "e-mail", "the report"),
]
DB_QUERIES = [  # (query, its clauses over words, the docs that hit)
    ('name:"annual report"', [(["annual", "report"], S, NAME)], {0, 9}),
    ("name:e-mail", [(["e", "mail"], S, NAME)], {2}),
    ("text:user@example.com", [(["user", "example", "com"], S, TEXT)], {2, 8}),
    ('+name:"q3 report" +budget', [(["q3", "report"], M, NAME), (["budget"], M, None)], {3, 4}),
    ("name:report e-mail", [(["report"], S, NAME), (["e", "mail"], S, None)], {0, 2, 3, 4, 7, 9, 11}),
    ('name:"annual report" text:"annual report"', [(["annual", "report"], S, NAME), (["annual", "report"], S, TEXT)],
     {0, 6, 9}),
    ('budget -name:"q3 report"', [(["budget"], S, None), (["q3", "report"], X, NAME)], {1, 10}),
    ('+text:"annual report" name:"annual report"', [(["annual", "report"], M, TEXT), (["annual", "report"], S, NAME)],
     {0, 6}),
    ('+name:"missing words" budget', [(["missing", "words"], M, NAME), (["budget"], S, None)], set()),
]


def db_reference(d, ns):
    """the reference's hit lists [(score, global doc)] of DB_QUERIES over the namespace's current segments"""
    from test_gpu_phrase import py_tokens
    segs = d.segments(ns)
    keep = [g for seg in segs for g in seg]
    info = d.merge_info(ns)
    vocab = {}
    tt, tg, nt, ng = [], [], [], []
    for g in keep:
        for src, dst, dg in ((DB_DOCS[g][1], tt, tg), (DB_DOCS[g][2] or "", nt, ng)):
            toks, gaps = py_tokens(src)
            dst.append([vocab.setdefault(w, len(vocab)) for w in toks])
            dg.append(gaps or None)
    ref = fp.Ref(len(vocab), tt, tg, nt, ng)
    assert ref.pstats.n == info["n_docs_stats"]
    ref.pstats.tot = tuple(info["tot_tokens"])  # the namespace's totals
    bounds = np.cumsum([0] + [len(s) for s in segs])
    out = []
    for _, cl, _ in DB_QUERIES:
        q = [fp.P([vocab.get(w, fp.MISSING) for w in ws], oc, f) for ws, oc, f in cl]
        s, dd = ref.search(q, 20, seg_bounds=bounds)
        out.append([(np.float32(x), keep[int(y)]) for x, y in zip(s, dd)])
    return out


def test_db_search_and_json(native, ctx, fields, switch):
    from fugu_amd import db
    d = db.Database(ctx)
    ns = "fphr"
    d.create_namespace(ns)
    for i, (rid, text, nm) in enumerate(DB_DOCS):
        d.upsert(db.ObjectRecord(rid, text, metadata={"name": nm} if nm else None), ns)
        if i in (3, 7, 11):  # three commits: three segments (until the merger joins them)
            d.commit(ns)
    d.merge_wait(ns)
    assert switch() == 0 and fields() == 0
    fields(1)
    for q, _, _ in DB_QUERIES:  # refused with the new switch off, as today
        with pytest.raises(native.Unsupported, match="field-qualified phrase|field clause beside a phrase clause"):
            d.search(ns, q)
        with pytest.raises(native.Unsupported):
            d.search_json(ns, q)
    switch(1)
    got = [d.search(ns, q, per_page=20) for q, _, _ in DB_QUERIES]
    want = db_reference(d, ns)
    for q, g, w in zip(DB_QUERIES, got, want):
        assert [x for _, x in g] == [x for _, x in w], (q[0], g, w)
        assert [np.float32(s).view(np.uint32) for s, _ in g] == [s.view(np.uint32) for s, _ in w], (q[0], g, w)
        assert {x for _, x in g} == q[2], (q[0], g)
    plain = d.search(ns, '"annual report"', per_page=20)
    assert [(np.float32(s).view(np.uint32), g) for s, g in got[5]] == [(np.float32(s).view(np.uint32), g) for s, g in plain]
    for (q, _, _), r in zip(DB_QUERIES, got):
        js = json.loads(d.search_json(ns, q, per_page=20))
        assert [x["id"] for x in js["results"]] == [DB_DOCS[g][0] for _, g in r]
        assert np.allclose([x["score"] for x in js["results"]], [x for x, _ in r], rtol=1e-6, atol=0)
    with pytest.raises(native.Unsupported, match="field clause in a count query"):
        d.facet_counts(ns, "/", 'name:"annual report"')
    with pytest.raises(native.Unsupported, match="field-qualified group"):
        d.search(ns, 'name:("annual report" budget)')
    with pytest.raises(native.Unsupported, match="slop, prefix, boost"):
        d.search(ns, 'name:"annual report"~2')
    with pytest.raises(native.Unsupported, match=r"field outside \[text, name\]"):
        d.search(ns, 'id:"annual report"')
    switch(0)
    with pytest.raises(native.Unsupported, match="field-qualified phrase"):  # the same process, off again
        d.search(ns, 'name:"annual report"')
