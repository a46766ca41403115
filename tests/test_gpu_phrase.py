"""Phrase queries on the device (k_phrase) against the numpy
reference tests/phrase_ref.py: doc ids and order exact, scores within 1e-5
relative (the known-answer corpus bit for bit).

- one index: the known-answer corpus, then 6000 docs (names, deletions, dropped
  tokens) x 256 phrases at k = 1, 10, 1000;
- the same corpus as 3 segments under global statistics, one of them built
  under its own statistics and rescored with a changed `deleted`: single- and
  multi-snapshot plans, fg_search_sharded, and a batch mixing phrases with AND /
  OR term queries;
- fg_db: hyphenated words, quoted phrases, a dropped long token, a merge, a
  replaced doc, through fg_db_search and the JSON handler;
- what stays FG_EUNSUPPORTED / FG_EINVAL.
test_phrase_ref.py checks, without a GPU, that the corpus and queries used
here exercise what they are meant to (hits, long lead lists, every query kind).
"""
import json
import re

import numpy as np
import pytest

import phrase_ref as pr
from shard_ref import merge_topk_numpy

pytestmark = pytest.mark.gpu
RTOL = 1e-5


@pytest.fixture(scope="module")
def native():
    from fugu_amd import native as nat
    if nat.device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    return nat


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context((0,))


def check(s, d, n, want, k, tag=""):
    """device rows (s, d, n) against the reference lists `want` [(scores, docs)] cut at k"""
    for i, (rs, rd) in enumerate(want):
        rs, rd = rs[:k], rd[:k]
        m = int(n[i])
        assert m == len(rd), (tag, i, m, len(rd))
        assert np.array_equal(d[i, :m].astype(np.int64), rd.astype(np.int64)), (tag, i)
        assert np.allclose(s[i, :m], rs, rtol=RTOL, atol=0), (tag, i)


# ------------------------------------------------------------------ known answer
def test_known_answer_bit_for_bit(native, ctx):
    docs = pr.kat_corpus()
    off = np.cumsum([0] + [len(x) for x in docs]).astype(np.uint64)
    tok = np.concatenate(docs).astype(np.uint32)
    ix = native.Index.from_docs(ctx, off, tok, 5, positions=True)
    assert ix.stats().has_positions
    text = pr.Field(docs)
    st = pr.Stats.of(text, None, 5)
    qs = [[0, 1], [1, 2], [0, 0]]
    s, d, n = ix.search_batch([0, 2, 4, 6], [t for q in qs for t in q], 10, phrase_len=[2, 0] * 3,
                              phrase_pos=[0, 1] * 3)
    for i, q in enumerate(qs):
        rs, rd, _ = pr.search(text, None, st, q, [0, 1], 10)
        m = int(n[i])
        assert d[i, :m].tolist() == rd.tolist(), (q, d[i, :m], rd)
        assert s[i, :m].view(np.uint32).tolist() == rs.view(np.uint32).tolist(), (q, s[i, :m], rs)
    # Must and Should phrases are the same query; a MustNot phrase alone has no hits
    for oc, hits in ((native.OCCUR_SHOULD, 2), (native.OCCUR_MUST_NOT, 0)):
        _, _, n1 = ix.search_batch([0, 2], [0, 1], 10, occur=[oc, oc], phrase_len=[2, 0], phrase_pos=[0, 1])
        assert int(n1[0]) == hits


# ------------------------------------------------------------------ 6000 docs
@pytest.fixture(scope="module")
def corpus(native, ctx):
    c = pr.Synth()
    text, name = pr.Field(c.text, c.text_gaps), pr.Field(c.name, c.name_gaps)
    st = pr.Stats.of(text, name, pr.V)
    to, tt, tg = c.csr(c.text, c.text_gaps)
    no, nt, ng = c.csr(c.name, c.name_gaps)
    ix = native.Index.from_docs(ctx, to, tt, pr.V, no, nt, deleted=c.deleted, positions=True, text_gaps=tg,
                                name_gaps=ng)
    want = [pr.search(text, name, st, t, o, 1000, deleted=c.deleted)[:2] for t, o in c.queries]
    return c, ix, want, (text, name, st)


@pytest.mark.parametrize("k", [1, 10, 1000])
def test_corpus_matches_reference(native, corpus, k):
    c, ix, want, _ = corpus
    s, d, n = ix.search_batch(*c.batch()[:2], k, phrase_len=c.batch()[2], phrase_pos=c.batch()[3])
    check(s, d, n, want, k, f"k={k}")
    assert (n > 0).mean() >= 0.75


def test_forward_index_is_counted(native, ctx, corpus):
    c, ix, _, _ = corpus
    to, tt, tg = c.csr(c.text, c.text_gaps)
    no, nt, ng = c.csr(c.name, c.name_gaps)
    plain = native.Index.from_docs(ctx, to, tt, pr.V, no, nt, deleted=c.deleted)
    a, b = ix.stats(), plain.stats()
    assert a.has_positions and not b.has_positions
    fwd = 4 * (len(tt) + len(tg) + len(nt) + len(ng)) + 2 * 8 * (c.n + 1)
    assert fwd <= a.device_bytes - b.device_bytes <= fwd + 4 * 512  # (allocation rounding)
    # everything else is as without positions: gaps count nowhere
    assert (a.n_postings, a.tot_tokens, a.avgdl) == (b.n_postings, b.tot_tokens, b.avgdl)


# ------------------------------------------------------------------ segments, rescores, mixed batches
@pytest.fixture(scope="module")
def segments(native, ctx, corpus):
    c, ix, _, (text, name, st) = corpus
    cuts = [0, 1700, 4300, c.n]
    parts, g = [], None
    for lo, hi in zip(cuts, cuts[1:]):
        to, tt, tg = c.csr(c.text, c.text_gaps, lo, hi)
        no, nt, ng = c.csr(c.name, c.name_gaps, lo, hi)
        parts.append((to, tt, tg, no, nt, ng))
        x = native.docs_stats(to, tt, pr.V, no, nt)
        g = x if g is None else g + x
    assert (g.n_docs, tuple(g.tot_tokens)) == (st.n, st.tot) and np.array_equal(g.df_text, st.df_text)
    dele = c.deleted.copy()
    dele[cuts[1]:cuts[2]:7] = ~dele[cuts[1]:cuts[2]:7]  # the middle segment's deletions change after its build
    ixs = []
    for s_, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        to, tt, tg, no, nt, ng = parts[s_]
        kw = dict(positions=True, text_gaps=tg, name_gaps=ng)
        if s_ == 1:  # built under its OWN statistics and the old deletions, then rescored: query-time statistics
            own = native.Index.from_docs(ctx, to, tt, pr.V, no, nt, deleted=c.deleted[lo:hi], **kw)
            ixs.append(own.rescore(g, deleted=dele[lo:hi]))
            assert ixs[-1].stats().has_positions
        else:
            ixs.append(native.Index.from_docs(ctx, to, tt, pr.V, no, nt, deleted=dele[lo:hi], global_stats=g, **kw))
    want = [pr.search(text, name, st, t, o, 1000, deleted=dele)[:2] for t, o in c.queries]
    return c, ixs, np.array(cuts[:-1], np.int64), want


@pytest.mark.parametrize("k", [10, 1000])
def test_segments_equal_one_index(native, ctx, segments, k):
    c, ixs, base, want = segments
    q_off, terms, plen, ppos = c.batch()
    # fg_search_sharded: one multi-snapshot plan, the merged select
    s, d, sh, n = native.search_sharded(ixs, q_off, terms, k, ctx=ctx, phrase_len=plen, phrase_pos=ppos)
    gd = d.astype(np.int64) + base[sh]
    check(s, gd, n, want, k, "sharded")
    # single-snapshot plans, merged on the host (the small k: the merge is a Python loop)
    per = [ix.search_batch(q_off, terms, k, phrase_len=plen, phrase_pos=ppos) for ix in ixs]
    if k == 10:
        es, ed, esh, en = merge_topk_numpy(np.stack([p[0] for p in per]), np.stack([p[1] for p in per]),
                                           np.stack([p[2] for p in per]), k)
        check(es, ed.astype(np.int64) + base[esh], en, want, k, "single plans")
    # a multi-snapshot plan's per-slot lists (the slots of a query share its threshold, so
    # a slot may keep fewer than k) merge to the same result
    plan = native.Plan(ixs, q_off, terms, k, phrase_len=plen, phrase_pos=ppos)
    plan.execute()
    ps, pd, pn = plan.results()
    nq, S = len(q_off) - 1, len(ixs)
    if k == 10:
        es, ed, esh, en = merge_topk_numpy(ps.reshape(S, nq, k), pd.reshape(S, nq, k), pn.reshape(S, nq), k)
        check(es, ed.astype(np.int64) + base[esh], en, want, k, "multi-snapshot plan")
    assert np.array_equal(np.minimum(pn.reshape(S, nq).sum(0), k), n)


def test_batch_mixes_phrases_and_term_queries(native, ctx, corpus, segments):
    c, ix, want, _ = corpus
    _, ixs, base, swant = segments
    r = np.random.default_rng(3)
    M, S, X = native.OCCUR_MUST, native.OCCUR_SHOULD, native.OCCUR_MUST_NOT
    qs, kinds = [], []  # (terms, occur, phrase_len, phrase_pos)
    for i in range(96):
        if i % 3 == 0:
            t, o = c.queries[(i * 5) % 256]
            qs.append((t, [M if i % 2 else S] * len(t), [len(t)] + [0] * (len(t) - 1), o))
            kinds.append((i * 5) % 256)
        else:
            m = int(r.integers(1, 5))
            t = [int(x) for x in r.integers(0, pr.V_TEXT, m)]
            oc = [M] * m if i % 3 == 1 else [S] * m
            if m > 2 and i % 4 == 0:
                oc[-1] = X
            qs.append((t, oc, [1] * m, [0] * m))
            kinds.append(-1)
    q_off = np.cumsum([0] + [len(q[0]) for q in qs]).astype(np.uint32)
    cat = lambda j: np.array([x for q in qs for x in q[j]])  # noqa: E731
    k = 100
    tq = [i for i, kd in enumerate(kinds) if kd < 0]
    t_off = np.cumsum([0] + [len(qs[i][0]) for i in tq]).astype(np.uint32)
    t_terms = np.array([x for i in tq for x in qs[i][0]], np.uint32)
    t_occ = np.array([x for i in tq for x in qs[i][1]], np.uint8)
    for tag, run, alone, ref in (
            ("one index", lambda *a, **kw: ix.search_batch(*a, **kw), None, want),
            ("segments", lambda *a, **kw: native.search_sharded(ixs, *a, ctx=ctx, **kw), None, swant)):
        out = run(q_off, cat(0), k, occur=cat(1), phrase_len=cat(2), phrase_pos=cat(3))
        solo = run(t_off, t_terms, k, occur=t_occ)
        s, d, n = out[0], out[1], out[-1]
        if tag == "segments":
            d = d.astype(np.int64) + base[out[2]]
        check(s[[i for i, kd in enumerate(kinds) if kd >= 0]], d[[i for i, kd in enumerate(kinds) if kd >= 0]],
              n[[i for i, kd in enumerate(kinds) if kd >= 0]], [ref[kd] for kd in kinds if kd >= 0], k, tag)
        sd = solo[1] if tag == "one index" else solo[1].astype(np.int64) + base[solo[2]]
        for j, i in enumerate(tq):  # the term queries: exactly what the batch without phrases returns
            m = int(solo[-1][j])
            assert int(n[i]) == m, (tag, i)
            assert np.array_equal(d[i, :m], sd[j, :m]) and np.array_equal(s[i, :m], solo[0][j, :m]), (tag, i)
        assert sum(int(solo[-1][j]) > 0 for j in range(len(tq))) > len(tq) // 2


# ------------------------------------------------------------------ fg_db
def py_tokens(text):
    """(tokens, gaps) of the default analyzer on ASCII text"""
    toks, gaps = [], []
    for w in re.findall(r"[0-9A-Za-z]+", text):
        if len(w) >= 40:
            gaps.append(len(toks))
        else:
            toks.append(w.lower())
    return toks, gaps


LONG = "x" * 45
DOCS = [
    ("d0", "send me an e-mail about the e-mail server", None),
    ("d1", "mail e then nothing", None),
    ("d2", "a state-of-the-art index in New York", "New York guide"),
    ("d3", "york new and the art of state", None),
    ("d4", f"alpha {LONG} beta", None),
    ("d5", "alpha beta gamma", None),
    ("d6", "e mail e mail e mail", "new york new york"),
    ("d7", "nothing here", "state of the art"),
    ("d8", "the last one mentions e-mail once", None),
]
QUERIES = [("e-mail", ["e", "mail"], [0, 1]), ('"new york"', ["new", "york"], [0, 1]),
           ('"alpha beta"', ["alpha", "beta"], [0, 1]), ("state-of-the-art", ["state", "of", "the", "art"], [0, 1, 2, 3]),
           (f'"alpha {LONG} beta"', ["alpha", "beta"], [0, 2]), ('+"E-Mail server"', ["e", "mail", "server"], [0, 1, 2])]


def db_reference(d, ns, docs, deleted):
    """the reference's hit lists [(score, global doc)] of QUERIES over the namespace's current segments"""
    keep = [g for seg in d.segments(ns) for g in seg]
    info = d.merge_info(ns)
    vocab = {}
    tt, tg, nt, ng = [], [], [], []
    for g in keep:
        for src, dst, dg in ((docs[g][1], tt, tg), (docs[g][2] or "", nt, ng)):
            toks, gaps = py_tokens(src)
            dst.append([vocab.setdefault(w, len(vocab)) for w in toks])
            dg.append(gaps or None)
    text, name = pr.Field(tt, tg), pr.Field(nt, ng)
    st = pr.Stats.of(text, name, len(vocab))
    assert st.n == info["n_docs_stats"]
    st.tot = tuple(info["tot_tokens"])  # (a merge that drops deleted docs re-derives the totals: test_host.py)
    dele = np.array([deleted[g] for g in keep], bool)
    out = []
    for _, words, offs in QUERIES:
        s, dd, _ = pr.search(text, name, st, [vocab.get(w, 0xFFFFFFFF) for w in words], offs, 20, deleted=dele)
        out.append([(float(x), keep[int(y)]) for x, y in zip(s, dd)])
    return out


def db_results(d, ns):
    return [d.search(ns, q, per_page=20) for q, _, _ in QUERIES]


def same(got, want):
    assert [[g for _, g in r] for r in got] == [[g for _, g in r] for r in want], (got, want)
    for a, b in zip(got, want):
        assert np.allclose([x for x, _ in a], [x for x, _ in b], rtol=RTOL, atol=0)


def test_db_phrases_commits_merge_and_replace(native, ctx):
    from fugu_amd import db
    d = db.Database(ctx)
    ns = "phr"
    d.create_namespace(ns)
    deleted = [False] * len(DOCS)
    for i, (rid, text, nm) in enumerate(DOCS):  # 9 commits, one segment each: the merger runs
        d.upsert(db.ObjectRecord(rid, text, metadata={"name": nm} if nm else None), ns)
        d.commit(ns)
        if i == 5:
            first = db_results(d, ns)
            same(first, db_reference(d, ns, DOCS, deleted))
    d.merge_wait(ns)
    assert d.merge_info(ns)["merges"] >= 1
    got = db_results(d, ns)
    want = db_reference(d, ns, DOCS, deleted)
    same(got, want)
    docs_of = lambda r: [g for _, g in r]  # noqa: E731
    assert set(docs_of(got[0])) == {0, 6, 8} and set(docs_of(got[1])) == {2, 6}
    assert docs_of(got[2]) == [5] and docs_of(got[4]) == [4] and set(docs_of(got[3])) == {2, 7}
    assert docs_of(got[5]) == [0]
    js = json.loads(d.search_json(ns, "e-mail", per_page=20))
    assert [r["id"] for r in js["results"]] == [DOCS[g][0] for g in docs_of(got[0])]
    assert np.allclose([r["score"] for r in js["results"]], [x for x, _ in got[0]], rtol=RTOL, atol=0)
    # a replacement without the phrase removes the old hit
    docs = DOCS + [("d8", "the last one mentions mail once", None)]
    deleted = deleted + [False]
    deleted[8] = True
    d.upsert(db.ObjectRecord("d8", docs[-1][1]), ns)
    d.commit(ns)
    d.merge_wait(ns)
    got = db_results(d, ns)
    same(got, db_reference(d, ns, docs, deleted))
    assert set(docs_of(got[0])) == {0, 6}
    # outside the subset: the handler reports the reason
    for q, why in (("e-mail server", "phrase clause beside other clauses"),):
        with pytest.raises(native.Unsupported, match=why):
            d.search(ns, q)
    with pytest.raises(native.Unsupported, match="phrase with facet filters"):
        d.search(ns, "e-mail", filters=["/metadata/name"])


# ------------------------------------------------------------------ refusals
def test_refusals(native, ctx, corpus):
    c, ix, _, _ = corpus
    with pytest.raises(native.Unsupported, match="phrase clause beside other clauses"):
        ix.search_batch([0, 3], [0, 1, 2], 10, phrase_len=[2, 0, 1], phrase_pos=[0, 1, 0])
    to, tt, _ = c.csr(c.text, c.text_gaps, 0, 200)
    fo = np.arange(201, dtype=np.uint64)
    fx = native.Index.from_docs(ctx, to, tt, pr.V, positions=True, facets=(fo, np.zeros(200, np.uint32), 1))
    with pytest.raises(native.Unsupported, match="phrase with facet filters"):
        fx.search_batch([0, 2], [0, 1], 10, f_off=[0, 1], f_terms=[0], phrase_len=[2, 0], phrase_pos=[0, 1])
    assert int(fx.search_batch([0, 2], [0, 1], 10, phrase_len=[2, 0], phrase_pos=[0, 1])[2][0]) > 0
    plain = native.Index.from_docs(ctx, to, tt, pr.V)
    with pytest.raises(native.Unsupported, match="snapshot built without positions"):
        plain.search_batch([0, 2], [0, 1], 10, phrase_len=[2, 0], phrase_pos=[0, 1])
    with pytest.raises(native.Unsupported, match="snapshot built without positions"):
        native.search_sharded([fx, plain], [0, 2], [0, 1], 10, phrase_len=[2, 0], phrase_pos=[0, 1])
    # phrase_len of all ones is today's batch, positions or not
    a = plain.search_batch([0, 2], [0, 1], 10, phrase_len=[1, 1], phrase_pos=[0, 0])
    b = plain.search_batch([0, 2], [0, 1], 10)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
    with pytest.raises(native.Unsupported):
        ix.search_batch([0, 17], [0] * 17, 10, phrase_len=[17] + [0] * 16, phrase_pos=list(range(17)))
    for bad_len, bad_pos in (([2, 1], [0, 1]), ([3, 0], [0, 1]), ([2, 0], [0, 0]), ([2, 0], [1, 2]), ([0, 2], [0, 1])):
        with pytest.raises(native.FuguError) as e:
            ix.search_batch([0, 2], [0, 1], 10, phrase_len=bad_len, phrase_pos=bad_pos)
        assert e.value.code == native.FG_EINVAL, (bad_len, bad_pos)
    with pytest.raises(native.FuguError) as e:
        ix.model([0, 2], [0, 1], 10, phrase_len=[2, 0], phrase_pos=[0, 1])
    assert e.value.code == native.FG_EINVAL
