"""fg_count_batch on the device against tests/count_ref.py (exact equality: the
outputs are integers): hit totals and facet counts of every query kind over one
snapshot, over the same docs as three snapshots (one with its own term
dictionary, one rescored with changed deletions), through several query slices,
on indexes of 31 and 64 docs, under every probe structure, through fg_db's
facet_counts / facet_tree / facets_json (three commits, and a merged segment), the refusals, and beside searches on
other threads."""
import json
import os
import threading

import numpy as np
import pytest

import count_ref as cr

pytestmark = pytest.mark.gpu

RANK_ENVS = [{"FUGU_RANK_GIB": "0"}, {"FUGU_RANK_GIB": "0.02", "FUGU_RANK_PLAIN_DIV": "16384"},
             {"FUGU_RANK_PLAIN_DIV": "16384"}, {"FUGU_RANK_PLAIN_DIV": "1"},
             {"FUGU_RANK_GIB": "0.05", "FUGU_RANK_PLAIN_DIV": "16"}]
RANK_IDS = ["directory_only", "few_rank_terms", "plain_rank_only", "sparse_rank_only", "all_kinds"]


@pytest.fixture(scope="module")
def native():
    from fugu_amd import native as nat
    if nat.device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    return nat


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context((0,))


@pytest.fixture(scope="module")
def main():
    """(corpus, labelled queries, batch arrays, count terms as ids, reference total, reference count)"""
    c = cr.main_corpus()
    qs = cr.query_batch(c)
    plain = [(cl, fl) for _, cl, fl in qs]
    cts = list(range(len(c.fdict))) + [None]  # every facet term of the dictionary and one missing id
    total, count = cr.count_batch(c, plain, cts)
    ct_ids = np.array([0xFFFFFFFF if t is None else t for t in cts], np.uint32)
    return c, qs, cr.batch_arrays(plain), ct_ids, total, count


def build(native, ctx, c, n_terms=None, deleted="own"):
    to, tt, no, nt, facets = c.csr()
    dl = c.deleted if isinstance(deleted, str) else deleted
    return native.Index.from_docs(ctx, to, tt, n_terms or c.n_terms, name_off=no, name_tok=nt, deleted=dl, threads=8,
                                  facets=facets)


def run(native, ixs, arrays, ct_ids):
    q_off, terms, occur, f_off, f_terms = arrays
    return native.count_batch(ixs, q_off, terms, ct_ids, f_off=f_off, f_terms=f_terms, occur=occur)


def same(got, want_total, want_count, labels, what):
    total, count = got
    assert total.dtype == np.uint64 and count.dtype == np.uint64
    bad = [(labels[i][0], int(total[i]), int(want_total[i])) for i in np.nonzero(total != want_total)[0]]
    assert not bad, (what, bad)
    bad = [(labels[i][0], int(j), int(count[i, j]), int(want_count[i, j])) for i, j in zip(*np.nonzero(count != want_count))]
    assert not bad, (what, bad[:10])


@pytest.fixture(scope="module")
def main_index(native, ctx, main):
    return build(native, ctx, main[0])


def test_single_snapshot(native, main, main_index):
    c, qs, arrays, ct_ids, total, count = main
    same(run(native, [main_index], arrays, ct_ids), total, count, qs, "one snapshot")
    # n_count == 0: out_count is NULL
    t0, c0 = run(native, [main_index], arrays, np.zeros(0, np.uint32))
    assert np.array_equal(t0, total) and c0.shape == (len(qs), 0)
    # an empty batch
    e = np.zeros(1, np.uint32)
    t1, c1 = native.count_batch([main_index], e, np.zeros(0, np.uint32), ct_ids)
    assert t1.shape == (0,) and c1.shape == (0, len(ct_ids))


def test_three_snapshots(native, ctx, main):
    """the same docs as three segments of the namespace: totals and counts are summed"""
    c, qs, arrays, ct_ids, total, count = main
    a, b = 15001, 24010
    ca, cb, cc = c.slice(0, a), c.slice(a, b), c.slice(b, c.n)
    ia = build(native, ctx, ca)
    # its own term dictionary: the docs hold fewer than a quarter of the vocabulary it is given
    big_vocab = 1024
    assert len({t for d in range(cb.n) for t in cb.text[d] + (cb.name[d] or [])}) * 4 < big_vocab
    ib = build(native, ctx, cb, n_terms=big_vocab)
    # built with no deletions, then rescored with the segment's deletions
    to, tt, no, nt, facets = cc.csr()
    base = build(native, ctx, cc, deleted=None)
    assert int(run(native, [base], arrays, ct_ids)[0][0]) == cc.n  # AllQuery before the deletions
    g = native.docs_stats(to, tt, cc.n_terms, name_off=no, name_tok=nt, threads=8, facets=facets)
    ic = base.rescore(g, deleted=cc.deleted)
    same(run(native, [ia, ib, ic], arrays, ct_ids), total, count, qs, "three snapshots")
    # each segment alone equals the reference over its own docs
    plain = [(cl, fl) for _, cl, fl in qs]
    cts = [None if t == 0xFFFFFFFF else int(t) for t in ct_ids]
    for ix, seg, what in ((ib, cb, "own dictionary"), (ic, cc, "rescored")):
        st, sc = cr.count_batch(seg, plain, cts)
        same(run(native, [ix], arrays, ct_ids), st, sc, qs, what)
    for x in (ia, ib, ic, base):
        x.close()


@pytest.mark.parametrize("kb", ["4", "11", "60"])
def test_query_slices(native, main, main_index, kb):
    """FUGU_COUNT_WS_KB shrinks the bound on a pass's match bitmaps (ceil(40037 / 32)
    words = 5008 B per query): 1, 2 and 12 queries per slice"""
    c, qs, arrays, ct_ids, total, count = main
    old = os.environ.get("FUGU_COUNT_WS_KB")
    os.environ["FUGU_COUNT_WS_KB"] = kb
    try:
        got = run(native, [main_index], arrays, ct_ids)
    finally:
        if old is None:
            os.environ.pop("FUGU_COUNT_WS_KB", None)
        else:
            os.environ["FUGU_COUNT_WS_KB"] = old
    same(got, total, count, qs, f"slices of {kb} KiB")


@pytest.mark.parametrize("n", [31, 64, 33])
def test_edge_indexes(native, ctx, n):
    """a single partial bitmap word, the exact word boundary, one bit into the second word"""
    c = cr._corpus(n, 5 + n, 7)
    c.deleted[n - 1] = 0  # the last doc of the last word stays alive
    c = cr.Corpus(c.text, c.name, c.facets, c.deleted, c.n_terms)
    qs = cr.query_batch(c)
    plain = [(cl, fl) for _, cl, fl in qs]
    cts = list(range(len(c.fdict))) + [None]
    total, count = cr.count_batch(c, plain, cts)
    assert total[0] == len(c.alive) > 0
    ix = build(native, ctx, c)
    ct_ids = np.array([0xFFFFFFFF if t is None else t for t in cts], np.uint32)
    same(run(native, [ix], cr.batch_arrays(plain), ct_ids), total, count, qs, n)
    ix.close()


@pytest.mark.parametrize("env", RANK_ENVS, ids=RANK_IDS)
def test_probe_paths(native, ctx, main, env):
    """the main check with every probe structure term_has_doc reads: the bucket
    directory alone, plain rank words, sparse rank words, and mixtures"""
    c, qs, arrays, ct_ids, total, count = main
    old = {k: os.environ.get(k) for k in ("FUGU_RANK_GIB", "FUGU_RANK_PLAIN_DIV")}
    os.environ.update(env)
    try:
        ix = build(native, ctx, c)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    st = ix.stats()
    print(env, "rank terms", st.n_rank_terms, "sparse", st.n_sparse_rank_terms)
    if env.get("FUGU_RANK_GIB") == "0":
        assert st.n_rank_terms == 0
    else:
        assert st.n_rank_terms > 0
    if env.get("FUGU_RANK_PLAIN_DIV") == "16384":
        assert st.n_sparse_rank_terms == 0
    if env.get("FUGU_RANK_PLAIN_DIV") == "1":
        assert st.n_sparse_rank_terms > 0
    same(run(native, [ix], arrays, ct_ids), total, count, qs, env)
    ix.close()


# ---------------------------------------------------------------- fg_db
WORDS = ["alpha", "beta", "gamma", "delta", "epsilon", "zeta"]


def db_docs():
    """[(commit, id, text, name or None, facets)]: three commits; d3 and d17 are
    replaced in a later commit (their first versions stay as deleted docs of the
    older segments), d8 twice"""
    rng = np.random.RandomState(9)
    docs = []
    for i in range(60):
        words = [WORDS[int(w)] for w in rng.randint(0, len(WORDS), int(rng.randint(1, 6)))]
        fl = []
        if i % 7 != 0:
            fl.append(f"/org/{i % 4}" + (f"/team/{i % 3}" if i % 5 else ""))
        if i % 3 == 0:
            fl.append("/kind/" + "ab"[i % 2])
        if i % 4 == 1:
            fl.append("/namespace/docs/organization/" + ("acme" if i % 8 == 1 else "initech"))
        if i % 10 == 9:
            fl.append("/namespace/docs")
        docs.append((i // 20, f"d{i}", " ".join(words), "beta" if i % 9 == 4 else None, fl))
    docs.insert(30, (1, "d3", "alpha beta", None, ["/org/3", "/kind/b"]))
    docs.append((2, "d17", "zeta", None, []))
    docs.insert(35, (1, "d8", "gamma alpha", None, ["/org/1/team/2"]))
    docs.append((2, "d8", "beta beta alpha", None, ["/org/1/team/0", "/org/1/team/1"]))
    return docs


def db_reference(docs):
    """(reference corpus, word -> term id): docs in insertion order, an id's earlier versions deleted"""
    tid = {w: i for i, w in enumerate(WORDS)}
    seen, deleted = {}, [0] * len(docs)
    for i, (_, id_, _, _, _) in enumerate(docs):
        if id_ in seen:
            deleted[seen[id_]] = 1
        seen[id_] = i
    c = cr.Corpus([[tid[w] for w in t.split()] for _, _, t, _, _ in docs],
                  [None if n is None else [tid[n]] for _, _, _, n, _ in docs], [fl for *_, fl in docs], deleted,
                  len(WORDS))
    return c, tid


@pytest.fixture(scope="module")
def database(native, ctx):
    from fugu_amd import db
    docs = db_docs()
    d = db.Database(ctx)
    d.create_namespace("docs")
    last = 0
    for commit, id_, text, name, fl in docs:
        if commit != last:
            d.commit("docs")
            last = commit
        d.upsert(db.ObjectRecord(id_, text, facets=fl, metadata=None if name is None else {"name": name}), "docs")
    d.commit("docs")
    d.merge_wait("docs")
    c, tid = db_reference(docs)
    deleted = c.deleted
    assert d.doc_count("docs") == (len(docs), len(docs) - sum(deleted)) and sum(deleted) == 4
    assert d.merge_info("docs")["segments"] == 3
    yield d, c, tid
    d.close()


def test_db_facet_counts(database):
    d, c, tid = database
    for root in ("/", "/org", "/org/3", "/kind", "/namespace/docs", "/nothing"):
        pairs, total = d.facet_counts("docs", root)
        assert total == len(c.alive), root
        assert pairs == cr.children(c, root, c.alive), root
    assert d.facet_counts("docs", "/org")[0]  # not vacuous
    # a text query (Should Should) with a prefix filter and an exact one
    m = cr.match_set(c, [(cr.SHOULD, tid["alpha"]), (cr.SHOULD, tid["beta"])], [c.fid("/kind/a"), c.fid("/org/1")])
    assert 0 < len(m) < len(c.alive)
    for root in ("/", "/org", "/org/1"):
        pairs, total = d.facet_counts("docs", root, "alpha beta", filters=["/org/1/*", "/kind/a"])
        assert total == len(m)
        assert pairs == cr.children(c, root, m), root
    # Must / MustNot, a term the dictionary lacks, and `name` matches
    for q, cl in (("+alpha -beta", [(cr.MUST, tid["alpha"]), (cr.MUST_NOT, tid["beta"])]),
                  ("+alpha +nosuchword", [(cr.MUST, tid["alpha"]), (cr.MUST, None)]),
                  ("beta", [(cr.SHOULD, tid["beta"])])):
        m = cr.match_set(c, cl, None)
        assert d.facet_counts("docs", "/", q) == (cr.children(c, "/", m), len(m)), q


def test_db_facet_tree(database):
    d, c, _ = database

    def recurse(root, depth, max_depth):
        if max_depth is not None and depth >= max_depth:
            return []
        out = []
        for p, n in d.facet_counts("docs", root)[0]:
            out.append((p, n))
            out += recurse(p, depth + 1, max_depth)
        return out

    for max_depth in (1, 2, None):
        t = d.facet_tree("docs", max_depth)
        assert t == cr.tree(c, max_depth), max_depth
        assert t == recurse("/", 0, max_depth), max_depth
    assert len(d.facet_tree("docs", 1)) < len(d.facet_tree("docs", 2)) < len(d.facet_tree("docs"))
    assert d.facet_tree("docs", 0) == []


def test_db_facets_json(database):
    d, c, _ = database
    body = d.facets_json("docs")
    assert body.startswith('{"facets":[{"count":') and body.endswith('],"namespace":"docs","status":"success"}')
    js = json.loads(body)
    assert sorted(js) == ["facets", "namespace", "status"]
    # the handler asks for the children of "/" in the namespace's dataset (get_facets_at("/"))
    want = cr.children(c, "/", c.alive)
    assert [p for p, _ in want] == ["/kind", "/namespace", "/org"]
    assert [(f["path"], f["count"]) for f in js["facets"]] == want
    assert all(list(f) == ["count", "path"] for f in js["facets"])


def test_db_counts_over_a_merged_segment(native, ctx):
    """the same docs, a commit per 7: the 8th commit's eight segments are merged into
    one (deleted docs dropped, local doc ids remapped), two more commits follow and
    delete docs inside the merged segment; counts do not depend on the segmentation"""
    from fugu_amd import db
    docs = db_docs()
    c, tid = db_reference(docs)
    d = db.Database(ctx)
    d.create_namespace("m")
    for i, (_, id_, text, name, fl) in enumerate(docs):
        d.upsert(db.ObjectRecord(id_, text, facets=fl, metadata=None if name is None else {"name": name}), "m")
        if i % 7 == 6 or i == len(docs) - 1:
            d.commit("m")
            d.merge_wait("m")
    info = d.merge_info("m")
    assert info["merges"] >= 1 and info["segments"] < 10 and info["merged_docs"] > 0, info
    segs = d.segments("m")
    assert len(segs[0]) > 7  # the merged segment comes first
    assert any(c.deleted[g] for g in segs[0])  # ... and holds docs the later commits deleted
    for root in ("/", "/org", "/org/1", "/kind"):
        assert d.facet_counts("m", root) == (cr.children(c, root, c.alive), len(c.alive)), root
    m = cr.match_set(c, [(cr.SHOULD, tid["alpha"]), (cr.SHOULD, tid["beta"])], [c.fid("/kind/a"), c.fid("/org/1")])
    assert d.facet_counts("m", "/org", "alpha beta", filters=["/org/1/*", "/kind/a"]) == (cr.children(c, "/org", m), len(m))
    assert d.facet_tree("m") == cr.tree(c)
    d.close()


# ---------------------------------------------------------------- refusals
def test_refusals(native, ctx, main, main_index):
    c, qs, arrays, ct_ids, total, count = main
    q_off, terms = np.array([0, 2], np.uint32), np.array([0, 1], np.uint32)
    with pytest.raises(native.Unsupported) as e:
        native.count_batch([main_index], q_off, terms, ct_ids, phrase_len=[2, 0], phrase_pos=[0, 1])
    assert "phrase clause in a count query" in str(e.value)
    with pytest.raises(native.Unsupported) as e:
        native.count_batch([main_index], q_off, terms, np.zeros(native.FG_MAX_COUNT_TERMS + 1, np.uint32))
    assert "FG_MAX_COUNT_TERMS" in str(e.value)
    many = np.zeros((native.FG_MAX_COUNT_CELLS >> 10) + 1, np.uint32)
    with pytest.raises(native.Unsupported) as e:
        native.count_batch([main_index], np.zeros(1025, np.uint32), np.zeros(0, np.uint32), many)
    assert "FG_MAX_COUNT_CELLS" in str(e.value)
    with pytest.raises(native.Unsupported):
        native.count_batch([main_index], np.array([0, 17], np.uint32), np.zeros(17, np.uint32), ct_ids)
    with pytest.raises(native.Unsupported):  # 9 facet clauses
        native.count_batch([main_index], np.array([0, 0], np.uint32), np.zeros(0, np.uint32), ct_ids,
                           f_off=[0, 9], f_terms=np.zeros(9, np.uint32))
    for bad in (dict(q_off=np.array([0, 2, 1], np.uint32), terms=np.array([0, 1], np.uint32)),
                dict(q_off=q_off, terms=terms, occur=[0, 3]), dict(q_off=q_off, terms=terms, mode=7)):
        with pytest.raises(native.FuguError) as e:
            native.count_batch([main_index], count_terms=ct_ids, **bad)
        assert e.value.code == native.FG_EINVAL, bad


def test_refuses_snapshots_on_two_devices(native, main, main_index):
    if native.device_count() < 2:
        pytest.skip("one GPU")
    c, qs, arrays, ct_ids, total, count = main
    ctx2 = native.Context((0, 1))
    small = cr.small_corpus()
    to, tt, no, nt, facets = small.csr()
    other = native.Index.from_docs(ctx2, to, tt, small.n_terms, name_off=no, name_tok=nt, device=1, facets=facets)
    with pytest.raises(native.Unsupported) as e:
        run(native, [main_index, other], arrays, ct_ids)
    assert "several devices" in str(e.value)
    other.close()


# ---------------------------------------------------------------- concurrency
def test_concurrent_counts_beside_a_search(native, main, main_index):
    c, qs, arrays, ct_ids, total, count = main
    sq_off = np.arange(0, 17, 2, dtype=np.uint32)
    sterms = np.arange(16, dtype=np.uint32)
    want_search = main_index.search_batch(sq_off, sterms, 10)
    halves = [(arrays, ct_ids, total, count), (arrays, ct_ids[:7], total, count[:, :7])]
    errors = []

    def counter(i):
        try:
            arr, cts, wt, wc = halves[i % 2]
            for _ in range(6):
                t, cn = run(native, [main_index], arr, cts)
                assert np.array_equal(t, wt) and np.array_equal(cn, wc), i
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    def searcher():
        try:
            for _ in range(12):
                s, dd, n = main_index.search_batch(sq_off, sterms, 10)
                assert np.array_equal(n, want_search[2]) and np.array_equal(dd, want_search[1])
                assert np.array_equal(s.view(np.uint32), want_search[0].view(np.uint32))
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=counter, args=(i,)) for i in range(4)] + [threading.Thread(target=searcher)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
