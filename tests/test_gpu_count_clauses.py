"""fg_count_batch with phrase and group clauses on the device (k_crow, k_cjoin behind
fg_count_clauses) against tests/count_clause_ref.py -- exact equality,
the outputs are integers: every clause kind under every occur, beside terms and
beside each other, absent clauses, with and without facet clauses, over one snapshot,
over the same docs as three snapshots (one with its own term dictionary, one rescored
with new deletions), through several query slices, 64 slots sharing one row, on
indexes of 31, 64 and 65 docs, under every probe structure, through fg_db's
facet_counts, the planner's messages, and the refusals with the switch off.  What the
corpus holds for the kernels' edges is pinned by tests/test_count_clause_ref.py."""
import os

import numpy as np
import pytest

import count_clause_ref as ccr
import count_ref as cr
from test_gpu_count import RANK_ENVS, RANK_IDS, db_docs, db_reference

pytestmark = pytest.mark.gpu


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
def on(native):
    """fg_count_clauses on; the setting found is restored in teardown"""
    was = native.count_clauses(1)
    yield
    native.count_clauses(was)


@pytest.fixture()
def groups(native):
    was = native.group_clauses(1)
    yield
    native.group_clauses(was)


def reference(c, qs):
    """(batch arrays, count terms as ids, reference total, reference count): every facet term and one missing id"""
    plain = [(cl, fl) for _, cl, fl in qs]
    cts = list(range(len(c.fdict))) + [None]
    total, count = ccr.count_batch(c, plain, cts)
    return ccr.batch_arrays(plain), np.array([ccr.MISSING if t is None else t for t in cts], np.uint32), total, count


@pytest.fixture(scope="module")
def main():
    c = ccr.main_corpus()
    qs = ccr.query_batch(c)
    return (c, qs) + reference(c, qs)


def build(native, ctx, c, n_terms=None, deleted="own", positions=True):
    to, tt, no, nt, facets = c.csr()
    tg, ng = c.gaps_csr()
    dl = c.deleted if isinstance(deleted, str) else deleted
    return native.Index.from_docs(ctx, to, tt, n_terms or c.n_terms, name_off=no, name_tok=nt, deleted=dl, threads=8,
                                  facets=facets, positions=positions, text_gaps=tg, name_gaps=ng)


def run(native, ixs, arrays, ct_ids):
    q_off, terms, occur, plen, ppos, f_off, f_terms = arrays
    return native.count_batch(ixs, q_off, terms, ct_ids, f_off=f_off, f_terms=f_terms, occur=occur, phrase_len=plen,
                              phrase_pos=ppos)


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


def test_single_snapshot(native, on, main, main_index):
    c, qs, arrays, ct_ids, total, count = main
    same(run(native, [main_index], arrays, ct_ids), total, count, qs, "one snapshot")
    t0, c0 = run(native, [main_index], arrays, np.zeros(0, np.uint32))  # n_count == 0
    assert np.array_equal(t0, total) and c0.shape == (len(qs), 0)
    # the two kernels ran, and the four others keep their trace
    native.count_trace(1)
    native.count_clause_trace(1)
    try:
        run(native, [main_index], arrays, ct_ids)
        ms, calls = native.count_clause_trace(-1)
        ms4, calls4 = native.count_trace(-1)
    finally:
        native.count_trace(0)
        native.count_clause_trace(0)
    assert calls == calls4 == 1 and ms["k_crow"] > 0 and ms["k_cjoin"] > 0 and ms4["k_cmatch"] > 0 and ms4["k_ccount"] > 0


def test_three_snapshots(native, ctx, on, main):
    """the same docs as three segments of the namespace: totals and counts are summed"""
    c, qs, arrays, ct_ids, total, count = main
    a, b = 4001, 7010
    ca, cb, cc = c.slice(0, a), c.slice(a, b), c.slice(b, c.n)
    ia = build(native, ctx, ca)
    # its own term dictionary: the docs hold fewer than a quarter of the vocabulary it is given, and the
    # forward index keeps vocabulary ids while the lists are numbered locally
    big_vocab = 1024
    assert len({t for d in range(cb.n) for t in cb.text[d] + (cb.name[d] or [])}) * 4 < big_vocab
    ib = build(native, ctx, cb, n_terms=big_vocab)
    # built with no deletions, then rescored with the segment's deletions
    to, tt, no, nt, facets = cc.csr()
    base = build(native, ctx, cc, deleted=None)
    g = native.docs_stats(to, tt, cc.n_terms, name_off=no, name_tok=nt, threads=8, facets=facets)
    ic = base.rescore(g, deleted=cc.deleted)
    same(run(native, [ia, ib, ic], arrays, ct_ids), total, count, qs, "three snapshots")
    plain = [(cl, fl) for _, cl, fl in qs]
    cts = [None if t == ccr.MISSING else int(t) for t in ct_ids]
    for ix, seg, what in ((ib, cb, "own dictionary"), (ic, cc, "rescored")):
        st, sc = ccr.count_batch(seg, plain, cts)
        same(run(native, [ix], arrays, ct_ids), st, sc, qs, what)
    # the deleted doc that ends in the phrase is counted until the rescore deletes it
    ph = ccr.batch_arrays([([ccr.P(ccr.MUST, [4, 5])], None)])
    before, after = run(native, [base], ph, ct_ids[:0])[0][0], run(native, [ic], ph, ct_ids[:0])[0][0]
    undeleted = ccr.Corpus(cc.text, cc.name, cc.facets, np.zeros(cc.n, np.uint8), cc.n_terms, cc.text_gaps, cc.name_gaps,
                           c.fdict)
    m = ccr.match_mask(undeleted, [ccr.P(ccr.MUST, [4, 5])], None)
    assert m[cc.n - 2] and cc.deleted[cc.n - 2] and int(before) == int(m.sum()) > int(after)
    for x in (ia, ib, ic, base):
        x.close()


@pytest.mark.parametrize("kb", ["4", "11", "60"])
def test_query_slices(native, on, main, main_index, kb):
    """FUGU_COUNT_WS_KB bounds a pass's match rows and clause rows together (ceil(12007 / 32)
    words = 1504 B per row): 2, 7 and 40 rows per slice -- at 2 a query with two clause rows
    exceeds the bound by itself and runs as a slice of its own"""
    c, qs, arrays, ct_ids, total, count = main
    assert (c.n + 31) // 32 * 4 == 1504
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


def test_slots_sharing_one_row(native, on, main, main_index):
    """64 queries around one phrase (and one group): the clause is one row of the slice"""
    c = main[0]
    qs = [(f"shared {i}", [ccr.P(ccr.MUST, [4, 5]), ccr.T(ccr.MUST if i % 2 else ccr.MUST_NOT, i % 50)] +
           ([ccr.ANY(ccr.MUST, [6, 2])] if i % 3 == 0 else []), [c.fid("/org/3")] if i % 5 == 0 else None)
          for i in range(64)]
    arrays, ct_ids, total, count = reference(c, qs)
    assert (total > 0).sum() > 32
    same(run(native, [main_index], arrays, ct_ids), total, count, qs, "64 slots, one phrase row")


@pytest.mark.parametrize("n", [31, 64, 65])
def test_edge_indexes(native, ctx, on, n):
    """a single partial bitmap word, the exact word boundary, one bit into the third word; doc n-1 matches"""
    c = ccr.corpus(n, 5 + n)
    qs = ccr.query_batch(c, full=False)
    arrays, ct_ids, total, count = reference(c, qs)
    assert ccr.match_mask(c, qs[0][1], None)[n - 1] and qs[0][0] == "S ph"
    ix = build(native, ctx, c)
    same(run(native, [ix], arrays, ct_ids), total, count, qs, n)
    ix.close()


@pytest.mark.parametrize("env", RANK_ENVS, ids=RANK_IDS)
def test_probe_paths(native, ctx, on, main, env):
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
    same(run(native, [ix], arrays, ct_ids), total, count, qs, env)
    ix.close()


# ---------------------------------------------------------------- fg_db
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
    base, tid = db_reference(docs)
    assert d.merge_info("docs")["segments"] == 3
    yield d, ccr.Corpus(base.text, base.name, base.facets, base.deleted, base.n_terms), tid
    d.close()


def test_db_facet_counts_and_tree(native, on, groups, database):
    """the host path through three commits: phrase and group queries, the facet tree below their matches"""
    d, c, tid = database
    M, S, X = ccr.MUST, ccr.SHOULD, ccr.MUST_NOT
    w = lambda *ws: [tid[x] for x in ws]  # noqa: E731
    cases = [
        ('"alpha beta"', [ccr.P(S, w("alpha", "beta"))], None),
        ('+"beta alpha" -gamma', [ccr.P(M, w("beta", "alpha")), ccr.T(X, tid["gamma"])], None),
        ('"alpha beta" zeta', [ccr.P(S, w("alpha", "beta")), ccr.T(S, tid["zeta"])], None),
        ("(alpha OR gamma) AND zeta", [ccr.ANY(M, w("alpha", "gamma")), ccr.T(M, tid["zeta"])], None),
        ("+(beta AND delta) -alpha", [ccr.ALL(M, w("beta", "delta")), ccr.T(X, tid["alpha"])], None),
        ('+"alpha beta" +(gamma delta)', [ccr.P(M, w("alpha", "beta")), ccr.ANY(M, w("gamma", "delta"))], None),
        ('"beta alpha"', [ccr.P(S, w("beta", "alpha"))], ["/org/1/*", "/kind/a"]),
        ("(alpha gamma) -zeta", [ccr.ANY(S, w("alpha", "gamma")), ccr.T(X, tid["zeta"])], ["/org/1/*", "/kind/a"]),
    ]
    seen = 0
    for q, clauses, filters in cases:
        flt = [c.fid("/kind/a"), c.fid("/org/1")] if filters else None
        m = set(np.flatnonzero(ccr.match_mask(c, clauses, flt)).tolist())
        seen += bool(m)

        def tree(root):  # the facet tree below the query's matches, from facet_counts alone
            out = []
            for p, n in d.facet_counts("docs", root, q, filters=filters)[0]:
                out += [(p, n)] + tree(p)
            return out

        def want(root):
            out = []
            for p, n in cr.children(c, root, m):
                out += [(p, n)] + want(p)
            return out

        assert d.facet_counts("docs", "/", q, filters=filters) == (cr.children(c, "/", m), len(m)), q
        assert tree("/") == want("/"), q
    assert seen >= 6
    assert d.facet_tree("docs") == cr.tree(c)  # AllQuery, as before


# ---------------------------------------------------------------- messages and refusals
def test_planner_messages(native, ctx, on, main, main_index):
    c = main[0]
    q_off, terms = np.array([0, 3], np.uint32), np.array([4, 5, 0], np.uint32)
    cases = [(dict(phrase_len=[4, 0, 0], phrase_pos=[0, 1, 2]), "query 0: bad phrase_len at term 0"),
             (dict(phrase_len=[1, 0, 1], phrase_pos=[0, 0, 0]), "query 0: bad phrase_len at term 1"),
             (dict(phrase_len=[0xC0000002, 0, 1], phrase_pos=[0, 0, 0]), "query 0: bad phrase_len at term 0"),
             (dict(phrase_len=[0x80000001, 1, 1], phrase_pos=[0, 0, 0]), "query 0: bad phrase_len at term 0"),
             (dict(phrase_len=[2, 0, 1], phrase_pos=[0, 0, 0]), "phrase offsets must increase"),
             (dict(phrase_len=[2, 0, 1], phrase_pos=[0, 1 << 30, 0]), "phrase offset too large")]
    for kw, msg in cases:
        with pytest.raises(native.FuguError) as e:
            native.count_batch([main_index], q_off, terms, **kw)
        assert e.value.code == native.FG_EINVAL and msg in str(e.value), kw
    small = ccr.corpus(64, 3)
    flat = build(native, ctx, small, positions=False)
    with pytest.raises(native.Unsupported) as e:
        native.count_batch([flat], q_off, terms, phrase_len=[1, 2, 0], phrase_pos=[0, 0, 1])
    assert "query 0: snapshot built without positions" in str(e.value)
    # groups and terms need no positions
    qs = [("any", [ccr.ANY(ccr.MUST, [2, 6]), ccr.T(ccr.MUST_NOT, 0)], None)]
    arrays, ct_ids, total, count = reference(small, qs)
    same(run(native, [flat], arrays, ct_ids), total, count, qs, "no positions")
    with pytest.raises(native.Unsupported):  # kMaxTerms holds
        native.count_batch([main_index], np.array([0, 17], np.uint32), np.zeros(17, np.uint32),
                           phrase_len=[2, 0] + [1] * 15, phrase_pos=[0, 1] + [0] * 15)
    flat.close()


def test_switch_off_refuses_as_before(native, groups, main, main_index, database):
    assert native.count_clauses() == 0
    q_off, terms = np.array([0, 2], np.uint32), np.array([4, 5], np.uint32)
    with pytest.raises(native.Unsupported) as e:
        native.count_batch([main_index], q_off, terms, phrase_len=[2, 0], phrase_pos=[0, 1])
    assert "query 0: phrase clause in a count query" in str(e.value)
    with pytest.raises(native.Unsupported) as e:
        native.count_batch([main_index], q_off, terms, phrase_len=[0x80000002, 0], phrase_pos=[0, 0])
    assert "query 0: group clause in a count query" in str(e.value)
    d = database[0]
    for q, msg in (('"alpha beta"', "phrase clause in a count query"), ("(alpha gamma) zeta", "group clause in a count query")):
        with pytest.raises(native.Unsupported) as e:
            d.facet_counts("docs", "/", q)
        assert "query outside the device subset: " + msg in str(e.value)
