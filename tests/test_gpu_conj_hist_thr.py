"""k_conj's publish-side histogram threshold (FUGU_CONJ_HIST_THR, fg_internal.h
kOptConjHistThr) against tests/bool_ref.py (runs on the MI355X box): an ending
multi-list item reads the query's bins back as it adds to them and publishes the
query-wide k-th edge, score-only, as a threshold.

  a. many items per query: 64 three-term and 16 five-term ANDs over the 8 most
     frequent terms of a 262,144-doc corpus (every lead list >= 3 items of 16
     chunks), k = 1 / 10 / 100, the setting on and off;
  b. ties at the k-th score: 100,000 docs that all score the same (one bin), as
     one snapshot and as two snapshots of a multi-snapshot plan's merged select:
     a score-only edge must not drop a tied doc;
  c. two linked single-snapshot plans over the halves of a.'s corpus;
  d. fewer than k matches (Must + MustNot + Should, and a facet filter): no
     threshold forms, every match is a candidate, on and off.
Bar: doc ids and score bits equal bool_ref's, and on == off.
"""
import os

import numpy as np
import pytest

import bool_ref as br
from seed_cases import N_BIG, N_TIE, big_case, few_case, tie_case

pytestmark = pytest.mark.gpu

VAR = "FUGU_CONJ_HIST_THR"
ITEM = 16 * 2048  # lead postings of a full work item (kMaxGroup chunks of kChunk)


@pytest.fixture(scope="module")
def native():
    from fugu_amd import native as nat
    if nat.device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    return nat


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context((0,))


def setting(value, fn):
    """fn() with the planner setting at `value` (read when a plan is made)."""
    old = os.environ.get(VAR)
    os.environ[VAR] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[VAR]
        else:
            os.environ[VAR] = old


def batch(qs):
    q_off = np.cumsum([0] + [len(q) for q in qs]).astype(np.uint32)
    return q_off, np.array([t for q in qs for t in q], np.uint32)


def assert_exact(s, d, n, want, what):
    ws, wd = want
    assert int(n) == len(wd), (what, int(n), len(wd))
    assert np.array_equal(np.asarray(d[:n], np.int64), wd), what
    assert np.array_equal(np.asarray(s[:n], np.float32).view(np.uint32), ws.view(np.uint32)), what


def same_live(a, b):
    """Two (scores, docs, counts) results: equal counts, and doc ids and score bits up to them."""
    assert np.array_equal(a[2], b[2])
    live = np.arange(a[0].shape[1])[None, :] < a[2][:, None]
    assert np.array_equal(a[1][live], b[1][live])
    assert np.array_equal(a[0][live].view(np.uint32), b[0][live].view(np.uint32))


@pytest.fixture(scope="module")
def big(native, ctx):
    from fugu_amd import synth
    c, ref, top, qs = big_case()
    ix = native.Index.from_docs(ctx, c.off, c.tok, synth.VOCAB, threads=16)
    # every lead list (the rarest of a query's terms) is at least three full work items
    assert min(ix.df(int(t)) for t in top) >= 3 * ITEM
    want = [ref.search(q, None, 100) for q in qs]
    assert all(len(w[1]) == 100 for w in want)
    yield {"c": c, "ref": ref, "qs": qs, "ix": ix, "want": want}
    ix.close()


@pytest.mark.parametrize("k", [1, 10, 100])
def test_many_items_per_query(native, big, k):
    q_off, terms = batch(big["qs"])
    got, cand = {}, {}
    for v in ("1", "0"):
        p = setting(v, lambda: big["ix"].plan(q_off, terms, k))
        assert p.info().total_chunks >= 3 * len(big["qs"])  # several items per query
        p.execute()
        got[v] = p.results()
        cand[v] = int(p.candidate_counts().sum())
        p.close()
        for i, w in enumerate(big["want"]):
            assert_exact(got[v][0][i], got[v][1][i], got[v][2][i], (w[0][:k], w[1][:k]), (v, k, i, big["qs"][i]))
    print(f"\nk={k}: candidates written on / off: {cand['1']} / {cand['0']}")
    same_live(got["1"], got["0"])


@pytest.mark.parametrize("k", [10, 100])
def test_ties_at_the_kth_score(native, ctx, k):
    import torch
    off, tok, V, qs = tie_case()
    ref = br.Corpus(V, off, tok)
    q_off, terms = batch(qs)
    nq = len(qs)
    want = [ref.search(q, None, k) for q in qs]
    for w in want:  # all scores equal: the first k docs
        assert np.array_equal(w[1], np.arange(k)) and len(set(w[0].view(np.uint32).tolist())) == 1
    one = native.Index.from_docs(ctx, off, tok, V, threads=16)
    half = N_TIE // 2
    bounds = np.array([0, half, N_TIE], np.int64)
    parts = [(off[b:e + 1] - off[b], tok[int(off[b]):int(off[e])]) for b, e in zip(bounds[:-1], bounds[1:])]
    g = native.docs_stats(*parts[0], V, threads=16) + native.docs_stats(*parts[1], V, threads=16)
    two = [native.Index.from_docs(ctx, o, t, V, threads=16, global_stats=g, keep_host=False) for o, t in parts]
    wseg = [ref.search(q, None, k, seg_bounds=bounds) for q in qs]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    for v in ("1", "0"):
        s, d, n = setting(v, lambda: one.search_batch(q_off, terms, k))
        for i in range(nq):
            assert_exact(s[i], d[i], n[i], want[i], ("one snapshot", v, k, i))
        p = setting(v, lambda: native.Plan(two, q_off, terms, k))
        os_ = torch.zeros(nq * k, dtype=torch.float32, device=dev)
        od, osh = (torch.zeros(nq * k, dtype=torch.int32, device=dev) for _ in range(2))
        on = torch.zeros(nq, dtype=torch.int32, device=dev)
        p.execute_merged(st, os_.data_ptr(), od.data_ptr(), osh.data_ptr(), on.data_ptr())
        torch.cuda.synchronize()
        ms, md = os_.cpu().numpy().reshape(nq, k), od.cpu().numpy().view(np.uint32).reshape(nq, k)
        msh, mn = osh.cpu().numpy().reshape(nq, k), on.cpu().numpy()
        for i in range(nq):
            m = int(mn[i])
            # (score desc, shard asc, doc asc): the first snapshot's first k docs
            assert (msh[i, :m] == 0).all(), (v, k, i)
            assert_exact(ms[i], md[i, :m].astype(np.int64) + bounds[msh[i, :m]], m, wseg[i], ("two snapshots", v, k, i))
        p.close()
    for ix in [one] + two:
        ix.close()


def test_linked_plans(native, ctx, big):
    """Two linked single-snapshot plans over the halves of the corpus (global
    statistics), run back to back on one stream: the merged hits."""
    import torch
    from fugu_amd import synth
    from fugu_amd.shard import merge_on_device
    c, ref, qs, k = big["c"], big["ref"], big["qs"], 100
    V = synth.VOCAB
    bounds = np.array([0, N_BIG // 2, N_BIG], np.int64)
    parts = [(c.off[b:e + 1] - c.off[b], c.tok[int(c.off[b]):int(c.off[e])]) for b, e in zip(bounds[:-1], bounds[1:])]
    g = native.docs_stats(*parts[0], V, threads=16) + native.docs_stats(*parts[1], V, threads=16)
    shards = [native.Index.from_docs(ctx, o, t, V, threads=16, global_stats=g, keep_host=False) for o, t in parts]
    q_off, terms = batch(qs)
    nq = len(qs)
    want = [ref.search(q, None, k, seg_bounds=bounds) for q in qs]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    outs = {}
    for v in ("1", "0"):
        plans = setting(v, lambda: [ix.plan(q_off, terms, k) for ix in shards])
        native.link_plans(plans)
        gs = torch.empty((2, nq * k), dtype=torch.float32, device=dev)
        gd = torch.empty((2, nq * k), dtype=torch.int32, device=dev)
        gn = torch.empty((2, nq), dtype=torch.int32, device=dev)
        for rep in range(2):  # the owner re-zeroes the shared state each round
            for r, p in enumerate(plans):
                p.execute(st, gs[r].data_ptr(), gd[r].data_ptr(), gn[r].data_ptr())
            ms, md, msh, mn = merge_on_device(gs, gd, gn, nq, k, st)
            torch.cuda.synchronize()
        ms, mn = ms.cpu().numpy().reshape(nq, k), mn.cpu().numpy()
        gdoc = md.cpu().numpy().view(np.uint32).reshape(nq, k).astype(np.int64) + bounds[msh.cpu().numpy().reshape(nq, k)]
        for i in range(nq):
            assert_exact(ms[i], gdoc[i], mn[i], want[i], ("linked", v, i))
        outs[v] = (ms, gdoc, mn)
        del p
        del plans[1:]  # the linked plan before its owner
        del plans
    for a, b in zip(outs["1"], outs["0"]):
        assert np.array_equal(a, b)
    for ix in shards:
        ix.close()


def test_fewer_than_k_matches(native, ctx):
    c, V, facets, ref, qs = few_case()
    k = 100
    q_off, terms = batch([q[0] for q in qs])
    occur = np.array([o for q in qs for o in q[1]], np.uint8)
    f_off, f_terms = batch([q[2] for q in qs])
    want = [ref.search(t, o, k, f) for t, o, f in qs]
    assert all(0 < len(w[1]) < k for w in want), [len(w[1]) for w in want]
    ix = native.Index.from_docs(ctx, c.off, c.tok, V, threads=16, facets=facets)
    got = {}
    for v in ("1", "0"):
        p = setting(v, lambda: ix.plan(q_off, terms, k, f_off=f_off, f_terms=f_terms, occur=occur))
        p.execute()
        got[v] = p.results()
        cand = p.candidate_counts()
        p.close()
        for i, w in enumerate(want):
            assert_exact(got[v][0][i], got[v][1][i], got[v][2][i], w, (v, i, qs[i]))
            assert int(cand[i]) == len(w[1]), (v, i)  # no threshold formed: every match was written
    same_live(got["1"], got["0"])
    ix.close()
