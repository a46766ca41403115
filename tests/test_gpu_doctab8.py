"""k_conj's one-byte bound tables (DevIndex::dtab8, ProbeDesc kPdBound) against
a build without them and the CPU oracle (runs on the MI355X box).

A deferred query (>= 3 unfiltered Must lists) whose first probed list has a
bound table tests one byte per candidate -- 0: absent, else an upper bound of
the posting's score -- before the exact probe; the survivors wait in the LDS
queue as (doc, lead score) and the flush probes the list exactly.  The bound
only ever drops what the exact score would drop, so a build with the tables
forced wide (FUGU_DOCTAB8_DIV=64, FUGU_DOCTAB8_LEAD=0) must return the hits of
a build with none (FUGU_DOCTAB8_DIV=0) bit for bit -- scores, doc ids, counts --
and both the oracle's (ids exact, scores rtol 1e-5).  N = 20,011 docs (no
multiple of 4, 32, 128 or 2048), a vocabulary of 2048 terms so that dozens are
dense, 256 queries, k = 10 and 100:
  * AND of 3-5 terms with a table term as the second list (the deferred path);
  * the same queries cut to 2 terms and facet-filtered: no bound, same hits;
  * a dense lead (>= 3 x 2048 postings) on all-dense lists under k = 100;
  * MustNot and Should clauses after the bounded list;
  * a hand-made corpus (below): scores that rise with the doc id, so that once a
    threshold exists nearly every candidate passes the bound and more than the
    queue's 896 entries survive between flushes (the overflow wave goes on
    inline); a lead whose short last chunk ends at doc N - 1 (the table's last
    byte, probed with a threshold); a table term present in doc 0, doc N - 1
    and otherwise only at multiples of 128; a term whose postings all score
    the same (every byte 255); plateaus of identical docs, so the k-th score is
    tied across more than k docs and the bound equals the threshold
    (doc-ascending ties are kept);
  * deletions under unchanged statistics (the tables stay in use);
  * a rescore to other statistics (the plan scores at query time and must not
    read the build-time table);
  * one plan over a snapshot with tables and one without, merged select.
"""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL = 1e-5
N = 20_011
V = 2048
CUT = 12_000  # the two snapshots of the last cases: [0, CUT) and [CUT, N)
NQ = 256
KS = (10, 100)
MUST, SHOULD, MUST_NOT = 0, 1, 2
FORCED = {"FUGU_DOCTAB8_DIV": "64", "FUGU_DOCTAB8_LEAD": "0"}
# the hand-made corpus: its sparsest table term holds N // 128 + 2 docs, under N / 64
FORCED_H = {"FUGU_DOCTAB8_DIV": "128", "FUGU_DOCTAB8_LEAD": "0"}
OFF = {"FUGU_DOCTAB8_DIV": "0"}
DEFAULT = {}


@contextlib.contextmanager
def env(e):
    """The FUGU_DOCTAB8_* environment of a build and of its plans (FUGU_DOCTAB8_LEAD
    is read when a plan is made), restored afterwards."""
    keys = ("FUGU_DOCTAB8_DIV", "FUGU_DOCTAB8_LEAD")
    old = {k: os.environ.get(k) for k in keys}
    for k in keys:
        os.environ.pop(k, None)
    os.environ.update(e)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def native():
    from fugu_amd import native as nat
    if nat.device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    assert (nat.OCCUR_MUST, nat.OCCUR_SHOULD, nat.OCCUR_MUST_NOT) == (MUST, SHOULD, MUST_NOT)
    return nat


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context((0,))


def flat(qs):
    return np.cumsum([0] + [len(q) for q in qs]).astype(np.uint32), np.array([x for q in qs for x in q], np.uint32)


def same_bits(a, b, what):
    """two device results: counts, doc ids and score bits identical"""
    assert np.array_equal(a[2], b[2]), what
    for i in range(len(a[2])):
        m = int(a[2][i])
        assert np.array_equal(a[1][i, :m], b[1][i, :m]), (what, i)
        assert np.array_equal(a[0][i, :m].view(np.uint32), b[0][i, :m].view(np.uint32)), (what, i)


def assert_hits(s, d, n, rs, rd, what):
    assert int(n) == len(rd), (what, int(n), len(rd))
    assert np.array_equal(np.asarray(d[:n], np.int64), np.asarray(rd, np.int64)), what
    rel = np.abs(s[:n].astype(np.float64) - rs) / np.maximum(np.abs(rs), 1e-30)
    assert (rel <= RTOL).all(), (what, rel.max())


def vs_oracle(res, want, what):
    rs, rd, rn = want
    assert np.array_equal(res[2], rn), what
    for i in range(len(rn)):
        assert_hits(res[0][i], res[1][i], res[2][i], rs[i, :rn[i]], rd[i, :rn[i]], (what, i))


def search(ix, e, q_off, terms, k, **kw):
    with env(e):
        return ix.search_batch(q_off, terms, k, **kw)


def in_cost_order(main, ts):
    """a query's terms in intersection order (cost = df, stable)"""
    return sorted(ts, key=lambda t: main["df"][t])


@pytest.fixture(scope="module")
def main(native, ctx):
    """The synthetic corpus with a facet field (doc % 5), its three builds, the
    oracle, and the terms the forced build gave bound tables."""
    from fugu_amd import synth
    from oracle import oracle as orc
    c = synth.corpus(N, V)
    facets = (np.arange(N + 1, dtype=np.uint64), (np.arange(N) % 5).astype(np.uint32), 5)
    ixs = {}
    for name, e in (("forced", FORCED), ("off", OFF), ("default", DEFAULT)):
        with env(e):
            ixs[name] = native.Index.from_docs(ctx, c.off, c.tok, V, threads=16, facets=facets)
    n_tab, tab_bytes = ixs["forced"].bound_tables()
    assert n_tab >= 8 and tab_bytes == n_tab * ((N + 127) // 128 * 128)  # the forced build really has tables
    assert ixs["off"].bound_tables() == (0, 0)
    assert ixs["forced"].stats().device_bytes - ixs["off"].stats().device_bytes >= tab_bytes
    assert ixs["forced"].doc_tables() == ixs["off"].doc_tables()  # the f32 tables are reported apart, unchanged
    df = np.array([ixs["off"].df(t) for t in range(V)])
    tabs = set(np.argsort(-df, kind="stable")[:n_tab].tolist())
    assert all(df[t] * 64 >= N for t in tabs)
    ref = orc.OracleIndex(V, c.off, c.tok, threads=16, facet_off=facets[0], facet_tok=facets[1], n_fterms=5)
    yield dict(c=c, facets=facets, ixs=ixs, tabs=tabs, df=df, ref=ref)
    ref.close()
    for ix in ixs.values():
        ix.close()


@pytest.fixture(scope="module")
def and_queries(main):
    """AND of 3-5 terms, and what the oracle returns for them (shared, read-only)"""
    from fugu_amd import synth
    q_off, terms = synth.queries(NQ, 3, 5, max_rank=96, seed_q=4321)
    second = sum(in_cost_order(main, terms[q_off[i]:q_off[i + 1]].tolist())[1] in main["tabs"] for i in range(NQ))
    assert second >= 64, second  # a table term as the second list
    want = {k: main["ref"].search_batch(q_off, terms, k, threads=16)[:3] for k in KS}
    assert all(w[2].sum() > 0 for w in want.values())
    return q_off, terms, want


def test_and_queries_on_the_deferred_path(native, main, and_queries):
    q_off, terms, want = and_queries
    for k in KS:
        on = search(main["ixs"]["forced"], FORCED, q_off, terms, k)
        off = search(main["ixs"]["off"], OFF, q_off, terms, k)
        same_bits(on, off, ("forced", k))
        same_bits(search(main["ixs"]["default"], DEFAULT, q_off, terms, k), off, ("default", k))
        vs_oracle(on, want[k], ("forced", k))
        vs_oracle(off, want[k], ("off", k))


def test_two_term_and_facet_filtered_take_no_bound(native, main, and_queries):
    q_off, terms, _ = and_queries
    # the same queries cut to their first two lists
    two = [in_cost_order(main, terms[q_off[i]:q_off[i + 1]].tolist())[:2] for i in range(NQ)]
    t_off, t_terms = flat(two)
    for k in KS:
        on = search(main["ixs"]["forced"], FORCED, t_off, t_terms, k)
        off = search(main["ixs"]["off"], OFF, t_off, t_terms, k)
        same_bits(on, off, ("two", k))
        rs, rd, rn, _, _ = main["ref"].search_batch(t_off, t_terms, k, threads=16)
        assert rn.sum() > 0
        vs_oracle(on, (rs, rd, rn), ("two", k))
    # ... and whole, with 1-2 facet clauses each
    fl = [[j % 5] if j % 2 else [j % 5, (j + 2) % 5] for j in range(NQ)]
    f_off, f_terms = flat(fl)
    for k in KS:
        on = search(main["ixs"]["forced"], FORCED, q_off, terms, k, f_off=f_off, f_terms=f_terms)
        off = search(main["ixs"]["off"], OFF, q_off, terms, k, f_off=f_off, f_terms=f_terms)
        same_bits(on, off, ("facet", k))
        rs, rd, rn, _, _ = main["ref"].search_batch(q_off, terms, k, threads=16, f_off=f_off, f_terms=f_terms)
        assert rn.sum() > 0
        vs_oracle(on, (rs, rd, rn), ("facet", k))


def test_dense_lead_on_all_dense_lists(native, main):
    dense = np.argsort(-main["df"], kind="stable")[:16].tolist()
    assert all(main["df"][t] >= 3 * 2048 for t in dense) and set(dense) <= main["tabs"]
    rng = np.random.default_rng(11)
    qs = [rng.choice(dense, size=3 + j % 3, replace=False).tolist() for j in range(NQ)]
    q_off, terms = flat(qs)
    on = search(main["ixs"]["forced"], FORCED, q_off, terms, 100)
    off = search(main["ixs"]["off"], OFF, q_off, terms, 100)
    same_bits(on, off, "dense")
    same_bits(search(main["ixs"]["default"], DEFAULT, q_off, terms, 100), off, "dense default")
    rs, rd, rn, _, _ = main["ref"].search_batch(q_off, terms, 100, threads=16)
    assert (rn == 100).all()
    vs_oracle(on, (rs, rd, rn), "dense")


def test_must_not_and_should_after_the_bounded_list(native, main):
    df, tabs = main["df"], sorted(main["tabs"], key=lambda t: -main["df"][t])
    plain = [t for t in np.argsort(-df, kind="stable").tolist() if t not in main["tabs"]]
    lead = plain[40]  # (rarer than every table term: it leads)
    qs, occ = [], []
    for j in range(16):
        t, u, w = tabs[40 + j % 8], tabs[(j + 3) % 8], tabs[8 + j % 8]  # df: t < w < u
        qs += [[lead, t, u, w], [lead, t, u, w], [lead, t, u, w, tabs[20]], [lead, t, w]]
        occ += [[MUST, MUST, MUST, MUST_NOT], [MUST, MUST, MUST, SHOULD], [MUST, MUST, MUST, SHOULD, MUST_NOT],
                [MUST, MUST, MUST]]
    q_off, terms = flat(qs)
    occur = np.array([x for o in occ for x in o], np.uint8)
    for k in KS:
        on = search(main["ixs"]["forced"], FORCED, q_off, terms, k, occur=occur)
        off = search(main["ixs"]["off"], OFF, q_off, terms, k, occur=occur)
        same_bits(on, off, ("occur", k))
        rs, rd, rn, _, _ = main["ref"].search_batch(q_off, terms, k, threads=16, occur=occur)
        assert (rn > 0).sum() >= len(qs) // 2
        vs_oracle(on, (rs, rd, rn), ("occur", k))
        vs_oracle(off, (rs, rd, rn), ("occur off", k))


LEN_H = 120  # tokens per hand-made doc (one fieldnorm for all)
PLATEAU = 700


@pytest.fixture(scope="module")
def handmade(native, ctx):
    """Docs of one length.  `a` (the lead: 8 x 2048 + 100 docs, doc 0 and doc N - 1
    among them, so its last chunk is short and ends at the last byte), `b` and `c`
    (every doc) occur 1 + doc // 700 times in their docs: scores rise with the doc
    id in plateaus of 700 identical docs.  `same`: once in every doc but the first
    2000 (all postings score the same).  `x`: once in doc 0, doc N - 1 and the
    other multiples of 128; `ls`: a sparse lead over some of them.  The filler
    vocabulary is uniform and sparse, so exactly the hand-made terms get tables."""
    from oracle import oracle as orc
    V0 = 1 << 20
    rng = np.random.default_rng(3)
    names = ["a", "b", "c", "same", "x", "ls", "half"]
    T = {n: V0 + i for i, n in enumerate(names)}
    a_docs = np.union1d(np.sort(rng.choice(np.arange(1, N - 1), 8 * 2048 + 98, replace=False)), [0, N - 1])
    x_docs = np.union1d(np.arange(0, N, 128), [N - 1])
    ls_docs = np.union1d(x_docs[::2], np.union1d(np.arange(5, N, 331), [0, N - 1]))
    has = {"a": np.zeros(N, bool), "x": np.zeros(N, bool), "ls": np.zeros(N, bool)}
    has["a"][a_docs] = has["x"][x_docs] = has["ls"][ls_docs] = True
    assert len(a_docs) == 8 * 2048 + 100 and len(x_docs) * 128 >= N > len(x_docs) * 64 and len(ls_docs) < len(x_docs)
    off = np.arange(N + 1, dtype=np.uint64) * LEN_H
    tok = rng.integers(0, V0, N * LEN_H, dtype=np.uint32).reshape(N, LEN_H)
    for d in range(N):
        r = 1 + d // PLATEAU
        row = [T["b"]] * r + [T["c"]] * r + ([T["a"]] * r if has["a"][d] else [])
        row += ([T["same"]] if d >= 2000 else []) + ([T["x"]] if has["x"][d] else []) + ([T["ls"]] if has["ls"][d] else [])
        row += [T["half"]] if d % 2 == 0 else []
        tok[d, :len(row)] = row
    tok = tok.reshape(-1)
    Vh = V0 + len(T)
    with env(FORCED_H):
        on = native.Index.from_docs(ctx, off, tok, Vh, threads=16)
    with env(OFF):
        no = native.Index.from_docs(ctx, off, tok, Vh, threads=16)
    # the hand-made terms, and only they (`ls`, under N / 128 docs, only ever leads: none)
    assert on.bound_tables()[0] == len(T) - 1 and len(ls_docs) * 128 < N, on.bound_tables()
    ref = orc.OracleIndex(Vh, off, tok, threads=16)
    yield dict(T=T, on=on, no=no, ref=ref, a_docs=a_docs, x_docs=x_docs, ls_docs=ls_docs)
    ref.close()
    on.close()
    no.close()


def test_handmade_overflow_ties_and_table_edges(native, handmade):
    h, T = handmade, handmade["T"]
    base = [[T["a"], T["b"], T["c"]],             # rising scores: the queue overflows; ties at the top plateau
            [T["a"], T["same"], T["c"]],          # every byte 255: the bound is the score
            [T["a"], T["same"], T["b"], T["c"]],
            [T["ls"], T["x"], T["half"]],         # bytes at multiples of 128, doc 0 and doc N - 1
            [T["ls"], T["x"], T["b"]],
            [T["ls"], T["x"], T["half"], T["c"]],
            [T["x"], T["half"], T["b"]],          # the sparse table term leads
            [T["half"], T["same"], T["c"]]]
    # a full batch: a query's chunks then run several to a work item, so the later
    # chunks of an item (its short last one too) see the threshold of the earlier ones
    qs = [base[j % len(base)] for j in range(NQ)]
    q_off, terms = flat(qs)
    for k in KS:
        a = search(h["on"], FORCED_H, q_off, terms, k)
        b = search(h["no"], OFF, q_off, terms, k)
        same_bits(a, b, ("handmade", k))
        rs, rd, rn, _, _ = h["ref"].search_batch(q_off[:len(base) + 1], terms[:q_off[len(base)]], k, threads=16)
        for part in (a, b):
            first = tuple(x[:len(base)] for x in part)
            vs_oracle(first, (rs, rd, rn), ("handmade", k))
        # the top plateau's first k docs of `a`, doc-ascending, doc N - 1 past them
        top = h["a_docs"][h["a_docs"] >= (N - 1) // PLATEAU * PLATEAU]
        assert len(top) > k and np.array_equal(a[1][0, :k], top[:k])
        assert len(set(a[0][0, :k].tolist())) == 1
    # ls & x (& half, & b: x's docs are even): doc 0 and doc N - 1 among the hits
    got = search(h["on"], FORCED_H, q_off, terms, 1000)
    same_bits(got, search(h["no"], OFF, q_off, terms, 1000), ("handmade", 1000))
    want = np.intersect1d(h["ls_docs"], h["x_docs"])
    assert {0, N - 1} <= set(want.tolist()) and (want % 2 == 0).all()
    for qi in (3, 4):
        assert set(got[1][qi, :got[2][qi]].tolist()) == set(want.tolist()), qi


def test_deletions_keep_the_tables(native, main):
    """Deletions under the build's own statistics: the rescored snapshot shares
    the tables and plans on them; no deleted doc appears."""
    from fugu_amd import synth
    from oracle import oracle as orc
    c = main["c"]
    rng = np.random.default_rng(5)
    dl = (rng.random(N) < 0.3).astype(np.uint8)
    dl[0] = 0
    dl[N - 1] = 1
    g = native.docs_stats(c.off, c.tok, V, threads=16, facets=main["facets"])
    re_on = main["ixs"]["forced"].rescore(g, deleted=dl)
    re_off = main["ixs"]["off"].rescore(g, deleted=dl)
    assert re_on.bound_tables() == main["ixs"]["forced"].bound_tables() and re_off.bound_tables() == (0, 0)
    ref = orc.OracleIndex(V, c.off, c.tok, deleted=dl, threads=16)
    q_off, terms = synth.queries(NQ, 3, 5, max_rank=96, seed_q=77)
    for k in KS:
        a = search(re_on, FORCED, q_off, terms, k)
        b = search(re_off, OFF, q_off, terms, k)
        same_bits(a, b, ("deleted", k))
        for i in range(NQ):
            assert not dl[a[1][i, :a[2][i]]].any(), i
        rs, rd, rn, _, _ = ref.search_batch(q_off, terms, k, threads=16)
        vs_oracle(a, (rs, rd, rn), ("deleted", k))
    ref.close()
    re_on.close()
    re_off.close()


@pytest.fixture(scope="module")
def halves(native, ctx, main):
    """The corpus as two commits, [0, CUT) and [CUT, N): the first built under its
    own statistics with tables (then rescored to the namespace's), and both under
    the namespace's, the first with and without tables, the second without."""
    c = main["c"]
    a = (c.off[:CUT + 1].copy(), c.tok[:c.off[CUT]])
    b = (c.off[CUT:] - c.off[CUT], c.tok[c.off[CUT]:])
    g = native.docs_stats(*a, V, threads=16) + native.docs_stats(*b, V, threads=16)
    with env(FORCED):
        own_a = native.Index.from_docs(ctx, *a, V, threads=16)
        seg_a_on = native.Index.from_docs(ctx, *a, V, threads=16, global_stats=g)
    with env(OFF):
        seg_a_off = native.Index.from_docs(ctx, *a, V, threads=16, global_stats=g)
        seg_b = native.Index.from_docs(ctx, *b, V, threads=16, global_stats=g)
    assert own_a.bound_tables()[0] >= 8 and seg_a_on.bound_tables()[0] >= 8
    assert seg_a_off.bound_tables() == (0, 0) and seg_b.bound_tables() == (0, 0)
    d = dict(g=g, own_a=own_a, seg_a_on=seg_a_on, seg_a_off=seg_a_off, seg_b=seg_b,
             cuts=np.array([0, CUT, N], np.uint32))
    yield d
    for k in ("own_a", "seg_a_on", "seg_a_off", "seg_b"):
        d[k].close()


def merged(native, ixs, e, q_off, terms, k):
    """fg_plan_execute_merged of one plan over the snapshots: (scores, global doc ids, counts)"""
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    nq = len(q_off) - 1
    with env(e):
        p = native.Plan(ixs, q_off, terms, k)
    os_ = torch.zeros(nq * k, dtype=torch.float32, device=dev)
    od, osh = (torch.zeros(nq * k, dtype=torch.int32, device=dev) for _ in range(2))
    on = torch.zeros(nq, dtype=torch.int32, device=dev)
    p.execute_merged(st, os_.data_ptr(), od.data_ptr(), osh.data_ptr(), on.data_ptr())
    torch.cuda.synchronize()
    p.close()
    base = np.array([0, CUT], np.int64)
    gd = od.cpu().numpy().view(np.uint32).reshape(nq, k).astype(np.int64) + base[osh.cpu().numpy().reshape(nq, k)]
    return os_.cpu().numpy().reshape(nq, k), gd, on.cpu().numpy().astype(np.uint32)


@pytest.fixture(scope="module")
def seg_queries(main, halves):
    """3-5 term ANDs and the oracle's segmented search of them (shared, read-only)"""
    from fugu_amd import synth
    q_off, terms = synth.queries(NQ, 3, 5, max_rank=96, seed_q=91)
    want = {k: [main["ref"].search(terms[q_off[i]:q_off[i + 1]], k, seg_bounds=halves["cuts"]) for i in range(NQ)]
            for k in KS}
    return q_off, terms, want


def test_rescore_runs_the_query_time_path(native, main, halves, seg_queries):
    """After a commit elsewhere the first snapshot's statistics are no longer its
    build's: the plan scores from the payloads.  Its hits are those of a snapshot
    built under the new statistics without tables, bit for bit (the table bounds
    the OLD statistics' scores: pruning on it could drop true hits), and with the
    second snapshot the oracle's segmented search."""
    h = halves
    q_off, terms, want = seg_queries
    re_a = h["own_a"].rescore(h["g"])
    assert re_a.bound_tables() == h["own_a"].bound_tables()  # shared, and not read
    for k in KS:
        x = search(re_a, FORCED, q_off, terms, k)
        y = search(h["seg_a_off"], OFF, q_off, terms, k)
        same_bits(x, y, ("rescored", k))
        old = search(h["own_a"], FORCED, q_off, terms, k)  # (the statistics do differ: the check above has teeth)
        assert any(not np.array_equal(old[0][i, :old[2][i]], x[0][i, :x[2][i]]) for i in range(NQ))
        s, gd, n = merged(native, [re_a, h["seg_b"]], FORCED, q_off, terms, k)
        for i in range(NQ):
            assert_hits(s[i], gd[i], n[i], *want[k][i], ("rescored merged", k, i))
    re_a.close()


def test_plan_over_a_snapshot_with_tables_and_one_without(native, main, halves, seg_queries):
    h = halves
    q_off, terms, want = seg_queries
    for k in KS:
        s, gd, n = merged(native, [h["seg_a_on"], h["seg_b"]], FORCED, q_off, terms, k)
        s0, gd0, n0 = merged(native, [h["seg_a_off"], h["seg_b"]], OFF, q_off, terms, k)
        assert np.array_equal(n, n0)
        for i in range(NQ):
            m = int(n[i])
            assert np.array_equal(gd[i, :m], gd0[i, :m]) and np.array_equal(s[i, :m].view(np.uint32), s0[i, :m].view(np.uint32)), (k, i)
            assert_hits(s[i], gd[i], n[i], *want[k][i], ("two snapshots", k, i))
