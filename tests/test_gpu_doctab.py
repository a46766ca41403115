"""k_conj's doc-indexed score tables (DevIndex::dtab, ProbeDesc kPdTab) against
the rank-word path and the CPU oracle (runs on the MI355X box).

A probed clause of a term that has a table reads its score at doc << 2 of the
table instead of rank word -> psc[off + pos].  The table holds the same psc
values, so a build with tables forced wide (FUGU_DOCTAB_DIV=64,
FUGU_DOCTAB_LEAD=0) must return the hits of a build with none
(FUGU_DOCTAB_DIV=0) bit for bit -- scores, doc ids, counts -- and both the
oracle's (ids exact, scores rtol 1e-5).  N = 20,011 docs (no multiple of 32,
2048 or 4096), a vocabulary of 2048 terms so that dozens are dense:
  * AND of 2-5 terms, 256 queries, k = 10 and 100, a table term as the second
    list, as a later one (the deferred flush) and in 2-term queries;
  * a table term as MustNot and as Should, and facet-filtered queries (the
    inline path: no deferred probes);
  * hand-made docs: table terms present in doc 0, doc N - 1 and otherwise only
    at multiples of 32, under a lead list of 2048 + 1 postings (the short last
    chunk probes the table's last entry);
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
FORCED = {"FUGU_DOCTAB_DIV": "64", "FUGU_DOCTAB_LEAD": "0"}
OFF = {"FUGU_DOCTAB_DIV": "0"}
DEFAULT = {}


@contextlib.contextmanager
def env(e):
    """The FUGU_DOCTAB_* environment of a build and of its plans (FUGU_DOCTAB_LEAD
    is read when a plan is made), restored afterwards."""
    keys = ("FUGU_DOCTAB_DIV", "FUGU_DOCTAB_LEAD")
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


@pytest.fixture(scope="module")
def main(native, ctx):
    """The synthetic corpus with a facet field (doc % 5), its three builds, the
    oracle, and the terms the forced build gave tables."""
    from fugu_amd import synth
    from oracle import oracle as orc
    c = synth.corpus(N, V)
    facets = (np.arange(N + 1, dtype=np.uint64), (np.arange(N) % 5).astype(np.uint32), 5)
    ixs = {}
    for name, e in (("forced", FORCED), ("off", OFF), ("default", DEFAULT)):
        with env(e):
            ixs[name] = native.Index.from_docs(ctx, c.off, c.tok, V, threads=16, facets=facets)
    n_tab, tab_bytes = ixs["forced"].doc_tables()
    assert n_tab >= 8 and tab_bytes == n_tab * 4 * ((N + 31) // 32 * 32)  # the forced build really has tables
    assert ixs["off"].doc_tables() == (0, 0)
    assert ixs["forced"].stats().device_bytes - ixs["off"].stats().device_bytes >= tab_bytes
    assert ixs["forced"].stats().n_dense_f32 == 0
    # the tables' terms: the densest, ties by term id (build.cpp choose_doctab_terms)
    df = np.array([ixs["off"].df(t) for t in range(V)])
    tabs = set(np.argsort(-df, kind="stable")[:n_tab].tolist())
    assert all(df[t] * 64 >= N for t in tabs)
    ref = orc.OracleIndex(V, c.off, c.tok, threads=16, facet_off=facets[0], facet_tok=facets[1], n_fterms=5)
    yield dict(c=c, facets=facets, ixs=ixs, tabs=tabs, df=df, ref=ref)
    ref.close()
    for ix in ixs.values():
        ix.close()


def search(ix, e, q_off, terms, k, **kw):
    with env(e):
        return ix.search_batch(q_off, terms, k, **kw)


def test_and_queries(native, main):
    from fugu_amd import synth
    q_off, terms = synth.queries(NQ, 2, 5, max_rank=96, seed_q=1234)
    # where the table terms sit in intersection order (cost = df, stable)
    second = later = two = 0
    for i in range(NQ):
        ts = terms[q_off[i]:q_off[i + 1]].tolist()
        order = sorted(ts, key=lambda t: main["df"][t])
        second += order[1] in main["tabs"]
        later += any(t in main["tabs"] for t in order[2:])
        two += len(ts) == 2 and order[1] in main["tabs"]
    assert second >= 16 and later >= 16 and two >= 4, (second, later, two)
    for k in KS:
        on = search(main["ixs"]["forced"], FORCED, q_off, terms, k)
        off = search(main["ixs"]["off"], OFF, q_off, terms, k)
        dflt = search(main["ixs"]["default"], DEFAULT, q_off, terms, k)
        same_bits(on, off, ("forced", k))
        same_bits(dflt, off, ("default", k))
        rs, rd, rn, _, _ = main["ref"].search_batch(q_off, terms, k, threads=16)
        assert rn.sum() > 0
        vs_oracle(on, (rs, rd, rn), ("forced", k))
        vs_oracle(off, (rs, rd, rn), ("off", k))


def test_occur_mixes_and_facet_filter(native, main):
    df, tabs = main["df"], sorted(main["tabs"], key=lambda t: -main["df"][t])
    plain = [t for t in np.argsort(-df, kind="stable").tolist() if t not in main["tabs"]]
    lead, mid = plain[40], plain[4]  # (rarer than every table term: they lead)
    qs, occ = [], []
    for j, t in enumerate(tabs[:8]):
        u = tabs[(j + 3) % 8]
        qs += [[lead, t], [lead, mid, t], [mid, t], [lead, mid, t, u], [lead, t, u, mid]]
        occ += [[MUST, MUST_NOT], [MUST, MUST, MUST_NOT], [MUST, SHOULD], [MUST, MUST, MUST_NOT, SHOULD],
                [MUST, MUST, SHOULD, MUST_NOT]]
    q_off, terms = flat(qs)
    occur = np.array([x for o in occ for x in o], np.uint8)
    for k in KS:
        on = search(main["ixs"]["forced"], FORCED, q_off, terms, k, occur=occur)
        off = search(main["ixs"]["off"], OFF, q_off, terms, k, occur=occur)
        same_bits(on, off, ("occur", k))
        same_bits(search(main["ixs"]["default"], DEFAULT, q_off, terms, k, occur=occur), off, ("occur default", k))
        rs, rd, rn, _, _ = main["ref"].search_batch(q_off, terms, k, threads=16, occur=occur)
        assert (rn > 0).sum() >= len(qs) // 2  # an Exclude that never fired (or always) would show here
        vs_oracle(on, (rs, rd, rn), ("occur", k))
        vs_oracle(off, (rs, rd, rn), ("occur off", k))
    # facet-filtered conjunctions: 3-term ANDs with 1-2 facet clauses
    fq = [[lead, tabs[j % 8], tabs[(j + 1) % 8]] for j in range(16)] + [[mid, tabs[j % 8]] for j in range(8)]
    fl = [[j % 5] if j % 2 else [j % 5, (j + 2) % 5] for j in range(len(fq))]
    q_off, terms = flat(fq)
    f_off, f_terms = flat(fl)
    for k in KS:
        on = search(main["ixs"]["forced"], FORCED, q_off, terms, k, f_off=f_off, f_terms=f_terms)
        off = search(main["ixs"]["off"], OFF, q_off, terms, k, f_off=f_off, f_terms=f_terms)
        same_bits(on, off, ("facet", k))
        rs, rd, rn, _, _ = main["ref"].search_batch(q_off, terms, k, threads=16, f_off=f_off, f_terms=f_terms)
        assert (rn > 0).all()
        vs_oracle(on, (rs, rd, rn), ("facet", k))


def test_handmade_table_edges(native, ctx):
    """Table terms present in doc 0 and doc N - 1 and otherwise only at multiples
    of 32 (`x`; `xd` also in every doc of [4096, 8192), so it is denser than the
    lead), under a lead list of 2048 + 1 postings whose last chunk holds doc
    N - 1 alone.  The filler vocabulary is uniform and sparse, so exactly the
    hand-made terms get tables."""
    from fugu_amd import synth
    from oracle import oracle as orc
    V0 = 1 << 20
    c = synth.corpus(N, V0, 0.0)
    m32 = np.arange(0, N, 32)
    docs_of = {
        "x": np.union1d(m32, [N - 1]),
        "xd": np.union1d(np.union1d(m32, np.arange(4096, 8192)), [N - 1]),
        "lead": np.unique(np.round(np.linspace(0, N - 1, 2049)).astype(np.int64)),
        "half": np.union1d(np.arange(0, N, 2), [N - 1]),
    }
    assert len(docs_of["lead"]) == 2049 and docs_of["lead"][-1] == N - 1 and (N - 1) % 32
    T = {name: V0 + i for i, name in enumerate(docs_of)}
    extra = [[] for _ in range(N)]
    for name, ds in docs_of.items():
        for d in ds:
            extra[int(d)].append(T[name])
    lens = np.diff(c.off).astype(np.int64) + np.array([len(e) for e in extra])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    tok = np.empty(int(off[-1]), np.uint32)
    src, dst = c.off.astype(np.int64), off.astype(np.int64)
    for d in range(N):
        n_own = int(src[d + 1] - src[d])
        tok[dst[d]:dst[d] + n_own] = c.tok[src[d]:src[d + 1]]
        tok[dst[d] + n_own:dst[d + 1]] = extra[d]
    Vh = V0 + len(T)
    with env(FORCED):
        on = native.Index.from_docs(ctx, off, tok, Vh, threads=16)
    with env(OFF):
        no = native.Index.from_docs(ctx, off, tok, Vh, threads=16)
    assert on.doc_tables()[0] == len(T), on.doc_tables()  # the hand-made terms, and only they, are dense
    qs = [[T["lead"], T["xd"]], [T["lead"], T["half"], T["xd"]], [T["lead"], T["xd"], T["half"]],
          [T["lead"], T["x"]], [T["lead"], T["x"]], [T["lead"], T["half"], T["x"]], [T["x"], T["lead"]],
          [T["x"], T["half"], T["xd"]]]
    occ = [[MUST, MUST], [MUST] * 3, [MUST] * 3, [MUST, MUST_NOT], [MUST, SHOULD], [MUST, MUST, SHOULD], [MUST, MUST],
           [MUST] * 3]
    q_off, terms = flat(qs)
    occur = np.array([x for o in occ for x in o], np.uint8)
    ref = orc.OracleIndex(Vh, off, tok, threads=16)
    for k in KS + (1000,):
        a = search(on, FORCED, q_off, terms, k, occur=occur)
        b = search(no, OFF, q_off, terms, k, occur=occur)
        same_bits(a, b, ("handmade", k))
        rs, rd, rn, _, _ = ref.search_batch(q_off, terms, k, threads=16, occur=occur)
        vs_oracle(a, (rs, rd, rn), ("handmade", k))
        vs_oracle(b, (rs, rd, rn), ("handmade off", k))
    # the first query's hits are lead & xd: doc 0 and doc N - 1 among them
    want = np.intersect1d(docs_of["lead"], docs_of["xd"])
    got = search(on, FORCED, q_off, terms, 1000, occur=occur)
    assert int(got[2][0]) == min(1000, len(want)) and {0, N - 1} <= set(got[1][0, :got[2][0]].tolist())
    assert {0, N - 1} <= set(got[1][6, :got[2][6]].tolist())  # x & lead
    ref.close()
    on.close()
    no.close()


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
    assert re_on.doc_tables() == main["ixs"]["forced"].doc_tables() and re_off.doc_tables() == (0, 0)
    ref = orc.OracleIndex(V, c.off, c.tok, deleted=dl, threads=16)
    q_off, terms = synth.queries(NQ, 2, 4, max_rank=96, seed_q=77)
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
    assert own_a.doc_tables()[0] >= 8 and seg_a_on.doc_tables()[0] >= 8
    assert seg_a_off.doc_tables() == (0, 0) and seg_b.doc_tables() == (0, 0)
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


def test_rescore_runs_the_query_time_path(native, main, halves):
    """After a commit elsewhere the first snapshot's statistics are no longer its
    build's: the plan scores from the payloads.  Its hits are those of a snapshot
    built under the new statistics without tables, bit for bit (the table holds
    the OLD statistics' scores: reading it would show in every score), and with
    the second snapshot the oracle's segmented search."""
    from fugu_amd import synth
    h = halves
    re_a = h["own_a"].rescore(h["g"])
    assert re_a.doc_tables() == h["own_a"].doc_tables()  # shared, and not read
    q_off, terms = synth.queries(NQ, 2, 4, max_rank=96, seed_q=91)
    for k in KS:
        x = search(re_a, FORCED, q_off, terms, k)
        y = search(h["seg_a_off"], OFF, q_off, terms, k)
        same_bits(x, y, ("rescored", k))
        old = search(h["own_a"], FORCED, q_off, terms, k)  # (the statistics do differ: the check above has teeth)
        assert any(not np.array_equal(old[0][i, :old[2][i]], x[0][i, :x[2][i]]) for i in range(NQ))
        s, gd, n = merged(native, [re_a, h["seg_b"]], FORCED, q_off, terms, k)
        for i in range(NQ):
            rs, rd = main["ref"].search(terms[q_off[i]:q_off[i + 1]], k, seg_bounds=h["cuts"])
            assert_hits(s[i], gd[i], n[i], rs, rd, ("rescored merged", k, i))
    re_a.close()


def test_plan_over_a_snapshot_with_tables_and_one_without(native, main, halves):
    from fugu_amd import synth
    h = halves
    q_off, terms = synth.queries(NQ, 2, 5, max_rank=96, seed_q=33)
    for k in KS:
        s, gd, n = merged(native, [h["seg_a_on"], h["seg_b"]], FORCED, q_off, terms, k)
        s0, gd0, n0 = merged(native, [h["seg_a_off"], h["seg_b"]], OFF, q_off, terms, k)
        assert np.array_equal(n, n0)
        for i in range(NQ):
            m = int(n[i])
            assert np.array_equal(gd[i, :m], gd0[i, :m]) and np.array_equal(s[i, :m].view(np.uint32), s0[i, :m].view(np.uint32)), (k, i)
            rs, rd = main["ref"].search(terms[q_off[i]:q_off[i + 1]], k, seg_bounds=h["cuts"])
            assert_hits(s[i], gd[i], n[i], rs, rd, ("two snapshots", k, i))
