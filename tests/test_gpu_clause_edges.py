"""Device search at 6-16 clauses and on the edges of the ranges k_disj reads,
against tests/bool_ref.py (runs on the MI355X box).  The corpora and queries are
clause_edges.py's (test_bool_ref.py pins them, and bool_ref to the fixtures and
the C oracle, on the CPU); the oracle is not used here.

  a. one snapshot under three rank layouts (directory only: every clause through
     k_disj's rescoring; the default: the direct path; all kinds), k = 1 .. 1024, the
     batch of 64, batches of one (kDisjSmallSpread: one tile per item) and the
     batch repeated to 256 queries: the same bits in every batch shape;
  b. the snapshot rescored to the statistics of a namespace three times as
     large: scores at query time from the payloads (escaped tf, name field);
  c. facet clauses of kFmaskChunk - 1, kFmaskChunk and kFmaskChunk + 1 postings on
     k_disj, k_conj and k_scan;
  d. the widest work items: a plan over 64 snapshots and 256 queries has one
     item group per query and snapshot (gpq = max(1, 64 / 64)), so a query of ns
     Should clauses over the 35 tiles of the first snapshot gets items of
     G = min(kDisjMaxGroup = 32, kDisjMaxPairs = 256 / ns, 35) tiles: 32 tiles at 2
     clauses, 32 tiles / 256 pairs at 8, 28 / 252 at 9, 16 / 256 at 16, that is
     ceil(35 / G) = 2, 2, 2 and 3 items; the 63 tiny snapshots hold none of the
     terms and get none.  64 queries of each: 64 * 9 = 576 items;
  e. fg_count_batch on the 16-clause queries;
  f. 16 terms are accepted and 17 refused, by search, a multi-snapshot plan and count.
Counts and doc ids exact, scores within the project's 1e-5 relative.
"""
import numpy as np
import pytest

import bool_ref as br
import clause_edges as ce
import synth_ref as sr
from shard_ref import merge_topk_numpy
from test_gpu_probe_desc import ENVS, ENV_IDS, with_env

pytestmark = pytest.mark.gpu

RTOL = 1e-5
LAYOUTS = {"directory_only": ENVS[ENV_IDS.index("directory_only")], "default": {},
           "all_kinds": ENVS[ENV_IDS.index("all_kinds")]}
SINGLES = ("should16", "must16", "must4_not2_should10")
BITS = {"hits": 0, "same_bits": 0}


@pytest.fixture(scope="module")
def native():
    from fugu_amd import native as nat
    if nat.device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    assert (nat.OCCUR_MUST, nat.OCCUR_SHOULD, nat.OCCUR_MUST_NOT) == (br.MUST, br.SHOULD, br.MUST_NOT)
    return nat


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context((0,))


@pytest.fixture(scope="module")
def case():
    """clause_edges.edges_case() and bool_ref's full hit lists (k = 1024) of its batch."""
    c = dict(ce.edges_case())
    c["want"] = [c["ref"].search(c["qs"][i], c["occ"][i], max(ce.KS)) for i in range(64)]
    return c


@pytest.fixture(scope="module")
def index_of(native, ctx, case):
    """The edges snapshot under a rank layout, built once."""
    c, built = case, {}

    def get(layout):
        if layout not in built:
            built[layout] = with_env(LAYOUTS[layout], lambda: native.Index.from_docs(
                ctx, c["off"], c["tok"], c["V"], name_off=c["name_off"], name_tok=c["name_tok"], deleted=c["deleted"],
                threads=16, facets=c["facets"]))
        return built[layout]

    yield get
    print(f"\nclause edges: {BITS['same_bits']} of {BITS['hits']} compared scores bit-identical to bool_ref")
    for ix in built.values():
        ix.close()


def assert_hits(s, d, n, want, k, what):
    rs, rd = want[0][:k], want[1][:k]
    assert int(n) == len(rd), (what, int(n), len(rd))
    assert np.array_equal(np.asarray(d[:n], np.int64), rd), what
    rel = np.abs(s[:n].astype(np.float64) - rs) / np.maximum(np.abs(rs), 1e-30)
    assert (rel <= RTOL).all(), (what, rel.max())
    BITS["hits"] += len(rd)
    BITS["same_bits"] += int((s[:n].view(np.uint32) == rs.view(np.uint32)).sum())


def same_bits(a, b, what):
    """Two device results of the same queries: equal counts, doc ids and score bits."""
    assert np.array_equal(a[2], b[2]), what
    live = np.arange(a[0].shape[1])[None, :] < a[2][:, None]
    assert np.array_equal(a[1][live], b[1][live]), what
    assert np.array_equal(a[0][live].view(np.uint32), b[0][live].view(np.uint32)), what


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_one_snapshot(native, case, index_of, layout):
    c = case
    ix = index_of(layout)
    if layout == "directory_only":
        assert ix.stats().n_rank_terms == 0
    else:
        assert ix.stats().n_rank_terms > 0
    rep = np.tile(np.arange(64), 4)
    rq_off, rterms, roccur = ce._batch([c["qs"][i] for i in rep], [c["occ"][i] for i in rep])
    for k in ce.KS:
        got = ix.search_batch(c["q_off"], c["terms"], k, occur=c["occur"])
        for i in range(64):
            assert_hits(got[0][i], got[1][i], got[2][i], c["want"][i], k, (layout, k, i))
        for name in SINGLES:  # a batch of one: 16x more, shorter items
            i = c["Q"][name]
            one = ix.search_batch([0, len(c["qs"][i])], c["qs"][i], k, occur=c["occ"][i])
            same_bits(one, tuple(x[i:i + 1] for x in got), (layout, k, name, "batch of one"))
        big = ix.search_batch(rq_off, rterms, k, occur=roccur)  # 256 queries: fewer items per query
        same_bits(big, tuple(x[rep] for x in got), (layout, k, "batch of 256"))


@pytest.mark.parametrize("layout", ["default", "directory_only"])
def test_query_time_scoring(native, case, index_of, layout):
    """The snapshot after commits elsewhere in its namespace: rescored to the
    statistics of the corpus plus 100,000 further docs."""
    c = case
    more = sr.corpus(100_000, c["V"], 1.0, ce.SEED_L + 7, ce.SEED_T + 7)
    g2 = native.docs_stats(c["off"], c["tok"], c["V"], name_off=c["name_off"], name_tok=c["name_tok"], threads=16,
                           facets=c["facets"]) + native.docs_stats(*more, c["V"], threads=16)
    assert g2.n_docs == 3 * c["N"]
    ix = index_of(layout).rescore(g2, deleted=c["deleted"])  # (a rescore states the deletions anew)
    want = [c["ref"].search(c["qs"][i], c["occ"][i], 1000, stats=g2) for i in range(64)]
    assert all(not np.array_equal(w[0][:1], v[0][:1]) for w, v in zip(want, c["want"]) if len(w[0]))  # (other scores)
    for k in (10, 1000):
        s, d, n = ix.search_batch(c["q_off"], c["terms"], k, occur=c["occur"])
        for i in range(64):
            assert_hits(s[i], d[i], n[i], want[i], k, (layout, "rescored", k, i))
    ix.close()


def test_facet_filter(native, case, index_of):
    c = case
    ix = index_of("default")
    texts = [(c["qs"][c["Q"][n]], c["occ"][c["Q"][n]]) for n in SINGLES] + [([], [])]  # (no text: k_scan)
    fsets = ([0], [1], [2], [1, br.MISSING], [br.MISSING, 2])
    qs = [(t, o, f) for f in fsets for t, o in texts]
    q_off, terms, occur = ce._batch([q[0] for q in qs], [q[1] for q in qs])
    f_off = np.cumsum([0] + [len(q[2]) for q in qs]).astype(np.uint32)
    f_terms = np.array([x for q in qs for x in q[2]], np.uint32)
    want = [c["ref"].search(t, o, 1000, f) for t, o, f in qs]
    assert all(len(w[1]) > 0 for w in want)
    for k in (10, 1000):
        s, d, n = ix.search_batch(q_off, terms, k, f_off=f_off, f_terms=f_terms, occur=occur)
        for i in range(len(qs)):
            assert_hits(s[i], d[i], n[i], want[i], k, ("facets", qs[i][2], len(qs[i][0]), k))


def test_widest_work_items(native, ctx):
    import torch
    w = ce.wide_case()
    off, tok, bounds, V, k, nq, S = w["off"], w["tok"], w["bounds"], w["V"], 100, 256, 64
    g = native.docs_stats(off, tok, V, threads=16)
    ixs = []
    for s in range(S):
        b0, b1 = int(bounds[s]), int(bounds[s + 1])
        ixs.append(native.Index.from_docs(ctx, off[b0:b1 + 1] - off[b0], tok[int(off[b0]):int(off[b1])], V, threads=16,
                                          global_stats=g, keep_host=False))
    want = [w["ref"].search(q, [br.SHOULD] * len(q), k, seg_bounds=bounds) for q in w["base"]]
    assert all(len(x[1]) == k and x[1].max() < ce.N_WIDE0 for x in want)
    p = native.Plan(ixs, w["q_off"], w["terms"], k, occur=w["occur"])
    groups = {2: 32, 8: 32, 9: 28, 16: 16}  # clauses -> tiles per item (the docstring's derivation)
    assert p.info().total_chunks == sum(-(-35 // groups[len(q)]) for q in w["qs"]) == 576
    p.execute()
    s, d, n = p.results()
    s, d, n = s.reshape(S, nq, k), d.reshape(S, nq, k), n.reshape(S, nq)
    assert (n[1:] == 0).all()
    for i in range(nq):
        assert_hits(s[0, i], d[0, i], n[0, i], want[i % 4], k, ("slot", i))
    ms, md, msh, mn = merge_topk_numpy(s, d, n, k)
    dev = torch.device("cuda:0")
    os_ = torch.zeros(nq * k, dtype=torch.float32, device=dev)
    od, osh = (torch.zeros(nq * k, dtype=torch.int32, device=dev) for _ in range(2))
    on = torch.zeros(nq, dtype=torch.int32, device=dev)
    p.execute_merged(torch.cuda.current_stream(dev).cuda_stream, os_.data_ptr(), od.data_ptr(), osh.data_ptr(),
                     on.data_ptr())
    torch.cuda.synchronize()
    gs, gd = os_.cpu().numpy().reshape(nq, k), od.cpu().numpy().view(np.uint32).reshape(nq, k)
    gsh, gn = osh.cpu().numpy().reshape(nq, k), on.cpu().numpy()
    for i in range(nq):
        for what, (xs, xd, xsh, xn) in (("slots", (ms, md, msh, mn)), ("merged", (gs, gd, gsh, gn))):
            m = int(xn[i])
            assert_hits(xs[i], xd[i, :m].astype(np.int64) + bounds[xsh[i, :m]], m, want[i % 4], k, (what, i))
    p.close()
    for ix in ixs:
        ix.close()


def test_counts(native, case, index_of):
    c = case
    ix = index_of("default")
    names = [n for n, i in c["Q"].items() if len(c["qs"][i]) == 16]
    assert len(names) >= 10
    qs = [(c["qs"][c["Q"][n]], c["occ"][c["Q"][n]], f) for f in ([], [2], [0, br.MISSING]) for n in names]
    q_off, terms, occur = ce._batch([q[0] for q in qs], [q[1] for q in qs])
    f_off = np.cumsum([0] + [len(q[2]) for q in qs]).astype(np.uint32)
    f_terms = np.array([x for q in qs for x in q[2]], np.uint32)
    cts = [0, 1, 2, br.MISSING]
    total, count = native.count_batch([ix], q_off, terms, cts, f_off=f_off, f_terms=f_terms, occur=occur)
    for i, (t, o, f) in enumerate(qs):
        wt, wc = c["ref"].count(t, o, f, cts)
        assert (int(total[i]), count[i].tolist()) == (wt, wc), (i, f)
    assert total.max() > 10_000 and (total > 0).mean() > 0.8


def test_limits(native, ctx):
    """FG_MAX_TERMS = 16: accepted; 17: FG_EUNSUPPORTED naming the query, the whole batch refused."""
    V = 1 << 12
    ixs = []
    for seed in (1, 2):
        off, tok = sr.corpus(2000, V, 1.0, ce.SEED_L + seed, ce.SEED_T + seed)
        ixs.append(native.Index.from_docs(ctx, off, tok, V, threads=4))
    for occ in (br.MUST, br.SHOULD):
        for bad in (False, True):
            qs = [[1, 2], list(range(16)), [3], list(range(17 if bad else 16)), [4, 5, 6]]
            q_off, terms, occur = ce._batch(qs, [[occ] * len(q) for q in qs])
            calls = (lambda: ixs[0].search_batch(q_off, terms, 10, occur=occur),
                     lambda: native.Plan(ixs, q_off, terms, 10, occur=occur).close(),
                     lambda: native.count_batch(ixs, q_off, terms, occur=occur))
            for call in calls:
                if bad:
                    with pytest.raises(native.Unsupported, match=r"query 3 has 17 terms"):
                        call()
                else:
                    call()
    for ix in ixs:
        ix.close()
