"""The top-k kernels on rising, flat and falling score staircases (runs on the
MI355X box): stair_cases.py's corpus and queries against its references on
(doc, score bits) and the hit count, with no tolerance, at every K of stair_cases.KS
(512 and 513 straddle a plateau, 1024 = kTrunc = kMaxK).  test_stair_cases.py shows
without a GPU that these inputs fill the kernels' key buffer to its last slot and
the survivor queues to their caps.  Every test sets the five switches through the
`on` fixture, which restores what it found.

- solo: one query per plan.  The plan's work items are counted (a chunk kernel's
  passes in chunks of kChunk lead postings; one item for the one-tile sweeps), and a
  query led by su / sv or the facet staircase is ONE item: nothing prunes it from
  outside and its buffer fills as the model says.  The plan is then run a second
  time: a replay gives the same rows;
- one batch of every query, the set repeated to 64 slots (k_disj groups tiles as
  for a real batch) and to 256 (from 256 queries on the planner gives a long list
  items of several chunks: a chunk's end, a truncation to K, then more rounds);
- three segments cut on and off the 512 grid, under the corpus' statistics:
  fg_search_sharded and a multi-snapshot plan merged on the host, global doc =
  segment base + local doc.  Two cuts.  (0, 2148, 8192, 8704): one chunk + 100, a
  segment that ends where the fourth chunk does, and the last 512 docs -- the best
  rising docs, the worst falling ones.  (0, 612, 4708, 8704): a first segment
  smaller than K, then one of exactly two chunks.  The flat queries tie every hit
  of every segment with the published score-only threshold: the answer is the
  first K docs, of segment 0 and under the second cut then of segment 1.
"""
import time

import numpy as np
import pytest

import filter_clause_ref as fc
import stair_cases as sc

pytestmark = pytest.mark.gpu
T0 = time.time()


@pytest.fixture(scope="module")
def native():
    from fugu_amd import native as nat
    if nat.device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    yield nat
    print(f"\ntest_gpu_stairs.py: {time.time() - T0:.1f} s wall")


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context((0,))


@pytest.fixture()
def on(native):
    """phrase_clauses, group_clauses, filter_clauses, group_phrase_clauses, group_member_phrases on; restored after"""
    fns = [getattr(native, name) for name in sc.SWITCHES]
    was = [f() for f in fns]
    for f in fns:
        f(1)
    yield
    for f, w in zip(fns, was):
        f(w)


def build(native, ctx, c, lo=0, hi=sc.N, **kw):
    args, gaps = c.world.csr(lo, hi)
    return native.Index.from_docs(ctx, *args, positions=True, deleted=c.deleted[lo:hi].astype(np.uint8),
                                  facets=fc.segment(c.fac, lo, hi), **gaps, **kw)


@pytest.fixture(scope="module")
def world(native, ctx):
    """(corpus, index, {case name: the reference's top 1024}): computed once, shared, never changed"""
    c = sc.corpus()
    return c, build(native, ctx, c), {case.name: case.search(sc.KMAXK) for case in sc.CASES}


@pytest.fixture(scope="module", params=[sc.SEG_CUTS, sc.SEG_CUTS_SMALL], ids=["cut2148", "cut612"])
def segments(request, native, ctx):
    """(the three snapshots under the corpus' statistics, their first docs, {case name: the reference's top 1024 with
    the Musts ordered by each segment's own costs})"""
    c = sc.corpus()
    cuts = list(request.param)
    g = None
    for lo, hi in zip(cuts, cuts[1:]):
        x = native.docs_stats(*c.world.csr(lo, hi)[0], facets=fc.segment(c.fac, lo, hi))
        g = x if g is None else g + x
    own = c.terms.own
    assert (g.n_docs, tuple(g.tot_tokens)) == (own.n_docs, tuple(own.tot_tokens))
    assert np.array_equal(np.asarray(g.df_text, np.int64), own.df_text)
    assert np.array_equal(np.asarray(g.df_facet, np.int64), c.facets.df) and g.tot_facet_tokens == c.facets.tot
    ixs = [build(native, ctx, c, lo, hi, global_stats=g) for lo, hi in zip(cuts, cuts[1:])]
    return ixs, np.array(cuts[:-1], np.int64), {case.name: case.search(sc.KMAXK, seg_bounds=cuts) for case in sc.CASES}


def check(s, d, n, cases, want, k, tag):
    """device rows (s, d, n) against the reference's lists cut at k: the count, then (doc, score bits)"""
    for i, case in enumerate(cases):
        rs, rd = want[case.name]
        rs, rd = rs[:k], rd[:k]
        m = int(n[i])
        assert m == len(rd), (tag, case.name, k, m, len(rd))
        gd, gs = np.asarray(d[i, :m], np.int64), np.asarray(s[i, :m], np.float32).view(np.uint32)
        bad = np.flatnonzero((gd != rd) | (gs != rs.view(np.uint32)))
        assert len(bad) == 0, (tag, case.name, k, len(bad), [(int(x), int(gd[x]), int(rd[x]), float(s[i, x]), float(rs[x]))
                                                           for x in bad[:3]])


def slots(n):
    return [sc.CASES[i % len(sc.CASES)] for i in range(n)]


# ------------------------------------------------------------------ solo, and the replay
@pytest.mark.parametrize("k", sc.KS)
def test_solo_and_replay(native, world, on, k):
    c, ix, want = world
    for case in sc.CASES:
        q_off, terms, kw = sc.batch([case])
        plan = ix.plan(q_off, terms, k, **kw)
        items = plan.info().total_chunks
        if case.items() is not None:  # which kernel runs it: the pass structure, in chunks of its lead lists
            assert items == case.items(), (case.name, case.kernel, items, case.items())
        assert items >= 1 and (items == 1 or not case.single), (case.name, items)
        plan.execute()
        first = plan.results()
        check(*first, [case], want, k, "solo")
        plan.execute()
        again = plan.results()
        check(*again, [case], want, k, "replay")
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first, again)), case.name
        plan.close()


# ------------------------------------------------------------------ one batch of every query
@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("n_slots", [64, 256])
def test_batch_of_every_query(native, world, on, n_slots, k):
    c, ix, want = world
    cases = slots(n_slots)
    assert {x.name for x in cases} == set(sc.BY_NAME)
    q_off, terms, kw = sc.batch(cases)
    plan = ix.plan(q_off, terms, k, **kw)
    plan.execute()
    first = plan.results()
    check(*first, cases, want, k, f"batch of {n_slots}")
    plan.execute()
    check(*plan.results(), cases, want, k, f"batch of {n_slots}, replay")
    plan.close()
    check(*ix.search_batch(q_off, terms, k, **kw), cases, want, k, f"search_batch of {n_slots}")


# ------------------------------------------------------------------ three segments
def merge_slots(ps, pd, pn, base, k):
    """a multi-snapshot plan's slot rows [S * nq, k] merged per query by (score desc, global doc asc)"""
    S = len(base)
    nq = len(pn) // S
    ps, pd, pn = ps.reshape(S, nq, k), pd.reshape(S, nq, k), pn.reshape(S, nq)
    out_s, out_d, out_n = np.zeros((nq, k), np.float32), np.zeros((nq, k), np.int64), np.zeros(nq, np.int64)
    for q in range(nq):
        s = np.concatenate([ps[x, q, :pn[x, q]] for x in range(S)])
        d = np.concatenate([pd[x, q, :pn[x, q]].astype(np.int64) + base[x] for x in range(S)])
        o = np.lexsort((d, -s.astype(np.float64)))[:k]
        out_s[q, :len(o)], out_d[q, :len(o)], out_n[q] = s[o], d[o], len(o)
    return out_s, out_d, out_n


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("n_slots", [64, 256])
def test_three_segments(native, ctx, segments, on, n_slots, k):
    ixs, base, want = segments
    cases = slots(n_slots)
    q_off, terms, kw = sc.batch(cases)
    s, d, sh, n = native.search_sharded(ixs, q_off, terms, k, ctx=ctx, **kw)
    check(s, d.astype(np.int64) + base[sh], n, cases, want, k, f"sharded, {n_slots} slots")
    plan = native.Plan(ixs, q_off, terms, k, **kw)
    plan.execute()
    check(*merge_slots(*plan.results(), base, k), cases, want, k, f"multi-snapshot plan, {n_slots} slots")
    plan.execute()
    check(*merge_slots(*plan.results(), base, k), cases, want, k, f"multi-snapshot plan, {n_slots} slots, replay")
    plan.close()


def test_flat_queries_take_the_first_docs_of_the_first_segments(segments):
    """what the three-segment layout asks of a flat query, in the reference's numbers: the first K alive docs, which
    under the second cut are all of segment 0 and then the first of segment 1"""
    _, base, want = segments
    alive = np.flatnonzero(~sc.corpus().deleted)
    for case in sc.CASES:
        if case.order == "flat":
            assert np.array_equal(want[case.name][1], alive[:sc.KMAXK])
    assert base[1] in (sc.SEG_CUTS[1], sc.SEG_CUTS_SMALL[1])
    assert sc.SEG_CUTS_SMALL[1] < 1000 < alive[sc.KMAXK - 1] < sc.SEG_CUTS[1]
