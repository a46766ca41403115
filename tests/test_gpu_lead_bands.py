"""Score-tiered lead copies (DevIndex::bdoc / bpsc / bcmax) on the
device (runs on the MI355X box): the copies' structure read back through
fg_index_band_read, and k_conj leading from them -- chunk skip on the copy's
chunk maxima, early exit of items that skipped everything -- against
tests/bool_ref.py, with the tiers forced on (FUGU_BAND_DIV / FUGU_BAND_MIN_DOCS)
against off, unseeded and at seeded thresholds (seed_cases.py's rows, the
property of test_gpu_seeded_thr.py: a plan seeded with the lowest key of a score
s returns the reference hits with score >= s cut to k; seeded with the exact k-th
score, whole tiers are skipped from the first work item on).  Nothing expected
comes from a device run.
"""
import contextlib
import os

import numpy as np
import pytest

import seed_cases as sc
from test_gpu_seeded_thr import assert_list, check_case, run

pytestmark = pytest.mark.gpu

BAND_KEYS = ("FUGU_BAND_DIV", "FUGU_BAND_MIN_DOCS", "FUGU_BAND_FRAC", "FUGU_BAND_LEAD", "FUGU_BAND_UB_RATIO",
             "FUGU_BAND_SHARES", "FUGU_BAND_XCD_WEIGHT")
# every term in >= 1/64 of the docs, the 64 densest, whatever the snapshot's size and the copies' bytes,
# and every query of >= 2 lists leads from its copy, whatever its other lists weigh
ON = {"FUGU_BAND_DIV": "64", "FUGU_BAND_MIN_DOCS": "0", "FUGU_BAND_FRAC": "0", "FUGU_BAND_UB_RATIO": "0"}
OFF = {"FUGU_BAND_DIV": "0"}  # nothing built
ALL = {**ON, "FUGU_BAND_DIV": str(1 << 30)}  # every term (the structure test's few)
CHUNK, TIERS, SHARES, DEN, SHIFT = 2048, 5, (4, 8, 12, 14), 16, 16


@contextlib.contextmanager
def env(e):
    """The tier settings (read when an index or a plan is made), restored afterwards."""
    old = {k: os.environ.get(k) for k in BAND_KEYS}
    for k in BAND_KEYS:
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
    assert hasattr(nat._lib, "fg_index_band_read") and hasattr(nat._lib, "fg_plan_tiered_slots")
    return nat


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context((0,))


def planner(make, taken, e):
    """make() under the settings e, noting the plan's tiered-slot count in `taken`."""
    def f():
        with env(e):
            p = make()
        taken.append(p.tiered_slots())
        return p
    return f


# ---- structure

LENGTHS = (1, 2, 2047, 2048, 2049, 3 * 2048 + 1)


@pytest.fixture(scope="module")
def shaped(native, ctx):
    """8,000 docs over 14 terms: term j < 6 in LENGTHS[j] random docs with tf 1-4, eight
    filler terms that vary the doc lengths (so the scores spread), every term tiered."""
    rng = np.random.default_rng(99)
    N, V = 8000, 14
    rows = [[] for _ in range(N)]
    for j, n in enumerate(LENGTHS):
        for d in rng.choice(N, n, replace=False):
            rows[d] += [j] * int(rng.integers(1, 5))
    for d in range(N):
        rows[d] += [6 + int(x) for x in rng.integers(0, 8, int(rng.integers(1, 40)))]
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    tok = np.array([t for r in rows for t in r], np.uint32)
    with env(ALL):
        ix = native.Index.from_docs(ctx, off, tok, V, threads=16)
    yield ix, V
    ix.close()


def test_structure(native, shaped):
    ix, V = shaped
    n, nbytes = ix.lead_bands()
    dfs = [ix.df(t) for t in range(V)]
    assert n == V and dfs[:len(LENGTHS)] == list(LENGTHS)
    assert nbytes == sum(8 * df + 4 * ((df + CHUNK - 1) // CHUNK) for df in dfs)
    for t in range(V):
        doc, s, cmax, cuts = ix.band_read(t)
        sdoc, ss, cmax2, cuts2 = ix.band_read(t, source=True)
        df = dfs[t]
        assert len(doc) == df and np.array_equal(cmax, cmax2) and np.array_equal(cuts, cuts2)
        assert (np.diff(sdoc.astype(np.int64)) > 0).all()
        bits, sbits = s.view(np.uint32), ss.view(np.uint32)
        # a permutation of the term's (doc, score bits)
        o = np.argsort(doc, kind="stable")
        assert np.array_equal(doc[o], sdoc) and np.array_equal(bits[o], sbits), t
        # the cuts against the list sorted by score: cut i is the bin of the ceil(df * share)-th best
        sb = np.sort(sbits >> SHIFT)[::-1]
        want = [int(sb[max(1, -(-df * sh // DEN)) - 1]) for sh in SHARES]
        assert [int(c) for c in cuts] == want, (t, cuts, want)
        # tier-major, docs ascending inside a tier, a tier's scores inside its cuts
        tier = (bits[:, None] >> SHIFT < cuts[None, :]).sum(1)
        assert (np.diff(tier) >= 0).all() and tier[0] == 0, t
        same = np.diff(tier) == 0
        assert (np.diff(doc.astype(np.int64))[same] > 0).all(), t
        # every chunk maximum is its chunk's, bit for bit
        for c in range(len(cmax)):
            assert cmax[c:c + 1].view(np.uint32)[0] == bits[c * CHUNK:(c + 1) * CHUNK].max(), (t, c)
    assert ix.band_read(V + 5) is None


def test_structure_off(native, ctx):
    """FUGU_BAND_DIV=0 builds nothing, and the default leaves a snapshot below FUGU_BAND_MIN_DOCS alone."""
    d = sc.few_cases().data
    for e in (OFF, {}):
        with env(e):
            ix = native.Index.from_docs(ctx, d["c"].off[:4001], d["c"].tok[:int(d["c"].off[4000])], d["V"], threads=16)
        assert ix.lead_bands() == (0, 0) and ix.band_read(0) is None
        ix.close()


# ---- results: the big case (deferred ANDs, two-term ANDs, Must + Should, Must + MustNot)

@pytest.fixture(scope="module")
def big(native, ctx):
    case = sc.big_cases()["one"]
    c, V = case.data["c"], case.data["V"]
    built = {}
    for name, e in (("on", ON), ("off", OFF)):
        with env(e):
            built[name] = native.Index.from_docs(ctx, c.off, c.tok, V, threads=16)
    yield case, built
    for ix in built.values():
        ix.close()


def test_big_builds(native, big):
    case, built = big
    n, nbytes = built["on"].lead_bands()
    assert n >= 8 and built["off"].lead_bands() == (0, 0)
    for t in case.data["top"]:
        assert built["on"].band_read(int(t)) is not None
    s_on, s_off = built["on"].stats().device_bytes, built["off"].stats().device_bytes
    assert 0 <= s_on - s_off - nbytes < 4096  # (counted in device_bytes; 256-B part alignment)


@pytest.mark.parametrize("k", [1, 10, 100, 1000])
def test_big(native, big, k):
    """Tiers on against the reference, unseeded and at every seed row; on against off."""
    case, built = big
    q_off, terms, kw = case.batch()
    taken = []
    check_case(case, k, planner(lambda: built["on"].plan(q_off, terms, k, **kw), taken, ON), True, (case.name, "tiers", k))
    multi = sum(1 for t, o, _ in case.queries if len(t) >= 2 and sc.M in o)
    assert taken and all(x == multi for x in taken), (taken, multi)  # every Must-driven query of >= 2 lists
    off_taken = []
    a, _ = run(case, planner(lambda: built["off"].plan(q_off, terms, k, **kw), off_taken, OFF), k)
    b, _ = run(case, planner(lambda: built["on"].plan(q_off, terms, k, **kw), taken, ON), k)
    c, _ = run(case, planner(lambda: built["on"].plan(q_off, terms, k, **kw), off_taken, {**ON, "FUGU_BAND_LEAD": "0"}), k)
    assert off_taken == [0, 0]
    for x in (b, c):
        assert np.array_equal(a[2], x[2]) and np.array_equal(a[1], x[1])
        assert np.array_equal(a[0].view(np.uint32), x[0].view(np.uint32))


def test_replay(native, big):
    """One seeded plan over tiered leads executed twice."""
    case, built = big
    k = 100
    q_off, terms, kw = case.batch()
    seed = case.seeds(k)["kth"]
    taken = []
    (a, b), cand = run(case, planner(lambda: built["on"].plan(q_off, terms, k, **kw), taken, ON), k, seed=seed, twice=True)
    exp = case.expect(seed, k)
    for got in (a, b):
        for i in range(len(case)):
            assert assert_list(got, i, exp[i][:2], True, ("replay", i))
    assert all(min(c, k) <= cand[i] <= c for i, (_, _, c) in enumerate(exp))
    assert taken[0] > 0


# ---- ties: every chunk bound equals the threshold, nothing may be lost

@pytest.mark.parametrize("k", [10, 100])
def test_ties(native, ctx, k):
    case = sc.tie_cases()["one"]
    d = case.data
    with env(ON):
        ix = native.Index.from_docs(ctx, d["off"], d["tok"], d["V"], threads=16)
    assert all(ix.band_read(t) is not None for t in (1, 2, 3))
    q_off, terms, kw = case.batch()
    taken = []
    check_case(case, k, planner(lambda: ix.plan(q_off, terms, k, **kw), taken, ON), True, (case.name, "tiers", k))
    assert all(x == len(case) for x in taken)
    ix.close()


# ---- few: fewer than k matches, Must + MustNot + Should around rare terms, facets

def test_few(native, ctx):
    case = sc.few_cases()
    d = case.data
    with env(ON):
        ix = native.Index.from_docs(ctx, d["c"].off, d["c"].tok, d["V"], threads=16, facets=d["facets"])
    assert ix.lead_bands()[0] >= 8
    (k,) = case.ks
    q_off, terms, kw = case.batch()
    taken = []
    check_case(case, k, planner(lambda: ix.plan(q_off, terms, k, **kw), taken, ON), True, (case.name, "tiers", k))
    assert all(x >= 8 for x in taken)  # the frequent terms under a facet lead from their copies
    ix.close()


# ---- edges: facet filters, deleted docs, the name field; a rescored snapshot keeps the doc-ordered lists

@pytest.fixture(scope="module")
def edges(native, ctx):
    cs = sc.edges_cases()
    c = cs["plain"].data["c"]
    with env(ON):
        ix = native.Index.from_docs(ctx, c["off"], c["tok"], c["V"], name_off=c["name_off"], name_tok=c["name_tok"],
                                    deleted=c["deleted"], threads=16, facets=c["facets"])
    g2 = native.docs_stats(c["off"], c["tok"], c["V"], name_off=c["name_off"], name_tok=c["name_tok"], threads=16,
                           facets=c["facets"]) + native.docs_stats(*cs["rescored"].data["more"], c["V"], threads=16)
    rs = ix.rescore(g2, deleted=c["deleted"])
    yield cs, ix, rs
    rs.close()
    ix.close()


@pytest.mark.parametrize("which", ["plain", "facets", "rescored"])
def test_edges(native, edges, which):
    cs, ix, rs = edges
    case, k = cs[which], 10
    assert c_deleted(cs) > 0 and ix.lead_bands()[0] > 0
    assert rs.lead_bands() == ix.lead_bands()  # (shared with the rescore, as psc is)
    q_off, terms, kw = case.batch()
    use = rs if which == "rescored" else ix
    taken = []
    check_case(case, k, planner(lambda: use.plan(q_off, terms, k, **kw), taken, ON), False, (case.name, "tiers", k))
    if which == "rescored":
        assert all(x == 0 for x in taken), taken  # query-time scores: the copies hold build-time ones
    else:
        assert all(x > 0 for x in taken), taken


def c_deleted(cs):
    d = cs["plain"].data["c"]["deleted"]
    return 0 if d is None else int(np.asarray(d).sum())


# ---- two snapshots of one plan: per slot, and through the merged select

@pytest.fixture(scope="module")
def halves(native, ctx):
    case = sc.big_cases()["two"]
    d = case.data
    parts = sc.split(d["c"].off, d["c"].tok, case.bounds)
    g = native.docs_stats(*parts[0], d["V"], threads=16) + native.docs_stats(*parts[1], d["V"], threads=16)
    with env(ON):
        ixs = [native.Index.from_docs(ctx, o, t, d["V"], threads=16, global_stats=g, keep_host=False) for o, t in parts]
    yield case, ixs
    for ix in ixs:
        ix.close()


@pytest.mark.parametrize("merged", [False, True], ids=["slots", "merged"])
def test_two_snapshots(native, halves, merged):
    case, ixs = halves
    k = 10
    assert all(ix.lead_bands()[0] >= 8 for ix in ixs)
    q_off, terms, kw = case.batch()
    taken = []
    check_case(case, k, planner(lambda: native.Plan(ixs, q_off, terms, k, **kw), taken, ON), True,
               (case.name, "tiers merged" if merged else "tiers slots", k), merged=merged)
    assert all(x > 0 for x in taken)
