"""k_conj's and k_disj's pruning at seeded thresholds, against tests/bool_ref.py
(runs on the MI355X box).  Both kernels keep a key exactly when key >= threshold
and prune only on upper bounds (block maxima, MaxScore bounds, one-byte bound
tables, tile / sub-tile / bucket maxima, the rescore factor, the facet maximum,
inflate_bound's margin, the histogram k-th edge), so a plan whose starting
threshold is the lowest key of a score s (Plan.seed_thresholds) must return the
reference hits with score >= s, cut to k.  Seeded with the exact k-th score every
bound meets the tightest valid threshold from the first work item on, whatever
the scheduling; seeded above it, the result shows that the kernel read the seed.

The cases, seeds and expected lists are seed_cases.py's (test_seed_cases.py pins
them on the CPU); nothing expected comes from a device run.  Per case, k and
setting: the unseeded plan against the reference first (doc ids and counts
exact; score bits in the big, tie and few cases, 1e-5 relative in the edges
cases), then a fresh plan per seed row for the queries whose unseeded scores
were the reference's bits (a reference score is a valid seed only then): counts,
doc ids and score bits equal the filtered reference list, and the candidates
written lie in [min(c, k), c] for the c reference hits at or above the seed.
"""
import contextlib
import os

import numpy as np
import pytest

import seed_cases as sc
from shard_ref import merge_topk_numpy
from test_gpu_clause_edges import LAYOUTS

pytestmark = pytest.mark.gpu

RTOL = 1e-5
ENV_KEYS = ("FUGU_CONJ_HIST_THR", "FUGU_DOCTAB8_DIV", "FUGU_DOCTAB8_LEAD", "FUGU_DOCTAB_DIV", "FUGU_DOCTAB_LEAD",
            "FUGU_RANK_GIB", "FUGU_RANK_PLAIN_DIV")
# the big case's settings: (the environment of the build and of its plans, the build it shares)
SETTINGS = {
    "default": ({}, "default"),
    "hist_thr_off": ({"FUGU_CONJ_HIST_THR": "0"}, "default"),  # (read when a plan is made)
    "bound_tables": ({"FUGU_DOCTAB8_DIV": "64", "FUGU_DOCTAB8_LEAD": "0"}, "bound_tables"),
    "no_bound_tables": ({"FUGU_DOCTAB8_DIV": "0"}, "no_bound_tables"),
    "score_tables": ({"FUGU_DOCTAB_DIV": "64", "FUGU_DOCTAB_LEAD": "0"}, "score_tables"),
    "no_score_tables": ({"FUGU_DOCTAB_DIV": "0"}, "no_score_tables"),
}
TOTALS = {}  # (case, setting, k) -> queries left out, candidates written unseeded / at the exact k-th seed


@contextlib.contextmanager
def env(e):
    """The planner's and builder's settings (read when an index or a plan is made), restored afterwards."""
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    for k in ENV_KEYS:
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
    assert (nat.OCCUR_MUST, nat.OCCUR_SHOULD, nat.OCCUR_MUST_NOT) == (sc.M, sc.S, sc.X)
    yield nat
    print("\nseeded thresholds: case / setting / k: queries left out, candidates written unseeded -> at the exact k-th seed")
    for (name, setting, k), (out, c0, c1) in TOTALS.items():
        print(f"  {name} / {setting} / k={k}: {out} left out, {c0} -> {c1}")


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context((0,))


def test_library_seeds_thresholds(native):
    """Every test below relies on fg_plan_seed_thr0: a library without it fails here, it does not skip."""
    assert hasattr(native._lib, "fg_plan_seed_thr0"), "the library lacks fg_plan_seed_thr0"


def run(case, make_plan, k, seed=None, merged=False, twice=False):
    """One fresh plan, seeded or not: (scores, global docs, counts) per batch query
    and the candidates written per batch query (summed over the snapshots)."""
    nq = len(case)
    bounds = np.array([0] if case.bounds is None else case.bounds, np.int64)
    S = max(len(bounds) - 1, 1)
    p = make_plan()
    assert p.n_batch == nq and p.n_segs == S
    if seed is not None:
        p.seed_thresholds(seed)
    outs = []
    for _ in range(2 if twice else 1):
        if merged:
            import torch
            dev = torch.device("cuda:0")
            os_ = torch.zeros(nq * k, dtype=torch.float32, device=dev)
            od, osh = (torch.zeros(nq * k, dtype=torch.int32, device=dev) for _ in range(2))
            on = torch.zeros(nq, dtype=torch.int32, device=dev)
            p.execute_merged(torch.cuda.current_stream(dev).cuda_stream, os_.data_ptr(), od.data_ptr(), osh.data_ptr(),
                             on.data_ptr())
            torch.cuda.synchronize()
            s, n = os_.cpu().numpy().reshape(nq, k), on.cpu().numpy()
            d, sh = od.cpu().numpy().view(np.uint32).reshape(nq, k), osh.cpu().numpy().reshape(nq, k)
        else:
            p.execute()
            s, d, n = p.results()
            sh = np.zeros((nq, k), np.int32)
            if S > 1:
                s, d, sh, n = merge_topk_numpy(s.reshape(S, nq, k), d.reshape(S, nq, k), n.reshape(S, nq), k)
        live = np.arange(k)[None, :] < np.asarray(n)[:, None]
        gd = np.where(live, d.astype(np.int64) + bounds[np.where(live, sh, 0)], -1)
        outs.append((np.asarray(s, np.float32), gd, np.asarray(n, np.int64)))
    cand = p.candidate_counts().astype(np.int64).reshape(S, nq).sum(0)
    p.close()
    return (outs if twice else outs[0]), cand


def assert_list(got, i, want, bits, what):
    """Query i of a result against (scores, docs): counts and doc ids exact, scores
    by bits or within RTOL.  Returns whether the scores are the reference's bits."""
    (s, d, n), (ws, wd) = got, want
    m = int(n[i])
    assert m == len(wd), (what, i, m, len(wd))
    assert np.array_equal(d[i, :m], wd), (what, i)
    same = np.array_equal(s[i, :m].view(np.uint32), ws.view(np.uint32))
    if bits:
        assert same, (what, i)
    else:
        rel = np.abs(s[i, :m].astype(np.float64) - ws) / np.maximum(np.abs(ws), 1e-30)
        assert (rel <= RTOL).all(), (what, i, rel.max())
    return same


def check_case(case, k, make_plan, bits, what, merged=False):
    """The unseeded run, then every seed row (the module's docstring)."""
    nq = len(case)
    zero = np.zeros(nq, np.float32)
    got, cand0 = run(case, make_plan, k, merged=merged)
    exp = case.expect(zero, k)
    same = np.array([assert_list(got, i, exp[i][:2], bits, (what, "unseeded")) for i in range(nq)])
    assert all(min(c, k) <= cand0[i] <= c for i, (_, _, c) in enumerate(exp)), (what, "unseeded candidates")
    out = int((~same).sum())
    print(f"\n{what}: {out} of {nq} queries left out (unseeded scores not the reference's bits)")
    assert out <= (0 if bits else nq // 8), (what, np.flatnonzero(~same))
    seeds = case.seeds(k)
    for row in sc.ROWS:
        seed = np.where(same, seeds[row], zero).astype(np.float32)
        got, cand = run(case, make_plan, k, seed=seed, merged=merged)
        exp = case.expect(seed, k)
        for i in np.flatnonzero(same):
            assert assert_list(got, i, exp[i][:2], True, (what, row, float(seed[i])))
            c = exp[i][2]
            assert min(c, k) <= cand[i] <= c, (what, row, i, int(cand[i]), c)
        if row == "kth":
            key = (case.name + (" merged" if merged else ""), what[1], k)
            TOTALS[key] = (out, int(cand0.sum()), int(cand.sum()))
            print(f"{what}: candidates written unseeded -> at the exact k-th seed: {cand0.sum()} -> {cand.sum()}")


# ---- edges: k_disj's bound classes, escaped tf, the name field, MustNot, deletions, facets

@pytest.fixture(scope="module")
def edges(native, ctx):
    """The edges snapshot under a rank layout, and rescored to 3x the namespace statistics."""
    cs = sc.edges_cases()
    c = cs["plain"].data["c"]
    built = {}

    def get(layout, rescored):
        if (layout, False) not in built:
            with env(LAYOUTS[layout]):
                built[layout, False] = native.Index.from_docs(
                    ctx, c["off"], c["tok"], c["V"], name_off=c["name_off"], name_tok=c["name_tok"],
                    deleted=c["deleted"], threads=16, facets=c["facets"])
        if rescored and (layout, True) not in built:
            g = cs["rescored"].stats
            g2 = native.docs_stats(c["off"], c["tok"], c["V"], name_off=c["name_off"], name_tok=c["name_tok"], threads=16,
                                   facets=c["facets"]) + native.docs_stats(*cs["rescored"].data["more"], c["V"], threads=16)
            # the statistics the reference scored with
            assert (g2.n_docs, tuple(g2.tot_tokens), g2.tot_facet_tokens) == (g.n_docs, g.tot_tokens, g.tot_facet_tokens)
            assert np.array_equal(g2.df_text, g.df_text) and np.array_equal(g2.df_name, g.df_name)
            assert np.array_equal(g2.df_facet, g.df_facet)
            built[layout, True] = built[layout, False].rescore(g2, deleted=c["deleted"])
        return built[layout, rescored]

    yield cs, get
    for ix in built.values():
        ix.close()


@pytest.mark.parametrize("k", [1, 10, 1000])
@pytest.mark.parametrize("which", ["plain", "rescored", "facets"])
@pytest.mark.parametrize("layout", ["default", "directory_only"])
def test_edges(native, edges, layout, which, k):
    cs, get = edges
    case = cs[which]
    ix = get(layout, which == "rescored")
    assert (get(layout, False).stats().n_rank_terms == 0) == (layout == "directory_only")
    q_off, terms, kw = case.batch()
    check_case(case, k, lambda: ix.plan(q_off, terms, k, **kw), False, (case.name, layout, k))


# ---- big: several work items per query; deferred ANDs, kSingle, Must + Should / MustNot, dense ORs

@pytest.fixture(scope="module")
def big(native, ctx):
    cs = sc.big_cases()
    case = cs["one"]
    c, V = case.data["c"], case.data["V"]
    built = {}

    def get(setting):
        e, build = SETTINGS[setting]
        if build not in built:
            with env(e):
                built[build] = native.Index.from_docs(ctx, c.off, c.tok, V, threads=16)
        return built[build], e

    yield cs, get
    for ix in built.values():
        ix.close()


def test_big_builds(native, big):
    """The forced builds really have tables, the others of that pair none; every lead list is several work items."""
    _, get = big
    n8, b8 = get("bound_tables")[0].bound_tables()
    assert n8 >= 8 and b8 >= n8 * sc.N_BIG
    assert get("no_bound_tables")[0].bound_tables() == (0, 0)
    nt, bt = get("score_tables")[0].doc_tables()
    assert nt >= 8 and bt >= nt * 4 * sc.N_BIG
    assert get("no_score_tables")[0].doc_tables() == (0, 0)
    ix = get("default")[0]
    assert min(ix.df(int(t)) for t in big[0]["one"].data["top"]) >= 3 * 16 * 2048


@pytest.mark.parametrize("k", [10, 100, 1000])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_big(native, big, setting, k):
    cs, get = big
    case = cs["one"]
    ix, e = get(setting)
    q_off, terms, kw = case.batch()

    def make_plan():
        with env(e):
            return ix.plan(q_off, terms, k, **kw)

    check_case(case, k, make_plan, True, (case.name, setting, k))


def test_replay(native, big):
    """A seeded plan executed twice: the seed is plan state and survives the run's own reset."""
    cs, get = big
    case, k = cs["one"], 100
    ix, _ = get("default")
    q_off, terms, kw = case.batch()
    seed = case.seeds(k)["kth"]
    (a, b), cand = run(case, lambda: ix.plan(q_off, terms, k, **kw), k, seed=seed, twice=True)
    exp = case.expect(seed, k)
    for got in (a, b):
        for i in range(len(case)):
            assert assert_list(got, i, exp[i][:2], True, ("replay", i))
    assert all(min(c, k) <= cand[i] <= c for i, (_, _, c) in enumerate(exp))


# ---- ties: bound == threshold == every key

@pytest.fixture(scope="module")
def ties(native, ctx):
    cs = sc.tie_cases()
    d = cs["one"].data
    ixs = [native.Index.from_docs(ctx, d["off"], d["tok"], d["V"], threads=16)]
    yield cs, ixs[0]
    ixs[0].close()


@pytest.mark.parametrize("k", [10, 100])
def test_ties(native, ties, k):
    cs, ix = ties
    case = cs["one"]
    q_off, terms, kw = case.batch()
    check_case(case, k, lambda: ix.plan(q_off, terms, k, **kw), True, (case.name, "default", k))


# ---- two snapshots of one multi-snapshot plan: the global k-th score as every slot's seed

@pytest.fixture(scope="module")
def halves(native, ctx):
    built = {}

    def get(which):
        if which not in built:
            case = (sc.big_cases() if which == "big" else sc.tie_cases())["two"]
            d = case.data
            off, tok = (d["c"].off, d["c"].tok) if which == "big" else (d["off"], d["tok"])
            parts = sc.split(off, tok, case.bounds)
            g = native.docs_stats(*parts[0], d["V"], threads=16) + native.docs_stats(*parts[1], d["V"], threads=16)
            built[which] = (case, [native.Index.from_docs(ctx, o, t, d["V"], threads=16, global_stats=g, keep_host=False)
                                   for o, t in parts])
        return built[which]

    yield get
    for _, ixs in built.values():
        for ix in ixs:
            ix.close()


@pytest.mark.parametrize("merged", [False, True], ids=["slots", "merged"])
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("which", ["big", "ties"])
def test_two_snapshots(native, halves, which, k, merged):
    case, ixs = halves(which)
    q_off, terms, kw = case.batch()
    check_case(case, k, lambda: native.Plan(ixs, q_off, terms, k, **kw), True,
               (case.name, "merged" if merged else "slots", k), merged=merged)


# ---- few: fewer than k matches

def test_few(native, ctx):
    case = sc.few_cases()
    d = case.data
    ix = native.Index.from_docs(ctx, d["c"].off, d["c"].tok, d["V"], threads=16, facets=d["facets"])
    (k,) = case.ks
    q_off, terms, kw = case.batch()
    check_case(case, k, lambda: ix.plan(q_off, terms, k, **kw), True, (case.name, "default", k))
    ix.close()
