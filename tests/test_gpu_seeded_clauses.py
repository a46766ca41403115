"""k_scan's, k_phrase's, k_bphrase's and k_group's pruning at seeded thresholds
(runs on the MI355X box).  The four kernels keep a key exactly when key >=
threshold and prune only on upper bounds -- k_phrase on field_score at the lead
posting's own tf (the bare weight for an escaped tf byte) plus f_tab[bits] under
a filter, k_group on group_bound of a whole chunk plus f_max after inflate_bound,
k_scan on (largest score, first doc of the tile) -- so, as in
test_gpu_seeded_thr.py, a plan whose starting threshold is the lowest key of a
score s (Plan.seed_thresholds) must return the reference hits with score >= s,
cut to k.  Unseeded, these kernels meet a high threshold only when another work
item of the query published one first; seeded with the exact k-th score every
bound meets the tightest valid threshold from the first work item on.

The cases, seeds and expected lists are seed_clause_cases.py's
(test_seed_clause_cases.py pins them on the CPU); nothing expected comes from a
device run.  run, assert_list and check_case are test_gpu_seeded_thr.py's: per
case and k the unseeded plan against the reference first (counts, doc ids and
score bits; no query may be left out), then a fresh plan per seed row: counts,
doc ids and score bits equal the filtered reference list, and the candidates
written lie in [min(c, k), c] for the c reference hits at or above the seed.
The switches are set through the `on` fixture, which restores what it found.
"""
import numpy as np
import pytest

import filter_clause_ref as fc
import group_ref as gr
import phrase_ref as pr
import seed_clause_cases as scc
import test_gpu_seeded_thr as stt
from test_gpu_seeded_thr import assert_list, check_case, env, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from fugu_amd import native as nat
    if nat.device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    before = set(stt.TOTALS)
    yield nat
    print("\nseeded clause kernels: case / k: candidates written unseeded -> at the exact k-th seed")
    for key, (out, c0, c1) in stt.TOTALS.items():
        if key not in before:
            print(f"  {key[0]} / k={key[2]}: {c0} -> {c1}")


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context((0,))


@pytest.fixture()
def on(native):
    """phrase_clauses, group_clauses and filter_clauses on; the settings found are restored in teardown"""
    fns = (native.phrase_clauses, native.group_clauses, native.filter_clauses)
    was = [f() for f in fns]
    for f in fns:
        f(1)
    yield
    for f, w in zip(fns, was):
        f(w)


def phrase_parts(c, fac, lo=0, hi=None):
    """the from_docs arguments of docs [lo, hi) of a phrase_ref.Synth"""
    hi = c.n if hi is None else hi
    to, tt, tg = c.csr(c.text, c.text_gaps, lo, hi)
    no, nt, ng = c.csr(c.name, c.name_gaps, lo, hi)
    kw = dict(deleted=c.deleted[lo:hi], positions=True, text_gaps=tg, name_gaps=ng)
    if fac is not None:
        kw["facets"] = fc.segment(fac, lo, hi)
    return (to, tt, pr.V, no, nt), kw


def group_parts(c, fac, lo=0, hi=gr.N):
    to, tt, no, nt = c.segment(lo, hi)
    return (to, tt, gr.V, no, nt), dict(deleted=c.deleted[lo:hi], facets=fc.segment(fac, lo, hi))


def parts_of(base, lo, hi):
    fam = scc.family(base)
    if base == "group":
        return group_parts(gr.synth(), fam.fac, lo, hi)
    return phrase_parts(fc.phrase_synth(), fam.fac, lo, hi)


@pytest.fixture(scope="module")
def world(native, ctx):
    """The snapshots, each built once: get("phrase" | "group" | "big" | "scan" | "esc") -> an index,
    get(("split", "phrase" | "group")) -> the three snapshots of that corpus under summed statistics."""
    built = {}

    def make(what):
        with env({}):
            if what in ("phrase", "group"):
                args, kw = parts_of(what, 0, scc.family(what).n)
                return native.Index.from_docs(ctx, *args, **kw)
            if what == "big":
                fam = scc.big_phrase_case().data["fam"]
                args, kw = phrase_parts(fam.synth, fam.fac)
                return native.Index.from_docs(ctx, *args, **kw)
            if what == "esc":
                args, kw = phrase_parts(scc.esc_case().data["synth"], None)
                return native.Index.from_docs(ctx, *args, **kw)
            if what == "scan":
                d = scc.scan_case().data
                return native.Index.from_docs(ctx, d["c"].off, d["c"].tok, d["V"], deleted=d["deleted"], threads=16,
                                              facets=d["facets"])
            base = what[1]
            fam = scc.family(base)
            parts = [parts_of(base, lo, hi) for lo, hi in zip(fam.cuts, fam.cuts[1:])]
            g = None
            for args, kw in parts:
                x = native.docs_stats(*args, facets=kw["facets"])
                g = x if g is None else g + x
            assert np.array_equal(np.asarray(g.df_facet, np.int64), fam.facets.df) and g.n_docs == fam.n
            return [native.Index.from_docs(ctx, *args, global_stats=g, **kw) for args, kw in parts]

    def get(what):
        if what not in built:
            built[what] = make(what)
        return built[what]

    yield get
    for ix in built.values():
        for x in (ix if isinstance(ix, list) else [ix]):
            x.close()


def planner(native, target, case, k):
    q_off, terms, kw = case.batch()
    if isinstance(target, list):
        return lambda: native.Plan(target, q_off, terms, k, **kw)
    return lambda: target.plan(q_off, terms, k, **kw)


INDEX_OF = {"phrase": "phrase", "bphrase": "phrase", "group": "group"}


# ---- the three families on one snapshot, unfiltered and filtered

@pytest.mark.parametrize("k", scc.KS)
@pytest.mark.parametrize("name", scc.FAMILIES)
def test_family(native, world, on, name, k):
    case = scc.family_case(name)
    make_plan = planner(native, world(INDEX_OF[name]), case, k)
    check_case(case, k, make_plan, True, (case.name, "default", k))


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("name", scc.FAMILIES)
def test_filtered(native, world, on, name, k):
    case = scc.filtered_case(name)
    check_case(case, k, planner(native, world(INDEX_OF[name]), case, k), True, (case.name, "default", k))


def test_big_phrase(native, world, on):
    """A lead list of more than 4 x 2048 postings, the query 256 times: several work items of several chunks each"""
    case = scc.big_phrase_case()
    (k,) = case.ks
    check_case(case, k, planner(native, world("big"), case, k), True, (case.name, "default", k))


# ---- k_scan: facet unions and AllQuery; the tile break at equality

@pytest.mark.parametrize("k", [10, 1000])
def test_scan(native, world, k):
    case = scc.scan_case()
    make_plan = planner(native, world("scan"), case, k)
    check_case(case, k, make_plan, True, (case.name, "default", k))


# ---- k_phrase's bound on an escaped tf byte under a live threshold

@pytest.mark.parametrize("k", scc.ESC_KS)
def test_escaped_tf(native, world, on, k):
    case = scc.esc_case()
    check_case(case, k, planner(native, world("esc"), case, k), True, (case.name, "default", k))


# ---- three snapshots of one multi-snapshot plan: the global k-th score as every slot's seed

@pytest.mark.parametrize("merged", [False, True], ids=["slots", "merged"])
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("name", ["phrase", "bphrase", "group", "group filtered"])
def test_three_snapshots(native, world, on, name, k, merged):
    case = scc.split_case(name)
    ixs = world(("split", INDEX_OF[name.split()[0]]))
    check_case(case, k, planner(native, ixs, case, k), True, (case.name, "merged" if merged else "slots", k),
               merged=merged)


# ---- a seeded plan executed twice

@pytest.mark.parametrize("name", ["scan", "phrase", "bphrase", "group", "group filtered"])
def test_replay(native, world, on, name):
    """The seed is plan state and survives the run's own reset."""
    k = 10
    if name == "scan":
        case, ix = scc.scan_case(), world("scan")
    elif name.endswith("filtered"):
        case, ix = scc.filtered_case("group"), world("group")
    else:
        case, ix = scc.family_case(name), world(INDEX_OF[name])
    seed = case.seeds(k)["kth"]
    (a, b), cand = run(case, planner(native, ix, case, k), k, seed=seed, twice=True)
    exp = case.expect(seed, k)
    for got in (a, b):
        for i in range(len(case)):
            assert assert_list(got, i, exp[i][:2], True, ("replay", name, i))
    assert all(min(c, k) <= cand[i] <= c for i, (_, _, c) in enumerate(exp))


# ---- one batch of every shape

def test_mixed_batch(native, world, on):
    """Phrase, phrase-beside, group, filtered, facet-only, AllQuery and plain AND / OR rows in one plan:
    every kernel runs in it, and every row is checked against its own reference, unseeded and at each seed row."""
    case = scc.mixed_case()
    (k,) = case.ks
    make_plan = planner(native, world("phrase"), case, k)
    check_case(case, k, make_plan, True, (case.name, "default", k))


# ---- the kernels read the seed

@pytest.mark.parametrize("kernel", ["k_scan", "k_phrase", "k_bphrase", "k_group"])
def test_library_reads_the_seed(native, world, on, kernel):
    """At the top row every query returns the reference's top-score hits alone, and some query returns fewer
    hits than it does unseeded: a kernel that ignores the plan's starting threshold fails here, it does not skip."""
    k = 10
    name = {"k_scan": "scan", "k_phrase": "phrase", "k_bphrase": "bphrase", "k_group": "group"}[kernel]
    case = scc.scan_case() if name == "scan" else scc.family_case(name)
    make_plan = planner(native, world("scan" if name == "scan" else INDEX_OF[name]), case, k)
    (_, _, n0), _ = run(case, make_plan, k)
    seed = case.seeds(k)["top"]
    got, _ = run(case, make_plan, k, seed=seed)
    exp = case.expect(seed, k)
    want = np.array([len(d) for _, d, _ in exp])
    assert (want < n0).sum() >= max(len(case) // 8, 1), (kernel, "the case decides nothing")
    assert np.array_equal(got[2], want), (kernel, np.flatnonzero(got[2] != want))
    assert (got[2] < n0).any(), kernel
