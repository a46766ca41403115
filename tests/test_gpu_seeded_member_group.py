"""k_mgroup's pruning at seeded thresholds (runs on the MI355X box).  The kernel
keeps a key exactly when key >= threshold and prunes only on an upper bound --
mgroup_bound of a whole lead chunk, a phrase member bounded by its field weights,
after inflate_bound -- so, as in test_gpu_seeded_thr.py, a plan whose starting
threshold is the lowest key of a score s (Plan.seed_thresholds) must return the
reference hits with score >= s, cut to k.  Seeded with the exact k-th score the
bound meets the tightest valid threshold from the first work item on.

The cases are member_group_ref's queries of a Must kind (m_any_m, corpus A), a
Should kind (s_any_s, corpus A) and repeat (corpus B: "e e" as a member on the 2047 /
2048 / 2049 / 8193-posting lists; test_member_group_ref.py shows on the CPU that the
chunk bound lies below the k-th score on the last at k = 1); the hit lists are the reference's, and
nothing expected comes from a device run.  run, assert_list and check_case are
test_gpu_seeded_thr.py's: per case and k the unseeded plan against the reference
first (counts, doc ids and score bits; no query may be left out), then a fresh
plan per seed row: counts, doc ids and score bits equal the filtered reference
list, and the candidates written lie in [min(c, k), c] for the c reference hits
at or above the seed.
"""
import functools

import numpy as np
import pytest

import member_group_ref as gp
import seed_clause_cases as scc
import test_gpu_seeded_thr as stt
from test_gpu_seeded_thr import check_case

pytestmark = pytest.mark.gpu
CASES = {"m_any_m": "A", "s_any_s": "A", "repeat": "B"}


@pytest.fixture(scope="module")
def native():
    from fugu_amd import native as nat
    if nat.device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    before = set(stt.TOTALS)
    yield nat
    print("\nseeded k_mgroup: case / k: candidates written unseeded -> at the exact k-th seed")
    for key, (out, c0, c1) in stt.TOTALS.items():
        if key not in before:
            print(f"  {key[0]} / k={key[2]}: {c0} -> {c1}")


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context((0,))


@pytest.fixture()
def on(native):
    """group_clauses and group_member_phrases on; the settings found are restored in teardown"""
    fns = (native.group_clauses, native.group_member_phrases)
    was = [f() for f in fns]
    for f in fns:
        f(1)
    yield
    for f, w in zip(fns, was):
        f(w)


@functools.lru_cache(maxsize=None)
def case_of(kind):
    """the kind's queries with the reference's whole hit lists"""
    w = gp.world(CASES[kind])
    qs = gp.queries(w.name)[kind]
    q_off, terms, occur, plen, ppos = gp.batch(qs)
    full = [scc.ordered(*gp.ref_of(w.name).hits(q)) for q in qs]
    return scc.ClauseCase("mgroup " + kind, gp.KS, (q_off, terms, dict(occur=occur, phrase_len=plen, phrase_pos=ppos)), full)


@pytest.fixture(scope="module")
def index(native, ctx):
    built = {}

    def get(name):
        if name not in built:
            w = gp.world(name)
            args, gaps = w.csr()
            built[name] = native.Index.from_docs(ctx, *args, positions=True, deleted=w.deleted.astype(np.uint8), **gaps)
        return built[name]

    yield get
    for ix in built.values():
        ix.close()


@pytest.mark.parametrize("k", gp.KS)
@pytest.mark.parametrize("kind", list(CASES))
def test_seeded(native, index, on, kind, k):
    case = case_of(kind)
    ix = index(CASES[kind])
    q_off, terms, kw = case.batch()
    check_case(case, k, lambda: ix.plan(q_off, terms, k, **kw), True, (case.name, "default", k))


def test_library_reads_the_seed(native, index, on):
    """At the top row every query returns the reference's top-score hits alone, and some query returns fewer hits
    than it does unseeded: a kernel that ignores the plan's starting threshold fails here."""
    k = 10
    case = case_of("repeat")
    ix = index("B")
    q_off, terms, kw = case.batch()
    make_plan = lambda: ix.plan(q_off, terms, k, **kw)  # noqa: E731
    (_, _, n0), _ = stt.run(case, make_plan, k)
    seed = case.seeds(k)["top"]
    got, _ = stt.run(case, make_plan, k, seed=seed)
    want = np.array([len(d) for _, d, _ in case.expect(seed, k)])
    assert (want < n0).any(), "the case decides nothing"
    assert np.array_equal(got[2], want), np.flatnonzero(got[2] != want)
