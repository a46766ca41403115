"""Pins the cases of test_gpu_seeded_clauses.py (seed_clause_cases.py) on the CPU,
so that the device test cannot pass vacuously: per family some query's (k+1)-th
hit ties the k-th at every k (the exact seed must keep the tie), at least a third
of the queries have a strict score drop before the k-th hit (the rows above the
k-th score then return fewer than k), at least half have 2k hits (the loose row
is a real seed); the esc queries' expected lists hold docs on both sides of the
escaped tf byte, and the scan case has its AllQuery tie and its short list.
Counted from the references alone.
"""
import numpy as np
import pytest

import filter_clause_ref as fc
import seed_cases as sc
import seed_clause_cases as scc

# queries whose (k+1)-th hit ties the k-th, at k = 1, 10, 100, 1000: floors
TIES = {"phrase": (11, 19, 44, 32), "bphrase": (7, 16, 60, 101), "group": (5, 24, 43, 59)}
TIES_FILTERED_10 = {"phrase": 50, "bphrase": 39, "group": 30}
N_QUERIES = {"phrase": 87 + len(scc.PHRASE_PAIRS), "bphrase": 192, "group": 144}


def check_decides(case, ks_drop=(10, 100)):
    """a third of the queries drop strictly before the k-th hit, half have 2k hits at k = 10; the rows' lists"""
    n = len(case)
    for k in ks_drop:
        if k in case.ks:
            assert 3 * int(case.strict_drop(k).sum()) >= n, (case.name, k, int(case.strict_drop(k).sum()), n)
    assert 2 * int((case.hits() >= 20).sum()) >= n, (case.name, int((case.hits() >= 20).sum()), n)
    for k in case.ks:
        sd = case.seeds(k)
        for row in ("zero", "loose", "kth"):  # at or below the k-th score: the plain top k
            for (es, ed, c), (ws, wd) in zip(case.expect(sd[row], k), case.full):
                assert len(ed) == min(k, len(ws)) and c >= len(ed) and np.array_equal(ed, wd[:len(ed)])
        for i, (es, ed, c) in enumerate(case.expect(sd["top"], k)):
            assert len(es) == 0 or (es == es[0]).all()


@pytest.mark.parametrize("name", scc.FAMILIES)
def test_families(name):
    case = scc.family_case(name)
    assert len(case) == N_QUERIES[name] and case.ks == (1, 10, 100, 1000)
    check_decides(case)
    got = [int(case.tie_across(k).sum()) for k in case.ks]
    assert all(g >= w for g, w in zip(got, TIES[name])), (name, got)
    fl = scc.filtered_case(name)
    assert len(fl) == len(scc.family(name).cases) >= 5 * N_QUERIES[name]
    # (at k = 100 the filters leave fewer long lists: phrase 124 of 585, below a third; the floor is pinned at
    # k = 10, where the filtered cases run their tightest seeds, and the unfiltered families carry k = 100)
    check_decides(fl, ks_drop=(10,))
    assert 8 * int(fl.strict_drop(100).sum()) >= len(fl)
    assert int(fl.tie_across(10).sum()) >= TIES_FILTERED_10[name], (name, int(fl.tie_across(10).sum()))
    assert fl.tie_across(100).any()
    # a filtered list is no copy of the unfiltered one: the facet union's score is in the seed
    i, _ = scc.family(name).cases[0]
    assert not np.array_equal(fl.full[0][0][:1], case.full[i][0][:1]) or len(fl.full[0][0]) == 0


def test_big_phrase():
    case = scc.big_phrase_case()
    assert len(case) == fc.BIG_COPIES >= 256 and case.ks == (10,)
    assert case.hits().min() >= 20 and case.strict_drop(10).any()
    assert len({len(s) for s, _ in case.full}) >= 3  # the filters differ


@pytest.mark.parametrize("name", ["phrase", "bphrase", "group", "group filtered"])
def test_split(name):
    case = scc.split_case(name)
    assert len(case.bounds) == 4 and case.bounds[0] == 0 and case.bounds[-1] == case.data["fam"].n
    check_decides(case)
    assert all(case.tie_across(k).any() for k in case.ks)
    one = scc.filtered_case("group") if name.endswith("filtered") else scc.family_case(name)
    assert len(one) == len(case)
    # the same hits, whatever the cut (the scores' last bits may differ: each snapshot orders its own clauses)
    assert all(len(a[0]) == len(b[0]) for a, b in zip(one.full, case.full))
    for k in case.ks:  # the k-th hit lies in different snapshots for different queries
        kth = np.array([d[k - 1] for _, d in case.full if len(d) >= k])
        assert len(np.unique(np.searchsorted(case.bounds, kth, side="right"))) >= 2, (name, k)


def test_scan():
    case = scc.scan_case()
    names = case.data["names"]
    alive = np.flatnonzero(case.data["deleted"] == 0)
    assert len(alive) < scc.N_SCAN > 2 * 4096 and alive[1] == 3
    s, d = case.full[names.index("all")]
    assert len(s) == len(alive) and (s == 1.0).all() and np.array_equal(d, alive[:sc.KEEP])
    for k in case.ks:  # every seed row of AllQuery is 1.0: bound == threshold == every key
        assert all(case.seeds(k)[r][names.index("all")] == 1.0 for r in sc.ROWS[1:])
    few = case.hits()[names.index("few")]
    assert 0 < few == scc.SCAN_FEW < 10 and case.hits()[names.index("few_and_missing")] == few
    assert {len(f) for _, _, f in case.queries} == {0, 1, 2, 3}
    assert sum(sc.br.MISSING in f for _, _, f in case.queries) == 3
    rest = [i for i, n in enumerate(names) if n not in ("few", "few_and_missing", "all")]
    assert (case.hits()[rest] >= 20).all() and (case.hits()[rest] >= 2000).sum() >= 10
    for k in case.ks:  # a facet union has at most 2^clauses scores: the k-th hit ties the next almost everywhere
        assert case.tie_across(k)[rest].sum() >= 3, k
    # the top score's docs are fewer than 10 for some query with more than 10 hits: the top row returns fewer
    small = [i for i in rest if int((case.full[i][0] == case.full[i][0][0]).sum()) < 10]
    assert len(small) >= 2
    # one score only: the first KEEP docs by doc id, all in the first tile, while the hits reach the last tile
    assert (case.full[names.index("root")][1] >> 12 == 0).all() and case.hits()[names.index("root")] > 4 * 4096


def test_esc():
    case = scc.esc_case()
    c = case.data["synth"]
    names = case.data["names"]
    tf = lambda docs, t: np.array([int((docs[int(d)] == t).sum()) for d in range(c.n)])  # noqa: E731
    ta, tb = tf(c.text, scc.ESC_A), tf(c.text, scc.ESC_B)
    assert all(ta[d] == tb[d] == n for d, n in c.esc_tf.items()) and len(c.esc_tf) == 64
    assert not c.deleted[c.esc_docs].any()
    for name in ("ab", "ba", "aba"):
        s, d = case.full[names.index(name)]
        assert len(s) >= 64
        for k in (10, 100):
            lead = ta[d[:k]]  # (= tb wherever it is large)
            assert (lead >= 255).any() and (lead <= 254).any(), (name, k)
        assert np.isin(d[9], c.esc_docs)  # the 10th hit lies among the long docs
    na = tf(c.name, scc.ESC_N1)
    assert all(na[d] == n for d, n in c.esc_name_tf.items()) and len(c.esc_name_tf) == 8
    s, d = case.full[names.index("name_only")]
    assert len(s) >= 80
    for k in (10, 100):
        assert (na[d[:k]] >= 255).any() and (na[d[:k]] <= 254).any(), k
    text_hits = sum(int(((x[:-1] == scc.ESC_N1) & (x[1:] == scc.ESC_N2)).sum()) for x in c.text if len(x) > 1)
    assert text_hits == 0  # the phrase occurs in names only
    # the [a, b] names: the name field's tf byte escapes too
    nab = tf(c.name, scc.ESC_A)
    top = case.full[names.index("ab")][1][:100]
    assert (nab[top] >= 255).any() and ((nab[top] > 0) & (nab[top] <= 254)).any()
    # beside 10 and 100, ks whose k-th hit is a text-only long doc with tf 256, 255, 254, 253
    s, d = case.full[names.index("ab")]
    assert [c.esc_tf.get(int(d[k - 1]), 0) for k in case.ks] == [400, 256, 255, 254, 253, 0]
    assert all((case.seeds(k)["kth"][:2] > 0).all() for k in case.ks) and case.hits()[names.index("aba")] == 64


def test_mixed():
    case = scc.mixed_case()
    assert case.ks == (10,) and len(case) >= 17
    h = case.hits()
    assert (h > 0).all() and (h >= 10).sum() >= len(case) - 2 and (h < 10).any()
    assert case.strict_drop(10).sum() >= len(case) // 3
