"""Pins the cases of test_gpu_seeded_thr.py (seed_cases.py) on the CPU, so that the
device test cannot pass vacuously: enough queries get a non-zero seed, enough
have a strict score drop before the k-th hit (the rows above the k-th score then
return fewer than k) and some have a tie across the k-th position (the exact
seed must keep the tied docs).  Counted with bool_ref alone; the counts of the
big case are those of fugu_amd.synth at its own vocabulary (2^20).
"""
import numpy as np
import pytest

import seed_cases as sc


def test_rows_of_one_list():
    """seeds() and expect() on a hand-made hit list."""
    ws = np.array([9, 7, 7, 5, 5, 5, 3, 2, 2, 1], np.float32)
    full = [(ws, np.arange(10, dtype=np.int64) + 100), (ws[:2], np.array([4, 8], np.int64))]
    sd = sc.seeds(full, 4)
    assert {r: v.tolist() for r, v in sd.items()} == {"zero": [0, 0], "loose": [2, 7], "kth": [5, 0], "half": [7, 7],
                                                      "top": [9, 9]}
    want = {"zero": [(4, 10), (2, 2)], "loose": [(4, 9), (2, 2)], "kth": [(4, 6), (2, 2)], "half": [(3, 3), (2, 2)],
            "top": [(1, 1), (1, 1)]}
    for row in sc.ROWS:
        got = sc.expect(full, sd[row], 4)
        assert [(len(s), c) for s, _, c in got] == want[row], row
        assert all(np.array_equal(d, w[1][:len(d)]) for (_, d, _), w in zip(got, full))
    assert sc.strict_drop(full, 4).tolist() == [True, False] and sc.strict_drop(full, 5).tolist() == [False, False]
    assert sc.tie_across(full, 4).tolist() == [True, False] and sc.tie_across(full, 3).tolist() == [False, False]


def check_rows(case, ref):
    """The rows at or below the k-th score expect the plain top k; those above it the hits at or above the seed."""
    for k in case.ks:
        sd = case.seeds(k)
        drop = case.strict_drop(k)
        for i in range(0, len(case), 7):
            t, o, f = case.queries[i]
            ws, wd = ref.search(t, o, k, f if len(f) else None, seg_bounds=case.bounds, stats=case.stats)
            for row in ("zero", "loose", "kth"):
                es, ed, c = case.expect(sd[row], k)[i]
                assert c >= len(wd) and np.array_equal(ed, wd) and np.array_equal(es.view(np.uint32), ws.view(np.uint32))
            for row in ("half", "top"):
                es, ed, c = case.expect(sd[row], k)[i]
                assert np.array_equal(ed, wd[:len(ed)]) and (sd[row][i] == 0 or (es >= sd[row][i]).all())
                if drop[i]:
                    assert len(ed) == c < k


def share(mask):
    return mask.sum() / len(mask)


def test_edges():
    cs = sc.edges_cases()
    ref = cs["plain"].data["c"]["ref"]
    for name in ("plain", "rescored"):
        case = cs[name]
        check_rows(case, ref)
        assert [int((case.hits() >= k).sum()) for k in case.ks] == [61, 53, 33]
        for k in case.ks:
            nz = case.seeds(k)["kth"] > 0
            assert np.array_equal(nz, case.hits() >= k)
            assert share(nz) >= (0.5 if k == 1000 else 0.75), (name, k)
            assert case.tie_across(k).sum() >= 1, (name, k)
            if k > 1:  # (no hit before the first)
                assert share(case.strict_drop(k)) >= 0.25, (name, k)
    plain = cs["plain"]
    assert [int(plain.strict_drop(k).sum()) for k in (10, 1000)] == [50, 19]
    assert [int(plain.tie_across(k).sum()) for k in (10, 1000)] == [2, 14]
    # other statistics, other scores
    assert all(not np.array_equal(a[0][:1], b[0][:1]) for a, b in zip(plain.full, cs["rescored"].full) if len(a[0]))
    # the facet-filtered queries: must16 matches the live edge docs alone (fewer than 10), so
    # at k >= 10 only should16 and must4_not2_should10 can be seeded; should16 under every
    # facet set has over 1000 hits
    fac = cs["facets"]
    check_rows(fac, ref)
    assert len(fac) == 15 and (fac.hits() > 0).all()
    assert [int((fac.seeds(k)["kth"] > 0).sum()) for k in fac.ks] == [15, 7, 5]
    assert fac.strict_drop(10).sum() >= 5 and fac.tie_across(10).sum() >= 1 and fac.tie_across(1000).sum() >= 1


@pytest.mark.parametrize("which", ["one", "two"])
def test_big(which):
    case = sc.big_cases()[which]
    kinds = np.array(case.data["kinds"])
    assert len(case) == 152 and [int((kinds == x).sum()) for x in ("and3", "and5", "and2", "single", "must_should",
                                                                   "must_not", "or")] == [64, 16, 16, 8, 16, 16, 16]
    assert case.hits().min() >= 1000  # every AND, single-term and OR query: a non-zero seed in every row
    for k in case.ks:
        assert (case.seeds(k)["kth"] > 0).all()
        assert share(case.strict_drop(k)) >= 0.25 and case.tie_across(k).sum() >= 1, k
    ands = (kinds == "and3") | (kinds == "and5")
    if which == "one":
        from seed_cases import big_case
        check_rows(case, big_case()[1])
        # the existing 80 ANDs: a strict drop before the k-th hit
        assert [int(case.strict_drop(k)[ands].sum()) for k in case.ks] == [80, 67, 39]
        assert [int(case.strict_drop(k).sum()) for k in case.ks] == [143, 109, 61]
        assert [int(case.tie_across(k).sum()) for k in case.ks] == [11, 50, 100]
        # every kind of query has a tie across some k and a strict drop before some k
        for x in set(kinds.tolist()):
            assert any(case.tie_across(k)[kinds == x].any() for k in case.ks), x
            assert any(case.strict_drop(k)[kinds == x].any() for k in case.ks), x


def test_ties_and_few():
    for case in sc.tie_cases().values():
        for k in case.ks:
            sd = case.seeds(k)
            assert all((sd[r] > 0).all() and np.array_equal(sd[r], sd["kth"]) for r in sc.ROWS[1:])
            for row in sc.ROWS:  # every seed rank gives the same score: the first k docs
                assert all(np.array_equal(d, np.arange(k)) and c == sc.N_TIE for _, d, c in case.expect(sd[row], k))
    few = sc.few_cases()
    (k,) = few.ks
    assert ((few.hits() > 0) & (few.hits() < k)).all()
    sd = few.seeds(k)
    assert (sd["kth"] == 0).all() and (sd["loose"] > 0).all() and (sd["top"] > 0).all()
    top = few.expect(sd["top"], k)
    assert all(len(s) == c >= 1 and (s == s[0]).all() for s, _, c in top)
    assert sum(c < h for (_, _, c), h in zip(top, few.hits())) == len(few)  # the top row leaves the top-score hits only
