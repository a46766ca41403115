"""The staircase cases decide what they claim (no GPU): everything here comes from
the references and from stair_cases.fill, the model of the kernels' buffers.

- every rising query's scores are one value per 512-doc step and strictly higher on
  each step than on the one before, the falling ones mirror them, the flat ones
  have one score;
- the model's buffer reaches exactly kBufD = 1536 keys at K = 1024 for every rising
  one-item query and never more at any K; at K = 1000 it peaks at K + kRound = 1512
  where a round is kRound LEAD docs (k_scan, k_group, k_gphrase, k_mgroup, k_disj);
- the survivor queues reach their caps exactly;
- the top K of a rising query is its hits regrouped best step first and doc-ascending
  inside a step (the last K hits in lead order where K is whole steps), of a flat one
  its first K docs, of a falling one the leading steps that hold K alive docs;
- in every group query the grouping (or the phrase) decides hits or score bits.
"""
import numpy as np
import pytest

import member_group_ref as mg
import stair_cases as sc

RISING = [c for c in sc.CASES if c.order == "rising"]
FALLING = [c for c in sc.CASES if c.order == "falling"]
FLAT = [c for c in sc.CASES if c.order == "flat"]
SINGLE = [c for c in sc.CASES if c.single and c.order in ("rising", "rising2")]
ids = lambda cs: [c.name for c in cs]  # noqa: E731


def steps_of(case):
    """[(step, the distinct scores of its hits)] over the steps with a hit"""
    d, s = case.hits()
    st = d // sc.STEP
    return [(x, np.unique(s[st == x])) for x in np.unique(st)]


def test_the_listed_queries_are_all_here():
    per = {k: [c.order for c in sc.CASES if c.kernel == k] for k in sc.KERNELS}
    for k in ("k_disj", "k_phrase", "k_bphrase", "k_group", "k_gphrase", "k_mgroup"):
        assert {"rising", "flat", "falling"} <= set(per[k]) | ({"flat"} if k == "k_disj" else set()), (k, per[k])
        assert any(c.single for c in sc.CASES if c.kernel == k and c.order == "rising"), k
    assert per["k_disj"].count("rising") == 3 and per["k_scan"] == ["rising", "rising2", "flat"]
    assert per["k_conj"] == ["rising"]
    assert sum(c.fterms is not None and not c.plain for c in sc.CASES) == 1  # the filtered phrase
    assert sc.KS == (1, 512, 513, 1000, 1024) and max(sc.KS) == sc.KMAXK == sc.KTRUNC
    assert sc.KBUFD == 1536 and sc.KQCAP == 1024 and sc.N == 17 * sc.STEP == 4 * sc.KCHUNK + sc.KROUND


def test_corpus_shape():
    c = sc.corpus()
    assert len(c.text) == sc.N and all(len(t) == sc.DOC_LEN for t in c.text)
    import phrase_ref as pr
    assert pr.TABLE[pr.fieldnorm_id(sc.DOC_LEN)] == sc.DOC_LEN  # an exact fieldnorm table entry
    assert all(int(t[-1]) == sc.FILL for t in c.text)          # no phrase crosses into the next doc
    assert all((np.diff(t.astype(np.int64)) >= 0).all() for t in c.text)  # ascending term ids, repeated by tf
    dele = np.flatnonzero(c.deleted)
    assert len(dele) == sc.N_DELETED >= sc.KBUFD - (1000 + sc.KROUND) and dele.max() < sc.STEP
    assert np.array_equal(c.terms.docs(sc.H), dele)             # h: on the deleted docs alone
    for t in (sc.U, sc.V_, sc.F_, sc.E):
        assert len(c.terms.docs(t)) == sc.N
    for t in (sc.SU, sc.SV):
        assert np.array_equal(c.terms.docs(t), np.arange(sc.N_SHORT)) and sc.N_SHORT == sc.KCHUNK
    for j in range(sc.N_FACETS):
        assert np.array_equal(c.terms.facet_docs(j), np.arange(sc.STEP * j, sc.N_FACET_DOCS))
    assert sc.N_FACET_DOCS == sc.KTILE
    ct = c.world.base.text.counts([sc.U, sc.U], [0, 1])
    assert np.array_equal(ct, np.arange(sc.N) // sc.STEP + 1)   # "t t" counts tf(t) - 1
    lo, a, b, hi = sc.SEG_CUTS
    assert a % sc.STEP and a > sc.KCHUNK and b == 4 * sc.KCHUNK and hi - b == sc.STEP
    lo, a, b, hi = sc.SEG_CUTS_SMALL
    assert a % sc.STEP and a - sc.N_DELETED < 1000 and b - a == 2 * sc.KCHUNK


@pytest.mark.parametrize("case", RISING, ids=ids(RISING))
def test_rising(case):
    st = steps_of(case)
    assert len(st) == (sc.N_SHORT if case.single and case.kernel != "k_scan" else
                       sc.N_FACET_DOCS if case.kernel == "k_scan" else sc.N) // sc.STEP
    assert all(len(v) == 1 for _, v in st), case.name            # identical within a step
    v = [x[0] for _, x in st]
    assert all(a < b for a, b in zip(v, v[1:])), (case.name, v)  # strictly higher on each step


def test_rising_with_a_double_last_plateau():
    st = steps_of(sc.BY_NAME["stair7"])
    v = [x[0] for _, x in st]
    assert all(len(x) == 1 for _, x in st) and all(a < b for a, b in zip(v[:-1], v[1:-1])) and v[-1] == v[-2]


@pytest.mark.parametrize("case", FALLING, ids=ids(FALLING))
def test_falling(case):
    st = steps_of(case)
    assert len(st) == sc.N_STEPS and all(len(v) == 1 for _, v in st), case.name
    v = [x[0] for _, x in st]
    assert all(a > b for a, b in zip(v, v[1:])), (case.name, v)


@pytest.mark.parametrize("case", FLAT, ids=ids(FLAT))
def test_flat(case):
    d, s = case.hits()
    assert len(d) == sc.N - sc.N_DELETED and len(np.unique(s)) == 1, case.name


def test_first_pass_emits_every_hit():
    """lead_rows takes every hit's key from the first pass: its lead list holds every hit"""
    c = sc.corpus()
    for case in sc.CASES:
        if case.leads[0] != "docs":
            assert set(case.hits()[0].tolist()) <= set(c.terms.docs(case.leads[0]).tolist()), case.name


# kernels whose rounds are kRound LEAD docs (or, k_disj, that truncate to K after every round): the deleted docs of
# step 0 leave the first three rounds 32 keys short.  k_phrase and k_bphrase take kRound SURVIVORS per round: the first
# three rounds of a chunk with >= 1536 survivors are full on any corpus, and the count reaches kBufD at every K.
LEAD_ROUNDS = ("k_scan", "k_group", "k_gphrase", "k_mgroup", "k_disj")


@pytest.mark.parametrize("case", SINGLE, ids=ids(SINGLE))
def test_buffer_fill(case):
    rows = sc.lead_rows(case)
    assert case.items() == 1
    top = {K: sc.fill(rows, K, case.kernel)[0] for K in sc.KS}
    assert top[1024] == sc.KBUFD == 1536, top
    assert top[1000] == (1512 if case.kernel in LEAD_ROUNDS else sc.KBUFD), top
    assert max(top.values()) <= sc.KBUFD, top


def test_buffer_fill_of_the_long_lists():
    """the u-led queries, every grouping of chunks the planner can choose: full at K = 1024, never past kBufD"""
    for case in RISING:
        if case.single or case.leads[0] == "docs":
            continue
        rows = sc.lead_rows(case)
        for group in (1, 2, sc.KPHRASE_MAX_GROUP):
            top = {K: sc.fill(rows, K, case.kernel, group)[0] for K in sc.KS}
            assert top[1024] == sc.KBUFD and max(top.values()) <= sc.KBUFD, (case.name, group, top)


def test_queue_fill():
    """The survivor queues reach their caps exactly.  queue[kChunk] of k_phrase / k_bphrase holds a chunk's alive
    lead docs: 2048 on the u-led queries (chunks 1 to 3), 2048 - 32 on the su-led ones, whose only chunk holds the
    deleted docs.  queue[kRound] of k_gphrase / k_mgroup holds a round's docs with an open phrase: 512 on both.
    k_disj's q: a pass starts with fewer than kRound entries waiting and adds at most kRound, so q never holds more
    than kQCap - 1 = 1023 and its last slot is never written; every list here is a multiple of kRound long and every
    posting passes bound 1 while scores rise, so `su sv` (as `u v`, `u v e`) queues and flushes exactly kRound per pass."""
    for case in RISING:
        if case.kernel in ("k_phrase", "k_bphrase"):
            want = sc.KCHUNK - (sc.N_DELETED if case.single else 0)
        elif case.kernel in ("k_gphrase", "k_mgroup"):
            want = 0 if '"h h"' in case.name else sc.KROUND  # (no doc has "h h" open: stage (a) appends every key)
        elif case.name == "su sv":
            want = sc.KROUND
        else:
            continue
        rows = sc.lead_rows(case)
        for K in sc.KS:
            assert sc.fill(rows, K, case.kernel)[1] == want, (case.name, K)
    assert {c.kernel for c in RISING if not c.single and sc.fill(sc.lead_rows(c), 1024, c.kernel)[1] == sc.KCHUNK} \
        == {"k_phrase", "k_bphrase"}
    assert 2 * sc.KROUND - 1 < sc.KQCAP


def test_a_raised_truncation_limit_needs_five_rounds():
    """scan_truncate's in-chunk limit at kTrunc + 1 overflows buf only when a round ends on exactly kTrunc + 1 keys
    and another round follows before the chunk's end: K = 513 (513 + 512), from the fifth round on.  A chunk has
    four rounds, so only k_scan's 8-round tile (and an item of several chunks, from 256 queries a batch on) gets
    there: `stair7` at K = 513 is the query whose dropped key -- one of step 6 -- is in the top K."""
    case = sc.BY_NAME["stair7"]
    s, d = case.search(513)
    assert (d // sc.STEP == 6).sum() == 512 and (d // sc.STEP == 7).sum() == 1
    s, d = sc.BY_NAME["stair8"].search(513)
    assert (d // sc.STEP == 7).sum() == 512 and (d // sc.STEP == 6).sum() == 1


@pytest.mark.parametrize("case", RISING, ids=ids(RISING))
def test_rising_top_k(case):
    """The hits regrouped best step first, doc-ascending inside a step, cut at K.  Where K is a multiple of the step
    these are the last K hits in lead (= doc) order; elsewhere the cut falls inside a plateau and takes its FIRST
    docs: K = 1 is the first doc of the last step, K = 513 the last step and the first doc of the one before."""
    d, s = case.hits()
    assert (np.diff(d) > 0).all()
    st = d // sc.STEP
    regrouped = np.concatenate([d[st == x] for x in sorted(set(st.tolist()), reverse=True)])
    for K in sc.KS:
        got = case.search(K)[1]
        assert np.array_equal(got, regrouped[:K]), (case.name, K)
        if K % sc.STEP == 0:
            assert np.array_equal(np.sort(got), d[-K:]), (case.name, K)
    assert case.search(1)[1][0] == d[-1] - sc.STEP + 1 and case.search(513)[1][-1] == d[-1] - 2 * sc.STEP + 1


@pytest.mark.parametrize("case", FLAT, ids=ids(FLAT))
def test_flat_top_k(case):
    d, _ = case.hits()
    for K in sc.KS:
        assert np.array_equal(case.search(K)[1], d[:K]), (case.name, K)
    for cuts in (sc.SEG_CUTS, sc.SEG_CUTS_SMALL):  # in segments: the first K docs, segment 0 then segment 1
        for K in sc.KS:
            assert np.array_equal(case.search(K, seg_bounds=cuts)[1], d[:K]), (case.name, K)
    small = sc.SEG_CUTS_SMALL[1] - sc.N_DELETED  # one segment under the first cut; two at K = 1000 and 1024 under the second
    assert d[sc.KMAXK - 1] < sc.SEG_CUTS[1] and d[small - 1] < sc.SEG_CUTS_SMALL[1] <= d[small] and 513 < small < 1000


@pytest.mark.parametrize("case", FALLING, ids=ids(FALLING))
def test_falling_top_k(case):
    """wholly inside the leading steps that hold K alive docs: ceil(K / 512) steps but for the deleted docs of step 0"""
    for K in sc.KS:
        steps = -(-(K + sc.N_DELETED) // sc.STEP)
        d = case.search(K)[1]
        assert len(d) == K and d.max() < steps * sc.STEP, (case.name, K)
        assert steps == -(-K // sc.STEP) + (K % sc.STEP == 0 or K % sc.STEP > sc.STEP - sc.N_DELETED)


def flattened(query):
    """every group member a clause of its group's occur"""
    return [(oc, m) for oc, b in query for m in (b[1] if mg.is_group(b) else [b])]


def unphrased(query):
    """every phrase, clause or member, replaced by its first term"""
    first = lambda x: x[1][0] if mg.is_phrase(x) else x  # noqa: E731
    return [(oc, (b[0], [first(m) for m in b[1]])) if mg.is_group(b) else (oc, first(b)) for oc, b in query]


def differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


def test_grouping_decides():
    ref = sc.corpus().ref
    for case in sc.CASES:
        if case.kernel not in ("k_group", "k_gphrase", "k_mgroup"):
            continue
        own = ref.hits(case.query)
        by_group = differs(own, ref.hits(flattened(case.query)))
        if case.kernel == "k_group":
            assert by_group, case.name
        else:
            assert by_group or differs(own, ref.hits(unphrased(case.query))), case.name
            if '"h h"' not in case.name:  # ("h h" matches nowhere: there the grouping alone decides)
                assert differs(own, ref.hits(unphrased(case.query))), case.name  # the phrase decides the bits
