"""Score staircases: a hand-made corpus whose scores RISE, stay FLAT or FALL along
every lead list, the queries that run it through the eight top-k kernels, and a
model of the kernels' local key buffer and survivor queues (test infrastructure;
it calls nothing of libfugu).

Seven kernels keep their local top-k in ScanShared (k_disj: in its twin,
DisjShared): buf[kBufD] holds kTrunc + kRound keys because a round appends at most
kRound keys onto at most kTrunc kept ones, and the survivor queues hold one chunk
(k_phrase, k_bphrase), one round (k_gphrase, k_mgroup) or two passes (k_disj).
Every append is wave_append, which drops a key past the cap without a sign.  The
random corpora never come near these caps: after a few rounds the threshold rejects
nearly every doc.  Here scores rise with the doc id in plateaus of 512 docs, so
every doc enters and every round fills the buffer to its last slot; or they are
flat, so the doc id alone decides, across work items and segments; or they fall,
so the first round sets the final threshold.

The corpus: N = 8704 docs = 17 steps of 512, step s = d // 512: four full
2048-posting lead chunks and a fifth of 512.  Every doc has 64 text tokens (an exact
fieldnorm table entry) and no name, so a score depends on tf or a phrase count
alone.  A doc lists its tokens in ascending term id, each repeated by its tf
(group_ref's convention read by position: "t t" counts tf(t) - 1), and ends in
fillers that no query uses, so no phrase crosses into the next doc.
  u   tf s + 2, every doc            rises
  v   tf s + 1, every doc            rises
  f   tf 18 - s, every doc           falls
  e   tf 2, every doc                flat; "e e" counts 1
  h   tf 1, the deleted docs only    no alive doc holds it: the groups' second member
  su  tf s + 2, docs 0..2047         rises; one lead chunk
  sv  tf s + 1, docs 0..2047         rises; one lead chunk
  eight facet terms, facet j on the docs d >= 512 j of the first 4096: the facet
  union rises in eight plateaus inside one k_scan / k_disj tile
N_DELETED = 32 docs of step 0 are deleted, none elsewhere.

Where this departs from a corpus with su / sv on docs 0..4095, h on the even docs
and a handful of deletions, and why:
  * The planner groups kPhraseMaxGroup chunks into one work item only when a list
    has more chunks than the query's share of items (plan.cpp: G = ceil(chunks /
    per_q), per_q = 64 for a batch of one, 16 for 64 queries, 4 from 256 on), so at
    this size every item is ONE chunk unless the batch holds >= 256 queries.  su
    and sv are therefore one chunk long: a query led by them really is one work
    item in a batch of one, no other item's threshold reaches it and its buffer's
    fill is the model's, on the device too.
  * An item that starts empty appends 3 x 512 keys before its first truncation
    (1024 keys are not "past kTrunc"), whatever K <= 1024 is.  It peaks at
    K + kRound = 1512 for K = 1000 only if at least 24 lead docs of its first three
    rounds append nothing: hence 32 deletions, not a handful.  The same 32 docs are
    missing from the chunk's survivor queue, so k_phrase's and k_bphrase's queue
    reaches its cap on the u-led queries (chunks 1 to 3) and 2048 - 32 on the su-led.
  * u, v, e and f are in every doc, so their idf is ~6e-5 and an h on the even docs
    (idf ~0.7) would decide every order by itself: no step would be one plateau and
    no flat query flat.  With h in every doc the nested sums have the flat sums' bits
    and the grouping decides nothing.  So h is on the 32 deleted docs alone: a member
    with postings that no hit holds.  An any-of group goes on without it, an all-of
    group with it never matches, and the flattened query -- h a clause of its own --
    loses every hit or another score (test_stair_cases.py checks it per query).

`fill` replays ONE work item that sees no foreign threshold, from the kernel
comments (the documented invariant); it proves that the inputs saturate the
structures and is never an expected result: those come from bool_ref.Corpus (term
and facet-only queries), member_group_ref.Ref over group_phrase_ref.World (clause
queries) and filter_clause_ref.Facets (the filtered phrase).
"""
import functools

import numpy as np

import bool_ref as br
import filter_clause_ref as fc
import group_phrase_ref as gp
import member_group_ref as mg

F = np.float32
M, S, X = mg.M, mg.S, mg.X
ANY, ALL = mg.ANY, mg.ALL
T, P, G, Ph = mg.T, mg.P, mg.G, mg.Ph

# ------------------------------------------------------------------ the kernels' constants
KCHUNK = 2048            # fg_internal.h:22 kChunk = kThreads * kItems: the postings of a lead chunk
KPHRASE_MAX_GROUP = 4    # fg_internal.h:213 kPhraseMaxGroup: at most this many lead chunks per work item
KTILE = 4096             # fg_internal.h:173 FG_TILE_SHIFT 12: the docs of a k_disj / k_scan tile
KTRUNC = 1024            # kernels.hip:441 FG_TRUNC -> :446 kTrunc: truncate the local buffer past this
KROUND = 512             # fg_internal.h:184 FG_DISJ_ROUND -> kernels.hip:1260 kRound: postings / docs per pass
KBUFD = KTRUNC + KROUND  # kernels.hip:1261 kBufD: kept keys + one pass of hits
KQCAP = 2 * KROUND       # kernels.hip:1263 kQCap: k_disj's bound-2 queue
KMAXK = 1024             # fg_internal.h:25 kMaxK

STEP = 512
N_STEPS = 17
N = STEP * N_STEPS       # 8704
DOC_LEN = 64
N_SHORT = 2048           # su, sv: docs [0, N_SHORT), one lead chunk
N_FACET_DOCS = 4096
N_FACETS = 8
N_DELETED = 32           # >= kBufD - (1000 + kRound) = 24, see above
U, V_, F_, E, H, SU, SV, FILL = range(8)
V = 8                    # the vocabulary
KS = (1, 512, 513, 1000, 1024)
SEG_CUTS = (0, 2148, 8192, N)   # one chunk + 100; ends on the fourth chunk's end; the last 512 docs
SEG_CUTS_SMALL = (0, 612, 4708, N)  # fewer docs than K; exactly two chunks; the rest
DELETED_DOCS = tuple(16 * i + 5 for i in range(N_DELETED))  # spread over step 0


def tf_of(d):
    s = d // STEP
    tf = {U: s + 2, V_: s + 1, F_: 18 - s, E: 2}
    if d in DELETED_DOCS:
        tf[H] = 1
    if d < N_SHORT:
        tf[SU], tf[SV] = s + 2, s + 1
    return tf


class Corpus:
    def __init__(self):
        self.text = []
        for d in range(N):
            tf = tf_of(d)
            row = [t for t in sorted(tf) for _ in range(tf[t])]
            assert len(row) < DOC_LEN
            self.text.append(np.array(row + [FILL] * (DOC_LEN - len(row)), np.uint32))
        self.deleted = np.zeros(N, bool)
        self.deleted[list(DELETED_DOCS)] = True
        has = np.zeros((N, N_FACETS), bool)
        for j in range(N_FACETS):
            has[STEP * j:N_FACET_DOCS, j] = True
        off = np.zeros(N + 1, np.uint64)
        off[1:] = np.cumsum(has.sum(1))
        self.fac = (off, np.nonzero(has)[1].astype(np.uint32), N_FACETS)
        empty = [np.zeros(0, np.uint32)] * N
        none = [None] * N
        pools = dict(mid=[U, V_, F_, E], rare=[SU, SV, H], name_only=[])
        self.world = gp.World("stairs", V, self.text, none, empty, none, self.deleted, pools, SEG_CUTS)
        self.ref = mg.Ref(self.world.base)
        (to, tt, _, no, nt), _ = self.world.csr()
        self.terms = br.Corpus(V, to, tt, no, nt, deleted=self.deleted.astype(np.uint8), facets=self.fac)
        self.facets = fc.Facets(N, self.fac)
        self.fst = self.facets.stats()


@functools.lru_cache(maxsize=None)
def corpus():
    return Corpus()


# ------------------------------------------------------------------ the queries
STAIR = list(range(N_FACETS))       # the eight-facet staircase: 8 plateaus, the best the last
STAIR7 = list(range(N_FACETS - 1))  # without the last facet: steps 6 and 7 are ONE plateau of 1024 docs


class Case:
    """A query, the kernel that must run it and what its scores do along the lead list.
    query: clauses as member_group_ref's; fterms: its facet filter or None.
    leads: the lead list of each pass (a term id, or "docs" for the doc sweep of k_scan / k_disj / k_conj);
    single: in a batch of one the query is ONE work item, so its buffer's fill is deterministic."""

    def __init__(self, name, kernel, order, query, fterms=None, leads=(), single=False):
        self.name, self.kernel, self.order, self.query, self.fterms = name, kernel, order, query, fterms
        self.leads, self.single = tuple(leads), single

    @property
    def plain(self):
        """term clauses only (or none): bool_ref.Corpus is the reference"""
        return all(not isinstance(b, tuple) for _, b in self.query)

    def hits(self, seg_bounds=None):
        """(docs, scores) of every hit, in doc order per segment: the reference's"""
        c = corpus()
        if self.plain:
            return c.terms._hits([b for _, b in self.query], [oc for oc, _ in self.query], self.fterms, seg_bounds, None)
        d, s = c.ref.hits(self.query, seg_bounds=seg_bounds)
        if self.fterms is not None:
            fs, any_f = c.facets.union(self.fterms, c.fst)
            keep = any_f[d]
            d = d[keep]
            s = (s[keep] + fs[d]).astype(F)
        return d, s

    def search(self, k, seg_bounds=None):
        """top k by (score desc, doc asc): (scores f32, docs)"""
        d, s = self.hits(seg_bounds)
        o = np.lexsort((d, -s))[:k]
        return s[o], d[o]

    def items(self):
        """the query's work items in a batch of one: a chunk kernel's passes cut into chunks of kChunk postings
        (plan.cpp: one chunk per item while a list has no more chunks than the query's share of items); a doc
        sweep over one tile is one item, over more tiles None (the planner's grouping is not restated here)"""
        if self.leads == ("docs",):
            return 1 if self.single else None
        return sum(-(-len(corpus().terms.docs(lead)) // KCHUNK) for lead in self.leads)


def _cases():
    out = []
    add = lambda *a, **kw: out.append(Case(*a, **kw))  # noqa: E731
    # k_disj: a union of term clauses, one sweep over the tiles
    add("su sv", "k_disj", "rising", [T(S, SU), T(S, SV)], leads=["docs"], single=True)
    add("u v", "k_disj", "rising", [T(S, U), T(S, V_)], leads=["docs"])
    add("u v e", "k_disj", "rising", [T(S, U), T(S, V_), T(S, E)], leads=["docs"])
    add("f e", "k_disj", "falling", [T(S, F_), T(S, E)], leads=["docs"])
    # k_scan: no text clause
    add("stair8", "k_scan", "rising", [], fterms=STAIR, leads=["docs"], single=True)
    add("stair7", "k_scan", "rising2", [], fterms=STAIR7, leads=["docs"], single=True)
    add("all", "k_scan", "flat", [], leads=["docs"])
    # k_phrase
    add('"su su"', "k_phrase", "rising", [P(M, [SU, SU])], leads=[SU], single=True)
    add('"u u"', "k_phrase", "rising", [P(M, [U, U])], leads=[U])
    add('"e e"', "k_phrase", "flat", [P(M, [E, E])], leads=[E])
    add('"f f"', "k_phrase", "falling", [P(M, [F_, F_])], leads=[F_])
    add('"su su" / stair8', "k_phrase", "rising", [P(M, [SU, SU])], fterms=STAIR, leads=[SU], single=True)
    # k_bphrase: a phrase beside a term
    add('+"su su" +sv', "k_bphrase", "rising", [P(M, [SU, SU]), T(M, SV)], leads=[SU], single=True)
    add('"u u" v', "k_bphrase", "rising", [P(S, [U, U]), T(S, V_)], leads=[U, V_])
    add('"e e" h', "k_bphrase", "flat", [P(S, [E, E]), T(S, H)], leads=[E, H])
    add('+"f f" +e', "k_bphrase", "falling", [P(M, [F_, F_]), T(M, E)], leads=[F_])
    # k_group: a group of terms
    add("+(su | h) +sv", "k_group", "rising", [G(M, ANY, [SU, H]), T(M, SV)], leads=[SV], single=True)
    add("(u & v) (e & h)", "k_group", "rising", [G(S, ALL, [U, V_]), G(S, ALL, [E, H])], leads=[U, H])
    add("+(e | h) +e", "k_group", "flat", [G(M, ANY, [E, H]), T(M, E)], leads=[E])
    add("+(f | h) +e", "k_group", "falling", [G(M, ANY, [F_, H]), T(M, E)], leads=[E])
    # k_gphrase: a group beside a phrase
    add('+"su su" +(sv | h)', "k_gphrase", "rising", [P(M, [SU, SU]), G(M, ANY, [SV, H])], leads=[SU], single=True)
    add('"u u" (v | h)', "k_gphrase", "rising", [P(S, [U, U]), G(S, ANY, [V_, H])], leads=[U, V_, H])
    add('"e e" (e | h)', "k_gphrase", "flat", [P(S, [E, E]), G(S, ANY, [E, H])], leads=[E, E, H])
    add('+"f f" +(e | h)', "k_gphrase", "falling", [P(M, [F_, F_]), G(M, ANY, [E, H])], leads=[F_])
    # (no alive doc holds h, so no doc has "h h" open: every key is appended by stage (a)'s lanes, none by the waves)
    add('+(u | h) +v "h h"', "k_gphrase", "rising", [G(M, ANY, [U, H]), T(M, V_), P(S, [H, H])], leads=[V_])
    # k_mgroup: a phrase as a group member
    add('+("su su" | h) +sv', "k_mgroup", "rising", [G(M, ANY, [Ph([SU, SU]), H]), T(M, SV)], leads=[SV], single=True)
    add('("u u" | h) v', "k_mgroup", "rising", [G(S, ANY, [Ph([U, U]), H]), T(S, V_)], leads=[U, H, V_])
    add('("e e" | h) e', "k_mgroup", "flat", [G(S, ANY, [Ph([E, E]), H]), T(S, E)], leads=[E, H, E])
    add('+("f f" | h) +e', "k_mgroup", "falling", [G(M, ANY, [Ph([F_, F_]), H]), T(M, E)], leads=[E])
    add('+("h h" | u) +v', "k_mgroup", "rising", [G(M, ANY, [Ph([H, H]), U]), T(M, V_)], leads=[V_])  # stage (a) again
    # k_conj: the control (test_gpu_doctab8.py has its staircase)
    add("+u +v", "k_conj", "rising", [T(M, U), T(M, V_)], leads=["docs"])
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
KERNELS = ("k_disj", "k_scan", "k_phrase", "k_bphrase", "k_group", "k_gphrase", "k_mgroup", "k_conj")
SWITCHES = ("phrase_clauses", "group_clauses", "filter_clauses", "group_phrase_clauses", "group_member_phrases")


def batch(cases):
    """(q_off, terms, kw): the fg_query_batch arrays of the cases, their facet filters included"""
    q_off, terms, occur, plen, ppos = mg.batch([c.query for c in cases])
    f_off, f_terms = fc.filter_arrays([c.fterms for c in cases])
    return q_off, terms, dict(occur=occur, phrase_len=plen, phrase_pos=ppos, f_off=f_off, f_terms=f_terms)


# ------------------------------------------------------------------ the model of the buffers
def key_of(score, doc):
    """make_key: score bits above the complemented doc id, so at equal score the lower doc id is the larger key"""
    return (int(np.float32(score).view(np.uint32)) << 32) | (0xFFFFFFFF - int(doc))


def fill(lead, K, kernel, group=1):
    """Replay one pass of a query over its lead list as work items of `group` chunks that see no foreign threshold.
    lead: per lead posting in list order (key, queued): key the doc's key if this pass emits it else None (deleted,
          no match, another pass's); queued whether the doc waits in the kernel's survivor queue first.
    The kernels, from their comments:
      k_scan, k_group    a lane per lead doc, kRound docs, scan_truncate(limit kTrunc); at the chunk's (k_scan: the
                         tile's) end scan_truncate(limit K)
      k_gphrase, k_mgroup  the same rounds; a round's docs with an open phrase wait in queue[kRound], then append
      k_phrase, k_bphrase  the chunk's survivors wait in queue[kChunk]; then kRound SURVIVORS per round
      k_disj             postings past bound 1 wait in q[kQCap]; once kRound wait, kRound of them are scored and
                         appended, then disj_truncate(limit K): `lead` is the clause-0 segment of one tile
    A round appends the keys >= the threshold; a truncation past its limit keeps the K largest and raises the
    threshold to the K-th.  Returns (largest buffer count, largest queue count) over the items."""
    per_item = KCHUNK * group if kernel != "k_scan" else KTILE * 32
    chunk = KCHUNK if kernel not in ("k_scan", "k_disj") else KTILE
    top_buf = top_q = 0
    for i0 in range(0, len(lead), per_item):
        buf, thr = [], 0

        def truncate(limit):
            nonlocal buf, thr
            if len(buf) > limit:
                buf = sorted(buf, reverse=True)[:K]
                thr = max(thr, buf[-1])

        def append(keys):
            nonlocal top_buf
            buf.extend(k for k in keys if k is not None and k >= thr)
            top_buf = max(top_buf, len(buf))

        for c0 in range(i0, min(i0 + per_item, len(lead)), chunk):
            part = lead[c0:c0 + chunk]
            if kernel in ("k_phrase", "k_bphrase"):
                q = [k for k, queued in part if queued]
                top_q = max(top_q, len(q))
                for r0 in range(0, len(q), KROUND):
                    append(q[r0:r0 + KROUND])
                    truncate(KTRUNC)
            elif kernel == "k_disj":
                q = []
                for r0 in range(0, len(part), KROUND):
                    q += [k for k, queued in part[r0:r0 + KROUND] if queued]
                    top_q = max(top_q, len(q))
                    last = r0 + KROUND >= len(part)
                    while len(q) >= KROUND or (last and q):
                        append(q[:KROUND])
                        q = q[KROUND:]
                        truncate(K)
            else:
                for r0 in range(0, len(part), KROUND):
                    rnd = part[r0:r0 + KROUND]
                    top_q = max(top_q, sum(1 for _, queued in rnd if queued))
                    append([k for k, _ in rnd])
                    truncate(KTRUNC)
            truncate(K)
    return top_buf, top_q


def lead_rows(case):
    """fill's `lead` for the case's FIRST pass, which emits every hit (its clause matches every hit): the pass's lead
    list (or the first tile's docs) with the reference's keys.  A doc waits in a queue when it is alive and holds every
    term the queue's stage asks for; here every doc of a lead list holds the phrase's term twice, so that is: alive,
    for the kernels that have a queue."""
    c = corpus()
    d, s = case.hits()
    key = {int(x): key_of(y, x) for x, y in zip(d, s)}
    lead = case.leads[0]
    docs = range(min(KTILE, N)) if lead == "docs" else [int(x) for x in c.terms.docs(lead)]
    queue = case.kernel in ("k_phrase", "k_bphrase", "k_disj")
    if case.kernel in ("k_gphrase", "k_mgroup"):  # open: the doc holds every term of some phrase, clause or member
        phrases = [x for _, b in case.query for x in ([b] if mg.is_phrase(b) else b[1] if mg.is_group(b) else [])
                   if mg.is_phrase(x)]
        has = lambda t: set(int(y) for y in c.terms.docs(t))  # noqa: E731
        opened = set().union(*[set.intersection(*[has(t) for t in ph[1]]) for ph in phrases])
        return [(key.get(x), x in opened and not c.deleted[x]) for x in docs]
    if case.kernel == "k_disj":  # clause 0's postings of the tile; a deleted doc waits too (doc_alive is bound 2's)
        docs = [x for x in docs if x in set(int(y) for y in c.terms.docs(case.query[0][1]))]
        return [(key.get(x), True) for x in docs]
    return [(key.get(x), queue and not c.deleted[x]) for x in docs]
