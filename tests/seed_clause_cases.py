"""The cases of the seeded-threshold tests of k_scan, k_phrase, k_bphrase and
k_group (test_seed_clause_cases.py on the CPU, test_gpu_seeded_clauses.py on the
device).  seed_cases.py says what a seed row is; this module only supplies, per
case, the batch and `full`: the reference's whole hit list per query (all the
scores f32 descending, the docs of the first KEEP hits) in (score desc, doc asc)
order.  The lists come from the references that exist already (phrase_ref,
bool_phrase_ref, group_ref, filter_clause_ref, bool_ref); nothing expected
comes from a device run.

  phrase, bphrase, group   the family corpora and queries of filter_clause_ref, unfiltered
  filtered                 its (query, filter) cases: the seed is a whole score, text + facet union
  big phrase               its 20,000-doc corpus, one phrase 256 times: several work items per query
  scan                     facet-only queries and AllQuery over five 4096-doc tiles with deletions
  esc                      phrases in docs whose lead tf straddles the escaped tf byte (255)
  two snapshots            the family corpora cut at their tests' bounds, the global k-th score as seed
  mixed                    one batch of every shape on the phrase corpus
"""
from __future__ import annotations

import functools

import numpy as np

import bool_phrase_ref as bpr
import bool_ref as br
import filter_clause_ref as fc
import group_ref as gr
import phrase_ref as pr
import seed_cases as sc
import synth_ref as sr

F = np.float32
KEEP = sc.KEEP
KS = (1, 10, 100, 1000)
FAMILIES = ("phrase", "bphrase", "group")


def ordered(docs, scores):
    """A `full` entry of (docs, scores) in any order."""
    d, s = np.asarray(docs, np.int64), np.asarray(scores, F)
    o = np.lexsort((d, -s))
    return s[o], d[o][:KEEP]


class ClauseCase:
    """seed_cases.Case with the hit lists given: `args` = (q_off, terms, keyword
    arguments of Index.plan / Plan after k); bounds: the snapshots' doc ranges
    (None: one snapshot), the docs of `full` are global then."""

    def __init__(self, name, ks, args, full, bounds=None, **data):
        self.name, self.ks, self.args, self.full, self.data = name, tuple(ks), args, full, data
        self.bounds = None if bounds is None else np.array(bounds, np.int64)
        assert len(full) == len(args[0]) - 1 and max(self.ks) <= KEEP
        assert all(len(d) == min(len(s), KEEP) and (np.diff(s) <= 0).all() for s, d in full)

    def __len__(self):
        return len(self.full)

    def batch(self):
        return self.args

    def hits(self):
        return np.array([len(ws) for ws, _ in self.full])

    def seeds(self, k):
        return sc.seeds(self.full, k)

    def expect(self, seed, k):
        return sc.expect(self.full, seed, k)

    def strict_drop(self, k):
        return sc.strict_drop(self.full, k)

    def tie_across(self, k):
        return sc.tie_across(self.full, k)


def batch_of(name, queries, flists=None, synth=None):
    """(q_off, terms, kw) of a family's queries, with filter lists or without"""
    if name == "phrase":
        q_off, terms, plen, ppos = (synth or fc.phrase_synth()).batch(queries)
        kw = dict(phrase_len=plen, phrase_pos=ppos)
    else:
        q_off, terms, occur, plen, ppos = (bpr if name == "bphrase" else gr).batch(queries)
        kw = dict(occur=occur, phrase_len=plen, phrase_pos=ppos)
    if flists is not None:
        kw["f_off"], kw["f_terms"] = fc.filter_arrays(flists)
    return q_off, terms, kw


# filter_clause_ref.phrase_queries' 87 queries mostly have fewer than 100 hits: 13 have a strict score drop
# before the 100th, fewer than the third test_seed_clause_cases.py asks for.  Two-term phrases of frequent terms
# tie at that rank more often than not (few distinct counts and fieldnorms); these 30 are the first, in (a, b)
# order over terms below 30, whose phrase_ref list (117 to 4000 hits) drops strictly before its 100th hit.
PHRASE_PAIRS = [([a, b], [0, 1]) for a, b in (
    (0, 13), (0, 15), (0, 22), (0, 27), (1, 1), (1, 3), (1, 18), (1, 23), (2, 6), (2, 9), (2, 18), (2, 24), (3, 1), (3, 2),
    (3, 9), (3, 14), (3, 26), (3, 27), (4, 0), (4, 3), (4, 4), (4, 17), (4, 18), (5, 7), (6, 3), (6, 4), (6, 6), (6, 17),
    (6, 18), (7, 1))]


@functools.lru_cache(maxsize=None)
def phrase_family():
    c = fc.phrase_synth()
    base = fc.phrase_family()
    more = [q for q in PHRASE_PAIRS if q not in base.queries]
    return fc.Family("k_phrase", c.n, fc.PHRASE_CUTS, base.queries + more, base.hits + fc.phrase_hits(c, more))


def family(name):
    return {"phrase": phrase_family, "bphrase": fc.bphrase_family, "group": fc.group_family}[name]()


# ---- the three families, unfiltered and with their filter cases; one snapshot

@functools.lru_cache(maxsize=None)
def family_case(name):
    """Every query of the family without a filter (group: gr.KINDS' queries, LONG_LEAD_QUERY among them)."""
    fam = family(name)
    assert name != "group" or fc.LONG_LEAD_QUERY in fam.queries
    return ClauseCase(name, KS, batch_of(name, fam.queries), [ordered(d, s) for d, s in fam.hits])


@functools.lru_cache(maxsize=None)
def filtered_case(name):
    fam = family(name)
    full = [(s, d[:KEEP].astype(np.int64)) for s, d in (fam.want(case, fam.n) for case in fam.cases)]
    args = batch_of(name, [fam.queries[i] for i, _ in fam.cases], [f for _, f in fam.cases])
    return ClauseCase(name + " filtered", (10, 100), args, full)


@functools.lru_cache(maxsize=None)
def big_phrase_case():
    fam = fc.big_phrase_family()
    want = {tuple(f): fam.want((0, list(f)), fam.n) for f in fc.BIG_FILTERS}  # once per distinct filter
    full = [(want[tuple(f)][0], want[tuple(f)][1][:KEEP].astype(np.int64)) for _, f in fam.cases]
    args = batch_of("phrase", [fam.queries[i] for i, _ in fam.cases], [f for _, f in fam.cases], synth=fam.synth)
    return ClauseCase("big phrase filtered", (10,), args, full, fam=fam)


# ---- the families as three snapshots under summed statistics

@functools.lru_cache(maxsize=None)
def split_case(name):
    """phrase, bphrase, group: unfiltered; "group filtered": fc.group_family()'s cases.  The reference runs
    with seg_bounds (a phrase's score does not depend on the cut: phrase_ref has no clause order to choose)."""
    base = name.split()[0]
    fam = family(base)
    if base == "phrase":
        hits = fam.hits
    elif base == "bphrase":
        ref = bpr.of_synth(fc.phrase_synth())
        hits = [ref.hits(q, seg_bounds=fam.cuts) for q in fam.queries]
    else:
        ref = gr.Ref(gr.synth().corpus)
        hits = [ref.hits(q, seg_bounds=fam.cuts) for q in fam.queries]
    if name.endswith("filtered"):
        full = [(s, d[:KEEP].astype(np.int64)) for s, d in (fam.want(case, fam.n, hits=hits) for case in fam.cases)]
        args = batch_of(base, [fam.queries[i] for i, _ in fam.cases], [f for _, f in fam.cases])
    else:
        full = [ordered(d, s) for d, s in hits]
        args = batch_of(base, fam.queries)
    return ClauseCase(name + ", three snapshots", (10, 100), args, full, bounds=fam.cuts, fam=fam)


# ---- scan: no text terms

N_SCAN = sc.N_FEW
SCAN_FEW = 5  # docs of the added facet term
SCAN_QUERIES = {  # facet terms (synth_ref.facet_vocab ids; the last id is the added term)
    "root": [0], "ns": [2], "org": [22], "proj": [29],
    "two": [2, 20], "two_rare": [24, 8], "three": [3, 21, 22], "three_rare": [5, 24, 30],
    "missing": [br.MISSING, 23], "missing_first_of_three": [br.MISSING, 4, 21],
    "few": None,  # the added term alone: SCAN_FEW docs, fewer than k = 10
    "few_and_missing": None,
    "few_or_org": None,  # the added term beside frequent ones: the top scores are its few docs'
    "few_or_root_org": None,
    "all": [],  # AllQuery
}


@functools.lru_cache(maxsize=None)
def scan_case():
    """seed_cases.few_case()'s corpus (20,000 docs: five 4096-doc tiles) with a deletion vector and one
    more facet term on SCAN_FEW docs, one of them deleted."""
    from fugu_amd import synth
    V = 1 << 16
    c = synth.corpus(N_SCAN, V)
    fo, ft, nf = sr.facet_tokens(N_SCAN, 4242)
    r = np.random.default_rng(99)
    few_docs = np.sort(r.choice(N_SCAN, SCAN_FEW + 1, replace=False))
    ft = np.insert(ft, fo[few_docs + 1].astype(np.int64), nf).astype(np.uint32)
    add = np.zeros(N_SCAN + 1, np.uint64)
    add[few_docs + 1] = 1
    fo = (fo + np.cumsum(add)).astype(np.uint64)
    deleted = (r.random(N_SCAN) < 0.04).astype(np.uint8)
    deleted[few_docs] = 0
    deleted[few_docs[2]] = 1
    deleted[:3] = (0, 1, 1)  # the first alive docs are 0 and 3
    facets = (fo, ft, nf + 1)
    ref = br.Corpus(V, c.off, c.tok, deleted=deleted, facets=facets)
    names = list(SCAN_QUERIES)
    sets = dict(SCAN_QUERIES, few=[nf], few_and_missing=[br.MISSING, nf], few_or_org=[nf, 22], few_or_root_org=[0, nf, 22])
    qs = [([], [], sets[n]) for n in names]
    case = sc.Case("scan", (10, 1000), qs, ref, c=c, V=V, facets=facets, deleted=deleted, names=names)
    return case


# ---- esc: the lead posting's tf byte at and around its escape value

N_ESC = 3000
ESC_A, ESC_B, ESC_N1, ESC_N2 = 20, 21, 60, 61  # two mid-frequency text terms; two name-only ids
ESC_COUNTS = (120, 253, 254, 255, 256, 300, 400)
ESC_NAME_COUNTS = (253, 254, 254, 255, 255, 256, 300, 120)
# 10 and 100, and ranks among the text-only long docs: the k-th score is then a class of docs whose count IS the
# lead tf, below, at and above the escape value (bound == score == threshold for the tf bytes below it)
ESC_KS = (10, 32, 40, 48, 56, 100)
ESC_QUERIES = {"ab": ([ESC_A, ESC_B], [0, 1]), "ba": ([ESC_B, ESC_A], [0, 1]), "aba": ([ESC_A, ESC_B, ESC_A], [0, 1, 2]),
               "name_only": ([ESC_N1, ESC_N2], [0, 1])}


@functools.lru_cache(maxsize=None)
def esc_synth():
    """phrase_ref.Synth(3000) with 64 alive docs' text replaced by [a, b] * c and up to 40 tokens of the
    old text without a and b (so tf(a) = tf(b) = c there); 16 of them get a name too: 8 the same
    [a, b] * c (c around 255), 8 [n1, n2] * c of two name-only ids."""
    c = pr.Synth(n=N_ESC, seed=pr.SEED + 2)
    r = np.random.default_rng(pr.SEED + 3)
    docs = np.sort(r.choice(N_ESC, 64, replace=False))
    c.esc_docs, c.esc_tf, c.esc_name_tf = docs, {}, {}
    for j, d in enumerate(docs):
        d = int(d)
        cnt = ESC_COUNTS[j % len(ESC_COUNTS)]
        old = c.text[d]
        filler = old[(old != ESC_A) & (old != ESC_B)][:40]
        c.text[d] = np.concatenate([np.tile([ESC_A, ESC_B], cnt), filler]).astype(np.uint32)
        c.text_gaps[d] = None
        c.deleted[d] = False
        c.esc_tf[d] = cnt
        if j % 4 == 0:
            x = j // 4
            cn = ESC_NAME_COUNTS[x % len(ESC_NAME_COUNTS)]
            pair = [ESC_A, ESC_B] if x < 8 else [ESC_N1, ESC_N2]
            c.name[d] = np.tile(pair, cn).astype(np.uint32)
            c.name_gaps[d] = None
            if x >= 8:
                c.esc_name_tf[d] = cn
    return c


@functools.lru_cache(maxsize=None)
def esc_case():
    c = esc_synth()
    qs = [ESC_QUERIES[n] for n in ESC_QUERIES]
    full = [ordered(d, s) for d, s in fc.phrase_hits(c, qs)]
    return ClauseCase("esc", ESC_KS, batch_of("phrase", qs, synth=c), full, synth=c, names=list(ESC_QUERIES))


# ---- one mixed batch on the phrase corpus

@functools.lru_cache(maxsize=None)
def mixed_case():
    """Rows of every shape in one plan: phrases, phrases beside clauses, groups, each with and without a
    filter, facet-only queries, AllQuery and plain ANDs / ORs; every row with its own reference."""
    c = fc.phrase_synth()
    pf, bf = phrase_family(), fc.bphrase_family()
    bref = bpr.of_synth(c)
    gref = gr.Ref(bref.corpus)
    M, S = gr.MUST, gr.SHOULD
    dele = c.deleted
    alive = np.flatnonzero(~dele)
    flt, flt2 = [fc.A, fc.HOT, fc.B], [fc.AX, fc.E]
    rows, full = [], []  # rows: (terms, occur, phrase_len, phrase_pos, filter)

    def add(args, hits, f):
        _, t, kw = args
        n = len(t)
        rows.append((np.asarray(t).tolist(), np.asarray(kw.get("occur", [M] * n)).tolist(),
                     np.asarray(kw["phrase_len"]).tolist(), np.asarray(kw["phrase_pos"]).tolist(), f))
        s, d = pf.facets.filtered(hits, f or None, pf.fst, c.n)
        full.append((s, d[:KEEP].astype(np.int64)))

    for i, f in ((0, []), (1, flt), (5, [])):
        add(batch_of("phrase", [pf.queries[i]]), pf.hits[i], f)
    for i, f in ((0, []), (16, flt2), (3 * bpr.PER_KIND, [])):
        add(batch_of("bphrase", [bf.queries[i]]), bf.hits[i], f)
    groups = [[gr.G(M, gr.ANY, [5, 9]), gr.T(M, 2)], [gr.G(S, gr.ALL, [3, 7]), gr.T(S, 41)],
              [gr.G(M, gr.ANY, [4, 6]), gr.G(M, gr.ANY, [1, 12])]]
    for q, f in zip(groups, ([], flt2, flt)):
        add(batch_of("group", [q]), gref.hits(q, deleted=dele), f)
    plain = [([4, 11], [M, M]), ([0, 1, 2], [M, M, M]), ([4, 11], [S, S]), ([30, 41, 50], [S, S, S])]
    for (t, o), f in zip(plain, ([], flt, [], [])):
        td, ts = bref.corpus._hits(t, o, None, None, None)
        keep = ~dele[td]
        add((None, t, dict(occur=o, phrase_len=[1] * len(t), phrase_pos=[0] * len(t))), (td[keep], ts[keep]), f)
    for f in (flt, flt2, [fc.RARE]):  # the union alone
        _, any_f = pf.facets.union(f, pf.fst)
        fd = alive[any_f[alive]]
        add((None, [], dict(occur=[], phrase_len=[], phrase_pos=[])), (fd, np.zeros(len(fd), F)), f)
    rows.append(([], [], [], [], []))  # AllQuery
    full.append((np.ones(len(alive), F), alive[:KEEP].astype(np.int64)))
    q_off = np.cumsum([0] + [len(r[0]) for r in rows]).astype(np.uint32)
    cat = lambda j, t: np.array([x for r in rows for x in r[j]], t)  # noqa: E731
    f_off, f_terms = fc.filter_arrays([r[4] for r in rows])
    kw = dict(occur=cat(1, np.uint8), phrase_len=cat(2, np.uint32), phrase_pos=cat(3, np.uint32), f_off=f_off,
              f_terms=f_terms)
    return ClauseCase("mixed", (10,), (q_off, cat(0, np.uint32), kw), full)
