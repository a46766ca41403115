"""Reference for fg_count_batch (tantivy's `searcher.search(&query, &(Count,
FacetCollector))`), written from the specification alone: pure Python / numpy,
nothing of libfugu.

A corpus is per-doc token lists per field, per-doc facet paths and a deleted
flag.  A query is (clauses, filter): clauses = [(occur, term)] with occur 0 Must,
1 Should, 2 MustNot (term None = a term the dictionary lacks), filter = a list of
facet term ids (None = missing), Must-combined with the text query.

  match set: alive docs only.  With a Must clause: the docs in every Must term's
  merged (text U name) list; Shoulds do not matter.  Without: the docs in some
  Should list.  Minus every MustNot list.  A Must on a missing term: nothing; a
  Should / MustNot on one is dropped.  No positive clause: nothing.  A filter:
  additionally in the union of its facet lists (a missing facet term matches
  nothing).  No clauses at all: the filter union alone, or, without a filter,
  every alive doc (AllQuery).
  total = |match|; count[j] = |match & postings(count_terms[j])| -- the facet
  field indexes every ancestor of each facet of a doc (facet_ref.tokens), once per
  doc, so this is FacetCollector's count of that facet.
"""
from __future__ import annotations

import numpy as np

import facet_ref

MUST, SHOULD, MUST_NOT = 0, 1, 2


class Corpus:
    """text / name: per-doc token-id lists (name[d] None: no name value);
    facets: per-doc lists of facet paths; deleted: per-doc flags."""

    def __init__(self, text, name, facets, deleted, n_terms, fdict=None):
        self.text, self.name, self.facets = text, name, facets
        self.deleted = np.asarray(deleted, np.uint8)
        self.n = len(text)
        self.n_terms = n_terms
        # the facet dictionary: every FacetTokenizer token of every facet, ids in first-seen order
        # (fdict: the dictionary of the namespace this corpus is a segment of)
        self.fdict = {} if fdict is None else fdict
        self.ftok = []
        for fl in facets:
            toks = []
            for p in fl:
                for t in facet_ref.tokens(facet_ref.from_text(facet_ref.normalize(p))):
                    toks.append(self.fdict.setdefault(t, len(self.fdict)))
            self.ftok.append(toks)  # duplicates kept, as add_facets_to_document feeds them
        self.fterms = sorted(self.fdict, key=lambda e: e.encode())  # encoded byte order
        # inverted lists as Python sets
        self.post = {}
        for d in range(self.n):
            for t in set(text[d]) | set(name[d] or ()):
                self.post.setdefault(t, set()).add(d)
        self.fpost = {}
        for d, toks in enumerate(self.ftok):
            for t in set(toks):
                self.fpost.setdefault(t, set()).add(d)
        self.alive = {d for d in range(self.n) if not self.deleted[d]}

    def fid(self, path):
        """facet term id of a path, or None"""
        return self.fdict.get(facet_ref.from_text(path))

    def slice(self, a, b, deleted=None):
        """docs [a, b) as a corpus of their own SHARING this one's dictionaries"""
        return Corpus(self.text[a:b], self.name[a:b], self.facets[a:b],
                      self.deleted[a:b] if deleted is None else deleted, self.n_terms, self.fdict)

    # ---- the arrays fg_index_build_from_docs takes
    def csr(self):
        text_off = np.cumsum([0] + [len(t) for t in self.text]).astype(np.uint64)
        text_tok = np.array([x for t in self.text for x in t], np.uint32)
        name_off = np.cumsum([0] + [len(t or ()) for t in self.name]).astype(np.uint64)
        name_tok = np.array([x for t in self.name for x in (t or ())], np.uint32)
        f_off = np.cumsum([0] + [len(t) for t in self.ftok]).astype(np.uint64)
        f_tok = np.array([x for t in self.ftok for x in t], np.uint32)
        return text_off, text_tok, name_off, name_tok, (f_off, f_tok, len(self.fdict))


def match_set(c: Corpus, clauses, flt):
    """the spec's match set, from the inverted lists"""
    must = [t for o, t in clauses if o == MUST]
    should = [t for o, t in clauses if o == SHOULD and t in c.post]
    nots = [t for o, t in clauses if o == MUST_NOT and t in c.post]
    if clauses:
        if must:
            if any(t not in c.post for t in must):
                return set()
            m = set.intersection(*[c.post[t] for t in must])
        elif should:
            m = set.union(*[c.post[t] for t in should])
        else:
            return set()
        for t in nots:
            m = m - c.post[t]
        if flt:
            m = m & set().union(*[c.fpost.get(t, set()) for t in flt])
    elif flt:
        m = set().union(*[c.fpost.get(t, set()) for t in flt])
    else:
        m = set(range(c.n))
    return m & c.alive


def count_batch(c: Corpus, queries, count_terms):
    """(total [nq], count [nq, n_count]) as uint64"""
    total = np.zeros(len(queries), np.uint64)
    count = np.zeros((len(queries), len(count_terms)), np.uint64)
    for i, (clauses, flt) in enumerate(queries):
        m = match_set(c, clauses, flt)
        total[i] = len(m)
        for j, t in enumerate(count_terms):
            count[i, j] = len(m & c.fpost.get(t, set()))
    return total, count


def count_brute(c: Corpus, queries, count_terms):
    """the same, doc by doc from the docs' own tokens (no inverted lists)"""
    total = np.zeros(len(queries), np.uint64)
    count = np.zeros((len(queries), len(count_terms)), np.uint64)
    for d in range(c.n):
        if c.deleted[d]:
            continue
        toks = set(c.text[d]) | set(c.name[d] or ())
        ftoks = set(c.ftok[d])
        for i, (clauses, flt) in enumerate(queries):
            if clauses:
                must = [t for o, t in clauses if o == MUST]
                if must:
                    ok = all(t in toks for t in must)
                else:
                    ok = any(t in toks for o, t in clauses if o == SHOULD)
                ok = ok and not any(t in toks for o, t in clauses if o == MUST_NOT)
                if flt:
                    ok = ok and any(t in ftoks for t in flt)
            elif flt:
                ok = any(t in ftoks for t in flt)
            else:
                ok = True
            if ok:
                total[i] += 1
                for j, t in enumerate(count_terms):
                    count[i, j] += t in ftoks
    return total, count


def children(c: Corpus, root_path, m):
    """FacetCounts::get(root): [(Display path, count)] of the direct children of
    root with a nonzero count among the docs m, in encoded-facet byte order"""
    root = facet_ref.from_text(root_path)
    pre = root + facet_ref.SEP if root else ""
    out = []
    for e in c.fterms:
        if not e or not e.startswith(pre) or len(e) <= len(pre) or facet_ref.SEP in e[len(pre):]:
            continue
        n = len(m & c.fpost.get(c.fdict[e], set()))
        if n:
            out.append((facet_ref.display(e), n))
    return out


def tree(c: Corpus, max_depth=None, root="/", depth=0):
    """collect_facets_recursive: pre-order (Display path, AllQuery count), depth-limited"""
    if max_depth is not None and depth >= max_depth:
        return []
    out = []
    for p, n in children(c, root, c.alive):
        out.append((p, n))
        out += tree(c, max_depth, p, depth + 1)
    return out


# ---- the batch fg_count_batch takes
def batch_arrays(queries, missing=0xFFFFFFFF):
    q_off, terms, occur, f_off, f_terms = [0], [], [], [0], []
    for clauses, flt in queries:
        for o, t in clauses:
            occur.append(o)
            terms.append(missing if t is None else t)
        q_off.append(len(terms))
        for t in flt or ():
            f_terms.append(missing if t is None else t)
        f_off.append(len(f_terms))
    return (np.array(q_off, np.uint32), np.array(terms, np.uint32), np.array(occur, np.uint8),
            np.array(f_off, np.uint32), np.array(f_terms, np.uint32))


# ---- corpora (seeded)
DENSE, MID, RARE, NAME_ONLY = 0, 5, 62, 63  # term ids of main_corpus / small_corpus
VOCAB = 64


def _corpus(n, seed, rare_every):
    """Zipf(1) over term ids 0..61 in `text`, lengths 1-40; `name` (1-3 Zipf tokens,
    plus NAME_ONLY -- which occurs in no text -- on every 11th named doc) on a third
    of the docs; RARE in the text of every rare_every-th doc.  Facets: /org/{0..6},
    /org/i/team/{0..4}, /kind/{a,b,c}, /org/i alone on some docs, a few docs with
    /org itself, two teams of one org on some docs, none on ~10%.  5% deleted."""
    rng = np.random.RandomState(seed)
    w = 1.0 / np.arange(1, 63)
    cdf = np.cumsum(w / w.sum())
    draw = lambda k: np.minimum(np.searchsorted(cdf, rng.random_sample(k)), 61).tolist()  # noqa: E731
    text, name, facets = [], [], []
    for d in range(n):
        t = draw(int(rng.randint(1, 41)))
        if d % rare_every == 3:
            t.append(RARE)
        text.append(t)
        if d % 3 == 1:
            nm = draw(int(rng.randint(1, 4)))
            if d % 11 == 4:
                nm.append(NAME_ONLY)
            name.append(nm)
        else:
            name.append(None)
        r, fl = rng.random_sample(), []
        org, team = int(rng.randint(0, 7)), int(rng.randint(0, 5))
        if r < 0.10:
            pass
        elif r < 0.50:
            fl.append(f"/org/{org}/team/{team}")
        elif r < 0.65:
            fl.append(f"/org/{org}")
        elif r < 0.70:
            fl += [f"/org/{org}/team/{team}", f"/org/{org}/team/{(team + 2) % 5}"]  # two facets under one child
        elif r < 0.72:
            fl.append("/org")  # a facet equal to a root whose children are counted
        else:
            fl += [f"/org/{org}/team/{team}", f"/org/{(org + 3) % 7}"]
        if rng.random_sample() < 0.6:
            fl.append("/kind/" + "abc"[int(rng.randint(0, 3))])
        facets.append(fl)
    deleted = (rng.random_sample(n) < 0.05).astype(np.uint8)
    return Corpus(text, name, facets, deleted, VOCAB)


def main_corpus():
    return _corpus(40037, 20261, 1000)


def small_corpus(n=300):
    return _corpus(n, 77, 60)


def query_batch(c: Corpus):
    """[(label, clauses, filter)]: every query kind of the specification, then each
    text shape once more with a filter"""
    f = c.fid
    M, S, X = MUST, SHOULD, MUST_NOT
    text = [
        ("dense", [(S, DENSE)]), ("rare", [(S, RARE)]), ("name_only", [(S, NAME_ONLY)]), ("must_dense", [(M, 1)]),
        ("and2", [(M, 0), (M, 3)]), ("and2_rare", [(M, RARE), (M, 0)]), ("and3", [(M, 1), (M, 2), (M, 4)]),
        ("and3_mid", [(M, 7), (M, 9), (M, 0)]), ("or2", [(S, 2), (S, 6)]), ("or2_rare", [(S, RARE), (S, NAME_ONLY)]),
        ("or3", [(S, 10), (S, 20), (S, 30)]), ("or3_dense", [(S, 0), (S, 1), (S, RARE)]),
        ("+a b", [(M, 8), (S, 0)]), ("a -b", [(S, 3), (X, 0)]), ("a -rare", [(S, 0), (X, RARE)]),
        ("+a -b +c", [(M, 2), (X, 1), (M, 5)]), ("+a -b -c", [(M, 0), (X, 40), (X, NAME_ONLY)]),
        ("or2 -c", [(S, 12), (S, 13), (X, 2)]), ("must_missing", [(M, None), (M, 0)]),
        ("must_missing_alone", [(M, None)]), ("should_missing_beside", [(S, None), (S, 4)]),
        ("not_missing", [(S, 4), (X, None)]), ("not_only", [(X, 0)]), ("not_only2", [(X, 3), (X, RARE)]),
        ("should_missing_alone", [(S, None)]), ("dup_must", [(M, 6), (M, 6)]),
        ("and_name_only", [(M, NAME_ONLY), (M, 0)]), ("+rare mid", [(M, RARE), (S, MID)]),
    ]
    flt1, flt3 = [f("/org/3")], [f("/kind/a"), None, f("/org/1/team/2")]
    qs = [("all", [], None), ("facet1", [], [f("/org/2")]), ("facet3", [], [f("/kind/b"), f("/org/5/team/0"), None]),
          ("facet_missing", [], [None]), ("facet_root", [], [f("/org")]), ("facet_dup", [], [f("/kind/c"), f("/kind/c")])]
    qs += [(lab, cl, None) for lab, cl in text]
    qs += [(lab + "|f", cl, flt3 if i % 2 else flt1) for i, (lab, cl) in enumerate(text)]
    qs += [("dense|f_missing", [(S, DENSE)], [None]), ("and2|f_org", [(M, 0), (M, 1)], [f("/org")])]
    return qs


EMPTY_BY_DESIGN = ("facet_missing", "must_missing", "must_missing_alone", "not_only", "not_only2",
                   "should_missing_alone", "dense|f_missing")
