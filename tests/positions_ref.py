"""Positional postings of a small corpus, in numpy, for the tests of
fg_index_build_positional: what a tantivy host reads from a
segment's `text` / `name` inverted indexes -- merged postings by term with a tf
per field, fieldnorm ids, token totals, and each posting's positions -- made
from the token streams and gap lists phrase_ref.Field takes.  Also the forward
index rows such a snapshot must hold.  Calls nothing of libfugu.
"""
import numpy as np

import phrase_ref as pr

HOLE = 0xFFFFFFFF  # a dropped position in a forward row


def _field_postings(field, n_docs):
    """(key = term * n_docs + doc of each posting, ascending; tf; positions in posting order)"""
    start = np.zeros(field.n + 1, np.int64)
    np.add.at(start, field.owner + 1, 1)
    start = np.cumsum(start)
    pos = np.arange(len(field.flat), dtype=np.int64) - start[field.owner]
    keep = field.flat >= 0
    term, doc, pos = field.flat[keep], field.owner[keep], pos[keep]
    order = np.lexsort((pos, doc, term))
    key = term[order] * n_docs + doc[order]
    ukey, tf = np.unique(key, return_counts=True)
    return ukey, tf, pos[order].astype(np.uint32)


def rows(field):
    """(off u64 [n + 1], tok u32) of the field's forward rows: Field.flat per doc,
    HOLE at a dropped position, holes after a doc's last token cut (they are not
    represented in positional postings)."""
    out, off = [], [0]
    bounds = np.searchsorted(field.owner, np.arange(field.n + 1))
    for d in range(field.n):
        r = field.flat[bounds[d]:bounds[d + 1]]
        kept = np.nonzero(r >= 0)[0]
        r = r[:kept[-1] + 1] if len(kept) else r[:0]
        out.append(np.where(r >= 0, r, HOLE).astype(np.uint32))
        off.append(off[-1] + len(r))
    return np.array(off, np.uint64), (np.concatenate(out) if out else np.zeros(0, np.uint32)).astype(np.uint32)


def rows_from_postings(n_docs, term_off, doc, tf, pos):
    """(off, tok) of the forward rows the positional postings of one field describe:
    row length = the doc's largest position + 1, tok[off[doc] + position] = term."""
    tf = tf.astype(np.int64)
    term = np.repeat(np.arange(len(term_off) - 1), np.diff(term_off.astype(np.int64)))
    e_doc, e_term = np.repeat(doc.astype(np.int64), tf), np.repeat(term, tf)
    length = np.zeros(n_docs, np.int64)
    np.maximum.at(length, e_doc, pos.astype(np.int64) + 1)
    off = np.concatenate([[0], np.cumsum(length)])
    tok = np.full(off[-1], HOLE, np.uint32)
    tok[off[e_doc] + pos.astype(np.int64)] = e_term
    return off.astype(np.uint64), tok


class Postings:
    """The fg_index_input arrays and the two position arrays of `text` / `name`
    token streams (lists of token id sequences; name may be None) with their gap
    lists, over a vocabulary of n_terms."""

    def __init__(self, text, name, n_terms, text_gaps=None, name_gaps=None):
        n = len(text)
        self.n, self.n_terms = n, n_terms
        self.text = pr.Field(text, text_gaps)
        self.name = pr.Field(name, name_gaps) if name is not None else None
        kt, tft, self.text_pos = _field_postings(self.text, n)
        if self.name is not None:
            kn, tfn, self.name_pos = _field_postings(self.name, n)
        else:
            kn, tfn, self.name_pos = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint32)
        key = np.union1d(kt, kn)
        assert max(tft.max(initial=0), tfn.max(initial=0)) <= 0xFFFF
        self.tf_text = np.zeros(len(key), np.uint16)
        self.tf_text[np.searchsorted(key, kt)] = tft
        self.tf_name = np.zeros(len(key), np.uint16)
        self.tf_name[np.searchsorted(key, kn)] = tfn
        self.doc = (key % n).astype(np.uint32)
        self.term_off = np.searchsorted(key // n, np.arange(n_terms + 1)).astype(np.uint64)
        self.fn_text = np.array([pr.fieldnorm_id(int(x)) for x in self.text.len], np.uint8)
        self.fn_name = (np.array([pr.fieldnorm_id(int(x)) for x in self.name.len], np.uint8) if self.name is not None
                        else np.zeros(n, np.uint8))
        self.tot_tokens = (int(self.text.len.sum()), int(self.name.len.sum()) if self.name is not None else 0)

    def text_tf_off(self):
        """first entry of each posting in text_pos [P + 1]"""
        return np.concatenate([[0], np.cumsum(self.tf_text.astype(np.int64))])

    def args(self):
        """the positional arguments of native.Index.from_postings after ctx"""
        return (self.n, self.term_off, self.doc, self.tf_text, self.tf_name, self.fn_text, self.fn_name, self.tot_tokens)

    def positions(self):
        """from_postings' `positions` argument"""
        return (self.text_pos, self.name_pos if len(self.name_pos) else None)

    def rows(self, field):
        return rows(self.text if field == 0 else self.name)
