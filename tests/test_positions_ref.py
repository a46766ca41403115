"""What needs no GPU of fg_index_build_positional: the numpy helper
tests/positions_ref.py inverts the phrase corpus into positional postings that
describe exactly its forward rows, the corpus has what test_gpu_positions.py
relies on, and the host-side refusals of the new calls (which run before any
context or device is looked at)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import phrase_ref as pr
import positions_ref as po
from conftest import ROOT


@pytest.fixture(scope="module")
def synth():
    c = pr.Synth()
    return c, po.Postings(c.text, c.name, pr.V, c.text_gaps, c.name_gaps)


def test_round_trip_reproduces_the_rows(synth):
    c, p = synth
    for f, field, tf, pos in ((0, p.text, p.tf_text, p.text_pos), (1, p.name, p.tf_name, p.name_pos)):
        off, tok = po.rows_from_postings(p.n, p.term_off, p.doc, tf, pos)
        woff, wtok = p.rows(f)
        assert np.array_equal(off, woff) and np.array_equal(tok, wtok)
        # ... which are Field.flat itself, doc by doc (this corpus has no hole after a doc's last token)
        assert np.array_equal(np.where(tok == po.HOLE, pr.NONE, tok.astype(np.int64)), field.flat)
        assert np.array_equal(np.repeat(np.arange(p.n), np.diff(off.astype(np.int64))), field.owner)
    # the postings are what fg_index_build wants: docs ascending per term, a tf in some field
    for t in range(pr.V):
        d = p.doc[int(p.term_off[t]):int(p.term_off[t + 1])].astype(np.int64)
        assert (np.diff(d) > 0).all()
    assert ((p.tf_text > 0) | (p.tf_name > 0)).all()
    assert p.tot_tokens == (int(sum(len(x) for x in c.text)), int(sum(len(x) for x in c.name)))


def test_trailing_holes_are_cut():
    f = pr.Field([[1, 2], [], [3]], [[0, 0, 1], None, None])
    off, tok = po.rows(f)
    assert off.tolist() == [0, 5, 5, 6] and tok.tolist() == [po.HOLE, po.HOLE, 1, po.HOLE, 2, 3]
    f.flat = np.concatenate([f.flat[:5], [pr.NONE], f.flat[5:]])  # a hole after doc 0's last token
    f.owner = np.concatenate([f.owner[:5], [0], f.owner[5:]])
    off2, tok2 = po.rows(f)
    assert np.array_equal(off, off2) and np.array_equal(tok, tok2)


def test_corpus_has_what_the_gpu_test_relies_on(synth):
    c, p = synth
    off, tok = p.rows(0)
    holes = tok == po.HOLE
    assert (len(p.text_pos), int(holes.sum()), int((p.tf_text > 0).sum()), int(p.tf_text.max())) == (901179, 172, 224001, 81)
    assert int((holes[1:] & holes[:-1]).sum()) == 2 and int((np.diff(off.astype(np.int64)) == 0).sum()) == 0
    noff, ntok = p.rows(1)
    assert (len(p.name_pos), int((ntok == po.HOLE).sum())) == (10053, 40)
    assert p.tf_text.max() > 16  # longer than one lane's loop (fg_internal.h kFwdShort)


def test_slice_count_matches_the_header():
    from fugu_amd import native
    h = open(os.path.join(ROOT, "include", "fugu.h")).read()
    assert native.FWD_SCAN_SLICES == int(re.search(r"#define FG_FWD_SCAN_SLICES (\d+)", h).group(1))


def test_null_arguments_without_a_device():
    from fugu_amd import native
    lib = native.lib()
    assert lib.fg_index_build_positional(None, 0, None, None, None, None) == native.FG_EINVAL
    assert lib.fg_index_positions_get(None, 0, 0, 0, None, None, 0, None) == native.FG_EINVAL


def test_host_side_refusals_need_no_device(synth):
    """pos == NULL, a count that is not the field's tf sum, a NULL array with a count,
    name postings without name_pos: FG_EINVAL with the field named, found before the
    context is looked at (ctx is NULL here: a correct input gets as far as that)."""
    from fugu_amd import native
    lib = native.lib()
    c, p = synth
    keep, inp = native._index_input(*p.args())
    h = native._p()

    def build(pos):
        rc = lib.fg_index_build_positional(None, 0, C.byref(inp), None if pos is None else C.byref(pos), None, C.byref(h))
        return rc, (lib.fg_last_error() or b"").decode()

    rc, msg = build(None)
    assert rc == native.FG_EINVAL and "fg_index_build_global" in msg
    good = (p.text_pos, p.name_pos)
    for text_pos, name_pos, field in ((p.text_pos[:-1], p.name_pos, "text"), (np.append(p.text_pos, 7), p.name_pos, "text"),
                                      (p.text_pos, p.name_pos[:-1], "name"), (p.text_pos, None, "name")):
        pk, pos = native._positions_input(text_pos, name_pos)
        rc, msg = build(pos)
        assert rc == native.FG_EINVAL and msg.startswith(field + " positions"), (field, msg)
    for fld, field in (("text_pos", "text"), ("name_pos", "name")):  # a NULL array with its count
        pk, pos = native._positions_input(*good)
        setattr(pos, fld, None)
        rc, msg = build(pos)
        assert rc == native.FG_EINVAL and msg.startswith(field + " positions") and "NULL" in msg, msg
    # what fg_index_build_global rejects comes first, with its message
    pk, pos = native._positions_input(p.text_pos[:-1], p.name_pos)
    bkeep, bad = native._index_input(*p.args())
    bad.n_docs = 0
    assert lib.fg_index_build_positional(None, 0, C.byref(bad), C.byref(pos), None, C.byref(h)) == native.FG_EINVAL
    assert "n_docs out of range" in lib.fg_last_error().decode()
    # a correct input passes every host check of the positions: the refusal is the missing context
    pk, pos = native._positions_input(*good)
    rc, msg = build(pos)
    assert rc == native.FG_EINVAL and msg == "bad arguments", msg
    assert not h.value
