"""fg_index_build_positional on the device: the forward index built
by the k_fwd_* kernels from the positions of pre-inverted postings
(tests/positions_ref.py makes them from token streams) must be, entry for entry,
the one fg_index_build_from_docs keeps from the same streams -- so phrase queries
give bit-identical results on the two snapshots -- and invalid positions must be
refused, never stored.

- a known-answer corpus with the kernels' edges (an empty doc, holes, a posting of
  3000 positions, a row of 70,000);
- phrase_ref.Synth built both ways: rows, 256 phrases at k = 10 and 1000, the
  reference, device_bytes;
- corpora around the scans' slice count;
- three segments under global statistics, one rescored, one from token streams;
- the device-side refusals, each followed by a good build on the same context.
"""
import numpy as np
import pytest

import phrase_ref as pr
import positions_ref as po
from test_gpu_phrase import RTOL, check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from fugu_amd import native as nat
    if nat.device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    return nat


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context((0,))


def csr(docs, gaps):
    """(off, tok, gap) of token streams and per-doc gap lists: the fg_docs_input arrays"""
    off = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    tok = np.concatenate([np.zeros(0, np.uint32)] + [np.asarray(d, np.uint32) for d in docs]).astype(np.uint32)
    gap = [int(off[i]) + g for i in range(len(docs)) if gaps is not None and gaps[i] is not None for g in gaps[i]]
    return off, tok, np.array(gap, np.uint64)


def assert_rows(ix, p, fields=(0, 1)):
    for f in fields:
        woff, wtok = p.rows(f)
        off, tok = ix.positions(f)
        assert np.array_equal(off, woff), f
        assert np.array_equal(tok, wtok), f


def same_hits(a, b):
    """search_batch results of two snapshots, bit for bit"""
    assert np.array_equal(a[2], b[2])
    for i, m in enumerate(a[2]):
        assert np.array_equal(a[1][i, :m], b[1][i, :m]), i
        assert np.array_equal(a[0][i, :m].view(np.uint32), b[0][i, :m].view(np.uint32)), i


# ------------------------------------------------------------------ known answer
def test_known_answer_and_kernel_edges(native, ctx):
    V = 10
    text = [list(d) for d in pr.kat_corpus()]
    text.append([])                            # 4: an empty text
    text.append([1, 2])                        # 5: a hole at position 0, two in a row: _ 1 _ _ 2
    text.append([5] * 3000)                    # 6: one posting of 3000 positions (past the tf escape byte)
    text.append([i % 7 for i in range(70000)])  # 7: a row longer than 2^16, seven postings of 10,000
    text.append([0, 1, 2, 3])                  # 8
    gaps = [None] * len(text)
    gaps[5] = [0, 1, 1]
    name = [[] for _ in text]
    name[4] = [9, 9, 1]                        # term 9 is in `name` only
    name[8] = [0, 9]
    ngaps = [None] * len(text)
    ngaps[8] = [1]                             # 0 _ 9
    p = po.Postings(text, name, V, gaps, ngaps)
    assert p.tf_text.max() == 10000 and int(np.diff(p.rows(0)[0].astype(np.int64)).max()) == 70000
    ix = native.Index.from_postings(ctx, *p.args(), positions=p.positions())
    assert ix.stats().has_positions
    assert_rows(ix, p)
    assert ix.positions(0, 5, 1)[1].tolist() == [po.HOLE, 1, po.HOLE, po.HOLE, 2]
    assert ix.positions(1, 8, 1)[1].tolist() == [0, po.HOLE, 9]
    assert ix.positions(0, 4, 1)[0].tolist() == [0, 0]
    to, tt, tg = csr(text, gaps)
    no, nt, ng = csr(name, ngaps)
    twin = native.Index.from_docs(ctx, to, tt, V, no, nt, positions=True, text_gaps=tg, name_gaps=ng)
    for f in (0, 1):
        a, b = ix.positions(f), twin.positions(f)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    qs = [([0, 1], [0, 1]), ([1, 2], [0, 1]), ([0, 0], [0, 1]), ([5, 5, 5], [0, 1, 2]), ([1, 2], [0, 3]),
          ([6, 0, 1], [0, 1, 2]), ([9, 9], [0, 1]), ([0, 9], [0, 2]), ([9, 1], [0, 1]), ([2, 1], [0, 1])]
    q_off = np.cumsum([0] + [len(t) for t, _ in qs])
    terms = [x for t, _ in qs for x in t]
    plen = [len(t) if j == 0 else 0 for t, _ in qs for j in range(len(t))]
    ppos = [x for _, o in qs for x in o]
    a = ix.search_batch(q_off, terms, 10, phrase_len=plen, phrase_pos=ppos)
    b = twin.search_batch(q_off, terms, 10, phrase_len=plen, phrase_pos=ppos)
    same_hits(a, b)
    assert [int(x) for x in a[2]] == [4, 4, 2, 1, 1, 1, 1, 1, 1, 0], a[2]
    # ... and the reference agrees
    tf_, nf_ = pr.Field(text, gaps), pr.Field(name, ngaps)
    st = pr.Stats.of(tf_, nf_, V)
    check(a[0], a[1], a[2], [pr.search(tf_, nf_, st, t, o, 10)[:2] for t, o in qs], 10, "kat")


# ------------------------------------------------------------------ the 6000-doc corpus, built both ways
@pytest.fixture(scope="module")
def corpus(native, ctx):
    c = pr.Synth()
    p = po.Postings(c.text, c.name, pr.V, c.text_gaps, c.name_gaps)
    st = pr.Stats.of(p.text, p.name, pr.V)
    ix = native.Index.from_postings(ctx, *p.args(), deleted=c.deleted, positions=p.positions())
    to, tt, tg = c.csr(c.text, c.text_gaps)
    no, nt, ng = c.csr(c.name, c.name_gaps)
    twin = native.Index.from_docs(ctx, to, tt, pr.V, no, nt, deleted=c.deleted, positions=True, text_gaps=tg, name_gaps=ng)
    return c, p, st, ix, twin


def test_synth_rows(native, corpus):
    c, p, st, ix, twin = corpus
    assert ix.stats().has_positions and ix.stats().n_docs == 6000
    assert_rows(ix, p)
    for f in (0, 1):
        a, b = ix.positions(f), twin.positions(f)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # a range in the middle, and what the call refuses
    off, tok = ix.positions(0, 1000, 17)
    woff, wtok = p.rows(0)
    b0, b1 = int(woff[1000]), int(woff[1017])
    assert np.array_equal(off, woff[1000:1018] - woff[1000]) and np.array_equal(tok, wtok[b0:b1])
    for args in ((2, 0, 1), (0, 5999, 2)):
        with pytest.raises(native.FuguError) as e:
            ix.positions(*args)
        assert e.value.code == native.FG_EINVAL


@pytest.mark.parametrize("k", [10, 1000])
def test_synth_twins_and_reference(native, corpus, k):
    c, p, st, ix, twin = corpus
    q_off, terms, plen, ppos = c.batch()
    a = ix.search_batch(q_off, terms, k, phrase_len=plen, phrase_pos=ppos)
    b = twin.search_batch(q_off, terms, k, phrase_len=plen, phrase_pos=ppos)
    same_hits(a, b)
    want = [pr.search(p.text, p.name, st, t, o, k, deleted=c.deleted)[:2] for t, o in c.queries]
    check(a[0], a[1], a[2], want, k, f"k={k}")
    assert (a[2] > 0).mean() >= 0.75


def test_synth_forward_index_is_counted(native, ctx, corpus):
    c, p, st, ix, twin = corpus
    plain = native.Index.from_postings(ctx, *p.args(), deleted=c.deleted)
    a, b = ix.stats(), plain.stats()
    assert a.has_positions and not b.has_positions
    fwd = sum(4 * int(p.rows(f)[0][-1]) + 8 * (c.n + 1) for f in (0, 1))
    assert fwd <= a.device_bytes - b.device_bytes <= fwd + 4 * 512  # (allocation rounding)
    assert (a.n_postings, a.tot_tokens, a.avgdl) == (b.n_postings, b.tot_tokens, b.avgdl)
    # without positions a phrase is still refused
    with pytest.raises(native.Unsupported, match="snapshot built without positions"):
        plain.search_batch([0, 2], [0, 1], 10, phrase_len=[2, 0], phrase_pos=[0, 1])
    with pytest.raises(native.FuguError) as e:
        plain.positions(0)
    assert e.value.code == native.FG_EINVAL


# ------------------------------------------------------------------ the scans' slices
@pytest.mark.parametrize("n", ["1", "G-1", "G+1", "3G+7"])
def test_scan_edges(native, ctx, n):
    G = native.FWD_SCAN_SLICES
    n = {"1": 1, "G-1": G - 1, "G+1": G + 1, "3G+7": 3 * G + 7}[n]
    r = np.random.default_rng(n)
    text = [r.integers(0, 50, int(r.integers(1, 4))).astype(np.uint32) for _ in range(n)]
    p = po.Postings(text, None, 50)
    ix = native.Index.from_postings(ctx, *p.args(), positions=p.positions())
    assert_rows(ix, p, (0,))
    with pytest.raises(native.FuguError):  # (no name postings: no name forward index)
        ix.positions(1)


# ------------------------------------------------------------------ segments, a rescore, a token-stream segment
def test_segments_and_rescore(native, ctx, corpus):
    c, p, st, _, _ = corpus
    cuts = [0, 1700, 4300, c.n]
    dele = c.deleted.copy()
    dele[cuts[1]:cuts[2]:7] = ~dele[cuts[1]:cuts[2]:7]  # the middle segment's deletions change after its build
    parts, g = [], None
    for lo, hi in zip(cuts, cuts[1:]):
        parts.append(po.Postings(c.text[lo:hi], c.name[lo:hi], pr.V, c.text_gaps[lo:hi], c.name_gaps[lo:hi]))
        to, tt, _ = c.csr(c.text, c.text_gaps, lo, hi)
        no, nt, _ = c.csr(c.name, c.name_gaps, lo, hi)
        x = native.docs_stats(to, tt, pr.V, no, nt)
        g = x if g is None else g + x
    assert (g.n_docs, tuple(g.tot_tokens)) == (st.n, st.tot) and np.array_equal(g.df_text, st.df_text)
    ixs = []
    for s_, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        q = parts[s_]
        if s_ == 1:  # under its OWN statistics and the old deletions, then rescored: the forward index is shared
            own = native.Index.from_postings(ctx, *q.args(), deleted=c.deleted[lo:hi], positions=q.positions())
            ixs.append(own.rescore(g, deleted=dele[lo:hi]))
            assert ixs[-1].stats().has_positions
            assert_rows(ixs[-1], q)
        else:
            ixs.append(native.Index.from_postings(ctx, *q.args(), deleted=dele[lo:hi], global_stats=g,
                                                  positions=q.positions()))
    want = [pr.search(p.text, p.name, st, t, o, 10, deleted=dele)[:2] for t, o in c.queries]
    base = np.array(cuts[:-1], np.int64)
    q_off, terms, plen, ppos = c.batch()

    def run(segs, tag):
        s, d, sh, n = native.search_sharded(segs, q_off, terms, 10, ctx=ctx, phrase_len=plen, phrase_pos=ppos)
        check(s, d.astype(np.int64) + base[sh], n, want, 10, tag)
        return s, d, sh, n

    a = run(ixs, "positional segments")
    # the first segment from its token streams instead: the same answer, bit for bit
    to, tt, tg = c.csr(c.text, c.text_gaps, 0, cuts[1])
    no, nt, ng = c.csr(c.name, c.name_gaps, 0, cuts[1])
    tok_seg = native.Index.from_docs(ctx, to, tt, pr.V, no, nt, deleted=dele[:cuts[1]], global_stats=g, positions=True,
                                     text_gaps=tg, name_gaps=ng)
    b = run([tok_seg] + ixs[1:], "mixed segments")
    assert np.array_equal(a[3], b[3])
    for i, m in enumerate(a[3]):
        assert np.array_equal(a[0][i, :m].view(np.uint32), b[0][i, :m].view(np.uint32))
        assert np.array_equal(a[1][i, :m], b[1][i, :m]) and np.array_equal(a[2][i, :m], b[2][i, :m])


# ------------------------------------------------------------------ device-side refusals
def test_device_side_refusals(native, ctx):
    """Invalid positions that pass the host checks (the counts are right): the kernels
    find them, store nothing outside a row, and the build fails with FG_EINVAL."""
    c = pr.Synth(n=50)
    p = po.Postings(c.text, c.name, pr.V, c.text_gaps, c.name_gaps)
    start = p.text_tf_off()
    tf = p.tf_text.astype(np.int64)

    def swapped():
        q = int(np.nonzero(tf >= 2)[0][0])
        x = p.text_pos.copy()
        x[start[q]], x[start[q] + 1] = x[start[q] + 1], x[start[q]]
        return x

    def past_the_row():
        q = int(np.nonzero(tf >= 3)[0][0])
        x = p.text_pos.copy()
        x[start[q] + 1] = 10_000_000  # the posting's middle entry: its last one still sets the row's length
        return x

    def duplicated():
        one = np.nonzero(tf == 1)[0]
        for q in one:  # a posting of one position takes a position of another term in its doc
            others = np.nonzero((p.doc == p.doc[q]) & (tf > 0))[0]
            others = others[others != q]
            if len(others):
                x = p.text_pos.copy()
                x[start[q]] = x[start[others[0]]]
                return x
        raise AssertionError("no doc with a single-position posting beside another")

    def none_position():
        q = int(np.nonzero(tf >= 2)[0][0])
        x = p.text_pos.copy()
        x[start[q + 1] - 1] = 0xFFFFFFFF  # the posting's last entry: still ascending
        return x

    span = [int(t) for t in c.text[0][:2]]
    for make, why in ((swapped, "ascend"), (past_the_row, "positions"), (duplicated, "same"), (none_position, "0xFFFFFFFF")):
        with pytest.raises(native.FuguError, match=why) as e:
            native.Index.from_postings(ctx, *p.args(), positions=(make(), p.name_pos))
        assert e.value.code == native.FG_EINVAL, make.__name__
        assert "text positions" in str(e.value), make.__name__
        ok = native.Index.from_postings(ctx, *p.args(), positions=p.positions())  # the same context still builds
        assert_rows(ok, p)
        assert int(ok.search_batch([0, 2], span, 10, phrase_len=[2, 0], phrase_pos=[0, 1])[2][0]) > 0
    # the name field's positions are checked the same way
    nstart = np.concatenate([[0], np.cumsum(p.tf_name.astype(np.int64))])
    q = int(np.nonzero(p.tf_name >= 2)[0][0])
    x = p.name_pos.copy()
    x[nstart[q]], x[nstart[q] + 1] = x[nstart[q] + 1], x[nstart[q]]
    with pytest.raises(native.FuguError, match="name positions") as e:
        native.Index.from_postings(ctx, *p.args(), positions=(p.text_pos, x))
    assert e.value.code == native.FG_EINVAL
