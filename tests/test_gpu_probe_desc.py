"""k_conj's probe descriptors (fg_internal.h ProbeDesc, DevPlan::q_probe) at the
edges of the ranges they describe, against the CPU oracle (runs on the MI355X box).

The kernel reads a clause's rank words / block entries / bucket directory and
its scores through buffer resources whose byte sizes the planner computed, and
the lead list through a window of the chunk's own: a size one element short, a
base one term off or a last chunk handled wrongly shows as a missing or a
wrong hit at exactly these places:
  * lead lists of 1, 2047, 2048, 2049 and 4096 postings (the short last chunk;
    none; one posting past a full chunk; two full chunks);
  * matches at doc 0 and at doc N - 1 (the first and the last rank word, the
    last bucket of a directory, the last byte of every range);
  * probed terms whose matching posting is their last (pos = df - 1);
  * the vocabulary's last term, probed and leading (off[t + 1] = P);
  * Must + MustNot + Should in one query;
  * a plan over two snapshots of different sizes, per slot (fg_plan_execute) and
    merged (fg_plan_execute_merged);
  * the same after a commit elsewhere in the namespace: the older snapshot
    rescored, so the plan scores at query time from the payloads (feat 4).
Under each rank-layout environment of test_gpu_parity.py, k = 10 and 100: doc ids
bit-exact, scores within the project's 1e-5.
"""
import os

import numpy as np
import pytest

from shard_ref import merge_topk_numpy

pytestmark = pytest.mark.gpu

RTOL = 1e-5
N = 50_000
CUT = 30_000  # the two snapshots: [0, CUT) and [CUT, N)
LEADS = (1, 2047, 2048, 2049, 4096)
MUST, SHOULD, MUST_NOT = 0, 1, 2

ENVS = [{"FUGU_RANK_GIB": "0"}, {"FUGU_RANK_GIB": "0.02", "FUGU_RANK_PLAIN_DIV": "16384"},
        {"FUGU_RANK_PLAIN_DIV": "16384"}, {"FUGU_RANK_PLAIN_DIV": "1"},
        {"FUGU_RANK_GIB": "0.05", "FUGU_RANK_PLAIN_DIV": "16"}]
ENV_IDS = ["directory_only", "few_rank_terms", "plain_rank_only", "sparse_rank_only", "all_kinds"]


@pytest.fixture(scope="module")
def native():
    from fugu_amd import native as nat
    if nat.device_count() == 0:
        pytest.fail("no GPU visible: the gpu tests must run on the MI355X box")
    assert (nat.OCCUR_MUST, nat.OCCUR_SHOULD, nat.OCCUR_MUST_NOT) == (MUST, SHOULD, MUST_NOT)
    return nat


@pytest.fixture(scope="module")
def ctx(native):
    return native.Context((0,))


@pytest.fixture(scope="module")
def case():
    """The synthetic corpus with hand-made terms at the top of the vocabulary,
    the batch (64 queries) and the oracle's answers for k = 10 and 100."""
    from fugu_amd import synth
    from oracle import oracle as orc
    V = synth.VOCAB
    c = synth.corpus(N)
    docs_of = {}
    docs_of["last"] = (V - 1, np.union1d(np.arange(0, N, 3), [N - 1]))  # the vocabulary's last term, dense
    # (the other hand-made terms: ids the synthetic corpus does not use, so their lists are exactly these)
    free = iter(np.setdiff1d(np.arange(V - 4096, V - 1), c.tok)[::-1].tolist())
    docs_of["dense"] = (next(free), np.union1d(np.arange(0, N, 2), [N - 1]))  # in half the docs: plain rank words
    docs_of["sparse"] = (next(free), np.union1d(np.arange(0, N, 100), [N - 1]))  # 1 / 100: sparse rank words by default
    docs_of["rare"] = (next(free), np.array([0, 12_345, CUT - 1, CUT, N - 1]))  # directory only
    for n in LEADS:
        t = next(free)
        d = np.array([N - 1]) if n == 1 else np.unique(np.round(np.linspace(0, N - 1, n)).astype(np.int64))
        assert len(d) == n and d[-1] == N - 1
        docs_of[n] = (t, d)
    # append the hand-made terms to their docs (one occurrence each)
    extra = [[] for _ in range(N)]
    for term, ds in docs_of.values():
        for d in ds:
            extra[int(d)].append(term)
    lens = np.diff(c.off).astype(np.int64) + np.array([len(e) for e in extra])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    tok = np.empty(int(off[-1]), np.uint32)
    src, dst = c.off.astype(np.int64), off.astype(np.int64)
    for d in range(N):
        n_own = int(src[d + 1] - src[d])
        tok[dst[d]:dst[d] + n_own] = c.tok[src[d]:src[d + 1]]
        tok[dst[d] + n_own:dst[d + 1]] = extra[d]
    T = {k: v[0] for k, v in docs_of.items()}
    qs, occ = [], []

    def add(terms, occur=None):
        qs.append(list(terms))
        occ.append(list(occur) if occur else [MUST] * len(terms))

    for n in LEADS:
        add([T[n], T["dense"]])                 # each lead length against plain rank words
        add([T["sparse"], T[n], T["last"]])     # ... as a 3-term AND (the deferred probes) with the last term
    add([T["rare"], T["dense"], T["sparse"]])   # matches doc 0 and doc N - 1, every probed hit at pos = df - 1 too
    add([T["last"], T["dense"]])                # the last term leading
    add([T[4096], T["rare"]])                   # a directory list probed
    add([T[2049], T["dense"], T["sparse"], T["last"]], [MUST, MUST, MUST_NOT, SHOULD])
    add([T[4096], T["last"], T["rare"], T["dense"]], [MUST, MUST_NOT, SHOULD, SHOULD])
    add([T["dense"], T[2048], 0, T["sparse"]], [MUST, MUST, SHOULD, MUST_NOT])
    q_off_s, terms_s = synth.queries(64 - len(qs), 3, 3, seed_q=404)
    for i in range(len(q_off_s) - 1):
        add(terms_s[q_off_s[i]:q_off_s[i + 1]].tolist())
    assert len(qs) == 64
    q_off = np.cumsum([0] + [len(q) for q in qs]).astype(np.uint32)
    terms = np.array([x for q in qs for x in q], np.uint32)
    occur = np.array([x for o in occ for x in o], np.uint8)
    ref = orc.OracleIndex(V, off, tok, threads=16)
    cuts = np.array([0, CUT, N], np.uint32)
    want, want_seg = {}, {}
    for k in (10, 100):
        rs, rd, rn, _, _ = ref.search_batch(q_off, terms, k, threads=16, occur=occur)
        want[k] = (rs, rd, rn)
        want_seg[k] = [ref.search(terms[q_off[i]:q_off[i + 1]], k, occur=occur[q_off[i]:q_off[i + 1]], seg_bounds=cuts)
                       for i in range(64)]
    # the cases are what they claim to be
    for i, n in enumerate(LEADS):
        assert ref.df(T[n]) == n
        assert want[100][2][2 * i] == min(100, len(np.intersect1d(docs_of[n][1], docs_of["dense"][1])))
    assert set(want[100][1][10, :want[100][2][10]].tolist()) == {0, CUT, N - 1}  # the `rare` query
    ref.close()
    return dict(V=V, off=off, tok=tok, q_off=q_off, terms=terms, occur=occur, want=want, want_seg=want_seg, cuts=cuts)


def with_env(env, build):
    old = {k: os.environ.get(k) for k in ("FUGU_RANK_GIB", "FUGU_RANK_PLAIN_DIV")}
    os.environ.update(env)
    try:
        return build()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def assert_hits(s, d, n, rs, rd, what):
    assert int(n) == len(rd), (what, int(n), len(rd))
    assert np.array_equal(np.asarray(d[:n], np.int64), np.asarray(rd, np.int64)), what
    rel = np.abs(s[:n].astype(np.float64) - rs) / np.maximum(np.abs(rs), 1e-30)
    assert (rel <= RTOL).all(), (what, rel.max())


@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
def test_one_snapshot_vs_oracle(native, ctx, case, env):
    c = case
    ix = with_env(env, lambda: native.Index.from_docs(ctx, c["off"], c["tok"], c["V"], threads=16))
    if env.get("FUGU_RANK_GIB") == "0":
        assert ix.stats().n_rank_terms == 0
    for k in (10, 100):
        s, d, n = ix.search_batch(c["q_off"], c["terms"], k, occur=c["occur"])
        rs, rd, rn = c["want"][k]
        assert np.array_equal(n, rn), (env, k)
        for i in range(64):
            assert_hits(s[i], d[i], n[i], rs[i, :rn[i]], rd[i, :rn[i]], (env, k, i))
    ix.close()


def segment_inputs(native, c):
    off, tok, V = c["off"], c["tok"], c["V"]
    a = (off[:CUT + 1].copy(), tok[:off[CUT]])
    b = (off[CUT:] - off[CUT], tok[off[CUT]:])
    g = native.docs_stats(*a, V, threads=16) + native.docs_stats(*b, V, threads=16)
    return a, b, g


def check_two_snapshots(native, c, ixs, what):
    """One plan over the two snapshots: the slot lists merged on the host, and
    the merged select, against the oracle's segmented search."""
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    nq = 64
    for k in (10, 100):
        p = native.Plan(ixs, c["q_off"], c["terms"], k, occur=c["occur"])
        p.execute()
        s, d, n = p.results()
        ms, md, msh, mn = merge_topk_numpy(s.reshape(2, nq, k), d.reshape(2, nq, k), n.reshape(2, nq), k)
        os_ = torch.zeros(nq * k, dtype=torch.float32, device=dev)
        od, osh = (torch.zeros(nq * k, dtype=torch.int32, device=dev) for _ in range(2))
        on = torch.zeros(nq, dtype=torch.int32, device=dev)
        p.execute_merged(st, os_.data_ptr(), od.data_ptr(), osh.data_ptr(), on.data_ptr())
        torch.cuda.synchronize()
        gs = os_.cpu().numpy().reshape(nq, k)
        gd = od.cpu().numpy().view(np.uint32).reshape(nq, k)
        gsh = osh.cpu().numpy().reshape(nq, k)
        gn = on.cpu().numpy()
        for i in range(nq):
            rs, rd = c["want_seg"][k][i]
            m = int(mn[i])
            assert_hits(ms[i], md[i, :m].astype(np.int64) + c["cuts"][msh[i, :m]], m, rs, rd, (what, "slots", k, i))
            m = int(gn[i])
            assert_hits(gs[i], gd[i, :m].astype(np.int64) + c["cuts"][gsh[i, :m]], m, rs, rd, (what, "merged", k, i))
        p.close()


@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
def test_two_snapshots_and_commit_elsewhere_vs_oracle(native, ctx, case, env):
    c = case
    a, b, g = segment_inputs(native, c)

    def build():
        own = native.Index.from_docs(ctx, *a, c["V"], threads=16, keep_host=False)  # the first commit: its own statistics
        return (own, native.Index.from_docs(ctx, *a, c["V"], threads=16, global_stats=g, keep_host=False),
                native.Index.from_docs(ctx, *b, c["V"], threads=16, global_stats=g, keep_host=False))

    own, seg_a, seg_b = with_env(env, build)
    check_two_snapshots(native, c, [seg_a, seg_b], (env, "built"))
    # the second commit rescored the first snapshot: scores from the payloads (feat 4)
    re_a = own.rescore(g)
    check_two_snapshots(native, c, [re_a, seg_b], (env, "rescored"))
    for k in (10, 100):  # ... and alone: a fresh build's hits, bit for bit
        x = re_a.search_batch(c["q_off"], c["terms"], k, occur=c["occur"])
        y = seg_a.search_batch(c["q_off"], c["terms"], k, occur=c["occur"])
        assert np.array_equal(x[2], y[2]), (env, k)
        for i in range(64):
            m = int(x[2][i])
            assert np.array_equal(x[1][i, :m], y[1][i, :m]) and np.array_equal(x[0][i, :m], y[0][i, :m]), (env, k, i)
    for ix in (own, seg_a, seg_b, re_a):
        ix.close()
