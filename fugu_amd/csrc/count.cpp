// fg_count_batch: hit totals and facet counts of a batch over a namespace's
// snapshots (tantivy's (Count, FacetCollector)).  Host side: the
// batch is checked and split into clauses once, then every snapshot translates
// it to its own ids and lays out one PASS per slice of the batch (the tables of
// fg_internal.h DevCount); all passes' tables go up in one copy, the passes run
// back to back on the calling thread's stream, and the summed totals and counts
// come back in one copy.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "fg_host.h"

using fgh::fail;

namespace {

// The match bitmaps of one pass stay within this many bytes (a slice holds at
// least one query): env FUGU_COUNT_WS_KB, read per call, default 256 MiB -- 2048
// queries over 1M docs, 20 over 100M.  The filter-union bitmaps of the slice's
// distinct filters (at most one per query) come on top.
size_t match_bound() {
  const char* e = getenv("FUGU_COUNT_WS_KB");
  const long long kb = e ? atoll(e) : 0;
  return kb > 0 ? (size_t)kb << 10 : (size_t)256 << 20;
}

// A batch query as clauses of vocabulary / facet-dictionary ids
struct Clauses {
  std::vector<uint32_t> must, should, must_not, filter;
  bool text = false;  // the query has text terms
};

// One pass's host tables; the DevCount pointers are offsets into the staging
// until the workspace's address is known
struct Pass {
  uint32_t seg = 0;
  fg::DevCount d{};
  size_t ws_bytes = 0;  // match + fbits
  size_t n_filters = 0;
};

struct Staging {
  std::vector<char> bytes;
  size_t put(const std::vector<uint32_t>& v) {
    const size_t o = bytes.size();
    bytes.resize(o + ((v.size() * 4 + 255) & ~size_t(255)));
    if (!v.empty()) std::memcpy(bytes.data() + o, v.data(), v.size() * 4);
    return o;
  }
};

thread_local struct CountTrace {
  bool on = false;
  double ms[4] = {0, 0, 0, 0};
  uint32_t calls = 0;
} g_trace;

int check_batch(const fg_query_batch* q, std::vector<Clauses>& out) {
  if (q->n_queries && !q->q_off) return fail(FG_EINVAL, "bad arguments");
  const uint32_t nq = q->n_queries;
  if (nq && q->q_off[nq] > q->q_off[0] && !q->terms) return fail(FG_EINVAL, "q_off without terms");
  if (q->f_off && nq && q->f_off[nq] > q->f_off[0] && !q->f_terms) return fail(FG_EINVAL, "f_off without f_terms");
  if (q->mode != FG_MODE_AND && q->mode != FG_MODE_OR) return fail(FG_EINVAL, "bad mode %d", q->mode);
  out.assign(nq, Clauses{});
  for (uint32_t i = 0; i < nq; ++i) {
    Clauses& c = out[i];
    const uint32_t b = q->q_off[i], e = q->q_off[i + 1];
    if (e < b) return fail(FG_EINVAL, "q_off not monotone at query %u", i);
    if (e - b > fg::kMaxTerms) return fail(FG_EUNSUPPORTED, "query %u has %u terms (> %u)", i, e - b, fg::kMaxTerms);
    c.text = e > b;
    for (uint32_t j = b; j < e; ++j) {
      if (q->phrase_len && (q->phrase_len[j] & (FG_CLAUSE_ANY | FG_CLAUSE_ALL)) && fg_group_clauses(-1) > 0)
        return fail(FG_EUNSUPPORTED, "query %u: group clause in a count query", i);
      if (q->phrase_len && q->phrase_len[j] >= 2) return fail(FG_EUNSUPPORTED, "query %u: phrase clause in a count query", i);
      const uint8_t oc = q->occur ? q->occur[j] : (q->mode == FG_MODE_OR ? FG_OCCUR_SHOULD : FG_OCCUR_MUST);
      if (oc > FG_OCCUR_MUST_NOT) return fail(FG_EINVAL, "query %u: bad occur %u", i, (unsigned)oc);
      (oc == FG_OCCUR_MUST ? c.must : oc == FG_OCCUR_SHOULD ? c.should : c.must_not).push_back(q->terms[j]);
    }
    if (q->f_off) {
      const uint32_t fb = q->f_off[i], fe = q->f_off[i + 1];
      if (fe < fb) return fail(FG_EINVAL, "f_off not monotone at query %u", i);
      if (fe - fb > fg::kMaxFacetClauses)
        return fail(FG_EUNSUPPORTED, "query %u has %u facet clauses (> %u)", i, fe - fb, fg::kMaxFacetClauses);
      c.filter.assign(q->f_terms + fb, q->f_terms + fe);
    }
  }
  return FG_OK;
}

// The passes of snapshot `seg`: its queries in slices of `rows` slots
int plan_snapshot(const fg_index* ix, uint32_t seg, const std::vector<Clauses>& cl, const uint32_t* count_terms,
                  uint32_t n_count, size_t bound, Staging& st, std::vector<Pass>& passes) {
  const uint32_t nq = (uint32_t)cl.size();
  const uint64_t N = ix->n_docs;
  if (N == 0) return FG_OK;
  const uint32_t words = (uint32_t)((N + 31) / 32);
  const uint32_t rows = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, bound / (4ull * words)), 1u << 20);
  auto present = [&](uint32_t t) { return t < ix->n_terms && ix->off[t + 1] > ix->off[t]; };
  auto flen = [&](uint32_t t) -> uint64_t {
    return t < ix->n_fterms && (size_t)t + 1 < ix->foff.size() ? ix->foff[t + 1] - ix->foff[t] : 0;
  };
  auto tlen = [&](uint32_t t) { return ix->off[t + 1] - ix->off[t]; };
  // the count terms' chunks: the same for every pass of the snapshot
  std::vector<uint32_t> cc_j, cc_t, cc_s;
  for (uint32_t j = 0; j < n_count; ++j) {
    const uint64_t n = flen(count_terms[j]);
    for (uint64_t s = 0; s < n; s += fg::kCountFacetChunk) {
      cc_j.push_back(j);
      cc_t.push_back(count_terms[j]);
      cc_s.push_back((uint32_t)s);
    }
  }
  if (cc_j.size() > 0x7FFFFFFFull) return fail(FG_EUNSUPPORTED, "count terms too long (%zu work items)", cc_j.size());
  const size_t o_ccj = st.put(cc_j), o_cct = st.put(cc_t), o_ccs = st.put(cc_s);

  std::vector<uint32_t> q_m, q_terms, q_filter, w_q, w_kind, w_term, w_start, fc_f, fc_t, fc_s;
  for (uint32_t a = 0; a < nq; a += rows) {
    const uint32_t n = std::min(rows, nq - a);
    q_m.assign(n, 0);
    q_terms.assign((size_t)n * fg::kMaxTerms, 0);
    q_filter.assign(n, 0xFFFFFFFFu);
    for (auto* v : {&w_q, &w_kind, &w_term, &w_start, &fc_f, &fc_t, &fc_s}) v->clear();
    std::map<std::vector<uint32_t>, uint32_t> fid;  // the present terms of a clause list -> fbits row
    auto drive = [&](uint32_t i, uint32_t kind, uint32_t t, uint64_t len) {
      for (uint64_t s = 0; s < len; s += fg::kCountChunk) {
        w_q.push_back(i);
        w_kind.push_back(kind);
        w_term.push_back(t);
        w_start.push_back((uint32_t)s);
      }
    };
    for (uint32_t i = 0; i < n; ++i) {
      const Clauses& c = cl[a + i];
      // the filter's facet terms this snapshot holds (a missing one matches nothing)
      std::vector<uint32_t> fl;
      for (uint32_t t : c.filter)
        if (flen(t) && std::find(fl.begin(), fl.end(), t) == fl.end()) fl.push_back(t);
      if (!c.filter.empty() && fl.empty()) continue;  // the union is empty: no matches
      if (!c.text) {
        if (c.filter.empty()) {  // AllQuery
          for (uint32_t w = 0; w < words; w += fg::kCountWordChunk) {
            w_q.push_back(i);
            w_kind.push_back(fg::kCountFill);
            w_term.push_back(0);
            w_start.push_back(w);
          }
        } else {  // the facet union alone
          for (uint32_t t : fl) drive(i, fg::kCountFacet, t, flen(t));
        }
        continue;
      }
      // the snapshot's own term ids; a Should or MustNot on a term it lacks is
      // dropped, a Must on one empties the query here
      std::vector<uint32_t> tm, ts, tx;
      bool must_missing = false;
      for (uint32_t t : c.must) {
        const uint32_t l = fgh::local_term(ix, t);
        must_missing |= !present(l);
        tm.push_back(l);
      }
      if (must_missing) continue;
      for (uint32_t t : c.should) {
        const uint32_t l = fgh::local_term(ix, t);
        if (present(l)) ts.push_back(l);
      }
      for (uint32_t t : c.must_not) {
        const uint32_t l = fgh::local_term(ix, t);
        if (present(l)) tx.push_back(l);
      }
      if (tm.empty() && ts.empty()) continue;  // no positive clause: no matches
      uint32_t* qt = q_terms.data() + (size_t)i * fg::kMaxTerms;
      uint32_t np = 0, nmust = 0;
      if (!tm.empty()) {
        // the shortest Must list drives, the others are probed
        const size_t lead = std::min_element(tm.begin(), tm.end(), [&](uint32_t x, uint32_t y) { return tlen(x) < tlen(y); }) -
                            tm.begin();
        for (size_t j = 0; j < tm.size(); ++j)
          if (j != lead) qt[np++] = tm[j];
        nmust = np;
        drive(i, fg::kCountText, tm[lead], tlen(tm[lead]));
      } else {
        for (uint32_t t : ts) drive(i, fg::kCountText, t, tlen(t));
      }
      for (uint32_t t : tx) qt[np++] = t;
      q_m[i] = fg::qm_pack(np, nmust, (uint32_t)tx.size());
      if (!c.filter.empty()) {
        auto it = fid.find(fl);
        if (it == fid.end()) {
          it = fid.emplace(fl, (uint32_t)fid.size()).first;
          for (uint32_t t : fl)
            for (uint64_t s = 0, len = flen(t); s < len; s += fg::kCountFacetChunk) {
              fc_f.push_back(it->second);
              fc_t.push_back(t);
              fc_s.push_back((uint32_t)s);
            }
        }
        q_filter[i] = it->second;
      }
    }
    if (w_q.empty()) continue;  // no query of the slice can match here
    if (w_q.size() > 0x7FFFFFFFull || fc_f.size() > 0x7FFFFFFFull ||
        (uint64_t)n * ((words + fg::kCountWordChunk - 1) / fg::kCountWordChunk) > 0x7FFFFFFFull)
      return fail(FG_EUNSUPPORTED, "batch too large (%zu work items)", w_q.size());
    Pass p;
    p.seg = seg;
    p.n_filters = fid.size();
    p.ws_bytes = ((size_t)n + fid.size()) * words * 4;
    fg::DevCount& d = p.d;
    d.nq = n;
    d.q0 = a;
    d.words = words;
    d.n_count = n_count;
    d.n_fchunks = (uint32_t)fc_f.size();
    d.n_items = (uint32_t)w_q.size();
    d.n_cchunks = (uint32_t)cc_j.size();
    auto at = [](size_t o) { return reinterpret_cast<const uint32_t*>(o); };
    d.fc_filter = at(st.put(fc_f));
    d.fc_term = at(st.put(fc_t));
    d.fc_start = at(st.put(fc_s));
    d.w_q = at(st.put(w_q));
    d.w_kind = at(st.put(w_kind));
    d.w_term = at(st.put(w_term));
    d.w_start = at(st.put(w_start));
    d.q_m = at(st.put(q_m));
    d.q_terms = at(st.put(q_terms));
    d.q_filter = at(st.put(q_filter));
    d.cc_j = at(o_ccj);
    d.cc_term = at(o_cct);
    d.cc_start = at(o_ccs);
    passes.push_back(p);
  }
  return FG_OK;
}

}  // namespace

extern "C" {

// fugu.h: the calling thread's per-kernel HIP-event timing of fg_count_batch (tools/bench_count.py)
int fg_count_trace(int enable, double* ms_out, uint32_t* calls) {
  for (int i = 0; i < 4; ++i) {
    if (ms_out) ms_out[i] = g_trace.ms[i];
    g_trace.ms[i] = 0;
  }
  if (calls) *calls = g_trace.calls;
  g_trace.calls = 0;
  if (enable >= 0) g_trace.on = enable != 0;
  return FG_OK;
}

int fg_count_batch(fg_index* const* ixs, uint32_t n_segs, const fg_query_batch* q, const uint32_t* count_terms,
                   uint32_t n_count, uint64_t* out_total, uint64_t* out_count) {
  if (!ixs || n_segs == 0 || !q) return fail(FG_EINVAL, "bad arguments");
  if (n_segs > FG_MAX_SEGMENTS) return fail(FG_EUNSUPPORTED, "%u snapshots > FG_MAX_SEGMENTS=%d", n_segs, FG_MAX_SEGMENTS);
  for (uint32_t s = 0; s < n_segs; ++s) {
    if (!ixs[s]) return fail(FG_EINVAL, "NULL snapshot");
    if (ixs[s]->dev != ixs[0]->dev) return fail(FG_EUNSUPPORTED, "count over snapshots on several devices");
  }
  const uint32_t nq = q->n_queries;
  if (nq && !out_total) return fail(FG_EINVAL, "out_total is NULL");
  if (n_count && (!count_terms || (nq && !out_count))) return fail(FG_EINVAL, "n_count without count_terms / out_count");
  if (n_count > FG_MAX_COUNT_TERMS) return fail(FG_EUNSUPPORTED, "n_count=%u > FG_MAX_COUNT_TERMS=%d", n_count, FG_MAX_COUNT_TERMS);
  if ((uint64_t)nq * n_count > FG_MAX_COUNT_CELLS)
    return fail(FG_EUNSUPPORTED, "n_queries * n_count = %llu > FG_MAX_COUNT_CELLS=%d", (unsigned long long)nq * n_count,
                FG_MAX_COUNT_CELLS);
  std::vector<Clauses> cl;
  if (int rc = check_batch(q, cl)) return rc;
  if (nq == 0) return FG_OK;

  Staging st;
  std::vector<Pass> passes;
  const size_t bound = match_bound();
  for (uint32_t s = 0; s < n_segs; ++s)
    if (int rc = plan_snapshot(ixs[s], s, cl, count_terms, n_count, bound, st, passes)) return rc;

  const size_t n_out = (size_t)nq * (1 + (size_t)n_count);  // totals, then counts
  if (passes.empty()) {
    std::memset(out_total, 0, 8ull * nq);
    if (n_count) std::memset(out_count, 0, 8ull * nq * n_count);
    return FG_OK;
  }
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  size_t ws_max = 0;
  for (const Pass& p : passes) ws_max = std::max(ws_max, p.ws_bytes);
  const size_t s_tab = al(st.bytes.size()), s_out = al(8 * n_out), total = s_tab + s_out + al(ws_max);

  fg_index* ix0 = ixs[0];
  HIPCHK(hipSetDevice(ix0->dev));
  size_t got = 0;
  char* base = static_cast<char*>(ix0->pool->get(total, &got));
  if (!base) return fail(FG_EOOM, "count workspace hipMalloc(%zu) failed", total);
  struct Back {
    WsPool& pool;
    void* p;
    size_t n;
    ~Back() { pool.put(p, n); }
  } back{*ix0->pool, base, got};
  // the calling thread's own stream, as fg_search_batch: concurrent callers run side by side
  hipStream_t s = hipStreamPerThread;
  // every return below first waits for the stream: the workspace goes back to the pool
  auto finish = [&](int rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  };
  PinnedLease pin(*ix0->pinned, std::max(st.bytes.size(), 8 * n_out));
  const void* src = st.bytes.data();
  if (pin.p) {
    std::memcpy(pin.p, st.bytes.data(), st.bytes.size());
    src = pin.p;
  }
  if (hipMemcpyAsync(base, src, st.bytes.size(), hipMemcpyHostToDevice, s) != hipSuccess)
    return finish(fail(FG_EHIP, "count tables upload failed"));
  // (the staging is read again only after the stream has drained: the result copy below)
  unsigned long long* d_out = reinterpret_cast<unsigned long long*>(base + s_tab);
  if (hipMemsetAsync(d_out, 0, 8 * n_out, s) != hipSuccess) return finish(fail(FG_EHIP, "hipMemsetAsync failed"));
  char* ws = base + s_tab + s_out;

  // fg_count_trace's events, 5 per pass; destroyed on every way out
  struct Events {
    std::vector<hipEvent_t> v;
    ~Events() {
      for (hipEvent_t x : v)
        if (x) (void)hipEventDestroy(x);
    }
  } events;
  std::vector<hipEvent_t>& evs = events.v;
  const bool trace = g_trace.on;
  for (Pass& p : passes) {
    fg::DevCount& d = p.d;
    auto bind = [&](const uint32_t*& f) { f = reinterpret_cast<const uint32_t*>(base + reinterpret_cast<size_t>(f)); };
    for (auto* f : {&d.fc_filter, &d.fc_term, &d.fc_start, &d.w_q, &d.w_kind, &d.w_term, &d.w_start, &d.q_m, &d.q_terms,
                    &d.q_filter, &d.cc_j, &d.cc_term, &d.cc_start})
      bind(*f);
    d.match = reinterpret_cast<uint32_t*>(ws);
    d.fbits = d.match + (size_t)d.nq * d.words;
    d.total = d_out;
    d.count = d_out + nq;
    if (hipMemsetAsync(ws, 0, p.ws_bytes, s) != hipSuccess) return finish(fail(FG_EHIP, "hipMemsetAsync failed"));
    hipEvent_t* ev = nullptr;
    if (trace) {
      const size_t o = evs.size();
      evs.resize(o + 5, nullptr);
      bool ok = true;
      for (size_t i = o; i < o + 5; ++i) ok &= hipEventCreate(&evs[i]) == hipSuccess;
      if (ok) ev = evs.data() + o;
    }
    const hipError_t e = fg::launch_count(ixs[p.seg]->d, d, s, ev);
    if (e != hipSuccess) return finish(fail(FG_EHIP, "count kernels: %s", hipGetErrorString(e)));
  }
  // pinned when had: the pageable outputs are filled by one memcpy each after the sync
  void* dst = pin.p ? pin.p : nullptr;
  std::vector<uint64_t> host_out;
  if (!dst) {
    host_out.resize(n_out);
    dst = host_out.data();
  }
  hipError_t e = hipMemcpyAsync(dst, d_out, 8 * n_out, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (trace && e == hipSuccess) {
    for (size_t o = 0; o + 5 <= evs.size(); o += 5)
      for (int i = 0; i < 4; ++i) {
        float ms = 0.0f;
        if (evs[o + i] && evs[o + i + 1] && hipEventElapsedTime(&ms, evs[o + i], evs[o + i + 1]) == hipSuccess)
          g_trace.ms[i] += ms;
      }
    ++g_trace.calls;
  }
  if (e != hipSuccess) return finish(fail(FG_EHIP, "count results: %s", hipGetErrorString(e)));
  std::memcpy(out_total, dst, 8ull * nq);
  if (n_count) std::memcpy(out_count, static_cast<const uint64_t*>(dst) + nq, 8ull * nq * n_count);
  return FG_OK;
}

}  // extern "C"
