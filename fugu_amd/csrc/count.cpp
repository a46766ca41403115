// fg_count_batch: hit totals and facet counts of a batch over a namespace's
// snapshots (tantivy's (Count, FacetCollector)).  Host side: the
// batch is checked and split into clauses once, then every snapshot translates
// it to its own ids and lays out one PASS per slice of the batch (the tables of
// fg_internal.h DevCount); all passes' tables go up in one copy, the passes run
// back to back on the calling thread's stream, and the summed totals and counts
// come back in one copy.  With fg_count_clauses on a phrase or
// group clause becomes one bitmap row per distinct clause of a slice (k_crow),
// and the slots that hold one are joined by k_cjoin instead of k_cmatch.
#include <algorithm>
#include <atomic>
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
// distinct filters (at most one per query) come on top; the slice's distinct
// clause rows (fg_count_clauses) count inside the bound, with the match bitmaps.
size_t match_bound() {
  const char* e = getenv("FUGU_COUNT_WS_KB");
  const long long kb = e ? atoll(e) : 0;
  return kb > 0 ? (size_t)kb << 10 : (size_t)256 << 20;
}

// fg_count_clauses: phrase and group clauses are counted; process-wide, off by default
std::atomic<int> count_clauses_on{0};

// A phrase or group clause of a batch query (fg_count_clauses): one bitmap row per snapshot
struct RowClause {
  uint32_t kind = 0;  // fg::kRowAny / kRowAll / kRowPhrase
  uint8_t occur = 0;
  std::vector<uint32_t> terms, pos;  // vocabulary ids; a phrase's offsets
};

// A batch query as clauses of vocabulary / facet-dictionary ids
struct Clauses {
  std::vector<uint32_t> must, should, must_not, filter;
  std::vector<RowClause> rows;
  bool text = false;  // the query has text terms
};

// One pass's host tables; the DevCount pointers are offsets into the staging
// until the workspace's address is known
struct Pass {
  uint32_t seg = 0;
  fg::DevCount d{};
  size_t ws_bytes = 0;  // match + fbits + cbits
  size_t n_filters = 0;
};

// A batch query in one snapshot: its ids there, absent clauses resolved
using RowKey = std::vector<uint32_t>;  // kind, then the snapshot's term ids, then a phrase's offsets
struct Slot {
  bool none = false;  // no doc of the snapshot can match
  std::vector<uint32_t> fl, tm, ts, tx;
  std::vector<RowKey> rm, rs, rx;  // Must / Should / MustNot rows
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
thread_local struct ClauseTrace {  // fg_count_clause_trace: k_crow, k_cjoin
  bool on = false;
  double ms[2] = {0, 0};
  uint32_t calls = 0;
} g_ctrace;

// The clause table of query i with fg_count_clauses on: the planner's rules and
// messages (plan.cpp:plan_phrase); group flags count whatever fg_group_clauses says
int check_clauses(fg_index* const* ixs, uint32_t n_segs, const fg_query_batch* q, uint32_t i, Clauses& c) {
  const uint32_t b = q->q_off[i], e = q->q_off[i + 1];
  const uint32_t both = FG_CLAUSE_ANY | FG_CLAUSE_ALL;
  for (uint32_t j = b; j < e;) {
    const uint32_t raw = q->phrase_len[j], kind = raw & both;
    const uint32_t n = raw & ~both;
    // a field clause (fg_field_clauses) is not counted on the device, whatever the other switches say
    if ((raw & (FG_CLAUSE_TEXT | FG_CLAUSE_NAME)) && fg_field_clauses(-1) > 0)
      return fail(FG_EUNSUPPORTED, "query %u: field clause in a count query", i);
    if (kind) {
      if (kind == both || n < 2 || n > e - j) return fail(FG_EINVAL, "query %u: bad phrase_len at term %u", i, j - b);
      for (uint32_t x = 0; x < n; ++x) {
        if (x && q->phrase_len[j + x] != 0) return fail(FG_EINVAL, "query %u: phrase_len inside a group must be 0", i);
        if (q->phrase_pos[j + x] != 0) return fail(FG_EINVAL, "query %u: a group member's offset must be 0", i);
      }
    } else {
      if (n == 0 || n > e - j) return fail(FG_EINVAL, "query %u: bad phrase_len at term %u", i, j - b);
      for (uint32_t x = 1; x < n; ++x)
        if (q->phrase_len[j + x] != 0) return fail(FG_EINVAL, "query %u: phrase_len inside a phrase must be 0", i);
      if (n >= 2) {
        if (q->phrase_pos[j] != 0) return fail(FG_EINVAL, "query %u: a phrase's first offset must be 0", i);
        for (uint32_t x = 1; x < n; ++x)
          if (q->phrase_pos[j + x] <= q->phrase_pos[j + x - 1])
            return fail(FG_EINVAL, "query %u: phrase offsets must increase", i);
        for (uint32_t s = 0; s < n_segs; ++s)
          if (!ixs[s]->has_positions) return fail(FG_EUNSUPPORTED, "query %u: snapshot built without positions", i);
        if (q->phrase_pos[j + n - 1] >= (1u << 30)) return fail(FG_EINVAL, "query %u: phrase offset too large", i);
      }
    }
    const uint8_t oc = q->occur ? q->occur[j] : (q->mode == FG_MODE_OR ? FG_OCCUR_SHOULD : FG_OCCUR_MUST);
    if (oc > FG_OCCUR_MUST_NOT) return fail(FG_EINVAL, "query %u: bad occur %u", i, (unsigned)oc);
    if (n == 1) {
      (oc == FG_OCCUR_MUST ? c.must : oc == FG_OCCUR_SHOULD ? c.should : c.must_not).push_back(q->terms[j]);
    } else {
      RowClause r;
      r.kind = kind == FG_CLAUSE_ANY ? fg::kRowAny : kind == FG_CLAUSE_ALL ? fg::kRowAll : fg::kRowPhrase;
      r.occur = oc;
      r.terms.assign(q->terms + j, q->terms + j + n);
      if (!kind) r.pos.assign(q->phrase_pos + j, q->phrase_pos + j + n);
      c.rows.push_back(std::move(r));
    }
    j += n;
  }
  return FG_OK;
}

// clauses: fg_count_clauses as this call read it
int check_batch(fg_index* const* ixs, uint32_t n_segs, const fg_query_batch* q, bool clauses, std::vector<Clauses>& out) {
  if (clauses && q->phrase_len && !q->phrase_pos) return fail(FG_EINVAL, "phrase_len without phrase_pos");
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
    const bool table = clauses && q->phrase_len;  // the clause table decides, not the single entries below
    if (table)
      if (int rc = check_clauses(ixs, n_segs, q, i, c)) return rc;
    for (uint32_t j = b; j < e && !table; ++j) {
      if (q->phrase_len && (q->phrase_len[j] & (FG_CLAUSE_TEXT | FG_CLAUSE_NAME)) && fg_field_clauses(-1) > 0)
        return fail(FG_EUNSUPPORTED, "query %u: field clause in a count query", i);
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

// The passes of snapshot `seg`: its queries in slices of at most `rows` slots and clause rows together
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

  // Query i in this snapshot: its own term ids; a Should or MustNot clause on a
  // term it lacks is dropped, a Must on one empties the query here.  A phrase
  // with a term it lacks and an all-of group with a member it lacks are absent as
  // a whole; an any-of group goes on without such members, absent when none is left.
  auto resolve = [&](uint32_t i) {
    const Clauses& c = cl[i];
    Slot s;
    // the filter's facet terms this snapshot holds (a missing one matches nothing)
    for (uint32_t t : c.filter)
      if (flen(t) && std::find(s.fl.begin(), s.fl.end(), t) == s.fl.end()) s.fl.push_back(t);
    if (!c.filter.empty() && s.fl.empty()) s.none = true;  // the union is empty: no matches
    if (s.none || !c.text) return s;
    for (uint32_t t : c.must) {
      const uint32_t l = fgh::local_term(ix, t);
      s.none |= !present(l);
      s.tm.push_back(l);
    }
    for (uint32_t t : c.should) {
      const uint32_t l = fgh::local_term(ix, t);
      if (present(l)) s.ts.push_back(l);
    }
    for (uint32_t t : c.must_not) {
      const uint32_t l = fgh::local_term(ix, t);
      if (present(l)) s.tx.push_back(l);
    }
    for (const RowClause& r : c.rows) {
      RowKey key{r.kind};
      bool absent = false;
      for (uint32_t t : r.terms) {
        const uint32_t l = fgh::local_term(ix, t);
        if (present(l)) key.push_back(l);
        else if (r.kind != fg::kRowAny) absent = true;
      }
      if (r.kind != fg::kRowPhrase) {  // a group is a set of members
        std::sort(key.begin() + 1, key.end());
        key.erase(std::unique(key.begin() + 1, key.end()), key.end());
      }
      absent |= key.size() == 1;
      if (absent) {
        s.none |= r.occur == FG_OCCUR_MUST;
        continue;
      }
      key.insert(key.end(), r.pos.begin(), r.pos.end());
      (r.occur == FG_OCCUR_MUST ? s.rm : r.occur == FG_OCCUR_SHOULD ? s.rs : s.rx).push_back(std::move(key));
    }
    if (s.tm.empty() && s.ts.empty() && s.rm.empty() && s.rs.empty()) s.none = true;  // no positive clause: no matches
    return s;
  };

  std::vector<uint32_t> q_m, q_terms, q_filter, w_q, w_kind, w_term, w_start, fc_f, fc_t, fc_s;
  std::vector<uint32_t> q_rm, q_rows, j_q, j_kind, j_term, j_start, r_row, r_term, r_start, row_m, row_terms, row_pterm,
      row_ppos;
  std::vector<Slot> slots;
  for (uint32_t a = 0, n = 0; a < nq; a += n) {
    // the slice: as many queries as keep the match rows and the distinct clause rows within the bound
    // (identical clauses share a row: a batch around one phrase verifies it once), at least one
    std::map<RowKey, uint32_t> rid;  // a clause in this snapshot -> cbits row
    slots.clear();
    for (n = 0; a + n < nq && n < rows; ++n) {
      Slot s = resolve(a + n);
      std::vector<const RowKey*> fresh;
      if (!s.none)
        for (const auto* v : {&s.rm, &s.rs, &s.rx})
          for (const RowKey& k : *v)
            if (rid.emplace(k, 0).second) fresh.push_back(&k);
      if (n && (uint64_t)n + 1 + rid.size() > rows) {
        for (const RowKey* k : fresh) rid.erase(*k);
        break;
      }
      slots.push_back(std::move(s));
    }
    uint32_t n_rows = 0;
    for (auto& kv : rid) kv.second = n_rows++;
    q_m.assign(n, 0);
    q_terms.assign((size_t)n * fg::kMaxTerms, 0);
    q_filter.assign(n, 0xFFFFFFFFu);
    for (auto* v : {&w_q, &w_kind, &w_term, &w_start, &fc_f, &fc_t, &fc_s, &j_q, &j_kind, &j_term, &j_start, &r_row, &r_term,
                    &r_start})
      v->clear();
    q_rm.assign(n_rows ? n : 0, 0);
    q_rows.assign(n_rows ? (size_t)n * fg::kMaxTerms : 0, 0);
    row_m.assign(n_rows, 0);
    for (auto* v : {&row_terms, &row_pterm, &row_ppos}) v->assign((size_t)n_rows * fg::kMaxTerms, 0);
    // the rows' tables and k_crow's items
    for (const auto& kv : rid) {
      const RowKey& k = kv.first;
      const uint32_t r = kv.second, kind = k[0];
      const size_t at = (size_t)r * fg::kMaxTerms;
      auto crow = [&](uint32_t t) {
        for (uint64_t s = 0, len = tlen(t); s < len; s += fg::kCountChunk) {
          r_row.push_back(r);
          r_term.push_back(t);
          r_start.push_back((uint32_t)s);
        }
      };
      if (kind == fg::kRowAny) {  // every present member drives
        for (size_t j = 1; j < k.size(); ++j) crow(k[j]);
        row_m[r] = fg::row_pack(kind, 0, 0);
        continue;
      }
      // the phrase's terms: the first half of the rest of the key; its distinct terms in written order
      const uint32_t m = kind == fg::kRowPhrase ? (uint32_t)(k.size() - 1) / 2 : (uint32_t)k.size() - 1;
      std::vector<uint32_t> dist;
      for (uint32_t j = 0; j < m; ++j)
        if (std::find(dist.begin(), dist.end(), k[1 + j]) == dist.end()) dist.push_back(k[1 + j]);
      // the shortest list drives, the other distinct terms are probed
      const uint32_t lead = *std::min_element(dist.begin(), dist.end(), [&](uint32_t x, uint32_t y) { return tlen(x) < tlen(y); });
      uint32_t np = 0;
      for (uint32_t t : dist)
        if (t != lead) row_terms[at + np++] = t;
      if (kind == fg::kRowPhrase) {  // (vocabulary id, offset), the anchor -- the lead's first occurrence -- first
        const uint32_t anchor = (uint32_t)(std::find(k.begin() + 1, k.begin() + 1 + m, lead) - (k.begin() + 1));
        for (uint32_t j = 0, o = 1; j < m; ++j) {
          const uint32_t dst = j == anchor ? 0 : o++;
          row_pterm[at + dst] = ix->tmap.empty() ? k[1 + j] : ix->tmap[k[1 + j]];
          row_ppos[at + dst] = k[1 + m + j];
        }
      }
      row_m[r] = fg::row_pack(kind, np, kind == fg::kRowPhrase ? m : 0);
      crow(lead);
    }
    std::map<std::vector<uint32_t>, uint32_t> fid;  // the present terms of a clause list -> fbits row
    auto drive = [&](uint32_t i, uint32_t kind, uint32_t t, uint64_t len) {
      for (uint64_t s = 0; s < len; s += fg::kCountChunk) {
        w_q.push_back(i);
        w_kind.push_back(kind);
        w_term.push_back(t);
        w_start.push_back((uint32_t)s);
      }
    };
    auto jdrive = [&](uint32_t i, uint32_t t) {  // k_cjoin: a list driver
      for (uint64_t s = 0, len = tlen(t); s < len; s += fg::kCountChunk) {
        j_q.push_back(i);
        j_kind.push_back(fg::kCountText);
        j_term.push_back(t);
        j_start.push_back((uint32_t)s);
      }
    };
    auto jrow = [&](uint32_t i, uint32_t r) {  // ... a row driver
      for (uint32_t w = 0; w < words; w += fg::kCountWordChunk) {
        j_q.push_back(i);
        j_kind.push_back(fg::kCountRow);
        j_term.push_back(r);
        j_start.push_back(w);
      }
    };
    for (uint32_t i = 0; i < n; ++i) {
      const Clauses& c = cl[a + i];
      const Slot& sl = slots[i];
      if (sl.none) continue;
      const std::vector<uint32_t>&fl = sl.fl, &tm = sl.tm, &ts = sl.ts, &tx = sl.tx;
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
      const bool join = !(sl.rm.empty() && sl.rs.empty() && sl.rx.empty());  // a slot with a row is k_cjoin's
      uint32_t* qt = q_terms.data() + (size_t)i * fg::kMaxTerms;
      uint32_t np = 0, nmust = 0;
      if (!tm.empty()) {
        // the shortest Must list drives, the others are probed (and the rows only tested)
        const size_t lead = std::min_element(tm.begin(), tm.end(), [&](uint32_t x, uint32_t y) { return tlen(x) < tlen(y); }) -
                            tm.begin();
        for (size_t j = 0; j < tm.size(); ++j)
          if (j != lead) qt[np++] = tm[j];
        nmust = np;
        if (join) jdrive(i, tm[lead]);
        else drive(i, fg::kCountText, tm[lead], tlen(tm[lead]));
      } else if (!sl.rm.empty()) {  // the Musts are rows only: the first drives
        jrow(i, rid[sl.rm[0]]);
      } else {
        for (uint32_t t : ts) {
          if (join) jdrive(i, t);
          else drive(i, fg::kCountText, t, tlen(t));
        }
        for (const RowKey& k : sl.rs) jrow(i, rid[k]);
      }
      for (uint32_t t : tx) qt[np++] = t;
      if (join) {  // the tested rows: [Must rows][MustNot rows]
        uint32_t* qr = q_rows.data() + (size_t)i * fg::kMaxTerms;
        uint32_t nr = 0;
        for (const RowKey& k : sl.rm) qr[nr++] = rid[k];
        const uint32_t nrmust = nr;
        for (const RowKey& k : sl.rx) qr[nr++] = rid[k];
        q_rm[i] = nr | (nrmust << 16);
      }
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
    if (w_q.empty() && j_q.empty()) continue;  // no query of the slice can match here
    if (w_q.size() > 0x7FFFFFFFull || fc_f.size() > 0x7FFFFFFFull || j_q.size() > 0x7FFFFFFFull ||
        r_row.size() > 0x7FFFFFFFull ||
        (uint64_t)n * ((words + fg::kCountWordChunk - 1) / fg::kCountWordChunk) > 0x7FFFFFFFull)
      return fail(FG_EUNSUPPORTED, "batch too large (%zu work items)", w_q.size() + j_q.size() + r_row.size());
    Pass p;
    p.seg = seg;
    p.n_filters = fid.size();
    p.ws_bytes = ((size_t)n + fid.size() + n_rows) * words * 4;
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
    d.n_ritems = (uint32_t)r_row.size();
    d.n_jitems = (uint32_t)j_q.size();
    if (n_rows) {  // (without a row the pointers stay NULL: no kernel reads them)
      d.r_row = at(st.put(r_row));
      d.r_term = at(st.put(r_term));
      d.r_start = at(st.put(r_start));
      d.row_m = at(st.put(row_m));
      d.row_terms = at(st.put(row_terms));
      d.row_pterm = at(st.put(row_pterm));
      d.row_ppos = at(st.put(row_ppos));
      d.j_q = at(st.put(j_q));
      d.j_kind = at(st.put(j_kind));
      d.j_term = at(st.put(j_term));
      d.j_start = at(st.put(j_start));
      d.q_rm = at(st.put(q_rm));
      d.q_rows = at(st.put(q_rows));
    }
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

// fugu.h: the same for the two kernels of clause rows, k_crow and k_cjoin (tools/bench_count_clauses.py)
int fg_count_clause_trace(int enable, double* ms_out, uint32_t* calls) {
  for (int i = 0; i < 2; ++i) {
    if (ms_out) ms_out[i] = g_ctrace.ms[i];
    g_ctrace.ms[i] = 0;
  }
  if (calls) *calls = g_ctrace.calls;
  g_ctrace.calls = 0;
  if (enable >= 0) g_ctrace.on = enable != 0;
  return FG_OK;
}

int fg_count_clauses(int on) {
  if (on < 0) return count_clauses_on.load(std::memory_order_relaxed);
  return count_clauses_on.exchange(on != 0 ? 1 : 0, std::memory_order_relaxed);
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
  const bool clauses = fg_count_clauses(-1) > 0;  // read once per call
  if (int rc = check_batch(ixs, n_segs, q, clauses, cl)) return rc;
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

  // fg_count_trace's and fg_count_clause_trace's events, destroyed on every way out; evs: kCountEvents
  // slots per pass (a pass without clause rows records 5 events as before: the slots around the
  // kernels it does not launch share one)
  struct Events {
    std::vector<hipEvent_t> v;
    ~Events() {
      for (hipEvent_t x : v)
        if (x) (void)hipEventDestroy(x);
    }
  } events;
  std::vector<hipEvent_t> evs;
  const bool trace = g_trace.on || g_ctrace.on;
  constexpr size_t kEv = fg::kCountEvents;
  for (Pass& p : passes) {
    fg::DevCount& d = p.d;
    auto bind = [&](const uint32_t*& f) { f = reinterpret_cast<const uint32_t*>(base + reinterpret_cast<size_t>(f)); };
    for (auto* f : {&d.fc_filter, &d.fc_term, &d.fc_start, &d.w_q, &d.w_kind, &d.w_term, &d.w_start, &d.q_m, &d.q_terms,
                    &d.q_filter, &d.cc_j, &d.cc_term, &d.cc_start})
      bind(*f);
    if (d.n_jitems)
      for (auto* f : {&d.r_row, &d.r_term, &d.r_start, &d.row_m, &d.row_terms, &d.row_pterm, &d.row_ppos, &d.j_q, &d.j_kind,
                      &d.j_term, &d.j_start, &d.q_rm, &d.q_rows})
        bind(*f);
    d.match = reinterpret_cast<uint32_t*>(ws);
    d.fbits = d.match + (size_t)d.nq * d.words;
    d.cbits = d.fbits + p.n_filters * d.words;
    d.total = d_out;
    d.count = d_out + nq;
    if (hipMemsetAsync(ws, 0, p.ws_bytes, s) != hipSuccess) return finish(fail(FG_EHIP, "hipMemsetAsync failed"));
    hipEvent_t* ev = nullptr;
    if (trace) {
      const size_t o = evs.size();
      evs.resize(o + kEv, nullptr);
      const bool rows = d.n_ritems || d.n_jitems;
      bool ok = true;
      for (size_t i = 0; i < kEv; ++i) {
        if (!rows && (i == 2 || i == 4)) {  // after k_crow / k_cjoin, not launched: the slot before
          evs[o + i] = evs[o + i - 1];
          continue;
        }
        hipEvent_t x = nullptr;
        ok &= hipEventCreate(&x) == hipSuccess;
        events.v.push_back(x);
        evs[o + i] = x;
      }
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
    // the span after event x of launch_count: k_cfilter 0, k_crow 1, k_cmatch 2, k_cjoin 3, k_ccount 4, k_cfacet 5
    static const int span4[4] = {0, 2, 4, 5}, span2[2] = {1, 3};
    auto span = [&](size_t x) {
      float ms = 0.0f;
      return evs[x] && evs[x + 1] && hipEventElapsedTime(&ms, evs[x], evs[x + 1]) == hipSuccess ? (double)ms : 0.0;
    };
    for (size_t o = 0; o + kEv <= evs.size(); o += kEv) {
      if (g_trace.on)
        for (int i = 0; i < 4; ++i) g_trace.ms[i] += span(o + span4[i]);
      if (g_ctrace.on)
        for (int i = 0; i < 2; ++i) g_ctrace.ms[i] += span(o + span2[i]);
    }
    if (g_trace.on) ++g_trace.calls;
    if (g_ctrace.on) ++g_ctrace.calls;
  }
  if (e != hipSuccess) return finish(fail(FG_EHIP, "count results: %s", hipGetErrorString(e)));
  std::memcpy(out_total, dst, 8ull * nq);
  if (n_count) std::memcpy(out_count, static_cast<const uint64_t*>(dst) + nq, 8ull * nq * n_count);
  return FG_OK;
}

}  // extern "C"
