// libfugu batch planning (host only until the upload): each snapshot's side of
// a batch (plan_host), the pieces joined into one set of tables and work
// items, the items ordered for the kernels, and ONE workspace laid out, staged
// and uploaded.  fugu.cpp executes the plans.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fg_host.h"

using fgh::fail;

// (the bin width: the f32 bit patterns [lo, hi] in fewer than kQBins bins of 2^shift ulps)
fgh::Bins fgh::union_bins(uint32_t lo, uint32_t hi) {
  hi = std::max(hi, lo);
  uint32_t sh = 0;
  while (sh < 31 && ((uint64_t)(hi - lo) >> sh) >= fg::kQBins - 1) ++sh;
  return Bins{lo, hi, sh};
}

namespace {

// fg_phrase_clauses: queries with a phrase clause beside other clauses run on the
// device (k_bphrase); process-wide, off by default, read when a plan is created
std::atomic<int> phrase_clauses_on{0};
// fg_group_clauses: queries with a group clause run on the device (k_group); the same contract
std::atomic<int> group_clauses_on{0};
// fg_filter_clauses: phrase, phrase-beside and group queries may carry facet clauses; the same contract
std::atomic<int> filter_clauses_on{0};
// fg_group_phrase_clauses: queries with a group clause beside a phrase clause run on the device (k_gphrase); the
// same contract
std::atomic<int> group_phrase_clauses_on{0};
// fg_group_member_phrases: a group may hold phrase members (k_mgroup); the same contract
std::atomic<int> group_member_phrases_on{0};
// fg_field_clauses: queries with a field-qualified term clause run on the device (k_field); the same contract
std::atomic<int> field_clauses_on{0};
// fg_field_phrases: on top of fg_field_clauses, a field may stand on a phrase clause and a field term beside a
// phrase clause (k_fphrase); the same contract
std::atomic<int> field_phrases_on{0};

// stable LSD radix sort of `a` by its bits 32..63 (three 11-bit passes)
void radix_sort_hi32(std::vector<uint64_t>& a, std::vector<uint64_t>& tmp) {
  tmp.resize(a.size());
  for (int sh = 32; sh < 64; sh += 11) {
    uint32_t cnt[2049] = {0};
    for (uint64_t x : a) cnt[((x >> sh) & 2047u) + 1]++;
    for (int d = 0; d < 2048; ++d) cnt[d + 1] += cnt[d];
    for (uint64_t x : a) tmp[cnt[(x >> sh) & 2047u]++] = x;
    a.swap(tmp);
  }
}

struct WItem { double key; uint32_t q, c, n; };

// The host tables of a planned batch.  plan_host fills one per piece (one
// snapshot's side, built on the host alone, no HIP call: per-query tables,
// facet filters with ids local to the snapshot, unsorted work items);
// join_pieces joins several into one of query slots v = s * nq + q.
struct PlanTables {
  // per query (slot); the q_terms .. q_rup rows hold kMaxTerms entries each
  std::vector<uint32_t> q_m, q_terms, lead, q_filter, ngroup, q_hlo, q_hhi, q_hsh;
  std::vector<uint32_t> q_tier;  // DevPlan::q_tier: slots that lead from a score-tiered copy
  std::vector<uint32_t> q_pterm, q_ppos;  // phrase queries' (term, offset) rows; empty without phrase_len
  std::vector<uint32_t> q_clause;         // DevPlan::q_clause (k_bphrase / k_group / k_field slots); empty unless
                                          // fg_phrase_clauses, fg_group_clauses or fg_field_clauses is on
  std::vector<uint32_t> q_member;         // DevPlan::q_member (k_mgroup slots); empty unless fg_group_member_phrases
  std::vector<uint64_t> thr0;
  std::vector<float> q_ub, q_wt, q_wn, q_rup;
  std::vector<fg::ProbeDesc> q_probe;  // k_conj slots' probe descriptors (rows as above)
  // facet filters (fg_internal.h DevFilters) and the chunks of their postings
  uint32_t nf = 0;
  std::vector<uint32_t> f_shift, f_seg;  // f_seg: the filter's snapshot (joined tables only)
  std::vector<uint64_t> f_woff;
  std::vector<float> f_tab, f_max;
  std::vector<uint32_t> ch_f, ch_c, ch_t, ch_s;
  // work items: k_conj's, k_disj's, k_scan's, k_phrase's, k_bphrase's, k_group's, k_gphrase's, k_mgroup's, k_field's, k_fphrase's; items: all
  // of them as the kernels run them (order_items, joined tables only)
  std::vector<WItem> citems, ditems, scan, phrase, bphrase, group, gphrase, mgroup, field, fphrase, items;
  // (a thread's plans reuse one set: assign / push_back into kept capacity, no
  // page faults on fresh arrays -- ~0.2 ms of an 8-snapshot batch's planning)
  void clear() {
    auto all = [](auto&... v) { (v.clear(), ...); };
    all(q_m, q_terms, lead, q_filter, ngroup, q_hlo, q_hhi, q_hsh, thr0, q_ub, q_wt, q_wn, q_rup, f_shift, f_seg, f_woff,
        f_tab, f_max, ch_f, ch_c, ch_t, ch_s, citems, ditems, scan, phrase, bphrase, group, gphrase, mgroup, field, fphrase, items, q_pterm, q_ppos, q_clause, q_member,
        q_probe, q_tier);
    nf = 0;
  }
};

// Query i of the batch when it holds a phrase clause beside other clauses and
// fg_phrase_clauses is on (the clause table was checked by plan_phrase): facet
// clauses only with `filters` (fg_filter_clauses; the slot's q_filter is set by
// plan_host, `nomatch`: they match no doc of the snapshot, so no work items), a
// snapshot with positions, else FG_EUNSUPPORTED naming the reason.
// A Should or MustNot clause with a term the snapshot lacks is dropped, a Must
// one empties the slot; one Should and no Must is that clause as a Must.  The
// slot's clause table (fg_internal.h cl_pack) is in the order of the score sum:
// the Musts by (cost, clause position) -- a term clause's cost df_text + df_name,
// a phrase clause's the sum over the two fields of its terms' smallest doc count
// there (PhraseScorer's size hint is its intersection's; a field lacking a term:
// 0) --, then the MustNots, then the Shoulds in clause order; without a Must the
// Shoulds, then the MustNots.  q_terms / q_pterm / q_ppos hold the clauses' terms
// in that order, a phrase's anchor (the first occurrence of its term with the
// fewest postings) first; q_wt / q_wn [c] clause c's weights (a phrase's:
// Bm25Weight::for_terms, as plan_phrase's).  Work items (k_bphrase): with a Must,
// groups of the chunks of the shortest list among the Must clauses' first terms;
// without, one pass per Should clause over that clause's first term's list; the
// clause led from rides in the item's count word above kBpPassShift.
// (plan_field_phrase below repeats this function's absence rule, order, rows and item spreading with a field per
// clause: a change here is to be mirrored there by hand.)
int plan_bool_phrase(const fg_index* ix, const fg_query_batch* q, uint32_t i, uint32_t nq_size, uint32_t n_segs,
                     PlanTables& h, bool filters, bool nomatch) {
  const uint32_t b = q->q_off[i], e = q->q_off[i + 1];
  if (!filters && q->f_off && q->f_off[i + 1] > q->f_off[i])
    return fail(FG_EUNSUPPORTED, "query %u: phrase with facet filters", i);
  if (!ix->has_positions) return fail(FG_EUNSUPPORTED, "query %u: snapshot built without positions", i);
  auto len = [&](uint32_t t) { return ix->off[t + 1] - ix->off[t]; };
  struct Cl { uint32_t at, n, oc, pos, anchor; uint64_t cost; float wt, wn; };
  Cl cl[fg::kMaxTerms];
  uint32_t lt[fg::kMaxTerms];  // the query's terms as the snapshot's ids
  uint32_t ncl = 0, nm = 0, ns = 0;
  bool must_missing = false;
  for (uint32_t j = b, pos = 0; j < e; ++pos) {
    const uint32_t n = q->phrase_len[j];
    const uint32_t oc = q->occur ? q->occur[j] : (q->mode == FG_MODE_OR ? FG_OCCUR_SHOULD : FG_OCCUR_MUST);
    if (oc > FG_OCCUR_MUST_NOT) return fail(FG_EINVAL, "query %u: bad occur %u", i, oc);
    if (n >= 2 && q->phrase_pos[j + n - 1] >= (1u << 30)) return fail(FG_EINVAL, "query %u: phrase offset too large", i);
    Cl c{j - b, n, oc, pos, 0, 0, 0.0f, 0.0f};
    bool present = true;
    uint64_t ct = ~0ull, cn = ~0ull;
    float it = 0.0f, in = 0.0f;
    for (uint32_t x = 0; x < n && present; ++x) {
      const uint32_t t = lt[c.at + x] = fgh::local_term(ix, q->terms[j + x]);
      present = t < ix->n_terms && ix->off[t + 1] > ix->off[t];
      if (!present) break;
      ct = std::min<uint64_t>(ct, ix->df_text[t]);
      cn = std::min<uint64_t>(cn, ix->df_name[t]);
      it += ix->idf_text[t];
      in += ix->idf_name[t];
      if (len(t) < len(lt[c.at + c.anchor])) c.anchor = x;
    }
    j += n;
    if (!present) {
      must_missing |= oc == FG_OCCUR_MUST;
      continue;
    }
    if (n == 1) {
      c.cost = (uint64_t)ix->df_text[lt[c.at]] + ix->df_name[lt[c.at]];
      c.wt = ix->w_text[lt[c.at]];
      c.wn = ix->w_name[lt[c.at]];
    } else {
      c.cost = ct + cn;
      c.wt = it * (1.0f + 1.2f);  // (1 + K1), as bm25_weight's
      c.wn = in * (1.0f + 1.2f);
    }
    nm += oc == FG_OCCUR_MUST;
    ns += oc == FG_OCCUR_SHOULD;
    cl[ncl++] = c;
  }
  // a Must matches nothing, no positive clause, or facet clauses that match no doc: no hits
  if (must_missing || nm + ns == 0 || nomatch) return FG_OK;
  if (nm == 0 && ns == 1)
    for (uint32_t c = 0; c < ncl; ++c)
      if (cl[c].oc == FG_OCCUR_SHOULD) { cl[c].oc = FG_OCCUR_MUST; nm = 1; ns = 0; }
  // the order of the score sum
  auto rank = [&](const Cl& c) {
    if (nm) return c.oc == FG_OCCUR_MUST ? 0 : c.oc == FG_OCCUR_MUST_NOT ? 1 : 2;
    return c.oc == FG_OCCUR_SHOULD ? 0 : 1;
  };
  std::stable_sort(cl, cl + ncl, [&](const Cl& x, const Cl& y) {
    const int rx = rank(x), ry = rank(y);
    if (rx != ry) return rx < ry;
    return nm && rx == 0 && x.cost < y.cost;  // (stable: ties and the other kinds by clause position)
  });
  const size_t row = (size_t)i * fg::kMaxTerms;
  uint32_t first[fg::kMaxTerms], o = 0;
  for (uint32_t c = 0; c < ncl; ++c) {
    const Cl& x = cl[c];
    first[c] = o;
    for (uint32_t u = 0, at = 1; u < x.n; ++u) {
      const uint32_t dst = o + (u == x.anchor ? 0 : at++);
      h.q_terms[row + dst] = lt[x.at + u];
      h.q_pterm[row + dst] = q->terms[b + x.at + u];
      h.q_ppos[row + dst] = q->phrase_pos[b + x.at + u];
    }
    h.q_clause[row + c] = fg::cl_pack(o, x.n, x.oc, x.n >= 2, c);
    h.q_wt[row + c] = x.wt;
    h.q_wn[row + c] = x.wn;
    o += x.n;
  }
  h.q_m[i] = fg::qm_phrase(ncl, o);
  // the passes: the Must clause with the shortest first list, or every Should clause
  const uint32_t cdiv = n_segs <= 1 ? 1u : n_segs;
  const uint32_t per_q = std::max<uint32_t>(
      1, std::min<uint32_t>(64, std::max<uint32_t>(fg::kConjGroupsPerQuery, 1024 / std::max(nq_size, 1u))) / cdiv);
  auto lead_len = [&](uint32_t c) { return (uint64_t)len(h.q_terms[row + first[c]]); };
  uint32_t lo = 0, hi = nm ? 1 : ns;
  if (nm)
    for (uint32_t c = 1; c < nm; ++c)
      if (lead_len(c) < lead_len(lo)) lo = c;
  if (nm) hi = lo + 1;
  h.lead[i] = (uint32_t)lead_len(lo);
  uint32_t total = 0;
  for (uint32_t c = lo; c < hi; ++c) {
    const uint32_t nch = (uint32_t)((lead_len(c) + fg::kChunk - 1) / fg::kChunk);
    if (h.bphrase.size() + nch > 0x7FFFFFFFull)
      return fail(FG_EUNSUPPORTED, "batch too large (%zu work items)", h.bphrase.size());
    const uint32_t G = std::min<uint32_t>(fg::kPhraseMaxGroup, std::max<uint32_t>(1, (nch + per_q - 1) / per_q));
    const uint32_t ng = (nch + G - 1) / G;
    for (uint32_t g = 0; g < ng; ++g)
      h.bphrase.push_back(WItem{(g + 0.5) / ng, i, g * G, std::min(G, nch - g * G) | (c << fg::kBpPassShift)});
    total += ng;
  }
  h.ngroup[i] = total;
  return FG_OK;
}

// Query i of the batch when it holds a group clause and fg_group_clauses is on
// (the clause table was checked by plan_phrase; no phrase clause beside it): facet
// clauses only with `filters` (fg_filter_clauses; `nomatch` as plan_bool_phrase's),
// else FG_EUNSUPPORTED.  A member the snapshot lacks is absent: an
// any-of group goes on without it (with none left the group is absent), an all-of
// group is absent as a whole.  An absent Should or MustNot clause is dropped, an
// absent Must empties the slot; one Should and no Must is that clause as a Must.
// A clause's cost: a term's df_text + df_name, an any-of group's the sum of its
// members' costs, an all-of group's the smallest.  The slot's clause table
// (fg_internal.h cl_pack | kClAny / kClAll) is in the order of the score sum, as
// plan_bool_phrase's; the per-member rows q_terms / q_wt / q_wn / q_ub / q_rup
// hold the clauses' members in that order, an all-of group's by (cost, position).
// Work items (k_group), each with its pass (clause, member) in the count word:
//  * a Must that is a term or an all-of group exists: groups of the chunks of
//    the shortest list among those clauses' members;
//  * every Must is an any-of group: a pass per member of the first (cheapest);
//  * no Must: a pass per Should term, per Should all-of group (its shortest
//    member) and per member of every Should any-of group.
int plan_group(const fg_index* ix, const fg_query_batch* q, uint32_t i, uint32_t nq_size, uint32_t n_segs,
               PlanTables& h, bool filters, bool nomatch) {
  const uint32_t b = q->q_off[i], e = q->q_off[i + 1];
  if (!filters && q->f_off && q->f_off[i + 1] > q->f_off[i])
    return fail(FG_EUNSUPPORTED, "query %u: group with facet filters", i);
  auto len = [&](uint32_t t) { return (uint64_t)(ix->off[t + 1] - ix->off[t]); };
  struct Mem { uint32_t t; uint64_t cost; };
  struct Cl { uint32_t at, n, oc, kind; uint64_t cost; };
  Cl cl[fg::kMaxTerms];
  Mem mem[fg::kMaxTerms];  // the kept members, a clause's at [at, at + n) in written order
  uint32_t ncl = 0, nmem = 0, nm = 0, ns = 0;
  bool must_missing = false;
  for (uint32_t j = b; j < e;) {
    const uint32_t raw = q->phrase_len[j], flags = raw & (FG_CLAUSE_ANY | FG_CLAUSE_ALL);
    const uint32_t n = raw & ~(FG_CLAUSE_ANY | FG_CLAUSE_ALL);
    const uint32_t oc = q->occur ? q->occur[j] : (q->mode == FG_MODE_OR ? FG_OCCUR_SHOULD : FG_OCCUR_MUST);
    if (oc > FG_OCCUR_MUST_NOT) return fail(FG_EINVAL, "query %u: bad occur %u", i, oc);
    Cl c{nmem, 0, oc, flags == FG_CLAUSE_ANY ? fg::kClAny : flags == FG_CLAUSE_ALL ? fg::kClAll : 0u, 0};
    bool absent = false;
    for (uint32_t x = 0; x < n; ++x) {
      const uint32_t t = fgh::local_term(ix, q->terms[j + x]);
      if (!(t < ix->n_terms && ix->off[t + 1] > ix->off[t])) {
        absent |= c.kind != fg::kClAny;
        continue;
      }
      mem[nmem + c.n++] = Mem{t, (uint64_t)ix->df_text[t] + ix->df_name[t]};
    }
    j += n;
    if (absent || c.n == 0) {
      must_missing |= oc == FG_OCCUR_MUST;
      continue;
    }
    Mem* m0 = mem + c.at;
    if (c.kind == fg::kClAll) {
      std::stable_sort(m0, m0 + c.n, [](const Mem& x, const Mem& y) { return x.cost < y.cost; });
      c.cost = m0[0].cost;
    } else {
      for (uint32_t x = 0; x < c.n; ++x) c.cost += m0[x].cost;
    }
    nmem += c.n;
    nm += oc == FG_OCCUR_MUST;
    ns += oc == FG_OCCUR_SHOULD;
    cl[ncl++] = c;
  }
  // a Must matches nothing, no positive clause, or facet clauses that match no doc: no hits
  if (must_missing || nm + ns == 0 || nomatch) return FG_OK;
  if (nm == 0 && ns == 1)
    for (uint32_t c = 0; c < ncl; ++c)
      if (cl[c].oc == FG_OCCUR_SHOULD) { cl[c].oc = FG_OCCUR_MUST; nm = 1; ns = 0; }
  // the order of the score sum
  auto rank = [&](const Cl& c) {
    if (nm) return c.oc == FG_OCCUR_MUST ? 0 : c.oc == FG_OCCUR_MUST_NOT ? 1 : 2;
    return c.oc == FG_OCCUR_SHOULD ? 0 : 1;
  };
  std::stable_sort(cl, cl + ncl, [&](const Cl& x, const Cl& y) {
    const int rx = rank(x), ry = rank(y);
    if (rx != ry) return rx < ry;
    return nm && rx == 0 && x.cost < y.cost;  // (stable: ties and the other kinds by clause position)
  });
  const size_t row = (size_t)i * fg::kMaxTerms;
  uint32_t first[fg::kMaxTerms], o = 0;
  for (uint32_t c = 0; c < ncl; ++c) {
    const Cl& x = cl[c];
    first[c] = o;
    for (uint32_t u = 0; u < x.n; ++u) {
      const uint32_t t = mem[x.at + u].t;
      float rdn, rup;
      fgh::term_ratio(ix, t, &rdn, &rup);
      h.q_terms[row + o + u] = t;
      h.q_wt[row + o + u] = ix->w_text[t];
      h.q_wn[row + o + u] = ix->w_name[t];
      h.q_rup[row + o + u] = rup;
      h.q_ub[row + o + u] = fgh::term_max_scaled(ix, t, rup);
    }
    h.q_clause[row + c] = fg::cl_pack(o, x.n, x.oc, false, c) | x.kind;
    o += x.n;
  }
  h.q_m[i] = fg::qm_phrase(ncl, o);
  // the passes (clause, member)
  struct Pass { uint32_t c, m; };
  Pass pass[fg::kMaxTerms];
  uint32_t np = 0;
  auto term_of = [&](uint32_t c, uint32_t m) { return h.q_terms[row + first[c] + m]; };
  auto shortest = [&](uint32_t c) {
    uint32_t m = 0;
    for (uint32_t u = 1; u < cl[c].n; ++u)
      if (len(term_of(c, u)) < len(term_of(c, m))) m = u;
    return m;
  };
  bool driver = false;  // a Must that is a term or an all-of group
  for (uint32_t c = 0; c < nm; ++c) {
    if (cl[c].kind == fg::kClAny) continue;
    const Pass p{c, shortest(c)};
    if (!driver || len(term_of(p.c, p.m)) < len(term_of(pass[0].c, pass[0].m))) pass[0] = p;
    driver = true;
  }
  if (driver) {
    np = 1;
  } else {
    for (uint32_t c = 0; c < (nm ? 1u : ns); ++c) {
      if (cl[c].kind == fg::kClAny)
        for (uint32_t u = 0; u < cl[c].n; ++u) pass[np++] = Pass{c, u};
      else
        pass[np++] = Pass{c, shortest(c)};
    }
  }
  const uint32_t cdiv = n_segs <= 1 ? 1u : n_segs;
  const uint32_t per_q = std::max<uint32_t>(
      1, std::min<uint32_t>(64, std::max<uint32_t>(fg::kConjGroupsPerQuery, 1024 / std::max(nq_size, 1u))) / cdiv);
  h.lead[i] = (uint32_t)len(term_of(pass[0].c, pass[0].m));
  uint32_t total = 0;
  for (uint32_t x = 0; x < np; ++x) {
    const uint32_t nch = (uint32_t)((len(term_of(pass[x].c, pass[x].m)) + fg::kChunk - 1) / fg::kChunk);
    if (h.group.size() + nch > 0x7FFFFFFFull)
      return fail(FG_EUNSUPPORTED, "batch too large (%zu work items)", h.group.size());
    const uint32_t G = std::min<uint32_t>(fg::kPhraseMaxGroup, std::max<uint32_t>(1, (nch + per_q - 1) / per_q));
    const uint32_t ng = (nch + G - 1) / G;
    for (uint32_t g = 0; g < ng; ++g)
      h.group.push_back(WItem{(g + 0.5) / ng, i, g * G,
                              std::min(G, nch - g * G) | (pass[x].c << fg::kGrpClauseShift) |
                                  (pass[x].m << fg::kGrpMemberShift)});
    total += ng;
  }
  h.ngroup[i] = total;
  return FG_OK;
}

// Query i of the batch when it holds a group clause AND a phrase clause and
// fg_group_phrase_clauses is on (the clause table was checked by plan_phrase;
// DESIGN.md §18): never with facet clauses, whatever fg_filter_clauses says, and
// only on a snapshot with positions, else FG_EUNSUPPORTED.  Absence, the costs and
// the order of the score sum are plan_bool_phrase's for a phrase and plan_group's
// for a term or a group.  The slot's rows hold the clauses' terms, clause after
// clause in the clause table's order: a term's or a group member's row as
// plan_group's (q_terms / q_wt / q_wn / q_ub / q_rup); a phrase's rows q_terms /
// q_pterm / q_ppos with its anchor first, its two field weights (q_wt / q_wn) at its
// first row, and q_ub = (text weight, name weight, 0, ...) over its rows -- a field's
// entry 0.0 when some term of the phrase has no posting in that field here --:
// k_group's bound sums a clause's q_ub, which bounds the phrase's score by its weights.
// Work items (k_gphrase), each with its pass (clause, member) in the count word:
//  * a Must that is a term, a phrase or an all-of group exists: one pass, the
//    shortest list among the term, the phrase's anchor and the group's shortest member;
//  * every Must is an any-of group: a pass per member of the first (cheapest);
//  * no Must: a pass per Should term, per Should phrase (its anchor), per Should
//    all-of group (its shortest member) and per member of every Should any-of group.
int plan_group_phrase(const fg_index* ix, const fg_query_batch* q, uint32_t i, uint32_t nq_size, uint32_t n_segs,
                      PlanTables& h, bool nomatch) {
  const uint32_t b = q->q_off[i], e = q->q_off[i + 1];
  if (q->f_off && q->f_off[i + 1] > q->f_off[i])
    return fail(FG_EUNSUPPORTED, "query %u: group and phrase clauses with facet filters", i);
  if (!ix->has_positions) return fail(FG_EUNSUPPORTED, "query %u: snapshot built without positions", i);
  auto len = [&](uint32_t t) { return (uint64_t)(ix->off[t + 1] - ix->off[t]); };
  struct Mem { uint32_t t, vt, pp; uint64_t cost; };  // the snapshot's id, the vocabulary id, the offset in a phrase
  struct Cl { uint32_t at, n, oc, kind, anchor; uint64_t cost; float wt, wn, ubt, ubn; };
  Cl cl[fg::kMaxTerms];
  Mem mem[fg::kMaxTerms];  // the kept members, a clause's at [at, at + n) in written order
  uint32_t ncl = 0, nmem = 0, nm = 0, ns = 0;
  bool must_missing = false;
  for (uint32_t j = b; j < e;) {
    const uint32_t raw = q->phrase_len[j], flags = raw & (FG_CLAUSE_ANY | FG_CLAUSE_ALL);
    const uint32_t n = raw & ~(FG_CLAUSE_ANY | FG_CLAUSE_ALL);
    const uint32_t oc = q->occur ? q->occur[j] : (q->mode == FG_MODE_OR ? FG_OCCUR_SHOULD : FG_OCCUR_MUST);
    if (oc > FG_OCCUR_MUST_NOT) return fail(FG_EINVAL, "query %u: bad occur %u", i, oc);
    const bool phrase = !flags && n >= 2;
    if (phrase && q->phrase_pos[j + n - 1] >= (1u << 30)) return fail(FG_EINVAL, "query %u: phrase offset too large", i);
    Cl c{nmem, 0, oc, flags == FG_CLAUSE_ANY ? fg::kClAny : flags == FG_CLAUSE_ALL ? fg::kClAll : phrase ? fg::kClPhrase : 0u,
         0, 0, 0.0f, 0.0f, 0.0f, 0.0f};
    bool absent = false;
    uint64_t ct = ~0ull, cn = ~0ull;
    float it = 0.0f, in = 0.0f;
    for (uint32_t x = 0; x < n; ++x) {
      const uint32_t t = fgh::local_term(ix, q->terms[j + x]);
      if (!(t < ix->n_terms && ix->off[t + 1] > ix->off[t])) {
        absent |= c.kind != fg::kClAny;
        if (absent) break;
        continue;
      }
      if (phrase) {
        ct = std::min<uint64_t>(ct, ix->df_text[t]);
        cn = std::min<uint64_t>(cn, ix->df_name[t]);
        it += ix->idf_text[t];
        in += ix->idf_name[t];
        if (c.n && len(t) < len(mem[c.at + c.anchor].t)) c.anchor = c.n;
      }
      mem[nmem + c.n++] = Mem{t, q->terms[j + x], q->phrase_pos[j + x], (uint64_t)ix->df_text[t] + ix->df_name[t]};
    }
    j += n;
    if (absent || c.n == 0) {
      must_missing |= oc == FG_OCCUR_MUST;
      continue;
    }
    Mem* m0 = mem + c.at;
    if (phrase) {
      c.cost = ct + cn;
      c.wt = it * (1.0f + 1.2f);  // (1 + K1), as bm25_weight's
      c.wn = in * (1.0f + 1.2f);
      c.ubt = ct ? c.wt : 0.0f;
      c.ubn = cn ? c.wn : 0.0f;
    } else if (c.kind == fg::kClAll) {
      std::stable_sort(m0, m0 + c.n, [](const Mem& x, const Mem& y) { return x.cost < y.cost; });
      c.cost = m0[0].cost;
    } else {
      for (uint32_t x = 0; x < c.n; ++x) c.cost += m0[x].cost;
    }
    nmem += c.n;
    nm += oc == FG_OCCUR_MUST;
    ns += oc == FG_OCCUR_SHOULD;
    cl[ncl++] = c;
  }
  // a Must matches nothing, no positive clause, or facet clauses that match no doc: no hits
  if (must_missing || nm + ns == 0 || nomatch) return FG_OK;
  if (nm == 0 && ns == 1)
    for (uint32_t c = 0; c < ncl; ++c)
      if (cl[c].oc == FG_OCCUR_SHOULD) { cl[c].oc = FG_OCCUR_MUST; nm = 1; ns = 0; }
  // the order of the score sum
  auto rank = [&](const Cl& c) {
    if (nm) return c.oc == FG_OCCUR_MUST ? 0 : c.oc == FG_OCCUR_MUST_NOT ? 1 : 2;
    return c.oc == FG_OCCUR_SHOULD ? 0 : 1;
  };
  std::stable_sort(cl, cl + ncl, [&](const Cl& x, const Cl& y) {
    const int rx = rank(x), ry = rank(y);
    if (rx != ry) return rx < ry;
    return nm && rx == 0 && x.cost < y.cost;  // (stable: ties and the other kinds by clause position)
  });
  const size_t row = (size_t)i * fg::kMaxTerms;
  uint32_t first[fg::kMaxTerms], o = 0;
  for (uint32_t c = 0; c < ncl; ++c) {
    const Cl& x = cl[c];
    first[c] = o;
    for (uint32_t u = 0, at = 1; u < x.n; ++u) {
      const Mem& m = mem[x.at + u];
      if (x.kind == fg::kClPhrase) {
        const uint32_t dst = o + (u == x.anchor ? 0 : at++);
        h.q_terms[row + dst] = m.t;
        h.q_pterm[row + dst] = m.vt;
        h.q_ppos[row + dst] = m.pp;
        continue;
      }
      float rdn, rup;
      fgh::term_ratio(ix, m.t, &rdn, &rup);
      h.q_terms[row + o + u] = m.t;
      h.q_wt[row + o + u] = ix->w_text[m.t];
      h.q_wn[row + o + u] = ix->w_name[m.t];
      h.q_rup[row + o + u] = rup;
      h.q_ub[row + o + u] = fgh::term_max_scaled(ix, m.t, rup);
    }
    if (x.kind == fg::kClPhrase) {
      h.q_wt[row + o] = x.wt;
      h.q_wn[row + o] = x.wn;
      // the bound (a phrase has >= 2 rows): a field's weight, or 0.0 where some term of the phrase has no posting
      // in that field of this snapshot (x.ubt / x.ubn: the phrase cannot match there)
      h.q_ub[row + o] = x.ubt;
      h.q_ub[row + o + 1] = x.ubn;
    }
    h.q_clause[row + c] = fg::cl_pack(o, x.n, x.oc, x.kind == fg::kClPhrase, c) | (x.kind & (fg::kClAny | fg::kClAll));
    o += x.n;
  }
  h.q_m[i] = fg::qm_phrase(ncl, o);
  // the passes (clause, member)
  struct Pass { uint32_t c, m; };
  Pass pass[fg::kMaxTerms];
  uint32_t np = 0;
  auto term_of = [&](uint32_t c, uint32_t m) { return h.q_terms[row + first[c] + m]; };
  auto candidate = [&](uint32_t c) {  // a term, a phrase's anchor (row 0), an all-of group's shortest member
    uint32_t m = 0;
    if (cl[c].kind == fg::kClAll)
      for (uint32_t u = 1; u < cl[c].n; ++u)
        if (len(term_of(c, u)) < len(term_of(c, m))) m = u;
    return m;
  };
  bool driver = false;  // a Must that is a term, a phrase or an all-of group
  for (uint32_t c = 0; c < nm; ++c) {
    if (cl[c].kind == fg::kClAny) continue;
    const Pass p{c, candidate(c)};
    if (!driver || len(term_of(p.c, p.m)) < len(term_of(pass[0].c, pass[0].m))) pass[0] = p;
    driver = true;
  }
  if (driver) {
    np = 1;
  } else {
    for (uint32_t c = 0; c < (nm ? 1u : ns); ++c) {
      if (cl[c].kind == fg::kClAny)
        for (uint32_t u = 0; u < cl[c].n; ++u) pass[np++] = Pass{c, u};
      else
        pass[np++] = Pass{c, candidate(c)};
    }
  }
  const uint32_t cdiv = n_segs <= 1 ? 1u : n_segs;
  const uint32_t per_q = std::max<uint32_t>(
      1, std::min<uint32_t>(64, std::max<uint32_t>(fg::kConjGroupsPerQuery, 1024 / std::max(nq_size, 1u))) / cdiv);
  h.lead[i] = (uint32_t)len(term_of(pass[0].c, pass[0].m));
  uint32_t total = 0;
  for (uint32_t x = 0; x < np; ++x) {
    const uint32_t nch = (uint32_t)((len(term_of(pass[x].c, pass[x].m)) + fg::kChunk - 1) / fg::kChunk);
    if (h.gphrase.size() + nch > 0x7FFFFFFFull)
      return fail(FG_EUNSUPPORTED, "batch too large (%zu work items)", h.gphrase.size());
    const uint32_t G = std::min<uint32_t>(fg::kPhraseMaxGroup, std::max<uint32_t>(1, (nch + per_q - 1) / per_q));
    const uint32_t ng = (nch + G - 1) / G;
    for (uint32_t g = 0; g < ng; ++g)
      h.gphrase.push_back(WItem{(g + 0.5) / ng, i, g * G,
                                std::min(G, nch - g * G) | (pass[x].c << fg::kGrpClauseShift) |
                                    (pass[x].m << fg::kGrpMemberShift)});
    total += ng;
  }
  h.ngroup[i] = total;
  return FG_OK;
}

// Query i of the batch when one of its groups holds a phrase member and
// fg_group_member_phrases is on (the clause table was checked by plan_phrase;
// DESIGN.md §19): never with facet clauses, only on a snapshot with positions, else
// FG_EUNSUPPORTED.  A group's members are the runs of its rows that begin at an
// offset 0: one row is a term, two or more a phrase.  A phrase (a member or a
// clause) with a term the snapshot lacks is absent; an any-of group goes on without
// an absent member (with none left it is absent), an all-of group is absent as a
// whole; the clause rules, the costs and the order of the score sum are
// plan_group_phrase's, a phrase member's cost a phrase clause's, an all-of group's
// members in (cost, position) order.  The slot's rows are plan_group_phrase's with a
// phrase member laid out as a phrase clause (anchor first, q_pterm / q_ppos, the
// field weights at its first row, q_ub = (text weight, name weight, 0, ...)); q_member
// marks, per clause, the rows that begin a member.  Work items (k_mgroup), each with
// its pass (clause, member) in the count word, a member led by its term's list or
// its phrase's anchor's:
//  * a Must that is a term, a phrase or an all-of group exists: one pass, the
//    shortest lead list among them (an all-of group's: its members' shortest);
//  * every Must is an any-of group: a pass per member of the first (cheapest);
//  * no Must: a pass per Should term, per Should phrase, per Should all-of group
//    and per member of every Should any-of group.
int plan_member_group(const fg_index* ix, const fg_query_batch* q, uint32_t i, uint32_t nq_size, uint32_t n_segs,
                      PlanTables& h, bool nomatch) {
  const uint32_t b = q->q_off[i], e = q->q_off[i + 1];
  if (q->f_off && q->f_off[i + 1] > q->f_off[i])
    return fail(FG_EUNSUPPORTED, "query %u: group with phrase members and facet filters", i);
  if (!ix->has_positions) return fail(FG_EUNSUPPORTED, "query %u: snapshot built without positions", i);
  auto len = [&](uint32_t t) { return (uint64_t)(ix->off[t + 1] - ix->off[t]); };
  struct Row { uint32_t t, vt, pp; };  // the snapshot's id, the vocabulary id, the offset in a phrase
  struct Mem { uint32_t at, n, anchor; uint64_t cost; float wt, wn, ubt, ubn; };  // rows [at, at + n)
  struct Cl { uint32_t at, n, oc, kind; uint64_t cost; };                         // members [at, at + n)
  Row rows[fg::kMaxTerms];
  Mem mem[fg::kMaxTerms];
  Cl cl[fg::kMaxTerms];
  uint32_t ncl = 0, nmem = 0, nrow = 0, nm = 0, ns = 0;
  bool must_missing = false;
  for (uint32_t j = b; j < e;) {
    const uint32_t raw = q->phrase_len[j], flags = raw & (FG_CLAUSE_ANY | FG_CLAUSE_ALL);
    const uint32_t n = raw & ~(FG_CLAUSE_ANY | FG_CLAUSE_ALL);
    const uint32_t oc = q->occur ? q->occur[j] : (q->mode == FG_MODE_OR ? FG_OCCUR_SHOULD : FG_OCCUR_MUST);
    if (oc > FG_OCCUR_MUST_NOT) return fail(FG_EINVAL, "query %u: bad occur %u", i, oc);
    if (q->phrase_pos[j + n - 1] >= (1u << 30)) return fail(FG_EINVAL, "query %u: phrase offset too large", i);
    Cl c{nmem, 0, oc, flags == FG_CLAUSE_ANY ? fg::kClAny : flags == FG_CLAUSE_ALL ? fg::kClAll : n >= 2 ? fg::kClPhrase : 0u, 0};
    const uint32_t row0 = nrow;
    bool absent = false;
    for (uint32_t x = 0; x < n;) {
      uint32_t xe = x + 1;  // the member's rows [x, xe): a group's run up to the next offset 0, a phrase clause's all
      while (xe < n && (!flags || q->phrase_pos[j + xe] != 0)) ++xe;
      Mem m{nrow, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f};
      uint64_t ct = ~0ull, cn = ~0ull;
      float it = 0.0f, in = 0.0f;
      bool gone = false;
      for (uint32_t y = x; y < xe && !gone; ++y) {
        const uint32_t t = fgh::local_term(ix, q->terms[j + y]);
        gone = !(t < ix->n_terms && ix->off[t + 1] > ix->off[t]);
        if (gone) break;
        ct = std::min<uint64_t>(ct, ix->df_text[t]);
        cn = std::min<uint64_t>(cn, ix->df_name[t]);
        it += ix->idf_text[t];
        in += ix->idf_name[t];
        if (m.n && len(t) < len(rows[m.at + m.anchor].t)) m.anchor = m.n;
        rows[m.at + m.n++] = Row{t, q->terms[j + y], q->phrase_pos[j + y]};
      }
      if (gone) {
        absent |= c.kind != fg::kClAny;
      } else {
        if (xe - x >= 2) {
          m.cost = ct + cn;
          m.wt = it * (1.0f + 1.2f);  // (1 + K1), as bm25_weight's
          m.wn = in * (1.0f + 1.2f);
          m.ubt = ct ? m.wt : 0.0f;
          m.ubn = cn ? m.wn : 0.0f;
        } else {
          m.cost = (uint64_t)ix->df_text[rows[m.at].t] + ix->df_name[rows[m.at].t];
        }
        nrow += m.n;
        mem[nmem + c.n++] = m;
      }
      x = xe;
    }
    j += n;
    if (absent || c.n == 0) {
      must_missing |= oc == FG_OCCUR_MUST;
      nrow = row0;
      continue;
    }
    Mem* m0 = mem + c.at;
    if (c.kind == fg::kClAll) {
      std::stable_sort(m0, m0 + c.n, [](const Mem& x, const Mem& y) { return x.cost < y.cost; });
      c.cost = m0[0].cost;
    } else {
      for (uint32_t x = 0; x < c.n; ++x) c.cost += m0[x].cost;
    }
    nmem += c.n;
    nm += oc == FG_OCCUR_MUST;
    ns += oc == FG_OCCUR_SHOULD;
    cl[ncl++] = c;
  }
  // a Must matches nothing, no positive clause, or facet clauses that match no doc: no hits
  if (must_missing || nm + ns == 0 || nomatch) return FG_OK;
  if (nm == 0 && ns == 1)
    for (uint32_t c = 0; c < ncl; ++c)
      if (cl[c].oc == FG_OCCUR_SHOULD) { cl[c].oc = FG_OCCUR_MUST; nm = 1; ns = 0; }
  // the order of the score sum
  auto rank = [&](const Cl& c) {
    if (nm) return c.oc == FG_OCCUR_MUST ? 0 : c.oc == FG_OCCUR_MUST_NOT ? 1 : 2;
    return c.oc == FG_OCCUR_SHOULD ? 0 : 1;
  };
  std::stable_sort(cl, cl + ncl, [&](const Cl& x, const Cl& y) {
    const int rx = rank(x), ry = rank(y);
    if (rx != ry) return rx < ry;
    return nm && rx == 0 && x.cost < y.cost;  // (stable: ties and the other kinds by clause position)
  });
  const size_t row = (size_t)i * fg::kMaxTerms;
  uint32_t lead_row[fg::kMaxTerms], first[fg::kMaxTerms], o = 0;  // lead_row: per member (cl.at + u), its first row
  for (uint32_t c = 0; c < ncl; ++c) {
    const Cl& x = cl[c];
    first[c] = o;
    uint32_t mask = 0;
    for (uint32_t u = 0; u < x.n; ++u) {
      const Mem& m = mem[x.at + u];
      lead_row[x.at + u] = o;
      mask |= 1u << (o - first[c]);
      if (m.n >= 2) {
        for (uint32_t y = 0, at = 1; y < m.n; ++y) {
          const uint32_t dst = o + (y == m.anchor ? 0 : at++);
          h.q_terms[row + dst] = rows[m.at + y].t;
          h.q_pterm[row + dst] = rows[m.at + y].vt;
          h.q_ppos[row + dst] = rows[m.at + y].pp;
        }
        h.q_wt[row + o] = m.wt;
        h.q_wn[row + o] = m.wn;
        // the bound: a field's weight, or 0.0 where some term of the phrase has no posting in that field here
        h.q_ub[row + o] = m.ubt;
        h.q_ub[row + o + 1] = m.ubn;
      } else {
        const uint32_t t = rows[m.at].t;
        float rdn, rup;
        fgh::term_ratio(ix, t, &rdn, &rup);
        h.q_terms[row + o] = t;
        h.q_wt[row + o] = ix->w_text[t];
        h.q_wn[row + o] = ix->w_name[t];
        h.q_rup[row + o] = rup;
        h.q_ub[row + o] = fgh::term_max_scaled(ix, t, rup);
      }
      o += m.n;
    }
    h.q_clause[row + c] =
        fg::cl_pack(first[c], o - first[c], x.oc, x.kind == fg::kClPhrase, c) | (x.kind & (fg::kClAny | fg::kClAll));
    h.q_member[row + c] = mask;
  }
  h.q_m[i] = fg::qm_phrase(ncl, o);
  // the passes (clause, member)
  struct Pass { uint32_t c, m; };
  Pass pass[fg::kMaxTerms];
  uint32_t np = 0;
  auto term_of = [&](uint32_t c, uint32_t m) { return h.q_terms[row + lead_row[cl[c].at + m]]; };
  auto candidate = [&](uint32_t c) {  // a term, a phrase's anchor, an all-of group's member with the shortest lead list
    uint32_t m = 0;
    if (cl[c].kind == fg::kClAll)
      for (uint32_t u = 1; u < cl[c].n; ++u)
        if (len(term_of(c, u)) < len(term_of(c, m))) m = u;
    return m;
  };
  bool driver = false;  // a Must that is a term, a phrase or an all-of group
  for (uint32_t c = 0; c < nm; ++c) {
    if (cl[c].kind == fg::kClAny) continue;
    const Pass p{c, candidate(c)};
    if (!driver || len(term_of(p.c, p.m)) < len(term_of(pass[0].c, pass[0].m))) pass[0] = p;
    driver = true;
  }
  if (driver) {
    np = 1;
  } else {
    for (uint32_t c = 0; c < (nm ? 1u : ns); ++c) {
      if (cl[c].kind == fg::kClAny)
        for (uint32_t u = 0; u < cl[c].n; ++u) pass[np++] = Pass{c, u};
      else
        pass[np++] = Pass{c, candidate(c)};
    }
  }
  const uint32_t cdiv = n_segs <= 1 ? 1u : n_segs;
  const uint32_t per_q = std::max<uint32_t>(
      1, std::min<uint32_t>(64, std::max<uint32_t>(fg::kConjGroupsPerQuery, 1024 / std::max(nq_size, 1u))) / cdiv);
  h.lead[i] = (uint32_t)len(term_of(pass[0].c, pass[0].m));
  uint32_t total = 0;
  for (uint32_t x = 0; x < np; ++x) {
    const uint32_t nch = (uint32_t)((len(term_of(pass[x].c, pass[x].m)) + fg::kChunk - 1) / fg::kChunk);
    if (h.mgroup.size() + nch > 0x7FFFFFFFull)
      return fail(FG_EUNSUPPORTED, "batch too large (%zu work items)", h.mgroup.size());
    const uint32_t G = std::min<uint32_t>(fg::kPhraseMaxGroup, std::max<uint32_t>(1, (nch + per_q - 1) / per_q));
    const uint32_t ng = (nch + G - 1) / G;
    for (uint32_t g = 0; g < ng; ++g)
      h.mgroup.push_back(WItem{(g + 0.5) / ng, i, g * G,
                               std::min(G, nch - g * G) | (pass[x].c << fg::kGrpClauseShift) |
                                   (pass[x].m << fg::kGrpMemberShift)});
    total += ng;
  }
  h.ngroup[i] = total;
  return FG_OK;
}

// Query i of the batch when it holds a field-qualified term clause and
// fg_field_clauses is on (the clause table was checked by plan_phrase: every clause
// is one term, some carry FG_CLAUSE_TEXT / FG_CLAUSE_NAME): never
// with facet clauses, whatever fg_filter_clauses says, else FG_EUNSUPPORTED.  A field
// clause is that field's TermQuery: absent in a snapshot that lacks the term in
// that field (df_text / df_name 0, or no name postings at all); absence, the order
// of the score sum and the passes are plan_group's for single-member clauses.  A
// clause's cost: an unqualified term's df_text + df_name, a field clause's the
// field's doc count alone.  The slot's rows (q_terms / q_wt / q_wn / q_ub / q_rup,
// one per clause) are plan_group's: q_ub / q_rup stay the MERGED term's, still upper
// bounds of a one-field score (the other field's part is >= 0 and f32 addition is
// monotone); the clause word carries the field (fg_internal.h kClText / kClName).
// Work items (k_field): with a Must, groups of the chunks of the shortest merged
// list among the Must clauses; without, a pass per Should clause.
int plan_field(const fg_index* ix, const fg_query_batch* q, uint32_t i, uint32_t nq_size, uint32_t n_segs,
               PlanTables& h, bool nomatch) {
  const uint32_t b = q->q_off[i], e = q->q_off[i + 1];
  if (q->f_off && q->f_off[i + 1] > q->f_off[i])
    return fail(FG_EUNSUPPORTED, "query %u: field clause with facet filters", i);
  auto len = [&](uint32_t t) { return (uint64_t)(ix->off[t + 1] - ix->off[t]); };
  struct Cl { uint32_t t, oc, field; uint64_t cost; };
  Cl cl[fg::kMaxTerms];
  uint32_t ncl = 0, nm = 0, ns = 0;
  bool must_missing = false;
  for (uint32_t j = b; j < e; ++j) {
    const uint32_t raw = q->phrase_len[j];
    const uint32_t oc = q->occur ? q->occur[j] : (q->mode == FG_MODE_OR ? FG_OCCUR_SHOULD : FG_OCCUR_MUST);
    if (oc > FG_OCCUR_MUST_NOT) return fail(FG_EINVAL, "query %u: bad occur %u", i, oc);
    Cl c{fgh::local_term(ix, q->terms[j]), oc, raw & FG_CLAUSE_TEXT ? fg::kClText : raw & FG_CLAUSE_NAME ? fg::kClName : 0u, 0};
    bool present = c.t < ix->n_terms && ix->off[c.t + 1] > ix->off[c.t];
    if (present) {
      const uint64_t dt = ix->df_text[c.t], dn = ix->d.tfn_name ? ix->df_name[c.t] : 0;
      c.cost = c.field == fg::kClText ? dt : c.field == fg::kClName ? dn : (uint64_t)ix->df_text[c.t] + ix->df_name[c.t];
      present = !c.field || c.cost > 0;  // a field clause: the term has postings in that field here
    }
    if (!present) {
      must_missing |= oc == FG_OCCUR_MUST;
      continue;
    }
    nm += oc == FG_OCCUR_MUST;
    ns += oc == FG_OCCUR_SHOULD;
    cl[ncl++] = c;
  }
  // a Must matches nothing, no positive clause, or facet clauses that match no doc: no hits
  if (must_missing || nm + ns == 0 || nomatch) return FG_OK;
  if (nm == 0 && ns == 1)
    for (uint32_t c = 0; c < ncl; ++c)
      if (cl[c].oc == FG_OCCUR_SHOULD) { cl[c].oc = FG_OCCUR_MUST; nm = 1; ns = 0; }
  // the order of the score sum
  auto rank = [&](const Cl& c) {
    if (nm) return c.oc == FG_OCCUR_MUST ? 0 : c.oc == FG_OCCUR_MUST_NOT ? 1 : 2;
    return c.oc == FG_OCCUR_SHOULD ? 0 : 1;
  };
  std::stable_sort(cl, cl + ncl, [&](const Cl& x, const Cl& y) {
    const int rx = rank(x), ry = rank(y);
    if (rx != ry) return rx < ry;
    return nm && rx == 0 && x.cost < y.cost;  // (stable: ties and the other kinds by clause position)
  });
  const size_t row = (size_t)i * fg::kMaxTerms;
  for (uint32_t c = 0; c < ncl; ++c) {
    const uint32_t t = cl[c].t;
    float rdn, rup;
    fgh::term_ratio(ix, t, &rdn, &rup);
    h.q_terms[row + c] = t;
    h.q_wt[row + c] = ix->w_text[t];
    h.q_wn[row + c] = ix->w_name[t];
    h.q_rup[row + c] = rup;
    h.q_ub[row + c] = fgh::term_max_scaled(ix, t, rup);
    h.q_clause[row + c] = fg::cl_pack(c, 1, cl[c].oc, false, c) | cl[c].field;
  }
  h.q_m[i] = fg::qm_phrase(ncl, ncl);
  // The slot starts at threshold 0 (h.thr0[i] stays 0) and takes no k-th floor: the
  // snapshot's per-term K-th scores and ladder floors are scores of the MERGED
  // clause, Should(text:t, name:t), not lower bounds of a one-field score; starting
  // from them would drop hits.
  // the passes: the Must clause with the shortest merged list, or every Should clause
  uint32_t lo = 0, hi = nm ? 1 : ns;
  for (uint32_t c = 1; c < nm; ++c)
    if (len(cl[c].t) < len(cl[lo].t)) lo = c;
  if (nm) hi = lo + 1;
  const uint32_t cdiv = n_segs <= 1 ? 1u : n_segs;
  const uint32_t per_q = std::max<uint32_t>(
      1, std::min<uint32_t>(64, std::max<uint32_t>(fg::kConjGroupsPerQuery, 1024 / std::max(nq_size, 1u))) / cdiv);
  h.lead[i] = (uint32_t)len(cl[lo].t);
  uint32_t total = 0;
  for (uint32_t c = lo; c < hi; ++c) {
    const uint32_t nch = (uint32_t)((len(cl[c].t) + fg::kChunk - 1) / fg::kChunk);
    if (h.field.size() + nch > 0x7FFFFFFFull)
      return fail(FG_EUNSUPPORTED, "batch too large (%zu work items)", h.field.size());
    const uint32_t G = std::min<uint32_t>(fg::kPhraseMaxGroup, std::max<uint32_t>(1, (nch + per_q - 1) / per_q));
    const uint32_t ng = (nch + G - 1) / G;
    for (uint32_t g = 0; g < ng; ++g)
      h.field.push_back(WItem{(g + 0.5) / ng, i, g * G, std::min(G, nch - g * G) | (c << fg::kGrpClauseShift)});
    total += ng;
  }
  h.ngroup[i] = total;
  return FG_OK;
}

// Query i of the batch when it holds a field-qualified phrase clause, or a field
// term clause beside a phrase clause, and fg_field_phrases is on top of
// fg_field_clauses (the clause table was checked by plan_phrase: term and phrase
// clauses, some carrying FG_CLAUSE_TEXT / FG_CLAUSE_NAME, no group):
// never with facet clauses, on a snapshot with positions, else FG_EUNSUPPORTED.
// A field clause is that field's TermQuery / PhraseQuery: absent in a snapshot
// where one of its terms has no posting in that field (df_text / df_name 0), and a
// `name` clause also where the snapshot has no name postings or no name forward
// index; absence, the order of the score sum and the passes are plan_bool_phrase's.
// A clause's cost: an unqualified term's df_text + df_name and an unqualified
// phrase's the sum over the fields of its terms' smallest doc count there, as
// plan_bool_phrase's; a field term's the field's doc count (plan_field's); a field
// phrase's the smallest doc count in that field among its terms -- the phrase's
// rule with the other field's summand dropped.  The slot's rows are
// plan_bool_phrase's, the clause word carrying the field (fg_internal.h kClText /
// kClName) beside kClPhrase; a field phrase's first row, its anchor, is the first
// occurrence of its term with the fewest postings in THAT field.  q_wt / q_wn [c]
// hold clause c's weights; a field clause uses its field's.  The slot starts at
// threshold 0 and takes no k-th floor, as plan_field argues.  Work items
// (k_fphrase): with a Must, groups of the chunks of the shortest merged list among
// the Must clauses' first terms; without, a pass per Should clause.
// (The absence rule, the order, the rows and the item spreading repeat plan_bool_phrase's: a change to either
// copy is to be mirrored in the other by hand.)
int plan_field_phrase(const fg_index* ix, const fg_query_batch* q, uint32_t i, uint32_t nq_size, uint32_t n_segs,
                      PlanTables& h, bool nomatch) {
  constexpr uint32_t kFlags = FG_CLAUSE_TEXT | FG_CLAUSE_NAME;
  const uint32_t b = q->q_off[i], e = q->q_off[i + 1];
  if (q->f_off && q->f_off[i + 1] > q->f_off[i])
    return fail(FG_EUNSUPPORTED, "query %u: field clause with facet filters", i);
  if (!ix->has_positions) return fail(FG_EUNSUPPORTED, "query %u: snapshot built without positions", i);
  const bool has_name = ix->d.tfn_name != nullptr && ix->d.fwd_off_name != nullptr;
  auto len = [&](uint32_t t) { return ix->off[t + 1] - ix->off[t]; };
  struct Cl { uint32_t at, n, oc, field, anchor; uint64_t cost; float wt, wn; };
  Cl cl[fg::kMaxTerms];
  uint32_t lt[fg::kMaxTerms];  // the query's terms as the snapshot's ids
  uint32_t ncl = 0, nm = 0, ns = 0;
  bool must_missing = false;
  for (uint32_t j = b; j < e;) {
    const uint32_t raw = q->phrase_len[j], n = raw & ~kFlags;
    const uint32_t oc = q->occur ? q->occur[j] : (q->mode == FG_MODE_OR ? FG_OCCUR_SHOULD : FG_OCCUR_MUST);
    if (oc > FG_OCCUR_MUST_NOT) return fail(FG_EINVAL, "query %u: bad occur %u", i, oc);
    if (n >= 2 && q->phrase_pos[j + n - 1] >= (1u << 30)) return fail(FG_EINVAL, "query %u: phrase offset too large", i);
    Cl c{j - b, n, oc, raw & FG_CLAUSE_TEXT ? fg::kClText : raw & FG_CLAUSE_NAME ? fg::kClName : 0u, 0, 0, 0.0f, 0.0f};
    bool present = c.field != fg::kClName || has_name;
    uint64_t ct = ~0ull, cn = ~0ull, ca = ~0ull;  // smallest doc counts: text, name; the anchor's in the clause's field
    float it = 0.0f, in = 0.0f;
    for (uint32_t x = 0; x < n && present; ++x) {
      const uint32_t t = lt[c.at + x] = fgh::local_term(ix, q->terms[j + x]);
      present = t < ix->n_terms && ix->off[t + 1] > ix->off[t];
      if (!present) break;
      const uint64_t dt = ix->df_text[t], dn = ix->df_name[t];
      // a field clause: every term has postings in that field here
      if ((c.field == fg::kClText && dt == 0) || (c.field == fg::kClName && dn == 0)) { present = false; break; }
      ct = std::min(ct, dt);
      cn = std::min(cn, dn);
      it += ix->idf_text[t];
      in += ix->idf_name[t];
      const uint64_t fewest = c.field == fg::kClText ? dt : c.field == fg::kClName ? dn : (uint64_t)len(t);
      if (fewest < ca) { ca = fewest; c.anchor = x; }
    }
    j += n;
    if (!present) {
      must_missing |= oc == FG_OCCUR_MUST;
      continue;
    }
    c.cost = c.field == fg::kClText ? ct : c.field == fg::kClName ? cn : ct + cn;  // (one term: its own counts)
    if (n == 1) {
      c.wt = ix->w_text[lt[c.at]];
      c.wn = ix->w_name[lt[c.at]];
    } else {
      c.wt = it * (1.0f + 1.2f);  // (1 + K1), as bm25_weight's
      c.wn = in * (1.0f + 1.2f);
    }
    nm += oc == FG_OCCUR_MUST;
    ns += oc == FG_OCCUR_SHOULD;
    cl[ncl++] = c;
  }
  // a Must matches nothing, no positive clause, or facet clauses that match no doc: no hits
  if (must_missing || nm + ns == 0 || nomatch) return FG_OK;
  if (nm == 0 && ns == 1)
    for (uint32_t c = 0; c < ncl; ++c)
      if (cl[c].oc == FG_OCCUR_SHOULD) { cl[c].oc = FG_OCCUR_MUST; nm = 1; ns = 0; }
  // the order of the score sum
  auto rank = [&](const Cl& c) {
    if (nm) return c.oc == FG_OCCUR_MUST ? 0 : c.oc == FG_OCCUR_MUST_NOT ? 1 : 2;
    return c.oc == FG_OCCUR_SHOULD ? 0 : 1;
  };
  std::stable_sort(cl, cl + ncl, [&](const Cl& x, const Cl& y) {
    const int rx = rank(x), ry = rank(y);
    if (rx != ry) return rx < ry;
    return nm && rx == 0 && x.cost < y.cost;  // (stable: ties and the other kinds by clause position)
  });
  const size_t row = (size_t)i * fg::kMaxTerms;
  uint32_t first[fg::kMaxTerms], o = 0;
  for (uint32_t c = 0; c < ncl; ++c) {
    const Cl& x = cl[c];
    first[c] = o;
    for (uint32_t u = 0, at = 1; u < x.n; ++u) {
      const uint32_t dst = o + (u == x.anchor ? 0 : at++);
      h.q_terms[row + dst] = lt[x.at + u];
      h.q_pterm[row + dst] = q->terms[b + x.at + u];
      h.q_ppos[row + dst] = q->phrase_pos[b + x.at + u];
    }
    h.q_clause[row + c] = fg::cl_pack(o, x.n, x.oc, x.n >= 2, c) | x.field;
    h.q_wt[row + c] = x.wt;
    h.q_wn[row + c] = x.wn;
    o += x.n;
  }
  h.q_m[i] = fg::qm_phrase(ncl, o);
  // (h.thr0[i] stays 0: the per-term K-th scores are the merged clause's, plan_field)
  // the passes: the Must clause with the shortest first list, or every Should clause
  const uint32_t cdiv = n_segs <= 1 ? 1u : n_segs;
  const uint32_t per_q = std::max<uint32_t>(
      1, std::min<uint32_t>(64, std::max<uint32_t>(fg::kConjGroupsPerQuery, 1024 / std::max(nq_size, 1u))) / cdiv);
  auto lead_len = [&](uint32_t c) { return (uint64_t)len(h.q_terms[row + first[c]]); };
  uint32_t lo = 0, hi = nm ? 1 : ns;
  if (nm)
    for (uint32_t c = 1; c < nm; ++c)
      if (lead_len(c) < lead_len(lo)) lo = c;
  if (nm) hi = lo + 1;
  h.lead[i] = (uint32_t)lead_len(lo);
  uint32_t total = 0;
  for (uint32_t c = lo; c < hi; ++c) {
    const uint32_t nch = (uint32_t)((lead_len(c) + fg::kChunk - 1) / fg::kChunk);
    if (h.fphrase.size() + nch > 0x7FFFFFFFull)
      return fail(FG_EUNSUPPORTED, "batch too large (%zu work items)", h.fphrase.size());
    const uint32_t G = std::min<uint32_t>(fg::kPhraseMaxGroup, std::max<uint32_t>(1, (nch + per_q - 1) / per_q));
    const uint32_t ng = (nch + G - 1) / G;
    for (uint32_t g = 0; g < ng; ++g)
      h.fphrase.push_back(WItem{(g + 0.5) / ng, i, g * G, std::min(G, nch - g * G) | (c << fg::kBpPassShift)});
    total += ng;
  }
  h.ngroup[i] = total;
  return FG_OK;
}

// Query i of the batch when it holds a phrase clause (fg_query_batch::phrase_len
// >= 2; *phrase = 0 otherwise, after checking the clause table; a group clause,
// fg_group_clauses, goes to plan_group, one beside a phrase clause, with
// fg_group_phrase_clauses `gphrase`, to plan_group_phrase; a group that holds a
// phrase member, with fg_group_member_phrases `members`, to plan_member_group; a query
// with a field-qualified term clause, fg_field_clauses `fields`, to plan_field; one with a field-qualified
// phrase clause, or a field term clause beside a phrase clause, fg_field_phrases `fphrases`, to
// plan_field_phrase): the device
// subset -- the phrase is the query's only clause (`beside`, fg_phrase_clauses:
// other clauses beside it go to plan_bool_phrase), facet clauses only with
// `filters` (fg_filter_clauses; `nomatch`: they match no doc of the snapshot, so
// the slot gets no work items), a snapshot with positions -- or FG_EUNSUPPORTED
// naming the reason.  The slot's rows:
// q_terms the phrase's distinct terms (the snapshot's ids), the lead -- the
// shortest merged list -- first; q_pterm / q_ppos the (vocabulary id, offset)
// list, the anchor (the first occurrence of the term with the fewest postings)
// first; q_wt[0] / q_wn[0] the field weights, Bm25Weight::for_terms: the terms'
// idfs summed in phrase order from 0.0 (a repeated term each time), times
// (1 + K1).  Work items (k_phrase): groups of the lead list's chunks, as k_conj's.
int plan_phrase(const fg_index* ix, const fg_query_batch* q, uint32_t i, uint32_t nq_size, uint32_t n_segs,
                PlanTables& h, int* phrase, bool beside, bool groups, bool filters, bool gphrase, bool members, bool fields,
                bool fphrases, bool nomatch) {
  *phrase = 0;
  const uint32_t b = q->q_off[i], e = q->q_off[i + 1], m = e - b;
  uint32_t n_clauses = 0, n_phr = 0, n_grp = 0, n_fld = 0, n_fphr = 0;  // (n_phr counts the field-qualified phrases too)
  bool has_pm = false;  // a group holds a nonzero offset: a phrase member (fg_group_member_phrases)
  for (uint32_t j = b; j < e;) {
    uint32_t n = q->phrase_len[j];
    // a field clause (fg_field_clauses; off: the flags make n a bad phrase_len, as before): a plain term
    // clause's entry with FG_CLAUSE_TEXT or FG_CLAUSE_NAME on it
    if (fields && (n & (FG_CLAUSE_TEXT | FG_CLAUSE_NAME))) {
      if ((n & (FG_CLAUSE_TEXT | FG_CLAUSE_NAME)) == (FG_CLAUSE_TEXT | FG_CLAUSE_NAME))
        return fail(FG_EINVAL, "query %u: bad phrase_len at term %u", i, j - b);
      if (n & (FG_CLAUSE_ANY | FG_CLAUSE_ALL)) return fail(FG_EUNSUPPORTED, "query %u: field-qualified group", i);
      const uint32_t cnt = n & ~(FG_CLAUSE_TEXT | FG_CLAUSE_NAME);
      if (cnt != 1) {
        if (!fphrases) return fail(FG_EUNSUPPORTED, "query %u: field-qualified phrase", i);
        // a field-qualified phrase clause (fg_field_phrases): flag | n on a phrase clause's first entry, the
        // other entries and the offsets as an unqualified phrase's
        if (cnt == 0 || cnt > e - j) return fail(FG_EINVAL, "query %u: bad phrase_len at term %u", i, j - b);
        for (uint32_t x = 1; x < cnt; ++x)
          if (q->phrase_len[j + x] != 0) return fail(FG_EINVAL, "query %u: phrase_len inside a phrase must be 0", i);
        if (q->phrase_pos[j] != 0) return fail(FG_EINVAL, "query %u: a phrase's first offset must be 0", i);
        for (uint32_t x = 1; x < cnt; ++x)
          if (q->phrase_pos[j + x] <= q->phrase_pos[j + x - 1])
            return fail(FG_EINVAL, "query %u: phrase offsets must increase", i);
        ++n_fphr;
        ++n_phr;
        ++n_clauses;
        j += cnt;
        continue;
      }
      ++n_fld;
      ++n_clauses;
      ++j;
      continue;
    }
    // a group clause (fg_group_clauses; off: the flags make n a bad phrase_len, as before)
    const uint32_t kind = groups ? n & (FG_CLAUSE_ANY | FG_CLAUSE_ALL) : 0u;
    if (kind) {
      n &= ~(FG_CLAUSE_ANY | FG_CLAUSE_ALL);
      if (kind == (FG_CLAUSE_ANY | FG_CLAUSE_ALL) || n < 2 || n > e - j)
        return fail(FG_EINVAL, "query %u: bad phrase_len at term %u", i, j - b);
      for (uint32_t x = 0; x < n; ++x) {
        if (x && fields && (q->phrase_len[j + x] & (FG_CLAUSE_TEXT | FG_CLAUSE_NAME)))
          return fail(FG_EUNSUPPORTED, "query %u: field-qualified group", i);
        if (x && q->phrase_len[j + x] != 0) return fail(FG_EINVAL, "query %u: phrase_len inside a group must be 0", i);
        const uint32_t pp = q->phrase_pos[j + x];
        if (!members || x == 0) {
          if (pp != 0) return fail(FG_EINVAL, "query %u: a group member's offset must be 0", i);
          continue;
        }
        // fg_group_member_phrases: an offset > 0 continues the member before it as the next term of a phrase
        if (pp == 0) continue;
        if (pp <= q->phrase_pos[j + x - 1]) return fail(FG_EINVAL, "query %u: phrase offsets must increase", i);
        if (pp >= (1u << 30)) return fail(FG_EINVAL, "query %u: phrase offset too large", i);
        has_pm = true;
      }
      if (members) {
        uint32_t nmem = 0;
        for (uint32_t x = 0; x < n; ++x) nmem += q->phrase_pos[j + x] == 0;
        if (nmem < 2) return fail(FG_EINVAL, "query %u: a group needs two members", i);
      }
      ++n_grp;
      ++n_clauses;
      j += n;
      continue;
    }
    if (n == 0 || n > e - j) return fail(FG_EINVAL, "query %u: bad phrase_len at term %u", i, j - b);
    for (uint32_t x = 1; x < n; ++x)
      if (q->phrase_len[j + x] != 0) return fail(FG_EINVAL, "query %u: phrase_len inside a phrase must be 0", i);
    if (n >= 2) {
      if (q->phrase_pos[j] != 0) return fail(FG_EINVAL, "query %u: a phrase's first offset must be 0", i);
      for (uint32_t x = 1; x < n; ++x)
        if (q->phrase_pos[j + x] <= q->phrase_pos[j + x - 1])
          return fail(FG_EINVAL, "query %u: phrase offsets must increase", i);
      ++n_phr;
    }
    ++n_clauses;
    j += n;
  }
  if (n_fld || n_fphr) {  // (whatever the other switches say)
    *phrase = 1;
    if (n_phr && !fphrases) return fail(FG_EUNSUPPORTED, "query %u: field clause beside a phrase clause", i);
    if (n_grp && n_fld) return fail(FG_EUNSUPPORTED, "query %u: field clause beside a group clause", i);
    if (n_grp) return fail(FG_EUNSUPPORTED, "query %u: field-qualified phrase beside a group clause", i);
    if (n_phr) return plan_field_phrase(ix, q, i, nq_size, n_segs, h, nomatch);  // fg_field_phrases
    return plan_field(ix, q, i, nq_size, n_segs, h, nomatch);
  }
  if (n_grp) {
    *phrase = 1;
    if (has_pm) return plan_member_group(ix, q, i, nq_size, n_segs, h, nomatch);
    if (n_phr && gphrase) return plan_group_phrase(ix, q, i, nq_size, n_segs, h, nomatch);
    if (n_phr) return fail(FG_EUNSUPPORTED, "query %u: group clause beside a phrase clause", i);
    return plan_group(ix, q, i, nq_size, n_segs, h, filters, nomatch);
  }
  if (!n_phr) return FG_OK;
  *phrase = 1;
  if (n_clauses > 1) {
    if (!beside) return fail(FG_EUNSUPPORTED, "query %u: phrase clause beside other clauses", i);
    return plan_bool_phrase(ix, q, i, nq_size, n_segs, h, filters, nomatch);
  }
  if (!filters && q->f_off && q->f_off[i + 1] > q->f_off[i])
    return fail(FG_EUNSUPPORTED, "query %u: phrase with facet filters", i);
  if (!ix->has_positions) return fail(FG_EUNSUPPORTED, "query %u: snapshot built without positions", i);
  if (q->phrase_pos[e - 1] >= (1u << 30)) return fail(FG_EINVAL, "query %u: phrase offset too large", i);
  const uint8_t oc = q->occur ? q->occur[b] : (q->mode == FG_MODE_OR ? FG_OCCUR_SHOULD : FG_OCCUR_MUST);
  if (oc > FG_OCCUR_MUST_NOT) return fail(FG_EINVAL, "query %u: bad occur %u", i, (unsigned)oc);
  if (oc == FG_OCCUR_MUST_NOT || nomatch) return FG_OK;  // no positive clause, or facet clauses that match no doc: no hits
  // the terms in this snapshot; one it lacks: no hits here
  uint32_t lt[fg::kMaxTerms], dist[fg::kMaxTerms], nd = 0;
  float it = 0.0f, in = 0.0f;
  for (uint32_t j = 0; j < m; ++j) {
    const uint32_t t = lt[j] = fgh::local_term(ix, q->terms[b + j]);
    if (!(t < ix->n_terms && ix->off[t + 1] > ix->off[t])) return FG_OK;
    it += ix->idf_text[t];
    in += ix->idf_name[t];
    if (std::find(dist, dist + nd, t) == dist + nd) dist[nd++] = t;
  }
  auto len = [&](uint32_t t) { return ix->off[t + 1] - ix->off[t]; };
  const uint32_t lead = *std::min_element(dist, dist + nd, [&](uint32_t x, uint32_t y) { return len(x) < len(y); });
  const size_t row = (size_t)i * fg::kMaxTerms;
  uint32_t* qt = h.q_terms.data() + row;
  qt[0] = lead;
  for (uint32_t j = 0, o = 1; j < nd; ++j)
    if (dist[j] != lead) qt[o++] = dist[j];
  const uint32_t anchor = (uint32_t)(std::find(lt, lt + m, lead) - lt);
  for (uint32_t j = 0, o = 1; j < m; ++j) {
    const uint32_t at = j == anchor ? 0 : o++;
    h.q_pterm[row + at] = q->terms[b + j];
    h.q_ppos[row + at] = q->phrase_pos[b + j];
  }
  h.q_m[i] = fg::qm_phrase(nd, m);
  h.q_wt[row] = it * (1.0f + 1.2f);  // (1 + K1), as bm25_weight's
  h.q_wn[row] = in * (1.0f + 1.2f);
  const uint64_t df0 = len(lead);
  h.lead[i] = (uint32_t)df0;
  const uint32_t nch = (uint32_t)((df0 + fg::kChunk - 1) / fg::kChunk);
  if (h.phrase.size() + nch > 0x7FFFFFFFull) return fail(FG_EUNSUPPORTED, "batch too large (%zu work items)", h.phrase.size());
  const uint32_t cdiv = n_segs <= 1 ? 1u : n_segs;
  const uint32_t per_q = std::max<uint32_t>(
      1, std::min<uint32_t>(64, std::max<uint32_t>(fg::kConjGroupsPerQuery, 1024 / std::max(nq_size, 1u))) / cdiv);
  const uint32_t G = std::min<uint32_t>(fg::kPhraseMaxGroup, std::max<uint32_t>(1, (nch + per_q - 1) / per_q));
  const uint32_t ng = (nch + G - 1) / G;
  h.ngroup[i] = ng;
  for (uint32_t g = 0; g < ng; ++g) h.phrase.push_back(WItem{(g + 0.5) / ng, i, g * G, std::min(G, nch - g * G)});
  return FG_OK;
}

// n_segs: the snapshots the plan spans; a query's work items are spread over
// all of them, so each snapshot gets its share of the per-query item counts.
// nq_size: the batch size the item counts are sized for (q may be a slice of
// that batch: plan_pieces plans a snapshot's queries in pieces)
// qtime: the plan forms its scores at query time (some snapshot's statistics
// changed since its build: DevPlan::feat), so the descriptors point at payloads
// beside, groups, filters, gphrase, members, fields: fg_phrase_clauses, fg_group_clauses, fg_filter_clauses,
// fg_group_phrase_clauses, fg_group_member_phrases, fg_field_clauses as the plan's creation read them;
// fphrases: fg_field_phrases, with fields
int plan_host(const fg_index* ix, const fg_query_batch* q, uint32_t k, uint32_t n_segs, PlanTables& h,
              uint32_t nq_size, bool qtime, bool beside, bool groups, bool filters, bool gphrase, bool members,
              bool fields, bool fphrases) {
  if (!ix || !q || (q->n_queries && !q->q_off)) return fail(FG_EINVAL, "bad arguments");
  if (q->n_queries && q->q_off[q->n_queries] > q->q_off[0] && !q->terms) return fail(FG_EINVAL, "q_off without terms");
  if (q->f_off && q->n_queries && q->f_off[q->n_queries] > q->f_off[0] && !q->f_terms)
    return fail(FG_EINVAL, "f_off without f_terms");
  if (k < 1) return fail(FG_EINVAL, "k must be >= 1 (TopDocs::with_limit asserts limit >= 1)");
  if (k > FG_MAX_K) return fail(FG_EUNSUPPORTED, "k=%u > FG_MAX_K=%d", k, FG_MAX_K);
  if (q->mode != FG_MODE_AND && q->mode != FG_MODE_OR) return fail(FG_EINVAL, "bad mode %d", q->mode);
  const uint32_t nq = q->n_queries;
  const uint64_t N = ix->n_docs;
  const bool disj = q->mode == FG_MODE_OR;
  const uint32_t tab_lead = fgh::doctab_lead(), tab8_lead = fgh::doctab8_lead();
  const bool tiers = !qtime && !ix->band_map.empty() && fgh::band_lead();
  const float tier_ratio = fgh::band_ub_ratio();
  h.clear();
  const size_t nqt = (size_t)nq * fg::kMaxTerms;
  for (auto* v : {&h.q_m, &h.lead, &h.q_tier}) v->assign(nq, 0);
  h.q_terms.assign(nqt, 0);
  h.thr0.assign(nq, 0);
  for (auto* v : {&h.q_ub, &h.q_wt, &h.q_wn}) v->assign(nqt, 0.0f);
  h.q_rup.assign(nqt, 1.0f);
  h.q_probe.assign(nqt, fg::ProbeDesc{});
  if (q->phrase_len) {
    if (!q->phrase_pos) return fail(FG_EINVAL, "phrase_len without phrase_pos");
    h.q_pterm.assign(nqt, 0);
    h.q_ppos.assign(nqt, 0);
    if (beside || groups || fields) h.q_clause.assign(nqt, 0);
    if (groups && members) h.q_member.assign(nqt, 0);
  }

  // ---- facet filters: one mask per distinct clause list (fg_internal.h DevFilters)
  h.q_filter.assign(nq, 0xFFFFFFFFu);
  std::vector<std::vector<uint32_t>> flist;
  std::vector<uint8_t> q_nomatch(nq, 0);  // the filter matches no doc: no work items
  if (q->f_off) {
    std::map<std::vector<uint32_t>, uint32_t> fid;
    for (uint32_t i = 0; i < nq; ++i) {
      const uint32_t b = q->f_off[i], e = q->f_off[i + 1];
      if (e < b) return fail(FG_EINVAL, "f_off not monotone at query %u", i);
      if (e == b) continue;
      if (e - b > fg::kMaxFacetClauses)
        return fail(FG_EUNSUPPORTED, "query %u has %u facet clauses (> %u)", i, e - b, fg::kMaxFacetClauses);
      std::vector<uint32_t> c(q->f_terms + b, q->f_terms + e);
      bool any = false;
      for (uint32_t t : c) any |= t < ix->n_fterms && ix->df_facet[t] > 0;
      if (!any) { q_nomatch[i] = 1; continue; }
      auto it = fid.find(c);
      if (it == fid.end()) {
        it = fid.emplace(c, (uint32_t)flist.size()).first;
        flist.push_back(std::move(c));
      }
      h.q_filter[i] = it->second;
    }
  }
  const uint32_t nf = h.nf = (uint32_t)flist.size();
  h.f_shift.assign(nf, 0);
  h.f_woff.assign(nf + 1, 0);
  h.f_tab.assign((size_t)nf * 256, 0.0f);
  h.f_max.assign(nf, 0.0f);
  std::vector<uint32_t> f_lo(nf, 0xFFFFFFFFu), f_hi(nf, 0);  // doc span of the filter's postings
  for (uint32_t f = 0; f < nf; ++f) {
    const std::vector<uint32_t>& c = flist[f];
    const uint32_t n = (uint32_t)c.size();
    const uint32_t sh = n <= 1 ? 0 : n <= 2 ? 1 : n <= 4 ? 2 : 3;
    if ((N << sh) > (1ull << 32)) return fail(FG_EUNSUPPORTED, "facet mask of %u clauses too large for %llu docs", n,
                                              (unsigned long long)N);
    h.f_shift[f] = sh;
    h.f_woff[f + 1] = h.f_woff[f] + ((((N << sh) + 31) / 32 + 63) & ~63ull);  // 256-B aligned masks
    // union score of each set of matching clauses: 0.0 + s_i in clause order (SumCombiner)
    for (uint32_t v = 0; v < (1u << n); ++v) {
      float sc = 0.0f;
      for (uint32_t i = 0; i < n; ++i)
        if ((v >> i) & 1u) sc += c[i] < ix->n_fterms ? ix->fscore[c[i]] : 0.0f;
      h.f_tab[(size_t)f * 256 + v] = sc;
      h.f_max[f] = std::max(h.f_max[f], sc);
    }
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t t = c[i];
      if (t >= ix->n_fterms || ix->df_facet[t] == 0) continue;
      f_lo[f] = std::min(f_lo[f], ix->ffirst[t]);
      f_hi[f] = std::max(f_hi[f], ix->flast[t]);
      const uint64_t df = ix->foff[t + 1] - ix->foff[t];
      for (uint64_t st = 0; st < df; st += fg::kFmaskChunk) {
        h.ch_f.push_back(f);
        h.ch_c.push_back(i);
        h.ch_t.push_back(t);
        h.ch_s.push_back((uint32_t)st);
      }
    }
  }

  // work items: each query's chunks (Must-driven: k_conj) or doc tiles (Should
  // only: k_disj) in ~kGroupsPerQuery groups, ordered as a doc sweep across the
  // batch (a group centred at doc fraction x runs with the other queries'
  // groups near x), ties by query.  Queries without text terms (facet-only /
  // AllQuery) scan doc tiles (k_scan).  Per-term occurs (q->occur) make a
  // query Must-driven when it has a Must clause (RequiredOptionalScorer over
  // its Shoulds), a union of its Shoulds otherwise; MustNot clauses exclude.
  // k_disj / k_scan groups per query, spread over the plan's snapshots; a small
  // batch (the batch-of-one latency: the GPU holds nothing else) splits each
  // query over up to 16x more, shorter items that run side by side
  const uint32_t gpq_batch =
      fg::kGroupsPerQuery * std::min<uint32_t>(fg::kDisjSmallSpread, std::max<uint32_t>(1, 256 / std::max(nq_size, 1u)));
  const uint32_t gpq = std::max<uint32_t>(1, gpq_batch / n_segs);
  // k_conj items per query per snapshot of a multi-snapshot plan: the single-
  // snapshot count / n_segs, so a query keeps ~the single-snapshot item count
  // over all its slots (C4, 8 x 1.25M namespaces: k_conj 1.300 -> 1.085 ms, /16
  // 1.065 ms, identical hits: profiles/r05/ab/c4_ab_r05q.json; round 4 measured
  // the opposite before the sparse rank words and the XCD split);
  const uint32_t conj_gpq = fg::kConjGroupsPerQuery, conj_maxg = fg::kMaxGroup;
  const uint32_t cdiv = n_segs <= 1 ? 1u : n_segs;
  h.ngroup.assign(nq, 0);
  for (auto* v : {&h.q_hlo, &h.q_hhi}) v->assign(nq, 0x3F800000u);
  h.q_hsh.assign(nq, 31);
  auto present = [&](uint32_t t) { return t < ix->n_terms && ix->off[t + 1] > ix->off[t]; };
  // a clause's query-time weights and bound factor (DevPlan::q_wt / q_wn / q_rup),
  // and its largest current score into cm[j] (the ratio computed once per clause)
  float cm[fg::kMaxTerms];
  auto set_clause = [&](uint32_t i, uint32_t j, uint32_t t) {
    const size_t x = (size_t)i * fg::kMaxTerms + j;
    h.q_wt[x] = ix->w_text[t];
    h.q_wn[x] = ix->w_name[t];
    float rdn, rup;
    fgh::term_ratio(ix, t, &rdn, &rup);
    h.q_rup[x] = rup;
    cm[j] = fgh::term_max_scaled(ix, t, rup);
  };
  // histogram bins of query i: bin 0 at the starting threshold (or ub / div), the
  // top bin at the query's largest possible score ub; ~kQBins bins between
  const float conj_lo_div = fgh::hist_lo_div();  // (Must-driven queries: FUGU_HIST_LO_DIV)
  auto set_bins = [&](uint32_t i, float ub, float div = 256.0f) {
    const float lo = h.thr0[i] ? fg::key_score(h.thr0[i]) : ub / div;
    uint32_t lb, hb;
    std::memcpy(&lb, &lo, 4);
    std::memcpy(&hb, &ub, 4);
    const fgh::Bins b = fgh::union_bins(std::max<uint32_t>(lb, 1), hb);
    h.q_hlo[i] = b.lo;
    h.q_hhi[i] = b.hi;
    h.q_hsh[i] = b.shift;
  };
  for (uint32_t i = 0; i < nq; ++i) {
    const uint32_t b = q->q_off[i], e = q->q_off[i + 1];
    if (e < b) return fail(FG_EINVAL, "q_off not monotone at query %u", i);
    const uint32_t m = e - b;
    if (m > fg::kMaxTerms) return fail(FG_EUNSUPPORTED, "query %u has %u terms (> %u)", i, m, fg::kMaxTerms);
    if (q->phrase_len) {
      int phrase = 0;
      if (int rc = plan_phrase(ix, q, i, nq_size, n_segs, h, &phrase, beside, groups, filters, gphrase, members, fields,
                               fphrases, q_nomatch[i] != 0))
        return rc;
      if (phrase) continue;
    }
    if (q_nomatch[i]) continue;  // the facet clauses match nothing: no hits
    const uint32_t flt = h.q_filter[i];
    const float fmx = flt == 0xFFFFFFFFu ? 0.0f : h.f_max[flt];
    if (m == 0) {
      // empty text query: the facet union alone, or AllQuery (src/db/search.rs:115-116, 131-137)
      h.q_m[i] = 0;
      const uint64_t dlo = flt == 0xFFFFFFFFu ? 0 : f_lo[flt], dhi = flt == 0xFFFFFFFFu ? N - 1 : f_hi[flt];
      const uint32_t tlo = (uint32_t)(dlo >> fg::kDisjTileShift), thi = (uint32_t)(dhi >> fg::kDisjTileShift);
      const uint32_t nt = thi - tlo + 1;
      const uint32_t G = std::min<uint32_t>(fg::kScanMaxGroup,
                                            std::max<uint32_t>(1, (nt + gpq - 1) / gpq));
      const uint32_t ng = (nt + G - 1) / G;
      h.ngroup[i] = ng;
      // the groups of all queries in doc order: the first groups publish the
      // thresholds that let the later ones stop early
      for (uint32_t g = 0; g < ng; ++g) h.scan.push_back(WItem{(double)g, i, tlo + g * G, std::min(G, nt - g * G)});
      continue;
    }
    // the query's clauses by occur; a Should or MustNot clause on a term the
    // snapshot lacks matches nothing and is dropped; a missing Must empties it
    uint32_t tm[fg::kMaxTerms], ts_[fg::kMaxTerms], tx[fg::kMaxTerms];
    uint32_t nm = 0, ns = 0, nx = 0;
    bool must_missing = false;
    for (uint32_t j = 0; j < m; ++j) {
      const uint32_t t = fgh::local_term(ix, q->terms[b + j]);  // (the snapshot's own ids from here on)
      const uint8_t oc = q->occur ? q->occur[b + j] : (disj ? FG_OCCUR_SHOULD : FG_OCCUR_MUST);
      if (oc > FG_OCCUR_MUST_NOT) return fail(FG_EINVAL, "query %u: bad occur %u", i, (unsigned)oc);
      if (oc == FG_OCCUR_MUST) {
        tm[nm++] = t;
        must_missing |= !present(t);
      } else if (present(t)) {
        (oc == FG_OCCUR_SHOULD ? ts_[ns++] : tx[nx++]) = t;
      }
    }
    // one positive clause: the union of one Should IS that clause, so it runs
    // Must-driven (k_conj's single-list and exclusion paths); same docs, same score
    if (nm == 0 && ns == 1) {
      tm[nm++] = ts_[0];
      ns = 0;
    }
    uint32_t* qt = h.q_terms.data() + (size_t)i * fg::kMaxTerms;
    if (nm == 0) {
      if (ns == 0) continue;  // no positive clause: EmptyScorer, no hits
      // Should clauses in clause order (SumCombiner order), then the MustNots
      uint32_t dlo = 0xFFFFFFFFu, dhi = 0;
      for (uint32_t j = 0; j < ns; ++j) {
        qt[j] = ts_[j];
        dlo = std::min(dlo, ix->first_doc[ts_[j]]);
        dhi = std::max(dhi, ix->last_doc[ts_[j]]);
      }
      for (uint32_t j = 0; j < nx; ++j) qt[ns + j] = tx[j];
      for (uint32_t j = 0; j < ns + nx; ++j) set_clause(i, j, qt[j]);
      h.q_m[i] = fg::qm_pack(ns + nx, 0, nx);
      if (flt != 0xFFFFFFFFu) {
        dlo = std::max(dlo, f_lo[flt]);
        dhi = std::min(dhi, f_hi[flt]);
        if (dlo > dhi) continue;  // the text and facet doc spans do not meet
      }
      // starting threshold: the best per-clause K'-th score for the smallest stored
      // K' >= k (unfiltered and unexcluded only: a filter or an exclusion may
      // remove a term's best docs)
      if (flt == 0xFFFFFFFFu && nx == 0) {
        float v = 0.0f;
        for (uint32_t c = 0; c < ns; ++c) v = std::max(v, fgh::term_kth_now(ix, qt[c], k, true));
        if (v > 0.0f) h.thr0[i] = fg::make_key(v, 0xFFFFFFFFu);  // lowest key with score v
      }
      float ub = fmx;
      for (uint32_t c = 0; c < ns; ++c) ub += cm[c];
      set_bins(i, ub);

      const uint32_t tlo = dlo >> fg::kDisjTileShift, thi = dhi >> fg::kDisjTileShift;
      const uint32_t nt = thi - tlo + 1;
      // tiles per item: ~gpq items per query (capping an item's postings, or the
      // items of heavy queries first, measured slower: ab_disj_itemcap_k*.log,
      // ab_disj_heavy_k*.log)
      const uint32_t G = std::min<uint32_t>(std::min(fg::kDisjMaxGroup, fg::kDisjMaxPairs / ns),
                                            std::max<uint32_t>(1, (nt + gpq - 1) / gpq));
      // (shorter first items -- G >> r, G >> (r-1), ... tiles -- so the items that
      // start with no threshold publish one early: r = 2 / 3 / 5 / 8 slower at
      // k = 1000 and 20, +0.4% to +7%: profiles/r05/ab/disj_ramp_r05t.log)
      // (shorter items at the end of each query's range -- half-size in its last
      // 1/8, 1/4, 1/2 -- measured +8.6 / +18 / +34% at top-20, +9 / +18 / +33% at
      // top-1000; 64-tile items -0.5% / +1.8%: profiles/r06/ab/)
      const uint32_t ng = (nt + G - 1) / G;
      for (uint32_t g = 0; g < ng; ++g) {
        const uint32_t t0 = tlo + g * G, n = std::min(G, nt - g * G);
        const double mid = ((double)t0 + 0.5 * n) * (double)(1u << fg::kDisjTileShift) / (double)ix->n_docs;
        h.ditems.push_back(WItem{mid, i, t0, n});
      }
      h.ngroup[i] = ng;
      if (h.ditems.size() > 0x7FFFFFFFull)
        return fail(FG_EUNSUPPORTED, "batch too large (%zu work items)", h.ditems.size());
      continue;
    }
    if (must_missing) continue;  // a Must clause matches nothing: no hits
    // tantivy intersect_scorers: the Must children sorted by cost (union cost =
    // df_text + df_name), stable; then the MustNots, then the Shoulds in clause order
    struct T { uint64_t cost; uint32_t pos, term; };
    T tc[fg::kMaxTerms];
    for (uint32_t j = 0; j < nm; ++j) tc[j] = T{(uint64_t)ix->df_text[tm[j]] + ix->df_name[tm[j]], j, tm[j]};
    std::stable_sort(tc, tc + nm, [](const T& x, const T& y) { return x.cost < y.cost; });
    for (uint32_t j = 0; j < nm; ++j) qt[j] = tc[j].term;
    for (uint32_t j = 0; j < nx; ++j) qt[nm + j] = tx[j];
    for (uint32_t j = 0; j < ns; ++j) qt[nm + nx + j] = ts_[j];
    const uint32_t mt = nm + nx + ns;
    for (uint32_t j = 0; j < mt; ++j) set_clause(i, j, qt[j]);
    h.q_m[i] = fg::qm_pack(mt, nm, nx);
    // MaxScore suffix bounds of the probed lists (k_conj prunes a candidate once its
    // partial score plus these cannot reach the query's threshold): the Must and
    // Should maxima from position j on (MustNots add nothing)
    {
      float acc = 0.0f;
      for (uint32_t j = mt; j-- > 1;) {
        if (j < nm || j >= nm + nx) acc += cm[j];
        h.q_ub[(size_t)i * fg::kMaxTerms + j] = acc;
      }
      // the clauses' probe descriptors: the lead list's, then each probed list's
      // with the bound applied after it
      const size_t row = (size_t)i * fg::kMaxTerms;
      const uint64_t lead_df = ix->off[qt[0] + 1] - ix->off[qt[0]];
      for (uint32_t j = 0; j < mt; ++j) {
        const uint32_t t = qt[j];
        const uint32_t tab = j && !qtime && !ix->dtab_map.empty() ? fgh::doctab_slot(*ix, t) : 0u;
        const fg::ProbeTerm pt{ix->off[t], ix->off[t + 1], ix->tmeta[t], ix->dir_off[t], tab};
        h.q_probe[row + j] =
            fg::probe_desc(ix->d, pt, j == 0, qtime, j + 1 < mt ? h.q_ub[row + j + 1] : 0.0f, lead_df, tab_lead);
      }
      // the first probed list's one-byte bound table, for a query that takes
      // k_conj's deferred path (>= 3 unfiltered Must lists and nothing else)
      if (!qtime && !ix->dtab8_map.empty() && mt >= 3 && nm == mt && flt == 0xFFFFFFFFu)
        fg::probe_desc_bound(ix->d, h.q_probe[row], h.q_probe[row + 1], fgh::doctab8_slot(*ix, qt[1]), ix->tmaxs[qt[1]],
                             true, qtime, ix->off[qt[1] + 1] - ix->off[qt[1]], lead_df, tab8_lead);
      // a query of >= 2 lists on build-time scores leads from its lead term's score-tiered
      // copy when the term has one: the same postings tier-major, so the sweep runs the
      // query's best tier first and k_conj skips the chunks the first bound would empty
      if (tiers && mt >= 2 && (tier_ratio == 0.0f || h.q_ub[row + 1] <= tier_ratio * cm[0]))
        if (const uint32_t b = fgh::band_slot(*ix, qt[0])) {
          fg::probe_desc_tier(ix->d, h.q_probe[row], ix->band_off[b - 1]);
          h.q_tier[i] = 1u + ix->band_c0[b - 1];
        }
    }
    // one list: its K'-th best alive score (the smallest stored K' >= k) bounds
    // the query's k-th best from below, so k_conj starts from that threshold and
    // skips the lead chunks whose block-max cannot reach it (the block-max
    // pruning tantivy's TopDocs runs on a single TermScorer: block_wand_single_scorer)
    if (mt == 1 && flt == 0xFFFFFFFFu) {
      const float v = fgh::term_kth_now(ix, qt[0], k, true);
      if (v > 0.0f) h.thr0[i] = fg::make_key(v, 0xFFFFFFFFu);  // lowest key with score v
    }
    {
      float ub = fmx + cm[0];
      for (uint32_t j = 1; j < mt; ++j)
        if (j < nm || j >= nm + nx) ub += cm[j];
      set_bins(i, ub, conj_lo_div);
    }
    const uint64_t df0 = ix->off[qt[0] + 1] - ix->off[qt[0]];
    h.lead[i] = (uint32_t)df0;
    const uint32_t nch = (uint32_t)((df0 + fg::kChunk - 1) / fg::kChunk);
    if (h.citems.size() + nch > 0x7FFFFFFFull)
      return fail(FG_EUNSUPPORTED, "batch too large (%zu work items)", h.citems.size());
    // items per query: ~kConjGroupsPerQuery in a full batch; a small batch (a
    // batch of one: the p50 latency) spreads a query over up to 64 items so its
    // chunks run side by side instead of up to kMaxGroup in a row, while its
    // k_final still reads at most 64 x k candidates
    // (a multi-snapshot plan: divided by cdiv, above)
    const uint32_t per_q =
        std::max<uint32_t>(1, std::min<uint32_t>(64, std::max<uint32_t>(conj_gpq, 1024 / std::max(nq_size, 1u))) / cdiv);
    const uint32_t G = std::min<uint32_t>(conj_maxg, std::max<uint32_t>(1, (nch + per_q - 1) / per_q));
    const uint32_t ng = (nch + G - 1) / G;
    h.ngroup[i] = ng;
    for (uint32_t g = 0; g < ng; ++g)
      h.citems.push_back(WItem{(g + 0.5) / ng, i, g * G, std::min(G, nch - g * G)});
  }
  return FG_OK;
}

// How a batch of nq1 queries on S snapshots is planned in pieces: each
// snapshot's queries in P slices of >= 128 queries so the host's threads all
// plan (8 snapshots on 16 threads: 2 pieces each); piece p = s * P + r holds
// snapshot s's queries [begin(r), begin(r + 1)), and the pieces joined in order
// give the same tables and item lists as one plan per snapshot (plan_host
// sizes items by the whole batch)
struct Pieces {
  uint32_t S = 1, nq1 = 0, P = 1;
  uint32_t count() const { return S * P; }
  uint32_t begin(uint32_t r) const { return (uint32_t)((uint64_t)nq1 * r / P); }
  uint32_t slot(uint32_t pc) const { return (pc / P) * nq1 + begin(pc % P); }  // the piece's first query slot
};

// Checks the arguments and plans every piece into hs[0 .. pc.count()), serially
// or (a large batch on several snapshots) on the worker threads.  Several
// snapshots' per-query tables are copied into their slots of J by the planning
// workers themselves; join_pieces joins the lists after.
int plan_pieces(fg_index* const* ixs, uint32_t S, const fg_query_batch* q, uint32_t k, std::vector<PlanTables>& hs,
                PlanTables& J, Pieces& pc) {
  if (!ixs || !q || S == 0 || S > FG_MAX_SEGMENTS) return fail(FG_EINVAL, "bad arguments");
  for (uint32_t s = 0; s < S; ++s) {
    if (!ixs[s]) return fail(FG_EINVAL, "NULL snapshot");
    if (ixs[s]->dev != ixs[0]->dev) return fail(FG_EINVAL, "the snapshots of one plan live on different devices");
  }
  const uint32_t nq1 = q->n_queries;  // batch queries
  if ((uint64_t)S * nq1 > 0x7FFFFFFFull) return fail(FG_EUNSUPPORTED, "batch too large (%u x %u query slots)", S, nq1);
  const bool par = S > 1 && nq1 >= 64;
  pc.S = S;
  pc.nq1 = nq1;
  pc.P = par ? std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)fgh::hw_threads(0) / S, nq1 / 128)) : 1u;
  const uint32_t n = pc.count();
  if (hs.size() < n) hs.resize(n);
  bool qt = false;  // fill_view's DevPlan::feat & 4
  for (uint32_t s = 0; s < S; ++s) {
    qt |= !ixs[s]->same_stats;
    if (!fg::probe_addr_ok(ixs[s]->d)) return fail(FG_EUNSUPPORTED, "snapshot %u: device arrays above 2^47", s);
  }
  const bool beside = phrase_clauses_on.load(std::memory_order_relaxed) != 0;  // (read once per plan)
  const bool groups = group_clauses_on.load(std::memory_order_relaxed) != 0;
  const bool filters = filter_clauses_on.load(std::memory_order_relaxed) != 0;
  const bool gphrase = group_phrase_clauses_on.load(std::memory_order_relaxed) != 0;
  const bool members = group_member_phrases_on.load(std::memory_order_relaxed) != 0;
  const bool fields = field_clauses_on.load(std::memory_order_relaxed) != 0;
  const bool fphrases = fields && field_phrases_on.load(std::memory_order_relaxed) != 0;  // (only on top of it)
  if (S == 1) return plan_host(ixs[0], q, k, S, hs[0], nq1, qt, beside, groups, filters, gphrase, members, fields, fphrases);  // (used in place: nothing to join)
  J.clear();
  const size_t nq = (size_t)S * nq1, nqt = nq * fg::kMaxTerms;
  for (auto* v : {&J.q_m, &J.lead, &J.ngroup, &J.q_tier}) v->resize(nq);
  J.thr0.resize(nq);
  J.q_terms.resize(nqt);
  for (auto* v : {&J.q_ub, &J.q_wt, &J.q_wn, &J.q_rup}) v->resize(nqt);
  J.q_probe.resize(nqt);
  if (q->phrase_len)
    for (auto* v : {&J.q_pterm, &J.q_ppos}) v->resize(nqt);
  if (q->phrase_len && (beside || groups || fields)) J.q_clause.resize(nqt);
  if (q->phrase_len && groups && members) J.q_member.resize(nqt);
  auto put_slot = [&](uint32_t p) {  // piece p's per-query tables into its slots
    const PlanTables& h = hs[p];
    const size_t v0 = pc.slot(p), t0 = v0 * fg::kMaxTerms;
    auto cp = [](auto& dst, const auto& src, size_t at) { std::copy(src.begin(), src.end(), dst.begin() + at); };
    cp(J.q_m, h.q_m, v0); cp(J.lead, h.lead, v0); cp(J.ngroup, h.ngroup, v0); cp(J.thr0, h.thr0, v0);
    cp(J.q_tier, h.q_tier, v0);
    cp(J.q_terms, h.q_terms, t0);
    cp(J.q_ub, h.q_ub, t0); cp(J.q_wt, h.q_wt, t0); cp(J.q_wn, h.q_wn, t0); cp(J.q_rup, h.q_rup, t0);
    cp(J.q_probe, h.q_probe, t0);
    cp(J.q_pterm, h.q_pterm, t0); cp(J.q_ppos, h.q_ppos, t0);  // (empty without phrase_len)
    cp(J.q_clause, h.q_clause, t0);
    cp(J.q_member, h.q_member, t0);
  };
  if (par) {
    std::vector<int> rcs(n, FG_OK);
    std::vector<std::string> errs(n);
    fgh::run_parallel(n, [&](uint32_t p) {
      const uint32_t a = pc.begin(p % pc.P), b = pc.begin(p % pc.P + 1);
      fg_query_batch qp = *q;  // the slice: q_off / f_off hold absolute offsets
      qp.n_queries = b - a;
      qp.q_off = q->q_off + a;
      if (q->f_off) qp.f_off = q->f_off + a;
      if ((rcs[p] = plan_host(ixs[p / pc.P], &qp, k, S, hs[p], nq1, qt, beside, groups, filters, gphrase, members, fields, fphrases))) errs[p] = fg_last_error();
      else put_slot(p);
    });
    for (uint32_t p = 0; p < n; ++p)
      if (rcs[p]) return fail(rcs[p], "snapshot %u: %s", p / pc.P, errs[p].c_str());
  } else {
    for (uint32_t s = 0; s < S; ++s) {
      if (int rc = plan_host(ixs[s], q, k, S, hs[s], nq1, qt, beside, groups, filters, gphrase, members, fields, fphrases)) {
        const std::string e = fg_last_error();
        return fail(rc, "snapshot %u: %s", s, e.c_str());
      }
      put_slot(s);
    }
  }
  return FG_OK;
}

// The batch's tables: the one piece of a single snapshot as it is; else the
// pieces' filters, chunk lists and items appended to J in piece order (filter
// ids and item slots renumbered), and one bin geometry per batch query.
PlanTables& join_pieces(const Pieces& pc, std::vector<PlanTables>& hs, PlanTables& J) {
  if (pc.S == 1) return hs[0];
  const uint32_t S = pc.S, nq1 = pc.nq1, P = pc.P;
  auto cat = [](auto& dst, const auto& src) { dst.insert(dst.end(), src.begin(), src.end()); };
  J.f_woff.push_back(0);
  for (uint32_t p = 0; p < pc.count(); ++p) {
    const PlanTables& h = hs[p];
    const uint32_t s = p / P, fb = J.nf, vb = pc.slot(p);
    for (uint32_t f : h.q_filter) J.q_filter.push_back(f == 0xFFFFFFFFu ? f : fb + f);
    cat(J.f_shift, h.f_shift); cat(J.f_tab, h.f_tab); cat(J.f_max, h.f_max);
    const uint64_t wb = J.f_woff.back();
    for (uint32_t f = 0; f < h.nf; ++f) {
      J.f_woff.push_back(wb + h.f_woff[f + 1]);
      J.f_seg.push_back(s);
    }
    for (uint32_t f : h.ch_f) J.ch_f.push_back(fb + f);
    cat(J.ch_c, h.ch_c); cat(J.ch_t, h.ch_t); cat(J.ch_s, h.ch_s);
    for (WItem x : h.citems) { x.q += vb; J.citems.push_back(x); }
    for (WItem x : h.ditems) { x.q += vb; J.ditems.push_back(x); }
    for (WItem x : h.scan) { x.q += vb; J.scan.push_back(x); }
    for (WItem x : h.phrase) { x.q += vb; J.phrase.push_back(x); }
    for (WItem x : h.bphrase) { x.q += vb; J.bphrase.push_back(x); }
    for (WItem x : h.group) { x.q += vb; J.group.push_back(x); }
    for (WItem x : h.gphrase) { x.q += vb; J.gphrase.push_back(x); }
    for (WItem x : h.mgroup) { x.q += vb; J.mgroup.push_back(x); }
    for (WItem x : h.field) { x.q += vb; J.field.push_back(x); }
    for (WItem x : h.fphrase) { x.q += vb; J.fphrase.push_back(x); }
    J.nf += h.nf;
  }
  // one bin geometry per batch query over the snapshots where it has work
  // items (fg_plan_link's rule): a bin counts the same scores in every slot
  const uint32_t nq = S * nq1;
  for (auto* v : {&J.q_hlo, &J.q_hhi}) v->assign(nq, 0x3F800000u);
  J.q_hsh.assign(nq, 31);
  for (uint32_t i = 0, r = 0; i < nq1; ++i) {
    while (i >= pc.begin(r + 1)) ++r;  // the piece of query i
    const uint32_t li = i - pc.begin(r);
    uint32_t l = 0, hh = 0;
    bool any = false;
    for (uint32_t s = 0; s < S; ++s) {
      const PlanTables& h = hs[s * P + r];
      if (!h.ngroup[li]) continue;
      l = std::max(l, h.q_hlo[li]);
      hh = std::max(hh, h.q_hhi[li]);
      any = true;
    }
    if (!any) continue;
    const fgh::Bins b = fgh::union_bins(l, hh);
    for (uint32_t s = 0; s < S; ++s) {
      J.q_hlo[s * nq1 + i] = b.lo;
      J.q_hhi[s * nq1 + i] = b.hi;
      J.q_hsh[s * nq1 + i] = b.shift;
    }
  }
  return J;
}

bool single_list(const PlanTables& t, const WItem& x) { return t.q_m[x.q] == fg::qm_pack(1, 1, 0); }

// k_conj: the sweep split into 8 query groups, one per XCD (the kernel hands
// XCD x the x-th eighth of its items), the queries whose lead list is the
// same term in one group, groups balanced by items: headline k_conj 1.049 ->
// 1.001 ms, identical hits (profiles/r05/ab/ab_xcd_key_balanced.log; by the
// second list, ab_xcd_part.json: L2 hit rate 0.32 -> 0.23, DRAM 4.09 -> 4.57
// GB, each XCD walks the whole doc range for fewer queries).  The same split of k_disj by
// densest clause: OR top-20 2.78 -> 3.30 ms, top-1000 5.26 -> 6.86 ms -- its
// sweep stays doc-ordered.
void xcd_groups(const PlanTables& t, uint32_t nq, std::vector<uint8_t>& q_grp) {
  q_grp.assign(nq, 0);
  // grouped by the lead list (ab_xcd_key_balanced.log: and3 1.001 ms, against 1.009
  // by the second list; the last list, the query alone and the slot's snapshot
  // measured no better)
  auto probe_term = [&](uint32_t qv) { return t.q_terms[(size_t)qv * fg::kMaxTerms]; };
  // the multi-list items only (single-list ones keep the sweep and run as a
  // launch of their own, k_conj<true> over the first n_single items), counted
  // per query slot (all of a slot's items share its lead term): the slots
  // radix-sorted by term, the (term, items) counts, the terms by items
  // (a comparison sort over every item's term cost ~0.4 ms of an 8-snapshot batch)
  static thread_local std::vector<uint64_t> ka, kb;
  ka.clear();
  for (uint32_t v = 0; v < nq; ++v)
    if (t.ngroup[v] && fg::qm_must(t.q_m[v]) && t.q_m[v] != fg::qm_pack(1, 1, 0))  // (k_conj slots only)
      ka.push_back(((uint64_t)probe_term(v) << 32) | v);
  radix_sort_hi32(ka, kb);
  std::vector<std::pair<uint64_t, uint32_t>> by;  // (items, first index in ka)
  for (size_t i = 0; i < ka.size();) {
    size_t j = i;
    uint64_t c = 0;
    for (; j < ka.size() && (ka[j] >> 32) == (ka[i] >> 32); ++j) c += t.ngroup[(uint32_t)ka[j]];
    by.emplace_back(c, (uint32_t)i);
    i = j;
  }
  std::sort(by.begin(), by.end(), [&](auto& a, auto& b) {
    return a.first > b.first || (a.first == b.first && (ka[a.second] >> 32) < (ka[b.second] >> 32));
  });
  uint64_t gl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (auto& [c, i0] : by) {
    const uint32_t g = (uint32_t)(std::min_element(gl, gl + 8) - gl);
    gl[g] += c;
    for (size_t j = i0; j < ka.size() && (ka[j] >> 32) == (ka[i0] >> 32); ++j) q_grp[(uint32_t)ka[j]] = (uint8_t)g;
  }
}

// k_conj (conj): single-list queries' items first (their own k_conj launch), each part
// in sweep order; k_disj: sweep order.  A stable LSD radix sort on (not single,
// key quantized to 31 bits): the order is a scheduling choice only (every
// order gives the same hits), and it takes a fraction of a comparison sort's
// host time on a 20K-item batch.
void sort_sweep(std::vector<WItem>& items, bool conj, const PlanTables& t, uint32_t nq) {
  const size_t n = items.size();
  static thread_local std::vector<uint64_t> a, bb;  // (sort key << 32) | item index
  a.resize(n);
  // (items of queries probing the same list next to each other within each
  // 1/2048 of the sweep, so one XCD's L2 serves that list to all of them:
  // measured slower, profiles/r04/ab/ab_sweep_*.log)
  std::vector<uint8_t> q_grp;
  if (conj) xcd_groups(t, nq, q_grp);
  for (size_t x = 0; x < n; ++x) {
    const double kk = std::min(std::max(items[x].key, 0.0), 1.0);
    const bool single = single_list(t, items[x]);
    // single-list items keep the plain sweep (grouped: C3's mix 1.07 -> 1.11 ms)
    // (within a group, the sweep alone: also keying the items of one second / third /
    // lead list together inside each 1/16 or 1/64 of the sweep ran 0.971 -> 1.004 /
    // 0.999 / 0.982 ms, identical hits: profiles/r06/ab/conj_order.log)
    const uint32_t sw = conj && !single ? ((uint32_t)q_grp[items[x].q] << 28) | (uint32_t)(kk * 268435455.0)
                                        : (uint32_t)(kk * 2147483647.0);
    const uint32_t rk = (conj && single ? 0u : 0x80000000u) | sw;
    a[x] = ((uint64_t)rk << 32) | (uint64_t)x;
  }
  radix_sort_hi32(a, bb);
  static thread_local std::vector<WItem> sorted;
  sorted.resize(n);
  for (size_t x = 0; x < n; ++x) sorted[x] = items[(uint32_t)a[x]];
  items.swap(sorted);
}

// order_items' result: the work items as the device reads them (k_conj's --
// the single-list queries' first --, k_disj's, k_scan's) and each query slot's
// offset into the candidate keys
struct WorkList {
  std::vector<uint32_t> work_q, work_c, work_n;
  std::vector<uint64_t> cand_off;
  uint64_t n_single = 0, n_conj = 0, n_main = 0, n_scan = 0, n_phrase = 0, n_bphrase = 0, n_group = 0, n_gphrase = 0, n_mgroup = 0, n_field = 0, n_fphrase = 0;
  uint32_t xcd_first[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // DevPlan::xcd_first
  uint64_t count() const { return n_main + n_scan + n_phrase + n_bphrase + n_group + n_gphrase + n_mgroup + n_field + n_fphrase; }
};

// k_conj's multi-list items (sorted) cut into the 8 XCDs' stretches by expected
// work when some slot leads from a tiered copy: an item of such a slot's first
// quarter (its best tiers, up to 1/4 of the postings) weighs 1 as every
// doc-ordered item does, a later one FUGU_BAND_XCD_WEIGHT (those mostly skip
// their chunks; 1: equal counts, as without tiers).
void xcd_stretches(const PlanTables& t, WorkList& w) {
  std::fill(w.xcd_first, w.xcd_first + 9, 0u);
  static const double low_w = [] {
    const char* e = getenv("FUGU_BAND_XCD_WEIGHT");
    const double v = e && *e ? atof(e) : 1.0;  // (0.5 / 0.25 / 0.1 ran the headline 0.831 -> 0.883 / 0.890 / 0.948 ms)
    return v > 0.0 && v <= 1.0 ? v : 1.0;
  }();
  const size_t n0 = w.n_single, n = t.citems.size() - n0;
  bool any = false;
  for (size_t x = n0; x < t.citems.size() && !any; ++x) any = t.q_tier[t.citems[x].q] != 0;
  if (!any || low_w == 1.0 || n < 64) return;
  auto weight = [&](const WItem& it) { return t.q_tier[it.q] && it.key >= 0.25 ? low_w : 1.0; };
  double total = 0.0;
  for (size_t x = n0; x < t.citems.size(); ++x) total += weight(t.citems[x]);
  double cum = 0.0;
  uint32_t xcd = 1;
  for (size_t x = n0; x < t.citems.size(); ++x) {
    cum += weight(t.citems[x]);
    while (xcd < 8 && cum >= total * xcd / 8.0) w.xcd_first[xcd++] = (uint32_t)(x - n0 + 1);
  }
  while (xcd < 8) w.xcd_first[xcd++] = (uint32_t)n;
  w.xcd_first[8] = (uint32_t)n;
}

int order_items(PlanTables& t, uint32_t nq, uint32_t k, WorkList& w) {
  if (t.f_woff[t.nf] * 4 > (8ull << 30)) return fail(FG_EUNSUPPORTED, "facet masks of this batch exceed 8 GiB");
  if (t.ch_f.size() > 0x7FFFFFFFull) return fail(FG_EUNSUPPORTED, "facet postings of this batch too large");
  if (t.citems.size() + t.ditems.size() + t.scan.size() + t.phrase.size() + t.bphrase.size() + t.group.size() + t.gphrase.size() + t.mgroup.size() + t.field.size() + t.fphrase.size() > 0x7FFFFFFFull)
    return fail(FG_EUNSUPPORTED, "batch too large (%zu work items)",
                t.citems.size() + t.ditems.size() + t.scan.size() + t.phrase.size() + t.bphrase.size() + t.group.size() + t.gphrase.size() + t.mgroup.size() + t.field.size() + t.fphrase.size());
  sort_sweep(t.citems, true, t, nq);
  sort_sweep(t.ditems, false, t, nq);
  auto& items = t.items;
  items.reserve(t.citems.size() + t.ditems.size() + t.scan.size() + t.phrase.size() + t.bphrase.size() + t.group.size() + t.gphrase.size() + t.mgroup.size() + t.field.size() + t.fphrase.size());
  items.insert(items.end(), t.citems.begin(), t.citems.end());
  w.n_conj = t.citems.size();
  items.insert(items.end(), t.ditems.begin(), t.ditems.end());
  w.n_single = 0;
  for (const WItem& x : t.citems) w.n_single += single_list(t, x) ? 1 : 0;
  xcd_stretches(t, w);
  std::stable_sort(t.scan.begin(), t.scan.end(), [](const WItem& a, const WItem& b) { return a.key < b.key; });
  w.n_main = items.size();
  w.n_scan = t.scan.size();
  // k_phrase: each query's lead chunks in list order, the queries side by side (a sweep, as k_conj's)
  std::stable_sort(t.phrase.begin(), t.phrase.end(), [](const WItem& a, const WItem& b) { return a.key < b.key; });
  w.n_phrase = t.phrase.size();
  // k_bphrase: the same sweep (a union's passes side by side)
  std::stable_sort(t.bphrase.begin(), t.bphrase.end(), [](const WItem& a, const WItem& b) { return a.key < b.key; });
  w.n_bphrase = t.bphrase.size();
  // k_group: the same sweep
  std::stable_sort(t.group.begin(), t.group.end(), [](const WItem& a, const WItem& b) { return a.key < b.key; });
  w.n_group = t.group.size();
  // k_gphrase: the same sweep
  std::stable_sort(t.gphrase.begin(), t.gphrase.end(), [](const WItem& a, const WItem& b) { return a.key < b.key; });
  w.n_gphrase = t.gphrase.size();
  // k_mgroup: the same sweep
  std::stable_sort(t.mgroup.begin(), t.mgroup.end(), [](const WItem& a, const WItem& b) { return a.key < b.key; });
  w.n_mgroup = t.mgroup.size();
  // k_field: the same sweep
  std::stable_sort(t.field.begin(), t.field.end(), [](const WItem& a, const WItem& b) { return a.key < b.key; });
  w.n_field = t.field.size();
  // k_fphrase: the same sweep
  std::stable_sort(t.fphrase.begin(), t.fphrase.end(), [](const WItem& a, const WItem& b) { return a.key < b.key; });
  w.n_fphrase = t.fphrase.size();
  const uint64_t chunks = w.count();  // work items (k_conj / k_disj, then k_scan, k_phrase, k_bphrase, k_group, k_gphrase, k_mgroup, k_field, k_fphrase)
  if (chunks > 0x7FFFFFFFull) return fail(FG_EUNSUPPORTED, "batch too large (%llu work items)", (unsigned long long)chunks);
  items.insert(items.end(), t.scan.begin(), t.scan.end());
  items.insert(items.end(), t.phrase.begin(), t.phrase.end());
  items.insert(items.end(), t.bphrase.begin(), t.bphrase.end());
  items.insert(items.end(), t.group.begin(), t.group.end());
  items.insert(items.end(), t.gphrase.begin(), t.gphrase.end());
  items.insert(items.end(), t.mgroup.begin(), t.mgroup.end());
  items.insert(items.end(), t.field.begin(), t.field.end());
  items.insert(items.end(), t.fphrase.begin(), t.fphrase.end());
  w.work_q.resize(chunks);
  w.work_c.resize(chunks);
  w.work_n.resize(chunks);
  w.cand_off.assign(nq + 1, 0);
  for (uint64_t x = 0; x < chunks; ++x) {
    w.work_q[x] = items[x].q;
    w.work_c[x] = items[x].c;
    w.work_n[x] = items[x].n;
  }
  // each work item appends at most k keys to its query's candidate list
  for (uint32_t i = 0; i < nq; ++i) w.cand_off[i + 1] = w.cand_off[i] + (uint64_t)t.ngroup[i] * k;
  return FG_OK;
}

// The regions of a plan's one allocation, in order.  add() returns a region's
// offset and advances by its 256-byte-rounded size; in() / out() also note the
// device pointer to bind and (in) the host bytes to stage, which place() does
// once the workspace and the staging buffer exist.
struct Layout {
  struct Region { size_t off, bytes; const void* src; void* field; void (*bind)(void* field, char* addr); };
  std::vector<Region> regions;
  size_t end = 0;
  size_t add(size_t bytes) {
    const size_t o = end;
    end += (bytes + 255) & ~size_t(255);
    return o;
  }
  // `slot` > bytes: a region larger than what is staged into it
  template <class T>
  size_t in(T*& field, const void* src, size_t bytes, size_t slot = 0) {
    auto bind = [](void* f, char* a) { *static_cast<T**>(f) = reinterpret_cast<T*>(a); };
    regions.push_back(Region{end, bytes, src, &field, bind});
    return add(std::max(bytes, slot));
  }
  template <class T> size_t out(T*& field, size_t bytes) { return in(field, nullptr, bytes); }
  void place(char* base, char* staging) const {
    for (const Region& r : regions) {
      if (r.src && r.bytes) std::memcpy(staging + r.off, r.src, r.bytes);
      r.bind(r.field, base + r.off);
    }
  }
};

// Lays out the plan's workspace, takes it from the pool, stages the inputs
// (pinned, or pageable when no pinned buffer is had) and starts their upload
// on `up`; sets the plan's device pointers.
int stage_and_upload(fg_plan* p, fg_index* const* ixs, PlanTables& t, const WorkList& w, bool sync, hipStream_t up) {
  fg_index* ix = ixs[0];
  const uint32_t S = p->n_segs, nq = p->nq, nq1 = p->nq_batch, k = p->k, nf = t.nf;
  const uint64_t chunks = w.count();
  const size_t nch = t.ch_f.size(), nqt = (size_t)nq * fg::kMaxTerms;
  // the snapshots' first docs in their concatenation (k_final's merged select)
  std::vector<uint32_t> seg_base;
  if (S > 1) {
    uint64_t b = 0;
    for (uint32_t x = 0; x < S; ++x) {
      seg_base.push_back((uint32_t)std::min<uint64_t>(b, 0xFFFFFFFFull));
      b += ixs[x]->n_docs;
    }
    if (b > 0xFFFFFFFFull) seg_base.clear();  // no merged select past 2^32 docs
  }
  // the snapshots' tf caches (query-time scoring, DevIndex::cache): one copy per
  // distinct set of statistics (a namespace's segments share one)
  std::vector<uint32_t> cache_of(S, 0);
  for (uint32_t x = 0; x < S; ++x) {
    uint32_t c = 0;
    while (c < x && std::memcmp(ixs[cache_of[c]]->cache, ixs[x]->cache, sizeof ixs[x]->cache) != 0) ++c;
    cache_of[x] = c < x ? cache_of[c] : x;  // x: the first snapshot with these statistics
  }
  // one allocation: [inputs | zeroed (thresh, cand_cnt, facet masks, hist) | candidates | outputs | diagnostics]
  Layout L;
  L.regions.reserve(48);
  fg::DevPlan& d = p->d;
  std::vector<fg::DevIndex> segs(S > 1 ? S : 0);  // (filled once the caches' addresses are known)
  L.in(d.q_m, t.q_m.data(), 4ull * nq);
  L.in(d.q_terms, t.q_terms.data(), 4 * nqt);
  L.in(d.q_lead_df, t.lead.data(), 4ull * nq);
  L.in(d.work_q, w.work_q.data(), 4ull * chunks);
  L.in(d.work_c, w.work_c.data(), 4ull * chunks);
  L.in(d.work_n, w.work_n.data(), 4ull * chunks);
  L.in(d.cand_off, w.cand_off.data(), 8ull * (nq + 1));
  L.in(d.q_thr0, t.thr0.data(), 8ull * nq);
  L.in(d.q_ub, t.q_ub.data(), 4 * nqt);
  L.in(d.q_probe, t.q_probe.data(), sizeof(fg::ProbeDesc) * nqt);
  L.in(d.q_tier, t.q_tier.data(), 4ull * nq);
  L.in(d.q_wt, t.q_wt.data(), 4 * nqt);
  L.in(d.q_wn, t.q_wn.data(), 4 * nqt);
  L.in(d.q_rup, t.q_rup.data(), 4 * nqt);
  L.in(d.q_pterm, t.q_pterm.data(), 4 * t.q_pterm.size());
  L.in(d.q_ppos, t.q_ppos.data(), 4 * t.q_ppos.size());
  L.in(d.q_clause, t.q_clause.data(), 4 * t.q_clause.size());
  L.in(d.q_member, t.q_member.data(), 4 * t.q_member.size());
  const size_t o_cache = L.add(4ull * 512 * S);  // (room for S even when fewer distinct caches are stored)
  L.in(d.f.q_filter, t.q_filter.data(), 4ull * nq);
  L.in(d.f.f_shift, t.f_shift.data(), 4ull * nf);
  L.in(d.f.f_woff, t.f_woff.data(), 8ull * nf);
  L.in(d.f.f_tab, t.f_tab.data(), 4ull * nf * 256);
  L.in(d.f.f_max, t.f_max.data(), 4ull * nf);
  L.in(d.f.ch_filter, t.ch_f.data(), 4ull * nch);
  L.in(d.f.ch_clause, t.ch_c.data(), 4ull * nch);
  L.in(d.f.ch_term, t.ch_t.data(), 4ull * nch);
  L.in(d.f.ch_start, t.ch_s.data(), 4ull * nch);
  L.in(d.q_hlo, t.q_hlo.data(), 4ull * nq);
  L.in(d.q_hsh, t.q_hsh.data(), 4ull * nq);
  if (S > 1) {
    L.in(d.f.f_seg, t.f_seg.data(), 4ull * nf);
    L.in(d.segs, segs.data(), sizeof(fg::DevIndex) * S);
    L.in(d.seg_base, seg_base.data(), 4ull * seg_base.size(), 4ull * S);
  }
  const size_t s_in = L.end;
  // one score histogram per query (DevPlan::hist: k_conj's and k_disj's running thresholds)
  // (thresholds and histograms: one per batch query, shared by its slots)
  L.out(d.thresh, 8ull * nq1);
  L.out(d.cand_cnt, 4ull * nq);
  L.out(d.f.fmask, 4ull * t.f_woff[nf]);
  L.out(d.hist, 4ull * nq1 * fg::kQBins);
  const size_t s_zero = L.end - s_in;
  L.out(d.cand_keys, 8ull * w.cand_off[nq]);
  // own_score, own_doc, own_n consecutive: fg_plan_results reads them in one copy
  L.out(p->own_score, 4ull * nq * k);
  L.out(p->own_doc, 4ull * nq * k);
  L.out(p->own_n, 4ull * nq);
#ifdef FG_DIAG
  const size_t o_dg = L.out(d.diag, 8ull * fg::kDiagPerWg * (chunks + nq));
  p->diag_words = (L.end - o_dg) / 8;
#endif
  const size_t total = L.end;

  HIPCHK(hipSetDevice(ix->dev));
  char* base = static_cast<char*>(ix->pool->get(std::max<size_t>(total, 256), &p->ws_got));
  if (!base) return fail(FG_EOOM, "plan workspace hipMalloc(%zu) failed", total);
  p->ws = base;
  p->ix = ix;  // owns the workspace from here on (returned to ix->pool); retained below
  fg_index_retain(ix);
  for (uint32_t s = 1; s < S; ++s) {
    fg_index_retain(ixs[s]);
    p->segs.push_back(ixs[s]);
  }
  p->ws_bytes = total;
  // a small zero region (thresholds, candidate counts, facet masks) travels
  // zeroed with the upload, so the first execute needs no memset
  const size_t s_up = s_in + (s_zero <= (64u << 10) ? s_zero : 0);
  PinnedLease pin(*ix->pinned, s_up);
  std::vector<char> staging_pageable;  // only if the pinned allocation failed
  char* staging = static_cast<char*>(pin.p);
  if (!staging) {
    staging_pageable.assign(s_up, 0);
    staging = staging_pageable.data();
  } else if (s_up > s_in) {
    std::memset(staging + s_in, 0, s_up - s_in);
  }
  // the distinct tf caches, and every snapshot's view with the address of its own
  std::vector<const float*> d_cache(S, nullptr);
  for (uint32_t x = 0, n = 0; x < S; ++x) {
    if (cache_of[x] != x) continue;
    std::memcpy(staging + o_cache + 4ull * 512 * n, ixs[x]->cache, 4ull * 512);
    d_cache[x] = (const float*)(base + o_cache + 4ull * 512 * n++);
  }
  for (uint32_t x = 0; x < S; ++x) d_cache[x] = d_cache[cache_of[x]];
  p->d0 = ix->d;
  p->d0.cache = d_cache[0];
  for (uint32_t s = 0; s < S && S > 1; ++s) {
    segs[s] = ixs[s]->d;
    segs[s].cache = d_cache[s];
  }
  L.place(base, staging);
  if (seg_base.empty()) d.seg_base = nullptr;
  if (!p->diag_words) d.diag = nullptr;
  p->zero_region = base + s_in;
  p->zero_bytes = s_zero;
  // on the planning thread's own stream (or the caller's `up`): a plan built
  // while another thread's batch runs does not serialise against it through the
  // legacy null stream
  HIPCHK(hipMemcpyAsync(base, staging, s_up, hipMemcpyHostToDevice, up));
  p->up_stream = up;
  p->zeroed = s_up > s_in;
  if (sync || !pin.p) {
    HIPCHK(hipStreamSynchronize(up));
  } else {
    p->pin = pin.p;  // the plan returns it (after a sync) when destroyed
    p->pin_n = pin.n;
    pin.p = nullptr;
  }
  return FG_OK;
}

// the scalar half of the plan's device view, and what the host keeps of the bins
void fill_view(fg_plan* p, fg_index* const* ixs, PlanTables& t, const WorkList& w) {
  const uint32_t S = p->n_segs, nq = p->nq, nq1 = p->nq_batch;
  p->d.n_queries = nq;
  p->d.total_chunks = (uint32_t)w.n_main;
  p->d.n_conj = (uint32_t)w.n_conj;
  p->d.n_scan = (uint32_t)w.n_scan;
  p->d.n_phrase = (uint32_t)w.n_phrase;
  p->d.n_bphrase = (uint32_t)w.n_bphrase;
  p->d.n_group = (uint32_t)w.n_group;
  p->d.n_gphrase = (uint32_t)w.n_gphrase;
  p->d.n_mgroup = (uint32_t)w.n_mgroup;
  p->d.n_field = (uint32_t)w.n_field;
  p->d.n_fphrase = (uint32_t)w.n_fphrase;
  p->d.n_single = (uint32_t)w.n_single;
  std::copy(w.xcd_first, w.xcd_first + 9, p->d.xcd_first);
  p->d.k = p->k;
  p->d.seg_nq = S > 1 ? nq1 : 0;
  p->d.n_segs = S;
  // query-time scores when some snapshot's statistics changed since its build
  // (a commit elsewhere in the namespace); else the build-time scores
  p->d.feat = 0;
  for (uint32_t x = 0; x < S; ++x)
    if (!ixs[x]->same_stats) p->d.feat = 4u;
  for (uint32_t x = 0; x < S && p->d.feat; ++x)
    p->d.feat |= (ixs[x]->d.tfn_name ? 1u : 0u) | (ixs[x]->d.n_esc ? 2u : 0u);
  // several snapshots: a batch query's slots share its threshold score-only, so a
  // doc of another snapshot tied with the k-th score is never pruned (the merge
  // breaks such ties by snapshot)
  p->d.pub_mask = S > 1 ? 0xFFFFFFFF00000000ull : ~0ull;
  p->d.opts = fgh::conj_hist_thr() ? fg::kOptConjHistThr : 0u;
  p->n_tiered = 0;
  for (uint32_t v = 0; v < nq; ++v) p->n_tiered += t.q_tier[v] ? 1u : 0u;
  p->h_any.assign(nq1, 0);
  for (uint32_t v = 0; v < nq; ++v)
    if (t.ngroup[v]) p->h_any[v % nq1] = 1;
  p->h_lo.swap(t.q_hlo);
  p->h_hi.swap(t.q_hhi);
  p->d.f.n_filters = t.nf;
  p->d.f.n_chunks = (uint32_t)t.ch_f.size();
}

}  // namespace

// Plans of one batch on one or several snapshots of one device (a multi-
// snapshot plan: DevPlan::segs, query slot v = s * nq + q): every snapshot is
// planned on the host (in parallel for a large batch), then the slots are
// joined into ONE set of work items, uploaded once and run by one launch per
// kernel.  Several snapshots share each batch query's threshold and histogram
// (score-only), and their bins span the union of the snapshots' score ranges.
int fgh::plan_create_multi(fg_index* const* ixs, uint32_t S, const fg_query_batch* q, uint32_t k, fg_plan** out,
                           bool sync, hipStream_t up) {
  if (!out) return fail(FG_EINVAL, "bad arguments");
  // FUGU_SHARD_TRACE: the planning phases of a multi-snapshot batch on stderr
  static const bool ptrace = getenv("FUGU_SHARD_TRACE") != nullptr;
  auto pnow = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double pt[5] = {ptrace ? pnow() : 0.0, 0, 0, 0, 0};
  // this thread's buffers, reused from plan to plan (PlanTables::clear); passed
  // by reference, so the planning workers see THIS thread's copies, not their
  // own thread_local ones
  static thread_local std::vector<PlanTables> hs_tl;
  static thread_local PlanTables J_tl;
  static thread_local WorkList w_tl;
  Pieces pc;
  if (int rc = plan_pieces(ixs, S, q, k, hs_tl, J_tl, pc)) return rc;
  if (ptrace) pt[1] = pnow();
  PlanTables& t = join_pieces(pc, hs_tl, J_tl);
  if (ptrace) pt[2] = pnow();
  const uint32_t nq1 = pc.nq1, nq = S * nq1;  // batch queries, query slots
  WorkList& w = w_tl;
  if (int rc = order_items(t, nq, k, w)) return rc;
  if (ptrace) pt[3] = pnow();
  auto p = std::make_unique<fg_plan>();
  p->nq = nq;
  p->nq_batch = nq1;
  p->n_segs = S;
  p->k = k;
  p->mode = q->mode;
  p->total_chunks = (uint32_t)w.count();
  p->n_scan = (uint32_t)w.n_scan;
  p->mem.dev = ixs[0]->dev;
  if (int rc = stage_and_upload(p.get(), ixs, t, w, sync, up)) return rc;
  fill_view(p.get(), ixs, t, w);
  if (ptrace && S > 1) {
    pt[4] = pnow();
    fprintf(stderr, "[fg plan] %u snapshots x %u queries: plan_host %.3f join %.3f items %.3f stage+upload %.3f ms\n", S,
            nq1, pt[1] - pt[0], pt[2] - pt[1], pt[3] - pt[2], pt[4] - pt[3]);
  }
  *out = p.release();
  return FG_OK;
}

int fg_plan_create(fg_index* ix, const fg_query_batch* q, uint32_t k, fg_plan** out) {
  return fgh::plan_create_multi(&ix, 1, q, k, out, true, hipStreamPerThread);
}

int fg_plan_create_multi(fg_index* const* ixs, uint32_t n_segs, const fg_query_batch* q, uint32_t k, fg_plan** out) {
  return fgh::plan_create_multi(ixs, n_segs, q, k, out, true, hipStreamPerThread);
}

int fg_phrase_clauses(int on) {
  if (on < 0) return phrase_clauses_on.load(std::memory_order_relaxed);
  return phrase_clauses_on.exchange(on != 0 ? 1 : 0, std::memory_order_relaxed);
}

int fg_group_clauses(int on) {
  if (on < 0) return group_clauses_on.load(std::memory_order_relaxed);
  return group_clauses_on.exchange(on != 0 ? 1 : 0, std::memory_order_relaxed);
}

int fg_filter_clauses(int on) {
  if (on < 0) return filter_clauses_on.load(std::memory_order_relaxed);
  return filter_clauses_on.exchange(on != 0 ? 1 : 0, std::memory_order_relaxed);
}

int fg_group_phrase_clauses(int on) {
  if (on < 0) return group_phrase_clauses_on.load(std::memory_order_relaxed);
  return group_phrase_clauses_on.exchange(on != 0 ? 1 : 0, std::memory_order_relaxed);
}

int fg_group_member_phrases(int on) {
  if (on < 0) return group_member_phrases_on.load(std::memory_order_relaxed);
  return group_member_phrases_on.exchange(on != 0 ? 1 : 0, std::memory_order_relaxed);
}

int fg_field_clauses(int on) {
  if (on < 0) return field_clauses_on.load(std::memory_order_relaxed);
  return field_clauses_on.exchange(on != 0 ? 1 : 0, std::memory_order_relaxed);
}

int fg_field_phrases(int on) {
  if (on < 0) return field_phrases_on.load(std::memory_order_relaxed);
  return field_phrases_on.exchange(on != 0 ? 1 : 0, std::memory_order_relaxed);
}

int fg_plan_tiered_slots(const fg_plan* p, uint32_t* out) {
  if (!p || !out) return fail(FG_EINVAL, "bad arguments");
  *out = p->n_tiered;
  return FG_OK;
}
