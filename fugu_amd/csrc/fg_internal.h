// Internal layout shared by the host side (fugu.cpp) and the gfx950 kernels
// (kernels.hip).  See DESIGN.md §HBM layout.
#pragma once
#include <algorithm>
#include <cstdint>
#include <initializer_list>

#include <hip/hip_runtime.h>

namespace fg {

constexpr uint32_t kBlock = 128;          // tantivy block size (bytes model only)
#ifndef FG_BUCKET
#define FG_BUCKET 4  // tools/ab_variants.py: 32 -> 4 took k_conj 1.686 -> 1.591 ms, k_disj 22.8 -> 20.2 ms
#endif
constexpr uint32_t kBucketTarget = FG_BUCKET;  // directory: expected postings per bucket
constexpr uint32_t kThreads = 256;        // 4 waves of 64 per workgroup
#ifndef FG_ITEMS
#define FG_ITEMS 8
#endif
constexpr uint32_t kItems = FG_ITEMS;     // lead candidates per lane
constexpr uint32_t kChunk = kThreads * kItems;   // 2048 lead candidates per work item
constexpr uint32_t kWaveSpan = kChunk / 4;       // 512 consecutive candidates per wave
constexpr uint32_t kMaxTerms = 16;        // terms per query (FG_MAX_TERMS)
constexpr uint32_t kMaxK = 1024;          // largest top-k the device select supports
#ifndef FG_FINALCAP
#define FG_FINALCAP 4096  // tools/ab_variants.py: 8192 -> 4096 took k_final 0.132 -> 0.083 ms (5 WGs per CU), OR k=1000 0.99 -> 0.75
#endif
constexpr uint32_t kFinalCap = FG_FINALCAP;  // candidates kept in LDS by the final select (>= kMaxK)
static_assert(FG_FINALCAP >= 1024, "the final sort runs in place for up to kMaxK keys");
#ifndef FG_RANK_DIV
#define FG_RANK_DIV 16384
#endif
#ifndef FG_RANK_GIB
#define FG_RANK_GIB 64    // env FUGU_RANK_GIB
#endif
constexpr uint32_t kRankDiv = FG_RANK_DIV;    // terms in >= 1/kRankDiv of the docs may get rank words
constexpr uint64_t kRankBudget = (uint64_t)FG_RANK_GIB << 30;    // ... densest first, within this many bytes
#ifndef FG_RANK_FACTOR
#define FG_RANK_FACTOR 4.0  // tools/ab_rank_budget.py sweep (profiles/r03/ab_rank_sweep.log); env FUGU_RANK_FACTOR
#endif
constexpr double kRankFactor = FG_RANK_FACTOR;  // ... and within this many times the snapshot's posting bytes
#ifndef FG_RANK_PLAIN_DIV
#define FG_RANK_PLAIN_DIV 32  // env FUGU_RANK_PLAIN_DIV; profiles/r05/ab/ab_rank_layout.log
#endif
// ... a term in >= 1/kRankPlainDiv of the docs gets plain rank words, a sparser
// one sparse rank words (DevIndex::srank), unless plain ones cost it less
constexpr uint32_t kRankPlainDiv = FG_RANK_PLAIN_DIV;
constexpr uint32_t kMaxDense = 32767;     // slots per kind (tmeta bits 16-30)
// Doc-indexed score tables (DevIndex::dtab) of the densest terms, beside their
// rank words: a term in >= 1/kDocTabDiv of the docs (env FUGU_DOCTAB_DIV, 0: no
// tables), densest first, within 1/kDocTabFrac of the snapshot's posting bytes
// (12 B each, as the rank budget counts them) and kDocTabMax tables; k_conj
// probes one when the lead list brings >= kDocTabLead candidates per 32-doc
// table line (env FUGU_DOCTAB_LEAD, 0: always).  Sweep: DESIGN.md §3,
// profiles/doc_tables/ab/.
#ifndef FG_DOCTAB_DIV
#define FG_DOCTAB_DIV 4   // sweep: AND3 0.904 -> 0.883 ms, AND 1-5 1.021 -> 0.978 ms; 8 and wider lose it again on AND3
#endif
#ifndef FG_DOCTAB_LEAD
#define FG_DOCTAB_LEAD 8  // against the parent build, interleaved: 8 -> -0.0225 ms, 4 -> -0.0107 ms (16 loses again)
#endif
constexpr uint32_t kDocTabDiv = FG_DOCTAB_DIV;
constexpr uint32_t kDocTabLead = FG_DOCTAB_LEAD;
constexpr uint32_t kDocTabFrac = 8;
constexpr uint32_t kDocTabMax = 64;       // tables per snapshot (DocTabJob rides in the kernel arguments)
constexpr uint32_t kDocTabMinDocs = 8192; // a snapshot of fewer docs (a commit's segment: a few lead chunks
                                          // per query, and its build must stay a short launch chain) gets none
// One-byte score BOUND tables (DevIndex::dtab8) of the dense terms: byte d of a
// term's table = quant8(its psc value at doc d, the term's maximum), 0 where the
// term is absent.  k_conj reads one in front of the exact probe of a deferred
// query's first probed list: presence and an upper bound of the score from ONE
// byte of a line that serves 128 docs, and only the candidates the bound lets
// through fetch the exact score.  A term in >= 1/kDocTab8Div of
// the docs (env FUGU_DOCTAB8_DIV, 0: no tables), densest first, within the same
// caps as the f32 tables (kDocTabFrac, kDocTabMax, kDocTabMinDocs); a plan
// attaches the bound when the lead list brings >= kDocTab8Lead candidates per
// 128-doc table line (env FUGU_DOCTAB8_LEAD, 0: always).  Sweep: DESIGN.md §3,
// profiles/doctab8/.
#ifndef FG_DOCTAB8_DIV
// OFF by default: against the parent build, interleaved, the best swept setting (4 / 8) took k_conj 0.8796 ->
// 0.8669 ms where the same kernel with no tables ran 0.8550 ms (tried and dropped as a default)
#define FG_DOCTAB8_DIV 0
#endif
#ifndef FG_DOCTAB8_LEAD
#define FG_DOCTAB8_LEAD 8
#endif
constexpr uint32_t kDocTab8Div = FG_DOCTAB8_DIV;
constexpr uint32_t kDocTab8Lead = FG_DOCTAB8_LEAD;
// Score-tiered lead copies (DevIndex::bdoc / bpsc / bcmax) of the densest terms:
// a second copy of the term's postings, stably partitioned into kBandTiers tiers
// by build-time score (docs ascend inside a tier), with the exact maximum of
// every kChunk postings of the copy.  A conjunction that leads from the copy
// skips the chunks whose maximum cannot pass the first MaxScore bound, as a
// single-list query skips by cmax.  A term in >= 1/kBandDiv of the
// docs (env FUGU_BAND_DIV, 0: none) of a snapshot of >= kBandMinDocs docs (env
// FUGU_BAND_MIN_DOCS), densest first, at most kBandMax terms and within
// 1/kBandFrac (env FUGU_BAND_FRAC, 0: no cap) of the snapshot's posting bytes
// (12 B each, as the rank budget counts them).
#ifndef FG_BAND_DIV
#define FG_BAND_DIV 8
#endif
constexpr uint32_t kBandDiv = FG_BAND_DIV;
constexpr uint32_t kBandMinDocs = 8192;
constexpr uint32_t kBandMax = 64;         // copies per snapshot (BandJob rides in the kernel arguments)
constexpr uint32_t kBandFrac = 4;
constexpr uint32_t kBandTiers = 5;
// tiers 0..i together hold about kBandShares[i] / kBandShareDen of the postings, the best scores first
// (a tier's chunks span 1 / its share of the doc range a doc-ordered chunk spans, so the probes of a small
// top tier share fewer lines: 1, 2, 4, 8 sixteenths ran the headline 0.831 ms against the parent's 0.817,
// 4, 8, 12, 14 ran it 0.748: DESIGN.md §3, profiles/lead_bands/)
constexpr uint32_t kBandShareDen = 16;
constexpr uint32_t kBandShares[kBandTiers - 1] = {4, 8, 12, 14};
// the cuts come from a histogram of the scores' f32 bits >> kBandShift (128 bins per octave)
constexpr uint32_t kBandShift = 16;
constexpr uint32_t kBandBins = 1u << 15;  // scores are finite and >= 0: bits < 2^31
__host__ __device__ inline uint32_t band_bin(uint32_t bits) {
  const uint32_t b = bits >> kBandShift;
  return b < kBandBins ? b : kBandBins - 1;
}
// The cuts of a term from its histogram h[kBandBins] of df postings: lo[i] is the
// lowest bin of tiers 0..i, the highest bin b such that the bins >= b hold at
// least df * kBandShares[i] / kBandShareDen postings (and at least one).  A bin --
// so every class of equal scores -- lies wholly in one tier.
// (shares: other cumulative shares than kBandShares, ascending, in 1/kBandShareDen: env FUGU_BAND_SHARES)
__host__ __device__ inline void band_cuts(const uint32_t* h, uint64_t df, uint32_t* lo /*[kBandTiers - 1]*/,
                                          const uint32_t* shares = nullptr) {
  uint64_t cum = 0;
  uint32_t i = 0;
  for (uint32_t b = kBandBins; b-- > 0 && i < kBandTiers - 1;) {
    cum += h[b];
    while (i < kBandTiers - 1 && cum > 0 && cum * kBandShareDen >= df * (shares ? shares[i] : kBandShares[i])) lo[i++] = b;
  }
  while (i < kBandTiers - 1) lo[i++] = 0;
}
// ... and the tier of a score under them: the number of cuts above its bin
__host__ __device__ inline uint32_t band_tier(uint32_t bits, const uint32_t* lo) {
  const uint32_t b = band_bin(bits);
  uint32_t t = 0;
  for (uint32_t i = 0; i < kBandTiers - 1; ++i) t += b < lo[i] ? 1u : 0u;
  return t;
}
constexpr uint32_t kRankChunkWords = 2048;  // k_rank: words (65536 docs) per workgroup
#ifndef FG_DISJ_GPQ
#define FG_DISJ_GPQ 64
#endif
constexpr uint32_t kGroupsPerQuery = FG_DISJ_GPQ;  // k_disj / k_scan: a query's doc tiles in ~this many work items
#ifndef FG_DISJ_SPREAD
#define FG_DISJ_SPREAD 16
#endif
constexpr uint32_t kDisjSmallSpread = FG_DISJ_SPREAD;  // ... times up to this for a small batch (batch of one: x16)
#ifndef FG_GPQ
// tools/ab_variants.py (ab_group*.log, round 2): 64 -> 16 with FG_MAXGROUP 16 -> 8: k_conj 1.08 -> 1.00 ms;
// round 5 (after the XCD split and the sparse rank words), 16 -> 8 with FG_MAXGROUP 8 -> 16: headline
// k_conj + k_final 1.043 -> 1.032 ms, C3 1.112 -> 1.075 ms, identical hits (profiles/r05/ab/conj_group_r05ab.log);
// round 6 (query-time-scoring build), 8 -> 4 items: headline k_conj + k_final 1.012 -> 0.984 ms, C3 1.049 ->
// 1.046 ms (2: 0.978 / 1.065; 1: 0.981 / 1.058; 3, 5, 6 and caps 12 / 20 / 24 / 32 between or worse),
// identical hits (profiles/r06/ab/conj_group_*.log)
#define FG_GPQ 4
#endif
constexpr uint32_t kConjGroupsPerQuery = FG_GPQ;  // k_conj: a query's lead chunks in ~this many work items
#ifndef FG_MAXGROUP
#define FG_MAXGROUP 16
#endif
constexpr uint32_t kMaxGroup = FG_MAXGROUP;  // ... of at most this many chunks each
#ifndef FG_HIST_BITS
#define FG_HIST_BITS 10  // tools/ab_variants.py: 11 -> 10 took k_conj 1.110 -> 1.082 ms (LDS 40.0 -> 35.9 KB, no spills)
#endif
constexpr uint32_t kHistBits = 11;                 // radix digit width of the LDS selects
constexpr uint32_t kHistBins = 1u << kHistBits;
constexpr uint32_t kConjHistBits = FG_HIST_BITS;   // ... k_conj's (its LDS sets its occupancy)
#ifndef FG_TILE_SHIFT
#define FG_TILE_SHIFT 12
#endif
constexpr uint32_t kDisjTileShift = FG_TILE_SHIFT;   // k_disj: 4096-doc tiles
// k_disj shape (A/B builds, profiles/r03/ab/ab_disj_occ*.log): postings per
// pass, the select's digit width, waves per SIMD (3 waves / 1024 / exhaustive
// LDS tiles / 11 bits -> 5 / 512 / none / 10: OR top-1000 7.97 -> 7.02 ms, top-20
// 5.28 -> 4.59 ms, identical outputs: more waves in flight beat more postings per
// wave and the exhaustive path's LDS; then the bound-2 LDS queue (9-bit digits):
// ab_disj_queue_k*.log, OR top-20 3.92 -> 3.23 ms, top-1000 6.13 -> 5.94 ms, and the
// next-pass prefetch: ab_disj_qpf_k*.log, 3.21 -> 3.15 / 5.94 -> 5.85 ms)
#ifndef FG_DISJ_ROUND
#define FG_DISJ_ROUND 512
#endif
#ifndef FG_DISJ_HBITS
#define FG_DISJ_HBITS 9  // the queue's LDS comes out of the select's digit width
#endif
#ifndef FG_DISJ_WAVES
#define FG_DISJ_WAVES 5
#endif
#ifndef FG_DISJ_G
#define FG_DISJ_G 1  // ab_disj_g_k*.log, ab_disj_gpq_k*.log: 4 / 2 / 1 -> OR top-1000 7.00 / 6.51 / 6.13 ms, top-20 4.60 / 4.27 / 3.94 ms
#endif
#ifndef FG_DISJ_MAXGROUP
#define FG_DISJ_MAXGROUP 32
#endif
constexpr uint32_t kDisjMaxGroup = FG_DISJ_MAXGROUP;  // ... at most this many tiles per work item
constexpr uint32_t kDisjMaxPairs = 256;  // ... and at most this many (tile, Should clause) pairs (k_disj LDS)
// per-term K-th best scores kept for these K (20: the /search default limit,
// ab_ktop20_k20.log: OR top-20 k_disj 4.27 -> 4.22 ms starting from it)
constexpr uint32_t kNumTopK = 5;
constexpr uint32_t kTopKs[kNumTopK] = {1, 10, 20, 100, 1000};
// fg_index_term_ladder: the same K-th scores at the ranks between them as well
// (ascending), from which the shards of a doc-sharded namespace bound the
// namespace-wide K-th score of a term (fg_kth_floor_combine: K = 1000 over 8
// shards needs each shard's 125th).  Computed on demand, never stored.
constexpr uint32_t kNumLadderExtra = 9;
constexpr uint32_t kLadderExtra[kNumLadderExtra] = {2, 3, 5, 13, 25, 50, 125, 250, 500};
constexpr uint32_t kNumLadder = kNumTopK + kNumLadderExtra;  // FG_LADDER_LEVELS
constexpr uint32_t kLadderKs[kNumLadder] = {1, 2, 3, 5, 10, 13, 20, 25, 50, 100, 125, 250, 500, 1000};

constexpr uint32_t kPhraseMaxGroup = 4;   // k_phrase: at most this many lead chunks per work item (each item starts
                                          // from the query's published threshold: shorter items prune sooner)
constexpr uint32_t kMaxFacetClauses = 8;  // facet clauses per query (FG_MAX_FACET_CLAUSES)
constexpr uint32_t kFmaskChunk = 8192;    // facet postings per k_fmask workgroup
constexpr uint32_t kScanMaxGroup = 32;    // k_scan: at most this many 4096-doc tiles per work item

constexpr uint32_t kModeAnd = 0;
constexpr uint32_t kModeOr = 1;

// Per-query running-threshold histograms (DevPlan::hist): every work item adds
// the exact scores of the hits it keeps; the largest bin edge with at least k
// counted docs at or above it is a lower bound of the query's k-th best score
// across ALL the query's work items (and across the shards of a linked group).
constexpr uint32_t kQBins = 512;

// Histogram bin of a hit key for query bins (lo, sh), or kQBins (not counted:
// below bin 0's edge).
__host__ __device__ inline uint32_t qbin(uint64_t key, uint32_t lo, uint32_t sh) {
  const uint32_t bits = (uint32_t)(key >> 32);
  if (bits < lo) return kQBins;
  const uint32_t b = (bits - lo) >> sh;
  return b < kQBins - 1 ? b : kQBins - 1;
}

// The k-th edge of a histogram, as one step over a descending run of its bins:
// c[0 .. n) are the counts of bins `first`, first - 1, ..., and `before` docs
// are counted in the bins above `first`.  When the highest bin b with at least
// K counted docs in bins >= b is one of the run's, returns its lower edge as
// the score-only key (lo + (b << sh)) << 32 (never 0: lo >= 1), else 0.  Over
// the whole histogram (first = kQBins - 1, before = 0) that is its running
// threshold; a workgroup calls it per thread on the thread's own bins with the
// prefix of a scan.  Counts that miss adds only lower the result.
__host__ __device__ inline uint64_t hist_kth_edge(const uint32_t* c, uint32_t n, uint32_t first, uint32_t before,
                                                  uint32_t K, uint32_t lo, uint32_t sh) {
  for (uint32_t i = 0; i < n; ++i) {
    if (before < K && before + c[i] >= K) return (uint64_t)(lo + ((first - i) << sh)) << 32;
    before += c[i];
  }
  return 0ull;
}

// DevPlan::q_m packing: bits 0-7 terms in q_terms, 8-15 Must clauses (k_conj
// queries; 0 for k_disj queries), 16-23 MustNot clauses.  q_terms holds, per
// query, k_conj: [Must (cost order)][MustNot][Should (clause order)];
// k_disj: [Should (clause order)][MustNot].
__host__ __device__ inline uint32_t qm_terms(uint32_t qm) { return qm & 0xFFu; }
__host__ __device__ inline uint32_t qm_must(uint32_t qm) { return (qm >> 8) & 0xFFu; }
__host__ __device__ inline uint32_t qm_not(uint32_t qm) { return (qm >> 16) & 0xFFu; }
__host__ __device__ inline uint32_t qm_pack(uint32_t m, uint32_t nm, uint32_t nx) { return m | (nm << 8) | (nx << 16); }
// a phrase query's slot (k_phrase): bits 0-7 its distinct terms, 24-31 the phrase's terms
__host__ __device__ inline uint32_t qm_phrase(uint32_t distinct, uint32_t n) { return distinct | (n << 24); }
__host__ __device__ inline uint32_t qm_phrase_terms(uint32_t qm) { return qm >> 24; }
// A slot of k_bphrase (a phrase clause beside other clauses): q_m =
// qm_phrase(clauses, terms); its DevPlan::q_clause row holds one word per clause
// in the order of the score sum -- [Must (cost order)][MustNot][Should (clause
// order)], or without a Must [Should (clause order)][MustNot] -- packed as:
// bits 0-3 the clause's first entry in the slot's q_terms / q_pterm / q_ppos
// rows, 4-8 its terms (1: a term clause), 9-10 its occur, 11 a phrase, 16-19 its
// position in the score sum (its index in the row).
constexpr uint32_t kClMust = 0, kClShould = 1, kClMustNot = 2;  // cl_occur: fugu.h FG_OCCUR_*
constexpr uint32_t kClPhrase = 1u << 11;
__host__ __device__ inline uint32_t cl_pack(uint32_t t0, uint32_t n, uint32_t occur, bool phrase, uint32_t pos) {
  return t0 | (n << 4) | (occur << 9) | (phrase ? kClPhrase : 0u) | (pos << 16);
}
__host__ __device__ inline uint32_t cl_first(uint32_t c) { return c & 15u; }
__host__ __device__ inline uint32_t cl_terms(uint32_t c) { return (c >> 4) & 31u; }
__host__ __device__ inline uint32_t cl_occur(uint32_t c) { return (c >> 9) & 3u; }
// a k_bphrase work item's work_n: the lead chunks of its group, and above them the
// clause it leads from (a Should-driven query: the pass)
constexpr uint32_t kBpPassShift = 8;
// A slot of k_group (a group clause: fg_group_clauses): q_m and the
// q_clause row as k_bphrase's (no phrase bit), a group clause marked kClAny (a
// nested Should-only query) or kClAll (a nested Must-only one) with its members
// in [cl_first, cl_first + cl_terms) of the slot's q_terms / q_wt / q_wn / q_ub /
// q_rup rows -- PER MEMBER here: the snapshot's term id, the two field weights,
// the member's largest current score (its scaled tmaxs) and its bound factor.
// An all-of group's members stand in (cost, position) order.
constexpr uint32_t kClAny = 1u << 12, kClAll = 1u << 13;
// A slot of k_field (a field-qualified term clause, `name:report`: fg_field_clauses,
// DESIGN.md §20): q_m, the q_clause row and work_n as k_group's, every clause ONE term
// (its row as a k_group member's), a field clause marked kClText or kClName: the
// clause is that field's TermQuery -- present where the field's tf > 0, scored by
// that field's part alone.  A clause with neither bit is the unqualified term.
constexpr uint32_t kClText = 1u << 14, kClName = 1u << 15;
// a k_group work item's work_n: the lead chunks of its group, above them the
// clause it leads from and that clause's member whose list it sweeps (the pass)
constexpr uint32_t kGrpClauseShift = 8, kGrpMemberShift = 12;
// A slot of k_gphrase (a group clause beside a phrase clause: fg_group_phrase_clauses,
// DESIGN.md §18): q_m, the q_clause row and work_n as k_group's, with phrase clauses
// (kClPhrase) among the clauses; DevPlan::n_gphrase describes the rows.
// A slot of k_mgroup (a group with phrase members: fg_group_member_phrases, DESIGN.md
// §19): the same, a group's MEMBERS being runs of rows -- one row a term, two or
// more a phrase laid out as a phrase clause's rows.  DevPlan::q_member holds, per
// clause, the mask of the clause's rows that begin a member (bit r: row cl_first + r);
// a pass's member (work_n, kGrpMemberShift) counts members, not rows.

// Rank words (DevIndex::rank): one u64 per 32 docs, the low half the docs'
// presence bits, the high half the number of the term's postings before the
// word's first doc.  (40 presence bits + a 24-bit rank per word -- 1.25x the docs
// per 128-B line -- measured slower: profiles/r04/ab/ab_and.log.)
__host__ __device__ inline uint32_t rank_word(uint32_t d) { return d >> 5; }
// the term's posting position of doc d from its rank word, or 0xFFFFFFFF (absent)
__host__ __device__ inline uint32_t rank_pos(uint64_t x, uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
  // recompute the bit from d after the word's load instead of keeping it live
  // across the load (without this k_conj spills 14 VGPRs: 1.06 -> 1.41 ms,
  // profiles/r04/ab/spilled_ab_and.log)
  asm volatile("" : "+v"(d));
#endif
  const uint32_t b = d & 31u;
  if (!((x >> b) & 1ull)) return 0xFFFFFFFFu;
  const uint32_t below = (uint32_t)x & ((1u << b) - 1u);
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)(x >> 32) + (uint32_t)__popc(below);
#else
  return (uint32_t)(x >> 32) + (uint32_t)__builtin_popcount(below);
#endif
}

// Sparse rank words (DevIndex::srank, rank-kind slots above n_prank): per
// 1024-doc block one u64, the low half a bit per 32-doc word of the block that
// holds any of the term's docs, the high half the index in srank_w of the
// block's first such word; srank_w holds only those words, in the rank-word
// format above, after a zero word at index 0 (the word of every doc no sparse
// term holds: a probe loads it unconditionally, with no predicate kept live
// across the load).  A probe is the block's 8-B load, then the word's.  A term
// in 1/2000 of the docs takes ~1/25 of its plain rank words' bytes.
__host__ __device__ inline uint32_t srank_block(uint32_t d) { return d >> 10; }
// the srank_w index of doc d's word from its block entry (0: the zero word)
__host__ __device__ inline uint32_t srank_index(uint64_t e, uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(d));  // as rank_pos: nothing derived from d stays live across the word's load
#endif
  const uint32_t w = (d >> 5) & 31u;
  const uint32_t below = (uint32_t)e & ((1u << w) - 1u);
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t i = (uint32_t)(e >> 32) + (uint32_t)__popc(below);
#else
  const uint32_t i = (uint32_t)(e >> 32) + (uint32_t)__builtin_popcount(below);
#endif
  return ((e >> w) & 1ull) ? i : 0u;
}

// u8 bounds of a score range [0, M] (k_disj's sub-tile maxima): a score s as
// the least q with q8_bound(q, M) >= s; q8_bound(255, M) = M covers every
// rounding.  The kernels compute q8_bound with the same f32 operations
// (-ffp-contract=off), so the bound holds bit for bit.
__host__ __device__ inline float q8_step(float M) { return M * (1.0f / 255.0f); }
__host__ __device__ inline float q8_bound(uint32_t q, float M) { return q >= 255u ? M : (float)q * q8_step(M); }
__host__ __device__ inline uint32_t quant8(float s, float M) {
  const float st = q8_step(M);
  if (!(st > 0.0f) || !(s < M)) return 255u;
  uint32_t q = (uint32_t)fminf(254.0f, ceilf(s / st));
  while (q < 255u && q8_bound(q, M) < s) ++q;
  return q;
}
constexpr uint32_t kSubShift = 9;  // 512-doc blocks: 8 per k_disj tile

// tmeta of a term: bits 0-7 = B_t (bucket shift), 8-15 = S_t (search steps),
// 16-30 = rank slot + 1 (0: none), bit 31 = set with a slot (the round-1 f32 score tables, bit 31
// clear, went with the precomputed scores);
// rank-kind slots 1..n_prank are plain rank words, the ones above sparse (srank)
__host__ __device__ inline uint32_t meta_slot(uint32_t meta) { return (meta >> 16) & 0x7FFFu; }
__host__ __device__ inline bool meta_rank(uint32_t meta) { return (meta >> 31) != 0; }

// Device view of one namespace snapshot (all pointers device-resident).
//
// Per term t the postings are doc[off[t] .. off[t+1]) (ascending) with tfn[]
// (the posting's term frequency and its doc's fieldnorm id) alongside, and a
// doc -> position directory: bucket b covers docs [b << B_t, (b+1) << B_t) and
// dir[dir_off[t] + b] = first position in the list with doc >= b << B_t (the
// last entry is df_t).  B_t is chosen so a bucket holds ~kBucketTarget (4)
// postings; a probe is one directory load and a <= S_t step search inside one
// or two lines.  The densest terms (within a byte budget) additionally get
// RANK WORDS: one u64 per 32 docs, the low half the docs' presence bits, the
// high half the number of the term's postings before the word's first doc.  A
// probe is one 8-B load; on a hit the posting's position is rank + popcount(bits
// below the doc), and its tfn one 2-B load.  Scattered single-dword probes each
// move a 128-B line (profiles/r02_start: tools/calib_fetch gather_lines), and a
// line of rank words covers 512 docs, so the candidates of a long lead list
// share lines.
//
// Scores follow the statistics of the moment, as tantivy's TermScorer's do
// (src/db/search.rs:162 -> query/bm25.rs Bm25Weight::score).  While a
// snapshot's statistics are the ones it was built with, its postings' scores
// are the build's (psc: one 4-B load, k_score computed them once).  After a
// commit elsewhere in the namespace changed the statistics (fg_index_rescore),
// the kernels form them AT QUERY TIME instead: w_text * (tf / (tf + cache[fn]))
// (+ the name field's part) from the posting's payload (tfn), the query's
// per-clause weights (DevPlan::q_wt / q_wn) and the snapshot's tf cache
// (DevIndex::cache, set by the plan) -- so a commit only builds its new segment
// and the older ones keep every device array.  The MaxScore bounds (bmax, tmax,
// tsub, tmaxs, cmax) are the maxima under the build's statistics; a plan scales
// them by a per-clause factor q_rup >= the largest ratio of a posting's current
// score to its build-time one (1 exactly when the statistics are the build's).
constexpr uint32_t kTfEsc = 255;  // tfn's tf byte: >= this -> the exact tf is in esc_pos / esc_tf
__host__ __device__ inline uint32_t tfn_pack(uint32_t tf, uint32_t fn) { return (fn << 8) | (tf < kTfEsc ? tf : kTfEsc); }
struct DevIndex {
  const uint32_t* doc;       // [P] doc ids, CSR by term, ascending within a term
  const float* psc;          // [P] the posting's score under the statistics the snapshot was BUILT with
                             //     (k_score, tantivy's f32 order): what a plan over snapshots whose
                             //     statistics are still the build's reads (DevPlan::feat without kFQt)
  const uint16_t* tfn;       // [P] (fn_text[doc] << 8) | min(tf_text, 255): tf_text 0 = no text occurrence
  const uint16_t* tfn_name;  // [P] the same for the `name` field, or nullptr (no name postings)
  const uint64_t* esc_pos;   // [n_esc] postings whose tf byte is kTfEsc in either field, ascending
  const uint32_t* esc_tf;    // [n_esc] their exact tf_text | tf_name << 16
  const float* cache;        // [256 or 512] K1 * ((1 - B) + B * TABLE[id] / avgdl): text, then name (plan-set)
  const uint64_t* off;       // [V+1] posting offsets
  const uint32_t* dir;       // [D] bucket directory (positions within the list)
  const uint32_t* dir_off;   // [V] first directory entry of each term
  const uint32_t* tmeta;     // [V] meta_slot / meta_rank above
  const uint64_t* rank;      // [n_prank * rank_words] rank words, rank-kind slots 1..n_prank
  const uint64_t* srank;     // [n_srank * srank_blocks] sparse rank block entries, rank-kind slots above
  const uint64_t* srank_w;   // sparse rank words (srank_index)
  const float* tmaxs;        // [V] largest posting score of each term (build statistics)
  const uint32_t* alive;     // [ceil(N/32)] alive bitset, or nullptr (no deletes)
  const float* bmax;         // [D] parallel to dir: max term score of the postings in each bucket
  const float* tmax;         // tile maxima (k_disj tiles) of the terms with B_t <= kDisjTileShift
  const uint32_t* toff;      // [V] first tmax / tdir entry of each term (n_tiles + 1 per term), or
                             //     0xFFFFFFFF (bucket >= tile: use bmax)
  const uint32_t* tdir;      // tile directory: tdir[toff[t] + i] = first posting of t at doc >= i << kDisjTileShift
  const uint64_t* tsub;      // parallel to tmax: byte b = the largest posting score among the tile's docs
                             //     [b << kSubShift, (b + 1) << kSubShift) quantized up against the tile maximum
                             //     (q8_bound); a bucket wider than a block counts in every block it covers
  const float* cmax;         // [score chunks] largest posting score of each kChunk-posting chunk of a
                             //     list (block-max: k_conj skips a lead chunk that cannot reach the threshold)
  const uint32_t* coff;      // [V] index of each term's first chunk in cmax
  const float* dtab;         // [n tables * dtab_stride] doc-indexed score tables of the densest terms (build
                             //     statistics, as psc): entry d of a table = the term's psc value at doc d,
                             //     -1.0f where the term is absent.  k_conj reads them through its probe
                             //     descriptors (kPdTab); which term owns which table: fg_index::dtab_map (host)
  const uint8_t* dtab8;      // [n tables * dtab8_stride] one-byte bound tables of the dense terms (build statistics):
                             //     byte d of a table = quant8(the term's psc value at doc d, tmaxs[term]), never 0
                             //     for a posting, 0 where the term is absent.  k_conj reads them through the
                             //     bound fields of clause 1's probe descriptor (kPdBound); which term owns which
                             //     table: fg_index::dtab8_map (host)
  const uint32_t* bdoc;      // [band postings] the score-tiered copies of the densest terms' doc ids (kBand*):
                             //     a term's df postings tier by tier, docs ascending inside a tier; which term
                             //     owns which run: fg_index::band_map (host)
  const float* bpsc;         // [band postings] ... and their build-time scores, the psc values bit for bit
  const float* bcmax;        // [band chunks] the largest score of each kChunk postings of a term's copy
  const uint32_t* fdoc;      // [PF] facet postings (doc ids, ascending), CSR by facet term
  const uint64_t* foff;      // [VF+1]
  uint64_t n_esc;
  uint32_t n_docs;
  uint32_t n_terms;
  uint32_t has_name;
  uint32_t n_fterms;
  uint32_t rank_words;       // words per plain rank-kind term: ceil(N / 32)
  uint32_t n_prank;          // plain rank-kind slots
  uint32_t srank_blocks;     // block entries per sparse rank-kind term: ceil(N / 1024)
  uint32_t dtab_stride;      // floats per score table: N rounded up to a 128-B line
  uint32_t dtab8_stride;     // bytes per bound table: N rounded up to a 128-B line
  // Forward index (fg_docs_input::keep_positions; nullptr without): per field the
  // doc's tokens addressed by POSITION, fwd[fwd_off[d] + p] = the VOCABULARY id of
  // the token at analyzer position p of doc d, kFwdNone where the analyzer dropped
  // one (RemoveLongFilter).  k_phrase verifies its candidates against it.  Shared
  // by a snapshot and its rescores (structure).
  const uint64_t* fwd_off;   // [N+1]
  const uint32_t* fwd;       // [fwd_off[N]]
  const uint64_t* fwd_off_name;  // [N+1], or nullptr (no `name` values)
  const uint32_t* fwd_name;
};
constexpr uint32_t kFwdNone = 0xFFFFFFFFu;  // a dropped position: equals no term id

// The exact tf_text | tf_name << 16 of posting p whose tf byte escaped (binary
// search of the snapshot's escape list; rare: tf >= 255)
__host__ __device__ inline uint32_t tf_escaped(const uint64_t* esc_pos, const uint32_t* esc_tf, uint64_t n, uint64_t p) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (esc_pos[mid] < p) lo = mid + 1; else hi = mid;
  }
  return lo < n ? esc_tf[lo] : 0u;
}

// Bm25Weight::score in tantivy's f32 operation order (query/bm25.rs: weight *
// (tf / (tf + cache[fieldnorm_id]))) for one field.  -ffp-contract=off and IEEE
// f32 division: bit-identical to the host arithmetic (fugu.cpp, the oracle).
__host__ __device__ inline float field_score(uint32_t tf, uint32_t fn, float w, const float* cache) {
  const float f = (float)tf;
  return w * (f / (f + cache[fn]));
}

// Probe descriptors (DevPlan::q_probe): everything k_conj needs to read one
// clause's lists, as eight words per (query slot, clause position) that the
// planner fills and a probe stage loads with ONE scalar load -- where the kernel
// used to chase terms[i] -> tmeta[t] / off[t] / dir_off[t] through two dependent
// memory round trips in front of every probe (probe descriptors).
// Three byte ranges, each a 48-bit device address (low word + a 16-bit high
// part) and, for the two the kernel reads through buffer resources, a size:
//   structure  entry i >= 1: the probed term's plain rank words, its sparse
//              block entries (then srank_index into DevIndex::srank_w), its
//              bucket directory, or (kPdTab) its doc-indexed score table, which
//              is read in place of both the structure and the scores; entry 0
//              (the lead list): its doc ids;
//   scores     the term's build-time scores psc + off[t], or (a query-time plan,
//              DevPlan::feat & 4) its tfn payloads;
//   aux        a directory term's doc ids doc + off[t] (no size: read through
//              plain loads inside the directory's buckets).
// A load through a range's buffer resource at a byte offset past its size moves
// no bytes and returns 0, so a lane that is not live passes kPdDead* and needs
// no branch.  A range of more than kPdMaxBytes cannot be addressed that way:
// kPdWide then tells the kernel to read that clause's ranges with plain
// predicated loads from the same base addresses.
struct ProbeDesc {
  uint32_t base_lo;   // structure: address bits 0-31
  uint32_t bytes;     //            size in bytes
  uint32_t sc_lo;     // scores / payloads: address bits 0-31
  uint32_t sc_bytes;  //            size in bytes
  uint32_t aux_lo;    // a directory term's doc ids: address bits 0-31
  uint32_t hi;        // address bits 32-47: structure | scores << 16
  uint32_t kind;      // bits 0-5 shift (structure index = doc >> shift: 5 plain rank words, 10 sparse
                      // block entries, B_t directory), 6-11 S_t (directory search steps), kPd* flags,
                      // 16-31 aux address bits 32-47
                      // A rank-word or table clause has no aux range and no S_t; entry 1 of a deferred
                      // query may carry a BOUND there (probe_desc_bound): kPdBound (bit 6), the bound
                      // table's address in aux_lo / bits 16-31, the term's maximum in ENTRY 0's aux_lo
  uint32_t ub;        // f32 bits of q_ub[i + 1], the MaxScore bound applied after list i (0.0 past the last)
};
static_assert(sizeof(ProbeDesc) == 32, "one s_load_dwordx8");
constexpr uint32_t kPdDir = 1u << 12;     // a bucket directory (else rank words)
constexpr uint32_t kPdWide = 1u << 13;    // a range does not fit a buffer resource: plain loads
constexpr uint32_t kPdSparse = 1u << 14;  // sparse rank words: the structure holds block entries
constexpr uint32_t kPdTab = 1u << 15;     // a doc-indexed score table (DevIndex::dtab): the score at doc << 2
constexpr uint32_t kPdBound = 1u << 6;    // (never with kPdDir) aux = the term's one-byte bound table (DevIndex::dtab8)
constexpr uint32_t kPdMaxBytes = 0x80000000u;  // largest range read through a buffer resource
// offsets of a lane that is not live: past every range, aligned to the load, and no
// dword of the load wraps around 2^32
constexpr uint32_t kPdDead8 = 0xFFFFFFF8u, kPdDead4 = 0xFFFFFFFCu, kPdDead2 = 0xFFFFFFFEu;
__host__ __device__ inline uint32_t pd_shift(uint32_t kind) { return kind & 0x3Fu; }
__host__ __device__ inline uint32_t pd_steps(uint32_t kind) { return (kind >> 6) & 0x3Fu; }
__host__ __device__ inline uint64_t pd_base(const ProbeDesc& p) { return ((uint64_t)(p.hi & 0xFFFFu) << 32) | p.base_lo; }
__host__ __device__ inline uint64_t pd_scores(const ProbeDesc& p) { return ((uint64_t)(p.hi >> 16) << 32) | p.sc_lo; }
__host__ __device__ inline uint64_t pd_aux(const ProbeDesc& p) { return ((uint64_t)(p.kind >> 16) << 32) | p.aux_lo; }

// What the planner knows of a term on the host (fg_index: off, tmeta, dir_off)
struct ProbeTerm {
  uint64_t off, end;  // its postings [off, end)
  uint32_t meta;      // tmeta
  uint32_t dir_off;   // first directory entry
  uint32_t tab;       // its score table's slot + 1 (DevIndex::dtab), 0: none
};

// Does a probe of a term with a score table (df of n_docs docs) read the table?
// A table line covers 32 docs, so lead_df * 32 / n_docs lead candidates share
// one: at least tab_lead of them (0: always), or the term is in half the docs
// (its psc is then as dense as its table).
inline bool probe_uses_table(uint64_t n_docs, uint64_t df, uint64_t lead_df, uint32_t tab_lead) {
  return lead_df * 32 >= n_docs * tab_lead || df * 2 >= n_docs;
}

// Do the arrays the descriptors point into lie where 48 bits address them?
// (every array is < 2^47 bytes, so its base below 2^47 covers its end)
inline bool probe_addr_ok(const DevIndex& ix) {
  for (const void* p : {(const void*)ix.doc, (const void*)ix.psc, (const void*)ix.tfn, (const void*)ix.dir,
                        (const void*)ix.rank, (const void*)ix.srank, (const void*)ix.dtab, (const void*)ix.dtab8,
                        (const void*)ix.bdoc, (const void*)ix.bpsc})
    if ((uint64_t)(uintptr_t)p >> 47) return false;
  return true;
}

// The descriptor of term t for a plan over snapshot view ix (device addresses;
// nothing is dereferenced): the lead list's (entry 0) or a probed list's, with
// the build-time scores or (qt) the payloads, ub = q_ub[i + 1].  A probed term
// with a score table gets a kPdTab descriptor over it when the plan runs on the
// build-time scores and the lead list (lead_df postings) is dense enough
// (probe_uses_table, tab_lead).
inline ProbeDesc probe_desc(const DevIndex& ix, const ProbeTerm& t, bool lead, bool qt, float ub, uint64_t lead_df = 0,
                            uint32_t tab_lead = kDocTabLead) {
  const uint64_t df = t.end - t.off;
  uint64_t base, bytes, aux = 0;
  uint32_t kind;
  const uint32_t slot = meta_slot(t.meta);
  if (lead) {
    base = (uint64_t)(uintptr_t)(ix.doc + t.off);
    bytes = df * 4;
    kind = 0;
  } else if (!qt && t.tab && ix.dtab && probe_uses_table(ix.n_docs, df, lead_df, tab_lead)) {
    base = (uint64_t)(uintptr_t)(ix.dtab + (uint64_t)(t.tab - 1) * ix.dtab_stride);
    bytes = (uint64_t)ix.n_docs * 4;  // (<= kPdMaxBytes: a longer table is not built)
    kind = kPdTab;
  } else if (slot && slot <= ix.n_prank) {
    base = (uint64_t)(uintptr_t)(ix.rank + (uint64_t)(slot - 1) * ix.rank_words);
    bytes = (uint64_t)ix.rank_words * 8;
    kind = 5u;
  } else if (slot) {
    base = (uint64_t)(uintptr_t)(ix.srank + (uint64_t)(slot - 1 - ix.n_prank) * ix.srank_blocks);
    bytes = (uint64_t)ix.srank_blocks * 8;
    kind = 10u | kPdSparse;
  } else {
    const uint32_t B = t.meta & 0xFFu, S = (t.meta >> 8) & 0xFFu;
    base = (uint64_t)(uintptr_t)(ix.dir + t.dir_off);
    bytes = ((((uint64_t)(ix.n_docs ? ix.n_docs - 1 : 0)) >> B) + 2) * 4;  // one entry per bucket and the closing one
    aux = (uint64_t)(uintptr_t)(ix.doc + t.off);
    kind = (B & 0x3Fu) | ((S & 0x3Fu) << 6) | kPdDir;
  }
  // (a table stands for the scores too: the kernel's score loads go through this range)
  const bool tab = (kind & kPdTab) != 0;
  const uint64_t sc = tab ? base : qt ? (uint64_t)(uintptr_t)(ix.tfn + t.off) : (uint64_t)(uintptr_t)(ix.psc + t.off);
  const uint64_t sc_bytes = tab ? bytes : df * (qt ? 2 : 4);
  // (addresses are packed in 48 bits: the planner refuses a snapshot whose arrays lie higher, probe_addr_ok)
  if (bytes > kPdMaxBytes || sc_bytes > kPdMaxBytes) kind |= kPdWide;
  ProbeDesc p;
  p.base_lo = (uint32_t)base;
  p.bytes = (uint32_t)std::min<uint64_t>(bytes, 0xFFFFFFFFull);
  p.sc_lo = (uint32_t)sc;
  p.sc_bytes = (uint32_t)std::min<uint64_t>(sc_bytes, 0xFFFFFFFFull);
  p.aux_lo = (uint32_t)aux;
  p.hi = (uint32_t)((base >> 32) & 0xFFFFu) | (uint32_t)((sc >> 32) & 0xFFFFu) << 16;
  p.kind = kind | (uint32_t)((aux >> 32) & 0xFFFFu) << 16;
  union { float f; uint32_t u; } c;
  c.f = ub;
  p.ub = c.u;
  return p;
}

// Does clause 1 of a deferred query read its term's bound table first?  The
// shape of probe_uses_table with a line of 128 docs: at least tab8_lead lead
// candidates per table line (0: always), or the term is in half the docs.
inline bool probe_uses_bound(uint64_t n_docs, uint64_t df, uint64_t lead_df, uint32_t tab8_lead) {
  return lead_df * 128 >= n_docs * tab8_lead || df * 2 >= n_docs;
}

// The bound of clause 1 (p1, the first probed list's descriptor as probe_desc
// made it; lead: entry 0): attached when the query takes k_conj's deferred path
// (>= 3 unfiltered Must lists and nothing else), the plan runs on build-time
// scores (!qt), the term has a bound table (tab8: its slot + 1) and the lead
// rule holds.  p1's exact ranges stay what they are; its unused aux fields take
// the table's address and kPdBound, entry 0's unused aux_lo the f32 bits of M
// (the term's build-time maximum, tmaxs: what the table was quantized against).
// Returns whether it was attached; otherwise both descriptors are untouched.
inline bool probe_desc_bound(const DevIndex& ix, ProbeDesc& lead, ProbeDesc& p1, uint32_t tab8, float M, bool deferred,
                             bool qt, uint64_t df, uint64_t lead_df, uint32_t tab8_lead = kDocTab8Lead) {
  if (!deferred || qt || !tab8 || !ix.dtab8 || !(M > 0.0f)) return false;
  if (p1.kind & (kPdDir | kPdWide)) return false;  // (a table term has rank words; a wide clause is probed item by item)
  if (!probe_uses_bound(ix.n_docs, df, lead_df, tab8_lead)) return false;
  const uint64_t a = (uint64_t)(uintptr_t)(ix.dtab8 + (uint64_t)(tab8 - 1) * ix.dtab8_stride);
  p1.aux_lo = (uint32_t)a;
  p1.kind = (p1.kind & 0xFFFFu) | kPdBound | (uint32_t)((a >> 32) & 0xFFFFu) << 16;
  union { float f; uint32_t u; } c;
  c.f = M;
  lead.aux_lo = c.u;
  return true;
}

// The lead descriptor of a slot that leads from its term's score-tiered copy
// (build-time plans only): the doc ids and scores of the copy at posting boff of
// bdoc / bpsc in place of the doc-ordered list's; sizes, aux and ub stay.  The
// slot's DevPlan::q_tier word tells the kernel, and where the chunk maxima lie.
inline void probe_desc_tier(const DevIndex& ix, ProbeDesc& lead, uint64_t boff) {
  const uint64_t base = (uint64_t)(uintptr_t)(ix.bdoc + boff), sc = (uint64_t)(uintptr_t)(ix.bpsc + boff);
  lead.base_lo = (uint32_t)base;
  lead.sc_lo = (uint32_t)sc;
  lead.hi = (uint32_t)((base >> 32) & 0xFFFFu) | (uint32_t)((sc >> 32) & 0xFFFFu) << 16;
}

// Facet filters of a planned batch (DevPlan).  Every distinct clause list
// (filter) gets a doc-indexed mask in HBM built by k_fmask from the facet
// postings: 2^shift bits per doc (shift 0..3, >= the filter's clause count),
// bit i set when the doc holds clause i's facet term.  f_tab[f*256 + bits] is
// the facet union's score for that set of matching clauses, summed on the
// host in clause order from 0.0 (SumCombiner), so the kernels add one f32.
struct DevFilters {
  uint32_t n_filters;
  uint32_t n_chunks;            // k_fmask workgroups
  const uint32_t* q_filter;     // [nq] filter of each query, 0xFFFFFFFF = none
  const uint32_t* f_shift;      // [n_filters] log2(bits per doc)
  const uint64_t* f_woff;       // [n_filters] first mask word
  const float* f_tab;           // [n_filters * 256]
  const float* f_max;           // [n_filters] largest f_tab entry (upper bound of the facet score)
  const uint32_t* ch_filter;    // [n_chunks] k_fmask chunk -> filter
  const uint32_t* ch_clause;    // [n_chunks] clause index in the filter
  const uint32_t* ch_term;      // [n_chunks] facet term
  const uint32_t* ch_start;     // [n_chunks] first posting of the chunk within the term's list
  const uint32_t* f_seg;        // [n_filters] the snapshot of each filter (multi-snapshot plans), or nullptr
  uint32_t* fmask;              // workspace, zeroed per run
};

__host__ __device__ inline uint32_t filter_bits(const uint32_t* mask, uint32_t shift, uint32_t d) {
  const uint32_t bit = d << shift;  // fits: the plan rejects n_docs << shift > 2^32
  return (mask[bit >> 5] >> (bit & 31)) & ((1u << (1u << shift)) - 1u);
}

// Device view of one planned batch.  Work items (query, 2048-candidate chunk
// of the query's lead list) are ordered as a doc sweep across the batch:
// items covering similar doc ranges of different queries run together, so the
// segments of hot posting lists they probe are shared through L2 / MALL.
constexpr uint32_t kMaxPeers = 15;  // peers of one plan (fugu.h FG_MAX_PEERS, fg_plan_set_peers)
// DevPlan::opts bit: a multi-list k_conj item that ends reads the query's bins
// back as it adds to them and publishes the query-wide k-th edge as a threshold
// (FUGU_CONJ_HIST_THR, default on)
constexpr uint32_t kOptConjHistThr = 1u;

struct DevPlan {
  uint32_t n_queries;
  uint32_t total_chunks;        // k_conj items [0, n_conj) then k_disj items [n_conj, total_chunks)
  uint32_t k;
  uint32_t n_conj;
  const uint32_t* q_m;          // [nq] packed term counts (qm_terms / qm_must / qm_not)
  const uint32_t* q_terms;      // [nq * kMaxTerms] term ids (layout: qm_pack above)
  const uint32_t* q_lead_df;    // [nq] length of the lead list (0 => empty result)
  const uint32_t* work_q;       // [total_chunks] query of each work item (sweep order)
  const uint32_t* work_c;       // [total_chunks] first chunk of the item's group (k_disj: first tile)
  const uint32_t* work_n;       // [total_chunks] chunks in the item's group (k_disj: tiles)
  const uint64_t* cand_off;     // [nq+1] candidate-list capacity offsets (work items of q * k)
  const uint64_t* q_thr0;       // [nq] starting threshold key, read by every top-k kernel; 0 = none (planned for k_disj / k_conj slots only: per-term top-K bound)
  const float* q_ub;            // [nq * kMaxTerms] k_conj MaxScore bounds: q_ub[i] = sum over the query's
                                //     terms j >= i (intersection order) of their scaled tmaxs, i >= 1
  const ProbeDesc* q_probe;     // [nq * kMaxTerms] k_conj's probe descriptors, on the slot's own snapshot: entry 0
                                //     the lead list's, entry i the i-th probed list's (q_terms order) with
                                //     q_ub[i + 1]; the first qm_terms entries of a k_conj slot are filled
  const uint32_t* q_tier;       // [nq] a k_conj slot that leads from its lead term's score-tiered copy (entry 0
                                //     of q_probe points at bdoc / bpsc): 1 + the index in DevIndex::bcmax of the
                                //     copy's first chunk; 0: the doc-ordered list
  const float* q_wt;            // [nq * kMaxTerms] each clause's BM25 weight, text field (query time)
  const float* q_wn;            // [nq * kMaxTerms] ... and name field
  const float* q_rup;           // [nq * kMaxTerms] factor on the clause's build-time bounds (tmax, bmax,
                                //     cmax, tsub's tile maxima): >= current score / build score of any posting
  const uint32_t* q_hlo;        // [nq] f32 bits of the histogram's bin 0 lower edge
  const uint32_t* q_hsh;        // [nq] bin width: 2^q_hsh f32 ulps
  // workspace, zeroed per run (thresh and hist may be a linked group's shared ones)
  uint64_t* thresh;             // [nq] monotone lower bound on the k-th best key (published score-only)
  uint32_t* hist;               // [nq * kQBins] counted hits per score bin
  uint64_t pub_mask;            // thresholds published as key & pub_mask: ~0 exact, or score-only (linked)
  uint32_t* cand_cnt;           // [nq] keys appended to each query's candidate list
  uint64_t* cand_keys;          // [cand_off[nq]] per-query candidate lists
  uint64_t* diag;               // diagnostic builds only (-DFG_DIAG): per-workgroup stamps
  uint32_t feat;                // kernel features the plan's snapshots need: bit 2 query-time scores (a snapshot
                                // whose statistics changed since its build), with bit 0 `name` postings
                                // (tfn_name) and bit 1 escaped tf bytes (esc_pos); the kernels are instantiated
                                // per value (0, 4 = query-time, 7 = query-time with names / escapes)
  uint32_t opts;                // planner settings read when the plan is made: kOptConjHistThr
  uint32_t xcd_first[9];        // k_conj's multi-list items by XCD, when the planner balanced them by expected
                                // work (tiered leads: items that mostly skip): XCD x runs the items
                                // [xcd_first[x], xcd_first[x + 1]) after the n_single first; xcd_first[8] = 0:
                                // equal counts
  uint32_t n_single;            // k_conj: the first n_single work items belong to single-list queries
  uint32_t n_scan;              // k_scan work items (queries with no text terms), after the total_chunks
                                // k_conj / k_disj items in work_q / work_c / work_n
  uint32_t n_phrase;            // k_phrase work items (phrase queries), after the k_scan items: (query slot,
                                // group of kChunk-posting chunks of the phrase's lead list).  A phrase slot's
                                // q_terms row holds its distinct terms (the snapshot's ids), the lead -- the
                                // one with the shortest list -- first; q_m = qm_phrase(distinct, terms);
                                // q_wt[row][0] / q_wn[row][0] are the phrase's two field weights
  const uint32_t* q_pterm;      // [nq * kMaxTerms] a phrase's terms as VOCABULARY ids (DevIndex::fwd), the
                                //     anchor -- the rarest term's first occurrence in the phrase -- first
  const uint32_t* q_ppos;       // [nq * kMaxTerms] ... and their position offsets within the phrase
  uint32_t n_bphrase;           // k_bphrase work items (queries with a phrase clause beside other clauses:
                                // fg_phrase_clauses), after the k_phrase items: (query slot, group of kChunk-
                                // posting chunks of a lead list, the clause led from in work_n's upper bits).
                                // Such a slot's q_terms / q_pterm / q_ppos rows hold every clause's terms
                                // (local ids / vocabulary ids / offsets), clause after clause in q_clause's
                                // order, a phrase's anchor first; q_wt / q_wn [row][c] are clause c's weights
  uint32_t n_fphrase;           // k_fphrase work items (queries with a field-qualified phrase clause,
                                // `name:"annual report"`, or a field term clause beside a phrase clause:
                                // fg_field_phrases), after the k_field items.  Such a slot's q_m,
                                // q_clause row, q_terms / q_pterm / q_ppos rows and work_n are k_bphrase's, a
                                // field clause -- a term or a phrase (kClPhrase) -- marked kClText or kClName:
                                // present where THAT field holds the term (the phrase), scored by that field's
                                // part alone.  A field phrase's first row, the anchor, is its term with the
                                // fewest postings in that field; q_wt / q_wn [c] hold clause c's weights, of
                                // which a field clause uses its field's
  const uint32_t* q_clause;     // [nq * kMaxTerms] the clause table (cl_pack); empty without such a slot
  uint32_t n_group;             // k_group work items (queries with a group clause: fg_group_clauses), after the
                                // k_bphrase items: (query slot, group of kChunk-posting chunks of a lead list,
                                // the (clause, member) led from in work_n's upper bits)
  uint32_t n_gphrase;           // k_gphrase work items (queries with a group clause AND a phrase clause:
                                // fg_group_phrase_clauses), after the k_group items, work_n as k_group's.  Such a
                                // slot's rows hold every clause's terms, clause after clause in q_clause's order:
                                // q_terms the snapshot's ids; q_wt / q_wn / q_ub / q_rup per member for term
                                // clauses and group members (as k_group's); a phrase clause (kClPhrase) has
                                // q_pterm / q_ppos over its rows (the anchor first), its two field weights in
                                // q_wt / q_wn at its first row, and q_ub = (text weight, name weight, 0, ...) over
                                // its rows (a field's entry 0.0 where the phrase cannot match in the snapshot), so
                                // group_bound's sum over a clause's rows bounds the phrase's score
  uint32_t n_mgroup;            // k_mgroup work items (queries with a group that holds a phrase member:
                                // fg_group_member_phrases), after the k_gphrase items, work_n as k_group's with
                                // the pass's member counted in members.  The rows as k_gphrase's; a phrase
                                // MEMBER's rows are a phrase clause's (anchor first, q_pterm / q_ppos, the field
                                // weights at its first row, q_ub = (text weight, name weight, 0, ...))
  uint32_t n_field;             // k_field work items (queries with a field-qualified term clause:
                                // fg_field_clauses), after the k_mgroup items, work_n as k_group's (the member 0)
  const uint32_t* q_member;     // [nq * kMaxTerms] per clause of such a slot: the mask of its rows that begin a
                                // member; empty without fg_group_member_phrases
  // Multi-snapshot plans (several segments / doc shards / namespaces of one
  // device in ONE launch per kernel): query slot v = s * seg_nq + q is query q
  // of the batch on snapshot segs[s]; every per-query array above is indexed by
  // the slot, except thresh and hist, which are the batch query's own (shared
  // score-only by the slots of q: pub_mask).  seg_nq = 0: one snapshot (the
  // kernel's DevIndex argument).
  const DevIndex* segs;         // [n_segs] or nullptr
  uint32_t seg_nq;              // queries of the batch (slots per snapshot), 0 = one snapshot
  uint32_t n_segs;
  const uint32_t* seg_base;     // [n_segs] first doc of each snapshot in the concatenation (k_final's merged
                                // select), or nullptr when the snapshots hold >= 2^32 docs together
  DevFilters f;
  // Peer plans (fg_plan_set_peers: the other doc shards of one namespace, on
  // other devices or in other processes): every threshold this plan publishes
  // and every count it adds to its histogram also go, score-only, into the
  // peers' thresh / hist of the same batch query, so each shard prunes with the
  // hits of all of them as they are found (the cross-device form of
  // fg_plan_link's shared words)
  uint32_t n_peers;
  uint32_t* peer_hist[kMaxPeers];
  uint64_t* peer_thr[kMaxPeers];
};

// The batch query of a query slot (thresh / hist index)
__host__ __device__ inline uint32_t slot_query(const DevPlan& pl, uint32_t v) {
  return pl.seg_nq ? v % pl.seg_nq : v;
}

// Device view of one (snapshot, query slice) pass of fg_count_batch (count.cpp;
// DESIGN.md §12): hit totals and facet counts, no scores.  Query slot i of the
// slice owns the bitmap match[i * words .. + words) (one bit per doc, zeroed
// per pass); the kernels run back to back on one stream:
//   k_cfilter  one bit per doc of each distinct facet clause list (the union
//              of its lists) into fbits[f * words ..];
//   k_cmatch   work items (slot, kCountChunk postings of a driver list): a
//              Should-only query drives every Should list, a Must-driven one its
//              shortest Must list, a textless filtered one the filter's facet
//              lists; AllQuery's items fill its words with ones.  Each doc is
//              probed in the slot's other Must lists and its MustNot lists
//              (term_has_doc), tested in the filter's bitmap, then set in match;
//   k_ccount   match &= alive, the bits at or past N cleared, popcount into
//              total[q0 + i];
//   k_cfacet   work items (count term j, kCountFacetChunk postings of its facet
//              list): the docs are loaded once and tested in every slot's bitmap,
//              count[(q0 + i) * n_count + j] += hits.
// total / count are the whole batch's (zeroed once per call) and sum over the
// snapshots of a namespace (disjoint docs).
// With fg_count_clauses a phrase or group clause of a slot is a
// ROW: one bitmap cbits[r * words .. + words) per distinct clause of the slice
// (zeroed per pass).  Two more kernels run, and k_cmatch keeps the slots without rows:
//   k_crow     after k_cfilter: work items (row, kCountChunk postings of a driver
//              list).  An any-of group drives every present member; an all-of
//              group its shortest member, the others probed (term_has_doc); a
//              phrase its rarest distinct term, the other distinct terms probed,
//              the survivors queued in LDS and verified one wave each against
//              fwd, then fwd_name (existence only);
//   k_cjoin    beside k_cmatch, for the slots that hold a row: k_cmatch's list
//              drivers (kCountText) and row drivers (kCountRow: (slot, row,
//              kCountWordChunk words), a lane per word) -- when the Musts are rows
//              only, and for every Should row.  A candidate is tested in the slot's
//              probed terms, its Must and MustNot rows and its filter row.
// (constants of their own, not the k_conj tuning macros: count.cpp is compiled once for every variant build)
constexpr uint32_t kCountItems = 8;                  // k_cmatch: driver postings per lane
constexpr uint32_t kCountChunk = kThreads * kCountItems;  // ... per work item (2048)
constexpr uint32_t kCountFacetChunk = kFmaskChunk;   // facet postings per k_cfilter / k_cfacet item
constexpr uint32_t kCountFacetItems = kCountFacetChunk / kThreads;  // ... per lane of k_cfacet (registers)
constexpr uint32_t kCountWordChunk = 2048;           // bitmap words per k_ccount workgroup / k_cmatch fill item
constexpr uint32_t kCountTile = 64;                  // k_cfacet: slots per LDS accumulation round
constexpr uint32_t kCountText = 0, kCountFacet = 1, kCountFill = 2;  // DevCount::w_kind
constexpr uint32_t kCountRow = 3;                                    // DevCount::j_kind: a row driver (k_cjoin)
constexpr uint32_t kRowAny = 0, kRowAll = 1, kRowPhrase = 2;         // row_pack kinds
// DevCount::row_m: bits 0-7 the row's probed terms, 8-15 a phrase's terms, 16-17 its kind
__host__ __device__ inline uint32_t row_pack(uint32_t kind, uint32_t probes, uint32_t n) { return probes | (n << 8) | (kind << 16); }
__host__ __device__ inline uint32_t row_probes(uint32_t rm) { return rm & 0xFFu; }
__host__ __device__ inline uint32_t row_phrase_terms(uint32_t rm) { return (rm >> 8) & 0xFFu; }
__host__ __device__ inline uint32_t row_kind(uint32_t rm) { return rm >> 16; }
struct DevCount {
  uint32_t nq;                  // slots of the slice
  uint32_t q0;                  // batch query of slot 0
  uint32_t words;               // ceil(N / 32)
  uint32_t n_count;
  uint32_t n_fchunks, n_items, n_cchunks;
  uint32_t* match;              // [nq * words] workspace, zeroed per pass
  uint32_t* fbits;              // [n_filters * words] workspace, zeroed per pass
  unsigned long long* total;    // [batch queries]
  unsigned long long* count;    // [batch queries * n_count]
  const uint32_t* fc_filter;    // [n_fchunks] k_cfilter item -> filter
  const uint32_t* fc_term;      // [n_fchunks] facet term
  const uint32_t* fc_start;     // [n_fchunks] first posting within the term's list
  const uint32_t* w_q;          // [n_items] k_cmatch item -> slot
  const uint32_t* w_kind;       // [n_items] kCountText / kCountFacet / kCountFill
  const uint32_t* w_term;       // [n_items] driver term (text or facet id of the snapshot); kCountFill: unused
  const uint32_t* w_start;      // [n_items] first posting within the driver list; kCountFill: first word
  const uint32_t* q_m;          // [nq] qm_pack(probed terms, of which Must, of which MustNot)
  const uint32_t* q_terms;      // [nq * kMaxTerms] probed terms: [other Musts][MustNots]
  const uint32_t* q_filter;     // [nq] the slot's filter (fbits row) or 0xFFFFFFFF
  const uint32_t* cc_j;         // [n_cchunks] k_cfacet item -> index in count_terms
  const uint32_t* cc_term;      // [n_cchunks] facet term
  const uint32_t* cc_start;     // [n_cchunks] first posting within the term's list
  // ---- clause rows (fg_count_clauses); n_ritems == n_jitems == 0 without one
  uint32_t n_ritems, n_jitems;
  uint32_t* cbits;              // [n_rows * words] workspace, zeroed per pass
  const uint32_t* r_row;        // [n_ritems] k_crow item -> row
  const uint32_t* r_term;       // [n_ritems] driver term (the snapshot's id)
  const uint32_t* r_start;      // [n_ritems] first posting within the driver list
  const uint32_t* row_m;        // [n_rows] row_pack(kind, probed terms, phrase terms)
  const uint32_t* row_terms;    // [n_rows * kMaxTerms] probed terms (the snapshot's ids): every one must hold the doc
  const uint32_t* row_pterm;    // [n_rows * kMaxTerms] a phrase's terms as VOCABULARY ids (DevIndex::fwd), anchor first
  const uint32_t* row_ppos;     // [n_rows * kMaxTerms] ... and their position offsets
  const uint32_t* j_q;          // [n_jitems] k_cjoin item -> slot
  const uint32_t* j_kind;       // [n_jitems] kCountText / kCountRow
  const uint32_t* j_term;       // [n_jitems] driver term, or driver row
  const uint32_t* j_start;      // [n_jitems] first posting within the driver list; kCountRow: first word
  const uint32_t* q_rm;         // [nq] tested rows | Must rows among them << 16
  const uint32_t* q_rows;       // [nq * kMaxTerms] tested rows: [Must rows][MustNot rows]
};

constexpr uint32_t kDiagPerWg = 16;  // u64 stamps per workgroup in diagnostic builds

// Key of a hit: larger is better.  (score bits << 32) | ~doc orders by
// score descending, then doc ascending (tantivy ComparableDoc order); scores
// are finite and >= 0 so the f32 bit pattern is order preserving.
__host__ __device__ inline uint64_t make_key(float score, uint32_t doc) {
  union { float f; uint32_t u; } c;
  c.f = score;
  return ((uint64_t)c.u << 32) | (uint64_t)(0xFFFFFFFFu - doc);
}
__host__ __device__ inline float key_score(uint64_t k) {
  union { float f; uint32_t u; } c;
  c.u = (uint32_t)(k >> 32);
  return c.f;
}
__host__ __device__ inline uint32_t key_doc(uint64_t k) { return 0xFFFFFFFFu - (uint32_t)k; }

// Bound tables of a snapshot build (k_score / k_bucket / k_tsub / k_ktop), run
// ONCE per segment build or merge: every posting's BM25 term score under the
// build's statistics (into a temporary), then the bounds the kernels prune with
// and the per-term K-th best scores.  A commit never runs them on an older
// segment (fg_index_rescore only scales them at query time: DevPlan::q_rup).
// Work is split into chunks of one term: k_score over postings, k_bucket over
// directory buckets; ch_* arrays are the chunk tables.
constexpr uint32_t kScoreChunk = kChunk;  // postings per k_score workgroup (= a k_conj lead chunk: cmax)
constexpr uint32_t kBucketChunk = 2048;  // buckets per k_bucket workgroup
static_assert(kScoreChunk == kChunk, "DevIndex::cmax: a k_score chunk is a k_conj lead chunk");
struct ScoreJob {
  const uint32_t* doc;
  const uint16_t* tfn;        // [P] DevIndex::tfn
  const uint16_t* tfn_name;   // [P] or nullptr
  const uint64_t* esc_pos;    // DevIndex::esc_pos / esc_tf
  const uint32_t* esc_tf;
  uint64_t n_esc;
  const uint64_t* off;        // [V+1]
  const uint32_t* dir;
  const uint32_t* dir_off;
  const uint32_t* tmeta;
  const uint32_t* toff;       // [V] tile-maxima offset or 0xFFFFFFFF
  const uint32_t* alive;      // bitset or nullptr
  const float* w_text;        // [V] idf * (1 + K1)
  const float* w_name;        // [V]
  const float* cache;         // [512] K1 * ((1 - B) + B * TABLE[id] / avgdl), text then name
  float* psc;                 // [P] out: the build's posting scores (a temporary, freed after the build)
  float* bmax;                // [D] out
  uint32_t* tmaxs;            // [V] out (f32 bits, zeroed first)
  uint32_t* tmax;             // [tiles] out (f32 bits, zeroed first)
  uint64_t* tsub;             // [tiles] out (k_tsub)
  const uint32_t* tterm;      // [tile-table terms] the term of each n_tiles + 1 tile entries, in toff order
  uint32_t n_tterm;           // tile-table terms
  uint32_t n_tiles;           // tiles per term (4096-doc k_disj tiles)
  float* ktop;                // [V * kNumTopK] out (zeroed first)
  float* ladder;              // [V * kNumLadderExtra] out (zeroed first) or nullptr: fg_index_term_ladder only
  float* cmax;               // [cmax entries] out: the largest score of each kChunk postings of a term
  const uint32_t* coff;       // [V] first cmax entry of each term
  // packed chunk tables (a chunk: terms [tf, tl], postings / directory entries
  // [e0, e1) of them; one long term's slice, or several whole short terms)
  const uint32_t* sc_tf;      // k_score chunks
  const uint32_t* sc_tl;
  const uint64_t* sc_e0;
  const uint64_t* sc_e1;
  const uint32_t* bk_tf;      // k_bucket chunks (global directory entries)
  const uint32_t* bk_tl;
  const uint32_t* bk_e0;
  const uint32_t* bk_e1;
  uint32_t n_terms;
  uint32_t grid_cap;          // at most this many workgroups per scoring launch (0: one per item)
  uint64_t n_dir;             // directory entries (dir_off of term n_terms)
  const uint32_t* kt_tiny;    // k_ktop_tiny: terms with 1..kKtopTiny postings (one wave each)
  uint32_t n_tiny;
  const uint32_t* kt_terms;   // k_ktop: terms with kKtopTiny+1..kKtopChunk postings
  // terms with more postings: k_ktop_part per chunk, then k_ktop_big per term
  const uint32_t* kb_terms;   // [n_big] the long terms
  const uint32_t* kb_chunk0;  // [n_big + 1] first chunk of each
  const uint32_t* kc_big;     // [n_chunks] long-term index of each chunk
  const uint32_t* kc_start;   // [n_chunks] first posting of each chunk within its term's list
  uint64_t* kc_keys;          // [n_chunks * kTopKs[last]] each chunk's best keys
  uint32_t* kc_cnt;           // [n_chunks]
  uint32_t* kb_stat;          // [3][n_big] alive postings, min / max alive score bits (0, ~0, 0 first)
  uint32_t n_big;
};
#ifndef FG_KTOP_CHUNK
#define FG_KTOP_CHUNK 32768
#endif
constexpr uint32_t kKtopChunk = FG_KTOP_CHUNK;  // postings per k_ktop_part workgroup (and k_ktop's largest term)
constexpr uint32_t kKtopTiny = 64;              // k_ktop_tiny: terms of at most this many postings, one wave each
constexpr uint32_t kPackTerms = 256;            // k_score / k_bucket: term ids per packed chunk

// The score tables of a build (k_dtab_fill / k_dtab_scatter): table i takes the
// scores psc[off[i] .. off[i] + df[i]) at their postings' docs.
struct DocTabJob {
  const uint32_t* doc;
  const float* psc;
  float* tab;
  uint64_t stride;  // floats per table
  uint32_t n;       // tables
  uint32_t df[kDocTabMax];
  uint64_t off[kDocTabMax];
};

// The bound tables of a build (k_dtab8_fill / k_dtab8_scatter): table i takes
// quant8(psc[off[i] + p], tmaxs[term[i]]) at the doc of posting p of its term.
struct DocTab8Job {
  const uint32_t* doc;
  const float* psc;
  const float* tmaxs;  // [V] the term maxima (k_bucket has run)
  uint8_t* tab;
  uint64_t stride;  // bytes per table (a multiple of 128)
  uint32_t n;       // tables
  uint32_t term[kDocTabMax];
  uint32_t df[kDocTabMax];
  uint64_t off[kDocTabMax];
};

// The score-tiered copies of a build (k_band_*): copy i takes the postings
// [off[i], off[i] + df[i]) of the snapshot into bdoc / bpsc at boff[i], its
// chunks are c0[i] .. c0[i + 1] of bcmax.  launch_band_hist fills hist (zeroed:
// kBandBins per copy) and the host cuts it (band_cuts -> lo); launch_band_copy
// counts every source chunk's postings per tier (cnt: per copy, tier-major),
// scans them into first positions, scatters and takes the copy's chunk maxima.
struct BandJob {
  const uint32_t* doc;
  const float* psc;
  uint32_t* bdoc;
  float* bpsc;
  float* bcmax;
  uint32_t* hist;   // [n * kBandBins] temporary, zeroed
  uint32_t* cnt;    // [n_chunks * kBandTiers] temporary
  uint32_t n;       // copies
  uint32_t n_chunks;
  uint32_t df[kBandMax];
  uint32_t c0[kBandMax + 1];
  uint64_t off[kBandMax];
  uint64_t boff[kBandMax];
  uint32_t lo[kBandMax][kBandTiers - 1];
};
hipError_t launch_band_hist(const BandJob& j, uint32_t grid_cap, hipStream_t s);
hipError_t launch_band_copy(const BandJob& j, uint32_t grid_cap, hipStream_t s);

// The forward index of ONE field from positional postings (fg_index_build_positional,
// DESIGN.md §13; k_fwd_*).  posting p of the snapshot (doc[p], CSR by term in off)
// owns tf[p] consecutive entries of pos from poff[p]: its token positions in the
// field of its doc.  launch_fwd_rows: poff = exclusive scan of tf, len[d] = the
// largest claimed position of doc d + 1, fwd_off = exclusive scan of len (its last
// entry, the row total, is what the host allocates fwd by).  launch_fwd_fill: fwd
// = kFwdNone everywhere, fwd[fwd_off[doc[p]] + x] = term(p) for every position x
// of every posting, and filled = the entries of fwd that are not kFwdNone.
// Invalid input sets bits of *err and stores nothing outside a row.
constexpr uint32_t kFwdSlices = 1024;  // G: slices of a scan (fugu.h FG_FWD_SCAN_SLICES)
constexpr uint32_t kFwdShort = 16;     // k_fwd_scatter: a posting of at most this many positions is one lane's loop
constexpr uint32_t kFwdErrOrder = 1u;  // a posting's positions do not strictly ascend
constexpr uint32_t kFwdErrNone = 2u;   // a position of kFwdNone
constexpr uint32_t kFwdErrRow = 4u;    // a position past its doc's row (after one of the above)
struct FwdJob {
  const uint32_t* doc;       // [P] DevIndex::doc
  const uint64_t* off;       // [V+1] DevIndex::off
  const uint16_t* tf;        // [P] the field's tf (a temporary)
  const uint32_t* pos;       // [n_pos] the field's positions in posting order (a temporary)
  uint64_t* poff;            // [P+1] temporary
  uint32_t* len;             // [N] temporary, zeroed
  uint64_t* part;            // [kFwdSlices + 1] temporary: a scan's slice sums, then their bases
  uint32_t* err;             // the error word, zeroed
  unsigned long long* filled;  // zeroed
  uint64_t* fwd_off;         // [N+1]
  uint32_t* fwd;             // [fwd_off[N]] (launch_fwd_fill)
  uint64_t n_fwd;            // fwd_off[N] (launch_fwd_fill)
  uint64_t n_post;           // P
  uint32_t n_docs;
  // k_score's packed chunks of the postings (ChunkTables): <= kScoreChunk postings of <= kPackTerms term ids each
  const uint32_t* sc_tf;
  const uint32_t* sc_tl;
  const uint64_t* sc_e0;
  const uint64_t* sc_e1;
  uint32_t n_chunks;
  uint32_t grid_cap;         // at most this many workgroups per launch (0: no cap)
};
// ev (or nullptr): 4 events each, recorded around launch_fwd_rows' three steps (the
// scan of tf, k_fwd_len, the scan of len: a scan's three kernels are one span) and
// around launch_fwd_fill's three kernels
hipError_t launch_fwd_rows(const FwdJob& j, hipStream_t s, hipEvent_t* ev = nullptr);
hipError_t launch_fwd_fill(const FwdJob& j, hipStream_t s, hipEvent_t* ev = nullptr);

// kernels.hip entry points (host-callable launchers)
hipError_t launch_conj(const DevIndex& ix, const DevPlan& pl, hipStream_t s);
// k_disj over the items [first, first + count) of the plan's k_disj range (in
// sweep order: the first part of every query's doc range first)
hipError_t launch_disj(const DevIndex& ix, const DevPlan& pl, hipStream_t s, uint32_t first = 0,
                       uint32_t count = 0xFFFFFFFFu);
hipError_t launch_fmask(const DevIndex& ix, const DevPlan& pl, hipStream_t s);
hipError_t launch_scan(const DevIndex& ix, const DevPlan& pl, hipStream_t s);
hipError_t launch_phrase(const DevIndex& ix, const DevPlan& pl, hipStream_t s);
hipError_t launch_bphrase(const DevIndex& ix, const DevPlan& pl, hipStream_t s);
hipError_t launch_group(const DevIndex& ix, const DevPlan& pl, hipStream_t s);
hipError_t launch_gphrase(const DevIndex& ix, const DevPlan& pl, hipStream_t s);
hipError_t launch_mgroup(const DevIndex& ix, const DevPlan& pl, hipStream_t s);
hipError_t launch_field(const DevIndex& ix, const DevPlan& pl, hipStream_t s);
hipError_t launch_fphrase(const DevIndex& ix, const DevPlan& pl, hipStream_t s);
// out_shard != nullptr: the merged select of a multi-snapshot plan (one list per batch query)
hipError_t launch_final(const DevPlan& pl, float* out_score, uint32_t* out_doc, uint32_t* out_n, hipStream_t s,
                        uint32_t* out_shard = nullptr);
// fg_count_batch's kernels of one pass, back to back on s (a kernel with no items is skipped): k_cfilter,
// k_crow, k_cmatch, k_cjoin, k_ccount, k_cfacet; ev: kCountEvents events recorded around them, or nullptr
// (ev[2] == ev[1] / ev[4] == ev[3]: one event for both slots, when k_crow / k_cjoin have no items)
constexpr uint32_t kCountEvents = 7;
hipError_t launch_count(const DevIndex& ix, const DevCount& c, hipStream_t s, hipEvent_t* ev = nullptr);
hipError_t launch_rank(const uint32_t* doc, const uint64_t* slot_base, const uint32_t* slot_n, uint32_t n_slots,
                       uint32_t n_words, uint64_t* out, hipStream_t s);
hipError_t launch_score(const ScoreJob& j, uint32_t n_chunks, hipStream_t s);
// the score tables of a build (DevIndex::dtab) from its posting scores: one fill pass, then one
// scatter over the chosen terms' postings
hipError_t launch_doctab(const DocTabJob& j, uint32_t grid_cap, hipStream_t s);
// the bound tables of a build (DevIndex::dtab8), after launch_bucket: one fill pass, one scatter
hipError_t launch_doctab8(const DocTab8Job& j, uint32_t grid_cap, hipStream_t s);
hipError_t launch_bucket(const ScoreJob& j, uint32_t n_chunks, uint32_t n_docs, hipStream_t s);  // packed chunks
hipError_t launch_tsub(const ScoreJob& j, uint32_t n_docs, hipStream_t s);                        // after k_bucket
hipError_t launch_ktop(const ScoreJob& j, uint32_t n_terms, uint32_t n_chunks, uint32_t n_big, hipStream_t s);
hipError_t launch_copy32(uint32_t* dst, const uint32_t* src, uint64_t n, uint32_t grid_cap, hipStream_t s);
hipError_t launch_merge(uint32_t n_shards, uint32_t n_queries, uint32_t k, const float* score, const uint32_t* doc,
                        const uint32_t* n, float* out_score, uint32_t* out_doc, uint32_t* out_shard, uint32_t* out_n,
                        hipStream_t s);

}  // namespace fg
