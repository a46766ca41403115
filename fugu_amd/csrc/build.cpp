// libfugu snapshot building: host postings from docs or postings, the
// statistics-independent structure and its upload (finish_index: a driver over
// named phases), the bound tables of a build (build_bounds), rescoring
// (rescore_one) and their C entry points of include/fugu.h.  Streams, pools,
// the statistics (set_stats / relate_stats) and everything about plans:
// fugu.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/fugu.h"
#include "fg_host.h"
#include "fg_internal.h"

namespace {

using fgh::dev_upload;
using fgh::fail;
using fgh::g_bt;
using fgh::hw_threads;
using fgh::parallel_dynamic;
using fgh::parallel_ranges;
using fgh::UploadBatch;
#define kBuildStream fgh::build_stream()

// Host-side postings before upload (merged text U name per term).
struct HostPostings {
  uint32_t n_docs = 0, n_terms = 0;
  std::vector<uint64_t> off;      // [V+1]
  std::vector<uint32_t> doc, tf;  // tf packed lo16 text / hi16 name
  std::vector<uint32_t> df_text, df_name;
  std::vector<uint8_t> fn_text, fn_name;
  std::vector<uint32_t> alive;    // bitset, empty when no deletes
  uint64_t tot[2] = {0, 0};
  bool has_name = false;
  // facet field: postings (docs only: IndexRecordOption::Basic) per facet term
  uint32_t n_fterms = 0;
  std::vector<uint64_t> foff{0};  // [VF+1]
  std::vector<uint32_t> fdoc;
  std::vector<uint32_t> df_facet;
  uint64_t tot_f = 0;             // total_num_tokens(facet), duplicates included
  uint64_t df(uint32_t t) const { return off[t + 1] - off[t]; }
};

// the alive bitset of `deleted` (NULL: empty, every doc alive)
std::vector<uint32_t> alive_from_deleted(const uint8_t* deleted, uint32_t N) {
  std::vector<uint32_t> alive;
  if (!deleted) return alive;
  alive.assign((N + 31) / 32, 0);
  for (uint32_t d = 0; d < N; ++d)
    if (!deleted[d]) alive[d >> 5] |= 1u << (d & 31);
  return alive;
}

// Parts of one device block, each rounded to 256 B (16 B at least)
struct Parts {
  struct P { size_t off = 0, bytes = 0; };
  size_t total = 0;
  P add(size_t bytes) {
    const P p{total, bytes};
    total += (std::max<size_t>(bytes, 16) + 255) & ~size_t(255);
    return p;
  }
  // the part's address in block `blk` (an empty part: nullptr)
  template <class T>
  static T* at(void* blk, P p) { return p.bytes ? reinterpret_cast<T*>(static_cast<char*>(blk) + p.off) : nullptr; }
};

// a stream-ordered temporary freed on the build stream at scope exit (freeing
// it does not synchronize the device: searches on other streams keep running)
struct AsyncTmp {
  void* p = nullptr;
  ~AsyncTmp() { if (p) (void)hipFreeAsync(p, kBuildStream); }
};

// the structure's chunk tables into a scoring job
void score_job_tables(const fgh::ChunkTables& c, fg::ScoreJob& j) {
  j.sc_tf = c.d_sc_tf;
  j.sc_tl = c.d_sc_tl;
  j.sc_e0 = c.d_sc_e0;
  j.sc_e1 = c.d_sc_e1;
  j.bk_tf = c.d_bk_tf;
  j.bk_tl = c.d_bk_tl;
  j.bk_e0 = c.d_bk_e0;
  j.bk_e1 = c.d_bk_e1;
  j.tterm = c.d_tterm;
  j.n_tterm = c.n_tterm;
  j.n_tiles = c.n_tiles;
  j.kt_tiny = c.d_kt_tiny;
  j.n_tiny = c.n_ktiny;
  j.kt_terms = c.d_kt_terms;
  j.kb_terms = c.d_kb_terms;
  j.kb_chunk0 = c.d_kb_chunk0;
  j.kc_big = c.d_kc_big;
  j.kc_start = c.d_kc_start;
  j.n_big = c.n_kbig;
}

// k_ktop over the build's scores (j.psc, j.alive -> j.ktop, and j.ladder when
// set; j's tables: score_postings): terms of <= kKtopChunk postings one
// workgroup each; longer terms in kKtopChunk-posting chunks (k_ktop_part), then
// one select per term over its chunks' best keys (k_ktop_big).  The key scratch
// is one stream-ordered temporary.
int ktop_pass(const fg_index* ix, fg::ScoreJob& j) {
  const size_t n_small = ix->n_kt, n_big = ix->n_kbig, n_chunks = ix->n_kchunks;
  const size_t kck_b = (8ull * n_chunks * fg::kTopKs[fg::kNumTopK - 1] + 255) & ~size_t(255);
  const size_t kcc_b = (4ull * n_chunks + 255) & ~size_t(255), kbs_b = 4ull * 3 * n_big;
  AsyncTmp ktmp;
  if (fgh::dev_malloc_async(&ktmp.p, kck_b + kcc_b + kbs_b + 16, kBuildStream) != hipSuccess)
    return fail(FG_EOOM, "hipMallocAsync(%zu) failed", kck_b + kcc_b + kbs_b);
  char* kb = static_cast<char*>(ktmp.p);
  uint32_t* d_kbs = reinterpret_cast<uint32_t*>(kb + kck_b + kcc_b);
  // per long term: alive postings 0, min alive score bits ~0, max 0 ([3][n_big])
  if (n_big) {
    HIPCHK(hipMemsetAsync(d_kbs, 0, 4ull * 3 * n_big, kBuildStream));
    HIPCHK(hipMemsetD32Async(d_kbs + n_big, (int)0xFFFFFFFFu, n_big, kBuildStream));
  }
  j.kc_keys = reinterpret_cast<uint64_t*>(kb);
  j.kc_cnt = reinterpret_cast<uint32_t*>(kb + kck_b);
  j.kb_stat = d_kbs;
  HIPCHK(fg::launch_ktop(j, (uint32_t)n_small, (uint32_t)n_chunks, (uint32_t)n_big, kBuildStream));
  return FG_OK;
}

// Every posting's score under the snapshot's CURRENT statistics (k_score) into
// `psc` (a build's bound block) or a stream-ordered temporary, for the bound
// kernels of a build and for fg_index_term_ladder.  `tmp` gets the temporary;
// j gets the postings inputs, the structure's chunk tables, the weights and
// caches (inside tmp) and j.psc / j.cmax (cmax: the caller's, or a scratch part
// of tmp).
int score_postings(const fg_index* ix, fg::ScoreJob& j, float* cmax, float* psc, AsyncTmp& tmp) {
  const uint32_t V = ix->n_terms;
  Parts L;
  const Parts::P p_psc = psc ? Parts::P{} : L.add(4ull * ix->n_postings + 16), p_wt = L.add(4ull * V),
                 p_wn = L.add(4ull * V), p_c = L.add(4ull * 512), p_cm = cmax ? Parts::P{} : L.add(4ull * ix->n_sc);
  if (fgh::dev_malloc_async(&tmp.p, L.total, kBuildStream) != hipSuccess)
    return fail(FG_EOOM, "hipMallocAsync(%zu) failed", L.total);
  char* t = static_cast<char*>(tmp.p);
  float* d_wt = reinterpret_cast<float*>(t + p_wt.off);
  float* d_wn = reinterpret_cast<float*>(t + p_wn.off);
  float* d_cache = reinterpret_cast<float*>(t + p_c.off);
  HIPCHK(hipMemcpyAsync(d_wt, ix->w_text.data(), 4ull * V, hipMemcpyHostToDevice, kBuildStream));
  HIPCHK(hipMemcpyAsync(d_wn, ix->w_name.data(), 4ull * V, hipMemcpyHostToDevice, kBuildStream));
  HIPCHK(hipMemcpyAsync(d_cache, ix->cache, 4ull * 512, hipMemcpyHostToDevice, kBuildStream));
  j.doc = ix->d.doc;
  j.tfn = ix->d.tfn;
  j.tfn_name = ix->d.tfn_name;
  j.esc_pos = ix->d.esc_pos;
  j.esc_tf = ix->d.esc_tf;
  j.n_esc = ix->d.n_esc;
  j.off = ix->d.off;
  j.dir = ix->d.dir;
  j.dir_off = ix->d.dir_off;
  j.tmeta = ix->d.tmeta;
  j.toff = ix->d.toff;
  j.w_text = d_wt;
  j.w_name = d_wn;
  j.cache = d_cache;
  j.psc = psc ? psc : reinterpret_cast<float*>(t + p_psc.off);
  j.cmax = cmax ? cmax : reinterpret_cast<float*>(t + p_cm.off);
  j.coff = ix->d.coff;
  score_job_tables(*ix, j);
  j.n_terms = V;
  j.grid_cap = fgh::bg_grid_cap(ix->dev);
  HIPCHK(fg::launch_score(j, ix->n_scb, kBuildStream));
  return FG_OK;
}

// The terms that get a doc-indexed score table (DevIndex::dtab): df >= N /
// FUGU_DOCTAB_DIV (default kDocTabDiv; 0: none), densest first (ties by term
// id), at most kDocTabMax and within 1/kDocTabFrac of the snapshot's own
// posting bytes (12 B each, as the rank budget counts them), so a small shard
// or namespace pays in proportion.  None for a snapshot of fewer than
// kDocTabMinDocs docs, or one whose table would not fit a buffer resource.
// The one-byte bound tables (DevIndex::dtab8) are chosen the same way: env
// FUGU_DOCTAB8_DIV (default kDocTab8Div), eb = 1 byte per doc.
std::vector<uint32_t> choose_doctab_terms(const fg_index* ix, uint64_t stride, const char* env = "FUGU_DOCTAB_DIV",
                                          uint32_t div = fg::kDocTabDiv, uint64_t eb = 4) {
  std::vector<uint32_t> ts;
  const uint64_t N = ix->n_docs;
  if (const char* e = getenv(env))
    if (*e) div = (uint32_t)std::max(0l, atol(e));
  if (!div || N < fg::kDocTabMinDocs || 4 * N > fg::kPdMaxBytes || !stride) return ts;
  auto df = [&](uint32_t t) { return ix->off[t + 1] - ix->off[t]; };
  for (uint32_t t = 0; t < ix->n_terms; ++t)
    if (df(t) * div >= N) ts.push_back(t);
  std::stable_sort(ts.begin(), ts.end(), [&](uint32_t a, uint32_t b) { return df(a) > df(b); });
  const uint64_t budget = 12ull * ix->n_postings / fg::kDocTabFrac;
  ts.resize(std::min<uint64_t>({(uint64_t)ts.size(), (uint64_t)fg::kDocTabMax, budget / (eb * stride)}));
  return ts;
}

// The terms that get a score-tiered lead copy (DevIndex::bdoc / bpsc / bcmax):
// df >= N / FUGU_BAND_DIV (default kBandDiv; 0: none) in a snapshot of >=
// FUGU_BAND_MIN_DOCS docs (default kBandMinDocs), densest first (ties by term
// id), at most kBandMax and within 1/FUGU_BAND_FRAC (default kBandFrac; 0: no
// cap) of the snapshot's posting bytes (12 B each; a copy takes 8 B per posting).
std::vector<uint32_t> choose_band_terms(const fg_index* ix) {
  std::vector<uint32_t> ts;
  const uint64_t N = ix->n_docs;
  uint32_t div = fg::kBandDiv;
  uint64_t min_docs = fg::kBandMinDocs, frac = fg::kBandFrac;
  if (const char* e = getenv("FUGU_BAND_DIV"))
    if (*e) div = (uint32_t)std::max(0l, atol(e));
  if (const char* e = getenv("FUGU_BAND_MIN_DOCS"))
    if (*e) min_docs = (uint64_t)std::max(0l, atol(e));
  if (const char* e = getenv("FUGU_BAND_FRAC"))
    if (*e) frac = (uint64_t)std::max(0l, atol(e));
  if (!div || N < min_docs) return ts;
  auto df = [&](uint32_t t) { return ix->off[t + 1] - ix->off[t]; };
  for (uint32_t t = 0; t < ix->n_terms; ++t)
    if (df(t) && df(t) * div >= N && df(t) < 0x80000000ull) ts.push_back(t);
  std::stable_sort(ts.begin(), ts.end(), [&](uint32_t a, uint32_t b) { return df(a) > df(b); });
  if (ts.size() > fg::kBandMax) ts.resize(fg::kBandMax);
  uint64_t left = frac ? 12ull * ix->n_postings / frac : ~0ull;
  size_t n = 0;
  while (n < ts.size() && 8 * df(ts[n]) <= left) left -= 8 * df(ts[n++]);
  ts.resize(n);
  return ts;
}

// The tiered copies of `terms` from the build's scores: histograms, the host's
// cuts, then the stable partition and the copies' chunk maxima (BandJob).
int build_bands(fg_index* ix, const std::vector<uint32_t>& terms, const float* d_psc, uint32_t* d_bdoc, float* d_bpsc,
                float* d_bcmax, uint32_t grid_cap) {
  fg::BandJob bj{};
  bj.doc = ix->d.doc;
  bj.psc = d_psc;
  bj.bdoc = d_bdoc;
  bj.bpsc = d_bpsc;
  bj.bcmax = d_bcmax;
  bj.n = (uint32_t)terms.size();
  std::vector<uint64_t> map(terms.size()), boffs(terms.size());
  std::vector<uint32_t> c0s(terms.size());
  uint64_t boff = 0;
  for (uint32_t i = 0; i < terms.size(); ++i) {
    const uint64_t df = ix->off[terms[i] + 1] - ix->off[terms[i]];
    bj.df[i] = (uint32_t)df;
    bj.off[i] = ix->off[terms[i]];
    bj.boff[i] = boffs[i] = boff;
    c0s[i] = bj.c0[i];
    bj.c0[i + 1] = bj.c0[i] + (uint32_t)((df + fg::kChunk - 1) / fg::kChunk);
    boff += df;
    map[i] = ((uint64_t)terms[i] << 32) | i;
  }
  bj.n_chunks = bj.c0[bj.n];
  const size_t hist_b = 4ull * fg::kBandBins * bj.n, cnt_b = 4ull * fg::kBandTiers * bj.n_chunks;
  AsyncTmp tmp;
  if (fgh::dev_malloc_async(&tmp.p, hist_b + cnt_b + 16, kBuildStream) != hipSuccess)
    return fail(FG_EOOM, "hipMallocAsync(%zu) failed", hist_b + cnt_b);
  bj.hist = static_cast<uint32_t*>(tmp.p);
  bj.cnt = bj.hist + (size_t)fg::kBandBins * bj.n;
  HIPCHK(hipMemsetAsync(bj.hist, 0, hist_b, kBuildStream));
  HIPCHK(fg::launch_band_hist(bj, grid_cap, kBuildStream));
  std::vector<uint32_t> h((size_t)fg::kBandBins * bj.n), lo((size_t)(fg::kBandTiers - 1) * bj.n);
  HIPCHK(hipMemcpyAsync(h.data(), bj.hist, hist_b, hipMemcpyDeviceToHost, kBuildStream));
  HIPCHK(hipStreamSynchronize(kBuildStream));
  // FUGU_BAND_SHARES=a:b:c:d (or commas): other cumulative tier shares, in sixteenths, ascending
  uint32_t shares[fg::kBandTiers - 1];
  std::copy(fg::kBandShares, fg::kBandShares + fg::kBandTiers - 1, shares);
  if (const char* e = getenv("FUGU_BAND_SHARES")) {
    unsigned a[4];
    if (sscanf(e, "%u%*[,:]%u%*[,:]%u%*[,:]%u", &a[0], &a[1], &a[2], &a[3]) == 4 && a[0] >= 1 && a[0] <= a[1] && a[1] <= a[2] &&
        a[2] <= a[3] && a[3] <= fg::kBandShareDen)
      std::copy(a, a + 4, shares);
  }
  for (uint32_t i = 0; i < bj.n; ++i) {
    fg::band_cuts(h.data() + (size_t)i * fg::kBandBins, bj.df[i], bj.lo[i], shares);
    std::copy(bj.lo[i], bj.lo[i] + fg::kBandTiers - 1, lo.begin() + (size_t)i * (fg::kBandTiers - 1));
  }
  HIPCHK(fg::launch_band_copy(bj, grid_cap, kBuildStream));
  std::sort(map.begin(), map.end());
  ix->band_map = std::move(map);
  ix->band_off = std::move(boffs);
  ix->band_c0 = std::move(c0s);
  ix->band_lo = std::move(lo);
  return FG_OK;
}

// The bounds of a freshly built structure under its build statistics (which
// are its current ones): the posting scores (k_score, with the block-max per
// 2048 postings), bucket / term / tile maxima (k_bucket), sub-tile maxima
// (k_tsub), per-term K-th best alive scores (k_ktop), and the read-back of
// tmaxs / ktop for the planner.  Once per build or merge: a commit's rescores of
// older segments share them (rescore_one).
int build_bounds(fg_index* ix, const std::vector<uint32_t>& alive) {
  const uint32_t V = ix->n_terms;
  HIPCHK(hipSetDevice(ix->dev));
  Parts L;
  const Parts::P p_psc = L.add(4ull * ix->n_postings + 16);  // 16 B of slack after the scores
  const Parts::P p_alive = L.add(4ull * alive.size()), p_bmax = L.add(4ull * ix->dir_entries), p_tmaxs = L.add(4ull * V),
                 p_tmax = L.add(4ull * ix->tile_entries), p_ktop = L.add(4ull * V * fg::kNumTopK),
                 p_cmax = L.add(4ull * ix->n_sc), p_tsub = L.add(8ull * ix->tile_entries);
  // the score tables last: a block without them is the same block cut short
  const uint64_t tab_stride = ((uint64_t)ix->n_docs + 31) & ~31ull;
  std::vector<uint32_t> tabs = choose_doctab_terms(ix, tab_stride);
  const size_t bounds_total = L.total;
  // (a kind with no table takes no part: not even an empty part's alignment slot)
  const Parts::P p_dtab = tabs.empty() ? Parts::P{} : L.add(4ull * tab_stride * tabs.size());
  // ... then the one-byte bound tables, the same way (FUGU_DOCTAB_DIV=0 leaves these)
  const uint64_t tab8_stride = ((uint64_t)ix->n_docs + 127) & ~127ull;
  std::vector<uint32_t> tabs8 = choose_doctab_terms(ix, tab8_stride, "FUGU_DOCTAB8_DIV", fg::kDocTab8Div, 1);
  const Parts::P p_dtab8 = tabs8.empty() ? Parts::P{} : L.add(tab8_stride * tabs8.size());
  // ... then the densest terms' score-tiered lead copies
  std::vector<uint32_t> bands = choose_band_terms(ix);
  uint64_t band_post = 0, band_chunks = 0;
  for (uint32_t t : bands) {
    const uint64_t df = ix->off[t + 1] - ix->off[t];
    band_post += df;
    band_chunks += (df + fg::kChunk - 1) / fg::kChunk;
  }
  const Parts::P p_bdoc = bands.empty() ? Parts::P{} : L.add(4 * band_post), p_bpsc = bands.empty() ? Parts::P{} : L.add(4 * band_post),
                 p_bcmax = bands.empty() ? Parts::P{} : L.add(4 * band_chunks);
  size_t total = L.total;
  if (!ix->spool) {
    ix->spool = std::make_shared<fgh::ScorePool>();
    ix->spool->dev = ix->dev;
  }
  auto sb = std::make_shared<fgh::ScoreBlock>();
  void* blk = ix->spool->get(total);
  if (!blk && !(tabs.empty() && tabs8.empty() && bands.empty())) {  // (a build never fails for want of the tables)
    (void)hipGetLastError();
    tabs.clear();
    tabs8.clear();
    bands.clear();
    total = bounds_total;
    blk = ix->spool->get(total);
  }
  if (!blk) return fail(FG_EOOM, "bound tables: hipMalloc(%zu) failed", total);
  sb->p = blk;
  sb->bytes = total;
  sb->pool = ix->spool;
  ix->sblock = sb;
  float *d_psc = Parts::at<float>(blk, p_psc), *d_bmax = Parts::at<float>(blk, p_bmax),
        *d_ktop = Parts::at<float>(blk, p_ktop), *d_cmax = Parts::at<float>(blk, p_cmax);
  uint32_t *d_alive = Parts::at<uint32_t>(blk, p_alive), *d_tmaxs = Parts::at<uint32_t>(blk, p_tmaxs),
           *d_tmax = Parts::at<uint32_t>(blk, p_tmax);
  uint64_t* d_tsub = Parts::at<uint64_t>(blk, p_tsub);
  if (d_alive) HIPCHK(hipMemcpyAsync(d_alive, alive.data(), 4ull * alive.size(), hipMemcpyHostToDevice, kBuildStream));
  HIPCHK(hipMemsetAsync(d_tmaxs, 0, 4ull * V, kBuildStream));
  HIPCHK(hipMemsetAsync(d_tmax, 0, std::max<size_t>(4ull * ix->tile_entries, 16), kBuildStream));
  HIPCHK(hipMemsetAsync(d_ktop, 0, 4ull * V * fg::kNumTopK, kBuildStream));
  g_bt.mark("bound tables + uploads");
  fg::ScoreJob j{};
  AsyncTmp tmp;
  if (int rc = score_postings(ix, j, d_cmax, d_psc, tmp)) return rc;
  // the densest terms' score tables from those scores (none: no launch)
  float* d_dtab = tabs.empty() ? nullptr : Parts::at<float>(blk, p_dtab);
  if (d_dtab) {
    fg::DocTabJob tj{};
    tj.doc = ix->d.doc;
    tj.psc = d_psc;
    tj.tab = d_dtab;
    tj.stride = tab_stride;
    tj.n = (uint32_t)tabs.size();
    std::vector<uint64_t> map(tabs.size());
    for (uint32_t i = 0; i < tabs.size(); ++i) {
      tj.off[i] = ix->off[tabs[i]];
      tj.df[i] = (uint32_t)(ix->off[tabs[i] + 1] - ix->off[tabs[i]]);
      map[i] = ((uint64_t)tabs[i] << 32) | i;
    }
    HIPCHK(fg::launch_doctab(tj, j.grid_cap, kBuildStream));
    std::sort(map.begin(), map.end());
    ix->dtab_map = std::move(map);
  }
  ix->dtab_bytes = 4ull * tab_stride * tabs.size();
  if (g_bt.on)
    fprintf(stderr, "[fg build] score tables: %zu terms, %.1f MiB\n", tabs.size(), (double)ix->dtab_bytes / (double)(1 << 20));
  uint32_t* d_bdoc = bands.empty() ? nullptr : Parts::at<uint32_t>(blk, p_bdoc);
  float *d_bpsc = bands.empty() ? nullptr : Parts::at<float>(blk, p_bpsc),
        *d_bcmax = bands.empty() ? nullptr : Parts::at<float>(blk, p_bcmax);
  if (d_bdoc)
    if (int rc = build_bands(ix, bands, d_psc, d_bdoc, d_bpsc, d_bcmax, j.grid_cap)) return rc;
  ix->band_bytes = bands.empty() ? 0 : 8 * band_post + 4 * band_chunks;
  if (g_bt.on)
    fprintf(stderr, "[fg build] tiered lead copies: %zu terms, %.1f MiB\n", bands.size(), (double)ix->band_bytes / (double)(1 << 20));
  j.alive = d_alive;
  j.bmax = d_bmax;
  j.tmaxs = d_tmaxs;
  j.tmax = d_tmax;
  j.ktop = d_ktop;
  j.n_dir = ix->dir_entries;
  HIPCHK(fg::launch_bucket(j, ix->n_bk, ix->n_docs, kBuildStream));
  // the dense terms' bound tables: each score quantized up against its term's
  // maximum, which k_bucket has just written (none: no launch)
  uint8_t* d_dtab8 = tabs8.empty() ? nullptr : Parts::at<uint8_t>(blk, p_dtab8);
  if (d_dtab8) {
    fg::DocTab8Job tj{};
    tj.doc = ix->d.doc;
    tj.psc = d_psc;
    tj.tmaxs = reinterpret_cast<const float*>(d_tmaxs);
    tj.tab = d_dtab8;
    tj.stride = tab8_stride;
    tj.n = (uint32_t)tabs8.size();
    std::vector<uint64_t> map(tabs8.size());
    for (uint32_t i = 0; i < tabs8.size(); ++i) {
      tj.term[i] = tabs8[i];
      tj.off[i] = ix->off[tabs8[i]];
      tj.df[i] = (uint32_t)(ix->off[tabs8[i] + 1] - ix->off[tabs8[i]]);
      map[i] = ((uint64_t)tabs8[i] << 32) | i;
    }
    HIPCHK(fg::launch_doctab8(tj, j.grid_cap, kBuildStream));
    std::sort(map.begin(), map.end());
    ix->dtab8_map = std::move(map);
  }
  ix->dtab8_bytes = tab8_stride * tabs8.size();
  if (g_bt.on)
    fprintf(stderr, "[fg build] bound tables: %zu terms, %.1f MiB\n", tabs8.size(), (double)ix->dtab8_bytes / (double)(1 << 20));
  j.tsub = d_tsub;
  HIPCHK(fg::launch_tsub(j, ix->n_docs, kBuildStream));
  if (int rc = ktop_pass(ix, j)) return rc;
  g_bt.mark("bound launches");
  // tmaxs [V] then ktop [V * kNumTopK], read straight into a pooled pinned block
  {
    const size_t hb = 4ull * V * (1 + fg::kNumTopK);
    float* h = static_cast<float*>(ix->spool->get_host(hb));
    if (h) {
      sb->hp = h;
      sb->hbytes = hb;
    } else {
      sb->hown.resize((size_t)V * (1 + fg::kNumTopK));
      h = sb->hown.data();
    }
    if (fgh::on_background() && sb->hp) {
      // a background build: the read-back as a copy kernel of short workgroups
      // on its low-priority stream (pinned host memory is device-visible), not a
      // copy-engine transfer (those held searches up: tools/rescore_stall.py)
      HIPCHK(fg::launch_copy32(reinterpret_cast<uint32_t*>(h), d_tmaxs, V, j.grid_cap, kBuildStream));
      HIPCHK(fg::launch_copy32(reinterpret_cast<uint32_t*>(h + V), reinterpret_cast<const uint32_t*>(d_ktop),
                               (uint64_t)V * fg::kNumTopK, j.grid_cap, kBuildStream));
    } else {
      HIPCHK(hipMemcpyAsync(h, d_tmaxs, 4ull * V, hipMemcpyDeviceToHost, kBuildStream));
      HIPCHK(hipMemcpyAsync(h + V, d_ktop, 4ull * V * fg::kNumTopK, hipMemcpyDeviceToHost, kBuildStream));
    }
    HIPCHK(hipStreamSynchronize(kBuildStream));
    ix->tmaxs = h;
    ix->ktop = h + V;
  }
  g_bt.mark("device bounds");
  // the build's statistics are the bounds' reference
  ix->wb_text = ix->w_text;
  ix->wb_name = ix->w_name;
  std::memcpy(ix->cache_b, ix->cache, sizeof ix->cache);
  ix->h_alive = alive;
  ix->h_alive_b = ix->h_alive;
  ix->n_dead = 0;
  fgh::relate_stats(ix);
  ix->d.psc = d_psc;
  ix->d.bmax = d_bmax;
  ix->d.tmaxs = reinterpret_cast<const float*>(d_tmaxs);
  ix->d.tmax = reinterpret_cast<const float*>(d_tmax);
  ix->d.tsub = d_tsub;
  ix->d.cmax = d_cmax;
  ix->d.dtab = d_dtab;
  ix->d.dtab_stride = (uint32_t)tab_stride;
  ix->d.dtab8 = d_dtab8;
  ix->d.dtab8_stride = (uint32_t)tab8_stride;
  ix->d.bdoc = d_bdoc;
  ix->d.bpsc = d_bpsc;
  ix->d.bcmax = d_bcmax;
  ix->d.alive = d_alive;
  ix->device_bytes = ix->struct_bytes + total;
  return FG_OK;
}

// ---------------------------------------------------------------- the structure
// The statistics-independent half of a snapshot (postings, tf, fieldnorm ids,
// bucket directory, rank words, facet postings, chunk tables): host tables that
// the phases below fill from the postings and upload_structure consumes.
struct StructTables {
  std::vector<uint32_t> dir, dir_off, tmeta;  // bucket_directory
  uint64_t n_dir = 0;                         // dir.size() (dir is freed after the upload)
  std::vector<uint32_t> toff, tdir, tterm;    // tile_directory
  uint64_t n_tiles = 0, n_tile_entries = 0;   // tiles per term; tdir.size()
  // chunk_tables: k_score / k_bucket chunks, block-max offsets, k_ktop's term classes
  std::vector<uint32_t> sc_tf, sc_tl, bk_tf, bk_tl, bk_e0, bk_e1;
  std::vector<uint64_t> sc_e0, sc_e1;
  std::vector<uint32_t> coff, kt, kt_tiny, kb_terms, kb_chunk0, kc_big, kc_start;
  uint32_t n_cmax = 0;
  // pack_payloads
  std::vector<uint16_t> tfn, tfn_name;
  std::vector<uint64_t> esc_pos;
  std::vector<uint32_t> esc_tf;
};

// doc -> position bucket directory (fg_internal.h DevIndex): bucket width
// 2^B_t docs with B_t the largest shift keeping ~kBucketTarget postings per
// bucket.  hp -> st.dir, dir_off, tmeta (B_t | S_t << 8: 2^S_t > the largest bucket).
int bucket_directory(const HostPostings& hp, StructTables& st) {
  const uint64_t N = hp.n_docs;
  const uint32_t V = hp.n_terms;
  std::vector<uint32_t>&dir = st.dir, &dir_off = st.dir_off, &tmeta = st.tmeta;
  dir_off.resize(V);
  tmeta.resize(V);
  uint64_t nd = 0;
  for (uint32_t t = 0; t < V; ++t) {
    const uint64_t n = hp.df(t);
    uint32_t B = 0;
    if (n == 0) B = 31;
    else while (B < 31 && (n << (B + 1)) <= (uint64_t)fg::kBucketTarget * N) ++B;
    const uint64_t nbk = ((N - 1) >> B) + 1;
    if (nd > 0xFFFFFFFFull) return fail(FG_EINVAL, "directory too large");
    dir_off[t] = (uint32_t)nd;
    tmeta[t] = B;
    nd += nbk + 1;
  }
  dir.resize(nd);
  st.n_dir = nd;
  // term ranges of about equal work (postings + a per-term constant): a million
  // mostly empty terms of a small segment cost one range grab per range, not
  // one per term, and the densest terms still spread over the threads
  std::vector<uint32_t> cuts{0};
  {
    const int nth = hw_threads(0);
    const uint64_t tot = hp.off[V] + 64ull * V, step = std::max<uint64_t>(1, tot / (uint64_t)(nth * 16));
    uint64_t acc = 0;
    for (uint32_t t = 0; t < V; ++t) {
      acc += hp.df(t) + 64;
      if (acc >= step) { cuts.push_back(t + 1); acc = 0; }
    }
    if (cuts.back() != V) cuts.push_back(V);
  }
  parallel_dynamic((uint32_t)cuts.size() - 1, hw_threads(0), 1, [&](int, uint32_t rb, uint32_t re) {
    for (uint32_t t = cuts[rb]; t < cuts[re]; ++t) {
      const uint64_t b0 = hp.off[t], n = hp.off[t + 1] - b0;
      const uint32_t B = tmeta[t];
      const uint64_t nbk = ((N - 1) >> B) + 1;
      uint32_t* dt = dir.data() + dir_off[t];
      uint64_t p = 0;
      uint32_t maxocc = 0;
      for (uint64_t b = 0; b <= nbk; ++b) {
        const uint64_t lo = b << B;
        const uint64_t p0 = p;
        while (p < n && hp.doc[b0 + p] < lo) ++p;
        dt[b] = (uint32_t)p;
        if (b) maxocc = std::max<uint32_t>(maxocc, (uint32_t)(p - p0));
      }
      uint32_t S = 0;
      while ((1ull << S) <= maxocc) ++S;  // 2^S > largest bucket
      tmeta[t] = B | (S << 8);
    }
  });
  return FG_OK;
}

// per-term tile maxima (4096-doc tiles of k_disj) for terms whose buckets are
// no wider than a tile: one load gives a clause's bound over a tile; and the
// tile directory beside them: tdir[toff + i] = the first posting of tile i
// (n_tiles + 1 entries per term, the last = df), so a tile's posting range
// is two adjacent loads -- 32 tiles per line, where the bucket directory puts
// a dense term's consecutive tile boundaries 4096 >> B_t entries apart.
// hp, st.dir / dir_off / tmeta -> st.toff, tdir, tterm (the tile-table terms in
// toff order: k_tsub)
void tile_directory(const HostPostings& hp, StructTables& st) {
  const uint64_t N = hp.n_docs;
  const uint32_t V = hp.n_terms;
  std::vector<uint32_t>&toff = st.toff, &tdir = st.tdir;
  toff.assign(V, 0xFFFFFFFFu);
  const uint64_t n_tiles = ((uint64_t)N + (1u << fg::kDisjTileShift) - 1) >> fg::kDisjTileShift;
  uint64_t ntm = 0;
  for (uint32_t t = 0; t < V; ++t)
    if ((st.tmeta[t] & 0xFFu) <= fg::kDisjTileShift && hp.df(t) > 0) {
      if (ntm + n_tiles + 1 > 0xFFFFFFFFull) break;
      toff[t] = (uint32_t)ntm;
      ntm += n_tiles + 1;
    }
  tdir.resize(ntm);
  st.n_tiles = n_tiles;
  st.n_tile_entries = ntm;
  st.tterm.reserve(ntm / (n_tiles + 1));
  for (uint32_t t = 0; t < V; ++t)
    if (toff[t] != 0xFFFFFFFFu) st.tterm.push_back(t);
  parallel_dynamic(V, hw_threads(0), 64, [&](int, uint32_t tb, uint32_t te) {
    for (uint32_t t = tb; t < te; ++t) {
      if (toff[t] == 0xFFFFFFFFu) continue;
      const uint32_t B = st.tmeta[t] & 0xFFu;
      const uint64_t nbk = ((N - 1) >> B) + 1;
      const uint32_t* dt = st.dir.data() + st.dir_off[t];
      for (uint64_t i = 0; i <= n_tiles; ++i)
        tdir[toff[t] + i] = dt[std::min<uint64_t>(i << (fg::kDisjTileShift - B), nbk)];
    }
  });
}

// PACKED chunks of a scoring kernel over terms [0, V), term t owning entries
// [off(t), off(t + 1)): a term of >= long_from entries in slices of `slice`
// entries, or several whole short terms together (<= kPackTerms term ids, <= a
// slice's entries) -- the long tail of a vocabulary in a workgroup per term was
// most of a small segment's scoring time.  Chunk c: terms [tf[c], tl[c]],
// entries [e0[c], e1[c]).
template <class O, class Off>
void pack_chunks(uint32_t V, Off off, O slice, O long_from, std::vector<uint32_t>& tf, std::vector<uint32_t>& tl,
                 std::vector<O>& e0, std::vector<O>& e1) {
  uint32_t pt0 = 0;  // the pack [pt0, t) stays open while short terms fit
  O pe0 = 0;
  bool open = false;
  auto flush = [&](uint32_t t_end) {  // terms [pt0, t_end)
    if (!open) return;
    tf.push_back(pt0);
    tl.push_back(t_end - 1);
    e0.push_back(pe0);
    e1.push_back(off(t_end));
    open = false;
  };
  for (uint32_t t = 0; t < V; ++t) {
    const O b = off(t), n = off(t + 1) - b;
    if (n >= long_from) {
      flush(t);
      for (O f = 0; f < n; f += slice) {
        tf.push_back(t);
        tl.push_back(t);
        e0.push_back(b + f);
        e1.push_back(b + std::min<O>(n, f + slice));
      }
      continue;
    }
    if (open && (off(t + 1) - pe0 > slice || t - pt0 >= fg::kPackTerms)) flush(t);
    if (!open) {
      pt0 = t;
      pe0 = b;
      open = true;
    }
  }
  flush(V);
}

// chunk tables of the scoring kernels (they depend on the postings only, so
// every rescore reuses them): k_score chunks over the postings (sc_*), k_bucket
// chunks over the directory entries (bk_*: each term's buckets + its end entry),
// each term's first block-max entry (coff; DevIndex::cmax: kChunk postings each)
// and k_ktop's term classes: <= kKtopTiny postings (kt_tiny), <= kKtopChunk one
// workgroup each (kt), longer terms (kb_terms) in kKtopChunk-posting chunks
// (kc_big / kc_start, the chunks of long term x from kb_chunk0[x])
int chunk_tables(const HostPostings& hp, StructTables& st) {
  const uint32_t V = hp.n_terms;
  pack_chunks<uint64_t>(V, [&](uint32_t t) { return hp.off[t]; }, fg::kScoreChunk, fg::kScoreChunk, st.sc_tf, st.sc_tl,
                        st.sc_e0, st.sc_e1);
  pack_chunks<uint32_t>(V, [&](uint32_t t) { return t < V ? st.dir_off[t] : (uint32_t)st.n_dir; }, fg::kBucketChunk,
                        fg::kBucketChunk + 1, st.bk_tf, st.bk_tl, st.bk_e0, st.bk_e1);
  st.coff.resize(V);
  for (uint32_t t = 0; t < V; ++t) {
    const uint64_t n = hp.df(t);
    st.coff[t] = st.n_cmax;
    st.n_cmax += (uint32_t)((n + fg::kChunk - 1) / fg::kChunk);
    if (!n) continue;
    if (n <= fg::kKtopTiny) {
      st.kt_tiny.push_back(t);
      continue;
    }
    if (n <= fg::kKtopChunk) {
      st.kt.push_back(t);
      continue;
    }
    st.kb_chunk0.push_back((uint32_t)st.kc_big.size());
    for (uint64_t s = 0; s < n; s += fg::kKtopChunk) {
      st.kc_big.push_back((uint32_t)st.kb_terms.size());
      st.kc_start.push_back((uint32_t)s);
    }
    st.kb_terms.push_back(t);
  }
  st.kb_chunk0.push_back((uint32_t)st.kc_big.size());
  if (st.sc_tf.size() > 0x7FFFFFFFull || st.bk_tf.size() > 0x7FFFFFFFull) return fail(FG_EUNSUPPORTED, "index too large");
  return FG_OK;
}

// the postings' payloads (DevIndex::tfn): per field (fieldnorm id of the doc
// << 8) | tf, 2 B per posting -- what a query-time score needs besides the
// clause's weight, beside the doc id -- and the postings whose tf does not fit
// the byte (>= 255) in a sorted escape list.  hp -> st.tfn, tfn_name, esc_pos, esc_tf
void pack_payloads(const HostPostings& hp, StructTables& st) {
  st.tfn.resize(hp.tf.size());
  st.tfn_name.resize(hp.has_name ? hp.tf.size() : 0);
  const size_t np = hp.tf.size(), piece = (np + 1023) / 1024;  // > 2^32 postings: 64-bit pieces
  std::vector<std::vector<uint64_t>> ep(1024);
  parallel_dynamic(1024, hw_threads(0), 8, [&](int, uint32_t b, uint32_t e) {
    for (uint32_t pc = b; pc < e; ++pc)
      for (size_t i = (size_t)pc * piece; i < std::min(np, (size_t)(pc + 1) * piece); ++i) {
        const uint32_t d = hp.doc[i], tt = hp.tf[i] & 0xFFFFu, tn = hp.tf[i] >> 16;
        st.tfn[i] = (uint16_t)fg::tfn_pack(tt, hp.fn_text[d]);
        if (hp.has_name) st.tfn_name[i] = (uint16_t)(tn ? fg::tfn_pack(tn, hp.fn_name[d]) : 0u);
        if (tt >= fg::kTfEsc || (hp.has_name && tn >= fg::kTfEsc)) ep[pc].push_back(i);
      }
  });
  for (auto& v : ep)
    for (uint64_t i : v) {
      st.esc_pos.push_back(i);
      st.esc_tf.push_back(hp.tf[i]);
    }
}

template <class T>
void put(UploadBatch& ub, const std::vector<T>& v, const T** out) {
  ub.add(v.data(), v.size(), const_cast<T**>(out));
}

// The postings and st's tables into ONE device allocation of ix->smem, their
// addresses into ix->d and ix's ChunkTables.  The large host arrays the build
// no longer needs (the payloads, hp.tf, the two directories) are freed here:
// they bound the peak host memory of a 10M-doc build.
int upload_structure(HostPostings& hp, StructTables& st, fg_index& ix) {
  fg::DevIndex& d = ix.d;
  UploadBatch ub;
  put(ub, hp.doc, &d.doc);
  put(ub, st.tfn, &d.tfn);
  if (hp.has_name) put(ub, st.tfn_name, &d.tfn_name);
  if (!st.esc_pos.empty()) {
    put(ub, st.esc_pos, &d.esc_pos);
    put(ub, st.esc_tf, &d.esc_tf);
  }
  put(ub, hp.off, &d.off);
  put(ub, st.dir, &d.dir);
  put(ub, st.dir_off, &d.dir_off);
  put(ub, st.toff, &d.toff);
  put(ub, st.tdir, &d.tdir);
  put(ub, st.tterm, &ix.d_tterm);
  put(ub, hp.fdoc, &d.fdoc);
  put(ub, hp.foff, &d.foff);
  put(ub, st.sc_tf, &ix.d_sc_tf);
  put(ub, st.sc_tl, &ix.d_sc_tl);
  put(ub, st.sc_e0, &ix.d_sc_e0);
  put(ub, st.sc_e1, &ix.d_sc_e1);
  put(ub, st.bk_tf, &ix.d_bk_tf);
  put(ub, st.bk_tl, &ix.d_bk_tl);
  put(ub, st.bk_e0, &ix.d_bk_e0);
  put(ub, st.bk_e1, &ix.d_bk_e1);
  put(ub, st.kt, &ix.d_kt_terms);
  put(ub, st.kt_tiny, &ix.d_kt_tiny);
  put(ub, st.kb_terms, &ix.d_kb_terms);
  put(ub, st.kb_chunk0, &ix.d_kb_chunk0);
  put(ub, st.kc_big, &ix.d_kc_big);
  put(ub, st.kc_start, &ix.d_kc_start);
  put(ub, st.coff, &d.coff);
  if (int rc = ub.commit(*ix.smem, &ix.struct_bytes)) return rc;
  d.n_esc = st.esc_pos.size();
  ix.n_scb = (uint32_t)st.sc_tf.size();
  ix.n_bk = (uint32_t)st.bk_tf.size();
  ix.n_kt = (uint32_t)st.kt.size();
  ix.n_ktiny = (uint32_t)st.kt_tiny.size();
  ix.n_kbig = (uint32_t)st.kb_terms.size();
  ix.n_kchunks = (uint32_t)st.kc_big.size();
  ix.n_sc = st.n_cmax;
  ix.n_tterm = (uint32_t)st.tterm.size();
  ix.n_tiles = (uint32_t)st.n_tiles;
  std::vector<uint16_t>().swap(st.tfn);
  std::vector<uint16_t>().swap(st.tfn_name);
  std::vector<uint32_t>().swap(hp.tf);
  std::vector<uint32_t>().swap(st.dir);
  std::vector<uint32_t>().swap(st.tdir);
  return FG_OK;
}

// ---------------------------------------------------------------- rank words
// Rank words (fg_internal.h DevIndex) for the terms with df >= N / kRankDiv,
// densest first (ties by term id), within a budget of the snapshot's own:
// FUGU_RANK_FACTOR (default kRankFactor) times its postings' bytes (doc id +
// tf + score, 12 B each), at most FUGU_RANK_GIB -- so a namespace's share
// depends on its size, not on how many namespaces were built on the device
// before it.  A term with df >= N / kRankPlainDiv (FUGU_RANK_PLAIN_DIV) gets
// plain rank words (8 B per 32 docs), a sparser one sparse rank words (8 B per
// 1024-doc block + 8 B per word holding any of its docs) unless plain ones
// cost it less (small snapshots).  A quarter of the free memory caps them
// only when HBM is short, and a failed allocation is retried with half the
// terms (down to none), so a build never fails for want of them.  They hang
// on doc ids only, so rescored snapshots share them.
struct RankChoice {
  uint32_t rank_words = 0, sblocks = 0;  // words per plain term, block entries per sparse term
  std::vector<uint32_t> plain, sparse, sparse_nw;  // the terms by kind; each sparse term's words
  uint64_t n_swords = 0;                           // sum of sparse_nw
  uint64_t *d_rank = nullptr, *d_srank = nullptr;
};

// the candidates: terms with df >= N / kRankDiv, densest first (ties by term
// id), and the words of each sparse one that hold any of its docs (host only)
struct RankCandidates {
  std::vector<uint32_t> by_df, nwords;
  uint32_t pdiv = fg::kRankPlainDiv;
  bool plain_df(const HostPostings& hp, uint32_t t) const { return hp.df(t) * pdiv >= hp.n_docs; }
};
void rank_candidates(const HostPostings& hp, RankCandidates& c) {
  const uint64_t N = hp.n_docs;
  std::vector<uint32_t>& by_df = c.by_df;
  for (uint32_t t = 0; t < hp.n_terms; ++t)
    if (hp.df(t) > 0 && hp.df(t) * fg::kRankDiv >= N) by_df.push_back(t);
  std::stable_sort(by_df.begin(), by_df.end(), [&](uint32_t a, uint32_t b) { return hp.df(a) > hp.df(b); });
  if (const char* e = getenv("FUGU_RANK_PLAIN_DIV"))
    if (*e) c.pdiv = (uint32_t)std::max(1l, atol(e));
  c.nwords.assign(by_df.size(), 0);
  parallel_dynamic((uint32_t)by_df.size(), hw_threads(0), 16, [&](int, uint32_t b, uint32_t e) {
    for (uint32_t i = b; i < e; ++i) {
      const uint32_t t = by_df[i];
      if (c.plain_df(hp, t)) continue;
      uint32_t n = 0, last = 0xFFFFFFFFu;
      for (uint64_t p = hp.off[t]; p < hp.off[t + 1]; ++p) {
        const uint32_t w = hp.doc[p] >> 5;
        n += w != last;
        last = w;
      }
      c.nwords[i] = n;
    }
  });
}

// the selection: the candidates in order while they fit the byte budget ->
// rk.plain / sparse / sparse_nw / n_swords (host only)
void select_rank_terms(const HostPostings& hp, const RankCandidates& c, uint64_t budget, RankChoice& rk) {
  const std::vector<uint32_t>&by_df = c.by_df, &nwords = c.nwords;
  uint64_t used = 0;
  for (size_t i = 0; i < by_df.size(); ++i) {
    const uint64_t cp = rk.rank_words * 8ull, cs = (rk.sblocks + (uint64_t)nwords[i]) * 8ull;
    const bool plain = c.plain_df(hp, by_df[i]) || cp <= cs;
    const uint64_t cost = plain ? cp : cs;
    if (used + cost > budget || rk.plain.size() + rk.sparse.size() >= fg::kMaxDense) break;
    if (!plain && rk.n_swords + nwords[i] >= 0xFFFFFFFFull) break;  // srank_w indices are u32
    used += cost;
    if (plain) {
      rk.plain.push_back(by_df[i]);
    } else {
      rk.sparse.push_back(by_df[i]);
      rk.sparse_nw.push_back(nwords[i]);
      rk.n_swords += nwords[i];
    }
  }
}

// the candidates, the budget, the selection within it, and the two device
// allocations (into sm), each retried with half its terms when it fails
int choose_rank_terms(const HostPostings& hp, DevAllocs& sm, uint64_t* bytes, RankChoice& rk) {
  const uint64_t N = hp.n_docs;
  rk.rank_words = (uint32_t)((N + 31) / 32);
  rk.sblocks = (uint32_t)((N + 1023) / 1024);
  RankCandidates cand;
  rank_candidates(hp, cand);
  const char* v = getenv("FUGU_RANK_GIB");
  const uint64_t cap = v && *v ? (uint64_t)(atof(v) * (double)(1ull << 30)) : fg::kRankBudget;
  const char* f = getenv("FUGU_RANK_FACTOR");
  const double factor = f && *f ? atof(f) : fg::kRankFactor;
  const uint64_t want = std::min<uint64_t>(cap, (uint64_t)(factor * 12.0 * (double)hp.off[hp.n_terms]));
  size_t free_b = ~size_t(0), total_b = 0;
  if (want > (256ull << 20)) HIPCHK(hipMemGetInfo(&free_b, &total_b));  // (~1 ms: not for a small segment's)
  select_rank_terms(hp, cand, std::min<uint64_t>(want, free_b / 4), rk);
  auto alloc = [&](uint64_t b, uint64_t** out) {
    void* q = nullptr;
    if (fgh::dev_malloc(&q, b) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    sm.ptrs.push_back(q);
    *bytes += b;
    *out = static_cast<uint64_t*>(q);
    return true;
  };
  while (!rk.plain.empty() && !alloc(rk.rank_words * 8ull * rk.plain.size(), &rk.d_rank)) rk.plain.resize(rk.plain.size() / 2);
  while (!rk.sparse.empty() && !alloc((rk.sblocks * (uint64_t)rk.sparse.size() + 1 + rk.n_swords) * 8ull, &rk.d_srank)) {
    rk.sparse.resize(rk.sparse.size() / 2);
    rk.sparse_nw.resize(rk.sparse.size());
    rk.n_swords = 0;
    for (uint32_t n : rk.sparse_nw) rk.n_swords += n;
  }
  return FG_OK;
}

// the sparse rank words, built on the host from the postings: per term its
// block entries, then the zero word and all terms' words (term by term), one
// upload to rk.d_srank; the terms' slots into tmeta
int build_sparse_rank(const HostPostings& hp, const RankChoice& rk, std::vector<uint32_t>& tmeta) {
  if (rk.sparse.empty()) return FG_OK;
  const uint32_t ns = (uint32_t)rk.sparse.size(), sblocks = rk.sblocks;
  const uint32_t first_slot = (uint32_t)rk.plain.size() + 1;
  std::vector<uint64_t> wbase(ns + 1, 1);
  for (uint32_t s2 = 0; s2 < ns; ++s2) wbase[s2 + 1] = wbase[s2] + rk.sparse_nw[s2];
  std::vector<uint64_t> hs(sblocks * (uint64_t)ns + 1 + rk.n_swords);
  hs[sblocks * (uint64_t)ns] = 0;
  parallel_dynamic(ns, hw_threads(0), 16, [&](int, uint32_t b, uint32_t e) {
    for (uint32_t s2 = b; s2 < e; ++s2) {
      const uint32_t t = rk.sparse[s2];
      uint64_t* blk = hs.data() + (uint64_t)s2 * sblocks;
      uint64_t* wd = hs.data() + (uint64_t)ns * sblocks;
      std::fill(blk, blk + sblocks, 0ull);
      uint64_t cur = wbase[s2];
      uint32_t last = 0xFFFFFFFFu;
      for (uint64_t p = hp.off[t]; p < hp.off[t + 1]; ++p) {
        const uint32_t d = hp.doc[p], w = d >> 5;
        if (w != last) {
          if (last != 0xFFFFFFFFu) ++cur;
          last = w;
          wd[cur] = (uint64_t)(p - hp.off[t]) << 32;  // postings before the word's first doc
          uint64_t& be = blk[fg::srank_block(d)];
          if (!(uint32_t)be) be = cur << 32;  // the block's first word
          be |= 1ull << (w & 31u);
        }
        wd[cur] |= 1ull << (d & 31u);
      }
    }
  });
  HIPCHK(hipMemcpyAsync(rk.d_srank, hs.data(), hs.size() * 8, hipMemcpyHostToDevice, kBuildStream));
  HIPCHK(hipStreamSynchronize(kBuildStream));
  for (uint32_t s2 = 0; s2 < ns; ++s2) tmeta[rk.sparse[s2]] |= ((first_slot + s2) << 16) | 0x80000000u;
  return FG_OK;
}

// one k_rank launch for every plain rank term (per slot the term's posting
// range) into rk.d_rank; the terms' slots into tmeta
int launch_plain_rank(const HostPostings& hp, const RankChoice& rk, const uint32_t* d_doc, std::vector<uint32_t>& tmeta) {
  if (rk.plain.empty()) return FG_OK;
  std::vector<uint64_t> sb(rk.plain.size());
  std::vector<uint32_t> sn(rk.plain.size());
  for (uint32_t s2 = 0; s2 < rk.plain.size(); ++s2) {
    const uint32_t t = rk.plain[s2];
    sb[s2] = hp.off[t];
    sn[s2] = (uint32_t)hp.df(t);
    tmeta[t] |= ((s2 + 1) << 16) | 0x80000000u;
  }
  // the slot tables are stream-ordered temporaries: freeing them does not
  // synchronise the device (hipFree would wait for every stream's work)
  void* d_tab = nullptr;
  const size_t nb = sb.size() * 8, nn = sn.size() * 4;
  if (fgh::dev_malloc_async(&d_tab, nb + nn + 16, kBuildStream) != hipSuccess) return fail(FG_EOOM, "hipMallocAsync failed");
  uint64_t* d_sb = static_cast<uint64_t*>(d_tab);
  uint32_t* d_sn = reinterpret_cast<uint32_t*>(static_cast<char*>(d_tab) + nb);
  HIPCHK(hipMemcpyAsync(d_sb, sb.data(), nb, hipMemcpyHostToDevice, kBuildStream));
  HIPCHK(hipMemcpyAsync(d_sn, sn.data(), nn, hipMemcpyHostToDevice, kBuildStream));
  HIPCHK(fg::launch_rank(d_doc, d_sb, d_sn, (uint32_t)rk.plain.size(), rk.rank_words, rk.d_rank, kBuildStream));
  HIPCHK(hipFreeAsync(d_tab, kBuildStream));
  HIPCHK(hipStreamSynchronize(kBuildStream));
  return FG_OK;
}

// host bookkeeping of the structure: the counts, the rank words' addresses and
// the host arrays the planner reads (moved out of hp and st)
void host_bookkeeping(fg_index& ix, HostPostings& hp, StructTables& st, const RankChoice& rk, bool keep_host) {
  const uint32_t V = hp.n_terms, VF = hp.n_fterms;
  ix.n_docs = hp.n_docs;
  ix.n_terms = ix.n_vocab = V;
  ix.has_name = hp.has_name;
  ix.n_postings = hp.off[V];
  ix.tot_local[0] = hp.tot[0];
  ix.tot_local[1] = hp.tot[1];
  ix.dir_entries = st.n_dir;
  ix.tile_entries = st.n_tile_entries;
  ix.n_rank = (uint32_t)(rk.plain.size() + rk.sparse.size());
  ix.n_srank_words = rk.sparse.empty() ? 0 : 1 + rk.n_swords;
  ix.tmeta = std::move(st.tmeta);
  ix.dir_off = std::move(st.dir_off);
  ix.d.rank = rk.d_rank;
  ix.d.srank = rk.d_srank;
  ix.d.srank_w = rk.d_srank ? rk.d_srank + (uint64_t)rk.sblocks * rk.sparse.size() : nullptr;
  ix.d.n_prank = (uint32_t)rk.plain.size();
  ix.d.srank_blocks = rk.sblocks;
  ix.d.rank_words = rk.rank_words;
  ix.d.n_docs = hp.n_docs;
  ix.d.n_terms = V;
  ix.d.has_name = hp.has_name ? 1u : 0u;
  ix.d.n_fterms = VF;
  ix.off = std::move(hp.off);
  ix.df_text = std::move(hp.df_text);
  ix.df_name = std::move(hp.df_name);
  // the first and last doc of each term's postings (docs, off) when it has any
  auto ends = [](uint32_t n, const auto& off, const std::vector<uint32_t>& docs, fgh::SharedVec<uint32_t>& first,
                 fgh::SharedVec<uint32_t>& last) {
    std::vector<uint32_t> fd(n, 0), ld(n, 0);
    for (uint32_t t = 0; t < n; ++t)
      if (off[t + 1] > off[t]) {
        fd[t] = docs[off[t]];
        ld[t] = docs[off[t + 1] - 1];
      }
    first = std::move(fd);
    last = std::move(ld);
  };
  ends(V, ix.off, hp.doc, ix.first_doc, ix.last_doc);
  if (keep_host) ix.h_doc = std::make_shared<const std::vector<uint32_t>>(std::move(hp.doc));
  ix.n_fterms = VF;
  ix.df_facet_local = hp.df_facet;
  ix.tot_f_local = hp.tot_f;
  ends(VF, hp.foff, hp.fdoc, ix.ffirst, ix.flast);
  ix.foff = std::move(hp.foff);
}

// the build's statistics: the shard's own, or the namespace's global ones
int build_statistics(fg_index* ix, const fg_global_stats* g) {
  const uint32_t VF = ix->n_fterms;
  if (g && VF && !g->df_facet) return fail(FG_EINVAL, "global statistics lack df_facet for a faceted shard");
  if (g && VF)
    for (uint32_t t = 0; t < VF; ++t)
      if (g->df_facet[t] < ix->df_facet_local[t]) return fail(FG_EINVAL, "global facet df of term %u is below this shard's", t);
  const uint64_t tot_local[2] = {ix->tot_local[0], ix->tot_local[1]};
  fgh::set_stats(ix, g ? g->n_docs : ix->n_docs, g ? g->tot_tokens : tot_local, g ? g->df_text : ix->df_text.data(),
                 g ? g->df_name : ix->df_name.data(), g ? g->tot_facet_tokens : ix->tot_f_local,
                 g && VF ? g->df_facet : ix->df_facet_local.data(), nullptr);
  return FG_OK;
}

// A snapshot from host postings: the structure's phases in order (their tables
// in st, uploaded into ix->smem), then the statistics and the bounds under
// them.  Consumes hp.  g: global statistics of a doc-sharded namespace (NULL:
// the shard's own).
int finish_index(int dev, HostPostings& hp, bool keep_host, fg_index** out, const fg_global_stats* g = nullptr) {
  auto ix = std::make_unique<fg_index>();
  ix->dev = dev;
  ix->mem.dev = dev;
  fgh::device_pools(dev, &ix->pool, &ix->pinned);
  ix->smem = std::make_shared<DevAllocs>();
  ix->smem->dev = dev;
  if (g && g->df_name == nullptr && hp.has_name) return fail(FG_EINVAL, "global statistics lack df_name for a shard with names");
  StructTables st;
  RankChoice rk;
  int rc;
  if ((rc = bucket_directory(hp, st))) return rc;
  g_bt.mark("directory");
  tile_directory(hp, st);
  if ((rc = chunk_tables(hp, st))) return rc;
  pack_payloads(hp, st);
  HIPCHK(hipSetDevice(dev));  // (host only up to here)
  if ((rc = upload_structure(hp, st, *ix))) return rc;
  g_bt.mark("upload");
  if ((rc = choose_rank_terms(hp, *ix->smem, &ix->struct_bytes, rk))) return rc;
  g_bt.mark("rank words: budget");
  if ((rc = build_sparse_rank(hp, rk, st.tmeta))) return rc;
  g_bt.mark("rank words: sparse");
  if ((rc = launch_plain_rank(hp, rk, ix->d.doc, st.tmeta))) return rc;
  if ((rc = dev_upload(*ix->smem, st.tmeta.data(), st.tmeta.size(), const_cast<uint32_t**>(&ix->d.tmeta), &ix->struct_bytes)))
    return rc;
  g_bt.mark("rank words");
  host_bookkeeping(*ix, hp, st, rk, keep_host);
  if ((rc = build_statistics(ix.get(), g))) return rc;
  g_bt.mark("weights");
  if ((rc = build_bounds(ix.get(), hp.alive))) return rc;
  g_bt.mark("tail");
  *out = ix.release();
  return FG_OK;
}

// ---------------------------------------------------------------- host postings from docs
// Sorted (term, tf) runs of one field of one doc into `runs` (term << 0, tf).
inline void doc_runs(const uint32_t* tok, uint64_t len, std::vector<uint32_t>& scratch,
                     std::vector<std::pair<uint32_t, uint32_t>>& runs) {
  runs.clear();
  if (!len) return;
  scratch.assign(tok, tok + len);
  std::sort(scratch.begin(), scratch.end());
  for (size_t i = 0; i < scratch.size();) {
    size_t j = i;
    while (j < scratch.size() && scratch[j] == scratch[i]) ++j;
    runs.emplace_back(scratch[i], (uint32_t)(j - i));
    i = j;
  }
}

// One doc's text and name runs merged by term: f(term, tf_text, tf_name) for
// each distinct term in ascending order (a tf of 0: not in that field); stops
// and returns false when f does.  One per thread (it keeps the scratch).
struct DocTerms {
  std::vector<uint32_t> scratch;
  std::vector<std::pair<uint32_t, uint32_t>> rt, rn;
  template <class F>
  bool walk(const fg_docs_input* in, bool has_name_in, uint32_t d, F&& f) {
    doc_runs(in->text_tok + in->text_off[d], in->text_off[d + 1] - in->text_off[d], scratch, rt);
    if (has_name_in) doc_runs(in->name_tok + in->name_off[d], in->name_off[d + 1] - in->name_off[d], scratch, rn);
    else rn.clear();
    size_t i = 0, j = 0;
    while (i < rt.size() || j < rn.size()) {
      const uint32_t a = i < rt.size() ? rt[i].first : 0xFFFFFFFFu;
      const uint32_t c = j < rn.size() ? rn[j].first : 0xFFFFFFFFu;
      const uint32_t term = std::min(a, c);
      uint32_t tt = 0, tn = 0;
      if (a == term) tt = rt[i++].second;
      if (c == term) tn = rn[j++].second;
      if (!f(term, tt, tn)) return false;
    }
    return true;
  }
};

// Facet postings from per-doc FacetTokenizer tokens (fg_docs_input): each doc
// once per distinct token (df), every token counted in total_num_tokens.
int build_facets(const fg_docs_input* in, HostPostings& hp, int T) {
  hp.n_fterms = 0;
  hp.foff.assign(1, 0);
  hp.fdoc.clear();
  hp.df_facet.clear();
  hp.tot_f = 0;
  if (!in->facet_off) return FG_OK;
  const uint32_t N = in->n_docs, VF = in->n_facet_terms;
  if (in->facet_off[0] != 0 || (!in->facet_tok && in->facet_off[N] > 0))
    return fail(FG_EINVAL, "bad facet token arrays");
  for (uint32_t d = 0; d < N; ++d)
    if (in->facet_off[d + 1] < in->facet_off[d]) return fail(FG_EINVAL, "facet_off not monotone at doc %u", d);
  hp.n_fterms = VF;
  hp.tot_f = in->facet_off[N];
  std::vector<std::vector<uint32_t>> cnt(T);
  std::atomic<bool> bad{false};
  auto runs = [&](uint32_t d, std::vector<uint32_t>& sc) {
    sc.assign(in->facet_tok + in->facet_off[d], in->facet_tok + in->facet_off[d + 1]);
    std::sort(sc.begin(), sc.end());
    sc.erase(std::unique(sc.begin(), sc.end()), sc.end());
  };
  parallel_ranges(N, T, [&](int t, uint32_t b, uint32_t e) {
    cnt[t].assign(VF, 0);
    std::vector<uint32_t> sc;
    for (uint32_t d = b; d < e; ++d) {
      runs(d, sc);
      for (uint32_t x : sc) {
        if (x >= VF) { bad = true; return; }
        cnt[t][x]++;
      }
    }
  });
  if (bad) return fail(FG_EINVAL, "facet token id >= n_facet_terms");
  std::vector<std::vector<uint64_t>> cur(T);
  hp.foff.assign(VF + 1, 0);
  hp.df_facet.assign(VF, 0);
  uint64_t acc = 0;
  for (int t = 0; t < T; ++t) cur[t].assign(VF, 0);
  for (uint32_t x = 0; x < VF; ++x) {
    hp.foff[x] = acc;
    for (int t = 0; t < T; ++t) {
      if (cnt[t].empty()) continue;
      cur[t][x] = acc;
      acc += cnt[t][x];
      hp.df_facet[x] += cnt[t][x];
    }
  }
  hp.foff[VF] = acc;
  hp.fdoc.resize(acc);
  parallel_ranges(N, T, [&](int t, uint32_t b, uint32_t e) {
    std::vector<uint32_t> sc;
    for (uint32_t d = b; d < e; ++d) {
      runs(d, sc);
      for (uint32_t x : sc) hp.fdoc[cur[t][x]++] = d;
    }
  });
  return FG_OK;
}

// A build's own term dictionary (fg_index::tmap).  Its docs' distinct terms are
// marked in a vocabulary bitset; when they are fewer than 1/kLocalDiv of the
// vocabulary (a commit's 1000 new docs hold ~2% of a 10M-doc namespace's), the
// build runs on local ids: the tokens renumbered in vocabulary order (a rank in
// the bitset) and the statistics gathered to them, so its work and its device
// arrays scale with its own terms, not the vocabulary's.  The marking stops as
// soon as the count passes the limit (a large build decides within its first
// docs).  L.tmap stays empty: vocabulary ids.
constexpr uint32_t kLocalDiv = 4;
struct LocalDict {
  std::vector<uint32_t> tmap, ttok, ntok, df_t, df_n;
  fg_docs_input in{};
  fg_global_stats g{};
};
int local_dict(const fg_docs_input* in, const fg_global_stats* g, LocalDict& L) {
  const uint32_t N = in->n_docs, V = in->n_terms;
  const bool has_name = in->name_off && in->name_tok;
  const uint64_t limit = V / kLocalDiv;
  std::vector<uint64_t> bits(((uint64_t)V + 63) / 64, 0);
  uint64_t n = 0;
  auto mark = [&](const uint32_t* tok, uint64_t b, uint64_t e) {
    for (uint64_t i = b; i < e; ++i) {
      const uint32_t t = tok[i];
      if (t >= V) return false;
      uint64_t& w = bits[t >> 6];
      const uint64_t m = 1ull << (t & 63);
      n += (w & m) == 0;
      w |= m;
    }
    return true;
  };
  for (uint32_t d = 0; d < N && n <= limit; ++d) {
    if (!mark(in->text_tok, in->text_off[d], in->text_off[d + 1])) return fail(FG_EINVAL, "token id >= n_terms");
    if (has_name && !mark(in->name_tok, in->name_off[d], in->name_off[d + 1]))
      return fail(FG_EINVAL, "token id >= n_terms");
  }
  if (n > limit || n == 0) return FG_OK;
  const uint32_t v = (uint32_t)n;
  std::vector<uint32_t> rank(bits.size());
  L.tmap.reserve(v);
  for (size_t w = 0; w < bits.size(); ++w) {
    rank[w] = (uint32_t)L.tmap.size();
    for (uint64_t x = bits[w]; x; x &= x - 1) L.tmap.push_back((uint32_t)(w * 64 + __builtin_ctzll(x)));
  }
  auto local = [&](uint32_t t) {
    return rank[t >> 6] + (uint32_t)__builtin_popcountll(bits[t >> 6] & ((1ull << (t & 63)) - 1));
  };
  const uint64_t nt = in->text_off[N], nn = has_name ? in->name_off[N] : 0;
  L.ttok.resize(nt);
  for (uint64_t i = in->text_off[0]; i < nt; ++i) L.ttok[i] = local(in->text_tok[i]);
  if (has_name) {
    L.ntok.resize(nn);
    for (uint64_t i = in->name_off[0]; i < nn; ++i) L.ntok[i] = local(in->name_tok[i]);
  }
  L.in = *in;
  L.in.n_terms = v;
  L.in.text_tok = L.ttok.data();
  if (has_name) L.in.name_tok = L.ntok.data();
  if (g) {
    L.df_t.resize(v);
    L.df_n.resize(v);
    for (uint32_t l = 0; l < v; ++l) {
      L.df_t[l] = g->df_text[L.tmap[l]];
      L.df_n[l] = g->df_name ? g->df_name[L.tmap[l]] : 0u;
    }
    L.g = *g;
    L.g.df_text = L.df_t.data();
    L.g.df_name = g->df_name ? L.df_n.data() : nullptr;
  }
  return FG_OK;
}

// global statistics usable for a snapshot of n_docs docs?
bool global_stats_ok(const fg_global_stats* g, uint64_t n_docs) {
  return !g || (g->df_text && g->n_docs >= n_docs && g->n_docs < 0x7FFFFFFFull);
}
// ... and no global df below the postings' own (`part`: what the message calls them)
int check_global_df(const fg_global_stats* g, const HostPostings& hp, const char* part) {
  if (g)
    for (uint32_t t = 0; t < hp.n_terms; ++t)
      if (g->df_text[t] < hp.df_text[t] || (g->df_name ? g->df_name[t] : 0u) < hp.df_name[t])
        return fail(FG_EINVAL, "global df of term %u is below this %s's", t, part);
  return FG_OK;
}

// Host postings from the docs' tokens in two passes over the docs (counts and
// offsets, then the fill), the facet postings, then finish_index.  (in, g: the
// caller's or local_dict's; checked by fg_index_build_from_docs_global.)
int build_from_docs(fg_ctx* ctx, int dev, const fg_docs_input* in, const fg_global_stats* g, fg_index** out) {
  if (std::find(ctx->devs.begin(), ctx->devs.end(), dev) == ctx->devs.end())
    return fail(FG_EINVAL, "device %d not in context", dev);
  const uint32_t N = in->n_docs, V = in->n_terms;
  const bool has_name_in = in->name_off && in->name_tok;
  // every thread of pass 1 zeroes and merges three vocabulary-sized count
  // arrays: a small build (a commit's new docs) uses few threads
  const int T = std::max(1, std::min(hw_threads(in->threads), (int)(N / 4096)));
  HostPostings hp;
  hp.n_docs = N;
  hp.n_terms = V;
  hp.fn_text.resize(N);
  hp.fn_name.assign(N, 0);
  // pass 1: per-thread counts (merged df, df_text, df_name), fieldnorms
  std::vector<std::vector<uint32_t>> cnt(T), dft(T), dfn(T);
  std::vector<uint64_t> tot_t(T, 0), tot_n(T, 0);
  std::atomic<bool> bad{false};
  parallel_ranges(N, T, [&](int t, uint32_t b, uint32_t e) {
    cnt[t].assign(V, 0);
    dft[t].assign(V, 0);
    dfn[t].assign(V, 0);
    DocTerms dt;
    for (uint32_t d = b; d < e; ++d) {
      const uint64_t lt = in->text_off[d + 1] - in->text_off[d];
      const uint64_t ln = has_name_in ? in->name_off[d + 1] - in->name_off[d] : 0;
      tot_t[t] += lt;
      tot_n[t] += ln;
      hp.fn_text[d] = fgh::fieldnorm_id(lt);
      if (has_name_in) hp.fn_name[d] = fgh::fieldnorm_id(ln);
      const bool ok = dt.walk(in, has_name_in, d, [&](uint32_t term, uint32_t tt, uint32_t tn) {
        if (term >= V) return false;
        cnt[t][term]++;
        dft[t][term] += tt != 0;
        dfn[t][term] += tn != 0;
        return true;
      });
      if (!ok) { bad = true; return; }
    }
  });
  if (bad) return fail(FG_EINVAL, "token id >= n_terms");
  const int used = (int)std::count_if(cnt.begin(), cnt.end(), [](auto& v) { return !v.empty(); });
  hp.off.assign(V + 1, 0);
  hp.df_text.assign(V, 0);
  hp.df_name.assign(V, 0);
  // per-thread write cursors (reuse cnt as u64 cursors via a separate array)
  std::vector<std::vector<uint64_t>> cur(used);
  for (int t = 0; t < used; ++t) cur[t].resize(V);
  uint64_t acc = 0;
  for (uint32_t term = 0; term < V; ++term) {
    hp.off[term] = acc;
    for (int t = 0; t < used; ++t) {
      cur[t][term] = acc;
      acc += cnt[t][term];
      hp.df_text[term] += dft[t][term];
      hp.df_name[term] += dfn[t][term];
    }
  }
  hp.off[V] = acc;
  cnt.clear();
  dft.clear();
  dfn.clear();
  for (int t = 0; t < used; ++t) { hp.tot[0] += tot_t[t]; hp.tot[1] += tot_n[t]; }
  hp.has_name = hp.tot[1] > 0;
  try {
    hp.doc.resize(acc);
    hp.tf.resize(acc);
  } catch (...) {
    return fail(FG_EOOM, "host postings (%llu) allocation failed", (unsigned long long)acc);
  }
  g_bt.mark("pass 1 counts + offsets");
  // pass 2: fill (thread t's docs land after threads < t within each term)
  parallel_ranges(N, T, [&](int t, uint32_t b, uint32_t e) {
    DocTerms dt;
    std::vector<uint64_t>& c = cur[t];
    for (uint32_t d = b; d < e; ++d)
      dt.walk(in, has_name_in, d, [&](uint32_t term, uint32_t tt, uint32_t tn) {
        const uint64_t p = c[term]++;
        hp.doc[p] = d;
        hp.tf[p] = std::min<uint32_t>(tt, 0xFFFF) | (std::min<uint32_t>(tn, 0xFFFF) << 16);
        return true;
      });
  });
  hp.alive = alive_from_deleted(in->deleted, N);
  if (int rc = check_global_df(g, hp, "shard")) return rc;
  g_bt.mark("pass 2 fill");
  if (int rc = build_facets(in, hp, T)) return rc;
  g_bt.mark("facets");
  return finish_index(dev, hp, in->keep_host_postings != 0, out, g);
}

// The forward index of a snapshot built with fg_docs_input::keep_positions
// (DevIndex::fwd_off / fwd): per field every doc's tokens laid out by analyzer
// position -- a gap entry leaves a kFwdNone hole before its token -- and
// uploaded on the build stream (the background stream of a commit or a merge).
// Structure: shared with the snapshot's rescores, counted in device_bytes.
int fwd_field(uint32_t N, const uint64_t* off, const uint32_t* tok, const uint64_t* gap, uint64_t n_gap,
              std::vector<uint64_t>& foff, std::vector<uint32_t>& fwd) {
  const uint64_t nt = off[N];
  for (uint64_t i = 0; i < n_gap; ++i)
    if (gap[i] >= nt || gap[i] < off[0] || (i && gap[i] < gap[i - 1]))
      return fail(FG_EINVAL, "gap list not ascending indices into the tokens");
  foff.resize((size_t)N + 1);
  try {
    fwd.resize(nt + n_gap);
  } catch (...) {
    return fail(FG_EOOM, "forward index (%llu positions) allocation failed", (unsigned long long)(nt + n_gap));
  }
  uint64_t g = 0, o = 0;
  for (uint32_t d = 0; d < N; ++d) {
    foff[d] = o;
    for (uint64_t i = off[d]; i < off[d + 1]; ++i) {
      for (; g < n_gap && gap[g] == i; ++g) fwd[o++] = fg::kFwdNone;
      fwd[o++] = tok[i];
    }
  }
  foff[N] = o;
  return FG_OK;
}

int attach_positions(fg_index* ix, const fg_docs_input* in) {
  if ((in->n_text_gap && !in->text_gap) || (in->n_name_gap && !in->name_gap)) return fail(FG_EINVAL, "gap count without a gap list");
  const uint32_t N = in->n_docs;
  const bool has_name_in = in->name_off && in->name_tok;
  HIPCHK(hipSetDevice(ix->dev));
  uint64_t bytes = 0;
  std::vector<uint64_t> foff;
  std::vector<uint32_t> fwd;
  // one field's forward index built and uploaded into the structure's allocations
  auto field = [&](const uint64_t* off, const uint32_t* tok, const uint64_t* gap, uint64_t n_gap, const uint64_t** d_off,
                   const uint32_t** d_fwd) {
    if (int rc = fwd_field(N, off, tok, gap, n_gap, foff, fwd)) return rc;
    if (int rc = dev_upload(*ix->smem, foff.data(), foff.size(), const_cast<uint64_t**>(d_off), &bytes)) return rc;
    return dev_upload(*ix->smem, fwd.data(), fwd.size(), const_cast<uint32_t**>(d_fwd), &bytes);
  };
  if (int rc = field(in->text_off, in->text_tok, in->text_gap, in->n_text_gap, &ix->d.fwd_off, &ix->d.fwd)) return rc;
  if (has_name_in && ix->d.tfn_name)  // (no name postings: no phrase matches there)
    if (int rc = field(in->name_off, in->name_tok, in->name_gap, in->n_name_gap, &ix->d.fwd_off_name, &ix->d.fwd_name))
      return rc;
  ix->struct_bytes += bytes;
  ix->device_bytes += bytes;
  ix->has_positions = true;
  g_bt.mark("forward index");
  return FG_OK;
}

// fg_index_build_global's first checks of `in` and g (after the NULL arguments;
// they need no context): fg_index_build_positional runs them before its own
int index_input_head(const fg_index_input* in, const fg_global_stats* g) {
  if (!global_stats_ok(g, in->n_docs)) return fail(FG_EINVAL, "bad global statistics");
  if (in->n_docs == 0 || in->n_docs >= 0x7FFFFFFFu) return fail(FG_EINVAL, "n_docs out of range");
  if (in->term_off[0] != 0) return fail(FG_EINVAL, "term_off[0] must be 0");
  if (in->term_off[in->n_terms] > 0 && (!in->doc || (!in->tf_text && !in->tf_name)))
    return fail(FG_EINVAL, "postings without doc ids or term frequencies");
  return FG_OK;
}

// ---------------------------------------------------------------- forward index from positional postings
// fg_index_build_positional's checks of `pos` against the postings' tf: host only
// (no context, no device), each message names the field.
int check_positions_input(const fg_index_input* in, const fg_positions_input* pos) {
  const uint64_t P = in->term_off[in->n_terms];
  uint64_t st = 0, sn = 0;
  if (in->tf_text)
    for (uint64_t p = 0; p < P; ++p) st += in->tf_text[p];
  if (in->tf_name)
    for (uint64_t p = 0; p < P; ++p) sn += in->tf_name[p];
  if (pos->n_text_pos && !pos->text_pos) return fail(FG_EINVAL, "text positions: text_pos is NULL with n_text_pos = %llu", (unsigned long long)pos->n_text_pos);
  if (pos->n_text_pos != st)
    return fail(FG_EINVAL, "text positions: n_text_pos = %llu, the postings' tf_text sum to %llu",
                (unsigned long long)pos->n_text_pos, (unsigned long long)st);
  if (pos->n_name_pos && !pos->name_pos) return fail(FG_EINVAL, "name positions: name_pos is NULL with n_name_pos = %llu", (unsigned long long)pos->n_name_pos);
  if (sn && !pos->name_pos) return fail(FG_EINVAL, "name positions: the postings have tf_name > 0 but name_pos is NULL");
  if (pos->n_name_pos != sn)
    return fail(FG_EINVAL, "name positions: n_name_pos = %llu, the postings' tf_name sum to %llu",
                (unsigned long long)pos->n_name_pos, (unsigned long long)sn);
  return FG_OK;
}

// One field's forward index built on the device from the field's
// tf per posting (tf may be nullptr: all 0) and its positions in posting order,
// over the snapshot's uploaded postings (ix->d.doc / off, k_score's chunk
// tables).  fwd_off and fwd go into the structure's allocations; the field's
// temporaries (tf, positions, posting offsets, row lengths) are one
// stream-ordered block freed when the field is done.  Two read-backs: the row
// total with the error word (fwd is allocated by it), then the error word with
// the count of filled entries.
int fwd_from_postings(fg_index* ix, const char* field, const uint16_t* tf, const uint32_t* pos, uint64_t n_pos,
                      const uint64_t** d_off, const uint32_t** d_fwd, uint64_t* bytes) {
  static_assert(fg::kFwdSlices == FG_FWD_SCAN_SLICES, "fugu.h FG_FWD_SCAN_SLICES");
  const uint64_t P = ix->n_postings, N = ix->n_docs;
  Parts L;
  const Parts::P p_tf = L.add(2 * P), p_pos = L.add(4 * n_pos), p_poff = L.add(8 * (P + 1)), p_len = L.add(4 * N),
                 p_part = L.add(8ull * (fg::kFwdSlices + 1)), p_words = L.add(16);
  AsyncTmp tmp;
  if (fgh::dev_malloc_async(&tmp.p, L.total, kBuildStream) != hipSuccess)
    return fail(FG_EOOM, "forward index (%s): hipMallocAsync(%zu) failed", field, L.total);
  char* t = static_cast<char*>(tmp.p);
  void* q = nullptr;
  const size_t off_b = 8 * (N + 1);
  if (fgh::dev_malloc(&q, off_b) != hipSuccess) return fail(FG_EOOM, "forward index (%s): hipMalloc(%zu) failed", field, off_b);
  ix->smem->ptrs.push_back(q);
  *bytes += off_b;
  // (events only under FUGU_BUILD_TRACE: the upload, then the 3 + 3 spans of the launches)
  hipEvent_t ev[8] = {};
  struct EvGuard {
    hipEvent_t* e;
    ~EvGuard() { for (int i = 0; i < 8; ++i) if (e[i]) (void)hipEventDestroy(e[i]); }
  } ev_guard{ev};
  const bool timed = g_bt.on;
  if (timed)
    for (auto& e : ev) HIPCHK(hipEventCreate(&e));
  fg::FwdJob j{};
  j.doc = ix->d.doc;
  j.off = ix->d.off;
  j.tf = reinterpret_cast<const uint16_t*>(t + p_tf.off);
  j.pos = reinterpret_cast<const uint32_t*>(t + p_pos.off);
  j.poff = reinterpret_cast<uint64_t*>(t + p_poff.off);
  j.len = reinterpret_cast<uint32_t*>(t + p_len.off);
  j.part = reinterpret_cast<uint64_t*>(t + p_part.off);
  j.err = reinterpret_cast<uint32_t*>(t + p_words.off);
  j.filled = reinterpret_cast<unsigned long long*>(t + p_words.off + 8);
  j.fwd_off = static_cast<uint64_t*>(q);
  j.n_post = P;
  j.n_docs = (uint32_t)N;
  j.sc_tf = ix->d_sc_tf;
  j.sc_tl = ix->d_sc_tl;
  j.sc_e0 = ix->d_sc_e0;
  j.sc_e1 = ix->d_sc_e1;
  j.n_chunks = ix->n_scb;
  j.grid_cap = fgh::bg_grid_cap(ix->dev);
  const auto t_up = std::chrono::steady_clock::now();
  if (P) {
    if (tf) HIPCHK(hipMemcpyAsync(t + p_tf.off, tf, 2 * P, hipMemcpyHostToDevice, kBuildStream));
    else HIPCHK(hipMemsetAsync(t + p_tf.off, 0, 2 * P, kBuildStream));
  }
  if (n_pos) HIPCHK(hipMemcpyAsync(t + p_pos.off, pos, 4 * n_pos, hipMemcpyHostToDevice, kBuildStream));
  HIPCHK(hipMemsetAsync(j.len, 0, 4 * N, kBuildStream));
  HIPCHK(hipMemsetAsync(j.err, 0, 16, kBuildStream));
  double up_ms = 0;
  if (timed) {
    HIPCHK(hipStreamSynchronize(kBuildStream));
    up_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_up).count();
  }
  HIPCHK(fg::launch_fwd_rows(j, kBuildStream, timed ? ev : nullptr));
  uint64_t total = 0;
  uint32_t err = 0;
  HIPCHK(hipMemcpyAsync(&total, j.fwd_off + N, 8, hipMemcpyDeviceToHost, kBuildStream));
  HIPCHK(hipMemcpyAsync(&err, j.err, 4, hipMemcpyDeviceToHost, kBuildStream));
  HIPCHK(hipStreamSynchronize(kBuildStream));
  auto refuse = [&](uint32_t e) {
    if (e & fg::kFwdErrNone) return fail(FG_EINVAL, "%s positions: a position of 0xFFFFFFFF", field);
    if (e & fg::kFwdErrOrder) return fail(FG_EINVAL, "%s positions: a posting's positions do not strictly ascend", field);
    return fail(FG_EINVAL, "%s positions: a position past its doc's last one", field);
  };
  if (err) return refuse(err);
  const size_t fwd_b = std::max<size_t>(4 * total, 16);
  if (total > (~size_t(0) >> 3) || fgh::dev_malloc(&q, fwd_b) != hipSuccess)
    return fail(FG_EOOM, "forward index (%s): hipMalloc of %llu positions failed", field, (unsigned long long)total);
  ix->smem->ptrs.push_back(q);
  *bytes += fwd_b;
  j.fwd = static_cast<uint32_t*>(q);
  j.n_fwd = total;
  HIPCHK(fg::launch_fwd_fill(j, kBuildStream, timed ? ev + 4 : nullptr));
  unsigned long long filled = 0;
  HIPCHK(hipMemcpyAsync(&err, j.err, 4, hipMemcpyDeviceToHost, kBuildStream));
  HIPCHK(hipMemcpyAsync(&filled, j.filled, 8, hipMemcpyDeviceToHost, kBuildStream));
  HIPCHK(hipStreamSynchronize(kBuildStream));
  if (err) return refuse(err);
  if (filled != n_pos)
    return fail(FG_EINVAL, "%s positions: two postings claim the same (doc, position) (%llu of %llu positions distinct)", field,
                filled, (unsigned long long)n_pos);
  if (timed) {
    float ms[6] = {};
    for (int i = 0; i < 3; ++i) {
      (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
      (void)hipEventElapsedTime(&ms[3 + i], ev[4 + i], ev[5 + i]);
    }
    fprintf(stderr,
            "[fg build] forward index (%s): %llu postings, %llu positions, %llu row entries; ms: upload %.3f, "
            "scan_tf %.3f, k_fwd_len %.3f, scan_len %.3f, k_fwd_fill %.3f, k_fwd_scatter %.3f, k_fwd_check %.3f\n",
            field, (unsigned long long)P, (unsigned long long)n_pos, (unsigned long long)total, up_ms, ms[0], ms[1], ms[2],
            ms[3], ms[4], ms[5]);
  }
  *d_off = j.fwd_off;
  *d_fwd = j.fwd;
  return FG_OK;
}

// The forward index of a snapshot built from positional postings
// (fg_index_build_positional), beside attach_positions: the same arrays, built by
// the k_fwd_* kernels from the positions of the caller's postings.  The two
// fields one after the other, so the peak is one field's temporaries.  `name`
// only when the snapshot has name payloads and the postings any name position.
int attach_positions_postings(fg_index* ix, const fg_index_input* in, const fg_positions_input* pos) {
  HIPCHK(hipSetDevice(ix->dev));
  uint64_t bytes = 0;
  int rc = fwd_from_postings(ix, "text", in->tf_text, pos->text_pos, pos->n_text_pos, &ix->d.fwd_off, &ix->d.fwd, &bytes);
  if (!rc && ix->d.tfn_name && pos->n_name_pos)
    rc = fwd_from_postings(ix, "name", in->tf_name, pos->name_pos, pos->n_name_pos, &ix->d.fwd_off_name, &ix->d.fwd_name,
                           &bytes);
  ix->struct_bytes += bytes;
  ix->device_bytes += bytes;
  if (rc) return rc;
  ix->has_positions = true;
  g_bt.mark("forward index (device)");
  return FG_OK;
}

// one snapshot rescored (fg_index_rescore); wts: shared precomputed weights or
// nullptr.  Host only: tantivy scores at query time (src/db/search.rs:162), so
// a new Searcher's statistics need no device work -- the snapshot shares every
// device array of its base (structure and bound tables) and gets the new
// statistics (plans read them), a new alive bitset when docs were deleted, and
// the ratios that scale the build-time bounds (relate_stats).
int rescore_one(const fg_index* base, const fg_global_stats* g, const uint8_t* deleted, fg_index** out,
                const fgh::Weights* wts) {
  if (!base || !g || !out || !g->df_text) return fail(FG_EINVAL, "bad arguments");
  const uint32_t N = base->n_docs, V = base->n_terms, VF = base->n_fterms;
  if (g->n_docs < N || g->n_docs >= 0x7FFFFFFFull) return fail(FG_EINVAL, "bad global statistics");
  if (base->has_name && !g->df_name) return fail(FG_EINVAL, "global statistics lack df_name for a snapshot with names");
  if (VF && !g->df_facet) return fail(FG_EINVAL, "global statistics lack df_facet for a faceted snapshot");
  // the statistics' doc frequencies of the snapshot's terms (gathered to local
  // ids when it has its own dictionary: a commit's rescores then cost its terms)
  const uint32_t* gt = g->df_text;
  const uint32_t* gn = g->df_name;
  std::vector<uint32_t> lt, ln;
  if (!base->tmap.empty()) {
    const uint32_t* tm = base->tmap.data();
    lt.resize(V);
    for (uint32_t t = 0; t < V; ++t) lt[t] = g->df_text[tm[t]];
    gt = lt.data();
    if (g->df_name) {
      ln.resize(V);
      for (uint32_t t = 0; t < V; ++t) ln[t] = g->df_name[tm[t]];
      gn = ln.data();
    }
    wts = nullptr;  // (shared weights are vocabulary-indexed)
  }
  {  // (branch-free scans: every older segment of every commit runs them over its terms)
    const uint32_t* bt = base->df_text.data();
    bool bad = false;
    for (uint32_t t = 0; t < V; ++t) bad |= gt[t] < bt[t];
    if (gn) {
      const uint32_t* bn = base->df_name.data();
      for (uint32_t t = 0; t < V; ++t) bad |= gn[t] < bn[t];
    } else if (base->has_name) {
      bad = true;
    }
    for (uint32_t t = 0; t < VF; ++t) bad |= g->df_facet[t] < base->df_facet_local[t];
    if (bad) return fail(FG_EINVAL, "global doc frequencies below this snapshot's own");
  }
  auto ix = std::make_unique<fg_index>();
  ix->dev = base->dev;
  ix->mem.dev = base->dev;
  fgh::device_pools(base->dev, &ix->pool, &ix->pinned);
  // the base's structure (shared device arrays and host bookkeeping), its
  // bounds and the build statistics they are under
  static_cast<fgh::IndexStructure&>(*ix) = *base;
  static_cast<fgh::IndexBounds&>(*ix) = *base;
  fgh::set_stats(ix.get(), g->n_docs, g->tot_tokens, gt, gn, g->tot_facet_tokens, VF ? g->df_facet : nullptr, wts);
  fgh::relate_stats(ix.get());
  // deletions: the alive bitset (the base's device copy when unchanged), and
  // the docs dead now that ktop's selection counted alive (term_kth)
  std::vector<uint32_t> alive = alive_from_deleted(deleted, N);
  if (alive == base->h_alive.vec()) {
    ix->h_alive = base->h_alive;
    ix->alive_hold = base->alive_hold;
  } else if (alive.empty()) {
    ix->d.alive = nullptr;
  } else {
    HIPCHK(hipSetDevice(ix->dev));
    auto m = std::make_shared<DevAllocs>();
    m->dev = ix->dev;
    uint64_t b = 0;
    if (int rc = dev_upload(*m, alive.data(), alive.size(), const_cast<uint32_t**>(&ix->d.alive), &b)) return rc;
    ix->alive_hold = m;
    ix->h_alive = std::move(alive);
  }
  {
    uint64_t dead = 0;
    const auto& now = ix->h_alive.vec();
    const auto& then = ix->h_alive_b.vec();
    for (uint32_t w = 0; w < (N + 31) / 32; ++w) {
      const uint32_t valid = (w + 1) * 32 <= N ? 0xFFFFFFFFu : (1u << (N & 31)) - 1u;
      const uint32_t a0 = then.empty() ? valid : then[w], a1 = now.empty() ? valid : now[w];
      dead += (uint32_t)__builtin_popcount(a0 & ~a1 & valid);
    }
    ix->n_dead = (uint32_t)std::min<uint64_t>(dead, 0xFFFFFFFFu);
  }
  *out = ix.release();
  return FG_OK;
}

}  // namespace

// ================================================================ C ABI
extern "C" {

int fg_index_build_from_docs(fg_ctx* ctx, int dev, const fg_docs_input* in, fg_index** out) {
  return fg_index_build_from_docs_global(ctx, dev, in, nullptr, out);
}

int fg_docs_stats(const fg_docs_input* in, uint32_t* df_text, uint32_t* df_name, uint64_t* tot_tokens2) {
  if (!in || !df_text || !df_name || !tot_tokens2 || !in->text_off || (!in->text_tok && in->text_off[in->n_docs] > 0))
    return fail(FG_EINVAL, "bad arguments");
  const uint32_t N = in->n_docs, V = in->n_terms;
  const bool has_name_in = in->name_off && in->name_tok;
  const int T = hw_threads(in->threads);
  std::vector<std::vector<uint32_t>> dft(T), dfn(T);
  std::vector<uint64_t> tt(T, 0), tn(T, 0);
  std::atomic<bool> bad{false};
  parallel_ranges(N, T, [&](int t, uint32_t b, uint32_t e) {
    dft[t].assign(V, 0);
    dfn[t].assign(V, 0);
    std::vector<uint32_t> scratch;
    std::vector<std::pair<uint32_t, uint32_t>> runs;
    for (uint32_t d = b; d < e; ++d) {
      const uint64_t lt = in->text_off[d + 1] - in->text_off[d];
      tt[t] += lt;
      doc_runs(in->text_tok + in->text_off[d], lt, scratch, runs);
      for (auto& r : runs) {
        if (r.first >= V) { bad = true; return; }
        dft[t][r.first]++;
      }
      if (has_name_in) {
        const uint64_t ln = in->name_off[d + 1] - in->name_off[d];
        tn[t] += ln;
        doc_runs(in->name_tok + in->name_off[d], ln, scratch, runs);
        for (auto& r : runs) {
          if (r.first >= V) { bad = true; return; }
          dfn[t][r.first]++;
        }
      }
    }
  });
  if (bad) return fail(FG_EINVAL, "token id >= n_terms");
  std::fill(df_text, df_text + V, 0u);
  std::fill(df_name, df_name + V, 0u);
  tot_tokens2[0] = tot_tokens2[1] = 0;
  for (int t = 0; t < T; ++t) {
    if (dft[t].empty()) continue;
    for (uint32_t v = 0; v < V; ++v) {
      df_text[v] += dft[t][v];
      df_name[v] += dfn[t][v];
    }
    tot_tokens2[0] += tt[t];
    tot_tokens2[1] += tn[t];
  }
  return FG_OK;
}

int fg_docs_facet_stats(const fg_docs_input* in, uint32_t* df_facet, uint64_t* tot_facet) {
  if (!in || !tot_facet || (in->facet_off && in->n_facet_terms && !df_facet)) return fail(FG_EINVAL, "bad arguments");
  HostPostings hp;
  if (int rc = build_facets(in, hp, hw_threads(in->threads))) return rc;
  if (hp.n_fterms) std::copy(hp.df_facet.begin(), hp.df_facet.end(), df_facet);
  *tot_facet = hp.tot_f;
  return FG_OK;
}

int fg_index_build_from_docs_global(fg_ctx* ctx, int dev, const fg_docs_input* in, const fg_global_stats* g,
                                    fg_index** out) {
  if (!ctx || !in || !out || !in->text_off || (!in->text_tok && in->text_off[in->n_docs] > 0))
    return fail(FG_EINVAL, "bad arguments");
  if (!global_stats_ok(g, in->n_docs)) return fail(FG_EINVAL, "bad global statistics");
  if (in->n_docs == 0) return fail(FG_EINVAL, "empty index (n_docs == 0)");
  if (in->n_docs >= 0x7FFFFFFFu) return fail(FG_EINVAL, "n_docs must be < 2^31 (tantivy DocId)");
  g_bt.start();
  LocalDict L;
  if (int rc = local_dict(in, g, L)) return rc;
  const uint32_t V = in->n_terms;
  fg_index* ix = nullptr;
  if (L.tmap.empty()) {
    if (int rc = build_from_docs(ctx, dev, in, g, &ix)) return rc;
  } else {
    g_bt.mark("local dictionary");
    if (int rc = build_from_docs(ctx, dev, &L.in, g ? &L.g : nullptr, &ix)) return rc;
    ix->tmap = std::move(L.tmap);
    ix->n_vocab = V;
  }
  // (from the caller's tokens: a snapshot with its own dictionary still keeps vocabulary ids here)
  if (in->keep_positions)
    if (int rc = attach_positions(ix, in)) {
      fg_index_release(ix);
      return rc;
    }
  *out = ix;
  return FG_OK;
}

int fg_index_build(fg_ctx* ctx, int dev, const fg_index_input* in, fg_index** out) {
  return fg_index_build_global(ctx, dev, in, nullptr, out);
}

int fg_index_build_global(fg_ctx* ctx, int dev, const fg_index_input* in, const fg_global_stats* g, fg_index** out) {
  if (!ctx || !in || !out || !in->term_off || !in->fn_text) return fail(FG_EINVAL, "bad arguments");
  if (int rc = index_input_head(in, g)) return rc;
  g_bt.start();
  if (std::find(ctx->devs.begin(), ctx->devs.end(), dev) == ctx->devs.end())
    return fail(FG_EINVAL, "device %d not in context", dev);
  HostPostings hp;
  const uint32_t N = in->n_docs, V = in->n_terms;
  hp.n_docs = N;
  hp.n_terms = V;
  for (uint32_t t = 0; t < V; ++t)
    if (in->term_off[t + 1] < in->term_off[t]) return fail(FG_EINVAL, "term_off not monotone at %u", t);
  hp.off.assign(in->term_off, in->term_off + V + 1);
  const uint64_t P = hp.off[V];
  hp.doc.assign(in->doc, in->doc + P);
  hp.tf.resize(P);
  hp.df_text.assign(V, 0);
  hp.df_name.assign(V, 0);
  for (uint32_t t = 0; t < V; ++t) {
    for (uint64_t p = hp.off[t]; p < hp.off[t + 1]; ++p) {
      uint32_t tt = in->tf_text ? in->tf_text[p] : 0, tn = in->tf_name ? in->tf_name[p] : 0;
      if (!tt && !tn) return fail(FG_EINVAL, "posting %llu has tf 0 in both fields", (unsigned long long)p);
      if (hp.doc[p] >= N || (p > hp.off[t] && hp.doc[p] <= hp.doc[p - 1]))
        return fail(FG_EINVAL, "postings of term %u not strictly ascending / in range", t);
      hp.tf[p] = tt | (tn << 16);
      hp.df_text[t] += tt ? 1 : 0;
      hp.df_name[t] += tn ? 1 : 0;
    }
  }
  hp.fn_text.assign(in->fn_text, in->fn_text + N);
  if (in->fn_name) hp.fn_name.assign(in->fn_name, in->fn_name + N); else hp.fn_name.assign(N, 0);
  hp.tot[0] = in->tot_tokens[0];
  hp.tot[1] = in->tot_tokens[1];
  hp.has_name = hp.tot[1] > 0;
  hp.alive = alive_from_deleted(in->deleted, N);
  if (in->facet_term_off) {
    const uint32_t VF = in->n_facet_terms;
    hp.n_fterms = VF;
    hp.foff.assign(in->facet_term_off, in->facet_term_off + VF + 1);
    if (hp.foff[0] != 0 || (!in->facet_doc && hp.foff[VF] > 0)) return fail(FG_EINVAL, "bad facet postings");
    hp.fdoc.assign(in->facet_doc, in->facet_doc + hp.foff[VF]);
    hp.df_facet.assign(VF, 0);
    for (uint32_t t = 0; t < VF; ++t) {
      if (hp.foff[t + 1] < hp.foff[t]) return fail(FG_EINVAL, "facet_term_off not monotone at %u", t);
      for (uint64_t p = hp.foff[t]; p < hp.foff[t + 1]; ++p)
        if (hp.fdoc[p] >= N || (p > hp.foff[t] && hp.fdoc[p] <= hp.fdoc[p - 1]))
          return fail(FG_EINVAL, "facet postings of term %u not strictly ascending / in range", t);
      hp.df_facet[t] = (uint32_t)(hp.foff[t + 1] - hp.foff[t]);
    }
    hp.tot_f = in->tot_facet_tokens;
  }
  if (int rc = check_global_df(g, hp, "segment")) return rc;
  return finish_index(dev, hp, true, out, g);
}

int fg_index_build_positional(fg_ctx* ctx, int dev, const fg_index_input* in, const fg_positions_input* pos,
                              const fg_global_stats* g, fg_index** out) {
  // the checks of `in` that need no context, then those of `pos`: all host work, before the device is touched
  if (!in || !out || !in->term_off || !in->fn_text) return fail(FG_EINVAL, "bad arguments");
  if (int rc = index_input_head(in, g)) return rc;
  if (!pos) return fail(FG_EINVAL, "no positions given (fg_index_build_global builds a snapshot without them)");
  if (int rc = check_positions_input(in, pos)) return rc;
  fg_index* ix = nullptr;
  if (int rc = fg_index_build_global(ctx, dev, in, g, &ix)) return rc;
  if (int rc = attach_positions_postings(ix, in, pos)) {
    fg_index_release(ix);
    return rc;
  }
  *out = ix;
  return FG_OK;
}

int fg_index_positions_get(const fg_index* ix, int field, uint32_t doc0, uint32_t n_docs, uint64_t* off_out,
                           uint32_t* tok_out, uint64_t cap, uint64_t* n_tok) {
  if (!ix || !off_out || !n_tok || (cap && !tok_out)) return fail(FG_EINVAL, "bad arguments");
  if (field != FG_FIELD_TEXT && field != FG_FIELD_NAME) return fail(FG_EINVAL, "field must be text (0) or name (1)");
  if (!ix->has_positions) return fail(FG_EINVAL, "snapshot built without positions");
  const uint64_t* d_off = field == FG_FIELD_TEXT ? ix->d.fwd_off : ix->d.fwd_off_name;
  const uint32_t* d_fwd = field == FG_FIELD_TEXT ? ix->d.fwd : ix->d.fwd_name;
  if (!d_off || !d_fwd) return fail(FG_EINVAL, "snapshot has no forward index of field %d", field);
  if ((uint64_t)doc0 + n_docs > ix->n_docs) return fail(FG_EINVAL, "docs [%u, %u + %u) past the snapshot's %u", doc0, doc0, n_docs, ix->n_docs);
  HIPCHK(hipSetDevice(ix->dev));
  HIPCHK(hipMemcpyAsync(off_out, d_off + doc0, 8ull * (n_docs + 1ull), hipMemcpyDeviceToHost, kBuildStream));
  HIPCHK(hipStreamSynchronize(kBuildStream));
  const uint64_t first = off_out[0], n = off_out[n_docs] - first;
  for (uint32_t i = 0; i <= n_docs; ++i) off_out[i] -= first;
  *n_tok = n;
  if (n > cap) return fail(FG_EINVAL, "%llu positions, room for %llu", (unsigned long long)n, (unsigned long long)cap);
  if (n) {
    HIPCHK(hipMemcpyAsync(tok_out, d_fwd + first, 4 * n, hipMemcpyDeviceToHost, kBuildStream));
    HIPCHK(hipStreamSynchronize(kBuildStream));
  }
  return FG_OK;
}

int fg_index_rescore(const fg_index* base, const fg_global_stats* g, const uint8_t* deleted, fg_index** out) {
  g_bt.start();
  return rescore_one(base, g, deleted, out, nullptr);
}

int fg_index_rescore_many(const fg_index* const* bases, uint32_t n, const fg_global_stats* g,
                          const uint8_t* const* deleted, fg_index** outs) {
  if ((n && (!bases || !outs)) || !g || !g->df_text) return fail(FG_EINVAL, "bad arguments");
  uint32_t V = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (!bases[i]) return fail(FG_EINVAL, "NULL snapshot %u", i);
    if (bases[i]->tmap.empty()) V = std::max(V, bases[i]->n_terms);
    outs[i] = nullptr;
  }
  if (n == 0) return FG_OK;
  // the weights once for every snapshot on vocabulary ids (they depend on the
  // statistics only; a snapshot with its own dictionary gathers its own)
  fgh::Weights wts;
  g_bt.start();
  if (V) {
    std::vector<float> wt, wn, it, in;
    fgh::bm25_weights(g->n_docs, g->df_text, g->df_name, V, wt, wn, it, in);
    wts.wt = std::move(wt);
    wts.wn = std::move(wn);
    wts.it = std::move(it);
    wts.in = std::move(in);
  }
  g_bt.mark("rescore: shared weights");
  for (uint32_t i = 0; i < n; ++i) {
    const int rc = rescore_one(bases[i], g, deleted ? deleted[i] : nullptr, &outs[i], &wts);
    g_bt.mark(bases[i]->tmap.empty() ? "rescore: a snapshot" : "rescore: a snapshot (own dictionary)");
    if (rc) {
      const std::string e = fg_last_error();
      for (uint32_t j2 = 0; j2 < n; ++j2)
        if (outs[j2]) {
          fg_index_release(outs[j2]);
          outs[j2] = nullptr;
        }
      return fail(rc, "snapshot %u: %s", i, e.c_str());
    }
  }
  return FG_OK;
}

int fg_index_term_ladder(const fg_index* ix, float* out) {
  if (!ix || !out) return fail(FG_EINVAL, "bad arguments");
  static_assert(fg::kNumLadder == FG_LADDER_LEVELS, "fugu.h FG_LADDER_LEVELS");
  const uint32_t V = ix->n_terms;
  if (V == 0) return FG_OK;
  HIPCHK(hipSetDevice(ix->dev));
  // one temporary: the main K-th scores [V * kNumTopK], then the extra levels
  const size_t nm = (size_t)V * fg::kNumTopK, nx = (size_t)V * fg::kNumLadderExtra;
  AsyncTmp tmp;
  if (fgh::dev_malloc_async(&tmp.p, 4 * (nm + nx) + 16, kBuildStream) != hipSuccess)
    return fail(FG_EOOM, "hipMallocAsync(%zu) failed", 4 * (nm + nx));
  float* d = static_cast<float*>(tmp.p);
  HIPCHK(hipMemsetAsync(d, 0, 4 * (nm + nx), kBuildStream));
  // the posting scores under the snapshot's statistics (a temporary), then k_ktop with the extra levels
  fg::ScoreJob j{};
  AsyncTmp ptmp;
  if (int rc = score_postings(ix, j, nullptr, nullptr, ptmp)) return rc;
  j.alive = ix->d.alive;
  j.ktop = d;
  j.ladder = d + nm;
  if (int rc = ktop_pass(ix, j)) return rc;
  std::vector<float> h(nm + nx);
  HIPCHK(hipMemcpyAsync(h.data(), d, 4 * (nm + nx), hipMemcpyDeviceToHost, kBuildStream));
  HIPCHK(hipStreamSynchronize(kBuildStream));
  // interleave into ascending K per term
  uint32_t src[fg::kNumLadder];  // level l: (main?, index)
  for (uint32_t l = 0; l < fg::kNumLadder; ++l) {
    src[l] = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < fg::kNumTopK; ++i)
      if (fg::kTopKs[i] == fg::kLadderKs[l]) src[l] = i;
    for (uint32_t i = 0; i < fg::kNumLadderExtra; ++i)
      if (fg::kLadderExtra[i] == fg::kLadderKs[l]) src[l] = 0x10000u | i;
    if (src[l] == 0xFFFFFFFFu) return fail(FG_EINVAL, "ladder level %u unmapped", l);
  }
  // (vocabulary ids: a snapshot with its own dictionary scatters its terms, zeros elsewhere)
  const uint32_t* tm = ix->tmap.empty() ? nullptr : ix->tmap.data();
  if (tm) std::fill(out, out + (size_t)ix->n_vocab * fg::kNumLadder, 0.0f);
  for (uint32_t t = 0; t < V; ++t)
    for (uint32_t l = 0; l < fg::kNumLadder; ++l) {
      const uint32_t s = src[l];
      out[(size_t)(tm ? tm[t] : t) * fg::kNumLadder + l] = (s & 0x10000u) ? h[nm + (size_t)t * fg::kNumLadderExtra + (s & 0xFFFFu)]
                                                            : h[(size_t)t * fg::kNumTopK + s];
    }
  return FG_OK;
}

}  // extern "C"
