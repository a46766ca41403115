// libfugu host side: streams, pools, a snapshot's statistics, plan execution
// and the C ABI of include/fugu.h (snapshot build and rescore: build.cpp; batch
// planning: plan.cpp).
//
// The BM25 statistics follow tantivy 0.24.1 as fugu uses it (SURVEY.md
// Appendix A): N = max_doc (deleted docs included), avgdl = total tokens / N,
// idf = ln(1 + (N - df + 0.5) / (df + 0.5)), weight = idf * (1 + K1), tf cache
// K1 * ((1 - B) + B * FIELD_NORMS_TABLE[id] / avgdl).  They are computed here,
// on the host, in that operation order with the host libm, so the device only
// multiplies/divides precomputed f32 values (bit-identical to the CPU path).
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <functional>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fugu.h"
#include "fg_host.h"
#include "fg_internal.h"

namespace {
thread_local std::string g_err;
}  // namespace

int fgh::fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// shared with host.cpp so fg_last_error() reports host-side failures too
void fg_set_last_error(const std::string& msg) { g_err = msg; }
int fg_host_threads();  // below (hw_threads(0)), shared with host.cpp

namespace {

using fgh::fail;
using fgh::hw_threads;
using fgh::parallel_dynamic;
using fgh::parallel_ranges;
using fgh::plan_create_multi;  // plan.cpp

// ---------------------------------------------------------------- tantivy constants
constexpr float kK1 = 1.2f;
constexpr float kB = 0.75f;

struct FieldNormTable {
  uint32_t v[256];
  FieldNormTable() {
    uint32_t i = 0;
    for (; i <= 40; ++i) v[i] = i;
    uint64_t x = 40, step = 2;
    while (i < 256) {
      for (int j = 0; j < 8 && i < 256; ++j) { x += step; v[i++] = (uint32_t)x; }
      step <<= 1;
    }
  }
};
const FieldNormTable& fn_table() {
  static const FieldNormTable t;
  return t;
}
float bm25_idf(uint64_t df, uint64_t n_docs) {
  float x = ((float)(n_docs - df) + 0.5f) / ((float)df + 0.5f);
  return logf(1.0f + x);
}
float bm25_weight(uint64_t df, uint64_t n_docs) { return bm25_idf(df, n_docs) * (1.0f + kK1); }
void bm25_cache(float avgdl, float* out) {
  const uint32_t* t = fn_table().v;
  for (int i = 0; i < 256; ++i) out[i] = kK1 * ((1.0f - kB) + (kB * (float)t[i]) / avgdl);
}
// kernels.hip term_score on the host (same f32 operations; -ffp-contract=off)
float term_score_host(uint32_t tfp, uint32_t fn_t, uint32_t fn_n, float wt, float wn, const float* cache) {
  float s = 0.0f;
  const uint32_t tt = tfp & 0xFFFFu, tn = tfp >> 16;
  if (tt) {
    const float tf = (float)tt;
    s += wt * (tf / (tf + cache[fn_t]));
  }
  if (tn) {
    const float tf = (float)tn;
    s += wn * (tf / (tf + cache[256 + fn_n]));
  }
  return s;
}

}  // namespace

uint8_t fgh::fieldnorm_id(uint64_t n) {
  const uint32_t* t = fn_table().v;
  uint32_t x = n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
  return (uint8_t)(std::upper_bound(t, t + 256, x) - t - 1);
}

thread_local fgh::BuildTrace fgh::g_bt;
void fgh::BuildTrace::start() {
  on = getenv("FUGU_BUILD_TRACE") != nullptr;
  t = std::chrono::steady_clock::now();
}
void fgh::BuildTrace::mark(const char* what) {
  if (!on) return;
  const auto n = std::chrono::steady_clock::now();
  // @: the phase's end on the steady clock (ms; Python's time.monotonic), to line
  // phases up with other threads' events (tools/stall_trace.py)
  fprintf(stderr, "[fg build] %-24s %9.1f ms @%.3f\n", what, std::chrono::duration<double, std::milli>(n - t).count(),
          std::chrono::duration<double, std::milli>(n.time_since_epoch()).count());
  t = n;
}

// Host threads for snapshot builds and planning: FUGU_THREADS when set; else
// OMP_NUM_THREADS when it states a share above one (16 per GPU on the box; a
// launcher's default of 1 -- torchrun sets it for every rank -- is not a CPU
// share and is ignored); else the CPUs this process may run on (affinity,
// capped by the cgroup quota), at most 64.
int fgh::hw_threads(int req) {
  if (req > 0) return std::min(req, 256);
  static const int n = [] {
    int t = 0;
    if (const char* e = getenv("FUGU_THREADS")) t = atoi(e);
    if (t <= 0)
      if (const char* e = getenv("OMP_NUM_THREADS"))
        if (atoi(e) > 1) t = atoi(e);
    if (t <= 0) {
      cpu_set_t cs;
      t = sched_getaffinity(0, sizeof cs, &cs) == 0 ? CPU_COUNT(&cs) : (int)std::thread::hardware_concurrency();
      if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0};
        long long per = 0;
        if (fscanf(f, "%31s %lld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0)
          t = std::min<long long>(t, std::max<long long>(1, atoll(q) / per));
        fclose(f);
      }
      t = std::min(t, 64);
    }
    t = std::max(1, std::min(t, 256));
    if (getenv("FUGU_BUILD_TRACE")) fprintf(stderr, "[fg build] host threads: %d\n", t);
    return t;
  }();
  return n;
}
int fg_host_threads() { return hw_threads(0); }

// fgh::pool_post's threads: as many as the host threads builds use, started on
// first use, never destroyed (idle ones end with the process)
void fgh::pool_post(std::function<void()> job) {
  struct Pool {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::function<void()>> q;
  };
  static Pool* pool = [] {
    auto* p = new Pool;
    for (int i = 0, n = std::max(1, hw_threads(0) - 1); i < n; ++i)
      std::thread([p] {
        for (;;) {
          std::function<void()> j;
          {
            std::unique_lock<std::mutex> l(p->mu);
            p->cv.wait(l, [&] { return !p->q.empty(); });
            j = std::move(p->q.front());
            p->q.pop_front();
          }
          j();
        }
      }).detach();
    return p;
  }();
  {
    std::lock_guard<std::mutex> l(pool->mu);
    pool->q.push_back(std::move(job));
  }
  pool->cv.notify_one();
}

namespace fgh {
namespace {
std::mutex& cache_mu() {
  static std::mutex m;
  return m;
}
std::vector<DevCache*>& caches() {
  static std::vector<DevCache*> v;
  return v;
}
}  // namespace
DevCache::DevCache() {
  std::lock_guard<std::mutex> l(cache_mu());
  caches().push_back(this);
}
void DevCache::unregister_cache() {
  std::lock_guard<std::mutex> l(cache_mu());
  auto& v = caches();
  v.erase(std::remove(v.begin(), v.end(), this), v.end());
}
// Stream-ordered allocations (hipMallocAsync: scoring scratch, rescore
// weights) keep their memory in the device's default pool instead of returning
// it at every synchronisation (release threshold: no limit).  A hipMallocAsync
// that maps fresh memory held up a search kernel on another stream for ~1 ms
// (4 MiB) to ~8.6 ms (256 MiB); with the pool kept, 0.04 ms
// (tools/stall_probe.hip, profiles/r05/stall/probe_r05q.json).  The pools are
// trimmed with the other caches when an allocation fails.
std::mutex& pool_mu() {
  static std::mutex m;
  return m;
}
std::vector<int>& kept_pools() {
  static std::vector<int> v;
  return v;
}
void keep_async_pool(int dev) {
  std::lock_guard<std::mutex> l(pool_mu());
  auto& v = kept_pools();
  if (std::find(v.begin(), v.end(), dev) != v.end()) return;
  hipMemPool_t pool = nullptr;
  if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess && pool) {
    uint64_t thr = ~0ull;
    if (hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thr) != hipSuccess) (void)hipGetLastError();
  } else {
    (void)hipGetLastError();
  }
  v.push_back(dev);
}
void drop_all_cached() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  {
    std::lock_guard<std::mutex> l(cache_mu());
    for (DevCache* c : caches()) c->drop_cached();
  }
  {
    std::lock_guard<std::mutex> l(pool_mu());
    for (int d : kept_pools()) {
      hipMemPool_t pool = nullptr;
      if (hipDeviceGetDefaultMemPool(&pool, d) == hipSuccess && pool) (void)hipMemPoolTrimTo(pool, 0);
      (void)hipGetLastError();
    }
  }
  (void)hipSetDevice(dev);
}
void device_pools(int dev, std::shared_ptr<WsPool>* ws, std::shared_ptr<PinnedPool>* pin) {
  static std::mutex mu;
  static std::map<int, std::pair<std::weak_ptr<WsPool>, std::weak_ptr<PinnedPool>>> reg;
  std::lock_guard<std::mutex> l(mu);
  auto& e = reg[dev];
  *ws = e.first.lock();
  if (!*ws) {
    *ws = std::make_shared<WsPool>();
    (*ws)->dev = dev;
    e.first = *ws;
  }
  *pin = e.second.lock();
  if (!*pin) {
    *pin = std::make_shared<PinnedPool>(64ull << 20);
    e.second = *pin;
  }
}
hipError_t dev_malloc(void** p, size_t bytes) {
  const uint64_t t0 = commit_trace_on() ? now_ns() : 0;
  if (hipMalloc(p, bytes) == hipSuccess) {
    if (t0 && now_ns() - t0 > 200000) trace_span("alloc", "hipMalloc (> 0.2 ms)", t0);
    return hipSuccess;
  }
  (void)hipGetLastError();
  drop_all_cached();
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) (void)hipGetLastError();
  return e;
}
hipError_t dev_malloc_async(void** p, size_t bytes, hipStream_t s) {
  int dev = 0;
  if (hipGetDevice(&dev) == hipSuccess) keep_async_pool(dev);
  if (hipMallocAsync(p, bytes, s) == hipSuccess) return hipSuccess;
  (void)hipGetLastError();
  drop_all_cached();
  const hipError_t e = hipMallocAsync(p, bytes, s);
  if (e != hipSuccess) (void)hipGetLastError();
  return e;
}
}  // namespace fgh
namespace {

// Snapshot builds and rescores run on the calling thread's own stream (never
// the legacy null stream, which serialises with every other stream): a
// commit's rescores of the older segments, its new segment's build and the
// background merger's build run side by side.  Uploads are synchronous with
// the host (the sources may be freed right after).
// (a thread may point it at another stream: fg_index_rescore_many's workers
// use the device's background streams; a thread under fg_thread_background
// uses one of them for everything it builds)
thread_local hipStream_t tl_build_stream = nullptr;
thread_local int tl_background = 0;
hipStream_t background_stream(int dev, uint32_t i);
}  // namespace
hipStream_t fgh::build_stream() {
  if (tl_build_stream) return tl_build_stream;
  if (tl_background) {
    thread_local const uint32_t mine = [] {
      static std::atomic<uint32_t> next{0};
      return next.fetch_add(1);
    }();
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess)
      if (hipStream_t st = background_stream(dev, mine)) return st;
  }
  return hipStreamPerThread;
}
#define kBuildStream fgh::build_stream()

// Does the calling thread work in the background (fg_thread_background, or a
// rescore worker on a background stream)?
bool fgh::on_background() { return tl_background || tl_build_stream; }
// The workgroup cap of a background scoring's launches (fg::ScoreJob::grid_cap):
// FUGU_BG_GRID workgroups per CU (default kBgGridPerCu; 0: no cap).  With the
// K-th reuse (kth_reuse_bound) and one background stream, GET /search during
// commits p99 0.37 -> 0.25 ms, 1.5x its idle p99 (profiles/r05/stall/bg_j2/);
// before the reuse the cap had raised p99 (the capped k_ktop held its slots)
static constexpr uint32_t kBgGridPerCu = 2;
uint32_t fgh::bg_grid_cap(int dev) {
  if (!on_background()) return 0;
  static const uint32_t per_cu = [] {
    const char* e = getenv("FUGU_BG_GRID");
    return e && *e ? (uint32_t)std::max(0, atoi(e)) : kBgGridPerCu;
  }();
  if (!per_cu) return 0;
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0) {
    (void)hipGetLastError();
    return 0;
  }
  return per_cu * (uint32_t)n_cu;
}
namespace {

// A high-priority stream on device `dev` for the calling thread's searches (the
// search path's own: its kernels are dispatched ahead of a commit's builds on
// the same GPU).  Streams come from a fixed per-device pool (kSearchStreams),
// handed out round-robin at a thread's first search and kept in a thread_local
// -- a server whose worker threads come and go (tokio's spawn_blocking pool
// retires idle threads) reuses the pool's streams instead of creating one per
// thread without bound.  Work on one stream is ordered, so threads sharing a
// stream serialise only their own launches; 16 streams >> the hardware queues.
static constexpr uint32_t kSearchStreams = 16;
// alt: the thread's second stream (the pool's stream half way round from its
// own), for a batch whose second half overlaps the first (fg_search_sharded)
static hipStream_t search_stream(int dev, bool alt = false) {
  thread_local std::map<int, std::pair<hipStream_t, hipStream_t>> mine;
  auto it = mine.find(dev);
  if (it != mine.end()) return alt ? it->second.second : it->second.first;
  static std::mutex mu;
  static std::map<int, std::pair<std::vector<hipStream_t>, uint32_t>> pools;
  hipStream_t s = hipStreamPerThread, s2 = hipStreamPerThread;
  {
    std::lock_guard<std::mutex> l(mu);
    auto& pool = pools[dev];
    if (pool.first.empty()) {
      int cur = 0, least = 0, greatest = 0;
      (void)hipGetDevice(&cur);
      (void)hipSetDevice(dev);
      if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) greatest = 0;
      for (uint32_t i = 0; i < kSearchStreams; ++i) {
        hipStream_t x = nullptr;
        if (hipStreamCreateWithPriority(&x, hipStreamNonBlocking, greatest) != hipSuccess) {
          (void)hipGetLastError();
          x = hipStreamPerThread;
        }
        pool.first.push_back(x);
      }
      (void)hipSetDevice(cur);
    }
    const uint32_t i = pool.second++ % kSearchStreams;
    s = pool.first[i];
    s2 = pool.first[(i + kSearchStreams / 2) % kSearchStreams];
  }
  mine[dev] = {s, s2};
  return alt ? s2 : s;
}

// The background stream of a device (a db's segment builds and merges),
// created once at low priority (the searches' own are high priority).  ONE
// stream: a commit's device work queues behind itself instead of all hitting the
// GPU together (GET /search during commits p99 0.62 -> 0.37 ms at the same
// commit latency, profiles/r05/stall/bg_j2/).  (A CU-masked stream measured no
// better: the mask is not honoured on this platform, tools/stall_probe.hip,
// profiles/r05/stall/probe_r05p.json.)
hipStream_t background_stream(int dev, uint32_t) {
  static std::mutex mu;
  static std::map<int, hipStream_t> streams;
  std::lock_guard<std::mutex> l(mu);
  auto it = streams.find(dev);
  if (it != streams.end()) return it->second;
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(dev);
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
  hipStream_t st = nullptr;
  if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, least) != hipSuccess) {
    (void)hipGetLastError();
    st = nullptr;
  }
  (void)hipSetDevice(cur);
  streams[dev] = st;
  return st;
}

}  // namespace

int fgh::dev_upload_bytes(DevAllocs& m, const void* src, size_t n, void** out, uint64_t* bytes) {
  size_t b = std::max<size_t>(n, 16);
  void* p = nullptr;
  if (fgh::dev_malloc(&p, b) != hipSuccess) return fail(FG_EOOM, "hipMalloc(%zu) failed", b);
  m.ptrs.push_back(p);
  if (n) {
    HIPCHK(hipMemcpyAsync(p, src, n, hipMemcpyHostToDevice, kBuildStream));
    HIPCHK(hipStreamSynchronize(kBuildStream));
  }
  *out = p;
  *bytes += b;
  return FG_OK;
}

int fgh::UploadBatch::commit(DevAllocs& m, uint64_t* bytes) {
  constexpr size_t kStagePiece = 1u << 20, kStageMax = 128ull << 20;
  // process-wide: builds run on many threads (a commit's builder, the merger)
  static PinnedPool stage_pool(256ull << 20);
  void* p = nullptr;
  if (fgh::dev_malloc(&p, std::max<size_t>(total, 256)) != hipSuccess) return fail(FG_EOOM, "hipMalloc(%zu) failed", total);
  m.ptrs.push_back(p);
  // the arrays laid out in a pooled pinned staging buffer by all host threads,
  // then ONE copy: a small segment's arrays are sized by the vocabulary (~40 MB
  // for 2^20 terms), and pageable copies of them -- staged by the runtime,
  // beside a commit's rescores -- took ~16 ms of a 1000-doc segment's build
  // (a bulk build's arrays are larger than the pool keeps: pageable copies)
  PinnedLease pin(stage_pool, total <= kStageMax ? total : 0);
  const bool staged = pin.p && total <= kStageMax;
  if (staged) {
    struct Piece { char* dst; const char* src; size_t n; };
    std::vector<Piece> pieces;
    size_t o = 0;
    for (const E& e : es) {
      for (size_t b = 0; b < e.bytes; b += kStagePiece)
        pieces.push_back(Piece{static_cast<char*>(pin.p) + o + b, static_cast<const char*>(e.src) + b,
                               std::min(kStagePiece, e.bytes - b)});
      o += slot(e.bytes);
    }
    parallel_dynamic((uint32_t)pieces.size(), std::min<int>(hw_threads(0), (int)pieces.size()), 1,
                     [&](int, uint32_t b, uint32_t e) {
      for (uint32_t i = b; i < e; ++i) std::memcpy(pieces[i].dst, pieces[i].src, pieces[i].n);
    });
    HIPCHK(hipMemcpyAsync(p, pin.p, total, hipMemcpyHostToDevice, kBuildStream));
  }
  size_t o = 0;
  for (const E& e : es) {
    char* d = static_cast<char*>(p) + o;
    if (!staged && e.bytes) HIPCHK(hipMemcpyAsync(d, e.src, e.bytes, hipMemcpyHostToDevice, kBuildStream));
    *e.out = d;
    o += slot(e.bytes);
  }
  HIPCHK(hipStreamSynchronize(kBuildStream));
  *bytes += total;
  return FG_OK;
}

static int check_device(int dev) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(FG_ENODEV, "no HIP device visible");
  if (dev < 0 || dev >= n) return fail(FG_ENODEV, "device %d out of range (%d visible)", dev, n);
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, dev));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(FG_ENODEV, "device %d is %s; libfugu is built for gfx950 only", dev, prop.gcnArchName);
  return FG_OK;
}

// ---------------------------------------------------------------- statistics and bounds
// The statistics-dependent state of a snapshot is host-only: BM25 weights and
// tf caches (tantivy's f32 order with the host libm), read by the plans; the
// device forms the scores at query time.  The bound tables (maxima and K-th
// best scores the kernels prune with) are computed on the device once per
// structure under its build statistics.  `df_t`/`df_n`/`df_f`: the statistics'
// doc frequencies (global for a doc-sharded namespace).

// BM25 weights of terms [0, V) for statistics (Ns, df_t, df_n) (tantivy's f32 order)
// and their idfs (it, in: a phrase's weight sums them before the (1 + K1) factor)
void fgh::bm25_weights(uint64_t Ns, const uint32_t* df_t, const uint32_t* df_n, uint32_t V, std::vector<float>& wt,
                  std::vector<float>& wn, std::vector<float>& it, std::vector<float>& in) {
  wt.resize(V);
  wn.resize(V);
  it.resize(V);
  in.resize(V);
  parallel_ranges(V, hw_threads(0), [&](int, uint32_t b, uint32_t e) {
    for (uint32_t t = b; t < e; ++t) {
      it[t] = bm25_idf(df_t[t], Ns);
      in[t] = bm25_idf(df_n ? df_n[t] : 0u, Ns);
      wt[t] = it[t] * (1.0f + kK1);
      wn[t] = in[t] * (1.0f + kK1);
    }
  });
}

// The statistics of a snapshot (host only, tantivy's f32 order with the host
// libm): N, token totals, avgdl and the tf caches, the BM25 weights (`wts`:
// shared precomputed ones of the same statistics, or nullptr: computed here),
// the facet clause scores.  The device sees them only through plans (query-time
// scoring: DevPlan::q_wt / q_wn and the plan's copy of the caches).
void fgh::set_stats(fg_index* ix, uint64_t Ns, const uint64_t tot2[2], const uint32_t* df_t, const uint32_t* df_n,
               uint64_t tot_f, const uint32_t* df_f, const fgh::Weights* wts) {
  const uint32_t V = ix->n_terms;
  ix->n_stats = Ns;
  ix->tot[0] = tot2[0];
  ix->tot[1] = tot2[1];
  for (int f = 0; f < 2; ++f) {
    ix->avgdl[f] = (float)ix->tot[f] / (float)Ns;  // total_num_tokens as f32 / N as f32
    bm25_cache(ix->avgdl[f], ix->cache + 256 * f);
  }
  if (wts) {  // shared: at least V terms
    ix->w_text = wts->wt;
    ix->w_name = wts->wn;
    ix->idf_text = wts->it;
    ix->idf_name = wts->in;
  } else {
    std::vector<float> wt, wn, it, in;
    bm25_weights(Ns, df_t, df_n, V, wt, wn, it, in);
    ix->w_text = std::move(wt);
    ix->w_name = std::move(wn);
    ix->idf_text = std::move(it);
    ix->idf_name = std::move(in);
  }
  // facet field: Bm25Weight of a facet TermQuery (tf 1, no fieldnorms ->
  // FieldNormReader::constant(max_doc, 1) -> id 1, avg = total_num_tokens / N)
  const uint32_t VF = ix->n_fterms;
  ix->tot_f = tot_f;
  ix->df_facet.assign(df_f, df_f + VF);
  ix->fscore.assign(VF, 0.0f);
  if (ix->tot_f > 0) {
    float cf[256];
    ix->avgdl_f = (float)ix->tot_f / (float)Ns;
    bm25_cache(ix->avgdl_f, cf);
    ix->cache_f1 = cf[1];
    for (uint32_t t = 0; t < VF; ++t) ix->fscore[t] = bm25_weight(ix->df_facet[t], Ns) * (1.0f / (1.0f + ix->cache_f1));
  }
}

// How the current statistics relate to the build's (fg_index::same_stats,
// cup / cdn): a posting's score w * tf / (tf + c[fn]) changes by (w' / w) *
// (tf + c[fn]) / (tf + c'[fn]); over tf >= 1 the second factor lies between 1
// and its value at tf = 1, so per field it is bounded by the extremes over the
// fieldnorm ids of (1 + c) / (1 + c').
void fgh::relate_stats(fg_index* ix) {
  ix->same_stats = std::memcmp(ix->cache, ix->cache_b, sizeof ix->cache) == 0 &&
                   (ix->w_text.data() == ix->wb_text.data() || ix->w_text.vec() == ix->wb_text.vec()) &&
                   (ix->w_name.data() == ix->wb_name.data() || ix->w_name.vec() == ix->wb_name.vec());
  for (int f = 0; f < 2; ++f) {
    double up = 1.0, dn = 1.0;
    for (int fn = 0; fn < 256; ++fn) {
      const double q = (1.0 + (double)ix->cache_b[256 * f + fn]) / (1.0 + (double)ix->cache[256 * f + fn]);
      if (!std::isfinite(q)) continue;  // (a field without tokens: no posting scores in it)
      up = std::max(up, q);
      dn = std::min(dn, q);
    }
    ix->cup[f] = up;
    ix->cdn[f] = dn;
  }
}

// Per-term bounds under the CURRENT statistics from the build-time tables
// (shared by the planner, fg_index_term_kth and the byte models).
namespace fgh {
// f32 factors with rdn * s_build <= s_now <= rup * s_build for every posting of
// term t (relate_stats' extremes times the weight ratio, over the fields the term
// has postings in, with a 2^-19 margin for the f32 roundings of both scores);
// exactly 1 when the statistics are the build's
void term_ratio(const fg_index* ix, uint32_t t, float* rdn, float* rup) {
  *rdn = *rup = 1.0f;
  if (ix->same_stats || t >= ix->n_terms) return;
  double lo = HUGE_VAL, hi = 0.0;
  for (int f = 0; f < (ix->has_name ? 2 : 1); ++f) {
    if ((f == 0 ? ix->df_text[t] : ix->df_name[t]) == 0) continue;  // no posting scores in the field
    const double wb = f == 0 ? ix->wb_text[t] : ix->wb_name[t], wn = f == 0 ? ix->w_text[t] : ix->w_name[t];
    if (!(wb > 0.0)) continue;
    const double r = wn / wb;
    hi = std::max(hi, r * ix->cup[f]);
    lo = std::min(lo, r * ix->cdn[f]);
  }
  if (!(hi > 0.0) || !std::isfinite(lo)) return;
  const double m = std::ldexp(1.0, -19);
  const double u = hi * (1.0 + m), d = lo * (1.0 - m);
  float fu = (float)u, fd = (float)d;
  if ((double)fu < u) fu = std::nextafter(fu, HUGE_VALF);
  if ((double)fd > d) fd = std::nextafter(fd, 0.0f);
  *rup = fu;
  *rdn = std::max(fd, 0.0f);
}
// the largest current score of term t (an upper bound; exact without a statistics change)
float term_max_scaled(const fg_index* ix, uint32_t t, float rup) {
  if (t >= ix->n_terms) return 0.0f;
  if (rup == 1.0f) return ix->tmaxs[t];
  const double v = (double)ix->tmaxs[t] * rup;
  float f = (float)v;
  if ((double)f < v) f = std::nextafter(f, HUGE_VALF);
  return f;
}
float term_max_now(const fg_index* ix, uint32_t t) {
  if (t >= ix->n_terms) return 0.0f;
  float rdn, rup;
  term_ratio(ix, t, &rdn, &rup);
  return term_max_scaled(ix, t, rup);
}
// a lower bound of term t's K-th best current score over the alive docs, K the
// smallest stored level >= k (0: none): the build's K'-th best for the smallest
// stored K' >= K + n_dead (at most n_dead of those docs died since), times rdn;
// or the namespace-wide floor of a doc-sharded namespace's shard when higher
float term_kth_now(const fg_index* ix, uint32_t t, uint32_t k, bool with_floor) {
  if (t >= ix->n_terms) return 0.0f;
  float v = 0.0f;
  const uint64_t need = (uint64_t)k + ix->n_dead;
  for (uint32_t j = 0; j < fg::kNumTopK; ++j) {
    if (fg::kTopKs[j] < need) continue;
    float rdn, rup;
    term_ratio(ix, t, &rdn, &rup);
    const double x = (double)ix->ktop[(size_t)t * fg::kNumTopK + j] * rdn;
    v = (float)x;
    if ((double)v > x) v = std::nextafter(v, 0.0f);
    break;
  }
  if (!with_floor) return v;
  if (const std::shared_ptr<const std::vector<float>> floor = std::atomic_load(&ix->kth_floor))
    for (uint32_t j = 0; j < fg::kNumTopK; ++j) {
      if (fg::kTopKs[j] < k) continue;
      v = std::max(v, (*floor)[(size_t)t * fg::kNumTopK + j]);
      break;
    }
  return v;
}
}  // namespace fgh

// ================================================================ C ABI
extern "C" {

const char* fg_last_error(void) { return g_err.c_str(); }
const char* fg_version(void) { return "libfugu 0.4 (gfx950)"; }
int fg_abi_version(void) { return FG_ABI_VERSION; }

int fg_device_count(int* out) {
  if (!out) return fail(FG_EINVAL, "out is NULL");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *out = n;
  return FG_OK;
}

int fg_ctx_create(int ndev, const int* devs, fg_ctx** out) {
  if (!out || ndev < 0 || (ndev > 0 && !devs)) return fail(FG_EINVAL, "bad arguments");
  auto c = std::make_unique<fg_ctx>();
  if (ndev == 0) {
    int n = 0;
    fg_device_count(&n);
    if (n == 0) return fail(FG_ENODEV, "no HIP device visible");
    c->devs.push_back(0);
  } else {
    c->devs.assign(devs, devs + ndev);
  }
  for (int d : c->devs) {
    int rc = check_device(d);
    if (rc) return rc;
  }
  // fg_search_sharded moves each shard's top-k to the first shard's device
  // with hipMemcpyPeerAsync: direct xGMI transfers need peer access, so it is
  // enabled on every pair that supports it (already-enabled is fine).  A pair
  // without it still works (the runtime stages the copy through the host);
  // fg_ctx_peer_access reports which pairs are direct.  The caller's current
  // device is restored.
  int prev = 0;
  HIPCHK(hipGetDevice(&prev));
  for (int a : c->devs)
    for (int b : c->devs) {
      if (a == b) continue;
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can) {
        (void)hipGetLastError();
        continue;
      }
      if (hipSetDevice(a) != hipSuccess) break;
      const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
      (void)hipGetLastError();
      if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) c->peers.emplace_back(a, b);
    }
  (void)hipSetDevice(prev);
  *out = c.release();
  return FG_OK;
}

int fg_ctx_destroy(fg_ctx* ctx) {
  delete ctx;
  return FG_OK;
}

int fg_ctx_peer_access(const fg_ctx* ctx, int a, int b, int* enabled) {
  if (!ctx || !enabled) return fail(FG_EINVAL, "bad arguments");
  *enabled = std::find(ctx->peers.begin(), ctx->peers.end(), std::make_pair(a, b)) != ctx->peers.end() ? 1 : 0;
  return FG_OK;
}

int fg_thread_background(int on) {
  const int prev = tl_background;
  tl_background = on ? 1 : 0;
  return prev;
}

int fg_index_retain(fg_index* ix) {
  if (!ix) return fail(FG_EINVAL, "NULL index");
  ix->refs.fetch_add(1);
  return FG_OK;
}

int fg_index_release(fg_index* ix) {
  if (!ix) return FG_OK;
  if (ix->refs.fetch_sub(1) == 1) delete ix;
  return FG_OK;
}

int fg_index_stats_get(const fg_index* ix, fg_index_stats* o) {
  if (!ix || !o) return fail(FG_EINVAL, "bad arguments");
  o->n_docs = ix->n_docs;
  o->n_terms = ix->n_vocab;
  o->n_postings = ix->n_postings;
  o->device_bytes = ix->device_bytes;
  o->tot_tokens[0] = ix->tot[0];
  o->tot_tokens[1] = ix->tot[1];
  o->avgdl[0] = ix->avgdl[0];
  o->avgdl[1] = ix->avgdl[1];
  o->has_name = ix->has_name;
  o->device = ix->dev;
  o->n_facet_terms = ix->n_fterms;
  o->tot_facet_tokens = ix->tot_f;
  o->n_dense_f32 = ix->n_dense;
  o->n_rank_terms = ix->n_rank;
  o->n_sparse_rank_terms = ix->n_rank - ix->d.n_prank;
  o->has_positions = ix->has_positions ? 1u : 0u;
  o->rank_bytes = 8ull * ix->d.n_prank * ix->d.rank_words +
                  8ull * (ix->n_rank - ix->d.n_prank) * ix->d.srank_blocks + 8ull * ix->n_srank_words;
  return FG_OK;
}

int fg_index_doctab_get(const fg_index* ix, uint32_t* n_terms, uint64_t* bytes) {
  if (!ix) return fail(FG_EINVAL, "bad arguments");
  if (n_terms) *n_terms = (uint32_t)ix->dtab_map.size();
  if (bytes) *bytes = ix->dtab_bytes;
  return FG_OK;
}

int fg_index_doctab8_get(const fg_index* ix, uint32_t* n_terms, uint64_t* bytes) {
  if (!ix) return fail(FG_EINVAL, "bad arguments");
  if (n_terms) *n_terms = (uint32_t)ix->dtab8_map.size();
  if (bytes) *bytes = ix->dtab8_bytes;
  return FG_OK;
}

int fg_index_bands_get(const fg_index* ix, uint32_t* n_terms, uint64_t* bytes) {
  if (!ix) return fail(FG_EINVAL, "bad arguments");
  if (n_terms) *n_terms = (uint32_t)ix->band_map.size();
  if (bytes) *bytes = ix->band_bytes;
  return FG_OK;
}

int fg_index_band_read(const fg_index* ix, uint32_t term, int source, uint32_t* doc, float* score, uint64_t cap,
                       float* cmax, uint32_t* cuts, uint64_t* n) {
  if (!ix || !n) return fail(FG_EINVAL, "bad arguments");
  *n = 0;
  term = fgh::local_term(ix, term);
  if (term >= ix->n_terms) return FG_OK;
  const uint32_t b = fgh::band_slot(*ix, term);
  if (!b) return FG_OK;
  const uint64_t df = ix->off[term + 1] - ix->off[term], nch = (df + fg::kChunk - 1) / fg::kChunk;
  *n = df;
  if ((doc || score || cmax) && cap < df) return fail(FG_EINVAL, "%llu postings, room for %llu", (unsigned long long)df, (unsigned long long)cap);
  HIPCHK(hipSetDevice(ix->dev));
  const uint32_t* d_doc = source ? ix->d.doc + ix->off[term] : ix->d.bdoc + ix->band_off[b - 1];
  const float* d_sc = source ? ix->d.psc + ix->off[term] : ix->d.bpsc + ix->band_off[b - 1];
  if (doc) HIPCHK(hipMemcpy(doc, d_doc, 4 * df, hipMemcpyDeviceToHost));
  if (score) HIPCHK(hipMemcpy(score, d_sc, 4 * df, hipMemcpyDeviceToHost));
  if (cmax) HIPCHK(hipMemcpy(cmax, ix->d.bcmax + ix->band_c0[b - 1], 4 * nch, hipMemcpyDeviceToHost));
  if (cuts) std::copy(ix->band_lo.begin() + (size_t)(b - 1) * (fg::kBandTiers - 1), ix->band_lo.begin() + (size_t)b * (fg::kBandTiers - 1), cuts);
  return FG_OK;
}

uint64_t fg_index_df(const fg_index* ix, int field, uint32_t term) {
  if (ix && field == FG_FIELD_FACET) return term < ix->n_fterms ? ix->df_facet[term] : 0;
  if (!ix) return 0;
  term = fgh::local_term(ix, term);
  if (term >= ix->n_terms) return 0;
  if (field == FG_FIELD_TEXT) return ix->df_text[term];
  if (field == FG_FIELD_NAME) return ix->df_name[term];
  return ix->off[term + 1] - ix->off[term];
}

int fg_index_term_kth(const fg_index* ix, uint32_t term, float* out) {
  if (!ix || !out) return fail(FG_EINVAL, "bad arguments");
  static_assert(fg::kNumTopK == 5, "fugu.h documents five K");
  term = fgh::local_term(ix, term);
  for (uint32_t k = 0; k < fg::kNumTopK; ++k) out[k] = fgh::term_kth_now(ix, term, fg::kTopKs[k], false);
  return FG_OK;
}

int fg_kth_floor_combine(uint32_t n_shards, uint32_t n_terms, const float* const* ladders, float* out) {
  if (!out || (n_shards && !ladders) || (n_terms && n_shards == 0)) return fail(FG_EINVAL, "bad arguments");
  for (uint32_t s = 0; s < n_shards; ++s)
    if (!ladders[s]) return fail(FG_EINVAL, "NULL ladder of shard %u", s);
  constexpr uint32_t L = fg::kNumLadder;
  fgh::parallel_dynamic(n_terms, fgh::hw_threads(0), 8192, [&](int, uint32_t b, uint32_t e) {
    std::vector<std::pair<float, uint32_t>> c;  // (score, shard * L + level)
    std::vector<uint32_t> cur(n_shards);        // the largest K of each shard at or above the sweep
    for (uint32_t t = b; t < e; ++t) {
      c.clear();
      for (uint32_t s = 0; s < n_shards; ++s)
        for (uint32_t l = 0; l < L; ++l) {
          const float v = ladders[s][(size_t)t * L + l];
          if (v > 0.0f) c.emplace_back(v, s * L + l);
        }
      std::sort(c.begin(), c.end(), [](const auto& x, const auto& y) { return x.first > y.first; });
      std::fill(cur.begin(), cur.end(), 0u);
      uint64_t total = 0;  // docs known to score >= the sweep's score
      float res[fg::kNumTopK] = {0, 0, 0, 0, 0};
      uint32_t next = 0;
      for (size_t i = 0; i < c.size() && next < fg::kNumTopK;) {
        const float x = c[i].first;
        for (; i < c.size() && c[i].first == x; ++i) {  // every level scoring exactly x counts at x
          const uint32_t s = c[i].second / L, K = fg::kLadderKs[c[i].second % L];
          if (K > cur[s]) {
            total += K - cur[s];
            cur[s] = K;
          }
        }
        for (; next < fg::kNumTopK && total >= fg::kTopKs[next]; ++next) res[next] = x;
      }
      for (uint32_t k = 0; k < fg::kNumTopK; ++k) out[(size_t)t * fg::kNumTopK + k] = res[k];
    }
  });
  return FG_OK;
}

int fg_index_set_kth_floor(fg_index* ix, const float* floor, uint32_t n_terms) {
  if (!ix) return fail(FG_EINVAL, "NULL index");
  std::shared_ptr<const std::vector<float>> f;
  if (floor) {
    if (n_terms != ix->n_vocab) return fail(FG_EINVAL, "floor of %u terms for a snapshot of %u", n_terms, ix->n_vocab);
    if (ix->tmap.empty()) {
      f = std::make_shared<const std::vector<float>>(floor, floor + (size_t)n_terms * fg::kNumTopK);
    } else {  // gathered to local ids
      std::vector<float> v((size_t)ix->n_terms * fg::kNumTopK);
      for (uint32_t t = 0; t < ix->n_terms; ++t)
        std::copy(floor + (size_t)ix->tmap[t] * fg::kNumTopK, floor + (size_t)(ix->tmap[t] + 1) * fg::kNumTopK,
                  v.begin() + (size_t)t * fg::kNumTopK);
      f = std::make_shared<const std::vector<float>>(std::move(v));
    }
  }
  std::atomic_store(&ix->kth_floor, f);
  return FG_OK;
}

int fg_index_bm25(const fg_index* ix, uint32_t term, float* w_text, float* w_name, float* cache512) {
  if (!ix) return fail(FG_EINVAL, "NULL index");
  term = fgh::local_term(ix, term);
  if (term < ix->n_terms) {
    if (w_text) *w_text = ix->w_text[term];
    if (w_name) *w_name = ix->w_name[term];
  } else {
    if (w_text) *w_text = bm25_weight(0, ix->n_stats);
    if (w_name) *w_name = bm25_weight(0, ix->n_stats);
  }
  if (cache512) std::memcpy(cache512, ix->cache, sizeof ix->cache);
  return FG_OK;
}

// the kernels of a planned batch on stream s, or of one part of it: the k_disj
// items [from, to) of its sweep (fractions of the k_disj range, in sweep order:
// every query's first docs first).  The first part (from = 0) zeroes the plan's
// state and runs k_fmask + k_conj, the last (to = 1) k_scan + k_final;
// out_shard != nullptr: a multi-snapshot plan's merged select
static int execute_impl(fg_plan* p, hipStream_t s, float* os, uint32_t* od, uint32_t* on, uint32_t* oshard,
                        double from = 0.0, double to = 1.0) {
  HIPCHK(hipSetDevice(p->ix->dev));
  const bool first = from <= 0.0, last = to >= 1.0;
  if (first && !p->d.n_peers) {  // (with peers: fg_plan_reset, ordered before every peer's execute)
    if (p->zeroed) p->zeroed = false;  // the first execute after the upload
    else HIPCHK(hipMemsetAsync(p->zero_region, 0, p->zero_bytes, s));
  }
  hipEvent_t ev[3] = {};
  if (p->profile) {
    for (auto& e : ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(ev[0], s));
  }
  if (first && p->d.f.n_chunks) HIPCHK(fg::launch_fmask(p->d0, p->d, s));
  if (first && p->d.n_conj) HIPCHK(fg::launch_conj(p->d0, p->d, s));
  const uint32_t nd = p->d.total_chunks - p->d.n_conj;
  const uint32_t a = first ? 0u : (uint32_t)std::min<double>(nd, std::llround(from * nd));
  const uint32_t b = last ? nd : (uint32_t)std::min<double>(nd, std::llround(to * nd));
  if (b > a) HIPCHK(fg::launch_disj(p->d0, p->d, s, a, b - a));
  if (last && p->d.n_scan) HIPCHK(fg::launch_scan(p->d0, p->d, s));
  if (last && p->d.n_phrase) HIPCHK(fg::launch_phrase(p->d0, p->d, s));
  if (last && p->d.n_bphrase) HIPCHK(fg::launch_bphrase(p->d0, p->d, s));
  if (last && p->d.n_group) HIPCHK(fg::launch_group(p->d0, p->d, s));
  if (last && p->d.n_gphrase) HIPCHK(fg::launch_gphrase(p->d0, p->d, s));
  if (last && p->d.n_mgroup) HIPCHK(fg::launch_mgroup(p->d0, p->d, s));
  if (last && p->d.n_field) HIPCHK(fg::launch_field(p->d0, p->d, s));
  if (last && p->d.n_fphrase) HIPCHK(fg::launch_fphrase(p->d0, p->d, s));
  if (p->profile) HIPCHK(hipEventRecord(ev[1], s));
  if (last) HIPCHK(fg::launch_final(p->d, os, od, on, s, oshard));
  if (p->profile) {
    HIPCHK(hipEventRecord(ev[2], s));
    p->pending.insert(p->pending.end(), ev, ev + 3);
  }
  p->last_stream = s;
  p->last_stream_used = true;
  return FG_OK;
}

int fg_plan_execute(fg_plan* p, void* stream, float* d_out_score, uint32_t* d_out_doc, uint32_t* d_out_n) {
  if (!p) return fail(FG_EINVAL, "NULL plan");
  return execute_impl(p, static_cast<hipStream_t>(stream), d_out_score ? d_out_score : p->own_score,
                      d_out_doc ? d_out_doc : p->own_doc, d_out_n ? d_out_n : p->own_n, nullptr);
}

// A multi-snapshot plan straight to the merged top-k of every batch query: the
// kernels of fg_plan_execute, then ONE k_final over all slots of each query
// (keys shifted by the snapshots' bases) in place of per-slot lists + merge
int fg_plan_execute_merged(fg_plan* p, void* stream, float* d_out_score, uint32_t* d_out_doc, uint32_t* d_out_shard,
                           uint32_t* d_out_n) {
  if (!p || !d_out_score || !d_out_doc || !d_out_shard || !d_out_n) return fail(FG_EINVAL, "bad arguments");
  if (p->n_segs < 2 || !p->d.seg_base)
    return fail(FG_EUNSUPPORTED, "not a multi-snapshot plan over < 2^32 docs (use fg_plan_execute + fg_merge_shards)");
  return execute_impl(p, static_cast<hipStream_t>(stream), d_out_score, d_out_doc, d_out_n, d_out_shard);
}

// One part of a plan's k_disj sweep (fugu.h): doc-sharded namespaces over
// several devices or processes exchange their per-query score histograms
// between the parts, so every shard's later items prune with the counts of all
// shards' earlier ones (what linked plans share through memory on one device)
int fg_plan_execute_part(fg_plan* p, void* stream, double from, double to, float* d_out_score, uint32_t* d_out_doc,
                         uint32_t* d_out_shard, uint32_t* d_out_n) {
  if (!p) return fail(FG_EINVAL, "NULL plan");
  if (!(from >= 0.0 && from < to && to <= 1.0)) return fail(FG_EINVAL, "part [%g, %g) not inside [0, 1)", from, to);
  // parts in sweep order, each starting where the last one ended (the first
  // zeroes the plan's state, the last runs the final select)
  if (from > 0.0 && from != p->part_next)
    return fail(FG_EINVAL, "part [%g, %g) does not continue the plan's sweep (next part starts at %g)", from, to,
                p->part_next);
  if (d_out_shard && (p->n_segs < 2 || !p->d.seg_base))
    return fail(FG_EUNSUPPORTED, "merged select: not a multi-snapshot plan over < 2^32 docs");
  if (d_out_shard && (!d_out_score || !d_out_doc || !d_out_n)) return fail(FG_EINVAL, "merged select needs every output");
  const int rc = execute_impl(p, static_cast<hipStream_t>(stream), d_out_score ? d_out_score : p->own_score,
                              d_out_doc ? d_out_doc : p->own_doc, d_out_n ? d_out_n : p->own_n, d_out_shard, from, to);
  if (rc == FG_OK) p->part_next = to >= 1.0 ? 0.0 : to;
  return rc;
}

int fg_plan_set_peers(fg_plan* p, fg_plan* const* peers, uint32_t n) {
  if (!p || (n && !peers)) return fail(FG_EINVAL, "bad arguments");
  if (n > FG_MAX_PEERS) return fail(FG_EUNSUPPORTED, "%u peers (> FG_MAX_PEERS = %d)", n, FG_MAX_PEERS);
  for (uint32_t i = 0; i < n; ++i) {
    const fg_plan* o = peers[i];
    if (!o || o == p) return fail(FG_EINVAL, "peer %u: NULL or the plan itself", i);
    if (o->nq_batch != p->nq_batch || o->k != p->k) return fail(FG_EINVAL, "peer %u plans another batch or k", i);
    if (o->h_lo.size() != p->h_lo.size()) return fail(FG_EINVAL, "peer %u: another number of query slots", i);
    if (o->ix->dev != p->ix->dev) {
      int ok = 0;
      HIPCHK(hipDeviceCanAccessPeer(&ok, p->ix->dev, o->ix->dev));
      if (!ok) return fail(FG_EUNSUPPORTED, "device %d cannot reach peer %u's device %d", p->ix->dev, i, o->ix->dev);
    }
  }
  p->d.n_peers = n;
  for (uint32_t i = 0; i < n; ++i) {
    p->d.peer_hist[i] = peers[i]->d.hist;
    p->d.peer_thr[i] = peers[i]->d.thresh;
  }
  if (n) p->d.pub_mask = 0xFFFFFFFF00000000ull;  // score-only: the peers' docs are other docs
  return FG_OK;
}

int fg_plan_ipc_export(const fg_plan* p, fg_plan_ipc* out) {
  if (!p || !out) return fail(FG_EINVAL, "bad arguments");
  const char* ws = static_cast<const char*>(p->ws);
  const char* th = reinterpret_cast<const char*>(p->d.thresh);
  const char* hi = reinterpret_cast<const char*>(p->d.hist);
  if (th < ws || th >= ws + p->ws_got || hi < ws || hi >= ws + p->ws_got)
    return fail(FG_EUNSUPPORTED, "the plan's thresholds are another plan's (linked): export that plan");
  std::memset(out, 0, sizeof *out);
  hipIpcMemHandle_t h;
  HIPCHK(hipSetDevice(p->ix->dev));
  HIPCHK(hipIpcGetMemHandle(&h, p->ws));
  static_assert(sizeof h <= sizeof out->handle, "fg_plan_ipc::handle");
  std::memcpy(out->handle, &h, sizeof h);
  out->thresh_off = (uint64_t)(th - ws);
  out->hist_off = (uint64_t)(hi - ws);
  out->n_queries = p->nq_batch;
  out->k = p->k;
  out->device = p->ix->dev;
  return FG_OK;
}

int fg_plan_set_ipc_peers(fg_plan* p, const fg_plan_ipc* peers, uint32_t n) {
  if (!p || (n && !peers)) return fail(FG_EINVAL, "bad arguments");
  if (n > FG_MAX_PEERS) return fail(FG_EUNSUPPORTED, "%u peers (> FG_MAX_PEERS = %d)", n, FG_MAX_PEERS);
  for (uint32_t i = 0; i < n; ++i)
    if (peers[i].n_queries != p->nq_batch || peers[i].k != p->k) return fail(FG_EINVAL, "peer %u plans another batch or k", i);
  HIPCHK(hipSetDevice(p->ix->dev));
  std::vector<void*> maps;
  for (uint32_t i = 0; i < n; ++i) {
    hipIpcMemHandle_t h;
    std::memcpy(&h, peers[i].handle, sizeof h);
    void* base = nullptr;
    if (hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
      (void)hipGetLastError();
      for (void* m : maps) (void)hipIpcCloseMemHandle(m);
      return fail(FG_EHIP, "peer %u: hipIpcOpenMemHandle failed", i);
    }
    maps.push_back(base);
  }
  for (void* m : p->ipc_maps) (void)hipIpcCloseMemHandle(m);
  p->ipc_maps = maps;
  p->d.n_peers = n;
  for (uint32_t i = 0; i < n; ++i) {
    p->d.peer_thr[i] = reinterpret_cast<uint64_t*>(static_cast<char*>(maps[i]) + peers[i].thresh_off);
    p->d.peer_hist[i] = reinterpret_cast<uint32_t*>(static_cast<char*>(maps[i]) + peers[i].hist_off);
  }
  if (n) p->d.pub_mask = 0xFFFFFFFF00000000ull;
  return FG_OK;
}

int fg_plan_reset(fg_plan* p, void* stream) {
  if (!p) return fail(FG_EINVAL, "NULL plan");
  HIPCHK(hipSetDevice(p->ix->dev));
  HIPCHK(hipMemsetAsync(p->zero_region, 0, p->zero_bytes, static_cast<hipStream_t>(stream)));
  p->zeroed = false;
  return FG_OK;
}

static_assert(fg::kQBins == FG_HIST_BINS, "fugu.h's histogram size");
static_assert(fg::kMaxPeers == FG_MAX_PEERS, "fugu.h's peer count");

int fg_plan_hist_span(const fg_plan* p, uint32_t* lo, uint32_t* hi) {
  if (!p || !lo || !hi) return fail(FG_EINVAL, "bad arguments");
  const uint32_t nb = p->nq_batch;
  for (uint32_t i = 0; i < nb; ++i) {
    const bool any = i < p->h_any.size() && p->h_any[i];
    lo[i] = any ? p->h_lo[i] : 0u;
    hi[i] = any ? p->h_hi[i] : 0u;
  }
  return FG_OK;
}

int fg_plan_set_hist_span(fg_plan* p, const uint32_t* lo, const uint32_t* hi) {
  if (!p || !lo || !hi) return fail(FG_EINVAL, "bad arguments");
  const uint32_t nb = p->nq_batch, S = p->n_segs;
  if (p->h_lo.size() < (size_t)nb * S || p->h_hi.size() < (size_t)nb * S)
    return fail(FG_EUNSUPPORTED, "a linked plan's bins are redrawn by fg_plan_link");
  std::vector<uint32_t> L(p->nq), SH(p->nq);
  for (uint32_t s = 0; s < S; ++s)
    for (uint32_t i = 0; i < nb; ++i) {
      const size_t v = (size_t)s * nb + i;
      // (both 0: no shard has work for the query, keep the plan's own bins)
      const bool own = lo[i] == 0 && hi[i] == 0;
      const fgh::Bins b = own ? fgh::union_bins(p->h_lo[v], p->h_hi[v]) : fgh::union_bins(lo[i], hi[i]);
      p->h_lo[v] = b.lo;
      p->h_hi[v] = b.hi;
      L[v] = b.lo;
      SH[v] = b.shift;
    }
  HIPCHK(hipSetDevice(p->ix->dev));
  if (p->pin) HIPCHK(hipStreamSynchronize(p->up_stream));  // an upload still in flight would overwrite them
  if (p->nq) {
    HIPCHK(hipMemcpy(const_cast<uint32_t*>(p->d.q_hlo), L.data(), 4ull * p->nq, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(const_cast<uint32_t*>(p->d.q_hsh), SH.data(), 4ull * p->nq, hipMemcpyHostToDevice));
  }
  return FG_OK;
}

int fg_plan_hist_copy(fg_plan* p, void* stream, uint32_t* d_buf, int into_plan) {
  if (!p || !d_buf) return fail(FG_EINVAL, "bad arguments");
  HIPCHK(hipSetDevice(p->ix->dev));
  const size_t bytes = 4ull * p->nq_batch * fg::kQBins;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (into_plan) HIPCHK(hipMemcpyAsync(p->d.hist, d_buf, bytes, hipMemcpyDeviceToDevice, s));
  else HIPCHK(hipMemcpyAsync(d_buf, p->d.hist, bytes, hipMemcpyDeviceToDevice, s));
  return FG_OK;
}

int fg_plan_results(fg_plan* p, float* out_score, uint32_t* out_doc, uint32_t* out_n) {
  if (!p) return fail(FG_EINVAL, "NULL plan");
  HIPCHK(hipSetDevice(p->ix->dev));
  // copies on the plan's stream (a per-thread stream under fg_search_batch), then wait for it
  const size_t nk = (size_t)p->nq * p->k;
  hipStream_t s = p->last_stream;
  // own_score, own_doc, own_n are consecutive in the workspace: one D2H into a
  // pinned buffer, then host copies (small batches: the batch-of-one latency)
  const char* first = reinterpret_cast<const char*>(p->own_score);
  const size_t span = reinterpret_cast<const char*>(p->own_n) + 4ull * p->nq - first;
  if (span <= (4ull << 20)) {
    PinnedLease pin(*p->ix->pinned, span);
    if (pin.p) {
      HIPCHK(hipMemcpyAsync(pin.p, first, span, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      const char* h = static_cast<const char*>(pin.p);
      if (out_score) std::memcpy(out_score, h, 4 * nk);
      if (out_doc) std::memcpy(out_doc, h + (reinterpret_cast<const char*>(p->own_doc) - first), 4 * nk);
      if (out_n) std::memcpy(out_n, h + (reinterpret_cast<const char*>(p->own_n) - first), 4ull * p->nq);
      return FG_OK;
    }
  }
  if (out_score) HIPCHK(hipMemcpyAsync(out_score, p->own_score, 4 * nk, hipMemcpyDeviceToHost, s));
  if (out_doc) HIPCHK(hipMemcpyAsync(out_doc, p->own_doc, 4 * nk, hipMemcpyDeviceToHost, s));
  if (out_n) HIPCHK(hipMemcpyAsync(out_n, p->own_n, 4ull * p->nq, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return FG_OK;
}

int fg_plan_info_get(const fg_plan* p, fg_plan_info* o) {
  if (!p || !o) return fail(FG_EINVAL, "bad arguments");
  o->n_queries = p->nq;
  o->k = p->k;
  o->total_chunks = p->total_chunks;
  o->workspace_bytes = p->ws_bytes;
  return FG_OK;
}

int fg_plan_profile(fg_plan* p, int enable) {
  if (!p) return fail(FG_EINVAL, "NULL plan");
  p->profile = enable != 0;
  return FG_OK;
}

int fg_plan_kernel_ms(fg_plan* p, double* ms_out, uint32_t* n_out) {
  if (!p) return fail(FG_EINVAL, "NULL plan");
  HIPCHK(hipSetDevice(p->ix->dev));
  for (size_t i = 0; i + 2 < p->pending.size(); i += 3) {
    HIPCHK(hipEventSynchronize(p->pending[i + 2]));
    for (int kx = 0; kx < 2; ++kx) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, p->pending[i + kx], p->pending[i + kx + 1]));
      p->ms[kx] += ms;
    }
    p->n_prof++;
  }
  for (hipEvent_t e : p->pending) (void)hipEventDestroy(e);
  p->pending.clear();
  if (ms_out) for (int kx = 0; kx < 2; ++kx) ms_out[kx] = p->ms[kx];
  if (n_out) *n_out = p->n_prof;
  p->ms[0] = p->ms[1] = 0;
  p->n_prof = 0;
  return FG_OK;
}

int fg_plan_diag(fg_plan* p, uint64_t* out, size_t n_words, uint32_t* cand_cnt) {
  if (!p) return fail(FG_EINVAL, "NULL plan");
  HIPCHK(hipSetDevice(p->ix->dev));
  HIPCHK(hipStreamSynchronize(p->last_stream));
  if (cand_cnt) HIPCHK(hipMemcpy(cand_cnt, p->d.cand_cnt, 4ull * p->nq, hipMemcpyDeviceToHost));
  if (out && n_words) {
    if (!p->d.diag) return fail(FG_EUNSUPPORTED, "not a diagnostic build (-DFG_DIAG)");
    HIPCHK(hipMemcpy(out, p->d.diag, 8 * std::min(n_words, p->diag_words), hipMemcpyDeviceToHost));
  }
  return FG_OK;
}

// Diagnostic (fg_host.h; tools/conj_threshold_ceiling.py): every slot of batch
// query i starts from the lowest key with score[i] (plan_host's convention for a
// single list's starting threshold; 0: none).  The bins stay as planned.
int fg_plan_seed_thr0(fg_plan* p, const float* score, uint32_t n) {
  if (!p || !score || n != p->nq_batch) return fail(FG_EINVAL, "bad arguments");
  std::vector<uint64_t> t((size_t)p->nq);
  for (uint32_t v = 0; v < p->nq; ++v) {
    const float s = score[v % p->nq_batch];
    t[v] = s > 0.0f ? fg::make_key(s, 0xFFFFFFFFu) : 0ull;
  }
  HIPCHK(hipSetDevice(p->ix->dev));
  if (p->pin) HIPCHK(hipStreamSynchronize(p->up_stream));  // an upload still in flight would overwrite them
  if (p->last_stream_used) HIPCHK(hipStreamSynchronize(p->last_stream));
  if (p->nq) HIPCHK(hipMemcpy(const_cast<uint64_t*>(p->d.q_thr0), t.data(), 8ull * p->nq, hipMemcpyHostToDevice));
  return FG_OK;
}

int fg_plan_destroy(fg_plan* p) {
  delete p;
  return FG_OK;
}

// One per-query threshold word and score histogram for plans of one batch on
// one device (fugu.h).  Every plan's bins are re-drawn over the union of the
// plans' score spans, so a bin means the same scores in every plan.
int fg_plan_link(fg_plan* const* plans, uint32_t n) {
  if (!plans || n == 0) return fail(FG_EINVAL, "bad arguments");
  fg_plan* o = plans[0];
  for (uint32_t i = 0; i < n; ++i) {
    if (!plans[i]) return fail(FG_EINVAL, "NULL plan");
    if (plans[i]->nq != o->nq || plans[i]->k != o->k) return fail(FG_EINVAL, "linked plans differ in batch or k");
    if (plans[i]->ix->dev != o->ix->dev) return fail(FG_EINVAL, "linked plans live on different devices");
    if (plans[i]->n_segs > 1) return fail(FG_EUNSUPPORTED, "a multi-snapshot plan already shares its thresholds");
  }
  const uint32_t nq = o->nq;
  std::vector<uint32_t> lo(nq, 0), sh(nq, 0);
  for (uint32_t q = 0; q < nq; ++q) {
    uint32_t l = 0, h = 0;
    for (uint32_t i = 0; i < n; ++i) {
      l = std::max(l, plans[i]->h_lo[q]);
      h = std::max(h, plans[i]->h_hi[q]);
    }
    const fgh::Bins b = fgh::union_bins(l, h);
    lo[q] = b.lo;
    sh[q] = b.shift;
  }
  HIPCHK(hipSetDevice(o->ix->dev));
  for (uint32_t i = 0; i < n; ++i) {
    fg_plan* p = plans[i];
    if (nq) {
      HIPCHK(hipMemcpy(const_cast<uint32_t*>(p->d.q_hlo), lo.data(), 4ull * nq, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(const_cast<uint32_t*>(p->d.q_hsh), sh.data(), 4ull * nq, hipMemcpyHostToDevice));
    }
    p->h_lo = lo;
    for (uint32_t q = 0; q < nq; ++q) p->h_hi[q] = std::max(p->h_hi[q], lo[q]);
    p->d.thresh = o->d.thresh;
    p->d.hist = o->d.hist;
    p->d.pub_mask = 0xFFFFFFFF00000000ull;  // score-only
  }
  return FG_OK;
}

int fg_search_batch(fg_index* ix, const fg_query_batch* q, uint32_t k, float* out_score, uint32_t* out_doc,
                    uint32_t* out_n) {
  fg_plan* p = nullptr;
  // execute is queued behind the upload on the same stream
  int rc = plan_create_multi(&ix, 1, q, k, &p, false, hipStreamPerThread);
  if (rc) return rc;
  std::unique_ptr<fg_plan> guard(p);
  // the calling thread's own stream: concurrent callers (tokio workers sharing
  // one Arc<Dataset>, src/db/config.rs:93) run their batches side by side
  if ((rc = fg_plan_execute(p, hipStreamPerThread, nullptr, nullptr, nullptr))) return rc;
  return fg_plan_results(p, out_score, out_doc, out_n);
}

int fg_merge_shards(uint32_t n_shards, uint32_t n_queries, uint32_t k, const float* d_score, const uint32_t* d_doc,
                    const uint32_t* d_n, float* d_out_score, uint32_t* d_out_doc, uint32_t* d_out_shard,
                    uint32_t* d_out_n, void* stream) {
  if (n_shards == 0 || n_shards > 64 || k == 0 || !d_score || !d_doc || !d_n || !d_out_score || !d_out_doc || !d_out_n)
    return fail(FG_EINVAL, "bad arguments");
  HIPCHK(fg::launch_merge(n_shards, n_queries, k, d_score, d_doc, d_n, d_out_score, d_out_doc, d_out_shard, d_out_n,
                          static_cast<hipStream_t>(stream)));
  return FG_OK;
}

// Persistent worker threads of fg_search_sharded's batch mode: a thread's
// first HIP call sets up per-thread runtime state, so threads made per call
// cost more than the planning they run.  Jobs never wait on other jobs, so a
// fixed pool serves any number of concurrent callers.  Never destroyed (idle
// workers end with the process).
class ShardWorkers {
 public:
  static ShardWorkers& get() {
    static ShardWorkers* w = new ShardWorkers(std::max(8, std::min(64, hw_threads(0))));
    return *w;
  }
  // f(0..n-1) on the workers; returns when all have run
  void run(uint32_t n, const std::function<void(uint32_t)>& f) {
    struct Batch { std::mutex m; std::condition_variable c; uint32_t left; } b;
    b.left = n;
    {
      std::lock_guard<std::mutex> l(mu_);
      for (uint32_t i = 0; i < n; ++i)
        q_.push_back([&b, &f, i] {
          f(i);
          std::lock_guard<std::mutex> lb(b.m);
          if (--b.left == 0) b.c.notify_all();
        });
    }
    cv_.notify_all();
    std::unique_lock<std::mutex> lb(b.m);
    b.c.wait(lb, [&] { return b.left == 0; });
  }

 private:
  explicit ShardWorkers(int n) {
    for (int i = 0; i < n; ++i)
      std::thread([this] {
        for (;;) {
          std::function<void()> job;
          {
            std::unique_lock<std::mutex> l(mu_);
            cv_.wait(l, [&] { return !q_.empty(); });
            job = std::move(q_.front());
            q_.pop_front();
          }
          job();
        }
      }).detach();
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> q_;
};

// One batch over several shards / segments / namespaces of one logical index
// (SURVEY.md §8b fg_search_sharded, §8e).  The shards of each device run as ONE
// multi-snapshot plan (fg_plan_create_multi: one upload, one launch per kernel,
// one shared score-only threshold per query); every shard's top-k lists land in
// gathered buffers on the first shard's device -- directly, or over xGMI
// (hipMemcpyPeerAsync) from another device -- and k_merge_rank merges them
// there into (score desc, shard asc, doc asc): tantivy's merge_fruits over
// DocAddress (segment_ord, doc).  Everything runs on the calling thread's
// per-thread streams.
}  // extern "C"
namespace fgh {
void run_parallel(uint32_t n, const std::function<void(uint32_t)>& f) { ShardWorkers::get().run(n, f); }
SearchTrace& search_trace() {
  static SearchTrace t;
  return t;
}
}  // namespace fgh
extern "C" {

int fg_search_trace(int enable, double* out_ms, uint32_t n, uint64_t* calls) {
  fgh::SearchTrace& t = fgh::search_trace();
  if (out_ms)
    for (uint32_t i = 0; i < n; ++i) out_ms[i] = i < fgh::kNumPhases ? (double)t.ns[i].exchange(0) * 1e-6 : 0.0;
  if (calls) *calls = t.calls.exchange(0);
  if (enable >= 0) t.on.store(enable ? 1 : 0);
  return FG_OK;
}

int fg_search_sharded(fg_ctx* ctx, fg_index* const* shards, uint32_t n_shards, const fg_query_batch* q, uint32_t k,
                      float* out_score, uint32_t* out_doc, uint32_t* out_shard, uint32_t* out_n) {
  if (!shards || n_shards == 0 || n_shards > FG_MAX_SEGMENTS || !q || k == 0 || !out_score || !out_doc || !out_n)
    return fail(FG_EINVAL, "bad arguments");
  for (uint32_t s = 0; s < n_shards; ++s) {
    if (!shards[s]) return fail(FG_EINVAL, "NULL shard");
    if (ctx && std::find(ctx->devs.begin(), ctx->devs.end(), shards[s]->dev) == ctx->devs.end())
      return fail(FG_EINVAL, "a shard lives on a device outside the context");
  }
  const uint32_t nq = q->n_queries;
  if (nq == 0) return FG_OK;
  if (k > FG_MAX_K) return fail(FG_EUNSUPPORTED, "k > FG_MAX_K");
  // ---- gathered lists + merged output on the first shard's device (its pool)
  const int dev0 = shards[0]->dev;
  const size_t nk = (size_t)nq * k;
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t g_s = al(4 * nk * n_shards), g_n = al(4ull * nq * n_shards), o_k = al(4 * nk), o_n = al(4ull * nq);
  const size_t total = 2 * g_s + g_n + 3 * o_k + o_n;
  size_t got = 0;
  HIPCHK(hipSetDevice(dev0));
  char* base = static_cast<char*>(shards[0]->pool->get(total, &got));
  if (!base) return fail(FG_EOOM, "hipMalloc of the shard merge buffers failed");
  float* gs = reinterpret_cast<float*>(base);
  uint32_t* gd = reinterpret_cast<uint32_t*>(base + g_s);
  uint32_t* gn = reinterpret_cast<uint32_t*>(base + 2 * g_s);
  float* ms = reinterpret_cast<float*>(base + 2 * g_s + g_n);
  uint32_t* md = reinterpret_cast<uint32_t*>(base + 2 * g_s + g_n + o_k);
  uint32_t* msh = reinterpret_cast<uint32_t*>(base + 2 * g_s + g_n + 2 * o_k);
  uint32_t* mn = reinterpret_cast<uint32_t*>(base + 2 * g_s + g_n + 3 * o_k);
  // the shards of each device, in shard order
  std::vector<int> gdev;
  std::vector<std::vector<uint32_t>> groups;
  for (uint32_t s = 0; s < n_shards; ++s) {
    const auto it = std::find(gdev.begin(), gdev.end(), shards[s]->dev);
    if (it == gdev.end()) {
      gdev.push_back(shards[s]->dev);
      groups.push_back({s});
    } else {
      groups[it - gdev.begin()].push_back(s);
    }
  }
  const size_t ng = groups.size();
  // every shard on the first device: the calling thread's high-priority stream
  // there, so a search's kernels are dispatched ahead of a commit's segment
  // build and the merger's; else per-thread streams
  const hipStream_t hs = ng == 1 && gdev[0] == dev0 ? search_stream(dev0) : hipStreamPerThread;
  // a batch run in two halves: the second half on the thread's second stream
  // there, so its kernels start while the first half's drain
  const hipStream_t hs2 = ng == 1 && gdev[0] == dev0 ? search_stream(dev0, true) : hs;
  uint32_t split = 0;  // the second half's first query (0: one part)
  bool merged = false;  // the plan's merged select already wrote ms / md / msh / mn
  std::vector<std::unique_ptr<fg_plan>> plans(ng), parts;
  std::vector<hipEvent_t> evs(ng, nullptr);
  // teardown (also on error returns): every device's stream drained, then the
  // events, the plans and the buffers
  struct Back {
    const std::vector<int>& dv; int d0; fg_index* ix0; void* p; size_t n; std::vector<hipEvent_t>& ev; hipStream_t s0,
        s1;
    ~Back() {
      for (size_t g = 0; g < dv.size(); ++g) {
        (void)hipSetDevice(dv[g]);
        (void)hipStreamSynchronize(hipStreamPerThread);
        if (ev[g]) (void)hipEventDestroy(ev[g]);
      }
      (void)hipSetDevice(d0);
      (void)hipStreamSynchronize(s0);
      if (s1 != s0) (void)hipStreamSynchronize(s1);
      ix0->pool->put(p, n);
    }
  } back{gdev, dev0, shards[0], base, got, evs, hs, hs2};
  static const bool trace_env = getenv("FUGU_SHARD_TRACE") != nullptr;
  fgh::SearchTrace& st = fgh::search_trace();
  const bool trace = trace_env || st.enabled();
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t_0 = trace ? now() : 0.0;
  double t_plan = 0.0;
  for (size_t g = 0; g < ng; ++g) {
    const std::vector<uint32_t>& gi = groups[g];
    const uint32_t S = (uint32_t)gi.size();
    std::vector<fg_index*> ixs(S);
    for (uint32_t j = 0; j < S; ++j) ixs[j] = shards[gi[j]];
    fg_plan* p = nullptr;
    // every shard on dev0 in one plan, a batch: its merged select writes the
    // merged lists directly (no per-shard lists, no k_merge_rank); a small batch
    // keeps one final select per shard (more workgroups in parallel: a single
    // query over 8 segments 0.070 vs 0.077 ms p50): the merged select from
    // batches of merged_min queries (tools/multi_ab.py, round 3).  A batch of
    // 2 x kPipeMin queries or more runs as two halves, the second planned on the
    // host while the first one's kernels run (C4, 1024 queries: one plan 478K
    // q/s, two halves 560K, four quarters 487K, 256 + 768 queries 513K)
    constexpr uint32_t merged_min = 256u, kPipeMin = 256u;
    uint64_t docs = 0;
    for (fg_index* x : ixs) docs += x->n_docs;
    if (ng == 1 && gdev[0] == dev0 && S > 1 && docs <= 0xFFFFFFFFull && nq >= merged_min) {
      const uint32_t np = nq >= 2 * kPipeMin ? 2u : 1u;
      for (uint32_t i = 0; i < np; ++i) {
        const uint32_t b = (uint32_t)((uint64_t)nq * i / np), e = (uint32_t)((uint64_t)nq * (i + 1) / np);
        fg_query_batch qi = *q;  // queries [b, e): the same term arrays, offsets from q_off[b]
        qi.n_queries = e - b;
        qi.q_off = q->q_off + b;
        if (q->f_off) qi.f_off = q->f_off + b;
        const double t_p = trace ? now() : 0.0;
        fg_plan* pi = nullptr;
        const hipStream_t si = i == 0 ? hs : hs2;
        if (i > 0) split = b;
        if (int rc = plan_create_multi(ixs.data(), S, &qi, k, &pi, false, si)) return rc;
        parts.emplace_back(pi);
        if (trace) t_plan += now() - t_p;
        if (int rc = execute_impl(pi, si, ms + (size_t)b * k, md + (size_t)b * k, mn + b, msh + (size_t)b * k)) return rc;
      }
      merged = true;
      break;
    }
    // the upload is queued on this thread's stream of the device, ahead of the
    // execute on the same stream: no host round trip
    const double t_p = trace ? now() : 0.0;
    if (int rc = plan_create_multi(ixs.data(), S, q, k, &p, false, hs)) {
      if (n_shards == 1) return rc;
      const std::string e = fg_last_error();
      return fail(rc, "device %d: %s", gdev[g], e.c_str());
    }
    plans[g].reset(p);
    if (trace) t_plan += now() - t_p;
    // lists straight into the gathered buffers when the group's shards are
    // consecutive and on dev0 ([S][nq][k] is the gathered layout)
    const bool direct = gdev[g] == dev0 && gi.back() - gi.front() + 1 == S;
    const size_t s0 = gi.front();
    if (int rc = direct ? fg_plan_execute(p, hs, gs + s0 * nk, gd + s0 * nk, gn + s0 * nq)
                        : fg_plan_execute(p, hs, nullptr, nullptr, nullptr))
      return rc;
    if (!direct) {
      for (uint32_t j = 0; j < S; ++j) {
        const size_t s = gi[j];
        if (gdev[g] == dev0) {
          HIPCHK(hipMemcpyAsync(gs + s * nk, p->own_score + j * nk, 4 * nk, hipMemcpyDeviceToDevice, hs));
          HIPCHK(hipMemcpyAsync(gd + s * nk, p->own_doc + j * nk, 4 * nk, hipMemcpyDeviceToDevice, hs));
          HIPCHK(hipMemcpyAsync(gn + s * nq, p->own_n + (size_t)j * nq, 4ull * nq, hipMemcpyDeviceToDevice,
                                hs));
        } else {
          HIPCHK(hipMemcpyPeerAsync(gs + s * nk, dev0, p->own_score + j * nk, gdev[g], 4 * nk, hs));
          HIPCHK(hipMemcpyPeerAsync(gd + s * nk, dev0, p->own_doc + j * nk, gdev[g], 4 * nk, hs));
          HIPCHK(hipMemcpyPeerAsync(gn + s * nq, dev0, p->own_n + (size_t)j * nq, gdev[g], 4ull * nq,
                                    hs));
        }
      }
    }
    if (gdev[g] != dev0) {
      HIPCHK(hipEventCreateWithFlags(&evs[g], hipEventDisableTiming));
      HIPCHK(hipEventRecord(evs[g], hs));
    }
  }
  const double t_run = trace ? now() : 0.0;
  HIPCHK(hipSetDevice(dev0));
  for (hipEvent_t e : evs)
    if (e) HIPCHK(hipStreamWaitEvent(hs, e, 0));
  if (!merged) HIPCHK(fg::launch_merge(n_shards, nq, k, gs, gd, gn, ms, md, msh, mn, hs));
  const bool two = split && hs2 != hs;
  if (trace_env) {
    HIPCHK(hipStreamSynchronize(hs));
    if (two) HIPCHK(hipStreamSynchronize(hs2));
    fprintf(stderr, "[fg_search_sharded] nq %u shards %u devices %zu merged %d: plan %.3f launch %.3f kernels+merge %.3f ms\n",
            nq, n_shards, ng, (int)merged, t_plan, t_run - t_0 - t_plan, now() - t_run);
  }
  // the search trace's phases: planning, launches, then the wait for the hits
  struct PhaseOut {
    fgh::SearchTrace& st; bool on; double t0, tp, tr; double (*clk)();
    ~PhaseOut() {
      if (!on) return;
      st.add(fgh::kPhPlan, (uint64_t)(tp * 1e6));
      st.add(fgh::kPhLaunch, (uint64_t)((tr - t0 - tp) * 1e6));
      st.add(fgh::kPhWait, (uint64_t)((clk() - tr) * 1e6));
    }
  } phase_out{st, st.enabled(), t_0, t_plan, t_run, +now};
  // the merged lists are consecutive: one D2H into a pinned buffer (small batches)
  const size_t span = 3 * o_k + 4ull * nq;
  if (span <= (4ull << 20)) {
    PinnedLease pin(*shards[0]->pinned, span);
    if (pin.p && two) {
      // each half's hits copied back on its own stream, the first half's copied
      // out of the pinned buffer while the second half's kernels run
      char* h = static_cast<char*>(pin.p);
      const char* d = reinterpret_cast<const char*>(ms);
      for (int half = 0; half < 2; ++half) {
        const hipStream_t sh = half ? hs2 : hs;
        const size_t q0 = half ? split : 0, q1 = half ? nq : split;
        for (size_t a = 0; a < 3; ++a)
          HIPCHK(hipMemcpyAsync(h + a * o_k + 4 * q0 * k, d + a * o_k + 4 * q0 * k, 4 * (q1 - q0) * k,
                                hipMemcpyDeviceToHost, sh));
        HIPCHK(hipMemcpyAsync(h + 3 * o_k + 4 * q0, d + 3 * o_k + 4 * q0, 4 * (q1 - q0), hipMemcpyDeviceToHost, sh));
      }
      for (int half = 0; half < 2; ++half) {
        HIPCHK(hipStreamSynchronize(half ? hs2 : hs));
        const size_t q0 = half ? split : 0, q1 = half ? nq : split;
        std::memcpy(out_score + q0 * k, h + 4 * q0 * k, 4 * (q1 - q0) * k);
        std::memcpy(out_doc + q0 * k, h + o_k + 4 * q0 * k, 4 * (q1 - q0) * k);
        if (out_shard) std::memcpy(out_shard + q0 * k, h + 2 * o_k + 4 * q0 * k, 4 * (q1 - q0) * k);
        std::memcpy(out_n + q0, h + 3 * o_k + 4 * q0, 4 * (q1 - q0));
      }
      return FG_OK;
    }
    if (two) HIPCHK(hipStreamSynchronize(hs2));  // (no pinned buffer: one copy on hs)
    if (pin.p) {
      HIPCHK(hipMemcpyAsync(pin.p, ms, span, hipMemcpyDeviceToHost, hs));
      HIPCHK(hipStreamSynchronize(hs));
      const char* h = static_cast<const char*>(pin.p);
      std::memcpy(out_score, h, 4 * nk);
      std::memcpy(out_doc, h + o_k, 4 * nk);
      if (out_shard) std::memcpy(out_shard, h + 2 * o_k, 4 * nk);
      std::memcpy(out_n, h + 3 * o_k, 4ull * nq);
      return FG_OK;
    }
  }
  if (two) HIPCHK(hipStreamSynchronize(hs2));
  HIPCHK(hipMemcpyAsync(out_score, ms, 4 * nk, hipMemcpyDeviceToHost, hs));
  HIPCHK(hipMemcpyAsync(out_doc, md, 4 * nk, hipMemcpyDeviceToHost, hs));
  if (out_shard) HIPCHK(hipMemcpyAsync(out_shard, msh, 4 * nk, hipMemcpyDeviceToHost, hs));
  HIPCHK(hipMemcpyAsync(out_n, mn, 4ull * nq, hipMemcpyDeviceToHost, hs));
  HIPCHK(hipStreamSynchronize(hs));
  return FG_OK;
}

}  // extern "C"
