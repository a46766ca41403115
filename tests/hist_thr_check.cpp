// Stand-alone check of fg::hist_kth_edge and fg::qbin (fg_internal.h), the
// pure rule behind the running threshold of a query's score histogram
// (hist_threshold, and the edge an ending k_conj item publishes): random
// unique keys arrive in "items" that each keep their own K best, the kept keys
// are binned, and after every item the edge is held against the true K-th key.
// Built with -fsanitize=address,undefined and run by tests/test_hist_thr.py.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <vector>

#include "fg_internal.h"

static int failures = 0;
#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      if (failures < 20) std::printf("%s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                           \
    }                                                       \
  } while (0)

using fg::kQBins;

// the edge over a whole histogram (bins ascending in h)
static uint64_t edge_of(const std::vector<uint32_t>& h, uint32_t K, uint32_t lo, uint32_t sh) {
  std::vector<uint32_t> d(h.rbegin(), h.rend());
  return fg::hist_kth_edge(d.data(), kQBins, kQBins - 1, 0, K, lo, sh);
}

// ... and as a workgroup forms it: two bins per "thread", each with the prefix of the bins above
static uint64_t edge_by_pairs(const std::vector<uint32_t>& h, uint32_t K, uint32_t lo, uint32_t sh) {
  uint64_t e = 0;
  uint32_t before = 0, found = 0;
  for (uint32_t t = 0; t < kQBins / 2; ++t) {
    const uint32_t b0 = kQBins - 1 - 2 * t, c[2] = {h[b0], h[b0 - 1]};
    if (const uint64_t x = fg::hist_kth_edge(c, 2, b0, before, K, lo, sh)) {
      e = x;
      ++found;
    }
    before += c[0] + c[1];
  }
  CHECK(found <= 1);
  return e;
}

static uint64_t bin_edge(uint32_t b, uint32_t lo, uint32_t sh) { return (uint64_t)(lo + (b << sh)) << 32; }

static void run(uint32_t K, uint32_t sh, uint32_t n_keys, bool equal_scores, uint32_t seed) {
  std::mt19937 rng(seed);
  const uint32_t lo = 0x3F800000u, span = kQBins << sh;
  // scores from a quarter of the span below bin 0 to a quarter above the top bin (clamped into it)
  std::vector<uint64_t> keys(n_keys);
  for (uint32_t i = 0; i < n_keys; ++i) {
    const uint32_t bits = equal_scores ? lo + span / 3 : lo - span / 4 + (uint32_t)(rng() % (span + span / 2));
    keys[i] = ((uint64_t)bits << 32) | (0xFFFFFFFFu - i);  // unique: doc i
  }
  std::shuffle(keys.begin(), keys.end(), rng);
  std::vector<uint32_t> h(kQBins, 0);
  std::vector<uint64_t> seen, counted;
  for (uint32_t at = 0; at < n_keys;) {
    // an item: some keys, of which it keeps its own K best
    const uint32_t n = std::min<uint32_t>(n_keys - at, 1 + rng() % (3 * K + 7));
    std::vector<uint64_t> item(keys.begin() + at, keys.begin() + at + n);
    at += n;
    seen.insert(seen.end(), item.begin(), item.end());
    std::sort(item.begin(), item.end(), std::greater<uint64_t>());
    if (item.size() > K) item.resize(K);
    for (uint64_t k : item) {
      const uint32_t b = fg::qbin(k, lo, sh);
      CHECK(b <= kQBins);
      CHECK((b == kQBins) == ((uint32_t)(k >> 32) < lo));
      if (b < kQBins) {
        CHECK(k >= bin_edge(b, lo, sh));
        CHECK(b == kQBins - 1 || k < bin_edge(b + 1, lo, sh));
        ++h[b];
        counted.push_back(k);
      }
    }
    const uint64_t e = edge_of(h, K, lo, sh);
    CHECK(e == edge_by_pairs(h, K, lo, sh));
    CHECK((e & 0xFFFFFFFFull) == 0);
    // never above the true K-th key of everything seen so far (0: fewer than K keys)
    std::sort(seen.begin(), seen.end(), std::greater<uint64_t>());
    const uint64_t kth = seen.size() >= K ? seen[K - 1] : 0ull;
    CHECK(e <= kth);
    if (equal_scores) CHECK(e <= ((uint64_t)(lo + span / 3) << 32));
    // ... and, once K keys are counted, no lower than that key's bin
    if (counted.size() >= K) {
      const uint32_t kb = fg::qbin(kth, lo, sh);
      CHECK(kb < kQBins);
      if (kb < kQBins) CHECK(e >= bin_edge(kb, lo, sh));
      CHECK(e != 0);
    } else {
      CHECK(e == 0);
    }
    // stale counts (any subset of the adds missing) never raise it
    for (int rep = 0; rep < 4; ++rep) {
      std::vector<uint32_t> g(h);
      for (uint64_t k : counted)
        if (rng() % (rep + 2) == 0) --g[fg::qbin(k, lo, sh)];
      CHECK(edge_of(g, K, lo, sh) <= e);
      CHECK(edge_by_pairs(g, K, lo, sh) == edge_of(g, K, lo, sh));
    }
    // the bins below a cut at or under the K-th bin do not matter
    if (e) {
      const uint32_t eb = fg::qbin(e, lo, sh);
      CHECK(bin_edge(eb, lo, sh) == e);
      for (uint32_t cut : {0u, eb / 2, eb}) {
        std::vector<uint32_t> g(h);
        std::fill(g.begin(), g.begin() + cut, 0u);
        CHECK(edge_of(g, K, lo, sh) == e);
      }
      // (a cut above it can only lower the edge)
      if (eb + 1 < kQBins) {
        std::vector<uint32_t> g(h);
        std::fill(g.begin(), g.begin() + eb + 1, 0u);
        CHECK(edge_of(g, K, lo, sh) == 0);
      }
    }
  }
}

int main() {
  uint32_t seed = 1;
  for (uint32_t K : {1u, 10u, 100u, 1000u})
    for (uint32_t sh : {0u, 17u}) {
      run(K, sh, 6 * K + 50, false, seed++);
      run(K, sh, 3 * K + 5, true, seed++);
    }
  // an empty histogram, K = 0, and a histogram with everything in the clamp bin
  std::vector<uint32_t> h(kQBins, 0);
  CHECK(edge_of(h, 10, 0x3F800000u, 17) == 0);
  h[kQBins - 1] = 10;
  CHECK(edge_of(h, 10, 0x3F800000u, 17) == bin_edge(kQBins - 1, 0x3F800000u, 17));
  CHECK(edge_of(h, 11, 0x3F800000u, 17) == 0);
  CHECK(edge_of(h, 0, 0x3F800000u, 17) == 0);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("hist_kth_edge ok\n");
  return 0;
}
