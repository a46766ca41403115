// Stand-alone check of fg::band_cuts / fg::band_tier / fg::band_bin
// (fg_internal.h), the pure cut and tier-of-score rule of the score-tiered lead
// copies: the cuts of a list's histogram are held against the list sorted by
// score, and the stable partition the rule implies (what k_band_scatter does on
// the device) is formed on the host and checked: a permutation, docs ascending
// inside a tier, tiers in score order, every class of equal scores in one tier,
// chunk maxima that bound their chunks.
// Built with -fsanitize=address,undefined and run by tests/test_band_cuts.py.
#include <algorithm>
#include <cstdio>
#include <cstring>
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

using fg::kBandBins;
using fg::kBandShareDen;
using fg::kBandShares;
using fg::kBandTiers;
using fg::kChunk;

static uint32_t bits_of(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

static void check_list(const std::vector<float>& sc, const char* what) {
  const uint64_t df = sc.size();
  std::vector<uint32_t> h(kBandBins, 0);
  for (float s : sc) h[fg::band_bin(bits_of(s))]++;
  uint32_t lo[kBandTiers - 1];
  fg::band_cuts(h.data(), df, lo);
  // the sorted reference: cut i is the bin of the ceil(df * share_i)-th best score,
  // the smallest set of whole bins from the top that holds that share
  std::vector<uint32_t> bins;
  for (float s : sc) bins.push_back(fg::band_bin(bits_of(s)));
  std::sort(bins.begin(), bins.end(), std::greater<uint32_t>());
  for (uint32_t i = 0; i + 1 < kBandTiers; ++i) {
    const uint64_t r = std::max<uint64_t>(1, (df * kBandShares[i] + kBandShareDen - 1) / kBandShareDen);  // 1-based rank
    CHECK(lo[i] == bins[r - 1]);
    if (i) CHECK(lo[i] <= lo[i - 1]);
    // tiers 0..i hold at least their share, and would not without their last bin
    const uint64_t have = std::upper_bound(bins.begin(), bins.end(), lo[i], std::greater<uint32_t>()) - bins.begin();
    const uint64_t above = std::lower_bound(bins.begin(), bins.end(), lo[i], std::greater<uint32_t>()) - bins.begin();
    CHECK(have * kBandShareDen >= df * kBandShares[i]);
    CHECK(above == 0 || above * kBandShareDen < df * kBandShares[i]);
  }
  // the stable partition
  std::vector<uint32_t> tier(df), cnt(kBandTiers, 0);
  for (uint64_t p = 0; p < df; ++p) {
    tier[p] = fg::band_tier(bits_of(sc[p]), lo);
    CHECK(tier[p] < kBandTiers);
    cnt[tier[p]]++;
  }
  CHECK(cnt[0] >= 1);  // the best score leads
  std::vector<uint32_t> at(kBandTiers, 0), bdoc(df, 0xFFFFFFFFu);
  std::vector<float> bsc(df);
  for (uint32_t t = 1; t < kBandTiers; ++t) at[t] = at[t - 1] + cnt[t - 1];
  std::vector<uint32_t> first = at;
  for (uint64_t p = 0; p < df; ++p) {
    bdoc[at[tier[p]]] = (uint32_t)p;  // (doc = list position: ascending)
    bsc[at[tier[p]]++] = sc[p];
  }
  for (uint32_t t = 0; t < kBandTiers; ++t) {
    const uint32_t b = first[t], e = b + cnt[t];
    for (uint32_t x = b; x < e; ++x) {
      if (x > b) CHECK(bdoc[x] > bdoc[x - 1]);
      // a tier's scores lie inside its cuts, so a better tier holds no lower score
      const uint32_t bn = fg::band_bin(bits_of(bsc[x]));
      if (t > 0) CHECK(bn < lo[t - 1]);
      if (t + 1 < kBandTiers) CHECK(bn >= lo[t]);
    }
  }
  // equal scores share a tier
  {
    std::vector<std::pair<uint32_t, uint32_t>> bt;
    for (uint64_t p = 0; p < df; ++p) bt.emplace_back(bits_of(sc[p]), tier[p]);
    std::sort(bt.begin(), bt.end());
    for (size_t x = 1; x < bt.size(); ++x) {
      if (bt[x].first == bt[x - 1].first) CHECK(bt[x].second == bt[x - 1].second);
      CHECK(bt[x].second <= bt[x - 1].second);  // ascending scores: tiers never get worse
    }
  }
  // chunk maxima of the copy bound every posting of their chunk, and one attains each
  for (uint64_t c0 = 0; c0 < df; c0 += kChunk) {
    const uint64_t c1 = std::min<uint64_t>(df, c0 + kChunk);
    const float m = *std::max_element(bsc.begin() + c0, bsc.begin() + c1);
    for (uint64_t x = c0; x < c1; ++x) CHECK(bsc[x] <= m);
  }
  if (failures) std::printf("  (in %s, df %llu)\n", what, (unsigned long long)df);
}

int main() {
  std::mt19937 rng(12345);
  // all scores equal: one class, one tier
  for (uint32_t df : {1u, 2u, 7u, 2048u, 2049u}) check_list(std::vector<float>(df, 1.5f), "all equal");
  {
    std::vector<float> v(1000, 0.75f);
    uint32_t lo[kBandTiers - 1];
    std::vector<uint32_t> h(kBandBins, 0);
    h[fg::band_bin(bits_of(0.75f))] = 1000;
    fg::band_cuts(h.data(), 1000, lo);
    for (uint32_t i = 0; i + 1 < kBandTiers; ++i) CHECK(lo[i] == fg::band_bin(bits_of(0.75f)));
    CHECK(fg::band_tier(bits_of(0.75f), lo) == 0);
  }
  // two values, at every split
  for (uint32_t df : {2u, 16u, 33u, 2048u, 2049u})
    for (uint32_t hi : {0u, 1u, df / 16, df / 16 + 1, df / 8, df / 2, df - 1, df}) {
      if (hi > df) continue;
      std::vector<float> v(df, 0.25f);
      for (uint32_t x = 0; x < hi; ++x) v[(x * 7919u) % df] = 2.0f;  // (collisions only lower the count)
      check_list(v, "two values");
    }
  // a tie class straddling a share: 1/32 of the list above it, then a class of a quarter of the list
  // (whatever the shares are, the class closes every share between 1/32 and 9/32 at once)
  for (uint32_t df : {64u, 2048u, 2049u, 3 * 2048u + 1}) {
    std::vector<float> v(df);
    for (uint32_t x = 0; x < df; ++x) v[x] = x % 32 == 0 ? 3.0f : x % 4 == 1 ? 1.0f : 0.001f * (float)(1 + x % 97);
    check_list(v, "tie class across a share");
    uint32_t lo[kBandTiers - 1];
    std::vector<uint32_t> h(kBandBins, 0);
    for (float s : v) h[fg::band_bin(bits_of(s))]++;
    fg::band_cuts(h.data(), df, lo);
    for (uint32_t i = 0; i + 1 < kBandTiers; ++i) {
      const bool in = kBandShares[i] * 32 > kBandShareDen && kBandShares[i] * 32 <= 9 * kBandShareDen;
      if (in) CHECK(lo[i] == fg::band_bin(bits_of(1.0f)));  // never split
      if (kBandShares[i] * 32 <= kBandShareDen) CHECK(lo[i] == fg::band_bin(bits_of(3.0f)));
      if (kBandShares[i] * 32 > 9 * kBandShareDen) CHECK(lo[i] < fg::band_bin(bits_of(1.0f)));
    }
  }
  // the lengths around a chunk, random scores of BM25's shape and of many octaves
  for (uint32_t df : {1u, 2u, 3u, 15u, 16u, 17u, 2047u, 2048u, 2049u, 3 * 2048u + 1, 50000u}) {
    std::vector<float> v(df);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    for (float& s : v) {
      const float tf = 1.0f + std::floor(8.0f * u(rng) * u(rng)), nrm = 0.3f + 2.0f * u(rng);
      s = 1.7f * (tf / (tf + nrm));
    }
    check_list(v, "bm25-like");
    for (float& s : v) s = std::ldexp(1.0f + u(rng), (int)(u(rng) * 40.0f) - 20);
    check_list(v, "many octaves");
  }
  // the bin rule at its ends
  CHECK(fg::band_bin(0u) == 0 && fg::band_bin(0x7F7FFFFFu) == 0x7F7Fu && fg::band_bin(0xFFFFFFFFu) == kBandBins - 1);
  // an empty histogram: every cut 0, everything in tier 0
  {
    std::vector<uint32_t> h(kBandBins, 0);
    uint32_t lo[kBandTiers - 1] = {9, 9, 9, 9};
    fg::band_cuts(h.data(), 0, lo);
    for (uint32_t i = 0; i + 1 < kBandTiers; ++i) CHECK(lo[i] == 0);
    CHECK(fg::band_tier(bits_of(1.0f), lo) == 0);
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("band_cuts ok\n");
  return 0;
}
