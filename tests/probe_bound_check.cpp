// Stand-alone check of fg::probe_desc_bound (fg_internal.h), the pure filler of
// the bound fields of clause 1's probe descriptor, and of the u8 quantization
// the bound tables are built with (quant8 / q8_bound): the bound fields for
// every rule (deferred or not, query-time plan, the lead rule on and off, no
// table, a directory or wide clause), an existing descriptor left bit for bit
// as it was when no bound applies, and the quantization over edge scores.  The
// addresses are made up and never dereferenced.  Built with
// -fsanitize=address,undefined and run by tests/test_probe_bound.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "fg_internal.h"

static int failures = 0;
#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      ++failures;                                           \
    }                                                       \
  } while (0)

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static bool same(const fg::ProbeDesc& a, const fg::ProbeDesc& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// the byte a build stores for a posting (kernels.hip k_dtab8_scatter)
static uint32_t stored(float s, float M) { return std::max(1u, fg::quant8(s, M)); }

static void check_quant(float s, float M) {
  const uint32_t q = stored(s, M);
  CHECK(q >= 1 && q <= 255);
  CHECK(fg::q8_bound(q, M) >= s);
  CHECK(fg::q8_bound(q, M) <= M || q == 255);
  // within one step of the least such byte: quant8 starts from ceil(s / step), whose
  // division rounds (it may land one above), and only ever corrects upwards
  if (q > 2 && q < 255) CHECK(fg::q8_bound(q - 2, M) < s);
}

int main() {
  using namespace fg;
  const uint64_t a_doc = 0x7f1200000000ull, a_psc = 0x7f3400001000ull, a_tfn = 0x7e5600000200ull;
  const uint64_t a_dir = 0x7f7800000040ull, a_rank = 0x7d9a00000100ull, a_srank = 0x7cbc00000800ull;
  const uint64_t a_dtab = 0x7bde00000400ull, a_dtab8 = 0x7aef12345680ull;
  DevIndex ix{};
  ix.doc = (const uint32_t*)a_doc;
  ix.psc = (const float*)a_psc;
  ix.tfn = (const uint16_t*)a_tfn;
  ix.dir = (const uint32_t*)a_dir;
  ix.rank = (const uint64_t*)a_rank;
  ix.srank = (const uint64_t*)a_srank;
  ix.dtab = (const float*)a_dtab;
  ix.dtab8 = (const uint8_t*)a_dtab8;
  ix.n_docs = 1000003;
  ix.rank_words = (ix.n_docs + 31) / 32;
  ix.srank_blocks = (ix.n_docs + 1023) / 1024;
  ix.dtab_stride = (ix.n_docs + 31) & ~31u;
  ix.dtab8_stride = (ix.n_docs + 127) & ~127u;
  ix.n_prank = 5;
  CHECK(probe_addr_ok(ix));
  CHECK(ix.dtab8_stride % 128 == 0 && ix.dtab8_stride >= ix.n_docs);

  const uint64_t off = 123456789, df = 400000, lead_df = 70000;  // lead: 8.96 candidates per 128-doc line
  const float M = 3.75f;
  const ProbeTerm lt{1000, 1000 + lead_df, 0x80000000u | (2u << 16), 11, 0};
  const ProbeTerm rk{off, off + df, 0x80000000u | (3u << 16) | 9u | (2u << 8), 777, 0};  // plain rank words
  const ProbeTerm tb{off, off + df, 0x80000000u | (3u << 16) | 9u | (2u << 8), 777, 2};  // ... with an f32 table
  const ProbeTerm dr{off, off + df, 7u | (3u << 8), 777, 0};                             // bucket directory
  const ProbeDesc lead0 = probe_desc(ix, lt, true, false, 2.0f);
  CHECK(lead0.aux_lo == 0);

  {  // attached to a rank-word clause: the exact ranges stay, the aux fields carry the table
    ProbeDesc l = lead0, p = probe_desc(ix, rk, false, false, 1.25f, lead_df);
    const ProbeDesc p0 = p;
    CHECK(probe_desc_bound(ix, l, p, 4, M, true, false, df, lead_df, 8));
    CHECK(pd_aux(p) == a_dtab8 + 3ull * ix.dtab8_stride);
    CHECK((p.kind & kPdBound) && !(p.kind & (kPdDir | kPdWide | kPdTab | kPdSparse)));
    CHECK(pd_shift(p.kind) == 5);
    CHECK(l.aux_lo == bits(M));
    // everything else as probe_desc made it
    CHECK(p.base_lo == p0.base_lo && p.bytes == p0.bytes && p.sc_lo == p0.sc_lo && p.sc_bytes == p0.sc_bytes);
    CHECK(p.hi == p0.hi && p.ub == p0.ub && (p.kind & 0xFFFFu & ~kPdBound) == (p0.kind & 0xFFFFu));
    ProbeDesc l2 = l;
    l2.aux_lo = 0;
    CHECK(same(l2, lead0));
    // the last doc's byte lies inside a range of n_docs bytes, the dead offset outside
    CHECK(ix.n_docs - 1 < ix.n_docs && 0xFFFFFFFFu >= ix.n_docs);
  }
  {  // attached to an f32-table clause (kPdTab): both ranges stay the table
    ProbeDesc l = lead0, p = probe_desc(ix, tb, false, false, 1.25f, lead_df, 0);
    CHECK(p.kind & kPdTab);
    const ProbeDesc p0 = p;
    CHECK(probe_desc_bound(ix, l, p, 1, M, true, false, df, lead_df, 8));
    CHECK((p.kind & kPdTab) && (p.kind & kPdBound) && pd_aux(p) == a_dtab8);
    CHECK(pd_base(p) == pd_base(p0) && pd_scores(p) == pd_scores(p0) && p.bytes == p0.bytes);
  }
  // every rule that keeps the bound off leaves both descriptors bit for bit
  struct Case { const char* what; const ProbeTerm* t; uint32_t tab8; float M; bool deferred, qt; uint64_t lead_df; uint32_t lead8; bool has8; };
  const Case off_cases[] = {
      {"not deferred", &rk, 4, M, false, false, lead_df, 8, true},
      {"query-time plan", &rk, 4, M, true, true, lead_df, 8, true},
      {"no table for the term", &rk, 0, M, true, false, lead_df, 8, true},
      {"no tables in the snapshot", &rk, 4, M, true, false, lead_df, 8, false},
      {"lead rule off", &rk, 4, M, true, false, 60000, 8, true},  // 7.68 per line < 8, df < N / 2
      {"directory clause", &dr, 4, M, true, false, lead_df, 8, true},
      {"no maximum", &rk, 4, 0.0f, true, false, lead_df, 8, true},
  };
  for (const Case& c : off_cases) {
    DevIndex x = ix;
    if (!c.has8) x.dtab8 = nullptr;
    ProbeDesc l = probe_desc(x, lt, true, c.qt, 2.0f);
    ProbeDesc p = probe_desc(x, *c.t, false, c.qt, 1.25f, c.lead_df);
    const ProbeDesc l0 = l, p0 = p;
    const bool on = probe_desc_bound(x, l, p, c.tab8, c.M, c.deferred, c.qt, df, c.lead_df, c.lead8);
    if (on || !same(l, l0) || !same(p, p0)) {
      std::printf("bound attached or descriptor changed: %s\n", c.what);
      ++failures;
    }
    CHECK(!pd_aux(p0) || (p0.kind & kPdDir));
  }
  {  // the lead rule: on at exactly lead8 per line, always at 0, and for a term in half the docs
    ProbeDesc l = lead0, p = probe_desc(ix, rk, false, false, 1.0f, lead_df);
    CHECK(probe_uses_bound(1280, 10, 80, 8) && !probe_uses_bound(1280, 10, 79, 8));
    CHECK(probe_uses_bound(1280, 10, 1, 0));
    CHECK(probe_uses_bound(1280, 640, 1, 1000) && !probe_uses_bound(1280, 639, 1, 1000));
    CHECK(probe_desc_bound(ix, l, p, 4, M, true, false, df, 60000, 0));
    ProbeDesc l2 = lead0, p2 = probe_desc(ix, rk, false, false, 1.0f, 60000);
    CHECK(probe_desc_bound(ix, l2, p2, 4, M, true, false, (ix.n_docs + 1) / 2, 60000, 8));
  }
  {  // a wide clause (scores past a buffer resource) is probed item by item: no bound
    const ProbeTerm w{off, off + 600000000ull, 0x80000000u | (1u << 16), 0, 0};
    ProbeDesc l = lead0, p = probe_desc(ix, w, false, false, 1.0f, lead_df);
    CHECK(p.kind & kPdWide);
    const ProbeDesc p0 = p;
    CHECK(!probe_desc_bound(ix, l, p, 4, M, true, false, 600000000ull, lead_df, 0));
    CHECK(same(p, p0) && same(l, lead0));
  }
  {  // a directory's S_t shares kPdBound's bit: such a descriptor never reads as bounded
    const ProbeDesc p = probe_desc(ix, dr, false, false, 1.0f);
    CHECK(pd_steps(p.kind) == 3 && (p.kind & kPdBound) && (p.kind & kPdDir));
  }
  {  // a table where 48 bits do not reach
    DevIndex high = ix;
    high.dtab8 = (const uint8_t*)0x0000800000000000ull;
    CHECK(!probe_addr_ok(high));
  }

  // ---- quant8 / q8_bound over edge scores
  const float Ms[] = {3.75f, 1.0f, 255.0f, 1e-3f, 17.123456f, std::numeric_limits<float>::min(),
                      std::numeric_limits<float>::denorm_min() * 300.0f, std::numeric_limits<float>::denorm_min(), 1e30f};
  for (float Mx : Ms) {
    check_quant(Mx, Mx);  // s = M
    CHECK(stored(Mx, Mx) == 255);
    check_quant(std::nextafterf(Mx, 0.0f), Mx);
    check_quant(std::numeric_limits<float>::denorm_min(), Mx);
    check_quant(Mx * 0.5f, Mx);
    const float st = q8_step(Mx);
    for (uint32_t q = 0; q <= 255; ++q) {
      const float e = q8_bound(q, Mx);  // a step's own edge, the score just above it and just below
      if (e > 0.0f && e <= Mx) {
        check_quant(e, Mx);
        if (q >= 1) CHECK(stored(e, Mx) <= q + 1 || !(st > 0.0f));
      }
      const float up = std::nextafterf(e, std::numeric_limits<float>::infinity());
      if (up > 0.0f && up <= Mx) {
        check_quant(up, Mx);
        CHECK(stored(up, Mx) > q || q == 255 || !(st > 0.0f));
      }
      const float dn = std::nextafterf(e, 0.0f);
      if (dn > 0.0f && dn <= Mx) check_quant(dn, Mx);
    }
  }
  // a term whose postings all score the same: every byte is 255, and its bound the score itself
  for (float s : {0.5f, 2.0f, 1e-20f}) CHECK(stored(s, s) == 255 && q8_bound(255, s) == s);
  // q8_bound is monotone in the byte (a larger byte never bounds less)
  for (float Mx : Ms)
    for (uint32_t q = 1; q <= 255; ++q) CHECK(q8_bound(q, Mx) >= q8_bound(q - 1, Mx));

  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("probe_bound ok\n");
  return 0;
}
