// Stand-alone check of fg::probe_desc (fg_internal.h), the pure filler of
// k_conj's probe descriptors: every field for a plain-rank, a sparse-rank and
// a directory term, the lead entry, a query-time plan's payload ranges, and
// the kPdWide flag of a range past what a buffer resource addresses.  The
// addresses are made up and never dereferenced.  Built with
// -fsanitize=address,undefined and run by tests/test_probe_desc.py.
#include <cstdio>
#include <cstring>

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

int main() {
  using namespace fg;
  // device arrays above 4 GiB, so every 16-bit high part is in play
  const uint64_t a_doc = 0x7f1200000000ull, a_psc = 0x7f3400001000ull, a_tfn = 0x7e5600000200ull;
  const uint64_t a_dir = 0x7f7800000040ull, a_rank = 0x7d9a00000100ull, a_srank = 0x7cbc00000800ull;
  DevIndex ix{};
  ix.doc = (const uint32_t*)a_doc;
  ix.psc = (const float*)a_psc;
  ix.tfn = (const uint16_t*)a_tfn;
  ix.dir = (const uint32_t*)a_dir;
  ix.rank = (const uint64_t*)a_rank;
  ix.srank = (const uint64_t*)a_srank;
  ix.n_docs = 1000003;
  ix.rank_words = (ix.n_docs + 31) / 32;
  ix.srank_blocks = (ix.n_docs + 1023) / 1024;
  ix.n_prank = 5;
  CHECK(probe_addr_ok(ix));

  const uint64_t off = 123456789, df = 4321;
  {  // plain rank words: slot 3 of 5
    const ProbeTerm t{off, off + df, 0x80000000u | (3u << 16) | 9u | (2u << 8), 777};
    const ProbeDesc p = probe_desc(ix, t, false, false, 1.25f);
    CHECK(pd_base(p) == a_rank + 2ull * ix.rank_words * 8);
    CHECK(p.bytes == ix.rank_words * 8);
    CHECK(pd_shift(p.kind) == 5 && pd_steps(p.kind) == 0);
    CHECK(!(p.kind & (kPdDir | kPdSparse | kPdWide)));
    CHECK(pd_scores(p) == a_psc + off * 4 && p.sc_bytes == df * 4);
    CHECK(pd_aux(p) == 0);
    CHECK(p.ub == bits(1.25f));
    CHECK(p.base_lo == (uint32_t)pd_base(p) && (p.hi & 0xFFFFu) == 0x7d9au && (p.hi >> 16) == 0x7f34u);
    // the last rank word and the last score lie inside, the dead offsets outside
    CHECK(((ix.n_docs - 1) >> 5) * 8 + 8 <= p.bytes && (df - 1) * 4 + 4 <= p.sc_bytes);
    CHECK(kPdDead8 >= p.bytes && kPdDead4 >= p.sc_bytes && (0xFFFFFFFFu << 2) == kPdDead4);
  }
  {  // sparse rank words: slot 7, the second sparse one
    const ProbeTerm t{off, off + df, 0x80000000u | (7u << 16) | 9u | (2u << 8), 777};
    const ProbeDesc p = probe_desc(ix, t, false, false, 0.0f);
    CHECK(pd_base(p) == a_srank + 1ull * ix.srank_blocks * 8);
    CHECK(p.bytes == ix.srank_blocks * 8);
    CHECK(pd_shift(p.kind) == 10 && (p.kind & kPdSparse) && !(p.kind & (kPdDir | kPdWide)));
    CHECK(pd_scores(p) == a_psc + off * 4 && p.sc_bytes == df * 4 && p.ub == 0);
    CHECK(((ix.n_docs - 1) >> 10) * 8 + 8 <= p.bytes);
  }
  {  // bucket directory: B = 7, S = 3, first entry 777
    const ProbeTerm t{off, off + df, 7u | (3u << 8), 777};
    const ProbeDesc p = probe_desc(ix, t, false, false, 2.5f);
    CHECK(pd_base(p) == a_dir + 777ull * 4);
    CHECK(p.bytes == (((ix.n_docs - 1) >> 7) + 2) * 4);
    CHECK((p.kind & kPdDir) && !(p.kind & (kPdSparse | kPdWide)));
    CHECK(pd_shift(p.kind) == 7 && pd_steps(p.kind) == 3);
    CHECK(pd_aux(p) == a_doc + off * 4 && p.aux_lo == (uint32_t)(a_doc + off * 4) && (p.kind >> 16) == 0x7f12u);
    CHECK(pd_scores(p) == a_psc + off * 4 && p.sc_bytes == df * 4 && p.ub == bits(2.5f));
    // the last doc's bucket and the closing entry after it: one 8-byte load inside
    CHECK(((ix.n_docs - 1) >> 7) * 4 + 8 <= p.bytes);
  }
  {  // the widest search a directory can ask for: S = 32
    const ProbeTerm t{off, off + df, 31u | (32u << 8), 0};
    const ProbeDesc p = probe_desc(ix, t, false, false, 0.0f);
    CHECK(pd_shift(p.kind) == 31 && pd_steps(p.kind) == 32 && p.bytes == 2 * 4);
  }
  {  // the lead entry: doc ids and scores of the same postings, whatever the term's probe kind
    const ProbeTerm t{off, off + df, 0x80000000u | (3u << 16), 777};
    const ProbeDesc p = probe_desc(ix, t, true, false, 3.0f);
    CHECK(pd_base(p) == a_doc + off * 4 && p.bytes == df * 4);
    CHECK((p.kind & 0xFFFFu) == 0 && pd_aux(p) == 0);
    CHECK(pd_scores(p) == a_psc + off * 4 && p.sc_bytes == df * 4 && p.ub == bits(3.0f));
  }
  {  // a query-time plan: the payloads, 2 bytes each
    const ProbeTerm t{off, off + df, 7u | (3u << 8), 777};
    const ProbeDesc p = probe_desc(ix, t, false, true, 0.5f);
    CHECK(pd_scores(p) == a_tfn + off * 2 && p.sc_bytes == df * 2 && (p.hi >> 16) == 0x7e56u);
    CHECK(kPdDead2 >= p.sc_bytes && (0xFFFFFFFFu << 1) == kPdDead2);
    const ProbeDesc l = probe_desc(ix, t, true, true, 0.5f);
    CHECK(pd_base(l) == a_doc + off * 4 && l.bytes == df * 4 && pd_scores(l) == a_tfn + off * 2 && l.sc_bytes == df * 2);
  }
  {  // a list whose scores pass kPdMaxBytes: flagged, the bases still exact
    const uint64_t big = 600000000ull;
    const ProbeTerm t{off, off + big, 0x80000000u | (1u << 16), 0};
    const ProbeDesc p = probe_desc(ix, t, false, false, 1.0f);
    CHECK((p.kind & kPdWide) && pd_shift(p.kind) == 5);
    CHECK(pd_base(p) == a_rank && pd_scores(p) == a_psc + off * 4);
    CHECK(p.sc_bytes == (uint32_t)(big * 4));
    const ProbeDesc q = probe_desc(ix, t, false, true, 1.0f);  // ... as 2-byte payloads they fit
    CHECK(!(q.kind & kPdWide) && q.sc_bytes == big * 2);
    const ProbeTerm e{off, off + (1ull << 29), 0x80000000u | (1u << 16), 0};  // exactly kPdMaxBytes fits
    CHECK(!(probe_desc(ix, e, false, false, 1.0f).kind & kPdWide));
    const ProbeTerm e1{off, off + (1ull << 29) + 1, 0x80000000u | (1u << 16), 0};
    CHECK(probe_desc(ix, e1, false, false, 1.0f).kind & kPdWide);
    const ProbeTerm h{off, off + (1ull << 31), 0, 0};  // sizes past 32 bits saturate
    const ProbeDesc w = probe_desc(ix, h, true, false, 1.0f);
    CHECK((w.kind & kPdWide) && w.bytes == 0xFFFFFFFFu && w.sc_bytes == 0xFFFFFFFFu);
  }
  {  // a directory of more buckets than a resource addresses
    DevIndex big = ix;
    big.n_docs = 0xFFFFFFF0u;
    const ProbeTerm t{off, off + df, 1u | (2u << 8), 0};
    CHECK(probe_desc(big, t, false, false, 0.0f).kind & kPdWide);
  }
  {  // arrays where 48 bits do not reach
    DevIndex high = ix;
    high.psc = (const float*)0x0000800000000000ull;
    CHECK(!probe_addr_ok(high));
  }
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("probe_desc ok\n");
  return 0;
}
