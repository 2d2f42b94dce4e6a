// fragment_check.cpp -- gevws_fragment_records (gev_amd/csrc/gevws_fragment_host.cpp)
// over random and edge record lists, built with -fsanitize=address,undefined:
// every output buffer is a heap block of exactly the size the contract names
// (need fragments, n + 1 table entries), so a write past it is caught, and the
// fragments are checked against the rule of include/gevws.h restated here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gevws.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
  return rng_state;
}

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "fragment_check: line %d: %s\n", __LINE__, #c); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

static gevws_out_frame rec(uint64_t len, int opcode, int fin, int rsv, uint64_t off, int64_t hdr_len) {
  gevws_out_frame r;
  memset(&r, 0, sizeof(r));
  r.hdr.fin = (uint8_t)fin, r.hdr.rsv = (uint8_t)rsv, r.hdr.opcode = (uint8_t)opcode;
  r.hdr.masked = (uint8_t)(rnd() & 1);
  for (int i = 0; i < 4; ++i) r.hdr.mask[i] = r.hdr.masked ? (uint8_t)rnd() : 0;
  r.hdr.length = hdr_len;
  r.payload_off = off, r.payload_len = len;
  return r;
}

static bool splits(const gevws_out_frame& r, uint64_t F) {
  return r.hdr.fin == 1 && (r.hdr.opcode == 1 || r.hdr.opcode == 2) && r.hdr.length >= 0 &&
         (uint64_t)r.hdr.length == r.payload_len && r.payload_len > F;
}

// One list through the call: sized by a first call with no room, then exact.
static void run(const std::vector<gevws_out_frame>& recs, uint64_t F) {
  const uint64_t n = recs.size();
  gevws_summary s;
  uint64_t* first = (uint64_t*)malloc((n + 1) * 8);
  memset(first, 0xEE, (n + 1) * 8);
  CHECK(gevws_fragment_records(n ? recs.data() : nullptr, n, F, nullptr, 0, first, &s) == GEVWS_OK);
  uint64_t want = 0, split = 0, bytes = 0;
  for (const auto& r : recs) {
    const uint64_t c = splits(r, F) ? (r.payload_len + F - 1) / F : 1;
    want += c, split += c > 1, bytes += r.payload_len;
  }
  CHECK(s.frames == want && s.payload_bytes == split && s.payload_len == bytes && s.errors == 0);
  CHECK(s.status == (want ? GEVWS_ERR_CAPACITY : GEVWS_OK));
  if (want) {
    for (uint64_t k = 0; k <= n; ++k) CHECK(first[k] == 0xEEEEEEEEEEEEEEEEull);  // nothing but the summary
    if (want > 1) {  // one short: still nothing
      gevws_out_frame* few = (gevws_out_frame*)malloc((want - 1) * sizeof(gevws_out_frame));
      memset(few, 0xEE, (want - 1) * sizeof(gevws_out_frame));
      CHECK(gevws_fragment_records(recs.data(), n, F, few, want - 1, first, &s) == GEVWS_OK);
      CHECK(s.status == GEVWS_ERR_CAPACITY && s.frames == want);
      for (uint64_t i = 0; i < (want - 1) * sizeof(gevws_out_frame); ++i) CHECK(((uint8_t*)few)[i] == 0xEE);
      free(few);
    }
  }
  gevws_out_frame* frags = (gevws_out_frame*)malloc((want ? want : 1) * sizeof(gevws_out_frame));
  CHECK(gevws_fragment_records(n ? recs.data() : nullptr, n, F, frags, want, first, &s) == GEVWS_OK);
  CHECK(s.status == GEVWS_OK && s.frames == want && s.payload_bytes == split && s.payload_len == bytes);
  CHECK(first[0] == 0 && first[n] == want);
  for (uint64_t k = 0; k < n; ++k) {
    const gevws_out_frame& r = recs[k];
    const uint64_t f0 = first[k], c = first[k + 1] - f0;
    CHECK(first[k + 1] > f0);
    if (!splits(r, F)) {
      CHECK(c == 1 && memcmp(&frags[f0], &r, sizeof(r)) == 0);
      continue;
    }
    CHECK(c == (r.payload_len + F - 1) / F && c >= 2);
    uint64_t at = r.payload_off;
    for (uint64_t i = 0; i < c; ++i) {
      const gevws_out_frame& f = frags[f0 + i];
      CHECK(f.hdr.fin == (i == c - 1));
      CHECK(f.hdr.rsv == (i == 0 ? r.hdr.rsv : 0) && f.hdr.opcode == (i == 0 ? r.hdr.opcode : 0));
      CHECK(f.hdr.masked == r.hdr.masked && memcmp(f.hdr.mask, r.hdr.mask, 4) == 0);
      CHECK(f.payload_off == at && (uint64_t)f.hdr.length == f.payload_len && f.hdr.length >= 0);
      CHECK(i == c - 1 ? (f.payload_len >= 1 && f.payload_len <= F) : f.payload_len == F);
      at += f.payload_len;
    }
    CHECK(at == r.payload_off + r.payload_len);
  }
  free(frags);
  free(first);
}

int main() {
  const uint64_t limits[] = {1, 2, 16, 17, 125, 126, 65535, 65536, 1ull << 40, UINT64_MAX};
  for (uint64_t F : limits) {
    // the lengths around the limit, every kind of record
    std::vector<gevws_out_frame> recs;
    const uint64_t lens[] = {0, 1, F - 1, F, F + 1, 2 * F - 1, 2 * F, 2 * F + 1, 3 * F + 7};
    uint64_t off = 0;
    for (uint64_t L : lens) {
      if (F > 65536 && L > 1) continue;  // (sums that wrap: lengths near 2^64 are tried below)
      for (int op : {0, 1, 2, 8, 9, 10})
        for (int fin : {0, 1})
          for (int rsv : {0, 4}) recs.push_back(rec(L, op, fin, rsv, off, (int64_t)L)), off += (L + 15) & ~15ull;
      recs.push_back(rec(L, 1, 1, 0, off, (int64_t)L + 1));
      recs.push_back(rec(L, 2, 1, 4, off, -1));
    }
    run(recs, F);
    // random lists
    for (int round = 0; round < 20; ++round) {
      std::vector<gevws_out_frame> rr;
      const uint64_t n = rnd() % 300, span = F > 4096 ? 8 : 6 * F + 1;
      for (uint64_t k = 0; k < n; ++k) {
        const uint64_t L = rnd() % span;
        const int kind = (int)(rnd() % 8);
        rr.push_back(rec(L, kind < 5 ? 1 + (int)(rnd() & 1) : (int)(rnd() % 16), kind != 5, (int)(rnd() % 8), rnd() >> 8,
                         kind == 6 ? (int64_t)(L + 1 + rnd() % 4) : (int64_t)L));
      }
      run(rr, F);
    }
  }
  run({}, 7);
  // a record of 4 097 fragments between one-fragment neighbours
  run({rec(1, 1, 1, 0, 0, 1), rec(4097, 2, 1, 4, 16, 4097), rec(0, 1, 1, 0, 8192, 0)}, 1);
  // records that pass through whatever their fields say: lengths and offsets at the top of the range
  run({rec(UINT64_MAX, 1, 1, 0, UINT64_MAX, -1), rec(1ull << 63, 2, 1, 0, 5, INT64_MIN), rec(UINT64_MAX, 9, 1, 0, 1, 3),
       rec(UINT64_MAX, 1, 0, 0, 1, INT64_MAX)},
      1);
  // 2^31 - 1 fragments are the most of one record: one more is malformed, and nothing is written
  {
    gevws_summary s;
    uint64_t first[4];
    memset(first, 0xEE, sizeof(first));
    const gevws_out_frame most[3] = {rec(3, 1, 1, 0, 0, 3), rec(0x7FFFFFFFull, 2, 1, 0, 0, 0x7FFFFFFFll),
                                     rec(2 * 0x7FFFFFFFull, 2, 1, 0, 0, 2 * 0x7FFFFFFFll)};
    CHECK(gevws_fragment_records(most, 3, 1, nullptr, 0, first, &s) == GEVWS_OK);
    CHECK(s.status == GEVWS_ERR_INVALID && s.errors == 1 && s.frames == 0 && s.payload_len == 0);
    CHECK(gevws_fragment_records(most, 3, 2, nullptr, 0, first, &s) == GEVWS_OK);
    CHECK(s.status == GEVWS_ERR_CAPACITY && s.errors == 0 && s.frames == 2 + 0x40000000ull + 0x7FFFFFFFull);
    CHECK(gevws_fragment_records(most, 2, 1, nullptr, 0, first, &s) == GEVWS_OK);
    CHECK(s.status == GEVWS_ERR_CAPACITY && s.frames == 3 + 0x7FFFFFFFull && s.payload_bytes == 2);
    const gevws_out_frame huge = rec(1ull << 40, 1, 1, 4, 0, 1ll << 40);
    CHECK(gevws_fragment_records(&huge, 1, 1, nullptr, 0, first, &s) == GEVWS_OK);
    CHECK(s.status == GEVWS_ERR_INVALID && s.errors == 1);
    for (uint64_t v : first) CHECK(v == 0xEEEEEEEEEEEEEEEEull);
    // invalid calls
    CHECK(gevws_fragment_records(most, 3, 0, nullptr, 0, first, &s) == GEVWS_ERR_INVALID);
    CHECK(gevws_fragment_records(most, 1ull << 32, 1, nullptr, 0, first, &s) == GEVWS_ERR_INVALID);
    CHECK(gevws_fragment_records(most, 3, 1, nullptr, 1, first, &s) == GEVWS_ERR_INVALID);
    CHECK(gevws_fragment_records(most, 3, 1, nullptr, 0, nullptr, &s) == GEVWS_ERR_INVALID);
    CHECK(gevws_fragment_records(most, 3, 1, nullptr, 0, first, nullptr) == GEVWS_ERR_INVALID);
  }
  printf("fragment_check ok\n");
  return 0;
}
