// gevws_fragment_host.cpp -- gevws_fragment_records (include/gevws.h): the
// fragment step of gevws_fragment.hip on host memory, by the same rule
// (gevws_fragment.hpp) -- the same fragments, table, summary and statuses.
// Plain C++: it also builds outside the library, under sanitizers
// (tests/cpp/fragment_check.cpp).
#include <cstring>

#include "gevws.h"
#include "gevws_fragment.hpp"

extern "C" int gevws_fragment_records(const gevws_out_frame* records, uint64_t n, uint64_t max_fragment_bytes,
                                      gevws_out_frame* frags, uint64_t max_frags, uint64_t* first,
                                      gevws_summary* summary) {
  using namespace gevws_fragment;
  if (max_fragment_bytes == 0 || n > kMaxRecords || max_frags > kMaxRecords) return GEVWS_ERR_INVALID;
  if (!summary || !first || (n && !records) || (max_frags && !frags)) return GEVWS_ERR_INVALID;
  const uint64_t F = max_fragment_bytes;
  gevws_summary s;
  memset(&s, 0, sizeof(s));
  // the verdict first: nothing but the summary is written without it
  uint64_t total = 0, split = 0, bytes = 0, malformed = 0;
  for (uint64_t k = 0; k < n; ++k) {
    bool bad;
    const uint64_t c = count(records[k], F, bad);
    total += c, split += c > 1, bytes += records[k].payload_len, malformed += bad;
  }
  if (malformed) {
    s.errors = malformed;
    s.status = GEVWS_ERR_INVALID;
    *summary = s;
    return GEVWS_OK;
  }
  s.frames = total;
  s.payload_bytes = split;
  s.payload_len = bytes;
  if (total > max_frags) {
    s.status = GEVWS_ERR_CAPACITY;
    *summary = s;
    return GEVWS_OK;
  }
  uint64_t at = 0;
  for (uint64_t k = 0; k < n; ++k) {
    bool bad;
    const uint64_t c = count(records[k], F, bad);
    first[k] = at;
    for (uint64_t i = 0; i < c; ++i) frags[at + i] = fragment(records[k], F, c, i);
    at += c;
  }
  first[n] = at;
  *summary = s;
  return GEVWS_OK;
}
