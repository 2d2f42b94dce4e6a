// gevws_push_host.cpp -- gevws_push_check (include/gevws.h): the push pass's
// record rule on host memory, by the code the device runs (gevws_push.hpp).
// Plain C++: it also builds outside the library, under sanitizers
// (tests/cpp/push_fuzz.cpp).
#include "gevws.h"
#include "gevws_push.hpp"

extern "C" int64_t gevws_push_check(const gevws_push* records, uint64_t n, uint32_t n_conns, uint32_t n_rooms,
                                    uint64_t src_bytes) {
  using namespace gevws_push_rule;
  if (n > kMaxPushes || (n && !records)) return GEVWS_ERR_INVALID;
  int64_t bad = 0;
  for (uint64_t p = 0; p < n; ++p)
    bad += malformed(records[p], p != 0, p ? key(records[p - 1]) : 0, n_conns, n_rooms, src_bytes);
  return bad;
}
