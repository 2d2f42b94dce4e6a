// gevws_fragment.hpp -- the rule that turns one outbound record into its
// fragments (RFC 6455 section 5.4; RFC 7692 section 6.1 for RSV1), written
// once for the device step (gevws_fragment.hip) and its host twin
// (gevws_fragment_host.cpp), both declared in include/gevws.h.  The reference
// writes every message as one frame (plugins/websocket/ws/write.go:48-84) and
// has no such rule.
//
// A record r splits under the limit F (>= 1, payload bytes a frame) exactly
// when it is a whole, consistent data message longer than F: fin == 1, opcode
// 1 or 2, hdr.length >= 0 and equal to payload_len, payload_len > F.  It then
// has c = ceil(payload_len / F) fragments; every other record has one, itself.
// A splittable record with c > 2^31 - 1 is malformed: with at most 2^32 - 1
// records every 64-bit sum of counts stays exact.
// Plain C++: the host file also builds outside the library, under sanitizers
// (tests/cpp/fragment_check.cpp).
#pragma once

#include <cstdint>

#include "gevws.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GEVWS_FRAG_HD __host__ __device__ __forceinline__
#else
#define GEVWS_FRAG_HD inline
#endif

namespace gevws_fragment {

constexpr uint64_t kMaxFragments = 0x7FFFFFFFull;  // of one record
constexpr uint64_t kMaxRecords = 0xFFFFFFFFull;    // of one call (and fragments it may be given room for)

GEVWS_FRAG_HD bool splittable(const gevws_out_frame& r, uint64_t F) {
  return r.hdr.fin == 1 && (r.hdr.opcode == 1 || r.hdr.opcode == 2) && r.hdr.length >= 0 &&
         (uint64_t)r.hdr.length == r.payload_len && r.payload_len > F;
}

// The record's fragment count (>= 1); bad: it is malformed (the count is then 0).
GEVWS_FRAG_HD uint64_t count(const gevws_out_frame& r, uint64_t F, bool& bad) {
  bad = false;
  if (!splittable(r, F)) return 1;
  const uint64_t c = r.payload_len / F + (r.payload_len % F != 0);  // (no sum that could wrap)
  if (c > kMaxFragments) {
    bad = true;
    return 0;
  }
  return c;
}

// Fragment i of the record's c (i < c).  c == 1: the record itself, byte for byte.
GEVWS_FRAG_HD gevws_out_frame fragment(const gevws_out_frame& r, uint64_t F, uint64_t c, uint64_t i) {
  if (c <= 1) return r;
  gevws_out_frame o = r;  // masked and mask are copied
  const uint64_t at = i * F, rest = r.payload_len - at;  // i < c <= 2^31 - 1 and i * F < payload_len
  const uint64_t len = rest < F ? rest : F;
  o.hdr.fin = i == c - 1;
  o.hdr.rsv = i == 0 ? r.hdr.rsv : 0;
  o.hdr.opcode = i == 0 ? r.hdr.opcode : 0;
  o.hdr.length = (int64_t)len;
  o.payload_len = len;
  o.payload_off = r.payload_off + at;
  return o;
}

}  // namespace gevws_fragment
