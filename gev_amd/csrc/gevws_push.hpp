// gevws_push.hpp -- the rules of the push pass (include/gevws.h, "Server
// push") that look at one record: when a gevws_push is malformed, and which of
// the two lists it enters.  Written once for the device steps (gevws_push.hip)
// and the host twin gevws_push_check (gevws_push_host.cpp).  The reference
// packs a pushed message on the host and sends it session by session
// (example/websocket/main.go:129-150 over connection.go:122); it has no
// record, no order and no lists.
// Plain C++: the host file also builds outside the library, under sanitizers
// (tests/cpp/push_fuzz.cpp).
#pragma once

#include <cstdint>

#include "gevws.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GEVWS_PUSH_HD __host__ __device__ __forceinline__
#else
#define GEVWS_PUSH_HD inline
#endif

namespace gevws_push_rule {

constexpr uint64_t kMaxPushes = 0xFFFFFFFFull;  // of one call
constexpr uint64_t kMaxLength = 0xFFFFFFFFull;  // of one body
constexpr uint64_t kMaxControl = 125;           // of a ping's or a pong's (RFC 6455 section 5.5)

// The list must not decrease in this.
GEVWS_PUSH_HD uint64_t key(const gevws_push& p) { return ((uint64_t)p.kind << 32) | p.target; }

GEVWS_PUSH_HD bool is_control(uint8_t opcode) { return opcode == 9 || opcode == 10; }

// Record p on its own and against the key of the record in front of it
// (has_prev false: p is the first): everything but the window bytes, which
// belong to the connections.  A record counts once, whatever is wrong with it.
GEVWS_PUSH_HD bool malformed(const gevws_push& p, bool has_prev, uint64_t prev_key, uint32_t n_conns,
                             uint32_t n_rooms, uint64_t src_bytes) {
  if (p.kind > GEVWS_PUSH_CONN) return true;
  if (p.kind == GEVWS_PUSH_ALL && p.target != 0) return true;
  if (p.kind == GEVWS_PUSH_ROOM && p.target >= n_rooms) return true;
  if (p.kind == GEVWS_PUSH_CONN && p.target >= n_conns) return true;
  if (p.opcode != 1 && p.opcode != 2 && !is_control(p.opcode)) return true;
  if (p.off % GEVWS_PAYLOAD_ALIGN != 0) return true;
  if (p.length > kMaxLength || p.off > src_bytes || p.length > src_bytes - p.off) return true;  // (no sum that could wrap)
  if (is_control(p.opcode) && p.length > kMaxControl) return true;
  for (int i = 0; i < 10; ++i)
    if (p.reserved[i]) return true;
  return has_prev && key(p) < prev_key;
}

// Which lists a well-formed record enters, from the number of its recipients
// that take plain (np) and that take deflate (nd): a control push is taken
// plain by every recipient.
GEVWS_PUSH_HD void lists(uint8_t opcode, uint64_t np, uint64_t nd, bool& plain, bool& deflate) {
  const bool ctl = is_control(opcode);
  plain = (ctl ? np + nd : np) > 0;
  deflate = !ctl && nd > 0;
}

}  // namespace gevws_push_rule
