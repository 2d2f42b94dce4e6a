// gevws_room_command.hpp -- the rule that reads a room command out of a text
// message's bytes, written once for the device step (gevws_room_commands.hip)
// and its host twin (gevws_room_command_host.cpp), both declared in
// include/gevws.h.  The reference has no rooms and no commands
// (example/websocket/main.go sends every message to every session).
//
// A command is at most 16 bytes, so one aligned 16-byte vector of the body
// decides: the rule takes it as two little-endian 64-bit words (byte i of the
// body is byte i of lo for i < 8, byte i - 8 of hi behind that) plus the
// body's length; only the first `length` bytes count, whatever the pad holds.
//   - leave: the 6 bytes "/leave".
//   - join: the 6 bytes "/join " and 1..10 bytes '0'..'9' behind them, nothing
//     else; leading zeros allowed.  The value (at most 9 999 999 999: 64 bits
//     hold it) names the room when it is < n_rooms; otherwise the command is
//     rejected.  GEVWS_ROOM_NONE is never < n_rooms, so 4294967295 never joins.
//   - anything else -- "/join" without digits, a byte behind the digits,
//     another letter case, "/leave " -- is no command.
// Which bodies are looked at (delivered, text, 6..16 bytes) is the caller's.
// Plain C++: the host file also builds outside the library, under sanitizers
// (tests/cpp/room_command_fuzz.cpp).
#pragma once

#include <cstdint>

#include "gevws.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GEVWS_CMD_HD __host__ __device__ __forceinline__
#else
#define GEVWS_CMD_HD inline
#endif

namespace gevws_room_command {

constexpr int kNone = 0;      // no command
constexpr int kChange = 1;    // a join, a move or a leave: {conn, room}
constexpr int kRejected = 2;  // a join whose room is not < n_rooms

constexpr uint64_t kMinLength = 6, kMaxLength = 16;  // of a body that can be a command
constexpr uint64_t kKeyMask = 0xFFFFFFFFFFFFull;     // the keyword: bytes 0..5
constexpr uint64_t kLeave = 0x657661656C2Full;       // "/leave"
constexpr uint64_t kJoin = 0x206E696F6A2Full;        // "/join "

// The class of a body of `length` bytes whose first 16 are {lo, hi}; room: the
// change's room (GEVWS_ROOM_NONE for a leave, and whenever there is no change).
GEVWS_CMD_HD int classify(uint64_t lo, uint64_t hi, uint64_t length, uint32_t n_rooms, uint32_t& room) {
  room = GEVWS_ROOM_NONE;
  if (length < kMinLength || length > kMaxLength) return kNone;
  const uint64_t key = lo & kKeyMask;
  if (length == kMinLength) return key == kLeave ? kChange : kNone;
  if (key != kJoin) return kNone;
  uint64_t value = 0;
  bool digits = true;
  for (uint32_t i = 6; i < 16; ++i) {  // (a byte at or behind `length` never counts; no early exit: straight code)
    const uint32_t d = (uint32_t)((i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8))) & 0xFF) - '0';
    const bool in = i < length;
    digits &= !in || d <= 9;
    value = in ? value * 10 + d : value;
  }
  if (!digits) return kNone;
  if (value >= n_rooms) return kRejected;
  room = (uint32_t)value;
  return kChange;
}

}  // namespace gevws_room_command
