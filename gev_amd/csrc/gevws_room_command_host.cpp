// gevws_room_command_host.cpp -- gevws_room_command_parse (include/gevws.h):
// the rule gevws_room_commands.hip applies to a looked-at body
// (gevws_room_command.hpp), on host bytes.  Only body[0, length) is read.
// Plain C++: it also builds outside the library, under sanitizers
// (tests/cpp/room_command_fuzz.cpp).
#include <cstring>

#include "gevws.h"
#include "gevws_room_command.hpp"

extern "C" int gevws_room_command_parse(const uint8_t* body, uint64_t length, uint32_t n_rooms, uint32_t* room) {
  using namespace gevws_room_command;
  uint32_t r = GEVWS_ROOM_NONE;
  int cls = kNone;
  if (length >= kMinLength && length <= kMaxLength) {
    if (!body) return GEVWS_ERR_INVALID;
    uint8_t v[16] = {0};
    memcpy(v, body, (size_t)length);
    uint64_t lo = 0, hi = 0;
    for (int i = 0; i < 8; ++i) {  // little-endian words, whatever the host
      lo |= (uint64_t)v[i] << (8 * i);
      hi |= (uint64_t)v[8 + i] << (8 * i);
    }
    cls = classify(lo, hi, length, n_rooms, r);
  }
  if (room) *room = r;
  return cls;
}
