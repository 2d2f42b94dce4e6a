// room_command_fuzz.cpp -- gevws_room_command_parse (gev_amd/csrc/
// gevws_room_command_host.cpp, the rule of gevws_room_command.hpp) under
// AddressSanitizer and UndefinedBehaviorSanitizer: random and mutated bodies,
// each placed at the end of a heap block of exactly its length, so a read
// behind body[length) is a heap-buffer-overflow; every result against a second
// reading of the contract written here byte by byte.  Stand-alone: builds with
// g++ alone, needs no GPU (tests/test_room_command_sanitizers.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gevws.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

// The contract, read a byte at a time: {class, room}.
static int expect(const std::string& b, uint32_t n_rooms, uint32_t* room) {
  *room = GEVWS_ROOM_NONE;
  if (b.size() < 6 || b.size() > 16) return 0;
  if (b == "/leave") return 1;
  if (b.compare(0, 6, "/join ") != 0 || b.size() == 6) return 0;
  unsigned __int128 v = 0;
  for (size_t i = 6; i < b.size(); ++i) {
    if (b[i] < '0' || b[i] > '9') return 0;
    v = v * 10 + (unsigned)(b[i] - '0');
  }
  if (v >= n_rooms) return 2;
  *room = (uint32_t)v;
  return 1;
}

static long checked = 0, classes[3] = {0, 0, 0};

static bool check(const std::string& b, uint32_t n_rooms) {
  // the body ends where its allocation ends; a zero-length body gets a one-byte block it must not read
  uint8_t* block = static_cast<uint8_t*>(malloc(b.size() ? b.size() : 1));
  if (!block) return false;
  if (b.size()) memcpy(block, b.data(), b.size());
  uint32_t got_room = 0x12345678u, want_room;
  const int got = gevws_room_command_parse(b.size() ? block : block + 1, b.size(), n_rooms, &got_room);
  const int again = gevws_room_command_parse(block, b.size(), n_rooms, nullptr);  // a NULL room is allowed
  free(block);
  const int want = expect(b, n_rooms, &want_room);
  if (got != want || again != want || got_room != want_room) {
    fprintf(stderr, "mismatch on a body of %zu bytes, n_rooms %u: got %d / %u, want %d / %u\n", b.size(), n_rooms, got,
            got_room, want, want_room);
    return false;
  }
  ++checked, ++classes[want];
  return true;
}

int main() {
  const uint32_t rooms[] = {0, 1, 2, 7, 10, 1000, 0x7FFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu};
  const char* seeds[] = {"/leave", "/join 0", "/join 6", "/join 10", "/join 999", "/join 4294967295", "/join 4294967296",
                         "/join 9999999999", "/join 0000000001", "/join 2147483647", "/join ", "/join", "/leave ",
                         "/JOIN 3", "/join 3\n", "/join 00000000001", "hello", ""};
  const char alphabet[] = "/joinleave 0123456789\n+-J\0\xff";
  for (uint32_t n_rooms : rooms) {
    for (const char* s : seeds) {
      const std::string base(s);
      if (!check(base, n_rooms)) return 1;
      for (size_t k = 0; k <= base.size(); ++k)  // every prefix
        if (!check(base.substr(0, k), n_rooms)) return 1;
      for (size_t i = 0; i < base.size(); ++i) {  // every single-byte mutation
        for (int v = 0; v < 256; ++v) {
          std::string m = base;
          m[i] = (char)v;
          if (!check(m, n_rooms)) return 1;
        }
      }
      for (int v = 0; v < 256; ++v)  // one more byte behind it
        if (!check(base + (char)v, n_rooms)) return 1;
    }
  }
  for (int it = 0; it < 400000; ++it) {  // random bodies over a narrow alphabet, lengths 0..20
    const size_t len = rnd() % 21;
    std::string b;
    const uint64_t kind = rnd() % 4;
    if (kind == 0) b = "/join ";
    if (kind == 1) b = "/leave";
    while (b.size() < len) {
      const uint64_t r = rnd();
      b += (kind == 0 && r % 8) ? (char)('0' + (r >> 8) % 10) : alphabet[(r >> 8) % (sizeof(alphabet) - 1)];
    }
    b.resize(len);
    if (!check(b, rooms[rnd() % (sizeof(rooms) / sizeof(rooms[0]))])) return 1;
  }
  // a length outside 6..16 reads nothing, a NULL body included; inside it a NULL body is an invalid call
  uint32_t room = 5;
  if (gevws_room_command_parse(nullptr, 0, 3, &room) != 0 || room != GEVWS_ROOM_NONE) return 1;
  if (gevws_room_command_parse(nullptr, 17, 3, &room) != 0 || gevws_room_command_parse(nullptr, ~0ull, 3, &room) != 0) return 1;
  if (gevws_room_command_parse(nullptr, 6, 3, &room) != GEVWS_ERR_INVALID) return 1;
  if (!classes[0] || !classes[1] || !classes[2]) return 1;
  printf("room_command_fuzz ok: %ld bodies (%ld none, %ld changes, %ld rejected)\n", checked, classes[0], classes[1],
         classes[2]);
  return 0;
}
