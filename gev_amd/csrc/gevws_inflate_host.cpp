// gevws_inflate_host.cpp -- gevws_inflate_raw (include/gevws.h): the decode
// core of gevws_inflate_core.hpp on host memory.  Plain C++: it also builds
// outside the library, under sanitizers (tests/cpp/inflate_fuzz.cpp).
#include "gevws.h"
#include "gevws_inflate_core.hpp"

namespace {

// S = in[0, n) then 00 00 ff ff; the sink is out[0, cap).
struct HostIo {
  const uint8_t* in;
  uint64_t n, rd;
  uint8_t* out;
  uint64_t wr;
  bool get(uint32_t& b) {
    if (rd < n) {
      b = in[rd++];
      return true;
    }
    if (rd < n + 4) {
      b = rd - n < 2 ? 0x00u : 0xffu;
      ++rd;
      return true;
    }
    return false;
  }
  void put(uint32_t b) { out[wr++] = (uint8_t)b; }
  void copy(uint32_t d, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i, ++wr) out[wr] = out[wr - d];
  }
  uint64_t stored(uint64_t want) {
    uint64_t got = 0;
    uint32_t b;
    while (got < want && get(b)) put(b), ++got;
    return got;
  }
};

}  // namespace

extern "C" int gevws_inflate_raw(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len) {
  if (out_len) *out_len = 0;
  if ((n && !in) || (cap && !out)) return GEVWS_ERR_INVALID;
  gevws_inflate::Tables t;
  HostIo io{in, n, 0, out, 0};
  uint64_t produced = 0;
  const int st = gevws_inflate::inflate(io, t, cap, &produced);
  if (out_len) *out_len = produced;
  return st;
}
