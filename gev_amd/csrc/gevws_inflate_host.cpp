// gevws_inflate_host.cpp -- gevws_inflate_raw (include/gevws.h): the decode
// core of gevws_inflate_core.hpp on host memory.  Plain C++: it also builds
// outside the library, under sanitizers (tests/cpp/inflate_fuzz.cpp), and
// gevws_inflate_raw_ctx, the same over one connection's context slot
// (tests/cpp/inflate_ctx_fuzz.cpp).
#include <cstring>

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

// The same over one connection's slot (context takeover): a copy may reach
// behind out[0] into the slot's ring, where stream byte i sits at i & 32767.
constexpr uint64_t kWin = 32768, kHead = GEVWS_INF_CTX_BYTES - kWin;
static_assert(kHead == 64, "the slot's head");
struct HostCtxIo : HostIo {
  const uint8_t* ring;
  uint64_t total;  // stream bytes before out[0]
  void copy(uint32_t d, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i, ++wr) out[wr] = d <= wr ? out[wr - d] : ring[(total + wr - d) & (kWin - 1)];
  }
};

}  // namespace

extern "C" int gevws_inflate_raw_ctx(const uint8_t* in, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* out_len,
                                     uint8_t* ctx) {
  if (out_len) *out_len = 0;
  if ((n && !in) || (cap && !out) || !ctx) return GEVWS_ERR_INVALID;
  uint64_t total;
  memcpy(&total, ctx, sizeof(total));
  if (ctx[8]) return ctx[8];  // the context was lost: sticky, nothing is decoded
  gevws_inflate::Tables t;
  HostCtxIo io{{in, n, 0, out, 0}, ctx + kHead, total};
  uint64_t produced = 0;
  const int st = gevws_inflate::inflate(io, t, cap, &produced, (uint32_t)(total < kWin ? total : kWin));
  if (out_len) *out_len = produced;
  if (st != GEVWS_MSG_OK) {
    ctx[8] = (uint8_t)st;
    return st;
  }
  for (uint64_t i = produced > kWin ? produced - kWin : 0; i < produced; ++i) ctx[kHead + ((total + i) & (kWin - 1))] = out[i];
  total += produced;
  memcpy(ctx, &total, sizeof(total));
  return st;
}

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
