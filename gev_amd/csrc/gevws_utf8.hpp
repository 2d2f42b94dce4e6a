// gevws_utf8.hpp -- the strict UTF-8 rule (unicode/utf8.Valid) per byte and per
// 16-byte vector, shared by the message layer's text check (gevws_message.hip)
// and the check of inflated text (gevws_inflate.hip).  Included after
// gevws_kernels.hpp; like it, nothing here has external linkage.
#pragma once

#include "gevws_kernels.hpp"

namespace {

// ------------------------------------------------------------------ the UTF-8 rule
// Whether byte c is wrong after the bytes p3 p2 p1 (0 before the start): a
// byte is a continuation (10xxxxxx) exactly when a lead byte one, two or three
// places back still asks for one; C0, C1 and F5..FF never appear; and the byte
// after E0 / ED / F0 / F4 stays in the narrowed range (no overlong forms, no
// surrogates, nothing above U+10FFFF).  unicode/utf8.Valid accepts exactly the
// strings with no wrong byte that do not end inside a sequence.
__host__ __device__ __forceinline__ uint32_t utf8_byte_bad(uint32_t c, uint32_t p1, uint32_t p2, uint32_t p3) {
  const bool must = p1 >= 0xC0 || p2 >= 0xE0 || p3 >= 0xF0;
  const bool cont = (c & 0xC0) == 0x80;
  return (uint32_t)((must != cont) || c == 0xC0 || c == 0xC1 || c >= 0xF5 || (p1 == 0xE0 && c < 0xA0) ||
                    (p1 == 0xED && c > 0x9F) || (p1 == 0xF0 && c < 0x90) || (p1 == 0xF4 && c > 0x8F));
}
// Continuation bytes a lead byte asks for.
__host__ __device__ __forceinline__ uint32_t utf8_need(uint32_t c) {
  return (uint32_t)(c >= 0xC0) + (uint32_t)(c >= 0xE0) + (uint32_t)(c >= 0xF0);
}

// Bit i = byte i of the vector v is wrong; prevw = the four bytes before it.
// A vector of ASCII can only be wrong in its first three bytes, after an
// unfinished sequence.
__device__ __forceinline__ uint32_t utf8_err16(u32x4 v, uint32_t prevw) {
  uint32_t p1 = prevw >> 24, p2 = (prevw >> 16) & 0xff, p3 = (prevw >> 8) & 0xff;
  if (((v[0] | v[1] | v[2] | v[3]) & 0x80808080u) == 0)
    return (uint32_t)(p1 >= 0xC0 || p2 >= 0xE0 || p3 >= 0xF0) | ((uint32_t)(p1 >= 0xE0 || p2 >= 0xF0) << 1) |
           ((uint32_t)(p1 >= 0xF0) << 2);
  uint32_t err = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t c = (v[w] >> (8 * b)) & 0xff;
      err |= utf8_byte_bad(c, p1, p2, p3) << (4 * w + b);
      p3 = p2;
      p2 = p1;
      p1 = c;
    }
  }
  return err;
}

// Wrong bytes among [lead, L) of vector j of the frame at p (16-byte aligned):
// the leading continuation bytes belong to the previous fragment's sequence
// and the bytes from L on are pad.
__device__ __forceinline__ uint32_t utf8_vec_bad(u32x4 v, uint32_t prevw, uint64_t j, uint64_t L, uint32_t lead) {
  const uint64_t left = L - 16 * j;
  uint32_t mask = left >= 16 ? 0xffffu : ((1u << (uint32_t)left) - 1u);
  if (j == 0) mask &= ~((1u << lead) - 1u);
  return utf8_err16(v, prevw) & mask;
}

}  // namespace
