// gevws_dispatch.hpp -- what HandlerWrap.OnMessage (plugins/websocket/wrap.go:38-90)
// answers to one decoded frame, shared by the frame-level dispatch
// (gevws_encode.hip: k_disp_count / k_disp_emit / k_handle_small) and the
// message chain's control step (gevws_respond.hip): the kind of reply, the
// close-reply body of util.HandleClose (util.go:27-46) with
// CheckCloseFrameData's texts (util.go:65-85), and the reply record itself.
// Included inside each file's own anonymous namespace copy, as
// gevws_kernels.hpp is; nothing here has external linkage.
#pragma once

#include "gevws_kernels.hpp"

namespace {

constexpr uint32_t kAuxSlot = 128;  // one close body (<= 125 bytes) per slot

__device__ __constant__ char kErrNotInUse[] = "status code is not in use";
__device__ __constant__ char kErrAppLevel[] = "status code is only application level";
__device__ __constant__ char kErrNoMeaning[] = "status code has no meaning yet";
__device__ __constant__ char kErrUnknown[] = "status code is not defined in spec";
__device__ __constant__ char kErrUtf8[] = "invalid utf8 sequence in close reason";

// unicode/utf8.ValidString: strict UTF-8.
__device__ bool utf8_valid(const uint8_t* p, uint64_t n) {
  uint64_t i = 0;
  while (i < n) {
    const uint32_t c = p[i];
    if (c < 0x80) { ++i; continue; }
    uint32_t need, lo = 0x80, hi = 0xBF;
    if (c >= 0xC2 && c <= 0xDF) need = 1;
    else if (c == 0xE0) { need = 2; lo = 0xA0; }
    else if ((c >= 0xE1 && c <= 0xEC) || c == 0xEE || c == 0xEF) need = 2;
    else if (c == 0xED) { need = 2; hi = 0x9F; }
    else if (c == 0xF0) { need = 3; lo = 0x90; }
    else if (c >= 0xF1 && c <= 0xF3) need = 3;
    else if (c == 0xF4) { need = 3; hi = 0x8F; }
    else return false;
    if (i + need >= n) return false;  // truncated sequence
    const uint32_t c1 = p[i + 1];
    if (c1 < lo || c1 > hi) return false;
    for (uint32_t k = 2; k <= need; ++k)
      if ((p[i + k] & 0xC0) != 0x80) return false;
    i += need + 1;
  }
  return true;
}

// 0: no reply, 1: reply with the frame's own payload, 2: close reply (aux body), 3: bare close header
__device__ __forceinline__ int disp_kind(const gevws_header& h, int policy, uint32_t& op_out) {
  const uint32_t op = h.opcode;
  if (op & 8) {
    if (op == 0x8) return h.length == 0 ? 3 : 2;
    if (op == 0x9) { op_out = 0xA; return 1; }
    if (op == 0xA) { op_out = 0x9; return 1; }
    return 0;
  }
  if (policy == GEVWS_HANDLER_NONE || h.length <= 0) return 0;
  op_out = policy == GEVWS_HANDLER_ECHO_BINARY ? 0x2u : 0x1u;
  return 1;
}

__device__ void put_close_body(uint8_t* dst, uint32_t code, const uint8_t* reason, uint64_t rlen, uint32_t& n) {
  // ws.NewCloseFrameBody (frame.go:251-259): BE16 code + reason cropped to 123 bytes
  const uint64_t crop = rlen < 123 ? rlen : 123;
  dst[0] = (uint8_t)(code >> 8);
  dst[1] = (uint8_t)code;
  for (uint64_t i = 0; i < crop; ++i) dst[2 + i] = reason[i];
  n = (uint32_t)(2 + crop);
}

__device__ void put_close_error(uint8_t* dst, const char* msg, uint32_t& n) {
  uint64_t len = 0;
  while (msg[len]) ++len;
  put_close_body(dst, 1002, reinterpret_cast<const uint8_t*>(msg), len, n);  // StatusProtocolError
}

// One reply record (and for a close its aux-slot body) for decoded frame f.
__device__ __forceinline__ void disp_reply(const gevws_frame& in, int kind, uint32_t op, uint64_t f, uint64_t r,
                                        uint64_t slot, const uint8_t* __restrict__ payload, uint64_t aux_off,
                                        gevws_out_frame* __restrict__ rep, int64_t* __restrict__ reply_of,
                                        uint8_t* __restrict__ aux_base) {
  reply_of[f] = (int64_t)r;
  gevws_out_frame o;
  memset(&o, 0, sizeof(o));
  o.hdr.fin = 1;
  if (kind == 1) {
    o.hdr.opcode = (uint8_t)op;
    o.hdr.length = in.hdr.length;
    o.payload_off = in.payload_off;
    o.payload_len = (uint64_t)in.hdr.length;
  } else if (kind == 3) {
    o.hdr.opcode = 0x8;  // WriteHeader(&Header{Fin: true, OpCode: OpClose}), util.go:28-33
  } else {
    uint8_t* body = aux_base + slot * kAuxSlot;
    const uint8_t* p = payload + in.payload_off;
    const uint64_t L = (uint64_t)in.hdr.length;
    uint32_t code = 0;
    const uint8_t* reason = p;
    uint64_t rlen = 0;
    if (L >= 2) {  // ParseCloseFrameData, read.go:89-102
      code = ((uint32_t)p[0] << 8) | p[1];
      reason = p + 2;
      rlen = L - 2;
    }
    uint32_t nb;
    const bool defined = code == 1000 || code == 1001 || code == 1002 || code == 1003 || code == 1007 ||
                         code == 1008 || code == 1009 || code == 1010 || code == 1011 || code == 1005 ||
                         code == 1006 || code == 1015;
    if (code <= 999) put_close_error(body, kErrNotInUse, nb);
    else if (code == 1005 || code == 1006 || code == 1015) put_close_error(body, kErrAppLevel, nb);
    else if (code == 1004) put_close_error(body, kErrNoMeaning, nb);
    else if (code >= 1000 && code <= 2999 && !defined) put_close_error(body, kErrUnknown, nb);
    else if (!utf8_valid(reason, rlen)) put_close_error(body, kErrUtf8, nb);
    else put_close_body(body, code, reason, rlen, nb);
    o.hdr.opcode = 0x8;
    o.hdr.length = nb;
    o.payload_off = aux_off + slot * kAuxSlot;
    o.payload_len = nb;
  }
  rep[r] = o;
}

}  // namespace
