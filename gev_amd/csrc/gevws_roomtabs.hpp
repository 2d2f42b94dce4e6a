// gevws_roomtabs.hpp -- what the steps that read the caller's room tables
// share (gevws_rooms.hip: the room broadcast; gevws_push.hip: the push pass):
// the gates of a chained call, the tables, the recipient kind of
// include/gevws.h ("Recipient kind") and the table check, one lane per record.
// Device code only; each file includes it into its own anonymous namespace
// copy, as it does gevws_kernels.hpp.
#pragma once

#include "gevws_kernels.hpp"

namespace {

constexpr uint32_t kNoRoom = GEVWS_ROOM_NONE;
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

// The summaries that gate a call: every `must` (null: none) has to be OK, the
// records are the first min(count->frames, max).
constexpr int kGateMax = 6;
struct Gates {
  const gevws_summary* must[kGateMax];
  const gevws_summary* count;
  uint64_t max;
};
__device__ __forceinline__ uint64_t gate_count(const Gates& g) {
#pragma unroll
  for (int i = 0; i < kGateMax; ++i)
    if (g.must[i] && g.must[i]->status != GEVWS_OK) return 0;
  return gated_count(g.max, g.count);
}

struct RoomTabs {
  const uint32_t* __restrict__ conn_room;  // [n_conns]
  const uint32_t* __restrict__ first;      // [n_rooms + 1]
  const uint32_t* __restrict__ members;    // [n_members]
  uint32_t n_rooms, n_members, n_conns;
};

__device__ __forceinline__ bool takes_deflate(const uint8_t* __restrict__ ext, uint32_t c) {
  if (!ext) return false;
  const uint32_t e = ext[c];
  return (e & GEVWS_EXT_DEFLATE) && !(e & GEVWS_EXT_SERVER_TAKEOVER);
}

__device__ __forceinline__ void count_up(uint64_t* __restrict__ counter, uint64_t v) {
  const uint64_t sm = wave_sum(v);
  if ((threadIdx.x & 63) == 0 && sm) atomicAdd(reinterpret_cast<unsigned long long*>(counter), (unsigned long long)sm);
}

// ------------------------------------------------------------------ the table check
struct RoomRec {
  uint32_t bad;     // malformed records among this lane's (a record counts once)
  uint32_t roomed;  // connection i has a room
  uint32_t room;    // member slot i's room (kNoRoom: none)
  uint32_t member;  // member slot i's connection, when it is one (else kNoSlot)
  bool member_bad;  // member slot i's record is among the malformed
};
// Lane i checks room record i (i <= n_rooms), member slot i (i < n_members)
// and connection i (i < n_conns).  Every index is bounded before it is used;
// the slot's room comes from a bisection of `first` whose every probe lies in
// [0, n_rooms), whatever the table holds.
__device__ __forceinline__ RoomRec rooms_check(const RoomTabs& T, uint64_t i) {
  RoomRec r{0u, 0u, kNoRoom, kNoSlot, false};
  if (i <= T.n_rooms) {
    const uint32_t fi = T.first[i];
    bool bad = i == 0 && fi != 0;
    if (i < T.n_rooms) bad |= fi > T.first[i + 1];
    else bad |= fi != T.n_members || T.n_members > T.n_conns;
    r.bad += bad;
  }
  if (i < T.n_members) {
    bool bad = T.n_rooms == 0;
    if (!bad) {
      uint32_t lo = 0, hi = T.n_rooms - 1;
      while (lo < hi) {  // (at most 32 rounds)
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        if (T.first[mid] <= i) lo = mid;
        else hi = mid - 1;
      }
      const uint32_t g = lo, a = T.first[g], b = T.first[g + 1];
      r.room = g;
      bad = !(a <= i && i < b);
      const uint32_t m = T.members[i];
      if (m >= T.n_conns) {
        bad = true;
      } else {
        r.member = m;
        bad |= T.conn_room[m] != g;
      }
      if (a < i) bad |= T.members[i - 1] >= m;  // strictly increasing inside a room
    }
    r.bad += bad;
    r.member_bad = bad;
  }
  if (i < T.n_conns) {
    const uint32_t g = T.conn_room[i];
    r.roomed = g != kNoRoom;
    r.bad += g != kNoRoom && g >= T.n_rooms;
  }
  return r;
}

}  // namespace
