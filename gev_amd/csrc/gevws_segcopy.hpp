// gevws_segcopy.hpp -- the byte-moving half of k_join_copy (gevws_join.hip) and
// k_send_gather (gevws_gather.hip): a list of byte segments copied into a
// 16-aligned region out[base, end) in 4 KiB output tiles.  A wave takes a tile
// a step, four 16-byte vectors a lane, 1 KiB apart; aligned non-temporal
// loads and stores, no LDS, no scratch memory.  What a segment is and how one
// is found is the caller's, a *map*:
//
//   Seg                        ds, de, src -- out[ds, de) come from src[0, de - ds)
//                              -- and whatever cursor the map needs
//   find(x, lo, hi, g) -> bool the segment that holds output byte x, among the
//                              tile map's entries [lo, hi]; false: x is a pad byte
//   next(g) -> bool            g -> the following segment with bytes (its ds may
//                              lie behind the old de: a pad gap); false: none
//   seek(T, lo, hi, have, g)   the segment at a tile's first byte, g the wave's
//                              last one when `have`; false: none, g is undefined
//   uniform(g)                 g's fields into SGPRs (every lane computed the same)
//
// A map checks every table entry where it reads it: tables that do not fit
// together give zeros here, never an address outside the map's checked ranges.
#pragma once

#include "gevws_kernels.hpp"

namespace {

constexpr int kSegBlock = 256;  // four waves
constexpr int kSegWaves = kSegBlock / 64;
constexpr int kSegVecs = (int)(kTile / (64 * 16));  // vectors a lane and tile: a wave takes a whole tile
static_assert(kSegVecs == 4, "one tile = four 1 KiB rows of a wave");
// Four waves a SIMD, the whole grid resident: k_join_copy has 114 VGPRs, k_send_gather 90, of 128.
constexpr int kSegWgPerCU = 4;
constexpr int kSegRounds = 4;            // segments of one tile a wave takes as whole rows ...
constexpr uint64_t kSegRowBytes = 1024;  // ... while they are at least this long; shorter ones lane by lane

// The destination vector at x assembled segment by segment: each segment's
// part from the one or two aligned source vectors that hold it (vectors with a
// counted byte only), gaps and bytes behind the last segment zero.
// seed: a segment that may hold x (the wave's current one), or null.
template <class Map>
__device__ __forceinline__ u32x4 seg_vector(const Map& M, uint64_t x, uint64_t lo, uint64_t hi,
                                            const typename Map::Seg* seed) {
  typename Map::Seg g;
  if (seed && x >= seed->ds && x < seed->de) g = *seed;
  else if (!M.find(x, lo, hi, g)) return u32x4{0, 0, 0, 0};  // a whole vector of pad
  u128 acc = 0;
  uint64_t p = x;
  const uint64_t xe = x + 16;
  for (;;) {
    const uint64_t stop = g.de < xe ? g.de : xe;
    const uint32_t cnt = (uint32_t)(stop - p);  // 1..16 bytes of this segment
    const uint8_t* sa = g.src + (p - g.ds);
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(sa) & 15);
    const uint8_t* a0 = sa - mis;
    u128 w = u128_of(ld16_nt(a0)) >> (8 * mis);
    if (mis + cnt > 16) w |= u128_of(ld16_nt(a0 + 16)) << (8 * (16 - mis));
    if (cnt < 16) w &= (((u128)1) << (8 * cnt)) - 1;
    acc |= w << (8 * (uint32_t)(p - x));
    p = stop;
    if (p >= xe || !M.next(g) || g.ds >= xe) break;  // (next is bounded by the map's own tables)
    if (g.ds > p) p = g.ds;
  }
  return u32x4_of(acc);
}

// The row rounds of the tile at T: while the wave's segment g is at least a row
// long, every lane copies its vectors that lie whole inside it -- all of a
// lane's loads before its first store -- the lane whose vector g's end cuts
// assembles that one from g, and the wave steps to the next segment.
// Returns the lane's `done` bits (bit u: vector u is stored).
template <class Map>
__device__ __forceinline__ uint32_t seg_rounds(const Map& M, typename Map::Seg& g, bool& have, uint64_t T, uint64_t lo,
                                               uint64_t hi, uint64_t end, uint32_t lane, uint8_t* __restrict__ out) {
  uint32_t done = 0;
  for (int round = 0; have && g.de - g.ds >= kSegRowBytes && round < kSegRounds; ++round) {
    // inside one segment the source is a constant byte shift off alignment (every x is on 16)
    const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(g.src) - g.ds) & 15);
    uint64_t x[kSegVecs];
    bool fast[kSegVecs];
    u32x4 v0[kSegVecs], v1[kSegVecs];
#pragma unroll
    for (int u = 0; u < kSegVecs; ++u) {
      x[u] = T + (uint64_t)u * 1024 + (uint64_t)lane * 16;
      // (end is on 16: a vector that starts below it is inside)
      fast[u] = !((done >> u) & 1) && x[u] >= g.ds && x[u] + 16 <= g.de && x[u] < end;
      if (fast[u]) {
        const uint8_t* a0 = g.src + (x[u] - g.ds) - mis;
        v0[u] = ld16_nt(a0);
        if (mis) v1[u] = ld16_nt(a0 + 16);
      }
    }
#pragma unroll
    for (int u = 0; u < kSegVecs; ++u)
      if (fast[u]) st16_nt(out + x[u], mis ? funnel16(v0[u], v1[u], mis) : v0[u]), done |= 1u << u;
    if (g.de >= T + kTile) break;
    // the vector the segment's end cuts starts inside it: no lookup for that one
#pragma unroll 1
    for (int u = 0; u < kSegVecs; ++u) {
      const uint64_t xu = T + (uint64_t)u * 1024 + (uint64_t)lane * 16;
      if (!((done >> u) & 1) && xu < end && xu >= g.ds && xu < g.de)
        st16_nt(out + xu, seg_vector(M, xu, lo, hi, &g)), done |= 1u << u;
    }
    // on to the next segment while segments are long enough for whole rows of the wave
    if (!M.next(g)) {
      have = false;
      break;
    }
    Map::uniform(g);
  }
  return done;
}

// A wave's tiles first, first + step, ... below stop, of the region's (tiles
// count from `base`, which is on 16 like `end`).  tile_map[t] is the map's
// entry (of n) that holds tile t's first byte: a byte of tile t is found
// between the entries of t and t + 1.  Every vector of every tile is stored
// exactly once, whole and inside [base, end).
template <class Map>
__device__ __forceinline__ void seg_copy_tiles(const Map& M, const uint32_t* __restrict__ tile_map, uint64_t n,
                                               uint64_t base, uint64_t end, uint64_t first, uint64_t stop,
                                               uint64_t step, uint8_t* __restrict__ out) {
  const uint64_t ntiles = (end - base + kTile - 1) / kTile;
  const uint32_t lane = threadIdx.x & 63;
  typename Map::Seg g;  // the wave's current segment, kept from tile to tile (wave-uniform)
  memset(&g, 0, sizeof(g));
  bool have = false;
  for (uint64_t t = first; t < stop; t += step) {
    const uint64_t T = base + t * kTile;
    uint64_t lo = tile_map[t], hi = t + 1 < ntiles ? (uint64_t)tile_map[t + 1] : n - 1;
    lo = lo < n ? lo : n - 1;
    hi = hi < n ? (hi > lo ? hi : lo) : n - 1;
    if (!(have && T >= g.ds && T < g.de)) {  // the segment at the tile's first byte
      have = M.seek(T, lo, hi, have, g);
      Map::uniform(g);
    }
    const uint32_t done = seg_rounds(M, g, have, T, lo, hi, end, lane, out);
    // what no round covered: short segments, pads, the start of what follows a pad
#pragma unroll 1
    for (int u = 0; u < kSegVecs; ++u) {
      const uint64_t xu = T + (uint64_t)u * 1024 + (uint64_t)lane * 16;
      if (!((done >> u) & 1) && xu < end) st16_nt(out + xu, seg_vector(M, xu, lo, hi, nullptr));
    }
  }
}

}  // namespace
