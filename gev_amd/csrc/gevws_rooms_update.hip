// gevws_rooms_update.hip -- membership changes on the device
// (gevws_rooms_update_async; include/gevws.h): join / move / leave records and
// the pass's closes applied to d_conn_room, and the CSR inverse of the result
// rebuilt, all on the stream.  The reference keeps its sessions in a host map
// (example/websocket/main.go: serv.sessions under a mutex); Rooms.csr is the
// host form of what this file computes, a stable argsort of the roomed
// connections by room.
//
// One memset and, for a sort of P passes (P = the bytes of n_rooms - 1, one
// for a single room, none without rooms), 8 + 5 P launches (7 + 5 P without a
// change list), no host round trip:
//   k_ru_changes   one lane per change: the record checked, then
//                  atomicMax(last[conn], i + 1) -- the largest index is the last
//                  in list order, whichever lane retires last
//   k_ru_resolve   one lane per connection: d_conn_room_in[c] checked, the new
//                  room (its last change, else the old room; none when the
//                  pass closed it) into scratch, cnt[room] += 1 (integer
//                  atomics, in LDS first when the rooms fit there:
//                  order-independent), block partials
//   k_scan_blocks / k_ru_verdict
//                  the summary; a failed gate or a bad record ends the call here
//   k_ru_sum / k_scan_blocks / k_ru_excl
//                  the exclusive scan of cnt: d_room_first_out
//   per pass: k_ru_hist        a digit histogram per workgroup (LDS), written
//                              digit-major / block-minor
//             k_ru_sum / k_scan_blocks / k_ru_excl
//                              that table scanned in place
//             k_ru_scatter     the stable scatter: a key's place is its rank
//                              among equal digits in its wave (ballots over the
//                              digit's bits, a popcount of the lower lanes), its
//                              wave's offset in the workgroup (an LDS table
//                              walked in wave order) and the scanned base.  No
//                              atomic places anything: the order would be lost.
//   k_ru_copy      the resolved rooms into d_conn_room_out
// The first pass reads the resolved rooms and drops the connections without a
// room; (room, connection) pairs ping-pong in scratch between passes; the last
// pass writes d_room_members_out.  Nothing but the summary is written before
// the verdict, every writer of an output returns unless the summary is
// GEVWS_OK, and every index is bounded before it is used.
#include "gevws_internal.hpp"

namespace {

static_assert(sizeof(gevws_room_change) == 8 && offsetof(gevws_room_change, room) == 4, "gevws_room_change layout");
static_assert(sizeof(gevws_conn_send) == 32 && offsetof(gevws_conn_send, flags) == 24, "gevws_conn_send layout");

constexpr uint32_t kNoRoom = GEVWS_ROOM_NONE;
constexpr int kRuRounds = 4;                          // rounds of kWalkBlock consecutive keys a workgroup
constexpr uint32_t kRuKeys = kWalkBlock * kRuRounds;  // the sort's keys per workgroup
constexpr uint32_t kRuScanPer = 4;                    // k_ru_sum / k_ru_excl: entries per lane
constexpr uint32_t kRuScanTile = kWalkBlock * kRuScanPer;
constexpr uint32_t kRuLdsRooms = 4096;  // k_ru_resolve counts up to this many rooms in LDS (16 KiB)
constexpr int kRuDigits = 256;
constexpr int kRuWaves = kWalkBlock / 64;
static_assert(kRuDigits == kWalkBlock, "one lane per digit in the scatter's LDS tables");

constexpr int kCtlBadChange = 0;  // ctl[]: malformed change records

struct RuGates {
  const gevws_summary* __restrict__ prev;  // may be null; also the change count's gate
  const gevws_summary* __restrict__ plan;  // may be null
};
// The first failing gate's status (GEVWS_OK: none).
__device__ __forceinline__ int ru_gate(const RuGates& g) {
  if (g.prev && g.prev->status != GEVWS_OK) return g.prev->status;
  if (g.plan && g.plan->status != GEVWS_OK) return g.plan->status;
  return GEVWS_OK;
}

__device__ __forceinline__ void count_up(uint64_t* __restrict__ counter, uint64_t v) {
  const uint64_t sm = wave_sum(v);
  if ((threadIdx.x & 63) == 0 && sm) atomicAdd(reinterpret_cast<unsigned long long*>(counter), (unsigned long long)sm);
}

// ------------------------------------------------------------------ changes, resolve, verdict
__global__ __launch_bounds__(kWalkBlock) void k_ru_changes(const gevws_room_change* __restrict__ changes,
                                                           uint64_t max_changes, RuGates G, uint32_t n_conns,
                                                           uint32_t n_rooms, uint32_t* __restrict__ last,
                                                           uint64_t* __restrict__ ctl) {
  uint64_t bad = 0;
  if (ru_gate(G) == GEVWS_OK) {
    const uint64_t n = gated_count(max_changes, G.prev);
    const uint64_t i = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
    if (i < n) {
      const gevws_room_change ch = changes[i];
      if (ch.conn >= n_conns || (ch.room >= n_rooms && ch.room != kNoRoom)) bad = 1;
      else atomicMax(last + ch.conn, (uint32_t)(i + 1));  // (i + 1 < 2^32: the call bounds max_changes)
    }
  }
  count_up(ctl + kCtlBadChange, bad);
}

// A workgroup resolves kRuKeys connections.  LDSCNT (n_rooms <= kRuLdsRooms):
// it counts its rooms in LDS and adds each non-empty one to cnt[] once -- a
// global atomic a connection queues a million of them on a few hundred
// addresses (1 M connections in 256 rooms: the whole call 0.51 ms that way,
// 0.079 ms this way).
template <bool LDSCNT>
__global__ __launch_bounds__(kWalkBlock) void k_ru_resolve(const uint32_t* __restrict__ room_in,
                                                           const gevws_room_change* __restrict__ changes,
                                                           const gevws_conn_send* __restrict__ conn_send, RuGates G,
                                                           uint32_t n_conns, uint32_t n_rooms,
                                                           const uint32_t* __restrict__ last,
                                                           uint32_t* __restrict__ room_new, uint32_t* __restrict__ cnt,
                                                           uint64_t* __restrict__ blk) {
  __shared__ uint32_t s_cnt[LDSCNT ? kRuLdsRooms : 1];
  if constexpr (LDSCNT) {
    for (uint32_t g = threadIdx.x; g < n_rooms; g += kWalkBlock) s_cnt[g] = 0;  // (n_rooms <= kRuLdsRooms)
    __syncthreads();
  }
  const bool open = ru_gate(G) == GEVWS_OK;
  uint64_t vals[4] = {0, 0, 0, 0};  // members, (changes read: the verdict's), moved, bad records
#pragma unroll
  for (int j = 0; j < kRuRounds; ++j) {
    const uint64_t c = (uint64_t)blockIdx.x * kRuKeys + (uint32_t)j * kWalkBlock + threadIdx.x;
    if (c >= n_conns || !open) continue;
    const uint32_t r = room_in[c];
    uint32_t nr = r;
    // last[c] names a change that k_ru_changes checked: below the count, its room < n_rooms or none
    const uint32_t l = changes ? last[c] : 0u;
    if (l) nr = changes[l - 1].room;
    if (conn_send && (conn_send[c].flags & GEVWS_CTL_SHUTDOWN)) nr = kNoRoom;
    room_new[c] = nr;
    if (nr < n_rooms) {
      if constexpr (LDSCNT) atomicAdd(&s_cnt[nr], 1u);
      else atomicAdd(cnt + nr, 1u);
      vals[0] += 1;
    }
    vals[2] += nr != r;
    vals[3] += r >= n_rooms && r != kNoRoom;
  }
  if constexpr (LDSCNT) {
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < n_rooms; g += kWalkBlock) {
      const uint32_t v = s_cnt[g];
      if (v) atomicAdd(cnt + g, v);
    }
  }
  block_partial<4>(vals, blk, blockIdx.x);
}

// The scan left {members, 0, moved, bad connections} in *sum: the summary from
// them, from the gates and from the bad changes.
__global__ void k_ru_verdict(RuGates G, uint64_t max_changes, int have_changes, const uint64_t* __restrict__ ctl,
                             gevws_summary* __restrict__ sum) {
  const gevws_summary s = *sum;
  gevws_summary o;
  memset(&o, 0, sizeof(o));
  const int gate = ru_gate(G);
  if (gate != GEVWS_OK) {
    o.status = gate;
  } else {
    const uint64_t bad = s.errors + ctl[kCtlBadChange];
    if (bad) {
      o.errors = bad;
      o.status = GEVWS_ERR_INVALID;
    } else {
      o.frames = s.frames;
      o.payload_len = s.payload_len;
      o.payload_bytes = have_changes ? gated_count(max_changes, G.prev) : 0;
    }
  }
  *sum = o;
}

// ------------------------------------------------------------------ exclusive scan of a u32 table
// Per-block sums of src[0, n) (kRuScanTile entries a block) for k_scan_blocks:
// the whole row of the partial, so the scan reads nothing that was not written.
// gate (may be null): unless it is GEVWS_OK src was not written (k_ru_hist
// returned) and is not read; the partials are zero.
__global__ __launch_bounds__(kWalkBlock) void k_ru_sum(const uint32_t* __restrict__ src, uint64_t n,
                                                       const gevws_summary* __restrict__ gate,
                                                       uint64_t* __restrict__ blk) {
  const uint64_t i0 = ((uint64_t)blockIdx.x * kWalkBlock + threadIdx.x) * kRuScanPer;
  uint64_t vals[kBlkFields] = {0, 0, 0, 0};
  if (!gate || gate->status == GEVWS_OK) {
#pragma unroll
    for (uint32_t r = 0; r < kRuScanPer; ++r)
      if (i0 + r < n) vals[0] += src[i0 + r];
  }
  block_partial<kBlkFields>(vals, blk, blockIdx.x);
}

// dst[i] = the sum of src[0, i) for i < n_out, with src taken as 0 at and
// behind n (n_out = n + 1 writes the total too).  dst may be src: a lane reads
// its entries before it writes them and nobody else's.  gate (may be null):
// returns unless it is GEVWS_OK.
__global__ __launch_bounds__(kWalkBlock) void k_ru_excl(const uint32_t* src, uint64_t n, uint64_t n_out,
                                                        const uint64_t* __restrict__ blk,
                                                        const gevws_summary* __restrict__ gate, uint32_t* dst) {
  if (gate && gate->status != GEVWS_OK) return;
  const uint64_t i0 = ((uint64_t)blockIdx.x * kWalkBlock + threadIdx.x) * kRuScanPer;
  uint32_t x[kRuScanPer];
  uint64_t v[1] = {0}, ex[1], tot[1];
#pragma unroll
  for (uint32_t r = 0; r < kRuScanPer; ++r) {
    x[r] = i0 + r < n ? src[i0 + r] : 0u;
    v[0] += x[r];
  }
  block_excl_scan<kWalkBlock, 1>(v, ex, tot);
  uint64_t at = blk[(uint64_t)blockIdx.x * kBlkFields] + ex[0];
#pragma unroll
  for (uint32_t r = 0; r < kRuScanPer; ++r) {
    if (i0 + r < n_out) dst[i0 + r] = (uint32_t)at;
    at += x[r];
  }
}

// ------------------------------------------------------------------ the sort
struct RuSrc {
  const uint32_t* __restrict__ keys;  // the first pass: the resolved rooms; later: the pairs' rooms
  const uint32_t* __restrict__ vals;  // later passes: the pairs' connections
  uint32_t n_conns;
};
// Key idx of a pass: false when there is none (behind the end, or, in the
// first pass, a connection without a room).
template <bool FIRST>
__device__ __forceinline__ bool ru_key(const RuSrc& S, uint64_t n_members, uint64_t idx, uint32_t& key,
                                       uint32_t& val) {
  key = 0, val = 0;
  if constexpr (FIRST) {
    if (idx >= S.n_conns) return false;
    key = S.keys[idx], val = (uint32_t)idx;
    return key != kNoRoom;
  } else {
    if (idx >= n_members || idx >= S.n_conns) return false;
    key = S.keys[idx], val = S.vals[idx];
    return true;
  }
}

template <bool FIRST>
__global__ __launch_bounds__(kWalkBlock) void k_ru_hist(RuSrc S, uint32_t shift, uint32_t nblk,
                                                        const gevws_summary* __restrict__ sum,
                                                        uint32_t* __restrict__ table) {
  if (sum->status != GEVWS_OK) return;
  __shared__ uint32_t s_hist[kRuDigits];
  const uint64_t n_members = sum->frames;
  s_hist[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRuRounds; ++r) {
    const uint64_t idx = (uint64_t)blockIdx.x * kRuKeys + (uint32_t)r * kWalkBlock + threadIdx.x;
    uint32_t key, val;
    if (ru_key<FIRST>(S, n_members, idx, key, val)) atomicAdd(&s_hist[(key >> shift) & 0xFF], 1u);
  }
  __syncthreads();
  table[(uint64_t)threadIdx.x * nblk + blockIdx.x] = s_hist[threadIdx.x];
}

// LAST: the connections alone into out_vals (d_room_members_out).
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kWalkBlock) void k_ru_scatter(RuSrc S, uint32_t shift, uint32_t nblk,
                                                           const gevws_summary* __restrict__ sum,
                                                           const uint32_t* __restrict__ table,
                                                           uint32_t* __restrict__ out_keys,
                                                           uint32_t* __restrict__ out_vals) {
  if (sum->status != GEVWS_OK) return;
  __shared__ uint32_t s_base[kRuDigits];         // where the digit's next key of this workgroup goes
  __shared__ uint32_t s_cnt[kRuWaves][kRuDigits];  // the round's keys of the digit, per wave
  const uint64_t n_members = sum->frames;
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  s_base[t] = table[(uint64_t)t * nblk + blockIdx.x];
#pragma unroll
  for (int j = 0; j < kRuWaves; ++j) s_cnt[j][t] = 0;
  __syncthreads();
  for (int r = 0; r < kRuRounds; ++r) {
    const uint64_t idx = (uint64_t)blockIdx.x * kRuKeys + (uint32_t)r * kWalkBlock + t;
    uint32_t key, val;
    const bool have = ru_key<FIRST>(S, n_members, idx, key, val);
    const uint32_t d = (key >> shift) & 0xFF;
    // the lanes of this wave that hold a key of the same digit
    uint64_t same = __ballot(have);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const uint64_t m = __ballot(bit);
      same &= bit ? m : ~m;
    }
    const uint64_t below = same & ((1ull << lane) - 1);
    if (have && below == 0) s_cnt[w][d] = (uint32_t)__popcll(same);
    __syncthreads();
    if (have) {
      uint32_t at = s_base[d] + (uint32_t)__popcll(below);
#pragma unroll
      for (int j = 0; j < kRuWaves; ++j) at += j < (int)w ? s_cnt[j][d] : 0u;
      if (at < S.n_conns) {  // (always: a place is below n_members)
        if constexpr (!LAST) out_keys[at] = key;
        out_vals[at] = val;
      }
    }
    __syncthreads();
    uint32_t all = 0;
#pragma unroll
    for (int j = 0; j < kRuWaves; ++j) {
      all += s_cnt[j][t];
      s_cnt[j][t] = 0;
    }
    s_base[t] += all;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kWalkBlock) void k_ru_copy(const uint32_t* __restrict__ room_new, uint32_t n_conns,
                                                        const gevws_summary* __restrict__ sum,
                                                        uint32_t* __restrict__ room_out) {
  if (sum->status != GEVWS_OK) return;
  const uint64_t c = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  if (c < n_conns) room_out[c] = room_new[c];
}

// ------------------------------------------------------------------ scratch
struct RuScratch {
  uint64_t* ctl;
  uint32_t* last;      // [c] the 1-based index of the last change that names c (0: none)
  uint32_t* cnt;       // [g] the room's members
  gevws_summary* sum;  // the table scans' summary: frames = the table's total, status GEVWS_OK (nobody reads it)
  uint64_t* blk_c;     // [nblkc][kBlkFields] k_ru_resolve's partials
  uint64_t* blk_t;     // [nblkt][kBlkFields] the table scans' partials
  uint32_t* room_new;  // [c]
  uint32_t* table;     // [digit][workgroup]
  uint32_t* keys[2];   // [c] the pairs between passes
  uint32_t* vals[2];
  size_t zero_bytes, total;
};
inline RuScratch ru_scratch(void* base, uint32_t n_conns, uint32_t n_rooms, uint32_t nblkc, uint32_t nblkt,
                            uint32_t nblks, bool pairs) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  RuScratch s{};
  size_t o = 0;
  s.ctl = reinterpret_cast<uint64_t*>(p + o), o += 256;
  s.last = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n_conns * 4 + 4);
  s.cnt = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n_rooms * 4 + 4);
  s.zero_bytes = o;
  s.sum = reinterpret_cast<gevws_summary*>(p + o), o += 256;
  s.blk_c = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)nblkc * kBlkFields * sizeof(uint64_t) + 8);
  s.blk_t = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)nblkt * kBlkFields * sizeof(uint64_t) + 8);
  s.room_new = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n_conns * 4 + 4);
  s.table = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)nblks * kRuDigits * 4 + 4);
  for (int i = 0; i < 2; ++i) {
    s.keys[i] = reinterpret_cast<uint32_t*>(p + o), o += pairs ? up((size_t)n_conns * 4 + 4) : 0;
    s.vals[i] = reinterpret_cast<uint32_t*>(p + o), o += pairs ? up((size_t)n_conns * 4 + 4) : 0;
  }
  s.total = o;
  return s;
}

inline uint32_t blocks_of(uint64_t n, uint64_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

using namespace gevws_impl;

extern "C" int gevws_rooms_update_async(gevws_ctx* ctx, void* stream, const uint32_t* d_conn_room_in,
                                        uint32_t n_conns, uint32_t n_rooms, const gevws_room_change* d_changes,
                                        uint64_t max_changes, const gevws_summary* d_prev,
                                        const gevws_conn_send* d_conn_send, const gevws_summary* d_plan_summary,
                                        uint32_t flags, uint32_t* d_conn_room_out, uint32_t* d_room_first_out,
                                        uint32_t* d_room_members_out, gevws_summary* d_summary) {
  if (!ctx || flags != 0 || !d_conn_room_out || !d_room_first_out || !d_room_members_out || !d_summary ||
      (n_conns && !d_conn_room_in) || d_conn_room_out == d_conn_room_in || max_changes > 0xFFFFFFFFull)
    return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  if (!d_changes) max_changes = 0;
  if (!max_changes) d_changes = nullptr;
  // the sort's passes: the bytes of the largest room id; one room still takes the pass that drops the roomless
  int passes = 0;
  if (n_rooms && n_conns) {
    passes = 1;
    for (uint32_t top = (n_rooms - 1) >> 8; top; top >>= 8) ++passes;
  }
  const uint32_t nblkc = n_conns ? blocks_of(n_conns, kRuKeys) : 1u;  // (one workgroup writes the zero partial)
  const uint32_t nblkcp = blocks_of(n_conns, kWalkBlock);
  const uint32_t nblkch = blocks_of(max_changes, kWalkBlock);
  const uint32_t nblks = blocks_of(n_conns, kRuKeys);
  const uint64_t n_first = (uint64_t)n_rooms + 1, n_table = (uint64_t)nblks * kRuDigits;
  const uint32_t nblkr = blocks_of(n_first, kRuScanTile), nblkh = blocks_of(n_table, kRuScanTile);
  const uint32_t nblkt = nblkr > nblkh ? nblkr : nblkh;
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, ru_scratch(nullptr, n_conns, n_rooms, nblkc, nblkt, nblks, passes > 1).total);
  if (r != GEVWS_OK) return r;
  const RuScratch s = ru_scratch(ctx->scratch, n_conns, n_rooms, nblkc, nblkt, nblks, passes > 1);
  const RuGates G{d_prev, d_plan_summary};
  // the block partials' scan: the 256-lane shape (the 1 024-lane one spills in this file)
  auto scan = [&](uint64_t* blk, uint32_t nblk, gevws_summary* sum) {
    k_scan_blocks<false, kBlkFields, kWalkBlock><<<1, kWalkBlock, 0, st>>>(blk, nblk, UINT64_MAX, UINT64_MAX, sum);
  };
  GEVWS_HIP(hipMemsetAsync(s.ctl, 0, s.zero_bytes, st));
  if (nblkch)
    k_ru_changes<<<nblkch, kWalkBlock, 0, st>>>(d_changes, max_changes, G, n_conns, n_rooms, s.last, s.ctl);
  if (n_rooms <= kRuLdsRooms)
    k_ru_resolve<true><<<nblkc, kWalkBlock, 0, st>>>(d_conn_room_in, d_changes, d_conn_send, G, n_conns, n_rooms,
                                                     s.last, s.room_new, s.cnt, s.blk_c);
  else
    k_ru_resolve<false><<<nblkc, kWalkBlock, 0, st>>>(d_conn_room_in, d_changes, d_conn_send, G, n_conns, n_rooms,
                                                      s.last, s.room_new, s.cnt, s.blk_c);
  scan(s.blk_c, nblkc, d_summary);
  k_ru_verdict<<<1, 1, 0, st>>>(G, max_changes, d_changes != nullptr, s.ctl, d_summary);
  // the room bases
  k_ru_sum<<<nblkr, kWalkBlock, 0, st>>>(s.cnt, n_rooms, nullptr, s.blk_t);
  scan(s.blk_t, nblkr, s.sum);
  k_ru_excl<<<nblkr, kWalkBlock, 0, st>>>(s.cnt, n_rooms, n_first, s.blk_t, d_summary, d_room_first_out);
  // the members
  for (int p = 0; p < passes; ++p) {
    const bool first = p == 0, lastp = p == passes - 1;
    const uint32_t shift = 8u * (uint32_t)p;
    const RuSrc S{first ? s.room_new : s.keys[(p - 1) & 1], first ? nullptr : s.vals[(p - 1) & 1], n_conns};
    uint32_t* ok = lastp ? nullptr : s.keys[p & 1];
    uint32_t* ov = lastp ? d_room_members_out : s.vals[p & 1];
    if (first) k_ru_hist<true><<<nblks, kWalkBlock, 0, st>>>(S, shift, nblks, d_summary, s.table);
    else k_ru_hist<false><<<nblks, kWalkBlock, 0, st>>>(S, shift, nblks, d_summary, s.table);
    k_ru_sum<<<nblkh, kWalkBlock, 0, st>>>(s.table, n_table, d_summary, s.blk_t);
    scan(s.blk_t, nblkh, s.sum);
    k_ru_excl<<<nblkh, kWalkBlock, 0, st>>>(s.table, n_table, n_table, s.blk_t, d_summary, s.table);
    auto scatter = first ? (lastp ? k_ru_scatter<true, true> : k_ru_scatter<true, false>)
                         : (lastp ? k_ru_scatter<false, true> : k_ru_scatter<false, false>);
    scatter<<<nblks, kWalkBlock, 0, st>>>(S, shift, nblks, d_summary, s.table, ok, ov);
  }
  if (n_conns) k_ru_copy<<<nblkcp, kWalkBlock, 0, st>>>(s.room_new, n_conns, d_summary, d_conn_room_out);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}
