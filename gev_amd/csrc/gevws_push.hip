// gevws_push.hip -- the push pass (gevws_push_lists_async,
// gevws_push_plan_async; include/gevws.h, "Server push"): messages the host
// originates, to every live connection, to a room's or to one.  A push enters
// the plain list and the deflate list once each, however many connections
// receive it, and the plan names the one encoded frame once per recipient.
// The reference packs on the host and sends session by session
// (example/websocket/main.go:129-150 loops over serv.sessions with
// Connection.Send, connection.go:122, over util.PackData, ws/util/util.go:10).
//
// The list is sorted by (kind, target) on the host, so a recipient's pushes
// are three contiguous slices of it -- the ALL pushes, its room's, its own --
// and their concatenation is the list order: no sort, no atomic placement and
// no merge here, and no lane walks a room.
//
// The list step, two memsets and five launches, no host round trip:
//   k_push_check   one lane per record: the room tables (rooms_check), per room
//                  and over all connections the live plain-takers, the live
//                  deflate-takers and their smallest window (integer atomics
//                  into zeroed scratch: order-independent; one per wave for
//                  the global ones), and the push records' own rule
//   k_pl_count / k_scan_blocks / k_pl_verdict / k_pl_emit
//                  the compaction into both lists at once (k_rr_emit's shape);
//                  the scan is the 256-lane instantiation, which keeps every
//                  register (one round of it covers 2 048 blocks)
//
// The plan, two memsets and nine launches:
//   k_push_check   as above, without windows
//   k_pp_lens      one lane per push: the length a plain-taker is sent and the
//                  length a deflate-taker is sent, every list index and table
//                  range checked; block partials
//   k_scan_blocks / k_pp_prefix
//                  their exclusive prefix sums over the list
//   k_pp_conns     one lane per connection: its three slices by bisection of
//                  the sorted keys, its count (their lengths) and its bytes
//                  (differences of the prefix sums); block partials
//   k_scan_blocks / k_pp_verdict / k_pp_conn_emit
//                  the summary, CAPACITY, d_conn_send
//   k_pp_emit      the hot loop, one lane per output entry: the recipient by
//                  bisection of the connections' first entries, the rank into
//                  one of its three slices, one 32-byte store
// Nothing but the summary is written before the verdict.  No payload byte is touched.
#include "gevws_internal.hpp"
#include "gevws_push.hpp"
#include "gevws_roomtabs.hpp"

namespace {

using namespace gevws_push_rule;

static_assert(sizeof(gevws_push) == 32 && offsetof(gevws_push, target) == 16 && offsetof(gevws_push, kind) == 20 &&
                  offsetof(gevws_push, opcode) == 21 && offsetof(gevws_push, reserved) == 22, "gevws_push layout");
static_assert(sizeof(gevws_send) == 32 && sizeof(gevws_conn_send) == 32 && sizeof(gevws_deflate_msg) == 24 &&
                  sizeof(gevws_out_frame) == 32, "record layouts");

// ctl[]: the call's counters
constexpr int kCtlBadTable = 0;  // malformed table records
constexpr int kCtlRoomed = 1;    // connections with a room
constexpr int kCtlBadPush = 2;   // malformed push records
constexpr int kCtlBadIdx = 3;    // (plan) pushes with a bad list index, table range or missing list
constexpr int kCtlAllPlain = 4;  // live connections that take plain
constexpr int kCtlAllDef = 5;    // live connections that take deflate

struct PushIn {
  const gevws_push* __restrict__ pushes;
  uint64_t src_bytes;
  const uint8_t* __restrict__ ext;    // may be null
  const uint8_t* __restrict__ wbits;  // may be null (the plan: always)
  const uint8_t* __restrict__ live;   // may be null
  int has_tabs;                       // 0: no room tables, every connection is in no room
};

__device__ __forceinline__ bool is_live(const uint8_t* __restrict__ live, uint32_t c) { return !live || live[c] != 0; }

// Connection c's effective window, 8..15; 0: its byte is outside {0, 8..15}.
__device__ __forceinline__ uint32_t window_of(const uint8_t* __restrict__ wbits, uint32_t c) {
  const uint32_t wb = wbits ? wbits[c] : 0u;
  if (wb == 0) return 15u;
  return wb < 8 || wb > 15 ? 0u : wb;
}

__device__ __forceinline__ uint32_t wave_min32(uint32_t x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t y = (uint32_t)__shfl_xor((int)x, d, 64);
    x = y < x ? y : x;
  }
  return x;
}

// The key of record i, from the 8 bytes that hold target, kind and opcode.
__device__ __forceinline__ uint64_t key_at(const gevws_push* __restrict__ pushes, uint64_t i) {
  const gevws_push& p = pushes[i];
  return ((uint64_t)p.kind << 32) | p.target;
}

__device__ __forceinline__ bool push_bad(const PushIn& P, const RoomTabs& T, const gevws_push& p, uint64_t i) {
  return malformed(p, i != 0, i ? key_at(P.pushes, i - 1) : 0u, T.n_conns, T.n_rooms, P.src_bytes);
}

// A member slot's part in its room's counts: kind 0 none, 1 a live plain-taker,
// 2 a live deflate-taker with the window wb.  The CSR is room-major, so the
// slots of a wave are often one room's: the wave then adds its sums with one
// atomic a counter (16 384 members of one room are 256 atomics an address
// instead of 16 384); a wave over several rooms adds lane by lane.  Integer
// adds and mins either way: the result is the same.  Every lane of the wave
// calls it.
__device__ __forceinline__ void room_takers(uint32_t* __restrict__ room_kind, uint32_t* __restrict__ room_wb,
                                            uint32_t kind, uint32_t room, uint32_t wb) {
  const uint64_t has = __ballot(kind != 0);
  if (!has) return;
  const int first = __ffsll((long long)has) - 1;
  const uint32_t g0 = (uint32_t)__shfl((int)room, first, 64);
  if (__all(kind == 0 || room == g0)) {
    const uint64_t np = wave_sum(kind == 1 ? 1u : 0u), nd = wave_sum(kind == 2 ? 1u : 0u);
    const uint32_t wm = wave_min32(kind == 2 ? wb : 0xFFFFFFFFu);
    if ((int)(threadIdx.x & 63) == first) {
      if (np) atomicAdd(room_kind + 2 * (uint64_t)g0, (uint32_t)np);
      if (nd) atomicAdd(room_kind + 2 * (uint64_t)g0 + 1, (uint32_t)nd), atomicMin(room_wb + g0, wm);
    }
  } else if (kind == 1) {
    atomicAdd(room_kind + 2 * (uint64_t)room, 1u);
  } else if (kind == 2) {
    atomicAdd(room_kind + 2 * (uint64_t)room + 1, 1u);
    atomicMin(room_wb + room, wb);
  }
}

// ------------------------------------------------------------------ the check, both calls
// Lane i checks room record i, member slot i, connection i (rooms_check, and
// the connection's window byte) and push record i.
__global__ __launch_bounds__(kWalkBlock) void k_push_check(PushIn P, RoomTabs T, Gates G,
                                                           uint32_t* __restrict__ room_kind,
                                                           uint32_t* __restrict__ room_wb,
                                                           uint32_t* __restrict__ all_wb, uint64_t* __restrict__ ctl) {
  const uint64_t i = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  const uint64_t n = gate_count(G);
  uint64_t bad_t = 0, roomed = 0, bad_p = 0, ap = 0, ad = 0;
  uint32_t wmin = 0xFFFFFFFFu, mkind = 0, mroom = kNoRoom, mwb = 0;
  if (n) {  // (a call without records reads none of its tables)
    RoomRec r{0u, 0u, kNoRoom, kNoSlot, false};
    if (P.has_tabs) r = rooms_check(T, i);
    bad_t = r.bad, roomed = r.roomed;
    if (r.member != kNoSlot && is_live(P.live, r.member)) {  // member slot i: one of its room's live takers
      mroom = r.room;
      if (takes_deflate(P.ext, r.member)) {
        mwb = window_of(P.wbits, r.member);
        mkind = mwb ? 2u : 0u;  // (a bad byte is its connection's record, below)
      } else {
        mkind = 1u;
      }
    }
    if (i < T.n_conns && is_live(P.live, (uint32_t)i)) {
      if (takes_deflate(P.ext, (uint32_t)i)) {
        const uint32_t wb = window_of(P.wbits, (uint32_t)i);
        if (wb) {
          ad = 1, wmin = wb;
        } else {  // (the connection's record counts once, whatever is wrong with it)
          const uint32_t g = P.has_tabs ? T.conn_room[i] : kNoRoom;
          bad_t += !(g != kNoRoom && g >= T.n_rooms);
        }
      } else {
        ap = 1;
      }
    }
    if (i < n) bad_p = push_bad(P, T, P.pushes[i], i);
  }
  room_takers(room_kind, room_wb, mkind, mroom, mwb);
  count_up(ctl + kCtlBadTable, bad_t);
  count_up(ctl + kCtlRoomed, roomed);
  count_up(ctl + kCtlBadPush, bad_p);
  count_up(ctl + kCtlAllPlain, ap);
  count_up(ctl + kCtlAllDef, ad);
  wmin = wave_min32(wmin);
  if ((threadIdx.x & 63) == 0 && wmin != 0xFFFFFFFFu) atomicMin(all_wb, wmin);
}

// The recipients of a well-formed push by kind, and the deflate-takers' smallest window.
struct Takers {
  uint64_t np, nd;
  uint32_t wb;
};
__device__ __forceinline__ Takers takers_of(const PushIn& P, const gevws_push& p,
                                            const uint32_t* __restrict__ room_kind,
                                            const uint32_t* __restrict__ room_wb,
                                            const uint32_t* __restrict__ all_wb, const uint64_t* __restrict__ ctl) {
  Takers t{0, 0, 15u};
  if (p.kind == GEVWS_PUSH_ALL) {
    t.np = ctl[kCtlAllPlain], t.nd = ctl[kCtlAllDef], t.wb = *all_wb;
  } else if (p.kind == GEVWS_PUSH_ROOM) {
    t.np = room_kind[2 * (uint64_t)p.target], t.nd = room_kind[2 * (uint64_t)p.target + 1], t.wb = room_wb[p.target];
  } else if (is_live(P.live, p.target)) {
    const bool d = takes_deflate(P.ext, p.target);
    t.np = !d, t.nd = d, t.wb = window_of(P.wbits, p.target);
  }
  return t;
}

// ------------------------------------------------------------------ the list step
struct PushDec {
  bool plain, deflate;
  uint32_t wb;
};
__device__ __forceinline__ PushDec pl_decide(const PushIn& P, const RoomTabs& T, const gevws_push& p, uint64_t i,
                                             const uint32_t* __restrict__ room_kind,
                                             const uint32_t* __restrict__ room_wb,
                                             const uint32_t* __restrict__ all_wb,
                                             const uint64_t* __restrict__ ctl) {
  PushDec r{false, false, 15u};
  if (push_bad(P, T, p, i)) return r;  // (its target indexes nothing)
  const Takers t = takers_of(P, p, room_kind, room_wb, all_wb, ctl);
  lists(p.opcode, t.np, t.nd, r.plain, r.deflate);
  r.wb = t.wb >= 8 && t.wb <= 15 ? t.wb : 15u;
  return r;
}

__global__ __launch_bounds__(kWalkBlock) void k_pl_count(PushIn P, RoomTabs T, Gates G,
                                                         const uint32_t* __restrict__ room_kind,
                                                         const uint32_t* __restrict__ room_wb,
                                                         const uint32_t* __restrict__ all_wb,
                                                         const uint64_t* __restrict__ ctl,
                                                         uint64_t* __restrict__ blk) {
  const uint64_t n = gate_count(G);
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[2] = {0, 0};  // deflate-list entries, plain-list entries
  if (m < n) {
    const PushDec r = pl_decide(P, T, P.pushes[m], m, room_kind, room_wb, all_wb, ctl);
    vals[0] = r.deflate, vals[1] = r.plain;
  }
  block_partial<2>(vals, blk, blockIdx.x);
}

// The scan left {deflate entries, plain entries} in *def_sum's frames /
// payload_bytes: the two summaries from them and from the check's counters.
__global__ void k_pl_verdict(Gates G, uint32_t n_members, const uint64_t* __restrict__ ctl,
                             gevws_summary* __restrict__ def_sum, gevws_summary* __restrict__ plain_sum) {
  const gevws_summary s = *def_sum;
  gevws_summary a, b;
  memset(&a, 0, sizeof(a));
  memset(&b, 0, sizeof(b));
  if (gate_count(G)) {
    const uint64_t bad = ctl[kCtlBadPush] + ctl[kCtlBadTable] + (ctl[kCtlRoomed] != n_members ? 1u : 0u);
    if (bad) {
      a.errors = b.errors = bad;
      a.status = b.status = GEVWS_ERR_INVALID;
    } else {
      a.frames = s.frames;
      b.frames = s.payload_bytes;
    }
  }
  *def_sum = a;
  *plain_sum = b;
}

__global__ __launch_bounds__(kWalkBlock) void k_pl_emit(PushIn P, RoomTabs T, Gates G,
                                                        const uint32_t* __restrict__ room_kind,
                                                        const uint32_t* __restrict__ room_wb,
                                                        const uint32_t* __restrict__ all_wb,
                                                        const uint64_t* __restrict__ ctl,
                                                        const uint64_t* __restrict__ blk,
                                                        const gevws_summary* __restrict__ def_sum,
                                                        gevws_deflate_msg* __restrict__ def_msgs,
                                                        gevws_out_frame* __restrict__ plain,
                                                        int64_t* __restrict__ plain_of, int64_t* __restrict__ def_of) {
  if (def_sum->status != GEVWS_OK) return;  // a malformed record: nothing written
  const uint64_t n = gate_count(G);
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  gevws_push p;
  memset(&p, 0, sizeof(p));
  PushDec r{false, false, 15u};
  if (m < n) {
    p = P.pushes[m];
    r = pl_decide(P, T, p, m, room_kind, room_wb, all_wb, ctl);
  }
  const uint64_t v[2] = {(uint64_t)r.deflate, (uint64_t)r.plain};
  uint64_t ex[2], tot[2];
  block_excl_scan<kWalkBlock, 2>(v, ex, tot);
  if (m >= n) return;
  int64_t pi = -1, di = -1;
  if (r.deflate) {
    const uint64_t k = blk[(uint64_t)blockIdx.x * kBlkFields + 0] + ex[0];
    gevws_deflate_msg d;
    memset(&d, 0, sizeof(d));
    d.payload_off = p.off;
    d.length = p.length;
    d.opcode = p.opcode;
    d.window_bits = (uint8_t)r.wb;
    def_msgs[k] = d;
    di = (int64_t)k;
  }
  if (r.plain) {
    const uint64_t k = blk[(uint64_t)blockIdx.x * kBlkFields + 1] + ex[1];
    gevws_out_frame o;
    memset(&o, 0, sizeof(o));
    o.hdr.fin = 1;
    o.hdr.opcode = p.opcode;
    o.hdr.length = (int64_t)p.length;
    o.payload_off = p.off;
    o.payload_len = p.length;
    plain[k] = o;
    pi = (int64_t)k;
  }
  plain_of[m] = pi;
  def_of[m] = di;
}

// What both calls keep in the context's scratch in front of their own arrays.
struct PushScratch {
  uint64_t* ctl;
  uint64_t* blk;        // [nblk][kBlkFields] the pushes' block partials
  uint64_t* blk_c;      // [nblkc][kBlkFields] (plan) the connections'
  gevws_summary* sum_p; // (plan) the push scan's summary (not used)
  uint32_t* room_kind;  // [g][2]: live plain-takers, live deflate-takers
  uint32_t* all_wb;     // the live deflate-takers' smallest window (all ones: none)
  uint32_t* room_wb;    // [g] the same per room
  // the plan's
  uint64_t* lenp;       // [p] the bytes a plain-taker is sent of push p
  uint64_t* lend;       // [p] the bytes a deflate-taker is sent
  uint64_t* prefp;      // [p] their exclusive prefix sums; [n] the totals
  uint64_t* prefd;
  uint32_t* cslice;     // [c][8]: the ALL slice's end, the room slice, the own slice, takes deflate
  uint64_t* cbytes;     // [c]
  uint64_t* cfirst;     // [c] the connection's first entry; [n_conns] all of them
  size_t zero_bytes, ones_off, ones_bytes, total;
};
inline PushScratch push_scratch(void* base, bool plan, uint64_t max_pushes, uint32_t nblk, uint32_t nblkc,
                                uint32_t n_rooms, uint32_t n_conns) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  PushScratch s{};
  size_t o = 0;
  s.ctl = reinterpret_cast<uint64_t*>(p + o), o += 256;
  s.blk = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)nblk * kBlkFields * sizeof(uint64_t) + 8);
  s.blk_c = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)nblkc * kBlkFields * sizeof(uint64_t) + 8);
  s.sum_p = reinterpret_cast<gevws_summary*>(p + o), o += 256;
  s.room_kind = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n_rooms * 8 + 8);
  s.zero_bytes = o;
  s.ones_off = o;
  s.all_wb = reinterpret_cast<uint32_t*>(p + o), o += 256;
  s.room_wb = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n_rooms * 4 + 4);
  s.ones_bytes = o - s.ones_off;
  if (plan) {
    s.lenp = reinterpret_cast<uint64_t*>(p + o), o += up(max_pushes * 8);
    s.lend = reinterpret_cast<uint64_t*>(p + o), o += up(max_pushes * 8);
    s.prefp = reinterpret_cast<uint64_t*>(p + o), o += up((max_pushes + 1) * 8);
    s.prefd = reinterpret_cast<uint64_t*>(p + o), o += up((max_pushes + 1) * 8);
    s.cslice = reinterpret_cast<uint32_t*>(p + o), o += up((size_t)n_conns * 32);
    s.cbytes = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)n_conns * 8);
    s.cfirst = reinterpret_cast<uint64_t*>(p + o), o += up(((size_t)n_conns + 1) * 8);
  }
  s.total = o;
  return s;
}

// ------------------------------------------------------------------ the plan
struct PlanIn {
  const gevws_summary* __restrict__ enc0;  // the plain wire's encode summary, its table below
  const gevws_summary* __restrict__ enc1;  // the deflated wire's
  const uint64_t* __restrict__ off0;
  const uint64_t* __restrict__ off1;
  const int64_t* __restrict__ plain_of;
  const int64_t* __restrict__ def_of;
};

// Entry idx of wire w's list as a byte range of that wire; false: an index
// outside the list, or a table that decreases.
__device__ __forceinline__ bool pp_range(const PlanIn& q, uint32_t w, uint64_t idx, uint64_t& off, uint64_t& len) {
  const gevws_summary* __restrict__ enc = w == 0 ? q.enc0 : q.enc1;
  const uint64_t* __restrict__ tab = w == 0 ? q.off0 : q.off1;
  const uint64_t cnt = enc->frames, total = enc->payload_bytes;
  if (idx >= cnt) return false;
  off = tab[idx];
  const uint64_t next = idx + 1 < cnt ? tab[idx + 1] : total;
  if (next < off) return false;
  len = next - off;
  return true;
}

__global__ __launch_bounds__(kWalkBlock) void k_pp_lens(PushIn P, PlanIn q, RoomTabs T, Gates G,
                                                        const uint32_t* __restrict__ room_kind,
                                                        const uint32_t* __restrict__ room_wb,
                                                        const uint32_t* __restrict__ all_wb,
                                                        uint64_t* __restrict__ ctl, uint64_t* __restrict__ lenp,
                                                        uint64_t* __restrict__ lend, uint64_t* __restrict__ blk) {
  const uint64_t n = gate_count(G);
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[2] = {0, 0};  // the bytes a plain-taker is sent, a deflate-taker
  uint64_t bad = 0;
  if (m < n) {
    const gevws_push p = P.pushes[m];
    if (!push_bad(P, T, p, m)) {  // (a malformed record is the check's, and its target indexes nothing)
      const Takers t = takers_of(P, p, room_kind, room_wb, all_wb, ctl);
      const int64_t ip = q.plain_of[m], id = q.def_of[m];
      uint64_t off, l0 = 0, l1 = 0;
      const bool in0 = ip >= 0, in1 = id >= 0;
      if (in0 && !pp_range(q, 0, (uint64_t)ip, off, l0)) bad = 1;
      if (in1 && !pp_range(q, 1, (uint64_t)id, off, l1)) bad = 1;
      if (t.np && !in0) bad = 1;          // a plain-taker needs it from the plain list
      if (t.nd && !in1 && !in0) bad = 1;  // a deflate-taker from either
      if (!bad) vals[0] = t.np ? l0 : 0u, vals[1] = t.nd ? (in1 ? l1 : l0) : 0u;
    }
    lenp[m] = vals[0], lend[m] = vals[1];
  }
  count_up(ctl + kCtlBadIdx, bad);
  block_partial<2>(vals, blk, blockIdx.x);
}

__global__ __launch_bounds__(kWalkBlock) void k_pp_prefix(Gates G, const uint64_t* __restrict__ lenp,
                                                          const uint64_t* __restrict__ lend,
                                                          const uint64_t* __restrict__ blk,
                                                          uint64_t* __restrict__ prefp,
                                                          uint64_t* __restrict__ prefd) {
  const uint64_t n = gate_count(G);
  const uint64_t m = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t v[2] = {0, 0};
  if (m < n) v[0] = lenp[m], v[1] = lend[m];
  uint64_t ex[2], tot[2];
  block_excl_scan<kWalkBlock, 2>(v, ex, tot);
  if (m >= n) return;
  const uint64_t b0 = blk[(uint64_t)blockIdx.x * kBlkFields + 0] + ex[0];
  const uint64_t b1 = blk[(uint64_t)blockIdx.x * kBlkFields + 1] + ex[1];
  prefp[m] = b0, prefd[m] = b1;
  if (m == n - 1) prefp[n] = b0 + v[0], prefd[n] = b1 + v[1];
}

// The first record of [0, n) whose key is at least k (n: none), by bisection:
// at most 33 rounds, every probe inside the checked count, whatever the list
// holds.
__device__ __forceinline__ uint32_t key_lower_bound(const gevws_push* __restrict__ pushes, uint64_t n, uint64_t k) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (key_at(pushes, mid) < k) lo = mid + 1;
    else hi = mid;
  }
  return (uint32_t)lo;  // (n <= 2^32 - 1)
}

struct ConnSlices {  // 32 bytes in scratch
  uint32_t all_end, room_lo, room_hi, own_lo, own_hi, deflate, pad[2];
};
static_assert(sizeof(ConnSlices) == 32, "cslice rows");

__global__ __launch_bounds__(kWalkBlock) void k_pp_conns(PushIn P, RoomTabs T, Gates G,
                                                         const uint64_t* __restrict__ prefp,
                                                         const uint64_t* __restrict__ prefd,
                                                         ConnSlices* __restrict__ cslice,
                                                         uint64_t* __restrict__ cbytes, uint64_t* __restrict__ blk) {
  const uint64_t n = gate_count(G);
  const uint32_t c = blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[3] = {0, 0, 0};  // entries, -, bytes
  if (n && c < T.n_conns) {
    ConnSlices s;
    memset(&s, 0, sizeof(s));
    if (is_live(P.live, c)) {
      s.deflate = takes_deflate(P.ext, c) ? 1u : 0u;
      s.all_end = key_lower_bound(P.pushes, n, (uint64_t)GEVWS_PUSH_ROOM << 32);
      const uint32_t g = P.has_tabs ? T.conn_room[c] : kNoRoom;
      if (g < T.n_rooms) {
        const uint64_t k = ((uint64_t)GEVWS_PUSH_ROOM << 32) | g;
        s.room_lo = key_lower_bound(P.pushes, n, k);
        s.room_hi = key_lower_bound(P.pushes, n, k + 1);
      }
      const uint64_t k = ((uint64_t)GEVWS_PUSH_CONN << 32) | c;
      s.own_lo = key_lower_bound(P.pushes, n, k);
      s.own_hi = key_lower_bound(P.pushes, n, k + 1);
      if (s.room_hi < s.room_lo) s.room_hi = s.room_lo;  // (a list out of order: the verdict is INVALID)
      if (s.own_hi < s.own_lo) s.own_hi = s.own_lo;
      const uint64_t* __restrict__ pre = s.deflate ? prefd : prefp;
      vals[0] = (uint64_t)s.all_end + (s.room_hi - s.room_lo) + (s.own_hi - s.own_lo);
      vals[2] = (pre[s.all_end] - pre[0]) + (pre[s.room_hi] - pre[s.room_lo]) + (pre[s.own_hi] - pre[s.own_lo]);
    }
    cslice[c] = s;
    cbytes[c] = vals[2];
  }
  block_partial<3>(vals, blk, blockIdx.x);
}

// The scan left {entries, -, bytes} in *sum's frames / payload_bytes /
// payload_len, and CAPACITY against max_sends: the summary from them and from
// the counters.
__global__ void k_pp_verdict(Gates G, uint32_t n_members, uint32_t n_conns, const uint64_t* __restrict__ ctl,
                             gevws_summary* __restrict__ sum) {
  const gevws_summary s = *sum;
  gevws_summary o;
  memset(&o, 0, sizeof(o));
  if (gate_count(G) && n_conns) {
    const uint64_t bad =
        ctl[kCtlBadPush] + ctl[kCtlBadTable] + (ctl[kCtlRoomed] != n_members ? 1u : 0u) + ctl[kCtlBadIdx];
    if (bad) {
      o.errors = bad;
      o.status = GEVWS_ERR_INVALID;
    } else {
      o.frames = s.frames;
      o.payload_bytes = s.payload_len;
      o.status = s.status;
    }
  }
  *sum = o;
}

__global__ __launch_bounds__(kWalkBlock) void k_pp_conn_emit(Gates G, uint32_t n_conns,
                                                             const ConnSlices* __restrict__ cslice,
                                                             const uint64_t* __restrict__ cbytes,
                                                             const uint64_t* __restrict__ blk,
                                                             const gevws_summary* __restrict__ sum,
                                                             uint64_t* __restrict__ cfirst,
                                                             gevws_conn_send* __restrict__ conn_send) {
  if (sum->status != GEVWS_OK) return;  // more entries than max_sends, or a malformed record: nothing written
  const bool live = gate_count(G) != 0;
  const uint32_t c = blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t v[1] = {0};
  if (live && c < n_conns) {
    const ConnSlices s = cslice[c];
    v[0] = (uint64_t)s.all_end + (s.room_hi - s.room_lo) + (s.own_hi - s.own_lo);
  }
  uint64_t ex[1], tot[1];
  block_excl_scan<kWalkBlock, 1>(v, ex, tot);
  if (!live || c >= n_conns) return;
  const uint64_t first = blk[(uint64_t)blockIdx.x * kBlkFields + 0] + ex[0];
  cfirst[c] = first;
  if (c == n_conns - 1) cfirst[n_conns] = first + v[0];
  gevws_conn_send o;
  memset(&o, 0, sizeof(o));
  o.first = first;
  o.count = v[0];
  o.bytes = cbytes[c];
  conn_send[c] = o;
}

// The hot loop, one lane per output entry: 32 bytes written.
__global__ __launch_bounds__(kWalkBlock) void k_pp_emit(PlanIn q, Gates G, uint32_t n_conns, uint64_t max_sends,
                                                        const ConnSlices* __restrict__ cslice,
                                                        const uint64_t* __restrict__ cfirst,
                                                        const gevws_summary* __restrict__ sum,
                                                        gevws_send* __restrict__ send) {
  if (sum->status != GEVWS_OK) return;
  const uint64_t n = gate_count(G);
  if (!n) return;
  const uint64_t total = sum->frames < max_sends ? sum->frames : max_sends;
  const uint64_t e = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  if (e >= total) return;
  // the recipient: the last connection whose first entry is at or before e (those before it there are empty)
  uint32_t lo = 0, hi = n_conns - 1;
  while (lo < hi) {  // (at most 32 rounds)
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (cfirst[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  const uint32_t c = lo;
  const ConnSlices s = cslice[c];
  uint64_t rank = e - cfirst[c], p;
  const uint64_t nroom = s.room_hi - s.room_lo;
  if (rank < s.all_end) p = rank;
  else if (rank - s.all_end < nroom) p = s.room_lo + (rank - s.all_end);
  else p = s.own_lo + (rank - s.all_end - nroom);
  if (p >= n) return;  // (never on a verdict of OK)
  const int64_t id = q.def_of[p];
  const uint32_t wire = s.deflate && id >= 0 ? 1u : 0u;
  const int64_t idx = wire ? id : q.plain_of[p];
  uint64_t off, len;
  if (idx < 0 || !pp_range(q, wire, (uint64_t)idx, off, len)) return;  // (checked by k_pp_lens)
  gevws_send o;
  o.off = off, o.len = len, o.frame = p, o.conn = c, o.wire = wire;
  send[e] = o;
}

// What both entry points ask of their room tables; the grid of the check.
inline bool tabs_ok(const uint32_t* conn_room, const uint32_t* first, const uint32_t* members, uint32_t n_conns,
                    uint32_t n_rooms, uint32_t n_members, int& has_tabs) {
  has_tabs = conn_room || first || members;
  if (!has_tabs) return n_rooms == 0 && n_members == 0;
  return first && (!n_conns || conn_room) && (!n_members || members);
}
inline uint32_t check_blocks(uint64_t max_pushes, uint32_t n_conns, uint32_t n_rooms, uint32_t n_members) {
  uint64_t recs = (uint64_t)n_rooms + 1;
  if (n_members > recs) recs = n_members;
  if (n_conns > recs) recs = n_conns;
  if (max_pushes > recs) recs = max_pushes;
  return (uint32_t)((recs + kWalkBlock - 1) / kWalkBlock);
}

}  // namespace

using namespace gevws_impl;

extern "C" int gevws_push_lists_async(gevws_ctx* ctx, void* stream, const gevws_push* d_pushes, uint64_t max_pushes,
                                      const gevws_summary* d_prev, uint64_t src_bytes, const uint8_t* d_conn_ext,
                                      const uint8_t* d_conn_window_bits, const uint8_t* d_conn_live,
                                      uint32_t n_conns, const uint32_t* d_conn_room, const uint32_t* d_room_first,
                                      const uint32_t* d_room_members, uint32_t n_rooms, uint32_t n_members,
                                      uint32_t flags, gevws_deflate_msg* d_def_msgs, gevws_summary* d_def_summary,
                                      gevws_out_frame* d_plain, gevws_summary* d_plain_summary, int64_t* d_plain_of,
                                      int64_t* d_def_of) {
  if (flags || max_pushes > kMaxPushes) return GEVWS_ERR_INVALID;
  if (!ctx || !d_def_summary || !d_plain_summary) return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  if (max_pushes == 0) {
    GEVWS_HIP(hipMemsetAsync(d_def_summary, 0, sizeof(gevws_summary), st));
    GEVWS_HIP(hipMemsetAsync(d_plain_summary, 0, sizeof(gevws_summary), st));
    return GEVWS_OK;
  }
  int has_tabs = 0;
  if (!d_pushes || !d_def_msgs || !d_plain || !d_plain_of || !d_def_of ||
      !tabs_ok(d_conn_room, d_room_first, d_room_members, n_conns, n_rooms, n_members, has_tabs))
    return GEVWS_ERR_INVALID;
  const uint32_t nblk = (uint32_t)((max_pushes + kWalkBlock - 1) / kWalkBlock);
  const uint32_t nblkt = check_blocks(max_pushes, n_conns, n_rooms, n_members);
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, push_scratch(nullptr, false, max_pushes, nblk, 0, n_rooms, n_conns).total);
  if (r != GEVWS_OK) return r;
  const PushScratch s = push_scratch(ctx->scratch, false, max_pushes, nblk, 0, n_rooms, n_conns);
  const RoomTabs T{d_conn_room, d_room_first, d_room_members, n_rooms, n_members, n_conns};
  const Gates G{{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, d_prev, max_pushes};
  const PushIn P{d_pushes, src_bytes, d_conn_ext, d_conn_window_bits, d_conn_live, has_tabs};
  GEVWS_HIP(hipMemsetAsync(s.ctl, 0, s.zero_bytes, st));
  GEVWS_HIP(hipMemsetAsync(reinterpret_cast<uint8_t*>(ctx->scratch) + s.ones_off, 0xFF, s.ones_bytes, st));
  k_push_check<<<nblkt, kWalkBlock, 0, st>>>(P, T, G, s.room_kind, s.room_wb, s.all_wb, s.ctl);
  k_pl_count<<<nblk, kWalkBlock, 0, st>>>(P, T, G, s.room_kind, s.room_wb, s.all_wb, s.ctl, s.blk);
  k_scan_blocks<false, kBlkFields, kWalkBlock><<<1, kWalkBlock, 0, st>>>(s.blk, nblk, UINT64_MAX, UINT64_MAX, d_def_summary);
  k_pl_verdict<<<1, 1, 0, st>>>(G, n_members, s.ctl, d_def_summary, d_plain_summary);
  k_pl_emit<<<nblk, kWalkBlock, 0, st>>>(P, T, G, s.room_kind, s.room_wb, s.all_wb, s.ctl, s.blk, d_def_summary,
                                         d_def_msgs, d_plain, d_plain_of, d_def_of);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}

extern "C" int gevws_push_plan_async(gevws_ctx* ctx, void* stream, const gevws_push* d_pushes, uint64_t max_pushes,
                                     const gevws_summary* d_prev, uint64_t src_bytes,
                                     const gevws_summary* d_plain_summary, const gevws_summary* d_def_summary,
                                     const int64_t* d_plain_of, const int64_t* d_def_of, const uint64_t* d_plain_off,
                                     const gevws_summary* d_plain_encoded, const uint64_t* d_def_off,
                                     const gevws_summary* d_def_encoded, const uint8_t* d_conn_ext,
                                     const uint8_t* d_conn_live, uint32_t n_conns, const uint32_t* d_conn_room,
                                     const uint32_t* d_room_first, const uint32_t* d_room_members, uint32_t n_rooms,
                                     uint32_t n_members, uint32_t flags, gevws_send* d_send, uint64_t max_sends,
                                     gevws_conn_send* d_conn_send, gevws_summary* d_summary) {
  if (flags || max_pushes > kMaxPushes || max_sends > 0xFFFFFFFFull) return GEVWS_ERR_INVALID;
  if (!ctx || !d_summary) return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  if (n_conns == 0 || max_pushes == 0) {
    GEVWS_HIP(hipMemsetAsync(d_summary, 0, sizeof(gevws_summary), st));
    return GEVWS_OK;
  }
  int has_tabs = 0;
  if (!d_pushes || !d_plain_summary || !d_def_summary || !d_plain_of || !d_def_of || !d_plain_off ||
      !d_plain_encoded || !d_def_off || !d_def_encoded || !d_conn_send || (max_sends && !d_send) ||
      !tabs_ok(d_conn_room, d_room_first, d_room_members, n_conns, n_rooms, n_members, has_tabs))
    return GEVWS_ERR_INVALID;
  const uint32_t nblk = (uint32_t)((max_pushes + kWalkBlock - 1) / kWalkBlock);
  const uint32_t nblkt = check_blocks(max_pushes, n_conns, n_rooms, n_members);
  const uint32_t nblkc = (uint32_t)(((uint64_t)n_conns + kWalkBlock - 1) / kWalkBlock);
  const uint32_t nblke = (uint32_t)((max_sends + kWalkBlock - 1) / kWalkBlock);
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, push_scratch(nullptr, true, max_pushes, nblk, nblkc, n_rooms, n_conns).total);
  if (r != GEVWS_OK) return r;
  const PushScratch s = push_scratch(ctx->scratch, true, max_pushes, nblk, nblkc, n_rooms, n_conns);
  const RoomTabs T{d_conn_room, d_room_first, d_room_members, n_rooms, n_members, n_conns};
  const Gates G{{d_plain_summary, d_def_summary, d_plain_encoded, d_def_encoded, nullptr, nullptr}, d_prev, max_pushes};
  const PushIn P{d_pushes, src_bytes, d_conn_ext, nullptr, d_conn_live, has_tabs};
  const PlanIn q{d_plain_encoded, d_def_encoded, d_plain_off, d_def_off, d_plain_of, d_def_of};
  ConnSlices* cslice = reinterpret_cast<ConnSlices*>(s.cslice);
  GEVWS_HIP(hipMemsetAsync(s.ctl, 0, s.zero_bytes, st));
  GEVWS_HIP(hipMemsetAsync(reinterpret_cast<uint8_t*>(ctx->scratch) + s.ones_off, 0xFF, s.ones_bytes, st));
  k_push_check<<<nblkt, kWalkBlock, 0, st>>>(P, T, G, s.room_kind, s.room_wb, s.all_wb, s.ctl);
  k_pp_lens<<<nblk, kWalkBlock, 0, st>>>(P, q, T, G, s.room_kind, s.room_wb, s.all_wb, s.ctl, s.lenp, s.lend, s.blk);
  k_scan_blocks<false, kBlkFields, kWalkBlock><<<1, kWalkBlock, 0, st>>>(s.blk, nblk, UINT64_MAX, UINT64_MAX, s.sum_p);
  k_pp_prefix<<<nblk, kWalkBlock, 0, st>>>(G, s.lenp, s.lend, s.blk, s.prefp, s.prefd);
  k_pp_conns<<<nblkc, kWalkBlock, 0, st>>>(P, T, G, s.prefp, s.prefd, cslice, s.cbytes, s.blk_c);
  k_scan_blocks<false, kBlkFields, kWalkBlock><<<1, kWalkBlock, 0, st>>>(s.blk_c, nblkc, max_sends, UINT64_MAX, d_summary);
  k_pp_verdict<<<1, 1, 0, st>>>(G, n_members, n_conns, s.ctl, d_summary);
  k_pp_conn_emit<<<nblkc, kWalkBlock, 0, st>>>(G, n_conns, cslice, s.cbytes, s.blk_c, d_summary, s.cfirst,
                                               d_conn_send);
  if (nblke) k_pp_emit<<<nblke, kWalkBlock, 0, st>>>(q, G, n_conns, max_sends, cslice, s.cfirst, d_summary, d_send);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}
