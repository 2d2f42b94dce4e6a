// gevws_gather.hip -- the step behind the send plan (gevws_send_gather_async,
// include/gevws.h): every connection's reply bytes, which the plan names as
// slices of three wire buffers, next to each other in one send buffer, one
// 16-aligned span a connection.  The reference writes each reply to its socket
// as it is made (plugins/websocket/wrap.go:38-90) and has no such step.
//
// Seven launches behind one memset, no host round trip:
//   k_gather_size     one lane per entry: its checks, its length into its
//                     connection's sum, block partials of the padded lengths
//                     (an entry's len, plus the span's pad on a connection's last)
//   k_gather_conns    one lane per connection: its range against the entry
//                     count and the connection before, its bytes against the sum
//   k_scan_blocks     block bases, the summary, CAPACITY
//   k_gather_verdict  one lane: the gates, INVALID
//   k_gather_place    one lane per entry: edst (where the entry's bytes go; never
//                     decreases, one for every record and the total behind them),
//                     the output-tile -> entry map
//   k_gather_spans    one lane per connection: d_conn_buf from edst
//   k_send_gather     the copy: the segmented copy k_join_copy runs too
//                     (gevws_segcopy.hpp), an entry a segment; every workgroup a
//                     contiguous run of 4 KiB output tiles, its four waves four
//                     tiles a step
// Nothing but the summary is written before the verdict.  Only k_send_gather
// touches reply bytes: len read, len rounded up to 16 a span written.
#include "gevws_internal.hpp"
#include "gevws_segcopy.hpp"

namespace {

static_assert(sizeof(gevws_send) == 32 && offsetof(gevws_send, len) == 8 && offsetof(gevws_send, conn) == 24 &&
                  offsetof(gevws_send, wire) == 28, "gevws_send layout");
static_assert(sizeof(gevws_conn_send) == 32 && offsetof(gevws_conn_send, count) == 8 &&
                  offsetof(gevws_conn_send, bytes) == 16 && offsetof(gevws_conn_send, flags) == 24,
              "gevws_conn_send layout");
static_assert(sizeof(gevws_conn_buf) == 32 && offsetof(gevws_conn_buf, bytes) == 8 &&
                  offsetof(gevws_conn_buf, flags) == 16 && offsetof(gevws_conn_buf, reserved) == 20,
              "gevws_conn_buf layout");

// The three wires: base and readable bytes.
struct GatherWires {
  const uint8_t* __restrict__ b0;
  const uint8_t* __restrict__ b1;
  const uint8_t* __restrict__ b2;
  uint64_t n0, n1, n2;
};
// One of three values by masks: a select between the fields' addresses would
// make the struct a table in scratch memory (0 for a wire above 2).
__device__ __forceinline__ uint64_t pick3(uint32_t wire, uint64_t a, uint64_t b, uint64_t c) {
  return (a & (0 - (uint64_t)(wire == 0))) | (b & (0 - (uint64_t)(wire == 1))) | (c & (0 - (uint64_t)(wire == 2)));
}
__device__ __forceinline__ uint64_t wire_bytes_of(const GatherWires& w, uint32_t wire) {
  return pick3(wire, w.n0, w.n1, w.n2);
}
__device__ __forceinline__ const uint8_t* wire_base_of(const GatherWires& w, uint32_t wire) {
  return reinterpret_cast<const uint8_t*>(pick3(wire, reinterpret_cast<uintptr_t>(w.b0),
                                                reinterpret_cast<uintptr_t>(w.b1), reinterpret_cast<uintptr_t>(w.b2)));
}

struct GatherScratch {
  uint64_t* ctl;       // [0] malformed connections
  uint64_t* blk;       // [nblk][kBlkFields]: entries, padded bytes, lengths, malformed entries
  uint64_t* acc;       // [c] the sum of len of the entries that name connection c
  uint64_t* edst;      // [k] where entry k's bytes start in d_buf; [n] the total
  uint32_t* tile_ent;  // [t] the entry that holds the first byte of output tile t
  size_t zero_bytes, total;
};
inline GatherScratch gather_scratch(void* base, uint64_t max_sends, uint32_t n_conns, uint32_t nblk, uint64_t buf_cap) {
  auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
  uint8_t* p = static_cast<uint8_t*>(base);
  GatherScratch s{};
  size_t o = 0;
  s.ctl = reinterpret_cast<uint64_t*>(p + o), o += 256;
  s.blk = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)nblk * kBlkFields * sizeof(uint64_t));
  s.acc = reinterpret_cast<uint64_t*>(p + o), o += up((size_t)n_conns * 8);
  s.zero_bytes = o;
  s.edst = reinterpret_cast<uint64_t*>(p + o), o += up((max_sends + 1) * 8);
  s.tile_ent = reinterpret_cast<uint32_t*>(p + o), o += up((buf_cap / kTile + 2) * 4);
  s.total = o;
  return s;
}

// ------------------------------------------------------------------ 1. checks and sizes
struct GatherDec {
  uint64_t len, padded;  // its bytes; with the span's pad when it is its connection's last entry
  uint32_t conn;
  bool bad;
};
// Entry k of n: every field is checked before it is used.
__device__ __forceinline__ GatherDec gather_decide(const gevws_send* __restrict__ send,
                                                   const gevws_conn_send* __restrict__ conn_send, uint32_t n_conns,
                                                   const GatherWires& w, uint64_t k) {
  const gevws_send e = send[k];
  GatherDec d{0, 0, 0u, true};
  if (e.wire > 2 || e.conn >= n_conns) return d;
  const uint64_t wb = wire_bytes_of(w, e.wire);
  if (e.off > wb || e.len > wb - e.off) return d;
  const gevws_conn_send cs = conn_send[e.conn];
  if (k < cs.first || k - cs.first >= cs.count) return d;
  d.bad = false;
  d.len = d.padded = e.len;
  d.conn = e.conn;
  if (k - cs.first == cs.count - 1) d.padded += (16 - (cs.bytes & 15)) & 15;
  return d;
}

__global__ __launch_bounds__(kWalkBlock) void k_gather_size(const gevws_send* __restrict__ send, uint64_t max_sends,
                                                            const gevws_conn_send* __restrict__ conn_send,
                                                            uint32_t n_conns, const gevws_summary* __restrict__ plan,
                                                            GatherWires w, uint64_t* __restrict__ acc,
                                                            uint64_t* __restrict__ blk) {
  const uint64_t n = gated_count(max_sends, plan);
  const uint64_t k = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[4] = {0, 0, 0, 0};  // entries, padded bytes, lengths, malformed entries
  uint64_t add = 0;
  uint32_t conn = 0;
  if (k < n) {
    const GatherDec d = gather_decide(send, conn_send, n_conns, w, k);
    vals[0] = 1, vals[1] = d.padded, vals[2] = d.len, vals[3] = d.bad;
    if (!d.bad) add = d.len, conn = d.conn;
  }
  // entries stand in connection order: where a wave's name one connection, one atomic for all of them
  const uint64_t act = __ballot(add != 0);
  if (act) {
    const int lead = __ffsll((unsigned long long)act) - 1;
    const uint32_t c0 = (uint32_t)__shfl((int)conn, lead, 64);
    if (__ballot(add != 0 && conn != c0) == 0) {
      const uint64_t sm = wave_sum(add);
      if ((int)(threadIdx.x & 63) == lead)
        atomicAdd(reinterpret_cast<unsigned long long*>(acc + c0), (unsigned long long)sm);
    } else if (add) {
      atomicAdd(reinterpret_cast<unsigned long long*>(acc + conn), (unsigned long long)add);
    }
  }
  block_partial<4>(vals, blk, blockIdx.x);
}

__global__ __launch_bounds__(kWalkBlock) void k_gather_conns(uint64_t max_sends,
                                                             const gevws_conn_send* __restrict__ conn_send,
                                                             uint32_t n_conns, const gevws_summary* __restrict__ plan,
                                                             const uint64_t* __restrict__ acc,
                                                             uint64_t* __restrict__ ctl) {
  const uint64_t n = gated_count(max_sends, plan);
  const uint32_t c = blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t bad = 0;
  if (n && c < n_conns) {
    const gevws_conn_send cs = conn_send[c];
    if (cs.first > n || cs.count > n - cs.first) bad = 1;
    if (c) {  // behind the connection before it (a range that overflows ends at the top)
      const gevws_conn_send pv = conn_send[c - 1];
      const uint64_t pend = pv.first + pv.count < pv.first ? UINT64_MAX : pv.first + pv.count;
      if (cs.first < pend) bad = 1;
    }
    if (cs.bytes != acc[c]) bad = 1;
  }
  const uint64_t sm = wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && sm) atomicAdd(reinterpret_cast<unsigned long long*>(ctl), (unsigned long long)sm);
}

// The scan left {entries, padded bytes, lengths, malformed entries} and
// CAPACITY against buf_cap in *sum: the gates and the malformed connections on top.
__global__ void k_gather_verdict(uint64_t max_sends, const gevws_summary* __restrict__ plan,
                                 const uint64_t* __restrict__ ctl, gevws_summary* __restrict__ sum) {
  const gevws_summary s = *sum;
  gevws_summary o;
  memset(&o, 0, sizeof(o));
  if (gated_count(max_sends, plan)) {
    if (s.errors || ctl[0]) {
      o.errors = s.errors + ctl[0];
      o.status = GEVWS_ERR_INVALID;
    } else {
      o.frames = s.frames;
      o.payload_bytes = s.payload_bytes;
      o.payload_len = s.payload_len;
      o.status = s.status;
    }
  }
  *sum = o;
}

// ------------------------------------------------------------------ 2. places and maps
__global__ __launch_bounds__(kWalkBlock) void k_gather_place(const gevws_send* __restrict__ send, uint64_t max_sends,
                                                             const gevws_conn_send* __restrict__ conn_send,
                                                             uint32_t n_conns, const gevws_summary* __restrict__ plan,
                                                             GatherWires w, const uint64_t* __restrict__ blk,
                                                             const gevws_summary* __restrict__ sum,
                                                             uint64_t* __restrict__ edst,
                                                             uint32_t* __restrict__ tile_ent) {
  if (sum->status != GEVWS_OK) return;  // capacity or a malformed record: nothing written
  const uint64_t n = gated_count(max_sends, plan);
  const uint64_t k = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t padded = 0;
  if (k < n) padded = gather_decide(send, conn_send, n_conns, w, k).padded;
  const uint64_t v[1] = {padded};
  uint64_t ex[1], tot[1];
  block_excl_scan<kWalkBlock, 1>(v, ex, tot);
  if (k >= n) return;
  const uint64_t dst = blk[(uint64_t)blockIdx.x * kBlkFields + 1] + ex[0];
  edst[k] = dst;
  if (k == n - 1) edst[n] = dst + padded;
  for (uint64_t t = (dst + kTile - 1) / kTile; t * kTile < dst + padded; ++t) tile_ent[t] = (uint32_t)k;
}

__global__ __launch_bounds__(kWalkBlock) void k_gather_spans(uint64_t max_sends,
                                                             const gevws_conn_send* __restrict__ conn_send,
                                                             uint32_t n_conns, const gevws_summary* __restrict__ plan,
                                                             const uint64_t* __restrict__ edst,
                                                             const gevws_summary* __restrict__ sum,
                                                             gevws_conn_buf* __restrict__ conn_buf) {
  if (sum->status != GEVWS_OK) return;
  const uint64_t n = gated_count(max_sends, plan);
  const uint32_t c = blockIdx.x * kWalkBlock + threadIdx.x;
  if (!n || c >= n_conns) return;
  const gevws_conn_send cs = conn_send[c];
  gevws_conn_buf o;
  memset(&o, 0, sizeof(o));
  o.off = edst[cs.first < n ? cs.first : n];  // (an empty connection: where the next span starts)
  o.bytes = cs.bytes;
  o.flags = cs.flags;
  conn_buf[c] = o;
}

// ------------------------------------------------------------------ 3. the copy
// One entry's bytes: d_buf[ds, de) come from src[0, de - ds).
struct GatherSeg {
  uint64_t ds, de;
  const uint8_t* src;
  uint64_t k;
};
// The map of the segmented copy (gevws_segcopy.hpp): an entry a segment, a
// span's pad a gap between two.
struct GatherMaps {
  using Seg = GatherSeg;
  const gevws_send* __restrict__ send;
  const uint64_t* __restrict__ edst;
  GatherWires w;
  uint64_t n, end;  // entries; the region is d_buf[0, end)

  // Entry k (k < n) as a segment.  Tables that do not fit together -- a wire or
  // a range outside the three wires, a place outside the region -- give an empty
  // one: never an address the size pass did not check.
  __device__ __forceinline__ void entry(uint64_t k, Seg& g) const {
    const gevws_send e = send[k];
    const uint64_t ds = edst[k];
    const uint64_t wb = wire_bytes_of(w, e.wire);
    const bool ok = e.wire <= 2 && e.off <= wb && e.len <= wb - e.off && ds <= end && e.len <= end - ds;
    g.k = k;
    g.ds = ds;
    g.de = ok ? ds + e.len : ds;
    g.src = wire_base_of(w, e.wire) + (ok ? e.off : 0);
  }
  // The entry at byte x of d_buf, among [lo, hi]: the last one that starts at or
  // before x (those before it at the same place are empty); false: x is a pad byte behind it.
  __device__ __forceinline__ bool find(uint64_t x, uint64_t lo, uint64_t hi, Seg& g) const {
    while (lo < hi) {
      const uint64_t mid = (lo + hi + 1) >> 1;
      if (edst[mid] <= x) lo = mid;
      else hi = mid - 1;
    }
    entry(lo, g);
    return x >= g.ds && x < g.de;
  }
  // The next entry with bytes (bounded by the entry count).
  __device__ __forceinline__ bool next(Seg& g) const {
    while (g.k + 1 < n) {
      entry(g.k + 1, g);
      if (g.de > g.ds) return true;
    }
    return false;
  }
  // A tile's first byte: the tile map's own entry, no bisection.
  __device__ __forceinline__ bool seek(uint64_t, uint64_t lo, uint64_t, bool, Seg& g) const {
    entry(lo, g);
    return true;
  }
  static __device__ __forceinline__ void uniform(Seg& g) {
    g.ds = uniform64(g.ds), g.de = uniform64(g.de), g.k = uniform64(g.k);
    g.src = reinterpret_cast<const uint8_t*>(uniform64(reinterpret_cast<uintptr_t>(g.src)));
  }
};

__global__ __launch_bounds__(kSegBlock) void k_send_gather(const gevws_send* __restrict__ send, uint64_t max_sends,
                                                           const gevws_summary* __restrict__ plan, GatherWires w,
                                                           const uint64_t* __restrict__ edst,
                                                           const uint32_t* __restrict__ tile_ent,
                                                           const gevws_summary* __restrict__ sum,
                                                           uint8_t* __restrict__ out) {
  if (sum->status != GEVWS_OK) return;
  const uint64_t n = gated_count(max_sends, plan), end = sum->payload_bytes;  // (end is on 16)
  if (n == 0 || end == 0) return;
  const GatherMaps M{send, edst, w, n, end};
  const uint64_t ntiles = (end + kTile - 1) / kTile;
  // the workgroup's run of tiles; its four waves take four tiles a step
  const uint64_t q = ntiles / gridDim.x, r = ntiles % gridDim.x;
  const uint64_t r0 = (uint64_t)blockIdx.x * q + (blockIdx.x < r ? blockIdx.x : r);
  const uint64_t r1 = r0 + q + (blockIdx.x < r ? 1 : 0);
  seg_copy_tiles(M, tile_ent, n, 0, end, r0 + uniform32(threadIdx.x >> 6), r1, kSegWaves, out);
}

}  // namespace

using namespace gevws_impl;

extern "C" int gevws_send_gather_async(gevws_ctx* ctx, void* stream, const gevws_send* d_send, uint64_t max_sends,
                                       const gevws_conn_send* d_conn_send, uint32_t n_conns,
                                       const gevws_summary* d_plan, const uint8_t* const d_wires[3],
                                       const uint64_t wire_bytes[3], uint32_t flags, uint8_t* d_buf, uint64_t buf_cap,
                                       gevws_conn_buf* d_conn_buf, gevws_summary* d_summary) {
  // vectors are loaded and stored whole and aligned: the wires and the buffer start on a 16-byte boundary
  if (flags || (reinterpret_cast<uintptr_t>(d_buf) & 15)) return GEVWS_ERR_INVALID;
  if (d_wires)
    for (int i = 0; i < 3; ++i)
      if (reinterpret_cast<uintptr_t>(d_wires[i]) & 15) return GEVWS_ERR_INVALID;
  if (!ctx || !d_summary || max_sends > 0xFFFFFFFFull) return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  if (n_conns == 0 || max_sends == 0) {
    GEVWS_HIP(hipMemsetAsync(d_summary, 0, sizeof(gevws_summary), st));
    return GEVWS_OK;
  }
  if (!d_send || !d_conn_send || !d_plan || !d_wires || !wire_bytes || !d_conn_buf || (buf_cap && !d_buf))
    return GEVWS_ERR_INVALID;
  for (int i = 0; i < 3; ++i)
    if (wire_bytes[i] && !d_wires[i]) return GEVWS_ERR_INVALID;
  const GatherWires w{d_wires[0], d_wires[1], d_wires[2], wire_bytes[0], wire_bytes[1], wire_bytes[2]};
  const uint32_t nblk = (uint32_t)((max_sends + kWalkBlock - 1) / kWalkBlock);
  const uint32_t nblkc = (n_conns + kWalkBlock - 1) / kWalkBlock;
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, gather_scratch(nullptr, max_sends, n_conns, nblk, buf_cap).total);
  if (r != GEVWS_OK) return r;
  const GatherScratch s = gather_scratch(ctx->scratch, max_sends, n_conns, nblk, buf_cap);
  GEVWS_HIP(hipMemsetAsync(s.ctl, 0, s.zero_bytes, st));
  k_gather_size<<<nblk, kWalkBlock, 0, st>>>(d_send, max_sends, d_conn_send, n_conns, d_plan, w, s.acc, s.blk);
  k_gather_conns<<<nblkc, kWalkBlock, 0, st>>>(max_sends, d_conn_send, n_conns, d_plan, s.acc, s.ctl);
  k_scan_blocks<false><<<1, kScanBlock, 0, st>>>(s.blk, nblk, UINT64_MAX, buf_cap, d_summary);
  k_gather_verdict<<<1, 1, 0, st>>>(max_sends, d_plan, s.ctl, d_summary);
  k_gather_place<<<nblk, kWalkBlock, 0, st>>>(d_send, max_sends, d_conn_send, n_conns, d_plan, w, s.blk, d_summary,
                                              s.edst, s.tile_ent);
  k_gather_spans<<<nblkc, kWalkBlock, 0, st>>>(max_sends, d_conn_send, n_conns, d_plan, s.edst, d_summary, d_conn_buf);
  k_send_gather<<<(uint32_t)ctx->num_cus * kSegWgPerCU, kSegBlock, 0, st>>>(d_send, max_sends, d_plan, w, s.edst,
                                                                            s.tile_ent, d_summary, d_buf);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}
