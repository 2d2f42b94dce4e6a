// gevws_fragment.hip -- a frame size limit for what the message chain sends
// (gevws_fragment_async, gevws_fragment_offsets_async; include/gevws.h): every
// outbound record longer than the limit becomes several records, the fragments
// of RFC 6455 section 5.4, before the encode; behind the encode the plans get
// one wire offset per reply again.  The rule is gevws_fragment.hpp's, shared
// with the host twin.  The reference writes every message as one frame
// (plugins/websocket/ws/write.go:48-84) and has no such step.
//
// gevws_fragment_async, five launches, no host round trip:
//   k_frag_count    one lane per record: its fragment count, block partials of
//                   {fragments, split records, payload bytes, malformed records}
//   k_scan_blocks   block bases, the summary, CAPACITY against max_frags
//   k_frag_verdict  one lane: the gate, INVALID
//   k_frag_first    one lane per record: d_first from the counts (recomputed:
//                   nothing but the summary is written before the verdict)
//   k_frag_emit     one lane per output fragment: its record by a bisection of
//                   d_first, one 32-byte record read, one 32-byte fragment
//                   written as two aligned 16-byte stores
// gevws_fragment_offsets_async, two launches behind one 256-byte memset:
//   k_fo_check      one lane per d_first entry: the tables against each other
//   k_fo_emit       one lane per record: d_reply_off[k] = d_frag_off[d_first[k]],
//                   lane 0 the summary
// No step reads payload bytes: no address is formed from record data.  Every
// loop is a bisection of at most 32 rounds or a grid stride over the output.
#include "gevws_internal.hpp"

#include "gevws_fragment.hpp"

namespace {

static_assert(sizeof(gevws_out_frame) == 32 && offsetof(gevws_out_frame, payload_off) == 16 &&
                  offsetof(gevws_out_frame, payload_len) == 24, "k_frag_emit moves gevws_out_frame as two 16-byte halves");

constexpr int kFragScanBlock = 256;        // k_scan_blocks' workgroup here: a block partial per 256 records
constexpr uint32_t kFragEmitWgPerCU = 16;  // k_frag_emit's grid at the most: a lane strides over the output

__device__ __forceinline__ bool frag_gate_failed(const gevws_summary* __restrict__ prev) {
  return prev && prev->status != GEVWS_OK;
}

__device__ __forceinline__ gevws_out_frame frag_load(const gevws_out_frame* __restrict__ p) {
  const uint8_t* b = reinterpret_cast<const uint8_t*>(p);
  const u32x4 v[2] = {ld16u(b), ld16u(b + 16)};
  gevws_out_frame r;
  __builtin_memcpy(&r, v, 32);
  return r;
}

// ------------------------------------------------------------------ 1. counts
__global__ __launch_bounds__(kWalkBlock) void k_frag_count(const gevws_out_frame* __restrict__ rec, uint64_t max_records,
                                                           const gevws_summary* __restrict__ prev, uint64_t F,
                                                           uint64_t* __restrict__ blk) {
  const uint64_t n = gated_count(max_records, prev);
  const uint64_t k = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t vals[4] = {0, 0, 0, 0};  // fragments, split records, payload bytes, malformed records
  if (k < n) {
    const gevws_out_frame r = frag_load(rec + k);
    bool bad;
    const uint64_t c = gevws_fragment::count(r, F, bad);
    vals[0] = c, vals[1] = c > 1, vals[2] = r.payload_len, vals[3] = bad;
  }
  block_partial<4>(vals, blk, blockIdx.x);
}

// The scan left {fragments, split records, payload bytes, malformed records}
// and CAPACITY against max_frags in *sum: the gate and INVALID on top.
__global__ void k_frag_verdict(const gevws_summary* __restrict__ prev, gevws_summary* __restrict__ sum) {
  const gevws_summary s = *sum;
  gevws_summary o;
  memset(&o, 0, sizeof(o));
  if (!frag_gate_failed(prev)) {
    if (s.errors) {
      o.errors = s.errors;
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

// ------------------------------------------------------------------ 2. d_first
__global__ __launch_bounds__(kWalkBlock) void k_frag_first(const gevws_out_frame* __restrict__ rec, uint64_t max_records,
                                                           const gevws_summary* __restrict__ prev, uint64_t F,
                                                           const uint64_t* __restrict__ blk,
                                                           const gevws_summary* __restrict__ sum,
                                                           uint64_t* __restrict__ first) {
  if (frag_gate_failed(prev) || sum->status != GEVWS_OK) return;  // (uniform over the grid)
  const uint64_t n = gated_count(max_records, prev);
  const uint64_t k = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t c = 0;
  if (k < n) {
    bool bad;
    c = gevws_fragment::count(frag_load(rec + k), F, bad);
  }
  const uint64_t v[1] = {c};
  uint64_t ex[1], tot[1];
  block_excl_scan<kWalkBlock, 1>(v, ex, tot);
  if (n == 0 && k == 0) first[0] = 0;
  if (k >= n) return;
  const uint64_t at = blk[(uint64_t)blockIdx.x * kBlkFields + 0] + ex[0];  // (exclusive after the scan)
  first[k] = at;
  if (k == n - 1) first[n] = at + c;
}

// ------------------------------------------------------------------ 3. the fragments
__global__ __launch_bounds__(kWalkBlock) void k_frag_emit(const gevws_out_frame* __restrict__ rec, uint64_t max_records,
                                                          const gevws_summary* __restrict__ prev, uint64_t F,
                                                          const uint64_t* __restrict__ first,
                                                          const gevws_summary* __restrict__ sum,
                                                          gevws_out_frame* __restrict__ frags, uint64_t max_frags) {
  if (frag_gate_failed(prev) || sum->status != GEVWS_OK) return;
  const uint64_t n = gated_count(max_records, prev);
  uint64_t total = sum->frames;
  total = total < max_frags ? total : max_frags;  // (OK means total <= max_frags: never past the buffer)
  if (n == 0) return;
  const uint64_t stride = (uint64_t)gridDim.x * kWalkBlock;
  for (uint64_t j = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x; j < total; j += stride) {
    // the record that holds fragment j: the last one whose first fragment is at or before j
    // (n < 2^32: 32 rounds; neighbouring lanes probe the same words)
    uint64_t lo = 0, hi = n - 1;
    for (int round = 0; round < 32 && lo < hi; ++round) {
      const uint64_t mid = (lo + hi + 1) >> 1;
      if (first[mid] <= j) lo = mid;
      else hi = mid - 1;
    }
    const uint64_t f0 = first[lo];
    const gevws_out_frame r = frag_load(rec + lo);
    bool bad;
    const uint64_t c = gevws_fragment::count(r, F, bad);
    if (j < f0 || j - f0 >= c) continue;  // (tables that do not fit the records: nothing made up)
    const gevws_out_frame o = gevws_fragment::fragment(r, F, c, j - f0);
    u32x4 v[2];
    __builtin_memcpy(v, &o, 32);
    u32x4* dst = reinterpret_cast<u32x4*>(frags + j);  // (frags is on a 16-byte boundary)
    dst[0] = v[0];
    dst[1] = v[1];
  }
}

// ------------------------------------------------------------------ the offsets behind the encode
struct FoGate {
  uint64_t n;     // the records; 0 when a gate failed
  int32_t status;  // the first failing gate's, or OK
  uint64_t need;   // the encode's need with its CAPACITY
};
__device__ __forceinline__ FoGate fo_gate(uint64_t max_records, const gevws_summary* __restrict__ prev,
                                          const gevws_summary* __restrict__ fragged,
                                          const gevws_summary* __restrict__ enc) {
  FoGate g{0, GEVWS_OK, 0};
  if (prev && prev->status != GEVWS_OK) g.status = prev->status;
  else if (fragged->status != GEVWS_OK) g.status = fragged->status;
  else if (enc->status != GEVWS_OK) {
    g.status = enc->status;
    if (g.status == GEVWS_ERR_CAPACITY) g.need = enc->payload_bytes;
  } else {
    g.n = gated_count(max_records, prev);
  }
  return g;
}

// Entry k of d_first[0, n]: a bad one counts once, whatever is wrong with it.
__global__ __launch_bounds__(kWalkBlock) void k_fo_check(const uint64_t* __restrict__ first, uint64_t max_records,
                                                         const gevws_summary* __restrict__ prev,
                                                         const gevws_summary* __restrict__ fragged,
                                                         const gevws_summary* __restrict__ enc,
                                                         uint64_t* __restrict__ ctl) {
  const FoGate g = fo_gate(max_records, prev, fragged, enc);
  const uint64_t k = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  uint64_t bad = 0;
  if (g.status == GEVWS_OK && k <= g.n) {
    const uint64_t v = first[k];
    if (k == 0 && v != 0) bad = 1;
    if (k < g.n && v > first[k + 1]) bad = 1;
    if (k == g.n && (v != fragged->frames || v != enc->frames)) bad = 1;
  }
  const uint64_t sm = wave_sum(bad);
  if ((threadIdx.x & 63) == 0 && sm) atomicAdd(reinterpret_cast<unsigned long long*>(ctl), (unsigned long long)sm);
}

__global__ __launch_bounds__(kWalkBlock) void k_fo_emit(const uint64_t* __restrict__ first, uint64_t max_records,
                                                        const gevws_summary* __restrict__ prev,
                                                        const gevws_summary* __restrict__ fragged,
                                                        const uint64_t* __restrict__ frag_off,
                                                        const gevws_summary* __restrict__ enc,
                                                        const uint64_t* __restrict__ ctl,
                                                        uint64_t* __restrict__ reply_off,
                                                        gevws_summary* __restrict__ sum) {
  const FoGate g = fo_gate(max_records, prev, fragged, enc);
  const uint64_t bad = ctl[0];
  const uint64_t k = (uint64_t)blockIdx.x * kWalkBlock + threadIdx.x;
  if (k == 0) {
    gevws_summary o;
    memset(&o, 0, sizeof(o));
    if (g.status != GEVWS_OK) {
      o.status = g.status;
      o.payload_bytes = g.need;
    } else if (bad) {
      o.errors = bad;
      o.status = GEVWS_ERR_INVALID;
    } else {
      o.frames = g.n;
      o.payload_bytes = enc->payload_bytes;
      o.payload_len = enc->payload_len;
    }
    *sum = o;
  }
  if (g.status != GEVWS_OK || bad || k >= g.n) return;
  // the check held: first[k] <= first[n] == the encode's count
  const uint64_t f = first[k];
  reply_off[k] = f < enc->frames ? frag_off[f] : enc->payload_bytes;
}

}  // namespace

using namespace gevws_impl;

extern "C" int gevws_fragment_async(gevws_ctx* ctx, void* stream, const gevws_out_frame* d_records,
                                    uint64_t max_records, const gevws_summary* d_prev, uint64_t max_fragment_bytes,
                                    uint32_t flags, gevws_out_frame* d_frags, uint64_t max_frags, uint64_t* d_first,
                                    gevws_summary* d_summary) {
  if (max_fragment_bytes == 0 || flags || max_records > gevws_fragment::kMaxRecords ||
      max_frags > gevws_fragment::kMaxRecords)
    return GEVWS_ERR_INVALID;
  // fragments are stored as whole aligned vectors
  if (reinterpret_cast<uintptr_t>(d_frags) & 15) return GEVWS_ERR_INVALID;
  if (!ctx || !d_summary || !d_first || (max_records && !d_records) || (max_frags && !d_frags))
    return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  const uint32_t nblk = (uint32_t)((max_records + kWalkBlock - 1) / kWalkBlock) + (max_records == 0);
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, (size_t)nblk * kBlkFields * sizeof(uint64_t));
  if (r != GEVWS_OK) return r;
  uint64_t* blk = static_cast<uint64_t*>(ctx->scratch);  // (every row is written whole by its block)
  const uint64_t F = max_fragment_bytes;
  k_frag_count<<<nblk, kWalkBlock, 0, st>>>(d_records, max_records, d_prev, F, blk);
  // (the decode's shape of the scan, four waves: in this file the 1 024-lane one is allocated with spills)
  k_scan_blocks<false, kBlkFields, kFragScanBlock><<<1, kFragScanBlock, 0, st>>>(blk, nblk, max_frags, UINT64_MAX,
                                                                                  d_summary);
  k_frag_verdict<<<1, 1, 0, st>>>(d_prev, d_summary);
  k_frag_first<<<nblk, kWalkBlock, 0, st>>>(d_records, max_records, d_prev, F, blk, d_summary, d_first);
  if (max_frags) {
    const uint64_t want = (max_frags + kWalkBlock - 1) / kWalkBlock, most = (uint64_t)ctx->num_cus * kFragEmitWgPerCU;
    k_frag_emit<<<(uint32_t)(want < most ? want : most), kWalkBlock, 0, st>>>(d_records, max_records, d_prev, F,
                                                                             d_first, d_summary, d_frags, max_frags);
  }
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}

extern "C" int gevws_fragment_offsets_async(gevws_ctx* ctx, void* stream, const uint64_t* d_first,
                                            uint64_t max_records, const gevws_summary* d_prev,
                                            const gevws_summary* d_fragged, const uint64_t* d_frag_off,
                                            const gevws_summary* d_frag_encoded, uint64_t* d_reply_off,
                                            gevws_summary* d_reply_encoded) {
  if (max_records > gevws_fragment::kMaxRecords) return GEVWS_ERR_INVALID;
  if (!ctx || !d_first || !d_fragged || !d_frag_off || !d_frag_encoded || !d_reply_encoded ||
      (max_records && !d_reply_off))
    return GEVWS_ERR_INVALID;
  DeviceGuard g(ctx->device);
  hipStream_t st = pick_stream(ctx, stream);
  int r = order_after_last(ctx, st);
  if (r != GEVWS_OK) return r;
  r = ensure_scratch(ctx, 256);
  if (r != GEVWS_OK) return r;
  uint64_t* ctl = static_cast<uint64_t*>(ctx->scratch);  // [0] bad entries
  GEVWS_HIP(hipMemsetAsync(ctl, 0, 256, st));
  const uint32_t nblk = (uint32_t)((max_records + 1 + kWalkBlock - 1) / kWalkBlock);  // n + 1 entries
  k_fo_check<<<nblk, kWalkBlock, 0, st>>>(d_first, max_records, d_prev, d_fragged, d_frag_encoded, ctl);
  k_fo_emit<<<nblk, kWalkBlock, 0, st>>>(d_first, max_records, d_prev, d_fragged, d_frag_off, d_frag_encoded, ctl,
                                         d_reply_off, d_reply_encoded);
  GEVWS_HIP(hipGetLastError());
  return mark_last(ctx, st);
}
