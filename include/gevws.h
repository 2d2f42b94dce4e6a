/*
 * gevws.h -- C ABI of the MI355X-native WebSocket frame-decode / payload-unmask
 * engine (gev_amd/libgevws.so).
 *
 * This is the drop-in boundary for gev's websocket Protocol plugin
 * (plugins/websocket/protocol.go:27-64, installed via gev.CustomProtocol,
 * options.go:83-87).  Every entry point names the reference interface it
 * replaces.  Conventions: plain C structs, caller-owned buffers, nothing
 * retained after return, int status (>= 0 ok, < 0 error).  One gevws_ctx per
 * event loop (thread-confined: it owns device scratch); no global mutable
 * state beyond one-time HIP runtime init.  See INTEGRATION.md for the cgo
 * binding a gev maintainer would add.
 */
#ifndef GEVWS_H
#define GEVWS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* 2 (round 5): the split-stream calls gevws_ctx_set_unmask_stream,
 * gevws_stream_create_cu_mask, gevws_stream_destroy and gevws_stream_cu_count
 * are gone, gevws_copy_async rejects unknown flag bits, and the round-1..3
 * measurement exports (gevws_gather_async, gevws_unmask_profile,
 * gevws_ctx_last_walk_budget, gevws_ctx_last_resumed; tuning keys 5, 6, 9-12)
 * removed in round 4 are counted here too. */
/* 3 (round 6): gevws_protocol_stats grew two fields (service_passes,
 * service_misses) -- a caller built against version 2 passes a smaller
 * struct to gevws_protocol_get_stats -- and the one-launch decode's limits
 * rose to GEVWS_ONE_LAUNCH_MAX_CONNS / _BYTES.  Added: the resident service
 * (gevws_ctx_set_service, _service_stop, _service_stats,
 * gevws_decode_batch_post, gevws_protocol_set_service), direct dispatch
 * (gevws_ctx_set_direct, _direct_dispatches, gevws_protocol_set_direct),
 * gevws_ctx_synchronize, gevws_ctx_last_split_fallbacks. */
#define GEVWS_ABI_VERSION 3

/* ---------------------------------------------------------------- status codes */
enum {
    GEVWS_OK = 0,
    GEVWS_NEED_MORE = 1,          /* (nil, nil): ws.ErrHeaderNotReady or the
                                     completeness gate failed (read.go:20-23,
                                     protocol.go:47, 59-61) */
    GEVWS_ERR_LEN_MSB = -1,       /* ws.ErrHeaderLengthMSB (read.go:12-16, 71-73);
                                     the connection stream is poisoned */
    GEVWS_ERR_CAPACITY = -2,      /* output records / payload arena too small;
                                     the summary holds the exact sizes needed */
    GEVWS_ERR_INVALID = -3,       /* bad argument */
    GEVWS_ERR_DEVICE = -4,        /* HIP runtime error */
    GEVWS_HANDSHAKE = 2,          /* (nil, out): UnPacket ran the upgrade and `out`
                                     holds the 101 response (protocol.go:29-37) */
    GEVWS_ERR_NOT_UPGRADED = -5,  /* UnPacket before the handshake on a protocol
                                     that has no upgrader (gevws_protocol_set_upgrader) */
    GEVWS_ERR_HANDSHAKE = -6      /* Upgrader.Upgrade failed (ws.go:158-343); `out`
                                     may hold the error response, which the caller
                                     sends, as protocol.go:31-34 returns (nil, out) */
};

/* Readable slack the caller must provide after the last byte of a device input
 * arena (kernels read whole 16-byte vectors). */
#define GEVWS_IN_PAD 64
/* Every payload in the output arena starts on this boundary. */
#define GEVWS_PAYLOAD_ALIGN 16
/* Output-arena tile (bytes) of the unmask kernel's work map. */
#define GEVWS_TILE 4096
/* The one-launch decode's limits (GEVWS_TUNE_SMALL_BATCH): batches of at most
 * this many connections and input bytes run as ONE kernel launch. */
#define GEVWS_ONE_LAUNCH_MAX_CONNS 1024u
#define GEVWS_ONE_LAUNCH_MAX_BYTES (128u * 1024u)

/* ws.Header, plugins/websocket/ws/frame.go:169-176.  Byte-identical to the Go
 * struct {Fin bool; Rsv byte; OpCode OpCode; Masked bool; Mask [4]byte;
 * Length int64} (offsets 0,1,2,3,4..7,8..15; 16 bytes). */
typedef struct gevws_header {
    uint8_t fin;
    uint8_t rsv;
    uint8_t opcode;
    uint8_t masked;
    uint8_t mask[4];
    int64_t length;
} gevws_header;

/* One connection's buffered bytes inside the batch input arena: the linear
 * join of its ring buffer's PeekAll() segments (connection.go:220-251). */
typedef struct gevws_conn_in {
    uint64_t off;
    uint64_t len;
} gevws_conn_in;

/* One decoded frame = one (ctx, out) pair UnPacket would have returned
 * (protocol.go:57-58).  Records are ordered by connection, then stream order.
 * The unmasked payload is payload_arena[payload_off, payload_off+hdr.length);
 * src_off is the absolute input-arena offset of the payload's first byte, so
 * the frame's header length is src_off minus the end of the previous frame. */
typedef struct gevws_frame {
    gevws_header hdr;
    uint64_t payload_off;
    uint64_t src_off;
} gevws_frame;

/* Per-connection result: what the handlerProtocol loop (connection.go:208-218)
 * would have consumed before UnPacket returned (nil, nil). */
typedef struct gevws_conn_out {
    uint64_t first_frame;   /* index of its first record */
    uint64_t consumed;      /* bytes of complete frames (sum of h + L) */
    uint64_t payload_base;  /* arena offset of its first payload */
    uint32_t nframes;
    int32_t status;         /* GEVWS_OK, GEVWS_ERR_LEN_MSB, or GEVWS_ERR_INVALID when
                               the stream [off, off + len) is not inside d_in[0, in_bytes)
                               (nothing of it is read) */
} gevws_conn_out;

/* Batch totals (written on the device). */
typedef struct gevws_summary {
    uint64_t frames;        /* decoded frames */
    uint64_t payload_bytes; /* arena bytes used (16-byte rounded lengths) */
    uint64_t payload_len;   /* sum of payload lengths */
    uint64_t errors;        /* connections with status < 0 */
    int32_t status;         /* GEVWS_OK or GEVWS_ERR_CAPACITY */
    uint32_t flags;         /* GEVWS_SUMMARY_* (decode only; informational) */
    uint64_t run_frames;    /* decode: frames the size (h + L) of the frame before them on
                               their connection -- the batch's uniformity, which picks the
                               unmask kernel's window scheme */
    uint64_t reserved[2];
} gevws_summary;

/* summary.flags: the connection table was not in increasing, non-overlapping
 * input order, so the header walk's per-connection entry runs were not used and
 * the record pass re-walked every chain (same result, slower). */
#define GEVWS_SUMMARY_UNORDERED 1u

typedef struct gevws_ctx gevws_ctx;

/* ---------------------------------------------------------------- library */
int gevws_abi_version(void);
const char *gevws_status_string(int status);
int gevws_device_count(void);

/* One context per event loop (the reference keeps one per-connection header
 * scratch, protocol.go:37; the batch engine keeps its scratch per loop).
 * Successive contexts on a device cycle their stream's priority over the
 * normal level and the levels below it (0, 1, ...): each priority level has
 * its own hardware queues, so several loops' passes run side by side, and a
 * context never outranks the application's normal-priority work.  The
 * environment variable GEVWS_STREAM_PRIORITIES=all adds the levels above
 * normal (0, -1, 1, ...); =normal keeps every context at 0. */
gevws_ctx *gevws_ctx_create(int device);
void gevws_ctx_destroy(gevws_ctx *ctx);
int gevws_ctx_device(const gevws_ctx *ctx);
/* The context's own non-blocking hipStream_t (one per event loop). */
void *gevws_ctx_stream(const gevws_ctx *ctx);
/* Makes `stream` wait for everything the context's last call enqueued (on
 * whichever stream that call was given).  The calls that use the context's
 * scratch (decode, encode, dispatch) order themselves after its previous such
 * call when the stream changes; the helpers that do not (gevws_copy_async,
 * gevws_cipher_async, gevws_synth_async, gevws_synth_verify_async) follow
 * plain HIP stream semantics, so a caller that points one at a decode's
 * outputs from another stream orders it first, with this or an event. */
int gevws_ctx_order_after_last(gevws_ctx *ctx, void *stream);
/* Tuning knobs for measurement and parity tests (defaults are the tuned
 * choice): GEVWS_TUNE_UNMASK_VARIANT the unmask kernel (0 = default: v3 4-tile
 * windows for batches of equal-size frames, v5 pipelined 8-tile windows with
 * a chunk -> frame map for mixed sizes, its workgroups taking runs of 16
 * tiles from a per-XCD counter; 1 = v5 for every batch; 2 = the default with
 * one contiguous run per workgroup on the v5 path),
 * GEVWS_TUNE_UNMASK_GRID its workgroup count (0 = auto; when set it caps the
 * encode's grid too), GEVWS_TUNE_ENCODE_VARIANT the encode's step (0 = the
 * default: two 4 KiB tiles a wave step when out_cap / n > 256 bytes, else
 * one, and the waves' runs of tiles chosen on the device; 1 / 2 = always one /
 * two tiles; 3 / 4 / 5 = two tiles with contiguous / cyclic / counter runs),
 * GEVWS_TUNE_WALK_VARIANT the header walk (0 = the
 * default choice per batch; 1 = plain chain walk without the uniform-stream
 * speculation; 2 = no per-frame entries, the record pass re-walks every
 * chain; 3 = the entries through the writer wave whatever the batch size),
 * GEVWS_TUNE_SMALL_BATCH the input size in bytes (default and maximum
 * GEVWS_ONE_LAUNCH_MAX_BYTES = 131 072; 0 = never) up to which a batch of at
 * most GEVWS_ONE_LAUNCH_MAX_CONNS = 1 024 connections is decoded by ONE kernel
 * launch -- walk, scan, records and unmask in a single workgroup with the
 * input staged in LDS -- when every other knob is at its default and
 * per-phase timing is off, GEVWS_TUNE_SPLIT_LANES the lanes per connection of the default
 * walk's split form (k_walk_split: lanes guess frame starts inside the stream
 * and walk the segments between the guesses; a connection whose guesses do
 * not all line up is re-walked serially, so the output never depends on
 * them): 0 = auto (the batch's connections x lanes up to 256 per CU, streams
 * of >= 32 KiB mean), 1 = never, 2 / 4 / 8 / 16 / 32 = always.  Keys 5, 6,
 * 9-12 (round 1-3 measurement variants) are retired and rejected. */
#define GEVWS_TUNE_UNMASK_VARIANT 1
#define GEVWS_TUNE_UNMASK_GRID 2
#define GEVWS_TUNE_ENCODE_VARIANT 3
#define GEVWS_TUNE_WALK_VARIANT 4
#define GEVWS_TUNE_SMALL_BATCH 7
#define GEVWS_TUNE_SPLIT_LANES 8
/* Split walk (GEVWS_TUNE_SPLIT_LANES): a connection is cut into segments of at
 * least this many bytes (default 16 384; 1 024 .. 2^30) ... */
#define GEVWS_TUNE_SPLIT_MIN_BYTES 13
/* ... and the auto choice doubles the lanes per connection while the walk
 * keeps at most this many lanes per CU (default 512; 64 .. 4 096). */
#define GEVWS_TUNE_SPLIT_LANES_PER_CU 14
int gevws_ctx_set_tuning(gevws_ctx *ctx, int key, int64_t value);
/* Lanes per connection the last multi-kernel decode's header walk used (1 =
 * not split; GEVWS_TUNE_SPLIT_LANES), -1 for a null context.  The auto choice
 * splits a batch of few connections once an earlier decode on this context
 * has shown long chains of small frames (>= 256 frames per connection of <= 4
 * KiB each). */
int gevws_ctx_last_split_lanes(const gevws_ctx *ctx);
/* Connections of the last multi-kernel decode's split walk whose guesses did
 * not line up, so the walk re-walked them serially (0 when it was not split;
 * -1 for a null context or a device error).  Waits for the context's last
 * call.  Measurement: each costs its whole chain's serial walk. */
int64_t gevws_ctx_last_split_fallbacks(gevws_ctx *ctx);
/* Completion signal of the one-launch kernels (a live pass's: the small-batch
 * decode and gevws_handle_decoded_async's one-workgroup form).  With d_flag
 * (the device address of a 32-bit word in mapped, coherent host memory) set,
 * each such launch numbers itself and its kernel stores that number there
 * after all its outputs are visible at system scope; a host then spins on
 * host memory instead of hipStreamSynchronize.  NULL turns it off (the
 * default).  gevws_ctx_completion_seq: the number the last call's last kernel
 * stores, or -1 when that call ended with another kernel or copy (the caller
 * synchronises the stream as usual). */
int gevws_ctx_set_completion_flag(gevws_ctx *ctx, uint32_t *d_flag);
/* The resident decode service (opt-in; a live loop's passes without the launch
 * call's ~5 us of host time).  With it on and a completion flag set,
 * gevws_decode_batch_post hands a pass of at most 256 connections and 64 KiB
 * to a kernel kept resident on the context's stream (launched by the first
 * post; 32 workgroups, as many as a launched live pass stages its input with):
 * the pass's arguments go into a mailbox in mapped host memory, the kernel
 * polls it, decodes exactly as the one-launch decode and stores the pass's
 * number in the completion word.  One pass at a time: a post before the last
 * posted pass has signalled is launched instead, behind it.  Any other call
 * that enqueues work on the context ends the instance first (the pass posted
 * before it still runs, and that work runs behind it); an instance also ends
 * 200 ms after its start (the next post replaces it after 100 ms).  While one
 * is live the context's stream does not drain: call gevws_ctx_service_stop
 * before synchronising it directly.  enable = 0 stops it and turns posting
 * off (the default).  gevws_ctx_service_stats: instances launched and passes
 * posted to them, since the context's creation. */
int gevws_ctx_set_service(gevws_ctx *ctx, int enable);
int gevws_ctx_service_stop(gevws_ctx *ctx);
int gevws_ctx_service_stats(const gevws_ctx *ctx, int64_t *launches, int64_t *posts);
/* Direct dispatch (opt-in; takes precedence over the service): with it on and
 * a completion flag set, gevws_decode_batch_post writes a pass that fits the
 * one-launch decode (<= GEVWS_ONE_LAUNCH_MAX_CONNS / _BYTES) as one AQL
 * dispatch packet into an HSA queue the context owns -- the same kernel body,
 * without the HIP runtime's launch call on the caller's path.  Work the
 * context enqueues on a stream after such passes first waits (on the host)
 * for their completion words, and a direct pass after stream work waits for
 * that work.  If the runtime's loader does not expose the kernels, the
 * context falls back to launching (gevws_ctx_direct_dispatches stays 0).
 * enable = 0 waits for the outstanding direct passes and turns it off. */
int gevws_ctx_set_direct(gevws_ctx *ctx, int enable);
int64_t gevws_ctx_direct_dispatches(const gevws_ctx *ctx);
/* Waits for everything the context has enqueued: its stream, the passes on
 * its own queue, a live service instance (stopped first). */
int gevws_ctx_synchronize(gevws_ctx *ctx);
/* With a completion flag set: d_ticks (device address of 4 u64 in mapped,
 * coherent host memory, or NULL = off) receives, before the flag, each
 * one-launch kernel's start and end tick of the GPU's constant-rate wall
 * clock (s_memrealtime; hipDeviceAttributeWallClockRate kHz): [0] / [1] the
 * small-batch decode, [2] / [3] the one-workgroup handler step. */
int gevws_ctx_set_timeline_ticks(gevws_ctx *ctx, uint64_t *d_ticks);
int64_t gevws_ctx_completion_seq(const gevws_ctx *ctx);
/* Workgroups of the last multi-kernel decode's unmask launch (-1 for a null
 * context): 4 per CU, or 32 per CU after a decode on this context of a batch
 * of mixed frame sizes below 8 GiB of output (the kernel then uses the wide
 * grid if this batch is one too). */
int gevws_ctx_last_unmask_grid(const gevws_ctx *ctx);
/* Human-readable name of a variant (GEVWS_TUNE_UNMASK_VARIANT or
 * GEVWS_TUNE_WALK_VARIANT), or NULL past the last one. */
const char *gevws_tuning_name(int key, int64_t value);
/* Per-phase HIP-event timing of the following decode calls (0 = off). */
int gevws_ctx_set_timing(gevws_ctx *ctx, int enable);
/* Waits for the timed calls since the previous query and returns the summed
 * ms per phase -- [0] header walk (count), [1] scan, [2] header walk (emit),
 * [3] unmask/compact -- and the number of calls; then resets. */
int gevws_ctx_timing(gevws_ctx *ctx, float ms_sum[4], uint32_t *calls);

/* ---------------------------------------------------------------- hot path
 * Device-resident batch decode: for every connection, repeated
 * websocket.(*Protocol).UnPacket (plugins/websocket/protocol.go:38-62 ->
 * ws.VirtualReadHeader read.go:19-84 -> completeness gate protocol.go:47 ->
 * payload copy protocol.go:50-51 -> ws.Cipher cipher.go:14-53) until it would
 * return (nil, nil), exactly as Connection.handlerProtocol drives it
 * (connection.go:208-218).  All pointers d_* are device pointers; d_in must
 * have GEVWS_IN_PAD readable bytes past in_bytes.  Enqueued on `stream`
 * (hipStream_t; NULL = the HIP default stream).  Returns GEVWS_OK when
 * enqueued; the batch's own outcome is d_summary->status. */
int gevws_decode_batch_async(gevws_ctx *ctx, void *stream, const uint8_t *d_in, uint64_t in_bytes,
                             const gevws_conn_in *d_conns, uint32_t n_conns,
                             gevws_frame *d_frames, uint64_t max_frames,
                             uint8_t *d_payload, uint64_t payload_cap,
                             gevws_conn_out *d_conn_out, gevws_summary *d_summary);
/* A live pass on the context's own stream: posted to the resident decode
 * service when it is on (gevws_ctx_set_service), a completion flag is set and
 * the pass fits its shape (<= 256 connections, <= 64 KiB), else
 * exactly gevws_decode_batch_async on the context's stream.  Either way the
 * caller waits for gevws_ctx_completion_seq in the completion word (-1: the
 * stream). */
int gevws_decode_batch_post(gevws_ctx *ctx, const uint8_t *d_in, uint64_t in_bytes,
                            const gevws_conn_in *d_conns, uint32_t n_conns, gevws_frame *d_frames,
                            uint64_t max_frames, uint8_t *d_payload, uint64_t payload_cap,
                            gevws_conn_out *d_conn_out, gevws_summary *d_summary);

/* Synchronous form: same work, waits, copies the summary to *h_summary and
 * returns its status. */
int gevws_decode_batch(gevws_ctx *ctx, void *stream, const uint8_t *d_in, uint64_t in_bytes,
                       const gevws_conn_in *d_conns, uint32_t n_conns, gevws_frame *d_frames,
                       uint64_t max_frames, uint8_t *d_payload, uint64_t payload_cap,
                       gevws_conn_out *d_conn_out, gevws_summary *h_summary);

/* ---------------------------------------------------------------- outbound encode
 * One reply frame: the header to serialise and where its payload bytes are
 * (e.g. a decoded frame's slot in a payload arena). */
typedef struct gevws_out_frame {
    gevws_header hdr;
    uint64_t payload_off;
    uint64_t payload_len;
} gevws_out_frame;

/* Extra writable bytes the caller must provide past out_cap (the encoder
 * stores whole 16-byte vectors; bytes past the wire total are zeroed). */
#define GEVWS_OUT_PAD 16

/* ws.FrameToBytes (frame.go:274-278) = ws.WriteHeader (write.go:48-84) +
 * payload, for n frames at once, written back to back into d_out (the bytes
 * handlerProtocol appends to its send buffer, connection.go:208-218).
 * d_out_off[f] receives frame f's wire offset; d_summary->payload_bytes the
 * wire total, ->payload_len the payload total, ->status GEVWS_ERR_CAPACITY if
 * the total exceeds out_cap (nothing written to d_out; d_out_off[f] then holds
 * frame f's wire size h + L).  Payload bytes are read as
 * 16-byte vectors: d_payload needs 16 readable bytes past its last payload
 * byte (a decode's payload arena has them).  Device pointers; enqueued on
 * `stream`. */
int gevws_encode_batch_async(gevws_ctx *ctx, void *stream, const gevws_out_frame *d_frames, uint64_t n,
                             const uint8_t *d_payload, uint8_t *d_out, uint64_t out_cap,
                             uint64_t *d_out_off, gevws_summary *d_summary);

/* ---------------------------------------------------------------- control-frame dispatch
 * HandlerWrap.OnMessage (plugins/websocket/wrap.go:38-90) over decoded frames:
 * close -> util.HandleClose reply (util.go:27-46; close-code checks and UTF-8
 * validation of the reason as CheckCloseFrameData, util.go:65-85) and a
 * ShutdownWrite; ping -> pong with the same payload; pong -> ping with the
 * same payload (util.go:54-56, as the reference does); other control opcodes ->
 * nothing; data frames -> `policy` standing in for the user's WSHandler. */
enum {
    GEVWS_HANDLER_NONE = 0,        /* user handler replies nothing */
    GEVWS_HANDLER_ECHO_BINARY = 1, /* benchmarks/websocket/server.go:22-29 */
    GEVWS_HANDLER_ECHO_TEXT = 2    /* example/websocket OnMessage shape */
};
/* Bytes of aux space per close reply body (bodies are <= 125 bytes). */
#define GEVWS_AUX_SLOT 128

/* d_frames/n: a decode's records; d_payload: its payload arena, whose region
 * [aux_off, aux_off + aux_cap) receives the close-reply bodies (one
 * GEVWS_AUX_SLOT each).  Writes the replies in stream order to d_replies
 * (capacity n; payload_off relative to d_payload, ready for
 * gevws_encode_batch_async with the same d_payload) and d_reply_of[f] = reply
 * index or -1.  d_summary: frames = replies, payload_bytes = aux slots used,
 * errors = close frames (ShutdownWrite calls), status GEVWS_ERR_CAPACITY if
 * the aux region is too small. */
int gevws_dispatch_async(gevws_ctx *ctx, void *stream, const gevws_frame *d_frames, uint64_t n, int policy,
                         uint8_t *d_payload, uint64_t aux_off, uint64_t aux_cap,
                         gevws_out_frame *d_replies, int64_t *d_reply_of, gevws_summary *d_summary);

/* The same two steps chained after a decode with no host round trip (a live
 * pass: decode -> HandlerWrap.OnMessage -> FrameToBytes on the device): the
 * frame / reply count is read on the device from the previous step's summary
 * (d_decoded: the decode's; d_dispatched: the dispatch's), none when that
 * step failed; max_frames / max_replies only bound the launch and the
 * buffers (d_reply_of: max_frames entries, d_replies / d_out_off:
 * max_replies). */
int gevws_dispatch_decoded_async(gevws_ctx *ctx, void *stream, const gevws_frame *d_frames, uint64_t max_frames,
                                 const gevws_summary *d_decoded, int policy, uint8_t *d_payload, uint64_t aux_off,
                                 uint64_t aux_cap, gevws_out_frame *d_replies, int64_t *d_reply_of,
                                 gevws_summary *d_summary);
int gevws_encode_replies_async(gevws_ctx *ctx, void *stream, const gevws_out_frame *d_replies,
                               uint64_t max_replies, const gevws_summary *d_dispatched, const uint8_t *d_payload,
                               uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off, gevws_summary *d_summary);
/* Both steps at once behind a decode: gevws_dispatch_decoded_async then
 * gevws_encode_replies_async (same arguments, summaries and outputs).  A pass
 * of at most 1 024 frames with out_cap < 2^31 -- a live event loop's -- runs
 * them as ONE kernel launch (one workgroup); larger ones take the two steps'
 * seven launches.  d_out needs GEVWS_OUT_PAD bytes of slack after out_cap. */
int gevws_handle_decoded_async(gevws_ctx *ctx, void *stream, const gevws_frame *d_frames, uint64_t max_frames,
                               const gevws_summary *d_decoded, int policy, uint8_t *d_payload, uint64_t aux_off,
                               uint64_t aux_cap, gevws_out_frame *d_replies, int64_t *d_reply_of,
                               gevws_summary *d_disp_summary, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off,
                               gevws_summary *d_enc_summary);

/* ---------------------------------------------------------------- message layer
 * What the reference leaves to the user's OnMessage (wrap.go:71 hands every
 * data frame's payload over as it is): RFC 6455 message assembly and checks
 * for a server reading client frames with no extension negotiated -- section
 * 5.2 (RSV bits, reserved opcodes), 5.4 (fragmentation), 5.5 (control frames
 * are not fragmented and carry <= 125 bytes) and 8.1 (text is UTF-8).  An
 * opt-in step behind a decode, beside gevws_dispatch_decoded_async.
 *
 * For each connection with status == GEVWS_OK its frames are taken in order,
 * starting from its carry state; the first hit of these checks, in this
 * order, fails the connection at that frame:
 *   1. rsv != 0                                      GEVWS_MSG_ERR_RSV           (5.2)
 *   2. opcode 3-7 or 0xB-0xF                         GEVWS_MSG_ERR_OPCODE        (5.2)
 *   3. control frame, fin == 0 or length > 125       GEVWS_MSG_ERR_CONTROL       (5.5)
 *   4. opcode 0 with no message open                 GEVWS_MSG_ERR_CONTINUATION  (5.4)
 *   5. opcode 1 / 2 while a message is open          GEVWS_MSG_ERR_INTERLEAVE    (5.4)
 *   6. in a text message, a byte that cannot continue a valid UTF-8 sequence
 *      (at the frame holding it), or the message's FIN frame ending inside a
 *      sequence (at the FIN frame)                   GEVWS_MSG_ERR_UTF8          (8.1)
 * UTF-8 is strict, as unicode/utf8.Valid: no overlong forms, no surrogates,
 * nothing above U+10FFFF.  The sequence state runs across the fragments of
 * one text message (control frames in between do not disturb it); payloads of
 * binary messages and of control frames are not validated (dispatch checks
 * the close reason).  A caller closes a failed connection with status 1002
 * (protocol error) for errors 1-5 and 1007 (invalid payload data) for 6
 * (section 7.4.1); gevws_control_async below builds that close frame. */
enum {
    GEVWS_MSG_OK = 0,
    GEVWS_MSG_ERR_RSV = 1,
    GEVWS_MSG_ERR_OPCODE = 2,
    GEVWS_MSG_ERR_CONTROL = 3,
    GEVWS_MSG_ERR_CONTINUATION = 4,
    GEVWS_MSG_ERR_INTERLEAVE = 5,
    GEVWS_MSG_ERR_UTF8 = 6
};
#define GEVWS_MSG_BEGIN 1u   /* opened in this batch */
#define GEVWS_MSG_END   2u   /* its FIN frame is in this batch */

/* What a connection carries from one pass to the next; zero = fresh. */
typedef struct gevws_msg_state {
    uint8_t opcode;     /* 0: no message open; 1 / 2: the open message's */
    uint8_t failed;     /* sticky GEVWS_MSG_ERR_* */
    uint8_t utf8_n;     /* 0..3 bytes of an unfinished sequence at the end of the open text message */
    uint8_t utf8[3];
    uint8_t reserved[2];
} gevws_msg_state;

/* One message: the data frames (opcode 1 / 2 and its continuations) from
 * first_frame on that map to it in d_msg_of.  A single-frame message's payload
 * is its frame's; a fragmented one's stays in its frames' slots
 * (gevws_join_async below gathers it into one contiguous body). */
typedef struct gevws_message {
    uint64_t first_frame;   /* record index of its first data frame in this batch */
    uint64_t length;        /* payload bytes of its data frames in this batch */
    uint32_t conn;
    uint32_t nframes;       /* its data frames in this batch */
    uint8_t opcode;         /* 1 text, 2 binary (from the carry state when continued) */
    uint8_t flags;          /* GEVWS_MSG_BEGIN | GEVWS_MSG_END */
    uint8_t status;         /* GEVWS_MSG_OK or GEVWS_MSG_ERR_UTF8 */
    uint8_t reserved[5];
} gevws_message;

typedef struct gevws_conn_msg {
    uint64_t first_message;
    uint64_t error_frame;   /* record index, or UINT64_MAX */
    uint32_t nmessages;
    int32_t error;          /* GEVWS_MSG_OK or the first GEVWS_MSG_ERR_* */
    uint64_t reserved;
} gevws_conn_msg;

/* d_frames / d_conn_out / d_decoded / d_payload: a decode's records,
 * per-connection table, summary and payload arena (the frame count is read on
 * the device from d_decoded, none if that decode failed; max_frames bounds the
 * launch, the scratch and d_msg_of; at most 2^32 - 1).  Every payload starts
 * on GEVWS_PAYLOAD_ALIGN and is read as whole 16-byte vectors, but only
 * hdr.length bytes of it count: the pad is never relied on.
 *
 * d_messages receives one record per message with at least one data frame in
 * this batch, ordered by connection, then stream order -- a message continued
 * from the carry state has no BEGIN flag and the state's opcode, one still
 * open after the connection's last frame has no END flag (the state carries
 * the rest).  d_msg_of[f] = the message of data frame f, -1 for every other
 * frame (valid control frames between fragments belong to no message).
 * d_conn_msg[c]: the connection's messages and its verdict.
 *
 * After a failure: on errors 1-5 the failing frame and every later frame of
 * the connection map to no message, and an open message is emitted as it
 * stood (no END, status OK); on a UTF-8 error the open message is emitted
 * with status GEVWS_MSG_ERR_UTF8, counting frames and bytes up to and
 * including the failing frame, without END, and the later frames map to no
 * message.  The error is sticky in the state: a connection that comes in
 * failed yields no messages and reports that error with error_frame ==
 * UINT64_MAX.  Connections with status < 0 or no frames yield nothing, report
 * what their state holds the same way, and keep their state.
 *
 * d_state: n_conns entries read and rewritten (NULL: every connection fresh,
 * nothing kept).  d_summary: frames = messages emitted, payload_len = payload
 * bytes of the text messages emitted (the bytes the UTF-8 check answers for),
 * errors = connections that failed in this batch, status GEVWS_ERR_CAPACITY
 * when there are more messages than max_messages -- frames then holds the
 * count needed, d_messages / d_conn_msg are not written and d_state is left
 * untouched, so the caller retries.  n_conns == 0, max_frames == 0, no
 * decoded frames or a failed d_decoded give a zero summary and read none of
 * the inputs (with connections, every d_conn_msg entry is still written: no
 * messages, no error). */
int gevws_messages_async(gevws_ctx *ctx, void *stream,
                         const gevws_frame *d_frames, uint64_t max_frames,
                         const gevws_conn_out *d_conn_out, uint32_t n_conns,
                         const gevws_summary *d_decoded, const uint8_t *d_payload,
                         gevws_msg_state *d_state,
                         gevws_message *d_messages, uint64_t max_messages,
                         int64_t *d_msg_of, gevws_conn_msg *d_conn_msg, gevws_summary *d_summary);

/* unicode/utf8.Valid(p[:n]) in host memory (scalar; the rule the device pass
 * applies per byte): 1 valid, 0 not. */
int gevws_utf8_valid(const uint8_t *p, uint64_t n);

/* ---------------------------------------------------------------- permessage-deflate (RFC 7692)
 * The message pass for connections that negotiated the extension, and the
 * step that inflates their compressed messages on the device.  Additions to
 * ABI version 3: nothing above changes.
 *
 * gevws_messages_ext_async is gevws_messages_async plus d_conn_ext, one byte
 * per connection; NULL or a zero byte is the plain pass, bit for bit
 * (gevws_messages_async is the NULL call).  For a connection with
 * GEVWS_EXT_DEFLATE (hdr.rsv is (b0 & 0x70) >> 4, so RSV1 is 4):
 *   - check 1 becomes: rsv & 3, or rsv & 4 on a control frame or on a
 *     continuation frame, is GEVWS_MSG_ERR_RSV; the order of the checks stays;
 *   - a frame with opcode 1 / 2 and RSV1 opens a compressed message: its
 *     record carries GEVWS_MSG_COMPRESSED, and while it is open
 *     gevws_msg_state.reserved[0] is 1 (zero: not compressed, so states
 *     written before stay valid); a message continued from the state is
 *     flagged from it;
 *   - text frames of a compressed message are not UTF-8-checked (their bytes
 *     are DEFLATE), do not count in summary.payload_len, and leave the
 *     state's utf8 fields zero. */
#define GEVWS_EXT_DEFLATE 1u
#define GEVWS_MSG_COMPRESSED 4u   /* gevws_message.flags */
int gevws_messages_ext_async(gevws_ctx *ctx, void *stream,
                             const gevws_frame *d_frames, uint64_t max_frames,
                             const gevws_conn_out *d_conn_out, uint32_t n_conns,
                             const gevws_summary *d_decoded, const uint8_t *d_payload,
                             gevws_msg_state *d_state,
                             gevws_message *d_messages, uint64_t max_messages,
                             int64_t *d_msg_of, gevws_conn_msg *d_conn_msg, gevws_summary *d_summary,
                             const uint8_t *d_conn_ext);

/* The inflate step, behind the message pass and on its tables.
 *
 * Input.  For every message with COMPRESSED | BEGIN | END the compressed
 * stream S is the payloads of its data frames in order -- the frames f from
 * first_frame on with d_msg_of[f] == m; control frames in between, empty
 * fragments and the slots' padding are skipped, only hdr.length bytes of a
 * frame are read -- followed by the four bytes 00 00 ff ff (RFC 7692 section
 * 7.2.2).  No context takeover: every message starts with an empty window
 * (gevws_deflate_negotiate answers offers accordingly;
 * gevws_inflate_ctx_async below is the step with client context takeover).
 *
 * Verdict.  S is raw DEFLATE (RFC 1951) read from bit 0.  A block that ends
 * with BFINAL set ends the message (the rest of S is ignored); a block that
 * ends with no whole byte of S unread ends it as well.  Running out of S
 * anywhere else, a distance beyond the bytes produced so far and anything
 * zlib's inflate rejects (block type 3, stored LEN != ~NLEN, more than 286
 * length or 30 distance codes, an over-subscribed or disallowed-incomplete
 * code, a repeat with nothing to repeat or past the end, no end-of-block code,
 * length symbols 286 / 287, distance symbols 30 / 31, an unassigned code) are
 * GEVWS_MSG_ERR_DEFLATE: truncation and malformation share the code.  More
 * than max_message_bytes (1 .. 2^32 - 1) bytes of output is
 * GEVWS_MSG_ERR_TOO_BIG.  A text message whose inflated bytes fail
 * gevws_utf8_valid is GEVWS_MSG_ERR_UTF8; its bytes and length are kept.
 *
 * Output.  d_inflated[m] belongs to d_messages[m].  The inflated messages lie
 * in d_out in message order, each on a GEVWS_PAYLOAD_ALIGN boundary, the pad
 * behind each zeroed; a message that failed with DEFLATE or TOO_BIG takes no
 * space.  Compressed messages without both BEGIN and END are not touched and
 * get GEVWS_INF_PENDING (the caller holds their input: a compressed message
 * is inflated by the pass that sees all of it).  Messages that are not
 * compressed get a zero record.  d_summary: frames = messages inflated with
 * status OK, payload_bytes = bytes of d_out used, payload_len = the sum of
 * the lengths, errors = messages that failed; status GEVWS_ERR_CAPACITY when
 * out_cap is too small -- payload_bytes then holds the need, nothing else is
 * written and d_state is untouched, so the caller retries.  With d_state, a
 * connection's first failed message in batch order sets its `failed` if that
 * was zero; its later messages are still inflated.  A failed d_msg_summary or
 * no messages give a zero summary and read none of the inputs. */
enum { GEVWS_MSG_ERR_DEFLATE = 7, GEVWS_MSG_ERR_TOO_BIG = 8 };   /* continue the GEVWS_MSG_* enum */
#define GEVWS_INF_DONE 1u      /* inflated in this call (status says how it went) */
#define GEVWS_INF_PENDING 2u   /* compressed, but not whole in this batch: not touched */
typedef struct gevws_inflated {   /* 32 bytes */
    uint64_t out_off;   /* into d_out, on GEVWS_PAYLOAD_ALIGN */
    uint64_t length;    /* inflated bytes; 0 unless status is OK or ERR_UTF8 */
    uint8_t status;     /* GEVWS_MSG_OK, _ERR_DEFLATE, _ERR_TOO_BIG, _ERR_UTF8 */
    uint8_t flags;      /* GEVWS_INF_*; 0 for a message that is not compressed */
    uint8_t reserved[14];
} gevws_inflated;
int gevws_inflate_async(gevws_ctx *ctx, void *stream, const gevws_frame *d_frames, uint64_t max_frames,
                        const gevws_message *d_messages, uint64_t max_messages, const int64_t *d_msg_of,
                        const gevws_summary *d_msg_summary, const uint8_t *d_payload,
                        uint64_t max_message_bytes, gevws_msg_state *d_state /* may be NULL */,
                        gevws_inflated *d_inflated, uint8_t *d_out, uint64_t out_cap, gevws_summary *d_summary);

/* The same decoder on host memory: in[0, n) is one message's compressed
 * payload (the tail 00 00 ff ff is appended inside), out[0, cap) receives at
 * most cap bytes.  Returns GEVWS_MSG_OK, GEVWS_MSG_ERR_DEFLATE or
 * GEVWS_MSG_ERR_TOO_BIG (more than cap bytes), or GEVWS_ERR_INVALID for a
 * NULL buffer; *out_len = the bytes written before the verdict. */
int gevws_inflate_raw(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len);

/* Client context takeover: the inflate step with a 32 KiB window per
 * connection, kept between messages and between passes.  Additions to ABI
 * version 3: nothing above changes.  (The outbound direction keeps
 * server_no_context_takeover; a compressed message that spans two passes is
 * GEVWS_INF_PENDING here and whole in gevws_inflate_carry_async.)
 *
 * GEVWS_EXT_CLIENT_TAKEOVER is a second bit of the d_conn_ext byte, set beside
 * GEVWS_EXT_DEFLATE for a connection whose client may keep its LZ77 window
 * (gevws_deflate_negotiate_flags says when).  The message pass looks at
 * GEVWS_EXT_DEFLATE only: the byte 3 is the byte 1 to it.
 *
 * Semantics.  For such a connection let H be the last min(32 768, total) bytes
 * of the inflated output of its earlier compressed messages -- earlier in this
 * pass and in earlier passes, in stream order.  H is what zlib's window holds,
 * so a distance of exactly 32 768 is allowed.  Verdict and bytes of the next
 * compressed message with payload P are what the rules above give for the
 * stream "H as stored blocks with BFINAL 0, then P" with max_message_bytes +
 * |H| as the limit, the first |H| output bytes dropped: a distance may reach
 * min(32 768, out + |H|) back, everything else is unchanged.
 *   - A block with BFINAL set ends the message as above; the window continues.
 *   - Uncompressed messages of the connection (RSV1 clear) do not enter the
 *     window.
 *   - A message that inflates but fails UTF-8 keeps the context: its bytes
 *     are in the window.
 *   - GEVWS_MSG_ERR_DEFLATE or GEVWS_MSG_ERR_TOO_BIG loses the context.  The
 *     connection's later compressed messages in the batch get GEVWS_INF_DONE,
 *     the first failure's status and length 0; they take no space and count
 *     in `errors`.  The slot is marked broken and the mark is sticky: in later
 *     passes every compressed message of the connection, whole or not, gets
 *     that status without being decoded.  With d_state, `failed` is set as
 *     above.
 *   - A compressed message without BEGIN or END stops the connection's chain:
 *     it and every later compressed message of the connection in the batch are
 *     GEVWS_INF_PENDING, and the window stands where the last whole message
 *     left it.  (A message without END is the connection's last; one without
 *     BEGIN is its first, so the slot is left untouched.)  Shown again, whole,
 *     in a later pass it is inflated then.
 *   - GEVWS_ERR_CAPACITY: nothing is written and the slots are untouched, byte
 *     for byte, so the retry sees the same contexts.
 *
 * The slot.  d_inf_ctx is a caller-owned device buffer of n_conns slots of
 * GEVWS_INF_CTX_BYTES each, on a 16-byte boundary; connection c's is slot c.
 * All-zero is a fresh connection.  Callers treat a slot as opaque; its layout
 * is a 64-byte head -- uint64 total (little-endian: the bytes the connection's
 * compressed messages have inflated to), uint8 broken (0, or the status that
 * lost the context), zeros -- and behind it the ring image: stream byte i sits
 * at ring[i & 32767], bytes never written stay zero.  A slot's content is a
 * function of the connection's stream only, not of how the stream was cut
 * into passes, and gevws_inflate_raw_ctx produces the same bytes on the host.
 * Behaviour depends on `total` only through min(total, 32 768) and total mod
 * 32 768: a connection that has inflated 2^32 or 2^62 bytes is served as one
 * that has inflated 70 000 (the tests relocate slots across those positions).
 * 32 832 bytes a connection: 538 MB of device memory for 16 384 connections.
 *
 * gevws_inflate_ctx_async is gevws_inflate_async plus d_conn_ext (one byte per
 * connection), d_inf_ctx and n_conns.  With either pointer NULL it is
 * gevws_inflate_async bit for bit (which is that NULL call).  A connection
 * without GEVWS_EXT_CLIENT_TAKEOVER is inflated as above and its slot is
 * neither read nor written.  A takeover connection's messages depend on each
 * other in order, so one wave inflates them one after another.  A message
 * record with conn >= n_conns makes the call GEVWS_ERR_INVALID on the device:
 * d_summary gets that status and the count of such records in `errors`, and
 * nothing else is written (no slot is indexed by such a record).  With
 * contexts max_messages is at most 0x7FF00000. */
#define GEVWS_EXT_CLIENT_TAKEOVER 2u
#define GEVWS_INF_CTX_BYTES (32768u + 64u)
int gevws_inflate_ctx_async(gevws_ctx *ctx, void *stream, const gevws_frame *d_frames, uint64_t max_frames,
                            const gevws_message *d_messages, uint64_t max_messages, const int64_t *d_msg_of,
                            const gevws_summary *d_msg_summary, const uint8_t *d_payload,
                            uint64_t max_message_bytes, gevws_msg_state *d_state /* may be NULL */,
                            gevws_inflated *d_inflated, uint8_t *d_out, uint64_t out_cap, gevws_summary *d_summary,
                            const uint8_t *d_conn_ext, uint8_t *d_inf_ctx, uint32_t n_conns);

/* gevws_inflate_raw over one slot in host memory (ctx[0, GEVWS_INF_CTX_BYTES)):
 * the message is inflated with the slot's window behind it, and a message
 * that inflates is appended to the window.  A failure marks the slot broken
 * and leaves its window; a broken slot returns its status at once with
 * *out_len = 0.  A zeroed slot gives gevws_inflate_raw's result.  A NULL ctx
 * is GEVWS_ERR_INVALID. */
int gevws_inflate_raw_ctx(const uint8_t *in, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len,
                          uint8_t *ctx);

/* Answers a Sec-WebSocket-Extensions request value (offer[0, n)) for a server
 * that inflates on the device: the first permessage-deflate offer it can
 * serve is answered with
 *   permessage-deflate; client_no_context_takeover; server_no_context_takeover
 * plus "; server_max_window_bits=N" when the offer carried it (any N in 8..15:
 * a server that compresses hands N to gevws_deflate_async as a message's
 * window_bits, one that answers uncompressed holds any N).  client_max_window_bits, with
 * or without a value in 8..15, is accepted and not echoed.  An offer with an
 * unknown parameter, a repeated one or a bad value is skipped.  *out_len = the
 * answer's length, 0 when no offer is usable or the value is malformed.
 * Returns GEVWS_OK, or GEVWS_ERR_CAPACITY when the answer does not fit
 * out[0, cap).  Meant to be called from the upgrader's extension_custom hook. */
int gevws_deflate_negotiate(const uint8_t *offer, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_len);

/* The same with flags, and the byte to store in d_conn_ext for the connection
 * (*conn_ext, may be NULL): GEVWS_EXT_DEFLATE, or 0 when no offer is usable.
 * Flags 0 writes gevws_deflate_negotiate's answer byte for byte.
 * GEVWS_NEGOTIATE_CLIENT_TAKEOVER leaves client_no_context_takeover out of the
 * answer, and sets GEVWS_EXT_CLIENT_TAKEOVER in *conn_ext, unless the chosen
 * offer carried the parameter: then it is echoed and the bit stays clear.
 * server_no_context_takeover is always sent, server_max_window_bits echoed as
 * above; client_max_window_bits is accepted and not echoed, so the client
 * uses 15, which the 32 KiB window of gevws_inflate_ctx_async holds.  Any
 * other flag bit is GEVWS_ERR_INVALID. */
#define GEVWS_NEGOTIATE_CLIENT_TAKEOVER 1u
int gevws_deflate_negotiate_flags(const uint8_t *offer, uint64_t n, uint32_t flags, uint8_t *out, uint64_t cap,
                                  uint64_t *out_len, uint8_t *conn_ext);

/* The deflate step: outbound messages compressed on the device, and the
 * gevws_out_frame records gevws_encode_batch_async frames them from.
 * Additions to ABI version 3: nothing above changes.
 *
 * Input.  d_msgs[i] is one message to send: its plain bytes are
 * d_src[payload_off, payload_off + length).  d_src has GEVWS_IN_PAD readable
 * bytes past src_bytes and is read as whole 16-byte vectors, but only `length`
 * bytes count.  The messages are the first max_msgs records, or with d_prev
 * the first min(d_prev->frames, max_msgs), none when d_prev->status < 0 (read
 * on the device, as gevws_dispatch_decoded_async reads d_decoded).  No
 * messages give a zero summary and read none of the inputs.
 *
 * Payload (RFC 7692 section 7.2.1).  A raw DEFLATE stream (RFC 1951) of
 * blocks with BFINAL 0, closed by an empty stored block whose last four bytes
 * 00 00 ff ff are taken off; an empty message is the single byte 00.  Blocks
 * are fixed-Huffman (BTYPE 01) with LZ77 matches of length 3..258, or stored
 * (BTYPE 00) wherever that is smaller; no dynamic codes unless the call asks
 * for them (GEVWS_DEFLATE_DYNAMIC below).  No match distance
 * exceeds 2^window_bits (0 stands for 15), so an answer that carried
 * server_max_window_bits=N is honoured with window_bits = N.  Every message
 * starts from an empty window: server_no_context_takeover, which
 * gevws_deflate_negotiate puts into every answer.  The bytes are valid
 * DEFLATE, not zlib's; they depend only on the message's bytes and its
 * window_bits -- not on its place in the batch, its neighbours, the pad
 * behind it or the grid -- and gevws_deflate_raw gives the same bytes.
 *
 * Output.  d_out_frames[i] = {hdr = {fin 1, rsv 4 (RSV1), opcode, masked 0,
 * mask 0, length c}, payload_off, payload_len c} with c the compressed
 * length; the payloads lie in d_out in message order, each on a
 * GEVWS_PAYLOAD_ALIGN boundary, the pad behind each zeroed.  d_out needs
 * GEVWS_OUT_PAD writable bytes past out_cap; it is then gevws_encode_batch_async's
 * d_payload as it stands.  With GEVWS_DEFLATE_PLAIN_IF_NOT_SMALLER in `flags`
 * a message with c >= length goes out plain: rsv 0, its bytes verbatim (RFC
 * 7692 section 6 leaves the choice to the sender, message by message).
 *
 * GEVWS_DEFLATE_DYNAMIC in `flags`.  Every 4 KiB of input (a run) becomes a
 * stored, fixed or dynamic-Huffman block (BTYPE 10), whichever ends at the
 * lowest bit; on a tie stored wins, then fixed.  The matches, the runs and
 * window_bits are as without the flag: a run's tokens are the same, only
 * their coding differs, and all three ends are known before a bit is written.
 * A stored or fixed block ends no later the earlier it starts, so a payload
 * with the flag is never longer than without it; gevws_deflate_bound holds
 * unchanged, and GEVWS_DEFLATE_PLAIN_IF_NOT_SMALLER compares against the
 * length with dynamic blocks.  A dynamic block's code comes from the run's
 * counts of the 286 literal / length symbols (end-of-block once) and the 30
 * distance symbols: code lengths of at most 15 bits, canonical codes (RFC 1951
 * section 3.2.2), HLIT / HDIST / HCLEN trimmed, the lengths run-length coded
 * with 16 / 17 / 18 (literal / length and distance lengths apart), the
 * code-length code of at most 7 bits.  A run without a match sends one
 * distance code of one bit.  The construction is one integer function of the
 * counts, ties broken by symbol index, shared by the device and
 * gevws_deflate_raw_flags.  Without the flag every byte is as before.
 *
 * d_summary: frames = records written, payload_bytes = bytes of d_out used,
 * payload_len = the sum of the wire payload lengths, errors 0.  status
 * GEVWS_ERR_CAPACITY when out_cap is too small: payload_bytes then holds the
 * need and nothing else is written, so the caller retries.  status
 * GEVWS_ERR_INVALID when a record is malformed -- an opcode other than 1 / 2,
 * window_bits outside {0, 8..15}, payload_off not on GEVWS_PAYLOAD_ALIGN, a
 * range outside d_src[0, src_bytes), a length above 2^32 - 1: errors then
 * counts such records, the other fields are zero and nothing else is written. */
#define GEVWS_DEFLATE_PLAIN_IF_NOT_SMALLER 1u     /* call flag */
#define GEVWS_DEFLATE_DYNAMIC 2u                  /* call flag: dynamic-Huffman blocks where they are smaller */
typedef struct gevws_deflate_msg {   /* 24 bytes: one message to send */
    uint64_t payload_off;   /* into d_src, a multiple of GEVWS_PAYLOAD_ALIGN */
    uint64_t length;        /* plain bytes, <= 2^32 - 1 */
    uint8_t opcode;         /* 1 text, 2 binary */
    uint8_t window_bits;    /* 0 = 15; else 8..15: the negotiated server_max_window_bits */
    uint8_t reserved[6];    /* zero */
} gevws_deflate_msg;

/* The most bytes a message of n plain bytes can become:
 * n + 5 * ceil(n / 4096) + 1 <= n + n / 512 + 16 (a stored block costs at
 * most 5 bytes, and the compressor decides per 4 KiB of input). */
uint64_t gevws_deflate_bound(uint64_t n);

int gevws_deflate_async(gevws_ctx *ctx, void *stream,
                        const gevws_deflate_msg *d_msgs, uint64_t max_msgs,
                        const gevws_summary *d_prev /* may be NULL */,
                        const uint8_t *d_src, uint64_t src_bytes, uint32_t flags,
                        gevws_out_frame *d_out_frames, uint8_t *d_out, uint64_t out_cap,
                        gevws_summary *d_summary);

/* The same compressor on host memory: in[0, n) is one message, window_bits as
 * in gevws_deflate_msg, out[0, cap) receives the payload the device would
 * write for it, byte for byte.  Returns GEVWS_OK; GEVWS_ERR_CAPACITY when the
 * payload does not fit (*out_len = the need, out untouched); GEVWS_ERR_INVALID
 * for a NULL buffer, n above 2^32 - 1 or a window_bits outside {0, 8..15}.
 * *out_len = the payload's length. */
int gevws_deflate_raw(const uint8_t *in, uint64_t n, int window_bits,
                      uint8_t *out, uint64_t cap, uint64_t *out_len);

/* gevws_deflate_raw with the call's flags: GEVWS_DEFLATE_DYNAMIC gives the
 * payload gevws_deflate_async writes with that flag, 0 is gevws_deflate_raw
 * bit for bit; any other bit (GEVWS_DEFLATE_PLAIN_IF_NOT_SMALLER too: the
 * caller compares *out_len with n) is GEVWS_ERR_INVALID. */
int gevws_deflate_raw_flags(const uint8_t *in, uint64_t n, int window_bits, uint32_t flags,
                            uint8_t *out, uint64_t cap, uint64_t *out_len);

/* Server context takeover: the deflate step with a window and a hash table
 * per connection, kept between messages and between calls.  Additions to ABI
 * version 3: nothing above changes.
 *
 * GEVWS_EXT_SERVER_TAKEOVER is a third bit of the d_conn_ext byte, set beside
 * GEVWS_EXT_DEFLATE for a connection whose answer left
 * server_no_context_takeover out (gevws_deflate_negotiate_takeover says when).
 * The message pass masks the byte with GEVWS_EXT_DEFLATE and the inflate step
 * tests GEVWS_EXT_CLIENT_TAKEOVER only: neither sees the new bit.
 *
 * The slot.  d_def_ctx is a caller-owned device buffer of n_conns slots of
 * GEVWS_DEF_CTX_BYTES each, on a 16-byte boundary; connection c's is slot c.
 * All-zero is a fresh connection.  Callers treat a slot as opaque; its layout
 * is a 64-byte head -- uint64 total (little-endian: the plain bytes of the
 * connection's compressed messages so far), zeros --, behind it the ring
 * image: stream byte i sits at ring[i & 32767] for the last min(total, 32 768)
 * stream bytes, bytes never written stay zero; and behind that the compressor's
 * hash table, 4 096 slots of 16 bits (little-endian), as the connection's
 * last step left it.  A slot's content is a function of the connection's
 * sequence of compressed messages (their bytes and window_bits; the call's
 * GEVWS_DEFLATE_DYNAMIC does not change it: the tokens are the same) -- not
 * of how the messages were cut into calls, the batch around
 * them, the grid or the pad bytes behind a message in d_src -- and
 * gevws_deflate_raw_ctx produces the same bytes on the host.  Behaviour
 * depends on `total` only through min(total, 32 768) and total mod 65 536 (the
 * table holds positions mod 65 536): a connection that has sent 2^32 or 2^62
 * bytes is served as one that has sent 70 000 (the tests relocate slots across
 * those positions).  41 024 bytes a
 * connection: 672 MB of device memory for 16 384 connections.
 *
 * gevws_deflate_ctx_async is gevws_deflate_async plus d_msg_conn (one
 * connection index per message), d_conn_ext (one byte per connection),
 * d_def_ctx and n_conns.
 *   - With any of the three pointers NULL it is gevws_deflate_async bit for
 *     bit (which is that NULL call).
 *   - A connection without GEVWS_EXT_SERVER_TAKEOVER is compressed as above;
 *     its slot is neither read nor written.
 *   - A takeover connection's message k gets the payload the compressor gives
 *     for its bytes with the connection's earlier compressed messages --
 *     earlier in this call's list and in earlier calls -- as history: a match
 *     may reach back min(2^window_bits, 30 720) bytes across the message's
 *     first byte.  The payload is still section 7.2.1's form: blocks with
 *     BFINAL 0, then the empty stored block with its 00 00 ff ff taken off.
 *     An empty message is the byte 00 and leaves the slot as it was.
 *   - A peer that feeds payload + 00 00 ff ff of each message in order to one
 *     raw inflater with a window of 2^window_bits gets the messages back.
 *   - The messages of a takeover connection must stand next to each other in
 *     the list, as one run of equal d_msg_conn: the wave of the run's first
 *     message compresses the run in order, in both passes.  A takeover
 *     connection that appears in two separate runs makes the call
 *     GEVWS_ERR_INVALID on the device (every run but one counts once in
 *     `errors`): two waves would race on one slot.
 *   - GEVWS_DEFLATE_PLAIN_IF_NOT_SMALLER does not apply to a takeover
 *     connection's messages: they always go out compressed, RSV1 set (a
 *     message sent plain would have to stay out of the peer's window).
 *     gevws_deflate_bound still holds, a run can always be a stored block.
 *     The flag works as before for the other connections of the call.
 *   - GEVWS_DEFLATE_DYNAMIC works with contexts: a run's tokens are the same,
 *     only their coding differs.
 *   - With d_prev a chain ends at the gated count: messages past it are not
 *     compressed and do not enter the window.
 *   - d_msg_conn[i] >= n_conns, or a malformed record (of any connection), is
 *     GEVWS_ERR_INVALID: `errors` counts the records, nothing else is written,
 *     no slot is written and none is indexed by such a record.
 *   - GEVWS_ERR_CAPACITY writes nothing: the slots are untouched byte for
 *     byte, so the retry sees the same contexts.
 *   - With contexts max_msgs is at most 0x7FF00000 (the grid is rounded up to
 *     a multiple of 1 024 workgroups). */
#define GEVWS_EXT_SERVER_TAKEOVER 4u
#define GEVWS_DEF_CTX_BYTES (64u + 32768u + 8192u)
int gevws_deflate_ctx_async(gevws_ctx *ctx, void *stream,
                            const gevws_deflate_msg *d_msgs, uint64_t max_msgs,
                            const gevws_summary *d_prev /* may be NULL */,
                            const uint8_t *d_src, uint64_t src_bytes, uint32_t flags,
                            gevws_out_frame *d_out_frames, uint8_t *d_out, uint64_t out_cap,
                            gevws_summary *d_summary, const uint32_t *d_msg_conn,
                            const uint8_t *d_conn_ext, uint8_t *d_def_ctx, uint32_t n_conns);

/* gevws_deflate_raw_flags over one slot in host memory
 * (ctx[0, GEVWS_DEF_CTX_BYTES)): the message is compressed with the slot's
 * window behind it and appended to the slot.  A zeroed slot gives
 * gevws_deflate_raw_flags's bytes.  On GEVWS_ERR_CAPACITY out and the slot are
 * untouched (*out_len = the need).  A NULL ctx is GEVWS_ERR_INVALID. */
int gevws_deflate_raw_ctx(const uint8_t *in, uint64_t n, int window_bits, uint32_t flags,
                          uint8_t *out, uint64_t cap, uint64_t *out_len, uint8_t *ctx);

/* gevws_deflate_negotiate_flags for a server that may keep its own window
 * too.  `flags` may hold GEVWS_NEGOTIATE_CLIENT_TAKEOVER and
 * GEVWS_NEGOTIATE_SERVER_TAKEOVER; any other bit is GEVWS_ERR_INVALID.  With
 * flags 0 or 1 it writes gevws_deflate_negotiate_flags's answer byte for
 * byte.  With the server bit server_no_context_takeover is left out of the
 * answer and GEVWS_EXT_SERVER_TAKEOVER is set in *conn_ext, unless the chosen
 * offer carried the parameter: then it is echoed and the bit stays clear (RFC
 * 7692 section 7.1.1.1).  server_max_window_bits is echoed as above: it is
 * the window_bits the caller gives every message of that connection. */
#define GEVWS_NEGOTIATE_SERVER_TAKEOVER 2u
int gevws_deflate_negotiate_takeover(const uint8_t *offer, uint64_t n, uint32_t flags, uint8_t *out, uint64_t cap,
                                     uint64_t *out_len, uint8_t *conn_ext);

/* The join step and the reply step: one contiguous body per whole message,
 * and the bodies turned into the deflate step's message list and the
 * encoder's frame list on the device, so that decode -> messages -> inflate ->
 * join -> reply -> deflate -> encode is one stream-ordered chain.  Additions
 * to ABI version 3: nothing above changes.
 *
 * gevws_join_async stands behind the message pass (and, where there is one,
 * the inflate step) and works on their tables; d_bodies[m] belongs to
 * d_messages[m].
 *
 * Delivered.  A message is delivered (GEVWS_BODY_WHOLE) when it has both
 * GEVWS_MSG_BEGIN and GEVWS_MSG_END, its status is GEVWS_MSG_OK and, if it is
 * GEVWS_MSG_COMPRESSED, d_inflated is given and d_inflated[m] has
 * GEVWS_INF_DONE with status GEVWS_MSG_OK.  Every other message -- one still
 * open or continued from the carry state, a UTF-8 failure, a failed or
 * pending inflate, a compressed message with d_inflated == NULL -- gets flags
 * 0, off = length = 0 and its status copied (a compressed message's is the
 * inflate record's when d_inflated is given), and takes no space.
 *
 * Where the bytes are.  A delivered compressed message gets
 * GEVWS_BODY_INFLATED: off / length are the inflate record's and nothing is
 * copied.  A delivered plain message with nframes >= 2 is copied
 * (GEVWS_BODY_JOINED); with GEVWS_JOIN_ALL in `flags` every delivered plain
 * message is.  Any other delivered message stays where it is: off is its one
 * frame's payload_off in d_payload.
 *
 * What is copied.  The first hdr.length bytes of each of the message's data
 * frames in order -- the frames f from first_frame on with d_msg_of[f] == m;
 * control frames in between, empty fragments and the slots' padding are
 * skipped.  Source bytes are read as whole aligned 16-byte vectors, and only
 * vectors that hold at least one counted byte: the arena's last vector may be
 * a fragment's last.  d_payload and d_out start on a 16-byte boundary.
 *
 * Where it lands.  The copied bodies lie in d_out in message order, each on a
 * GEVWS_PAYLOAD_ALIGN boundary, the pad behind each zeroed; a zero-length body
 * takes no space (its off is where the next one starts).  They start at
 * `base`: d_inflate_summary->payload_bytes rounded up to 16 when that summary
 * is given, else 0.  out_cap is the capacity of the whole of d_out, the
 * inflate's part included: in the chained use d_out is the inflate's own
 * buffer, and no byte below `base` is written.  Every store is a whole vector
 * inside [base, payload_bytes).
 *
 * d_summary: frames = delivered bodies, payload_bytes = base + the bytes the
 * copied bodies take (the new end of d_out), payload_len = the sum of the
 * delivered lengths, errors 0; status GEVWS_ERR_CAPACITY when payload_bytes >
 * out_cap -- payload_bytes then holds the need and neither d_bodies nor d_out
 * is written, so the caller retries.  A failed d_msg_summary, no messages, or
 * a given d_inflate_summary whose status is not GEVWS_OK give a zero summary
 * and read none of the inputs.  Any flag bit but GEVWS_JOIN_ALL is
 * GEVWS_ERR_INVALID from the call; max_frames is at most 2^32 - 1.
 * A message that spans two passes stays undelivered by this call;
 * gevws_join_carry_async below keeps a plain one's bytes from pass to pass and
 * delivers it.  gevws_join_async is that function's NULL call. */
#define GEVWS_JOIN_ALL 1u          /* call flag: copy single-frame plain messages too */
#define GEVWS_BODY_WHOLE    1u     /* delivered: off / length are valid */
#define GEVWS_BODY_JOINED   2u     /* its bytes were written to d_out by this call */
#define GEVWS_BODY_INFLATED 4u     /* its bytes are the inflate step's, already in d_out */
typedef struct gevws_body {        /* 32 bytes; d_bodies[m] belongs to d_messages[m] */
    uint64_t off;      /* into d_out if JOINED or INFLATED, else into d_payload; on GEVWS_PAYLOAD_ALIGN */
    uint64_t length;
    uint32_t conn;
    uint8_t opcode;    /* 1 / 2, the message's */
    uint8_t flags;     /* GEVWS_BODY_*; 0 = not delivered (off = length = 0) */
    uint8_t status;    /* the message's status; for a compressed message the inflate's */
    uint8_t reserved[9];
} gevws_body;
int gevws_join_async(gevws_ctx *ctx, void *stream, const gevws_frame *d_frames, uint64_t max_frames,
                     const gevws_message *d_messages, uint64_t max_messages, const int64_t *d_msg_of,
                     const gevws_summary *d_msg_summary, const uint8_t *d_payload,
                     const gevws_inflated *d_inflated /* may be NULL */,
                     const gevws_summary *d_inflate_summary /* may be NULL */, uint32_t flags,
                     gevws_body *d_bodies, uint8_t *d_out, uint64_t out_cap, gevws_summary *d_summary);

/* gevws_join_carry_async is gevws_join_async plus a second carry beside
 * gevws_msg_state: the bytes of each connection's open plain message, kept on
 * the device between passes, so that a message whose frames arrive over
 * several passes is delivered with the pass that holds its FIN frame.
 * Additions to ABI version 3: nothing above changes.
 *
 * The carry is a ping-pong between two caller-owned arenas: the (d_carry_out,
 * d_carry_dst) of one pass are the (d_carry_in, d_carry_src) of the next, with
 * the carry summary's payload_bytes as carry_src_bytes.  d_carry_dst overlaps
 * neither d_carry_src nor d_out.  Records and arenas are indexed by the
 * batch's connection index, as d_state and the takeover slots are.  Both
 * arenas start on a 16-byte boundary and are read and written as whole 16-byte
 * vectors (so they are allocated in whole vectors).
 *
 * NULL call.  With d_conn_msg, d_carry_out, d_carry_dst or d_carry_summary
 * NULL the call is gevws_join_async, bit for bit, and looks at none of the
 * other added arguments.
 *
 * Otherwise, with ci = d_carry_in[c] (all-zero when d_carry_in is NULL):
 *
 * Continued message (body side).  A message without GEVWS_MSG_BEGIN and
 * without GEVWS_MSG_COMPRESSED is its connection's first, continued from the
 * state.  The rule looks at the message alone, like every body's: an error
 * later in the same batch does not take a finished message back.
 *   - ci OPEN: its whole body is the carried bytes followed by its data
 *     frames' bytes (counted as above).  With GEVWS_MSG_END, status OK and a
 *     total <= max_message_bytes it is delivered WHOLE | JOINED, with or
 *     without GEVWS_JOIN_ALL, in d_out in message order like every copied
 *     body; length is the total.  With END and status OK but over the limit it
 *     is not delivered and its body status is GEVWS_MSG_ERR_TOO_BIG.  Without
 *     END, or with a failed status, it is undelivered as above.
 *   - ci LOST: not delivered; its body status is ci.status when that is
 *     nonzero, else the message's.
 *   - ci zero: undelivered exactly as in gevws_join_async.
 * d_summary counts continued deliveries like any other delivered body; its
 * errors stay 0.
 *
 * d_carry_out[c] (carry side), for a connection with d_conn_msg[c].error == 0:
 *   - Message still open: the connection's last message has no END.  A plain
 *     message that began in this batch becomes OPEN with its fragments' bytes;
 *     one that continues an OPEN ci becomes OPEN with the carried bytes
 *     followed by this batch's fragments.  Over max_message_bytes it becomes
 *     LOST with status GEVWS_MSG_ERR_TOO_BIG instead.  A compressed message
 *     that began in this batch becomes LOST with status 0; a continuation of a
 *     LOST ci becomes LOST with ci.status, of a zero ci LOST with status 0.
 *     (gevws_join_carry_ext_async below keeps them instead.)
 *   - No message in this batch (nmessages == 0: idle, control frames only,
 *     decode status < 0): the record moves forward unchanged in meaning -- an
 *     OPEN one's bytes are copied to d_carry_dst (the limit applies), a LOST
 *     one stays LOST with its opcode and status, a zero one stays zero.
 *   - Otherwise all-zero.  So a LOST record lasts until that message's END and
 *     no longer; the connection's next message is carried and delivered
 *     normally.
 * A connection with d_conn_msg[c].error != 0 gets an all-zero record: its
 * carry is dropped, and the caller closes it.  An OPEN record has off / length
 * / opcode, a LOST one opcode and status; every other field is zero.
 *
 * Layout of d_carry_dst.  OPEN bodies lie in connection order, each on a
 * 16-byte boundary, the pad behind each zeroed; a zero-length body takes no
 * space.  Every store is a whole vector inside [0, payload_bytes).
 *
 * d_carry_summary: frames = OPEN records written, payload_bytes = bytes of
 * d_carry_dst used, payload_len = the sum of their lengths, errors = bodies
 * and carries that became GEVWS_MSG_ERR_TOO_BIG in this call.
 *
 * Capacity.  payload_bytes > out_cap, or > carry_cap on the carry side, sets
 * GEVWS_ERR_CAPACITY in the summary concerned, with the need in it; the other
 * summary keeps its figures.  Then none of d_bodies, d_out, d_carry_out and
 * d_carry_dst is written.  The caller retries with the same inputs: the `in`
 * side is never written.
 *
 * Gates.  A failed d_msg_summary, or a given failed d_inflate_summary, copies
 * its status into both summaries (other fields 0); nothing else is written and
 * the caller keeps the old carry.  n_conns == 0 gives two zero summaries.
 * Zero messages with status OK is no gate for the carry side: the carries move
 * forward, and the body side gives a zero summary (max_messages == 0 too; the
 * message tables may then be NULL).
 *
 * Malformed input, checked before anything is indexed by it: a message with
 * conn >= n_conns; an OPEN input record with off % 16 != 0 or off + length >
 * carry_src_bytes; a d_conn_msg[c] whose messages do not lie inside the
 * message table.  Both summaries then get GEVWS_ERR_INVALID with `errors`
 * counting such records (a connection once), the other fields zero, and
 * nothing else is written.  max_message_bytes outside 1 .. 2^32 - 1, an
 * unknown flag bit, or an arena off its 16-byte boundary is GEVWS_ERR_INVALID
 * from the call. */
#define GEVWS_CARRY_OPEN 1u   /* off / length: the open message's bytes so far (plain, unless COMPRESSED below) */
#define GEVWS_CARRY_LOST 2u   /* a message is open but its bytes are not kept; status says why */
typedef struct gevws_carry {  /* 32 bytes per connection; all-zero = no message open */
    uint64_t off;      /* into the carry arena, on GEVWS_PAYLOAD_ALIGN */
    uint64_t length;   /* may be 0 with OPEN: opened by an empty fragment */
    uint8_t opcode;    /* 1 / 2 */
    uint8_t flags;     /* GEVWS_CARRY_* */
    uint8_t status;    /* LOST: GEVWS_MSG_ERR_TOO_BIG, or GEVWS_MSG_OK (compressed, or nothing carried in) */
    uint8_t reserved[13];
} gevws_carry;
int gevws_join_carry_async(gevws_ctx *ctx, void *stream, const gevws_frame *d_frames, uint64_t max_frames,
                           const gevws_message *d_messages, uint64_t max_messages, const int64_t *d_msg_of,
                           const gevws_summary *d_msg_summary, const uint8_t *d_payload,
                           const gevws_inflated *d_inflated /* may be NULL */,
                           const gevws_summary *d_inflate_summary /* may be NULL */, uint32_t flags,
                           gevws_body *d_bodies, uint8_t *d_out, uint64_t out_cap, gevws_summary *d_summary,
                           const gevws_conn_msg *d_conn_msg, uint32_t n_conns,
                           uint64_t max_message_bytes /* 1 .. 2^32-1 */,
                           const gevws_carry *d_carry_in /* may be NULL: every connection fresh */,
                           const uint8_t *d_carry_src, uint64_t carry_src_bytes,
                           gevws_carry *d_carry_out, uint8_t *d_carry_dst, uint64_t carry_cap,
                           gevws_summary *d_carry_summary);

/* Compressed messages that span passes: the carry keeps an open
 * permessage-deflate message's compressed bytes, and the inflate of the pass
 * that holds its FIN frame reads them as the front of its stream.  Nothing of
 * the decoder's state survives a pass.  Additions to ABI version 3: nothing
 * above changes.
 *
 * GEVWS_CARRY_COMPRESSED is a third bit of gevws_carry.flags, set beside
 * GEVWS_CARRY_OPEN: off / length are then the compressed payload bytes so far
 * (the tail 00 00 ff ff is never stored).  GEVWS_CARRY_KEEP_COMPRESSED is a bit
 * of carry_flags.
 *
 * gevws_join_carry_ext_async is gevws_join_carry_async plus carry_flags, and
 * gevws_join_carry_async is its carry_flags == 0 call, bit for bit (the
 * COMPRESSED bit of an input record is then not looked at).  Any other bit of
 * carry_flags is GEVWS_ERR_INVALID from the call; the bits of `flags` stay as
 * they are.  With GEVWS_CARRY_KEEP_COMPRESSED:
 *
 * d_carry_out[c] (carry side), where the connection's last message has
 * GEVWS_MSG_COMPRESSED and no END:
 *   - it began in this batch: OPEN | COMPRESSED with its data frames' bytes;
 *   - it continues an OPEN | COMPRESSED ci: OPEN | COMPRESSED with the carried
 *     bytes followed by this batch's fragments;
 *   - it continues a zero or LOST ci: LOST, as above;
 *   - it continues an OPEN ci without COMPRESSED (the caller mixed up its
 *     states): LOST with status 0.  So does a plain message without END that
 *     continues an OPEN | COMPRESSED ci.
 * max_message_bytes bounds the compressed bytes kept: over it the record is
 * LOST with GEVWS_MSG_ERR_TOO_BIG and counted in d_carry_summary.errors, like
 * a plain message.  The idle forward (nmessages == 0) keeps the bit and copies
 * the bytes.
 *
 * Continued message (body side).  A message with COMPRESSED and END and
 * without BEGIN is delivered WHOLE | INFLATED exactly when d_inflated[m] has
 * GEVWS_INF_DONE and status OK (gevws_inflate_carry_async below); off and
 * length are the inflate record's.  Otherwise it is undelivered with the
 * inflate record's status (without d_inflated: the message's).  The join
 * copies nothing of it.  A plain continued message over an OPEN | COMPRESSED
 * ci is undelivered, as over a zero one.
 *
 * Everything else -- layout, summaries, capacity, gates, malformed input -- is
 * as above, with the new bit allowed in an input record.
 *
 * gevws_inflate_carry_async is gevws_inflate_ctx_async plus d_carry_in,
 * d_carry_src and carry_src_bytes: the same `in` side the pass's join reads
 * afterwards.  The inflate only reads it.  With d_carry_in or d_carry_src NULL
 * it is gevws_inflate_ctx_async bit for bit (which is that NULL call).
 * Otherwise n_conns is required, with or without contexts (d_conn_ext or
 * d_inf_ctx NULL: no connection has takeover), and with ci =
 * d_carry_in[msg.conn] a compressed message without BEGIN, with END and with
 * message status OK is:
 *   - ci OPEN | COMPRESSED: whole.  Its stream S is the ci.length carried
 *     bytes, then its data frames' bytes as above, then 00 00 ff ff.  Verdict,
 *     bytes, max_message_bytes (which bounds the inflated output), the UTF-8
 *     pass, d_state.failed and the summary are what one pass that holds the
 *     whole message gives.  On a takeover connection it is the first link of
 *     the chain and the chain goes on behind it, so a slot stays a function of
 *     the connection's stream alone, for cuts inside a message too.
 *   - ci LOST with a nonzero status: GEVWS_INF_DONE, that status, length 0.  It
 *     takes no space and counts in `errors`; on a takeover connection it loses
 *     the context, as a failed message does.
 *   - anything else (ci zero, LOST with status 0, OPEN without COMPRESSED):
 *     GEVWS_INF_PENDING; it stops the chain, as above.
 * Messages without END are PENDING as above.
 *
 * Malformed input makes the call GEVWS_ERR_INVALID on the device, as a record
 * with conn >= n_conns does in gevws_inflate_ctx_async: a message record with
 * conn >= n_conns (counted a record), and an OPEN input record of a connection
 * that has a message in the batch with off % 16 != 0 or off + length >
 * carry_src_bytes (counted a connection).  d_summary gets the status and the
 * count in `errors`; nothing else is written, no slot is touched, and no
 * address is formed from such a field.  GEVWS_ERR_CAPACITY is as above: nothing
 * is written, the slots are untouched byte for byte, and the retry uses the
 * same inputs.  d_carry_src starts on a 16-byte boundary and is read as whole
 * vectors inside a record's [off, off + length) rounded down to 16, its last
 * ragged bytes one by one; with a carry max_messages is at most 0x7FF00000. */
#define GEVWS_CARRY_COMPRESSED 4u        /* gevws_carry.flags, beside OPEN: the bytes are compressed payload */
#define GEVWS_CARRY_KEEP_COMPRESSED 1u   /* carry_flags */
int gevws_join_carry_ext_async(gevws_ctx *ctx, void *stream, const gevws_frame *d_frames, uint64_t max_frames,
                               const gevws_message *d_messages, uint64_t max_messages, const int64_t *d_msg_of,
                               const gevws_summary *d_msg_summary, const uint8_t *d_payload,
                               const gevws_inflated *d_inflated /* may be NULL */,
                               const gevws_summary *d_inflate_summary /* may be NULL */, uint32_t flags,
                               gevws_body *d_bodies, uint8_t *d_out, uint64_t out_cap, gevws_summary *d_summary,
                               const gevws_conn_msg *d_conn_msg, uint32_t n_conns,
                               uint64_t max_message_bytes /* 1 .. 2^32-1 */,
                               const gevws_carry *d_carry_in /* may be NULL: every connection fresh */,
                               const uint8_t *d_carry_src, uint64_t carry_src_bytes,
                               gevws_carry *d_carry_out, uint8_t *d_carry_dst, uint64_t carry_cap,
                               gevws_summary *d_carry_summary, uint32_t carry_flags);
int gevws_inflate_carry_async(gevws_ctx *ctx, void *stream, const gevws_frame *d_frames, uint64_t max_frames,
                              const gevws_message *d_messages, uint64_t max_messages, const int64_t *d_msg_of,
                              const gevws_summary *d_msg_summary, const uint8_t *d_payload,
                              uint64_t max_message_bytes, gevws_msg_state *d_state /* may be NULL */,
                              gevws_inflated *d_inflated, uint8_t *d_out, uint64_t out_cap, gevws_summary *d_summary,
                              const uint8_t *d_conn_ext, uint8_t *d_inf_ctx, uint32_t n_conns,
                              const gevws_carry *d_carry_in, const uint8_t *d_carry_src, uint64_t carry_src_bytes);

/* gevws_reply_bodies_async is the message-level stand-in for the user's
 * handler, as gevws_dispatch_async's policy is at frame level: with
 * GEVWS_HANDLER_ECHO_BINARY (opcode 2) or GEVWS_HANDLER_ECHO_TEXT (opcode 1)
 * every delivered body gets one reply, in message order -- an empty message
 * too (compressed, it is the byte 00); GEVWS_HANDLER_NONE gives no replies and
 * looks at no record; any other policy is GEVWS_ERR_INVALID from the call.
 *
 * The bodies are the first min(d_msg_summary->frames, max_messages) records;
 * a failed d_msg_summary or d_join_summary gives two zero summaries and
 * writes nothing else.
 *   - The deflate list, for connections whose d_conn_ext byte has
 *     GEVWS_EXT_DEFLATE: d_def_msgs[k] = {body.off, body.length, opcode, the
 *     connection's d_conn_window_bits byte (0 when that is NULL; passed through
 *     unchecked, the deflate step rejects a bad one)}, d_def_conn[k] = the
 *     connection.  d_def_summary->frames is the count: the summary is the
 *     d_prev of gevws_deflate_ctx_async, with the join's d_out as d_src.  The
 *     list keeps the message order, which is by connection, so a connection's
 *     messages form one run of equal d_def_conn, as takeover requires.
 *   - The plain list, for every other connection (d_conn_ext == NULL: all):
 *     d_plain[k] = {hdr = {fin 1, rsv 0, opcode, masked 0, mask 0, length},
 *     payload_off = body.off, payload_len = length}, d_plain_conn[k] = the
 *     connection.  d_plain_summary->frames is the count: the summary is the
 *     d_dispatched of gevws_encode_replies_async, with the join's d_out as
 *     d_payload.
 *   - d_reply_of[m], for each of the bodies, = the index in its connection's
 *     list, or -1.
 *   - The two summaries' other fields are zero.  All five arrays hold
 *     max_messages entries.
 *   - Both lists address one arena, so a delivered body with neither
 *     GEVWS_BODY_JOINED nor GEVWS_BODY_INFLATED (a join without
 *     GEVWS_JOIN_ALL) is malformed, and so is conn >= n_conns: both summaries
 *     then get GEVWS_ERR_INVALID with `errors` counting such records, the
 *     other fields zero, and nothing else is written. */
int gevws_reply_bodies_async(gevws_ctx *ctx, void *stream, const gevws_body *d_bodies, uint64_t max_messages,
                             const gevws_summary *d_msg_summary, const gevws_summary *d_join_summary, int policy,
                             const uint8_t *d_conn_ext /* may be NULL */,
                             const uint8_t *d_conn_window_bits /* may be NULL: 0 */, uint32_t n_conns,
                             gevws_deflate_msg *d_def_msgs, uint32_t *d_def_conn, gevws_summary *d_def_summary,
                             gevws_out_frame *d_plain, uint32_t *d_plain_conn, gevws_summary *d_plain_summary,
                             int64_t *d_reply_of);

/* The control step and the send plan: the message chain answers every frame
 * a peer may send, closes a connection that failed a check, and states what
 * is written to each socket and in which order.  Additions to ABI version 3:
 * nothing above changes.  The chain of one pass is
 *   decode -> messages -> inflate -> join -> control -> reply -> deflate ->
 *   encode (plain list) -> encode (deflate records) -> encode (d_ctl) -> plan.
 *
 * gevws_control_async stands behind the join and before
 * gevws_reply_bodies_async.  d_frames / max_frames / d_conn_out / n_conns /
 * d_decoded / d_payload are the decode's, aux_off / aux_cap an aux region of
 * d_payload as in gevws_dispatch_async (GEVWS_AUX_SLOT bytes a slot); d_msg_of /
 * d_messages / max_messages / d_conn_msg / d_msg_summary the message pass's;
 * d_bodies / d_join_summary the join's.  The frames are the first
 * min(d_decoded->frames, max_frames), the messages the first
 * min(d_msg_summary->frames, max_messages).
 *
 * The cut.  A connection's cut is its first frame, in stream order, that is
 *   (a) a close frame (opcode 8);
 *   (b) d_conn_msg[c].error_frame, when d_conn_msg[c].error is 1..6;
 *   (c) the last data frame in this batch of the connection's first message
 *       whose d_bodies record has status != GEVWS_MSG_OK (GEVWS_MSG_ERR_UTF8
 *       found after inflating, GEVWS_MSG_ERR_DEFLATE, GEVWS_MSG_ERR_TOO_BIG).
 * A frame that is both (a) and (b) -- a close frame that fails a frame check --
 * counts as (b).  A connection that comes in failed (error != 0 with
 * error_frame == UINT64_MAX), one with d_conn_out[c].status < 0 and one without
 * frames have no cut and yield nothing: the host deals with them.
 *
 * Control replies: gevws_out_frame records in d_ctl over d_payload and its aux
 * region (ready for gevws_encode_replies_async with d_summary as d_dispatched
 * and the same d_payload), in frame order, from the frames up to and including
 * the cut; every frame behind the cut is ignored.
 *   - A ping gives a pong with the frame's payload in place.
 *   - A pong gives a ping (util.go:54-56, as gevws_dispatch_async does) unless
 *     GEVWS_CONTROL_NO_PING_FOR_PONG is set in `flags` (RFC 6455 section 5.5.3:
 *     a pong needs no answer).
 *   - A close frame -- the cut of kind (a) -- gives exactly the reply
 *     gevws_dispatch_async gives (util.HandleClose; one code serves both).
 *   - A cut of kind (b) or (c) gives the close of a failed connection: fin,
 *     opcode 8, a 2-byte body in an aux slot (the code, no reason).  The code
 *     is 1002 (protocol error) for errors 1-5, 1007 (invalid payload data) for
 *     GEVWS_MSG_ERR_UTF8 and GEVWS_MSG_ERR_DEFLATE, 1009 (message too big) for
 *     GEVWS_MSG_ERR_TOO_BIG, 1002 for any other status.  RFC 7692 names no code
 *     for a stream that does not inflate; 1007 is this library's choice.
 * Only the bytes of a body are written to its slot.
 *
 * Behind the cut.  Every message of the connection whose last data frame in
 * this batch lies behind the cut loses its body: d_bodies[m] gets off = length
 * = flags = 0 and status GEVWS_MSG_ERR_CLOSED (conn and opcode stay), so the
 * reply step builds no reply for it and a takeover window sees only what is
 * sent.  A message whose last data frame lies before the cut, or is the cut
 * (the failed message itself, already undelivered), keeps its record.
 *
 * Tables.  d_ctl and d_ctl_conn hold max_frames entries: d_ctl_conn[k] is the
 * connection of reply k.  d_ctl_of[f], for each of the frames, = the reply of
 * frame f or -1 (gevws_dispatch_async's d_reply_of).  d_msg_end[m], for each of
 * the messages, = the record index of its last data frame when it has
 * GEVWS_MSG_END, else UINT64_MAX.  d_conn_ctl[c], for every connection:
 * cut_frame (UINT64_MAX: none), close_code (0 unless GEVWS_CTL_FAILED) and
 * flags -- GEVWS_CTL_SHUTDOWN for any cut (the reference's ShutdownWrite,
 * wrap.go:52-56: the host sends what the plan lists and then stops feeding the
 * connection), GEVWS_CTL_FAILED beside it for kinds (b) and (c).
 *
 * d_summary: frames = control replies, payload_bytes = aux slots used, errors
 * = connections shut down.
 *   - GEVWS_ERR_CAPACITY when the slots do not fit in aux_cap: the counts are
 *     the need, and nothing but the summary is written -- d_bodies and every
 *     table stay byte for byte, so the caller retries.
 *   - A failed d_msg_summary or d_join_summary, no decoded frames or a failed
 *     d_decoded, n_conns == 0 or max_frames == 0 give a zero summary; nothing
 *     else is read or written.
 *   - A d_msg_of entry outside the message table (not -1 and not below the
 *     message count), or an error_frame (with error 1..6, not UINT64_MAX)
 *     outside its connection's frames, makes the call GEVWS_ERR_INVALID on the
 *     device: `errors` counts such connections, the other fields are zero and
 *     nothing else is written.  The check runs before anything is indexed by
 *     such a value.
 *   - Any flag bit but GEVWS_CONTROL_NO_PING_FOR_PONG is GEVWS_ERR_INVALID from
 *     the call; max_frames and max_messages are at most 2^32 - 1. */
enum { GEVWS_MSG_ERR_CLOSED = 9 };   /* continues the GEVWS_MSG_* enum: gevws_body.status behind a cut */
#define GEVWS_CONTROL_NO_PING_FOR_PONG 1u   /* call flag */
#define GEVWS_CTL_SHUTDOWN 1u   /* gevws_conn_ctl.flags: the connection has a cut */
#define GEVWS_CTL_FAILED   2u   /* beside it: the cut is a failure, close_code was sent */
typedef struct gevws_conn_ctl {   /* 32 bytes per connection */
    uint64_t cut_frame;     /* record index, or UINT64_MAX */
    uint32_t close_code;    /* 1002 / 1007 / 1009 with GEVWS_CTL_FAILED, else 0 */
    uint32_t flags;         /* GEVWS_CTL_* */
    uint64_t reserved[2];
} gevws_conn_ctl;
int gevws_control_async(gevws_ctx *ctx, void *stream, const gevws_frame *d_frames, uint64_t max_frames,
                        const gevws_conn_out *d_conn_out, uint32_t n_conns, const gevws_summary *d_decoded,
                        uint8_t *d_payload, uint64_t aux_off, uint64_t aux_cap, const int64_t *d_msg_of,
                        const gevws_message *d_messages, uint64_t max_messages, const gevws_conn_msg *d_conn_msg,
                        const gevws_summary *d_msg_summary, gevws_body *d_bodies,
                        const gevws_summary *d_join_summary, uint32_t flags, gevws_out_frame *d_ctl,
                        uint32_t *d_ctl_conn, int64_t *d_ctl_of, uint64_t *d_msg_end, gevws_conn_ctl *d_conn_ctl,
                        gevws_summary *d_summary);

/* gevws_send_plan_async runs last, behind the three encodes
 * (gevws_encode_replies_async of the reply step's plain list over the join's
 * arena, of the deflate step's records over its d_out, and of d_ctl over the
 * decode's payload arena).  Each wire comes with its d_out_off table and its
 * encode summary: `frames` is the list's count, `payload_bytes` the wire total.
 *
 * A frame triggers at most one reply:
 *   - its control reply, when d_ctl_of[f] >= 0 (wire 2);
 *   - otherwise the reply to message m = d_msg_of[f], when d_msg_end[m] == f
 *     and d_reply_of[m] >= 0: in the deflated wire (1) when the frame's
 *     connection has GEVWS_EXT_DEFLATE in its d_conn_ext byte, else in the
 *     plain wire (0; d_conn_ext == NULL: always).
 * The frame's connection is the one whose d_conn_out range holds it.  Records
 * are ordered by connection, then stream order, so the triggered replies in
 * frame order are the send order: a pong stands before the reply to the
 * message whose fragments surround the ping.
 *
 * d_send[k] (max_sends entries): reply k's bytes are wire[off, off + len) of
 * wire `wire` -- off from that wire's table, len up to the next entry's offset
 * or, for the list's last, the wire total -- triggered by `frame` of `conn`.
 * d_conn_send[c], for every connection: its entries are d_send[first, first +
 * count), `bytes` the sum of their len, `flags` d_conn_ctl[c].flags.
 * d_summary: frames = entries, payload_bytes = the sum of len, errors =
 * connections with GEVWS_CTL_SHUTDOWN.
 *   - GEVWS_ERR_CAPACITY when there are more entries than max_sends: frames
 *     holds the need and nothing else is written.
 *   - A failed d_decoded, d_msg_summary, d_join_summary, d_ctl_summary or
 *     encode summary, no decoded frames, n_conns == 0 or max_frames == 0 give
 *     a zero summary; nothing else is read or written.
 *   - A reply index outside its list's count, a d_msg_of entry outside the
 *     message table, a triggering frame that belongs to no connection or a
 *     table that decreases makes the call GEVWS_ERR_INVALID on the device:
 *     `errors` counts such frames, the other fields are zero and nothing else
 *     is written.  Every index is checked before it is used.
 * d_msg_end and d_reply_of hold max_messages entries; the messages are the
 * first min(d_msg_summary->frames, max_messages). */
typedef struct gevws_send {        /* 32 bytes */
    uint64_t off;      /* into its wire buffer */
    uint64_t len;
    uint64_t frame;    /* the decoded frame that triggered it */
    uint32_t conn;
    uint32_t wire;     /* 0 plain, 1 deflated, 2 control */
} gevws_send;
typedef struct gevws_conn_send {   /* 32 bytes per connection */
    uint64_t first;    /* its entries: d_send[first, first + count) */
    uint64_t count;
    uint64_t bytes;    /* the sum of their len */
    uint32_t flags;    /* GEVWS_CTL_*, copied from d_conn_ctl */
    uint32_t reserved;
} gevws_conn_send;
int gevws_send_plan_async(gevws_ctx *ctx, void *stream, uint64_t max_frames, const gevws_summary *d_decoded,
                          const gevws_conn_out *d_conn_out, uint32_t n_conns, const int64_t *d_msg_of,
                          const uint64_t *d_msg_end, const int64_t *d_reply_of, uint64_t max_messages,
                          const gevws_summary *d_msg_summary, const gevws_summary *d_join_summary,
                          const uint8_t *d_conn_ext /* may be NULL */, const int64_t *d_ctl_of,
                          const gevws_conn_ctl *d_conn_ctl, const gevws_summary *d_ctl_summary,
                          const uint64_t *d_plain_off, const gevws_summary *d_plain_encoded,
                          const uint64_t *d_def_off, const gevws_summary *d_def_encoded,
                          const uint64_t *d_ctl_off, const gevws_summary *d_ctl_encoded,
                          gevws_send *d_send, uint64_t max_sends, gevws_conn_send *d_conn_send,
                          gevws_summary *d_summary);

/* gevws_send_gather_async runs behind the plan: it puts every connection's
 * reply bytes next to each other in one buffer, so the host sends a pass with
 * one device-to-host copy (or none: d_buf may be mapped host memory) and one
 * write(fd, buf + off, bytes) per connection.
 *
 * It reads the plan's d_send / max_sends, d_conn_send / n_conns and summary
 * (d_plan), and the three wire buffers the entries point into: d_wires[w] is
 * wire w's base (0 plain, 1 deflated, 2 control) and wire_bytes[w] the number
 * of readable bytes behind it, its encode's payload_bytes.  Both are host
 * arrays of three, read during the call.  The encodes' GEVWS_OUT_PAD slack is
 * what lets the aligned 16-byte vector that holds a wire's last byte be loaded.
 *
 * d_conn_buf[c], for every connection (a gevws_conn_buf, below):
 *   - Span placement.  Connection c's span is d_buf[off, off + bytes).  It
 *     holds the len bytes of its entries d_send[first, first + count) in order,
 *     back to back.  Every span starts on a 16-byte boundary.  Spans lie in
 *     connection order.  The pad up to the next span is zeroed.
 *   - Empty connections.  A connection with count == 0 gets bytes = 0, and off
 *     is the next span's start (payload_bytes behind the last span).
 *   - flags is d_conn_send[c].flags, the reserved tail is zero.
 *   - Entries.  The entries are the first min(d_plan->frames, max_sends).
 * d_summary: frames = entries gathered, payload_bytes = buffer bytes used, pads
 * included (what the host copies; a multiple of 16), payload_len = the sum of
 * len, errors = 0.
 *   - Capacity.  GEVWS_ERR_CAPACITY when payload_bytes > buf_cap: the summary
 *     holds the need and nothing else is written.
 *   - Gates.  A failed d_plan, zero entries, n_conns == 0 or max_sends == 0
 *     give a zero summary; nothing else is read or written.
 *   - Malformed input makes the call GEVWS_ERR_INVALID on the device: `errors`
 *     counts the bad records (an entry or a connection counts once, whatever is
 *     wrong with it), the other fields are zero and nothing else is written.
 *     Every value is checked before it forms an address.  A bad entry has
 *     wire > 2, off + len beyond that wire's readable bytes (or overflowing),
 *     conn >= n_conns, or lies outside its connection's [first, first + count).
 *     A bad connection has a range beyond the entry count, a range that
 *     overlaps or precedes the previous connection's, or `bytes` not equal to
 *     the sum of its entries' len (the sum is taken over the entries that name
 *     the connection and are not bad themselves).
 *   - Invalid calls.  A non-zero `flags` is GEVWS_ERR_INVALID from the call,
 *     before any device is touched, even with every pointer NULL.  So is a
 *     wire base or a d_buf that is not 16-byte aligned, and max_sends >= 2^32.
 *   - Mapped host memory.  d_buf may be mapped host memory
 *     (gevws_pinned_alloc).  Every byte of [0, payload_bytes) is written exactly
 *     once, by an aligned 16-byte store; no byte at or past payload_bytes is
 *     written.  Of the wires only aligned vectors that hold a byte of an entry
 *     are loaded. */
typedef struct gevws_conn_buf {    /* 32 bytes per connection */
    uint64_t off;      /* its span: d_buf[off, off + bytes), off % 16 == 0 */
    uint64_t bytes;    /* d_conn_send[c].bytes */
    uint32_t flags;    /* GEVWS_CTL_*, copied from d_conn_send[c].flags */
    uint32_t reserved[3];
} gevws_conn_buf;
int gevws_send_gather_async(gevws_ctx *ctx, void *stream, const gevws_send *d_send, uint64_t max_sends,
                            const gevws_conn_send *d_conn_send, uint32_t n_conns, const gevws_summary *d_plan,
                            const uint8_t *const d_wires[3], const uint64_t wire_bytes[3], uint32_t flags,
                            uint8_t *d_buf, uint64_t buf_cap, gevws_conn_buf *d_conn_buf,
                            gevws_summary *d_summary);

/* Rooms: a delivered message goes to every connection in its sender's room
 * (the reference's example/websocket/main.go loops over serv.sessions on the
 * host).  Additions to ABI version 3: nothing above changes.  The chain of one
 * pass is the echo chain's with two steps exchanged:
 *   ... -> control -> gevws_reply_rooms_async -> deflate (no contexts) ->
 *   the three encodes -> gevws_room_plan_async -> gevws_send_gather_async.
 * A message is framed once and compressed once; the plan names its bytes once
 * per recipient, and the gather copies them.
 *
 * Room tables.  The caller owns them: device memory, read only.
 *   - d_conn_room[c] (n_conns entries): connection c's room, < n_rooms, or
 *     GEVWS_ROOM_NONE.  A connection receives from its room and publishes to
 *     it; a GEVWS_ROOM_NONE connection publishes nothing and is sent only its
 *     own control replies.
 *   - The inverse index in CSR form: d_room_first[n_rooms + 1] and
 *     d_room_members[n_members].  Room g's members are
 *     d_room_members[first[g], first[g + 1]), strictly increasing.
 *   - Well formed means: first[0] == 0; first never decreases; first[n_rooms]
 *     == n_members <= n_conns; every member < n_conns; members increase
 *     strictly inside a room; d_conn_room[member] == its room; every
 *     d_conn_room[c] is < n_rooms or GEVWS_ROOM_NONE; the connections with a
 *     room number n_members.  The two tables are then a bijection.  n_rooms ==
 *     0 with every connection GEVWS_ROOM_NONE is well formed.
 *   - Both calls check this on the device before anything is indexed by the
 *     tables.  The records are the n_rooms + 1 entries of d_room_first, the
 *     n_members slots and the n_conns connections; a record counts once,
 *     whatever is wrong with it, and a wrong number of roomed connections
 *     counts as one more.  Any bad record makes the call GEVWS_ERR_INVALID on
 *     the device: `errors` is the count, the other summary fields are zero and
 *     nothing else is written.
 *   - A call whose gates leave it no records (below) reads no table.
 *
 * Recipient kind.  A connection takes deflate when its d_conn_ext byte has
 * GEVWS_EXT_DEFLATE and not GEVWS_EXT_SERVER_TAKEOVER; otherwise it takes plain
 * (d_conn_ext == NULL: every connection).  A server-takeover connection gets a
 * broadcast message uncompressed, RSV1 clear: RFC 7692 section 6 leaves that
 * choice to the sender message by message, a message compressed in that
 * connection's own context could not be shared, and an uncompressed message
 * stays out of its window.
 *
 * gevws_reply_rooms_async is gevws_reply_bodies_async with rooms.
 *   - Inputs.  That function's, the room tables and `flags`.  policy, the
 *     bodies looked at, the gates (a failed d_msg_summary or d_join_summary
 *     gives two zero summaries and nothing else) and the malformed bodies (no
 *     GEVWS_BODY_JOINED / GEVWS_BODY_INFLATED, conn >= n_conns) are unchanged.
 *     GEVWS_HANDLER_NONE looks at no body and no table.
 *   - Flags.  GEVWS_ROOMS_SKIP_SENDER: a sender is not among its message's
 *     recipients.  Any other bit is GEVWS_ERR_INVALID from the call, before any
 *     device is touched, even with every pointer NULL.
 *   - Recipients.  A delivered body of sender c in room g goes to g's members,
 *     without c under GEVWS_ROOMS_SKIP_SENDER.  The body of a GEVWS_ROOM_NONE
 *     sender has none.
 *   - Lists.  The body enters the plain list (d_plain, as the reply step builds
 *     it: fin 1, rsv 0) exactly when a recipient takes plain, and the deflate
 *     list (d_def_msgs) exactly when a recipient takes deflate: both, one or
 *     neither.  d_plain_conn[k] / d_def_conn[k] are the sender.  Both lists
 *     keep the message order.  d_plain_of[m] / d_def_of[m], for each of the
 *     bodies, = the index in that list or -1.
 *   - Window.  window_bits of a deflate-list entry is the smallest effective
 *     d_conn_window_bits byte among the room's deflate-taking members (0, or a
 *     NULL table, counts as 15; the sender counts even when skipped), so one
 *     payload fits every recipient's server_max_window_bits.  The entry holds
 *     the value itself, 8..15.  A byte outside {0, 8..15} on a deflate-taking
 *     member makes that member's slot a bad record.
 *   - Summaries.  frames = the list's count, the other fields zero.  Bad table
 *     records and malformed bodies add up in `errors` of both.
 *   - The deflate list is for gevws_deflate_async (no contexts) over the join's
 *     d_out; the plain list for gevws_encode_replies_async, as in the echo.
 *
 * gevws_room_plan_async is gevws_send_plan_async with a fan-out.
 *   - Inputs.  That function's, with d_plain_of / d_def_of in the place of
 *     d_reply_of, plus the room tables and the same `flags`.
 *   - Publishing.  Frame f of sender s publishes when d_ctl_of[f] < 0, m =
 *     d_msg_of[f] is a message, d_msg_end[m] == f and s has a room: in wire 0
 *     when d_plain_of[m] >= 0 and in wire 1 when d_def_of[m] >= 0.  The bytes
 *     are that wire's [off, off + len), as the send plan takes them.
 *   - Order.  Recipient r, which takes wire w, is sent first every publication
 *     in wire w of its room's members in frame order (sender order, then stream
 *     order; r's own left out under GEVWS_ROOMS_SKIP_SENDER), then its own
 *     control replies in frame order (wire 2).  The close reply of a cut is
 *     therefore the last thing r is sent.
 *   - Outputs.  d_send / max_sends / d_conn_send / d_summary with the send
 *     plan's meaning, field for field: an entry is {off, len, frame = the
 *     publishing frame, conn = r, wire}; `errors` = connections with
 *     GEVWS_CTL_SHUTDOWN, d_conn_send[c].flags = d_conn_ctl[c].flags.
 *     gevws_send_gather_async runs over them unchanged.
 *   - Capacity, gates.  GEVWS_ERR_CAPACITY when there are more entries than
 *     max_sends: frames (and payload_bytes) hold the need and nothing else is
 *     written.  A failed d_decoded, d_msg_summary, d_join_summary,
 *     d_ctl_summary or encode summary, no decoded frames, n_conns == 0 or
 *     max_frames == 0 give a zero summary; nothing else is read or written.
 *   - Malformed input.  A reply index outside its list's count, a d_msg_of
 *     entry outside the message table, a frame that would send something and
 *     belongs to no connection or an offset table that decreases makes the
 *     call GEVWS_ERR_INVALID on the device, and so do bad room records:
 *     `errors` counts the frames and the records, the other fields are zero
 *     and nothing else is written.  Every index is checked before it is used.
 *   - Invalid calls.  A flag bit other than GEVWS_ROOMS_SKIP_SENDER or
 *     max_sends >= 2^32 is GEVWS_ERR_INVALID from the call, before any device
 *     is touched, even with every pointer NULL. */
#define GEVWS_ROOM_NONE 0xFFFFFFFFu
#define GEVWS_ROOMS_SKIP_SENDER 1u   /* call flag of both */
int gevws_reply_rooms_async(gevws_ctx *ctx, void *stream, const gevws_body *d_bodies, uint64_t max_messages,
                            const gevws_summary *d_msg_summary, const gevws_summary *d_join_summary, int policy,
                            const uint8_t *d_conn_ext /* may be NULL */,
                            const uint8_t *d_conn_window_bits /* may be NULL: 15 */, uint32_t n_conns,
                            const uint32_t *d_conn_room, const uint32_t *d_room_first,
                            const uint32_t *d_room_members, uint32_t n_rooms, uint32_t n_members, uint32_t flags,
                            gevws_deflate_msg *d_def_msgs, uint32_t *d_def_conn, gevws_summary *d_def_summary,
                            gevws_out_frame *d_plain, uint32_t *d_plain_conn, gevws_summary *d_plain_summary,
                            int64_t *d_plain_of, int64_t *d_def_of);
int gevws_room_plan_async(gevws_ctx *ctx, void *stream, uint64_t max_frames, const gevws_summary *d_decoded,
                          const gevws_conn_out *d_conn_out, uint32_t n_conns, const int64_t *d_msg_of,
                          const uint64_t *d_msg_end, const int64_t *d_plain_of, const int64_t *d_def_of,
                          uint64_t max_messages, const gevws_summary *d_msg_summary,
                          const gevws_summary *d_join_summary, const uint8_t *d_conn_ext /* may be NULL */,
                          const int64_t *d_ctl_of, const gevws_conn_ctl *d_conn_ctl,
                          const gevws_summary *d_ctl_summary, const uint64_t *d_plain_off,
                          const gevws_summary *d_plain_encoded, const uint64_t *d_def_off,
                          const gevws_summary *d_def_encoded, const uint64_t *d_ctl_off,
                          const gevws_summary *d_ctl_encoded, const uint32_t *d_conn_room,
                          const uint32_t *d_room_first, const uint32_t *d_room_members, uint32_t n_rooms,
                          uint32_t n_members, uint32_t flags, gevws_send *d_send, uint64_t max_sends,
                          gevws_conn_send *d_conn_send, gevws_summary *d_summary);

/* Membership changes on the device: joins, moves, leaves and the pass's closes
 * applied to d_conn_room, and the CSR inverse rebuilt, on the stream (the
 * reference edits serv.sessions on the host under a mutex).  Additions to ABI
 * version 3: nothing above changes.  The room tables can stay resident: the
 * host uploads the 8-byte change records, or nothing when the only changes are
 * the closes the plan already left in d_conn_send.
 *
 * gevws_rooms_update_async
 *   - Result.  Connection c's new room starts as d_conn_room_in[c].  The
 *     changes are then applied in list order: {conn, room} puts conn into room
 *     (< n_rooms: a join or a move; GEVWS_ROOM_NONE: a leave), and the last
 *     change that names a connection wins.  With d_conn_send, a connection
 *     whose d_conn_send[c].flags has GEVWS_CTL_SHUTDOWN ends in
 *     GEVWS_ROOM_NONE: a close beats a join in the same call.
 *   - Outputs.  d_conn_room_out (n_conns entries): the new rooms.
 *     d_room_first_out (n_rooms + 1 entries) and d_room_members_out: their CSR
 *     inverse, well formed as the room tables above define it -- rooms in
 *     order, a room's members strictly increasing: the tables a stable sort of
 *     the roomed connections by room gives.  d_room_members_out must hold
 *     n_conns entries; those at and behind n_members are not written.  The
 *     result is bit-exact: it does not depend on the grid, the scheduling or
 *     the order of any atomic.
 *   - The change count is max_changes, or min(d_prev->frames, max_changes) with
 *     d_prev (the summary of whatever made the list).  With d_changes == NULL
 *     the count is 0.  Without changes and without d_conn_send the call is a
 *     pure build of the CSR on the device.
 *   - n_rooms belongs to the call: a larger one than the tables were built
 *     with grows the room space.  Rooms may be empty.  n_rooms == 0 with every
 *     connection GEVWS_ROOM_NONE is valid.
 *   - Gates.  A d_prev or a d_plan_summary (the summary of the plan that wrote
 *     d_conn_send) whose status is not GEVWS_OK gives a zero summary with that
 *     status (d_prev's first) and nothing else is written: membership does not
 *     move for a pass that was not sent.
 *   - d_summary: frames = n_members, payload_len = the connections whose room
 *     differs between d_conn_room_in and d_conn_room_out, payload_bytes = the
 *     changes read, errors = 0, status GEVWS_OK.
 *   - Malformed input.  A d_conn_room_in[c] that is neither < n_rooms nor
 *     GEVWS_ROOM_NONE, a change with conn >= n_conns and a change whose room is
 *     neither < n_rooms nor GEVWS_ROOM_NONE are bad records, one counted per
 *     record.  Any of them makes the call GEVWS_ERR_INVALID on the device:
 *     `errors` is the count, the other fields are zero and nothing else is
 *     written.  Every index is checked before anything is indexed by it.
 *   - Invalid calls.  A NULL ctx, any bit of `flags` (none is defined), a NULL
 *     output, d_conn_room_in == NULL with n_conns > 0, d_conn_room_out ==
 *     d_conn_room_in or max_changes >= 2^32 is GEVWS_ERR_INVALID from the call,
 *     before any device is touched.
 *   - The inputs are never written, so a call that failed can be repeated as it
 *     was (the carry's ping-pong rule): the outputs of one call are the inputs
 *     of the next. */
typedef struct gevws_room_change {   /* 8 bytes */
    uint32_t conn;
    uint32_t room;                   /* < n_rooms joins / moves, GEVWS_ROOM_NONE leaves */
} gevws_room_change;
int gevws_rooms_update_async(gevws_ctx *ctx, void *stream, const uint32_t *d_conn_room_in, uint32_t n_conns,
                             uint32_t n_rooms, const gevws_room_change *d_changes /* may be NULL */,
                             uint64_t max_changes, const gevws_summary *d_prev /* may be NULL */,
                             const gevws_conn_send *d_conn_send /* may be NULL */,
                             const gevws_summary *d_plan_summary /* may be NULL */, uint32_t flags,
                             uint32_t *d_conn_room_out, uint32_t *d_room_first_out, uint32_t *d_room_members_out,
                             gevws_summary *d_summary);

/* Room commands: a client enters and leaves a room by what it sends.  "/join N"
 * and "/leave" in delivered text messages become the change records of
 * gevws_rooms_update_async on the device, and leave the broadcast (the
 * reference has no rooms and no commands).  Additions to ABI version 3:
 * nothing above changes.  The step stands behind the control step and in front
 * of the room reply step:
 *   ... -> join -> control -> gevws_room_commands_async ->
 *   gevws_reply_rooms_async -> ... -> gevws_room_plan_async -> gather, and
 *   between two passes gevws_rooms_update_async with d_changes / max_changes of
 *   this call and its d_summary as d_prev.
 * The message pass, the inflate step and the join run first, so a command that
 * arrives fragmented, split over two passes or compressed is a command like
 * any other by the time this step looks at it.
 *
 * The rule (gev_amd/csrc/gevws_room_command.hpp; gevws_room_command_parse is
 * the same rule on host bytes).
 *   - Looked at.  A body is looked at exactly when it is delivered
 *     (GEVWS_BODY_WHOLE), its opcode is 1 and its length is 6..16.  Only its
 *     first `length` bytes count, whatever lies behind them.
 *   - Leave.  The 6 bytes "/leave": the change {conn, GEVWS_ROOM_NONE}.
 *   - Join.  The 6 bytes "/join " followed by 1..10 bytes that are all '0'..'9'
 *     and nothing else; leading zeros are allowed; the value is taken in 64
 *     bits.  A value < n_rooms: the change {conn, value} (a join, or a move for
 *     a connection that has a room).  Any other value: a rejected command,
 *     which is stripped and makes no change.  4294967295 never passes:
 *     GEVWS_ROOM_NONE is not < n_rooms.
 *   - Everything else -- "/join" without digits, "/join 3\n", "/JOIN 3",
 *     "/leave ", a binary message of the same bytes -- is no command and is
 *     broadcast as before.
 *
 * gevws_room_commands_async
 *   - Inputs.  d_bodies / max_messages / d_msg_summary: the bodies are the first
 *     min(d_msg_summary->frames, max_messages).  d_join_summary the join's,
 *     d_ctl_summary the control step's (may be NULL), d_out / src_bytes the
 *     join's d_out and its readable bytes (what the deflate step is given).
 *     d_out starts on a 16-byte boundary, and a looked-at body is read as the
 *     whole aligned 16-byte vector at its `off`, as the join reads d_payload: the
 *     vector that holds the last byte of d_out is readable.  n_conns, n_rooms:
 *     the room tables'.  flags: none is defined.
 *   - d_changes (max_changes records): the changes in message order, that is by
 *     connection and then in stream order, so the update's rule that the last
 *     change of a connection wins is the client's last command.
 *   - d_change_of (max_messages entries): for each of the bodies the index of
 *     its change, -1 for no command, -2 for a rejected command.
 *   - Strip.  Every command body, accepted or rejected, is stripped in place as
 *     the control step strips a body behind a cut: off = length = flags = 0 and
 *     status GEVWS_MSG_COMMAND; conn and opcode stay.  No other body changes by
 *     a byte, and no byte of d_out is written.
 *   - d_summary: frames = changes written, payload_len = bodies stripped,
 *     payload_bytes = rejected commands, errors = 0, status GEVWS_OK.
 *   - Capacity.  More changes than max_changes is GEVWS_ERR_CAPACITY: frames
 *     holds the need, the other fields are zero and nothing else is written --
 *     d_bodies stays byte for byte, so the caller retries.
 *   - Gates.  A failed d_msg_summary, d_join_summary or (given) d_ctl_summary,
 *     no messages, or max_messages == 0 give a zero summary; nothing else is
 *     read or written.
 *   - Malformed input.  A delivered body with neither GEVWS_BODY_JOINED nor
 *     GEVWS_BODY_INFLATED or with conn >= n_conns (the reply step's two, on the
 *     same bodies), and a looked-at body with off % 16 != 0 or off + length >
 *     src_bytes, are bad records, each counted once.  Any of them makes the call
 *     GEVWS_ERR_INVALID on the device: `errors` is the count, the other fields
 *     are zero and nothing else is written.  The checks run before anything is
 *     loaded from `off` or indexed by `conn`.
 *   - Invalid calls.  A NULL ctx, any bit of `flags`, a NULL output (d_changes,
 *     d_change_of, d_summary), max_messages or max_changes >= 2^32 is
 *     GEVWS_ERR_INVALID from the call, before any device is touched, even with
 *     every pointer NULL.  With max_messages > 0 so is a NULL d_bodies,
 *     d_msg_summary or d_join_summary, a NULL d_out with src_bytes > 0 and a
 *     d_out that is not 16-byte aligned.
 *
 * Timing.  The update runs between passes, so a command takes effect at the
 * next pass:
 *   - a message behind "/join 3" in the same pass still goes to the old room
 *     (to nobody, from a connection that had none);
 *   - a command behind its connection's cut was stripped by the control step
 *     (GEVWS_MSG_ERR_CLOSED) and is no command;
 *   - a command in front of a close in the same pass is emitted, and the
 *     update's rule that a close beats a join settles it;
 *   - two commands of one connection in one pass: the last one wins.
 *
 * gevws_room_command_parse: the rule on host memory (FFI callers, CPU tests).
 * body[0, length) is read and nothing else; a length outside 6..16 reads
 * nothing.  Returns 0 for no command, 1 for a change and 2 for a rejected
 * command, or GEVWS_ERR_INVALID for a NULL body with a length of 6..16.  *room
 * (may be NULL) is the change's room -- GEVWS_ROOM_NONE for a leave -- and
 * GEVWS_ROOM_NONE whenever the result is not 1. */
enum { GEVWS_MSG_COMMAND = 10 };   /* continues the GEVWS_MSG_* enum: gevws_body.status of a stripped command */
int gevws_room_commands_async(gevws_ctx *ctx, void *stream, gevws_body *d_bodies, uint64_t max_messages,
                              const gevws_summary *d_msg_summary, const gevws_summary *d_join_summary,
                              const gevws_summary *d_ctl_summary /* may be NULL */, const uint8_t *d_out,
                              uint64_t src_bytes, uint32_t n_conns, uint32_t n_rooms, uint32_t flags,
                              gevws_room_change *d_changes, uint64_t max_changes,
                              int64_t *d_change_of /* max_messages entries */, gevws_summary *d_summary);
int gevws_room_command_parse(const uint8_t *body, uint64_t length, uint32_t n_rooms, uint32_t *room /* may be NULL */);

/* Outbound fragmentation: a frame size limit for what the chain sends (RFC
 * 6455 section 5.4; the reference writes every message as one frame,
 * write.go:48-84).  Additions to ABI version 3: nothing above changes.  Two
 * steps around the encode of a record list (the reply step's d_plain, or the
 * deflate step's d_out_frames):
 *   ... -> records -> gevws_fragment_async -> gevws_encode_replies_async over
 *   d_frags -> gevws_fragment_offsets_async -> the plan (send or room) -> gather.
 * A reply's fragments are adjacent in the wire, so one plan entry still names
 * the whole reply; the plans and the gather run unchanged.
 *
 * The rule (gev_amd/csrc/gevws_fragment.hpp), for a record r and the limit F =
 * max_fragment_bytes >= 1, bytes of payload a frame:
 *   - Splittable.  r splits exactly when hdr.fin == 1, hdr.opcode is 1 or 2,
 *     hdr.length >= 0, (uint64_t)hdr.length == payload_len and payload_len > F.
 *     It then has c = ceil(payload_len / F) fragments.
 *   - Every other record (a control frame, a record that is a fragment already,
 *     an inconsistent one, an empty or short message) has c = 1: its one
 *     fragment is the record itself, all 32 bytes.
 *   - Fragment i of a splittable record: hdr.fin = (i == c - 1); hdr.rsv =
 *     r's on i == 0, else 0 (RFC 7692 section 6.1: RSV1 on the first fragment
 *     only); hdr.opcode = r's on i == 0, else 0; hdr.masked and hdr.mask
 *     copied; hdr.length = payload_len = min(F, L - i F); payload_off =
 *     r.payload_off + i F.
 *   - Malformed.  A splittable record with c > 2^31 - 1, and nothing else.
 *
 * gevws_fragment_async
 *   - Records.  The first min(d_prev->frames, max_records) of d_records (d_prev
 *     == NULL: max_records).  d_prev is the summary of the step that made the
 *     list: the reply step's d_plain_summary, or the deflate step's.
 *   - d_frags (max_frags entries, on a 16-byte boundary): the fragments of
 *     record 0, then of record 1, and so on.  Their payload_off point into the
 *     payload arena the records pointed into.
 *   - d_first (max_records + 1 entries): d_first[k] is the index of record k's
 *     first fragment for k = 0..n, d_first[n] the total.  Entries behind n are
 *     not written.
 *   - d_summary: frames = the fragments, payload_len = the sum of their
 *     payload_len (the records', modulo 2^64), payload_bytes = the records that
 *     were split, errors = 0, status GEVWS_OK.  It is the d_dispatched of
 *     gevws_encode_replies_async over d_frags.
 *   - Capacity.  GEVWS_ERR_CAPACITY when there are more fragments than
 *     max_frags: the summary holds the same figures (frames is the need) and
 *     nothing else is written.
 *   - Gate.  A failed d_prev gives a zero summary; nothing else is read or
 *     written.
 *   - Malformed records make the call GEVWS_ERR_INVALID on the device: `errors`
 *     counts them, the other fields are zero and nothing else is written.
 *   - Invalid calls.  max_fragment_bytes == 0, any bit of `flags`, max_records
 *     or max_frags >= 2^32 are GEVWS_ERR_INVALID from the call, before any
 *     device is touched, even with every pointer NULL.  So is a d_frags that is
 *     not 16-byte aligned.
 *   - The step reads no payload byte and forms no address from record data.
 *
 * gevws_fragment_offsets_async runs behind the encode of d_frags.
 *   - Inputs.  d_first / max_records / d_prev as above, d_fragged the fragment
 *     step's summary, d_frag_off / d_frag_encoded the encode's offset table and
 *     summary.
 *   - d_reply_off[k] (max_records entries) = d_frag_off[d_first[k]] for the n
 *     records (the wire total for a record with no fragment).  d_reply_encoded:
 *     frames = n, payload_bytes and payload_len the encode's, status GEVWS_OK.
 *     The two stand where (d_plain_off, d_plain_encoded) or (d_def_off,
 *     d_def_encoded) stand in gevws_send_plan_async and gevws_room_plan_async:
 *     entry k's bytes run to the next reply's first fragment, or to the wire
 *     total.
 *   - Gates.  A failed d_prev, d_fragged or d_frag_encoded gives a zero summary
 *     that carries the first failing status (for the encode's
 *     GEVWS_ERR_CAPACITY also its need in payload_bytes); nothing else is read
 *     or written.
 *   - The tables must fit together: d_first[0] == 0, d_first never decreases
 *     over 0..n, d_first[n] == d_fragged->frames == d_frag_encoded->frames.
 *     Otherwise the call is GEVWS_ERR_INVALID on the device: `errors` counts the
 *     bad entries of d_first[0..n] (an entry counts once: 0 for a non-zero
 *     start, k for d_first[k] > d_first[k + 1], n for a wrong total), the other
 *     fields are zero and nothing else is written.  d_frag_off is indexed only
 *     after this check.
 *   - Invalid calls.  A NULL required pointer or max_records >= 2^32 is
 *     GEVWS_ERR_INVALID from the call.
 *
 * gevws_fragment_records is the fragment step on host memory (FFI callers, CPU
 * tests): the n records, the same outputs and the same statuses in *summary
 * (the call itself fails only as an invalid call does). */
int gevws_fragment_async(gevws_ctx *ctx, void *stream, const gevws_out_frame *d_records, uint64_t max_records,
                         const gevws_summary *d_prev /* may be NULL: max_records */, uint64_t max_fragment_bytes,
                         uint32_t flags, gevws_out_frame *d_frags, uint64_t max_frags,
                         uint64_t *d_first /* max_records + 1 entries */, gevws_summary *d_summary);
int gevws_fragment_offsets_async(gevws_ctx *ctx, void *stream, const uint64_t *d_first, uint64_t max_records,
                                 const gevws_summary *d_prev /* may be NULL */, const gevws_summary *d_fragged,
                                 const uint64_t *d_frag_off, const gevws_summary *d_frag_encoded,
                                 uint64_t *d_reply_off /* max_records entries */,
                                 gevws_summary *d_reply_encoded);
int gevws_fragment_records(const gevws_out_frame *records, uint64_t n, uint64_t max_fragment_bytes,
                           gevws_out_frame *frags, uint64_t max_frags, uint64_t *first, gevws_summary *summary);

/* Server push: messages that the host originates, to every connection, to a
 * room or to one connection (the reference's example/websocket/main.go:129-150
 * packs "publish message" on a timer and Sends it to every session, and lines
 * 103-115 Send from goroutines, through connection.go:122 over
 * ws/util/util.go:10).  Additions to ABI version 3: nothing above changes.  A
 * push pass is a chain of its own, with no decode in front:
 *   push records + body arena -> gevws_push_lists_async -> gevws_deflate_async
 *   (no contexts) -> gevws_encode_replies_async over the plain list and over
 *   the deflate step's records (with gevws_fragment_async /
 *   gevws_fragment_offsets_async around either, as in a broadcast) ->
 *   gevws_push_plan_async -> gevws_send_gather_async with an empty wire 2.
 * A push is framed once and compressed once, however many connections receive
 * it; the plan names its bytes once per recipient.  The output has the shape
 * of any other pass (d_send, d_conn_send, the gather's buffer).
 *
 * The record.  d_src is the body arena: device memory the caller fills, on a
 * 16-byte boundary, with the readable slack the encoder and the deflate step
 * ask of their payload arena.
 *   - off / length: the body, d_src[off, off + length).  off is a multiple of
 *     GEVWS_PAYLOAD_ALIGN.
 *   - kind / target: GEVWS_PUSH_ALL (target 0), GEVWS_PUSH_ROOM (target = the
 *     room, < n_rooms) or GEVWS_PUSH_CONN (target = the connection, < n_conns).
 *   - opcode: 1 text, 2 binary, 9 ping, 10 pong.  A close frame (8) is
 *     malformed: closing stays with the control step and the host.
 *   - Order.  The list must not decrease in the key (kind << 32) | target.  A
 *     recipient's pushes are then at most three contiguous slices -- the ALL
 *     pushes, its room's, its own -- and it is sent them in list order.  The
 *     host sorts (a stable sort keeps the order within a key); the device
 *     checks.
 *   - Count.  The records are the first min(d_prev->frames, max_pushes) of
 *     d_pushes; d_prev == NULL: max_pushes.  d_prev is the summary of whatever
 *     made the list on the device.
 *   - Malformed, each record counted once: a kind above 2; a target out of
 *     range, or nonzero for GEVWS_PUSH_ALL; an opcode outside {1, 2, 9, 10};
 *     off % 16 != 0; off + length > src_bytes, or the sum overflowing; length >
 *     2^32 - 1; a ping or pong longer than 125 bytes; a nonzero reserved byte;
 *     a key below the previous record's.  gevws_push_check counts them on the
 *     host by the same code (gev_amd/csrc/gevws_push.hpp).
 *
 * Recipients.  d_conn_live (n_conns bytes, may be NULL: every connection) says
 * which connections of the table are sessions: n_conns is a table size, and
 * the host clears the byte of a connection that an earlier pass shut down
 * (GEVWS_CTL_SHUTDOWN).  An ALL push goes to every live connection, a ROOM
 * push to the room's live members, a CONN push to its connection when it is
 * live.  A push without recipients enters no list and no plan entry; it is not
 * an error.  The recipient kind is the rooms' (above): a live connection takes
 * deflate when its d_conn_ext byte has GEVWS_EXT_DEFLATE and not
 * GEVWS_EXT_SERVER_TAKEOVER (d_conn_ext == NULL: none does), and every
 * recipient takes a ping or a pong plain.
 *
 * The room tables are those of gevws_reply_rooms_async, checked on the device
 * by the same rule before anything is indexed by them.  All three pointers may
 * be NULL with n_rooms == n_members == 0: every connection is then
 * GEVWS_ROOM_NONE and a ROOM push is malformed.
 *
 * gevws_push_lists_async
 *   - Plain list.  Push p enters d_plain exactly when at least one of its
 *     recipients takes it plain: a gevws_out_frame with fin 1, rsv 0, the
 *     push's opcode, unmasked, hdr.length = payload_len = length, payload_off =
 *     off.  It is for gevws_encode_replies_async over d_src.
 *   - Deflate list.  Push p enters d_def_msgs exactly when its opcode is 1 or 2
 *     and at least one recipient takes deflate: {off, length, opcode,
 *     window_bits}.  It is for gevws_deflate_async (no contexts) over d_src.  A
 *     push can be in both lists, in one or in neither.
 *   - Window.  window_bits of a deflate-list entry is the smallest effective
 *     d_conn_window_bits byte among the push's deflate-taking recipients (0, or
 *     a NULL table, counts as 15).  The entry holds the value itself, 8..15.  A
 *     byte outside {0, 8..15} on a live deflate-taking connection makes that
 *     connection's record a bad table record (counted once with whatever else
 *     is wrong with it).
 *   - Order and indices.  Both lists keep the push order.  d_plain_of[p] /
 *     d_def_of[p], for each of the records, = the index in that list or -1.
 *   - Summaries.  d_plain_summary / d_def_summary: frames = the list's count,
 *     the other fields zero.  Malformed records and bad table records add up in
 *     `errors` of both with GEVWS_ERR_INVALID; nothing else is then written.
 *   - Gates.  A failed d_prev or no records gives two zero summaries; nothing
 *     else is read (no table either) or written.
 *   - Invalid calls.  Any bit of `flags` (none is defined), max_pushes >= 2^32
 *     or a NULL ctx is GEVWS_ERR_INVALID from the call, before any device is
 *     touched, even with every pointer NULL.  So is a NULL summary and, with
 *     max_pushes > 0, a NULL d_pushes or list output, or room tables that are
 *     neither all NULL with n_rooms == n_members == 0 nor complete.
 *
 * gevws_push_plan_async runs behind the two encodes, or behind
 * gevws_fragment_offsets_async where a wire was fragmented.
 *   - Inputs.  The push list and its count as above; the list step's two
 *     summaries and (d_plain_off, d_plain_encoded), (d_def_off, d_def_encoded)
 *     with the meaning they have in gevws_room_plan_async: `frames` of an
 *     encode summary is its list's count and payload_bytes its wire total.
 *     d_plain_of / d_def_of, d_conn_ext, d_conn_live and the room tables as
 *     above.
 *   - Rule.  Recipient r is sent its pushes in list order.  Push p comes from
 *     wire 1 when r takes deflate and d_def_of[p] >= 0, otherwise from wire 0.
 *     d_send[k] = {off, len, frame = p, conn = r, wire}: off from that wire's
 *     table at the push's list index, len to the next entry's offset or to the
 *     wire total.
 *   - Outputs.  d_conn_send[c] = {first, count, bytes, flags = 0} for every
 *     connection, in connection order.  d_summary: frames = entries,
 *     payload_bytes = the sum of len, errors = 0.  gevws_send_gather_async
 *     runs over them unchanged.
 *   - Capacity.  GEVWS_ERR_CAPACITY when there are more entries than
 *     max_sends: frames and payload_bytes hold the need and nothing else is
 *     written.
 *   - Gates.  A failed d_prev, list summary or encode summary, no records or
 *     n_conns == 0 give a zero summary; nothing else is read or written.
 *   - Malformed input.  A malformed push record or a bad table record (as
 *     above, without the window bytes), a list index outside its list's count,
 *     an offset table that decreases at a listed push, and a push that a
 *     recipient needs from a list it is not in (such tables cannot come from
 *     the list step) make the call GEVWS_ERR_INVALID on the device: `errors` is
 *     the count (a push counts once), the other fields are zero and nothing
 *     else is written.  Every index is checked before it is used.
 *   - Invalid calls.  Any bit of `flags`, max_pushes or max_sends >= 2^32 or a
 *     NULL ctx is GEVWS_ERR_INVALID from the call, before any device is
 *     touched, even with every pointer NULL.
 *
 * gevws_push_check: the record rule on host memory (FFI callers, the Python
 * helper, CPU tests): the number of malformed records among records[0, n), or
 * GEVWS_ERR_INVALID for a NULL list with n > 0 or n >= 2^32.
 *
 * The host's side of the order (not enforced here): a push pass's spans are
 * written to the sockets in stream order with the passes around them, and a
 * connection that an earlier pass shut down is marked not live before the next
 * push. */
#define GEVWS_PUSH_ALL 0u
#define GEVWS_PUSH_ROOM 1u
#define GEVWS_PUSH_CONN 2u
typedef struct gevws_push {        /* 32 bytes */
    uint64_t off;                  /* into d_src, a multiple of GEVWS_PAYLOAD_ALIGN */
    uint64_t length;               /* <= 2^32 - 1; <= 125 for opcode 9 / 10 */
    uint32_t target;               /* ALL: 0; ROOM: room < n_rooms; CONN: connection < n_conns */
    uint8_t kind;                  /* GEVWS_PUSH_ALL / GEVWS_PUSH_ROOM / GEVWS_PUSH_CONN */
    uint8_t opcode;                /* 1 text, 2 binary, 9 ping, 10 pong */
    uint8_t reserved[10];          /* zero */
} gevws_push;
int gevws_push_lists_async(gevws_ctx *ctx, void *stream, const gevws_push *d_pushes, uint64_t max_pushes,
                           const gevws_summary *d_prev /* may be NULL: max_pushes */, uint64_t src_bytes,
                           const uint8_t *d_conn_ext /* may be NULL */,
                           const uint8_t *d_conn_window_bits /* may be NULL: 15 */,
                           const uint8_t *d_conn_live /* may be NULL: all */, uint32_t n_conns,
                           const uint32_t *d_conn_room, const uint32_t *d_room_first,
                           const uint32_t *d_room_members, uint32_t n_rooms, uint32_t n_members, uint32_t flags,
                           gevws_deflate_msg *d_def_msgs, gevws_summary *d_def_summary, gevws_out_frame *d_plain,
                           gevws_summary *d_plain_summary, int64_t *d_plain_of, int64_t *d_def_of);
int gevws_push_plan_async(gevws_ctx *ctx, void *stream, const gevws_push *d_pushes, uint64_t max_pushes,
                          const gevws_summary *d_prev /* may be NULL: max_pushes */, uint64_t src_bytes,
                          const gevws_summary *d_plain_summary, const gevws_summary *d_def_summary,
                          const int64_t *d_plain_of, const int64_t *d_def_of, const uint64_t *d_plain_off,
                          const gevws_summary *d_plain_encoded, const uint64_t *d_def_off,
                          const gevws_summary *d_def_encoded, const uint8_t *d_conn_ext /* may be NULL */,
                          const uint8_t *d_conn_live /* may be NULL: all */, uint32_t n_conns,
                          const uint32_t *d_conn_room, const uint32_t *d_room_first,
                          const uint32_t *d_room_members, uint32_t n_rooms, uint32_t n_members, uint32_t flags,
                          gevws_send *d_send, uint64_t max_sends, gevws_conn_send *d_conn_send,
                          gevws_summary *d_summary);
int64_t gevws_push_check(const gevws_push *records, uint64_t n, uint32_t n_conns, uint32_t n_rooms,
                         uint64_t src_bytes);

/* Measurement helper, not on the reference path: n bytes (n % 16 == 0, d_dst
 * 16-byte aligned, d_src any alignment) copied with the unmask kernel's
 * streaming access pattern minus the XOR and frame lookup -- the achievable
 * HBM rate bench.py reports beside the spec peak.  grid 0 = one workgroup per
 * CU (the unmask kernel's grid for large frames), each a contiguous run of
 * tiles; grid | 0x40000000 uses plain loads instead of the non-temporal ones the
 * unmask kernel's streaming path uses; grid | 0x20000000 copies in the
 * unmask's wave layout (each wave a contiguous 16 KiB span per step);
 * grid | 0x10000000 stores with plain 16-byte stores and then accepts a
 * d_dst of any alignment (the access pattern of an encode that scatters
 * aligned payload chunks to their wire positions); grid | 0x08000000 the
 * same with non-temporal stores. */
int gevws_copy_async(gevws_ctx *ctx, void *stream, uint8_t *d_dst, const uint8_t *d_src, uint64_t n,
                     uint32_t grid);

/* Host-ingress helper, not on the reference path: `bytes` of page-locked host
 * memory mapped into the device address space (hipHostMallocMapped).
 * *host_ptr is the CPU address, *dev_ptr the address kernels use; passing
 * *dev_ptr as gevws_decode_batch_async's d_payload makes the unmask kernel
 * write the decoded payload straight into host memory over PCIe (no D2H copy
 * of the arena).  GEVWS_ERR_DEVICE when the runtime refuses. */
int gevws_pinned_alloc(uint64_t bytes, void **host_ptr, void **dev_ptr);
int gevws_pinned_free(void *host_ptr);

/* Measurement helper, not on the reference path: `bytes` of device memory on
 * `device`, zeroed, of one of three kinds -- GEVWS_MEM_DEFAULT (hipMalloc:
 * coarse-grained, cached in L2), GEVWS_MEM_FINE (fine-grained) or
 * GEVWS_MEM_UNCACHED (hipDeviceMallocUncached: accesses bypass L2, so a
 * 16-byte header read need not fetch a whole 128-byte line).  An input arena
 * placed in it is decoded like any other.  Free with gevws_device_free. */
#define GEVWS_MEM_DEFAULT 0
#define GEVWS_MEM_FINE 1
#define GEVWS_MEM_UNCACHED 2
int gevws_device_alloc(int device, uint64_t bytes, int kind, void **ptr);
int gevws_device_free(int device, void *ptr);

/* ws.Cipher(payload, mask, offset), plugins/websocket/ws/cipher.go:14-53, on a
 * device buffer in place: p[i] ^= mask[(offset+i) % 4]. */
int gevws_cipher_async(gevws_ctx *ctx, void *stream, uint8_t *d_p, uint64_t n,
                       const uint8_t mask[4], uint64_t offset);

/* ---------------------------------------------------------------- per-frame host calls
 * For a host (cgo / C++) that looks at ONE frame at the head of a connection's
 * buffer -- e.g. to apply the reference's completeness gate (protocol.go:47)
 * before handing the connection to a device pass.  Plain host memory, no
 * context, no device work. */

/* ws.VirtualReadHeader (plugins/websocket/ws/read.go:19-84) on the `avail`
 * buffered bytes at p.  GEVWS_OK: *out = the header (ws.Header layout),
 * *hdr_len = its length (2..14); the frame is complete iff avail >= *hdr_len +
 * out->length (protocol.go:47).  GEVWS_NEED_MORE: fewer than 6 bytes
 * (ErrHeaderNotReady, read.go:20-23 -- even for a complete 2..5-byte frame) or
 * the extended header is not complete yet (Appendix A U1); *hdr_len = the
 * header length when at least 2 bytes are buffered, else 0.
 * GEVWS_ERR_LEN_MSB: ErrHeaderLengthMSB (read.go:71-73).  *out is written only
 * on GEVWS_OK. */
int gevws_parse_header(const uint8_t *p, uint64_t avail, gevws_header *out, uint32_t *hdr_len);

/* The same over a ring buffer's PeekAll() segments (first, end): the header may
 * straddle the wrap, as the virtual reads of read.go:27,63 allow. */
int gevws_parse_header_ring(const uint8_t *seg0, uint64_t n0, const uint8_t *seg1, uint64_t n1,
                            gevws_header *out, uint32_t *hdr_len);

/* ws.Cipher(p[:n], mask, offset) (plugins/websocket/ws/cipher.go:14-53) in host
 * memory, in place: p[i] ^= mask[(offset + i) % 4]. */
void gevws_cipher(uint8_t *p, uint64_t n, const uint8_t mask[4], uint64_t offset);

/* ---------------------------------------------------------------- synthetic batches
 * Device-side frame generator used by the bench and the full-size property
 * tests (no 64 GiB host buffer is ever built).  d_desc describes each frame:
 * header position in the arena, payload length, key, first header byte, and
 * length form (7, 16 or 64 bit).  Payload plaintext byte i of frame g is
 * byte (i & 7) of splitmix64(seed ^ (g * 0x9E3779B97F4A7C15) + (i >> 3)). */
typedef struct gevws_synth_desc {
    uint64_t hdr_off;   /* arena offset of the frame's first header byte */
    uint64_t length;    /* payload length */
    uint32_t mask;      /* key bytes, little-endian (mask[0] = low byte) */
    uint8_t b0;         /* FIN | RSV | opcode */
    uint8_t len_form;   /* 7, 16 or 64 */
    uint8_t masked;
    uint8_t pad;
} gevws_synth_desc;

int gevws_synth_async(gevws_ctx *ctx, void *stream, uint8_t *d_in, const gevws_synth_desc *d_desc,
                      uint64_t n_frames, uint64_t seed);
/* Property check of a decoded batch against the generator: counts mismatching
 * header fields, payload bytes (decode(mask(P)) == P) and non-zero pad bytes
 * into *d_mismatch (device uint64, accumulated).  Frame g of the batch must be
 * frame g of d_desc; records pointing outside [0, payload_cap) or not 16-byte
 * aligned count as mismatches and are not dereferenced: one outside the arena
 * counts its length + 1 and nothing else, a misaligned one counts its header
 * fields (the alignment among them) and none of its bytes. */
int gevws_synth_verify_async(gevws_ctx *ctx, void *stream, const gevws_synth_desc *d_desc,
                             uint64_t n_frames, uint64_t seed, const gevws_frame *d_frames,
                             const uint8_t *d_payload, uint64_t payload_cap, uint64_t *d_mismatch);

/* ---------------------------------------------------------------- host mirror
 * C++ host side above the device ABI, mirroring the reference's plugin
 * surface for this path (gev.Protocol, protocol.go:10-13; websocket.Protocol,
 * plugins/websocket/protocol.go:16-69; ringbuffer.RingBuffer as used at
 * read.go:20,27,63, protocol.go:47-60, connection.go:232-242). */
typedef struct gevws_ring gevws_ring;
typedef struct gevws_conn gevws_conn;
typedef struct gevws_protocol gevws_protocol;

/* ringbuffer.New(size) / Write / Length / PeekAll / Retrieve / IsEmpty. */
gevws_ring *gevws_ring_new(uint64_t size);
void gevws_ring_free(gevws_ring *r);
uint64_t gevws_ring_write(gevws_ring *r, const uint8_t *p, uint64_t n);
uint64_t gevws_ring_length(const gevws_ring *r);
uint64_t gevws_ring_capacity(const gevws_ring *r);
void gevws_ring_peek_all(const gevws_ring *r, const uint8_t **first, uint64_t *n_first,
                         const uint8_t **end, uint64_t *n_end);
void gevws_ring_retrieve(gevws_ring *r, uint64_t n);

/* gev.Connection's KeyValueContext as the websocket plugin uses it
 * (protocol.go:11-14, 28-39): the "gev_ws_upgraded" flag. */
gevws_conn *gevws_conn_new(void);
void gevws_conn_free(gevws_conn *c);
void gevws_conn_set_upgraded(gevws_conn *c, int upgraded);
int gevws_conn_upgraded(const gevws_conn *c);
/* Decoded frames still queued for delivery on this connection. */
uint64_t gevws_conn_pending(const gevws_conn *c);

/* websocket.New(u) (protocol.go:22-24), bound to a device context. */
gevws_protocol *gevws_protocol_new(gevws_ctx *ctx);
void gevws_protocol_free(gevws_protocol *p);

/* websocket.(*Protocol).UnPacket(c, buffer) (protocol.go:27-64): one frame per
 * call.  GEVWS_OK: *ctx_out = the header, (*out, *out_len) = the unmasked
 * payload (protocol-owned, valid until the next UnPacket on this connection),
 * h + L bytes consumed from `ring`.  GEVWS_NEED_MORE: (nil, nil), nothing
 * consumed.  < 0: logged and (nil, nil), as protocol.go:32-34, 41-45.  When the
 * connection has no queued frames the call decodes its buffered bytes on the
 * device first.  On a connection not yet upgraded it runs the handshake
 * (protocol.go:28-37; needs gevws_protocol_set_upgrader): GEVWS_HANDSHAKE with
 * (*out, *out_len) = the 101 response, or GEVWS_ERR_HANDSHAKE with the error
 * response (possibly empty) -- the driver loop (connection.go:208-218) keeps
 * calling while the status is GEVWS_OK or *out_len != 0, sending every `out`
 * that is not a frame payload. */
int gevws_protocol_unpacket(gevws_protocol *p, gevws_conn *c, gevws_ring *ring,
                            gevws_header *ctx_out, const uint8_t **out, uint64_t *out_len);

/* Batched driver for an event loop: one device pass over the buffered bytes of
 * n connections (stage -> H2D -> decode -> D2H); afterwards
 * gevws_protocol_unpacket returns their frames in stream order with no further
 * device work.  A pass still in flight from _begin below is finished (its
 * frames queued) first, as gevws_protocol_unpacket does.  Returns the number
 * of frames decoded, or < 0. */
int64_t gevws_protocol_unpacket_batch(gevws_protocol *p, gevws_conn *const *conns,
                                      gevws_ring *const *rings, uint32_t n);

/* gevws_protocol_unpacket_batch in two halves, so an event loop can read its
 * sockets while the device decodes (connection.go:208-251 runs read and
 * decode back to back; this overlaps them): _begin selects the connections
 * that can make progress, stages their buffered bytes and enqueues the pass
 * without waiting -- it returns the number of connections in the pass (0:
 * nothing to do) or < 0 (GEVWS_ERR_INVALID while a pass is in flight); _end
 * waits for that pass and queues its frames, returning the number of frames
 * decoded (0 when none is in flight) or < 0.  Between the two the rings may
 * take new bytes (gevws_ring_write; the pass decodes its staged copy) but must
 * not be read or retrieved; gevws_protocol_unpacket, _unpacket_batch and
 * gevws_decode_host_batch end a pass in flight first.  The protocol keeps the
 * `conns` and `rings` pointers (not the arrays) until _end: every connection
 * and ring listed must stay alive until then. */
int64_t gevws_protocol_unpacket_batch_begin(gevws_protocol *p, gevws_conn *const *conns,
                                            gevws_ring *const *rings, uint32_t n);
int64_t gevws_protocol_unpacket_batch_end(gevws_protocol *p);

/* Counters of a protocol's host ingress (not on the reference path):
 * device passes run, connections staged into them, bytes staged, UnPacket
 * calls answered NEED_MORE by the host-side gate without a device pass (the
 * first frame's h + L is not buffered yet, protocol.go:47), and the passes run
 * zero-copy (below). */
typedef struct gevws_protocol_stats {
    uint64_t device_passes;
    uint64_t conns_staged;
    uint64_t bytes_staged;
    uint64_t gated;
    uint64_t zero_copy_passes;
    uint64_t handler_passes;  /* passes that ran the device handler step */
    uint64_t chained_handler_passes; /* of those, enqueued behind a zero-copy
                                      * decode (one synchronisation per pass) */
    uint64_t signalled_passes;       /* waits answered by the kernels' completion
                                      * flag (gevws_ctx_set_completion_flag)
                                      * instead of a stream synchronisation */
    uint64_t service_passes;  /* passes posted to the resident decode service */
    uint64_t service_misses;  /* of those, launched again after the instance
                               * ended without them (not expected) */
} gevws_protocol_stats;
void gevws_protocol_get_stats(const gevws_protocol *p, gevws_protocol_stats *out);

/* Where a batched pass's time goes (measurement, not on the reference path):
 * host nanoseconds summed over the batched passes so far -- selecting the
 * ready connections (the host gate, protocol.go:47), staging their bytes into
 * pinned memory, enqueuing the launches (and copies), waiting for the
 * completion flag or the stream, and queueing the frames on their
 * connections -- and, for passes answered by the completion flag, the
 * one-launch kernels' own GPU time from their tick stamps.  ns_wait minus the
 * GPU time is the launch and completion latency. */
typedef struct gevws_protocol_timeline {
    uint64_t passes;
    uint64_t signalled;        /* passes whose wait was the completion flag (GPU times below) */
    uint64_t ns_select;
    uint64_t ns_stage;
    uint64_t ns_launch;
    uint64_t ns_wait;
    uint64_t ns_deliver;
    uint64_t ns_gpu_decode;    /* signalled passes: k_decode_small's start -> end */
    uint64_t ns_gpu_handler;   /* signalled passes with the handler step: k_handle_small's */
    uint64_t ns_gpu_gap;       /* signalled passes with the handler: decode end -> handler start */
} gevws_protocol_timeline;
void gevws_protocol_get_timeline(const gevws_protocol *p, gevws_protocol_timeline *out);

/* Batched passes over at most `bytes` of buffered input (default
 * GEVWS_ZERO_COPY_MAX_DEFAULT; 0 = never) run zero-copy: the kernels read the
 * pinned staging block and write records, payload and results into mapped
 * pinned host memory, so the pass is its launches and one synchronisation
 * with no H2D / D2H copies (a small pass is latency, not bytes).  Larger
 * passes copy in and out (DMA at the PCIe rate). */
#define GEVWS_ZERO_COPY_MAX_DEFAULT (256u * 1024u)

/* websocket.HandlerWrap.OnMessage (plugins/websocket/wrap.go:38-90) on the
 * device for every frame a pass decodes: policy GEVWS_HANDLER_* (-1 = off, the
 * default).  Each pass then also runs gevws_dispatch_async + encode over its
 * frames (close -> util.HandleClose reply, ping -> pong, pong -> ping, data ->
 * the policy's echo as a binary / text frame; FrameToBytes of each) and one
 * more synchronisation; gevws_protocol_reply hands out the answer. */
int gevws_protocol_set_handler(gevws_protocol *p, int policy);
/* The handler's answer for the frame gevws_protocol_unpacket last returned on
 * c: *reply / *len = the reply frame's wire bytes (the `out` OnMessage returns;
 * len 0 = none), *shutdown_write = 1 for a close frame (c.ShutdownWrite() after
 * sending the reply, wrap.go:52-56).  Valid until the next UnPacket on c.
 * GEVWS_ERR_INVALID when no frame was returned yet or the returned frame's
 * pass did not run the handler (decoded while it was off). */
int gevws_protocol_reply(const gevws_protocol *p, const gevws_conn *c, const uint8_t **reply, uint64_t *len,
                         int *shutdown_write);
void gevws_protocol_set_zero_copy_max(gevws_protocol *p, uint64_t bytes);
/* The protocol's zero-copy passes without a handler step go to its context's
 * resident decode service (gevws_ctx_set_service, gevws_decode_batch_post):
 * no launch call on the loop's path.  on = 0 stops it (the default). */
int gevws_protocol_set_service(gevws_protocol *p, int on);
/* The same for direct dispatch (gevws_ctx_set_direct): the protocol's
 * zero-copy passes without a handler step are written into its context's
 * own queue.  on = 0 turns it off (the default). */
int gevws_protocol_set_direct(gevws_protocol *p, int on);

/* One connection's buffered bytes in host memory, as ringbuffer.PeekAll()
 * returns them (first, end) -- e.g. two Go slices passed through cgo. */
typedef struct gevws_host_conn {
    const uint8_t *seg0;
    uint64_t n0;
    const uint8_t *seg1;
    uint64_t n1;
} gevws_host_conn;

/* Host-memory form of the batch decode for FFI callers (cgo): the segments of
 * n connections are staged into pinned memory, decoded on the device and the
 * results copied into the caller's buffers (frames, 16-byte-aligned payload
 * arena, per-connection results).  frames[i].src_off is relative to its own
 * connection's joined segments.  Returns the frame count, GEVWS_ERR_CAPACITY
 * (with *summary holding the sizes needed), or < 0.  Nothing is retained. */
int64_t gevws_decode_host_batch(gevws_protocol *p, const gevws_host_conn *conns, uint32_t n,
                                gevws_frame *frames, uint64_t max_frames, uint8_t *payload,
                                uint64_t payload_cap, gevws_conn_out *conn_out,
                                gevws_summary *summary);

/* One connection, segments as plain arguments (cgo may pass Go slice pointers
 * as arguments but not inside a struct): repeated UnPacket over
 * seg0 || seg1, i.e. ringbuffer.PeekAll()'s (first, end). */
int64_t gevws_decode_host_stream(gevws_protocol *p, const uint8_t *seg0, uint64_t n0,
                                 const uint8_t *seg1, uint64_t n1, gevws_frame *frames,
                                 uint64_t max_frames, uint8_t *payload, uint64_t payload_cap,
                                 gevws_conn_out *conn_out, gevws_summary *summary);

/* ---------------------------------------------------------------- handshake
 * ws.Upgrader (plugins/websocket/ws/ws.go:49-154) and Upgrader.Upgrade
 * (ws.go:158-343) with its HTTP helpers (http.go, nonce.go, util.go) -- host
 * code, once per connection. */
enum {
    GEVWS_HS_OK = 0,
    GEVWS_HS_MALFORMED_REQUEST = 1, /* ErrMalformedRequest (errors.go:60-64); also the
                                       head not yet complete (ws.go:176-198: nothing read) */
    GEVWS_HS_BAD_PROTOCOL = 2,      /* ErrHandshakeBadProtocol (errors.go:26-29) */
    GEVWS_HS_BAD_METHOD = 3,        /* ErrHandshakeBadMethod (errors.go:30-33) */
    GEVWS_HS_BAD_HOST = 4,          /* errors.go:34-37 */
    GEVWS_HS_BAD_UPGRADE = 5,       /* errors.go:38-41 */
    GEVWS_HS_BAD_CONNECTION = 6,    /* errors.go:42-45 */
    GEVWS_HS_BAD_SEC_ACCEPT = 7,    /* errors.go:46-49 (client side; never produced here) */
    GEVWS_HS_BAD_SEC_KEY = 8,       /* errors.go:50-53 */
    GEVWS_HS_BAD_SEC_VERSION = 9,   /* errors.go:54-57 */
    GEVWS_HS_UPGRADE_REQUIRED = 10, /* ErrHandshakeUpgradeRequired (errors.go:66-79): 426 */
    GEVWS_HS_HOOK = 11              /* an Upgrader hook returned an error */
};

/* What a hook returns with a non-zero result: RejectConnectionError(
 * RejectionStatus(code), RejectionReason(reason), RejectionHeader(header))
 * (errors.go:81-129), or with plain = 1 an ordinary Go error whose Error() is
 * `reason` (answered 500 without extra header, ws.go:325-333). */
typedef struct gevws_reject {
    int32_t code;            /* 0 -> 500 (ws.go:331-333) */
    int32_t plain;
    const char *reason;
    uint64_t reason_len;
    const uint8_t *header;   /* raw "Key: value\r\n" lines */
    uint64_t header_len;
} gevws_reject;

/* One parameter of a Sec-WebSocket-Extensions option (httphead.Option). */
typedef struct gevws_ext_param {
    const uint8_t *key;
    uint64_t key_len;
    const uint8_t *value;    /* NULL when the parameter has no value */
    uint64_t value_len;
} gevws_ext_param;

/* The Upgrader's function fields (ws.go:51-153); any may be NULL.  Every
 * argument is valid only until the hook returns.  Hooks returning int: 0 =
 * accept, non-zero = reject with *rej filled (strings copied before return). */
typedef struct gevws_upgrader_hooks {
    void *user;
    /* Protocol (ws.go:51-56): non-zero selects the offered token. */
    int (*protocol)(void *user, const uint8_t *token, uint64_t n);
    /* ProtocolCustom (ws.go:58-61): returns ok; *sel = the selected protocol. */
    int (*protocol_custom)(void *user, gevws_conn *c, const uint8_t *value, uint64_t n,
                           const uint8_t **sel, uint64_t *sel_n);
    /* Extension (ws.go:63-79): non-zero accepts the option. */
    int (*extension)(void *user, const uint8_t *name, uint64_t n, const gevws_ext_param *params,
                     uint32_t n_params);
    /* ExtensionCustom (ws.go:81-84): the header value and the extensions selected
     * so far (response text form) -> ok, *sel = the new selection's text. */
    int (*extension_custom)(void *user, gevws_conn *c, const uint8_t *value, uint64_t n,
                            const uint8_t *cur, uint64_t cur_n, const uint8_t **sel, uint64_t *sel_n);
    /* OnRequest (ws.go:97-106), OnHost (ws.go:108-121), OnHeader (ws.go:123-133). */
    int (*on_request)(void *user, gevws_conn *c, const uint8_t *uri, uint64_t n, gevws_reject *rej);
    int (*on_host)(void *user, gevws_conn *c, const uint8_t *host, uint64_t n, gevws_reject *rej);
    int (*on_header)(void *user, gevws_conn *c, const uint8_t *key, uint64_t kn, const uint8_t *value,
                     uint64_t vn, gevws_reject *rej);
    /* OnBeforeUpgrade (ws.go:135-153): 0 and optionally extra response header
     * lines in (*hdr, *hdr_len), or non-zero + *rej. */
    int (*on_before_upgrade)(void *user, gevws_conn *c, const uint8_t **hdr, uint64_t *hdr_len,
                             gevws_reject *rej);
} gevws_upgrader_hooks;

/* Upgrade's result: ws.Handshake (ws.go:40-47) plus the error.  Pointers are
 * owned by the connection and valid until its next handshake call. */
typedef struct gevws_handshake {
    const uint8_t *protocol;
    uint64_t protocol_len;
    const uint8_t *extensions;   /* as written in Sec-WebSocket-Extensions */
    uint64_t extensions_len;
    int32_t error;               /* GEVWS_HS_* */
    int32_t http_code;           /* 101, the error response status, or 0: nothing written */
    const char *reason;          /* err.Error(); "" on success */
} gevws_handshake;

typedef struct gevws_upgrader gevws_upgrader;

/* &ws.Upgrader{} -- immutable once configured, so one upgrader may serve every loop. */
gevws_upgrader *gevws_upgrader_new(void);
void gevws_upgrader_free(gevws_upgrader *u);
/* Upgrader.Header (ws.go:88-95) as raw header lines. */
void gevws_upgrader_set_header(gevws_upgrader *u, const uint8_t *hdr, uint64_t n);
void gevws_upgrader_set_hooks(gevws_upgrader *u, const gevws_upgrader_hooks *hooks);
/* Upgrader.Upgrade(c, in) (ws.go:158-343): consumes the request head from `in`
 * once it is complete; (*out, *out_len) = the 101 or error response (owned by
 * `c`; empty when the reference writes none).  GEVWS_OK or GEVWS_ERR_HANDSHAKE. */
int gevws_upgrader_upgrade(const gevws_upgrader *u, gevws_conn *c, gevws_ring *in, const uint8_t **out,
                           uint64_t *out_len, gevws_handshake *hs);
/* The connection's last handshake result (after UnPacket ran the upgrade). */
int gevws_conn_handshake(const gevws_conn *c, gevws_handshake *hs);
const char *gevws_handshake_error_string(int hs_error);
/* initAcceptFromNonce (nonce.go:23-39): 24-byte key -> 28-byte Sec-WebSocket-Accept. */
void gevws_accept_key(const uint8_t nonce[24], char accept[28]);
/* websocket.New(u) (protocol.go:22-24): UnPacket on a connection that is not
 * upgraded runs the handshake (protocol.go:28-37). */
void gevws_protocol_set_upgrader(gevws_protocol *p, const gevws_upgrader *u);

/* websocket.(*Protocol).Packet (protocol.go:67-69): identity. */
const uint8_t *gevws_protocol_packet(gevws_protocol *p, gevws_conn *c, const uint8_t *data,
                                     uint64_t n, uint64_t *out_len);

/* ---------------------------------------------------------------- multi-GPU in one process
 * A gev server drives all its event loops from one process (server.go:80-91):
 * with NumLoops loops placed on the node's GPUs round-robin (loop l on device
 * devices[l % n], one gevws_ctx per loop, load_balance.go:7-14 deals
 * connections to loops), each device decodes only its own loops' connections
 * and the one collective is the all-reduce(sum) of the decoded counts
 *  over RCCL / xGMI -- payloads never cross GPUs.
 * gevws_comm_create: ncclCommInitAll over `devices` (RCCL is loaded on first
 * use; NULL when it is absent or a device is not visible). */
typedef struct gevws_comm gevws_comm;
gevws_comm *gevws_comm_create(const int *devices, int n);
void gevws_comm_destroy(gevws_comm *comm);
int gevws_comm_size(const gevws_comm *comm);
/* For every device i of the communicator: d_counts[i] (int64[3], device
 * memory on device i) = the sum over all devices of {frames, payload_len,
 * errors} of their decode summaries d_summaries[i], enqueued on ctxs[i]'s
 * stream after whatever it holds and after ctxs[i]'s last decode, whichever
 * stream that ran on (one RCCL group, ncclAllReduce in place).
 * ctxs[i] must be on the communicator's device i.  The synchronous form
 * waits and also returns the totals in h_total. */
int gevws_counts_allreduce_async(gevws_comm *comm, gevws_ctx *const *ctxs, const gevws_summary *const *d_summaries,
                                 int64_t *const *d_counts);
int gevws_counts_allreduce(gevws_comm *comm, gevws_ctx *const *ctxs, const gevws_summary *const *d_summaries,
                           int64_t *const *d_counts, int64_t h_total[3]);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* GEVWS_H */
