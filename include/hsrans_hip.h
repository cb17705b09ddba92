/* hsrans_hip.h — C ABI of libhsrans_hip.so: MI355X (gfx950) implementation of the hypersonic-rANS
 * interleaved 32-bit-state / 16-bit-word decode path (rANS32x32 16w, rANS32x64 16w; raw, block_, mt_ containers).
 *
 * The reference (rainerzufalldererste/hypersonic-rANS @ 2024_10_08) has no FFI layer: its boundary is the set of
 * free C++ functions main.cpp stores in codec_info_t (src/main.cpp:146-155):
 *     size_t encode(const uint8_t *in, size_t len, uint8_t *out, size_t outCap, const hist_t *hist);
 *     size_t decode(const uint8_t *in, size_t inLen, uint8_t *out, size_t outCap);      // bytes produced, 0 = failure
 * This header is the C form of exactly that boundary (container / state count / histogram bits become arguments
 * instead of name suffixes) plus what a GPU replacement has to add: a context, a device-pointer
 * entry for device-resident pipelines, and an optional decode plan ("index") that lets many wavefronts work on ONE
 * stream.  include/hsrans_dropin.hpp declares the same functionality under the reference's own C++ names, include/hsrans_names.h
 * under the same names with C linkage (hsrans_<reference name>).
 *
 * Conventions kept from the reference: plain pointers + sizes, caller owns all buffers, return = bytes produced,
 * 0 on any failure, no exceptions cross this boundary, all entry points are re-entrant (per context).
 * The GPU entries (hsrans_decode_host, hsrans_decode_device*, hsrans_hpipe_*, ...) never fall back to the host: without a usable
 * gfx950 device they fail (return 0 / an error code).  The library's own host SIMD decoder sits behind entries that say so in
 * their name — hsrans_decode_cpu, hsrans_index_build_host — and behind the runtime-dispatch names of hsrans_dropin.hpp /
 * hsrans_names.h (`*_decode_auto_N` and the reference's own decoder names), the counterpart of the reference's CPUID dispatch.
 */
#ifndef HSRANS_HIP_H
#define HSRANS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSRANS_RAW 0   /* one histogram, one stream:           src/rANS32x64_16w.cpp, src/rANS32x32_16w.cpp        */
#define HSRANS_BLOCK 1 /* histogram swapped per block, inline: src/block_rANS32x64_16w_{encode,decode}.cpp         */
#define HSRANS_MT 2    /* independent blocks:                  src/mt_rANS32x64_16w_{encode,decode}.cpp            */

/* opaque handles of the GPU side (declared up here so that the host-side prototypes below that take a context are valid C as well) */
typedef struct hsrans_ctx hsrans_ctx;     /* device id, staging buffers, HIP streams/events */
typedef struct hsrans_dplan hsrans_dplan; /* a plan resident in device memory + its status word */

/* = reference hist_t (src/hist.h:16-20) */
typedef struct hsrans_hist
{
  uint16_t symbolCount[256];
  uint16_t cumul[256];
} hsrans_hist;

/* ------------------------------------------------------------------------------------------------------------
 * Host-side format functions (no GPU involved).  The reference's encoders are scalar CPU code too
 * (README.md:19-27 "all encoders scalar"); these produce streams its decoders accept.
 * ---------------------------------------------------------------------------------------------------------- */

/* replaces rANS32x64_16w_capacity (src/rANS32x64_16w.cpp:10), rANS32x32_16w_capacity (src/rANS32x32_16w.cpp:10),
 * block_rANS32x{32,64}_16w_capacity (src/block_rANS32x64_16w_encode.cpp:47), mt_…_capacity (src/mt_rANS32x64_16w_encode.cpp:50) */
size_t hsrans_capacity(int container, int states, size_t input_size);

/* replaces make_hist (src/hist.cpp:217): byte histogram normalised to sum 1 << bits */
void hsrans_make_hist(hsrans_hist *hist, const uint8_t *data, size_t size, uint32_t bits);

/* replaces rANS32x{32,64}_16w_encode_scalar_N (src/rANS32x64_16w.cpp:34), block_…_encode_N
 * (src/block_rANS32x64_16w_encode.cpp:137), mt_…_encode_N (src/mt_rANS32x64_16w_encode.cpp:140).
 * `hist` is used by HSRANS_RAW only (NULL = make_hist over the whole input, as src/main.cpp:746 does). */
size_t hsrans_encode(int container, int states, uint32_t bits, const uint8_t *in, size_t length, uint8_t *out, size_t out_capacity,
                     const hsrans_hist *hist);

typedef struct hsrans_encode_opts
{
  uint32_t block_size;       /* block_/mt_: symbols per block (multiple of 64); 0 = the reference's adaptive block policy      */
  uint32_t index_interval;   /* 0 = no plan; else emit a checkpoint every `index_interval` groups of `states` symbols         */
  uint8_t *plan_out;         /* receives the decode plan (see hsrans_plan_*) when index_interval != 0                         */
  size_t plan_capacity;      /* bytes available at plan_out (hsrans_plan_capacity)                                            */
  size_t plan_size;          /* out: bytes written to plan_out                                                                */
  uint32_t flags;            /* HSRANS_ENC_INDEPENDENT_BLOCKS: mt_ only, needs block_size != 0                                 */
  uint32_t reserved;
  const uint64_t *index_groups; /* optional explicit checkpoints: ascending absolute group indices (multiples of 4), e.g. from    */
  size_t n_index_groups;        /* hsrans_index_boundaries; used instead of index_interval when n_index_groups != 0                */
} hsrans_encode_opts;

/* mt_: start every block from fresh states (2^15) instead of carrying the encoder's states across block boundaries as
 * the reference's encoder does (src/mt_rANS32x64_16w_encode.cpp:220-222 initialises them once).  The stream stays a
 * valid mt_ stream (every block header stores its start states anyway) and the blocks become encodable independently —
 * this is the layout hsrans_encode_device produces, so that the two can be compared byte for byte. */
#define HSRANS_ENC_INDEPENDENT_BLOCKS 1u

/* Checkpoint positions that give the decode kernel exactly ONE chain per resident wavefront, each sized by the wave's
 * scheduling class (what the uniform-interval launch otherwise works out per launch): the smallest sidecar that still
 * fills the GPU — 8,192 checkpoints (2.5 MB) for any stream size on an MI355X, against one per `index_interval` groups
 * (15 MB per 100 MB at 32).  `ctx` NULL = the MI355X defaults (256 CUs), so streams can be indexed where they are
 * encoded.  Writes ascending group indices (multiples of 4) to groups_out and returns their count (0 = one chain is all
 * the stream is good for, or capacity too small); pass them as hsrans_encode_opts::index_groups, to hsrans_index_build_at,
 * or to hsrans_plan_thin.  A plan built for another geometry still decodes correctly, only less evenly. */
size_t hsrans_index_boundaries(const hsrans_ctx *ctx, int states, uint32_t bits, size_t decoded_size, uint64_t *groups_out, size_t capacity);

/* same as hsrans_encode, additionally emitting the sidecar decode plan; the stream bytes are unchanged by it */
size_t hsrans_encode_ex(int container, int states, uint32_t bits, const uint8_t *in, size_t length, uint8_t *out, size_t out_capacity,
                        const hsrans_hist *hist, hsrans_encode_opts *opts);

/* ------------------------------------------------------------------------------------------------------------
 * Decode plans.  A plan lists the independent chains (start states, read cursor, output range, histogram location)
 * one wavefront each will decode.  hsrans_plan_build derives it from the stream alone:
 *   raw    -> 1 chain (the format has no restart points: src/rANS32x64_16w.cpp:223-250 is one dependent chain);
 *   mt_    -> 1 chain per block, by following the header chain like src/mt_rANS32x64_16w_decode.cpp:166-227;
 *   block_ -> 1 chain that parses the inline headers on the device (src/block_rANS32x64_16w_decode.cpp:47-90).
 * A plan emitted by hsrans_encode_ex (or hsrans_index_build) additionally splits chains every `index_interval`
 * groups, which is what lets one stream fill the GPU.  Plans are position-independent byte blobs.
 * ---------------------------------------------------------------------------------------------------------- */
size_t hsrans_plan_capacity(int container, int states, size_t decoded_size, uint32_t index_interval, uint32_t block_size);
/* the same for a plan with `extra_chains` checkpoints (explicit index_groups) */
size_t hsrans_plan_capacity_chains(int container, int states, size_t decoded_size, size_t extra_chains, uint32_t block_size);
size_t hsrans_plan_build(int container, int states, uint32_t bits, const uint8_t *stream, size_t stream_length, size_t out_capacity,
                         uint8_t *plan_out, size_t plan_capacity);
uint32_t hsrans_plan_chain_count(const uint8_t *plan, size_t plan_size);
uint64_t hsrans_plan_decoded_length(const uint8_t *plan, size_t plan_size);
/* restrict a plan to chains [first, first+count): used to shard one stream over several GPUs (each rank decodes its
 * chains into the same output offsets of its own buffer).  Returns bytes written, 0 on error. */
size_t hsrans_plan_slice(const uint8_t *plan, size_t plan_size, uint32_t first_chain, uint32_t chain_count, uint8_t *out, size_t out_capacity);
/* output byte range [*begin, *end) covered by chains [first, first+count) */
int hsrans_plan_chain_range(const uint8_t *plan, size_t plan_size, uint32_t first_chain, uint32_t chain_count, uint64_t *begin, uint64_t *end);
/* Thin a raw-stream plan: keep only the chains that start at (or, when a boundary is not a chain start of `plan`, at the
 * last chain start before) the given ascending group indices, merging everything in between — a finer plan (e.g. one
 * checkpoint per 32 groups, good for any split over GPUs) becomes the one-chain-per-wave plan of one GPU.  Returns bytes
 * written, 0 on error (not a mergeable raw plan, capacity). */
size_t hsrans_plan_thin(const uint8_t *plan, size_t plan_size, const uint64_t *groups, size_t n_groups, uint8_t *out, size_t out_capacity);
/* stream byte ranges chains [first, first+count) can read: ranges = {head_begin, head_end, body_begin, body_end}; head is the
 * shared histogram of a raw stream (empty otherwise), body the chains' own headers and words up to the next chain's first
 * word.  A rank that decodes only these chains needs only these bytes of the stream in its HBM (at their stream offsets). */
int hsrans_plan_stream_ranges(const uint8_t *plan, size_t plan_size, uint32_t first_chain, uint32_t chain_count, uint64_t ranges[4]);

/* ------------------------------------------------------------------------------------------------------------
 * Host SIMD decoders with runtime dispatch (scalar / AVX2 / AVX-512) — the counterpart of the reference's CPU decoders and
 * of its dispatcher block_rANS32x64_decode_wrapper (src/block_rANS32x64_16w_decode.cpp:130-152), written from the format.
 * The GPU cannot speed up a stream that is one dependent chain (raw / block_ without an index: one wavefront, a third of a
 * CPU core); these serve that case in the `*_decode_auto_N` drop-in entries, build indexes of foreign streams faster than
 * one wavefront can, and are the in-run CPU comparator.  The GPU entries below never fall back to them.
 * `level`: 0 scalar, 1 AVX2, 2 AVX-512, -1 = the best this host supports.  `threads` >= 1 (independent chains / mt_ blocks
 * are spread over std::threads like the reference's thread pool, src/mt_rANS32x64_16w_decode.cpp:217-220).
 * ---------------------------------------------------------------------------------------------------------- */
int hsrans_cpu_level(void); /* 0 / 1 / 2: what hsrans_decode_cpu(level = -1) uses here */
/* replaces rANS32x{32,64}_16w_decode_{scalar,avx2_*,avx512_*}_N, block_…_decode_N, mt_…_decode[_mt]_N on the host */
size_t hsrans_decode_cpu(int level, uint32_t threads, int container, int states, uint32_t bits, const uint8_t *in, size_t in_length, uint8_t *out,
                         size_t out_capacity, const uint8_t *plan, size_t plan_size);
/* hsrans_index_build_at without a GPU: one (per mt_ block: parallel) host decode pass that records the checkpoints */
size_t hsrans_index_build_host(int level, uint32_t threads, int container, int states, uint32_t bits, const uint8_t *in, size_t in_length,
                               const uint64_t *groups, size_t n_groups, uint8_t *plan_out, size_t plan_capacity);

/* ------------------------------------------------------------------------------------------------------------
 * GPU side
 * ---------------------------------------------------------------------------------------------------------- */
#define HSRANS_OK 0
#define HSRANS_E_NO_DEVICE 1
#define HSRANS_E_ARG 2
#define HSRANS_E_FORMAT 3   /* malformed stream / plan (the reference's "return 0" cases) */
#define HSRANS_E_HIP 4
#define HSRANS_E_DEVICE 5   /* the kernel reported a malformed histogram / block header, or refused the ranges of a gather_indirect */

int hsrans_ctx_create(int device, hsrans_ctx **out_ctx);
void hsrans_ctx_destroy(hsrans_ctx *ctx);
const char *hsrans_ctx_device_name(const hsrans_ctx *ctx);
/* chains of the index hsrans_decode_host keeps from its last plan-less call (0 = none): see hsrans_decode_host */
uint32_t hsrans_ctx_host_index_chains(hsrans_ctx *ctx);

/* Host-pointer drop-in for decodeFunc (src/main.cpp:149): H2D, plan, launch, D2H.  Replaces
 * rANS32x{32,64}_16w_decode_*_N, block_rANS32x{32,64}_16w_decode_N, mt_rANS32x{32,64}_16w_decode[_mt]_N.
 * Returns the decoded length, 0 on failure. `plan` may be NULL (derived from the stream).
 * With plan == NULL, mt_, block_ and raw streams of >= 1 MiB leave an index behind: the first call's decode records checkpoints (as
 * hsrans_decode_device_indexing) and the context keeps the plan; a later call with the same `in`, in_length and codec launches it
 * — but only counts when the stream's first 128 bytes (compared on the host) and a 64-bit fingerprint of ALL stream bytes, computed on
 * the device beside the decode, equal the first call's (otherwise the call starts over; other bytes at the same address cost one
 * wasted launch).  The fingerprint is a mixing hash, not a MAC: it guards against ACCIDENTAL reuse of a buffer (another file read into
 * the same allocation), where a false match needs a 2^-64 coincidence; bytes crafted to collide with it would decode with the previous
 * stream's checkpoints — memory-safe (every read stays inside in_length) but wrong.  Callers that decode hostile streams through this
 * entry switch the cache off (HSRANS_HOST_INDEX_CACHE_OFF=1) or pass their own plan.  A loop over one file (src/main.cpp:860-889) thus runs the indexed kernels from its second iteration:
 * 100 MB mt_: 0.24 -> 0.06 ms of kernel per call; block_: 153 ms (one wavefront walks the inline headers) -> 0.09 ms; raw: 125 ms -> 0.04 ms (a raw stream's index comes from the host SIMD decoder's
 * pass, ~30 ms for 100 MB, during the first call — the one host-side step of this entry; HSRANS_HIP_STRICT=1: from the wavefront that
 * decodes the stream instead, ~125 ms once).  HSRANS_HOST_INDEX_CACHE_OFF=1 disables the cache: every call decodes what the stream alone
 * allows (a raw stream: one wavefront, k_decode_single). */
size_t hsrans_decode_host(hsrans_ctx *ctx, int container, int states, uint32_t bits, const uint8_t *in, size_t in_length, uint8_t *out,
                          size_t out_capacity, const uint8_t *plan, size_t plan_size);

/* Device-resident entry: everything asynchronous on `hip_stream` (a hipStream_t of the context's device; NULL = default
 * stream), graph-capturable (no allocation, no synchronisation).  `d_stream` must be 16-byte aligned, `d_out` 4-byte aligned.
 * Overlapping launches of ONE device plan (several streams, double-buffered outputs) are fine: plans with one chain per
 * wave (hsrans_index_boundaries) and mt_ plans without checkpoints keep no per-launch state on the device; uniform-interval
 * raw plans and block_/mt_ plans with checkpoints draw work from atomic ticket counters and own 32 sets of them, used round
 * robin, so up to 32 of their launches may be in flight at once — a captured graph node keeps the set it was captured with,
 * so replays of one captured graph must not overlap each other (HIP does not allow a hipGraphExec to run concurrently with
 * itself anyway).  The status word of a plan is shared by all its launches (error bits are only ever OR-ed in;
 * hsrans_dplan_status clears them). */
int hsrans_dplan_create(hsrans_ctx *ctx, const uint8_t *plan, size_t plan_size, hsrans_dplan **out_dplan);
void hsrans_dplan_destroy(hsrans_dplan *dplan);
int hsrans_decode_device(hsrans_ctx *ctx, hsrans_dplan *dplan, const void *d_stream, size_t stream_length, void *d_out, size_t out_capacity,
                         void *hip_stream);
/* The same launch for a caller that holds only a WINDOW of the stream in device memory — the bytes
 * [window_offset, window_offset + window_length) at d_window — e.g. one GPU's share of a stream sharded with
 * hsrans_plan_slice: the window must cover the body range hsrans_plan_stream_ranges reports for the plan's chains
 * (window_offset a multiple of 16, at or below body_begin: HSRANS_E_FORMAT otherwise — the lowest stream byte the plan's
 * chains read is recorded when the device plan is made); a raw stream's shared histogram need not be in it when the plan
 * carries its copy.  Requests beyond the window's end are dropped by the kernel's bounds check, never issued. */
int hsrans_decode_device_window(hsrans_ctx *ctx, hsrans_dplan *dplan, const void *d_window, size_t window_offset, size_t window_length, void *d_out,
                                size_t out_capacity, void *hip_stream);
/* ... and only a WINDOW of the output: d_out_window receives the decoded bytes [out_offset, out_offset + out_length)
 * (out_offset a multiple of 4; the plan's chains must write inside it, hsrans_plan_chain_range: HSRANS_E_FORMAT
 * otherwise).  A rank of a sharded decode then needs neither the whole stream nor the whole output in its HBM: the
 * sender side of the gather in src/mt_rANS32x64_16w_decode.cpp:217-220's fan-out, one GPU per run of blocks. */
int hsrans_decode_device_ranges(hsrans_ctx *ctx, hsrans_dplan *dplan, const void *d_window, size_t window_offset, size_t window_length, void *d_out_window,
                                size_t out_offset, size_t out_length, void *hip_stream);
/* ------------------------------------------------------------------------------------------------------------
 * Random access: byte ranges of a stream that stays compressed in device memory, ONE launch.
 * For every r < count the decoded bytes [ranges[r].offset, + ranges[r].length) of the stream land at
 * (uint8_t *)d_dst + ranges[r].dst_offset; no other byte of d_dst is written.  Only the chains that cover the ranges are
 * decoded: a range is cut into tasks (hsrans_gather_tasks), one wavefront each, and a wave enters the stream at the last
 * chain that starts at or before its task — found on the device, in the device plan; no host copy of the plan is needed —
 * decodes and drops what lies in front of its first byte, stores the rest clipped to the task and stops at its end.
 *   - asynchronous on hip_stream.  `ranges` (host memory) is read before the call returns: the caller may reuse it.
 *     Gathers of one context are ordered among themselves (a gather on another stream waits for the one before it:
 *     they share the context's task buffer).
 *   - d_stream 16-byte aligned, as everywhere.  d_dst and every dst_offset: ANY alignment.  Where a task's destination
 *     is 4-byte aligned against its source (address of d_dst + dst_offset - offset a multiple of 4) whole groups are
 *     stored as words; otherwise, and at a task's first and last group, as bytes.
 *   - ranges may overlap in the source.  Destinations that overlap are the caller's responsibility: which range's
 *     bytes end up in the overlap is unspecified (the bytes of the two ranges differ in general).
 *   - a malformed histogram / header sets the plan's status word as in every decode launch (hsrans_dplan_status).
 * Plans: every plan of planned chains — raw with an index (uniform interval, or hsrans_index_boundaries' device-shaped
 * one), mt_ with and without checkpoints (single-symbol blocks included), block_ with checkpoints, 32 / 64 states,
 * 10-15 bits, made on the host or written on the device (hsrans_encode_device(..., out_dplan),
 * hsrans_decode_device_indexing).  A raw stream WITHOUT an index is one chain: every task is correct and decodes from
 * the stream's first byte.  Plans with a host-built table decode with it (one LDS copy per workgroup), all others build
 * a table per wave from the histogram of the piece they enter.
 * Cost model: a wave decodes its task plus, in front of it, at most the bytes of ONE chain (the distance from the
 * chain's start to the task's first byte) — nothing for tasks that start on a checkpoint.
 * Returns HSRANS_E_ARG: a null handle or pointer, a plan of another context, a misaligned d_stream, a range with
 *   offset + length beyond the plan's decoded bytes or dst_offset + length beyond dst_capacity (nothing is launched);
 * HSRANS_E_FORMAT: a plan without entry points (a block_ stream without checkpoints: its blocks are found by walking
 *   the stream), stream_length != the plan's stream length;
 * HSRANS_OK with nothing launched: count == 0 or only empty ranges. */
typedef struct hsrans_range
{
  uint64_t offset, length, dst_offset;
} hsrans_range; /* 24 bytes */
int hsrans_decode_device_gather(hsrans_ctx *ctx, hsrans_dplan *dplan, const void *d_stream, size_t stream_length, const hsrans_range *ranges /* host */,
                                uint32_t count, void *d_dst, size_t dst_capacity, void *hip_stream);
/* The host-side cut of that call, a pure function (no GPU; for tests and planning, as hsrans_shard_layout and
 * hsrans_launch_choice): one task = one wavefront's work.  Every range is cut at the ABSOLUTE multiples of a segment
 * length L (hsrans_gather_segment): where the plan has a uniform checkpoint interval (PlanHeader::interval, in groups)
 * the base length is interval * states, so tasks start on checkpoints; otherwise the mean chain length
 * ceil(decoded_len / n_chains) rounded up to a multiple of `states`.  L is the smallest multiple of the base that is
 * >= the floor (4096 bytes), so short chains are taken several at a time and a task is never tiny.  Empty ranges give no
 * task; the tasks of a range tile it in order and share dst_delta = dst_offset - offset.
 * Returns the tasks the ranges need and writes at most `capacity` of them (out may be NULL when capacity is 0);
 * 0 for a null `ranges` with count > 0, a range beyond decoded_len, n_chains == 0 or states == 0. */
typedef struct hsrans_gather_task
{
  uint64_t begin, end; /* decoded bytes [begin, end) ... */
  int64_t dst_delta;   /* ... go to d_dst + byte + dst_delta */
} hsrans_gather_task; /* 24 bytes */
uint64_t hsrans_gather_segment(uint64_t decoded_len, uint32_t n_chains, uint32_t states, uint32_t interval /* 0 = none */);
size_t hsrans_gather_tasks(uint64_t decoded_len, uint32_t n_chains, uint32_t states, uint32_t interval /* 0 = none */, const hsrans_range *ranges,
                           uint32_t count, hsrans_gather_task *out, size_t capacity);
/* ------------------------------------------------------------------------------------------------------------
 * The same gather for ranges that are in DEVICE memory — an index lookup, a page table, the output of another kernel —
 * with no host round trip: n = d_count ? *d_count : max_count, and for the ranges d_ranges[0 .. n) the result is byte
 * for byte that of hsrans_decode_device_gather with the same ranges (same segment length L, hence the same tasks
 * hsrans_gather_tasks reports; same alignment rules; no other byte of d_dst is written).
 *   - asynchronous on hip_stream: two kernel launches and nothing else — no allocation, no synchronisation, no lock,
 *     no host read of device memory, no use of the context's task buffer.  The call can be captured into a graph.
 *   - d_ranges and *d_count are read when the launch RUNS, not when it is queued: a replayed graph gathers whatever
 *     they hold then.  Rows of d_ranges from n on are never read.
 *   - d_workspace: hsrans_gather_workspace_bytes(max_count) bytes of device memory, 256-byte aligned, contents
 *     irrelevant.  It belongs to one call in flight at a time; calls with different workspaces are independent of each
 *     other whatever streams they are on (the host-ranges entry orders the gathers of a context; this one does not).
 *   - the launch shape cannot depend on the ranges: the grid is sized from max_count and dst_capacity (no more tasks
 *     than max_count + dst_capacity / L have destinations of their own), capped at the waves the device holds at once,
 *     and the waves stride over the tasks, so any task total finishes.  Pass the dst_capacity the ranges can really
 *     address: a much larger one only starts workgroups that find nothing to do.
 * What only the device can see is checked there, all or nothing: *d_count > max_count, a range beyond the plan's decoded
 * bytes (or outside what a sliced plan decodes), dst_offset + length beyond dst_capacity, any 64-bit overflow in these
 * sums, a task total of 2^31 or more.  Then the call gathers NOTHING — not one byte of d_dst is written — and sets bit 8
 * of the plan's status word: hsrans_dplan_status returns HSRANS_E_DEVICE once and clears it, as for the other bits.
 * Returns HSRANS_E_ARG: a null handle or pointer (d_count may be NULL), a plan of another context, d_stream not 16-byte,
 *   d_ranges not 8-byte, d_count not 4-byte or d_workspace not 256-byte aligned, workspace_bytes too small;
 * HSRANS_E_FORMAT: as hsrans_decode_device_gather;
 * HSRANS_OK with nothing queued: max_count == 0.
 * hsrans_gather_workspace_bytes: a pure function; > 0 and a multiple of 256 for every max_count. */
size_t hsrans_gather_workspace_bytes(uint32_t max_count);
int hsrans_decode_device_gather_indirect(hsrans_ctx *ctx, hsrans_dplan *dplan, const void *d_stream, size_t stream_length,
                                         const hsrans_range *d_ranges /* DEVICE, 8-byte aligned */, const uint32_t *d_count /* DEVICE, or NULL = max_count */,
                                         uint32_t max_count, void *d_dst, size_t dst_capacity, void *d_workspace /* DEVICE, 256-byte aligned */,
                                         size_t workspace_bytes, void *hip_stream);
/* ------------------------------------------------------------------------------------------------------------
 * Byte ranges of MANY streams that stay compressed in device memory: a gather set binds `count` device plans to their
 * streams once, and one call then fetches ranges of any of them — for every r < count the decoded bytes
 * [ranges[r].offset, + ranges[r].length) of member ranges[r].member land at (uint8_t *)d_dst + ranges[r].dst_offset; no
 * other byte of d_dst is written.  Byte for byte what one hsrans_decode_device_gather per member gives with that
 * member's ranges, all into the same d_dst: every member is cut at the segment length L of its single call (a plan
 * made under HSRANS_GATHER_MIN_SEGMENT included), hence into the tasks hsrans_gather_tasks reports for it; the alignment
 * rules and the caller's responsibility for overlapping destinations are the single call's.
 *   - members: d_streams[k] (16-byte aligned, stream_lengths[k] == the plan's stream length) belongs to member k from
 *     hsrans_gather_set_create on; a member cannot be rebound.  A device plan may be a member of any number of sets, may
 *     appear twice in one set and stays usable alone (a gather keeps no per-launch state in a plan).  The plans must
 *     outlive the set and must not be refilled while it exists.  One record per member is uploaded, once, here.
 *   - launches: a member's kind is the decode-table layout its single gather uses — 0..2 a table per wave (bits <= 11,
 *     12, >= 13), 3..5 the plan's host-built table, one copy per workgroup — and a call makes ONE launch per kind that
 *     has tasks: at most six, whatever the number of members or ranges.  In the launches of kinds 3..5 a workgroup
 *     serves one member (hsrans_gather_batch_tasks).
 *   - asynchronous on hip_stream; `ranges` (host memory) is read before the call returns.  The task lists go through the
 *     context's task buffer: gathers of one context, single and batch alike, are ordered among themselves.
 *   - a malformed histogram sets the status word of THAT member's plan; hsrans_gather_set_status synchronises
 *     hip_stream once, fills member_status[members] (may be NULL) with each member's hsrans_dplan_status and returns
 *     the first that is not HSRANS_OK (a plan that is a member twice reports the same code for both).
 * hsrans_gather_set_create returns HSRANS_E_ARG: a null pointer, count == 0 or > 65,536, a plan of another context, a
 *   misaligned stream; HSRANS_E_FORMAT: a plan without entry points, stream_lengths[k] != the plan's stream length.
 * hsrans_decode_device_gather_batch returns HSRANS_E_ARG, nothing launched and nothing uploaded: member >= the set's
 *   members or reserved != 0, a range beyond the member's decoded bytes (or outside what a sliced plan decodes),
 *   dst_offset + length beyond dst_capacity, a null `ranges` with count > 0, 2^31 or more tasks;
 *   HSRANS_OK with nothing launched: count == 0 or only empty ranges. */
typedef struct hsrans_gather_set hsrans_gather_set;
typedef struct hsrans_member_range
{
  uint64_t offset, length, dst_offset;
  uint32_t member, reserved; /* reserved: 0 */
} hsrans_member_range; /* 32 bytes */
typedef struct hsrans_gather_set_info_t
{
  uint32_t members;
  uint32_t launches;         /* of the last hsrans_decode_device_gather_batch on the set (0: none yet, or it had nothing to do) */
  uint32_t kind_members[6];  /* members per kind */
  /* the last call, per kind: its tasks, the entries of its launch (tasks + padding), and the launch's shape */
  uint32_t kind_tasks[6], kind_entries[6], kind_grid[6], kind_waves[6], kind_lds_bytes[6];
} hsrans_gather_set_info_t;
int hsrans_gather_set_create(hsrans_ctx *ctx, hsrans_dplan *const *dplans, const void *const *d_streams, const size_t *stream_lengths,
                             uint32_t count /* 1 .. 65,536 */, hsrans_gather_set **out_set);
void hsrans_gather_set_destroy(hsrans_gather_set *set);
int hsrans_decode_device_gather_batch(hsrans_ctx *ctx, hsrans_gather_set *set, const hsrans_member_range *ranges /* host */, uint32_t count,
                                      void *d_dst, size_t dst_capacity, void *hip_stream);
int hsrans_gather_set_status(hsrans_ctx *ctx, hsrans_gather_set *set, void *hip_stream, int *member_status /* [members] or NULL */);
int hsrans_gather_set_info(const hsrans_gather_set *set, hsrans_gather_set_info_t *info);
/* ------------------------------------------------------------------------------------------------------------
 * The same gather for ranges that are in DEVICE memory — a page-table lookup, a router, a sampler — with no host
 * round trip: n = d_count ? *d_count : max_count, and for the rows d_ranges[0 .. n) the bytes written to d_dst are those
 * hsrans_decode_device_gather_batch writes for the same rows in host memory (every member cut at its own segment
 * length L; same alignment rules; overlapping destinations unspecified; no other byte of d_dst is written).
 *   - asynchronous on hip_stream: kernel launches and nothing else — no allocation, no synchronisation, no lock, no
 *     host read of device memory, no use of the context's task buffer; set->last is not written, so
 *     hsrans_gather_set_info keeps describing the last host-ranges call.  The call can be captured into a graph.
 *   - d_ranges and *d_count are read when the launches RUN: a replayed graph gathers whatever they hold then.  Rows of
 *     d_ranges from n on are never read.
 *   - launches: one cut launch (one workgroup: it checks the rows, sorts them by member and counts their tasks), then
 *     one launch per kind that has MEMBERS, whatever the ranges: at most seven kernels in a line.  In the launches of
 *     kinds 3..5 a workgroup serves whole units — `waves` consecutive tasks of one member — and reloads its table only
 *     where the member changes.  The grids are sized from what the host knows: per kind no more tasks than
 *     max_count + dst_capacity / (the kind's smallest member L) have destinations of their own; capped at the
 *     workgroups the device holds at once, and the kernels loop, so any total finishes.  Pass the dst_capacity the
 *     ranges can really address.
 *   - d_workspace: hsrans_gather_batch_workspace_bytes(the set's members, max_count) bytes of device memory, 256-byte
 *     aligned, contents irrelevant.  It belongs to one call in flight; calls with different workspaces on one set are
 *     independent of each other whatever streams they are on.
 * What only the device can see is checked there, all or nothing: *d_count > max_count, member >= the set's members,
 * reserved != 0, a range beyond its member's decoded bytes (or outside what a sliced plan decodes), dst_offset + length
 * beyond dst_capacity, any 64-bit overflow in these sums, a task total of 2^31 or more.  Then the call gathers NOTHING
 * — not one byte of d_dst is written — and sets bit 8 of a status word the SET owns (no member plan's word is touched):
 * hsrans_gather_set_refused synchronises hip_stream, returns HSRANS_E_DEVICE once and clears the word, else HSRANS_OK.
 * A malformed histogram still reaches the status word of that member's plan only (hsrans_gather_set_status).
 * Returns HSRANS_E_ARG, nothing queued: a null handle or pointer (d_count may be NULL), a set of another context,
 *   d_ranges not 8-byte, d_count not 4-byte or d_workspace not 256-byte aligned, workspace_bytes too small;
 * HSRANS_OK with nothing queued: max_count == 0.
 * hsrans_gather_batch_workspace_bytes: a pure function; > 0 and a multiple of 256 for members in 1 .. 65,536 and every
 *   max_count, non-decreasing in both; 0 for members == 0 or > 65,536.
 * hsrans_gather_set_indirect_info: a pure function of the set, max_count and dst_capacity (no device call) — members
 *   and kind_members, launches = the launches behind the cut, kind_grid / kind_waves / kind_lds_bytes = the shapes the
 *   entry will use (it computes them through the same function); kind_tasks and kind_entries are 0: only the device
 *   knows them. */
size_t hsrans_gather_batch_workspace_bytes(uint32_t members, uint32_t max_count);
int hsrans_decode_device_gather_batch_indirect(hsrans_ctx *ctx, hsrans_gather_set *set, const hsrans_member_range *d_ranges /* DEVICE, 8-byte aligned */,
                                               const uint32_t *d_count /* DEVICE, or NULL = max_count */, uint32_t max_count, void *d_dst, size_t dst_capacity,
                                               void *d_workspace /* DEVICE, 256-byte aligned */, size_t workspace_bytes, void *hip_stream);
int hsrans_gather_set_refused(hsrans_ctx *ctx, hsrans_gather_set *set, void *hip_stream);
int hsrans_gather_set_indirect_info(const hsrans_gather_set *set, uint32_t max_count, size_t dst_capacity, hsrans_gather_set_info_t *info);
/* The host-side cut of hsrans_decode_device_gather_batch, a pure function (no GPU): the task list of ONE kind's launch, in launch order — wave w
 * of workgroup b runs entry b * waves + w.  Every range is cut exactly as hsrans_gather_tasks cuts it for its member
 * (decoded_len, n_chains, states, interval), and the member's number stands beside each task.
 *   kinds 0..2 (a table per wave): the tasks of the ranges whose member is of `kind`, in range order.
 *   kinds 3..5 (one table per workgroup): the same tasks stable-sorted by member, each member's run padded with empty
 *     tasks (begin == end == 0, the same member) up to a multiple of `waves`: every workgroup serves exactly one member.
 *     A member without tasks contributes no entry.
 * Returns the entries of the launch and writes at most `capacity` of them (out may be NULL when capacity is 0); 0 for a
 * null pointer with a count > 0, a range beyond its member's decoded_len, member >= n_members, kind > 5, waves == 0, a
 * range that is not empty on a member with n_chains == 0 or states == 0. */
typedef struct hsrans_gather_member
{
  uint64_t decoded_len;
  uint32_t n_chains, states, interval, kind; /* kind 0..5; 3..5 = shared table */
} hsrans_gather_member; /* 24 bytes */
typedef struct hsrans_gather_batch_task
{
  uint64_t begin, end;
  int64_t dst_delta;
  uint32_t member, reserved;
} hsrans_gather_batch_task; /* 32 bytes */
size_t hsrans_gather_batch_tasks(const hsrans_gather_member *members, uint32_t n_members, const hsrans_member_range *ranges, uint32_t count,
                                 uint32_t kind, uint32_t waves, hsrans_gather_batch_task *out, size_t capacity);

/* Plan an mt_ stream that only exists in device memory: the header chain (src/mt_rANS32x64_16w_decode.cpp:166-227) is
 * followed by a device kernel; synchronises `hip_stream` twice (chain count, then the finished plan).
 * HSRANS_BLOCK: the inline headers are only found by decoding, so the plan is the walk plan hsrans_plan_build makes — from the stream's
 * first 16 + 4 * states bytes, which are copied down (one synchronisation), with hsrans_plan_build's checks of the lengths against
 * stream_length and out_capacity; hsrans_decode_device_indexing turns it into a plan with entry points.  HSRANS_RAW: HSRANS_E_ARG
 * (hsrans_plan_build needs nothing but the header either: copy it down). */
int hsrans_dplan_create_from_device_stream(hsrans_ctx *ctx, int container, int states, uint32_t bits, const void *d_stream, size_t stream_length,
                                           size_t out_capacity, void *hip_stream, hsrans_dplan **out_dplan);
/* copies the plan blob a dplan holds in device memory back to the host (inspection / tests); returns its size, 0 on error */
size_t hsrans_dplan_read_plan(hsrans_dplan *dplan, uint8_t *out, size_t capacity);
/* synchronises `hip_stream` and returns HSRANS_OK or HSRANS_E_DEVICE (kernel found a bad histogram/header) */
int hsrans_dplan_status(hsrans_ctx *ctx, hsrans_dplan *dplan, void *hip_stream);

/* ------------------------------------------------------------------------------------------------------------
 * K independent streams, ONE launch.  The reference decodes independent work from one pool — a task per mt_ block on its
 * thread pool (src/mt_rANS32x64_16w_decode.cpp:182-224), file after file in its benchmark loop (src/main.cpp:841-898); on the
 * GPU the pool is the device's resident wave slots.  One launch per stream pays the launch's prologue, tail and kernel boundary
 * (~11 of ~41 us for a 100 MB stream) K times, and launches put on several HIP streams cannot co-reside (every plan is shaped
 * to fill the device).  A batch deals the wave slots of ONE launch to its members — whole workgroups (a workgroup holds one
 * decode table), in proportion to the members' sizes, each member's chains cut into runs sized by the slots' scheduling
 * class — so the three are paid once.  Members keep their own device plans, status words and results.  block_/mt_ members with
 * checkpoints (64 states, <= 12 bits) share a launch of their own kind: all their blocks in one list, a workgroup per block and round —
 * many small streams then fill the device together instead of each launching a mostly empty one.  Raw members come in four kinds
 * with a shared kernel each (64 states <= 12 bits; 32 states <= 12 bits; 64 states 13 bits; 64 states 14-15 bits): a call makes one
 * launch per kind present.  A member no shared kernel takes (an un-indexed stream, a lone member of its kind) gets its own launch
 * behind them, in the same call.
 * Best served: raw streams of <= 12 bits (64 states, or 32: a launch per state count) with a uniform index
 * (hsrans_encode_opts::index_interval: any mix of sizes), with the index shaped for the batch (hsrans_index_boundaries_batch), or with
 * the one-chain-per-wavefront index of a launch of their own (hsrans_index_boundaries) when the members are 1, 2 or 4 of one size.
 * The dplans must outlive the batch and must not be refilled while it exists; a dplan belongs to at most one member.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct hsrans_batch hsrans_batch;
int hsrans_dplan_batch_create(hsrans_ctx *ctx, hsrans_dplan *const *dplans, uint32_t count, hsrans_batch **out_batch);
void hsrans_dplan_batch_destroy(hsrans_batch *batch);
/* member k: stream d_streams[k] (16-byte aligned, stream_lengths[k] bytes) -> d_outs[k] (4-byte aligned, out_capacities[k]).
 * Asynchronous on `hip_stream`, no allocation, no synchronisation; nothing is launched unless every member's arguments pass. */
int hsrans_decode_device_batch(hsrans_ctx *ctx, hsrans_batch *batch, const void *const *d_streams, const size_t *stream_lengths, void *const *d_outs,
                               const size_t *out_capacities, void *hip_stream);
/* synchronises `hip_stream`; member_status[k] (may be NULL) = hsrans_dplan_status of member k; returns the first failure or HSRANS_OK */
int hsrans_dplan_batch_status(hsrans_ctx *ctx, hsrans_batch *batch, void *hip_stream, int *member_status);
typedef struct hsrans_batch_info
{
  uint32_t members, launches;            /* kernel launches one hsrans_decode_device_batch call makes */
  uint32_t direct_members, solo_members; /* members in the shared one-chain-per-wave launch(es) / with a launch of their own */
  uint32_t grouped_members, groups;      /* block_/mt_ members with checkpoints sharing a grouped launch (one per histogram width); the groups (blocks,
                                          * parts of blocks, runs of single-symbol blocks) of the first grouped launch: more than its grid = by ticket */
  uint32_t grid, block, lds_bytes;       /* the (first) shared launch: the one-chain-per-wave one, or the grouped one where there is none */
  uint32_t class_weights[8];             /* one-chain-per-wave launch only (else 0): per-mille run lengths of the 8 wave scheduling classes it was dealt with */
  double imbalance;                      /* one-chain-per-wave launches only (else 0): the most loaded wave slot (groups / class weight) over the mean: 1.0 = all waves end together */
} hsrans_batch_info;
int hsrans_dplan_batch_info(const hsrans_batch *batch, hsrans_batch_info *info);
/* hsrans_index_boundaries for a stream that will be decoded as member `member` of a batch of `count` streams of the given decoded
 * sizes: exactly one chain per wave slot the batch launch deals that member (8,192 / count each for streams of one size: the sidecar
 * shrinks with the batch), sized by the slots' scheduling classes at the batch's run length.  64 states, bits 10..15, or 32 states, bits
 * 10..12 (the sizes given are those of the members of the same kind: see hsrans_dplan_batch_create).  A batch of
 * plans made this way is dealt without rounding (hsrans_batch_info::imbalance ~ 1.00); the plans still decode alone, or in another
 * batch, only less evenly.  32 states: two chains per wave slot.  Returns the number of group indices written (0 = one chain, or
 * capacity too small). */
size_t hsrans_index_boundaries_batch(const hsrans_ctx *ctx, int states, uint32_t bits, const size_t *decoded_sizes, uint32_t count, uint32_t member,
                                     uint64_t *groups_out, size_t capacity);
/* The dealing alone, without a device (tests, planning): members' chain starts in groups (chain_starts[m][0 .. n_chains[m]], the last
 * entry = all the member's groups) -> slots_out[4 * (wg * waves + wave)] = {member, first chain, end chain, flags}; returns the
 * imbalance (see above), < 0 on bad arguments.  weights NULL = the MI355X defaults of the 64-state launch. */
double hsrans_batch_deal(const uint64_t *const *chain_starts, const uint32_t *n_chains, uint32_t members, uint32_t grid, uint32_t waves, const uint32_t *weights,
                         uint32_t *slots_out);
/* diagnostics: with HSRANS_BATCH_STAMPS=1 in the environment when the batch is made, every wave of its first shared launch leaves
 * its finish time (100 MHz) in slot wg * waves + wave, the launch's first wave its entry time in the slot after the last */
size_t hsrans_dplan_batch_read_finish(hsrans_batch *batch, uint64_t *out, size_t capacity_u64);

/* ------------------------------------------------------------------------------------------------------------
 * Open-ended submission: streams that arrive one by one.  The reference's pool takes tasks as they come (thread_pool_add,
 * src/thread_pool.cpp:124-133) and its benchmark loop hands it file after file (src/main.cpp:841-898, :163-170); hsrans_dplan_batch_create
 * wants all members at once.  A queue collects submissions on the host (a submit launches nothing, except that the `max_members`-th
 * pending one flushes) and hsrans_queue_flush decodes everything pending with ONE batch launch.  What a batch costs to make (about a
 * millisecond) is paid once per shape: the queue keeps the last 8 batches it made; the same device plans in the same order reuse theirs
 * as it is, and OTHER raw plans of the same shapes (same decoded size and index geometry: a loop over files of one size class) reuse
 * its dealing — only a 64-byte record per member is rewritten, asynchronously in front of the launch.  Use one `hip_stream` per queue
 * at a time.  The buffers must stay valid until the flush's launch has run; per-member results: hsrans_dplan_status on the plans.
 * A plan submitted again while it is still pending flushes first (a plan is one member of a launch).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct hsrans_queue hsrans_queue;
typedef struct hsrans_queue_stats_t
{
  uint64_t submitted, flushes, launches; /* kernel launches made by the flushes */
  uint64_t batches_made, batches_reused; /* flushes that had to make a batch / found theirs in the cache */
  uint64_t retargeted;                   /* ... of the reused ones: with other plans of the same shapes */
} hsrans_queue_stats_t;
int hsrans_queue_create(hsrans_ctx *ctx, uint32_t max_members /* 1..32 */, hsrans_queue **out_queue);
void hsrans_queue_destroy(hsrans_queue *queue); /* synchronises the device */
int hsrans_queue_submit(hsrans_queue *queue, hsrans_dplan *dplan, const void *d_stream, size_t stream_length, void *d_out, size_t out_capacity, void *hip_stream);
int hsrans_queue_flush(hsrans_queue *queue, void *hip_stream); /* asynchronous on hip_stream; nothing pending: HSRANS_OK, nothing launched */
uint32_t hsrans_queue_pending(const hsrans_queue *queue);
int hsrans_queue_stats(const hsrans_queue *queue, hsrans_queue_stats_t *out);

/* ------------------------------------------------------------------------------------------------------------
 * ONE stream over the GPUs of a node: one process per GPU, the plan's chains cut into one contiguous run per rank, the decoded
 * ranges exchanged point to point over xGMI (RCCL ncclSend / ncclRecv groups on the communicator's own HIP stream), pipelined behind
 * the decode in `parts` sub-runs.  This is the C form of the reference's thread-pool fan-out behind the `thread_pool *` argument of
 * mt_rANS32x64_16w_decode_mt_N (src/mt_rANS32x64_16w.h:23-28): blocks handed to workers (src/mt_rANS32x64_16w_decode.cpp:217-220),
 * joined by thread_pool_await (:262) — a worker is a GPU, a block a chain, the join the exchange.  RCCL is bound at run time
 * (the librccl the process already carries, else the system's); without one these entries return HSRANS_E_NO_DEVICE.
 * Rendezvous: rank 0 calls hsrans_comm_unique_id and ships the 128 bytes to the other ranks by whatever it has (MPI, a file, a
 * socket); every rank then calls hsrans_comm_create with the same bytes (collective: returns when all `world` ranks have called).
 * ---------------------------------------------------------------------------------------------------------- */
#define HSRANS_COMM_ID_BYTES 128
typedef struct hsrans_comm hsrans_comm;
int hsrans_comm_unique_id(uint8_t id[HSRANS_COMM_ID_BYTES]);
int hsrans_comm_create(hsrans_ctx *ctx, const uint8_t id[HSRANS_COMM_ID_BYTES], int rank, int world, hsrans_comm **out_comm);
void hsrans_comm_destroy(hsrans_comm *comm);
int hsrans_comm_rank(const hsrans_comm *comm);
int hsrans_comm_world(const hsrans_comm *comm);
int hsrans_comm_rccl_version(void); /* 0: no RCCL could be bound */

/* Which chains / output bytes / stream bytes each rank owns, and how each rank's run is cut into `parts` sub-runs: pure host
 * arithmetic, identical on every rank, no GPU and no RCCL involved.  The chains are cut into `world` contiguous runs whose decoded
 * bytes follow `weights` (NULL = equal shares; e.g. a larger share for the rank a gather goes to, which sends nothing), every run
 * into `parts` sub-runs of equal decoded bytes.  shards[rank * parts + k] = sub-run k of `rank`; windows (may be NULL) receives
 * {begin, end} of the stream bytes each rank's chains read (begin aligned down to 16: hsrans_decode_device_window). */
typedef struct hsrans_shard
{
  uint32_t first_chain, chain_count; /* chain_count 0: nothing (fewer chains than sub-runs) */
  uint64_t out_begin, out_end;       /* decoded bytes [out_begin, out_end) */
} hsrans_shard;
int hsrans_shard_layout(const uint8_t *plan, size_t plan_size, uint32_t world, uint32_t parts, const double *weights, hsrans_shard *shards /* [world * parts] */,
                        uint64_t *windows /* [2 * world] or NULL */);

/* Everything that does not change between decodes of one (plan, communicator) pair, prepared once: this rank's sub-runs as device
 * plans, its stream window, the output bytes it holds.  root < 0: every rank ends with the whole output; root >= 0: that rank only
 * (the others then hold just their own range: out_base / out_length below). */
typedef struct hsrans_sharded hsrans_sharded;
int hsrans_sharded_create(hsrans_ctx *ctx, hsrans_comm *comm, const uint8_t *plan, size_t plan_size, uint32_t parts, const double *weights, int root,
                          hsrans_sharded **out_sharded);
/* one rank's share WITHOUT a communicator (decode only: hsrans_decode_sharded with HSRANS_SHARD_DECODE_ONLY) — a consumer that is
 * sharded like the decode, or tests that run every rank's GPU side on one GPU */
int hsrans_sharded_create_rank(hsrans_ctx *ctx, int rank, int world, const uint8_t *plan, size_t plan_size, uint32_t parts, const double *weights, int root,
                               hsrans_sharded **out_sharded);
void hsrans_sharded_destroy(hsrans_sharded *sharded);
typedef struct hsrans_sharded_info_t
{
  uint32_t world, rank, parts;
  int32_t root;
  uint64_t window_begin, window_end; /* stream bytes this rank must hold at d_window (d_window[0] = stream byte window_begin) */
  uint64_t out_base, out_length;     /* output bytes this rank's d_out holds (d_out[0] = output byte out_base) */
  uint64_t decoded_length, stream_length;
  uint32_t one_launch, reserved;     /* 1: this rank's sub-runs are decoded by ONE launch that publishes a completion word per sub-run */
} hsrans_sharded_info_t;
int hsrans_sharded_info(const hsrans_sharded *sharded, hsrans_sharded_info_t *info, hsrans_shard *shards /* [world * parts] or NULL */, size_t shard_capacity);
hsrans_dplan *hsrans_sharded_part_plan(hsrans_sharded *sharded, uint32_t part); /* this rank's sub-run `part` (launch info, status); NULL: no chains, or one launch for all */
hsrans_dplan *hsrans_sharded_whole_plan(hsrans_sharded *sharded);               /* this rank's whole run when ONE launch decodes all its sub-runs; NULL otherwise */
/* One decode of the stream: this rank's sub-runs are queued on `hip_stream`; with gather != 0 sub-run k's ranges go onto the links
 * (the communicator's stream waits for exactly that sub-run) while sub-run k + 1 decodes, and `hip_stream` continues when
 * the transfers are done.  block_/mt_ plans with checkpoints (64 states, <= 16 sub-runs): the sub-runs are ONE launch — every block of
 * the rank's run handed to the device in one pass, as src/mt_rANS32x64_16w_decode.cpp:182-224 hands them to its pool — that publishes a
 * completion word per sub-run, and the communicator's stream waits for the word (hipStreamWaitValue32); other plans, or
 * HSRANS_SHARD_ONE_LAUNCH=0 in the environment at hsrans_sharded_create: a launch per sub-run, an event behind each.  A receiving root posts all its receives first.  Asynchronous; collective when gather != 0 (every rank
 * of the communicator must make the same call). */
#define HSRANS_SHARD_DECODE_ONLY 0         /* every rank keeps its range */
#define HSRANS_SHARD_DECODE_AND_EXCHANGE 1 /* the step: decode, ranges exchanged behind it */
#define HSRANS_SHARD_EXCHANGE_ONLY 2       /* the ranges of an earlier decode-only call (to time the two legs apart) */
int hsrans_decode_sharded(hsrans_sharded *sharded, const void *d_window, void *d_out, int gather, void *hip_stream);
/* Makes `hip_stream` (another stream than the decode's) wait until sub-run `part` of the LAST hsrans_decode_sharded call queued on this
 * object is decoded and its bytes are visible device-wide — what the exchange does internally, for a consumer that is sharded like the
 * decode and can start on a sub-run while the next one is still being decoded (a worker of the reference's pool picking up finished
 * blocks: src/thread_pool.cpp:124-133).  One launch for all sub-runs: waits for the sub-run's completion word; else for its event. */
int hsrans_sharded_wait_part(hsrans_sharded *sharded, uint32_t part, void *hip_stream);
int hsrans_sharded_status(hsrans_sharded *sharded, void *hip_stream); /* as hsrans_dplan_status, over this rank's sub-runs */

/* First decode of a stream that came WITHOUT an index (e.g. a reference-emitted mt_ stream: one chain per block,
 * src/mt_rANS32x64_16w_decode.cpp:137-265 decodes it with one thread per block): decodes like hsrans_decode_device with
 * `dplan` (from hsrans_plan_build + hsrans_dplan_create, or from hsrans_dplan_create_from_device_stream; HSRANS_RAW,
 * HSRANS_MT and HSRANS_BLOCK, no checkpoints yet) and records the coder states and read cursor every `index_interval` groups
 * (multiple of 4) on the way.  *indexed receives a device plan with those checkpoints (the blob hsrans_index_build would return
 * for the same stream and interval) for every later decode of the same stream.  Synchronises `hip_stream`.  d_out is complete on
 * return.  HSRANS_E_DEVICE: the pass found a malformed stream (status cleared), *indexed is NULL, d_out is unspecified.
 * A block_ stream comes with its walk plan: the one wavefront that follows the inline headers (block_rANS32x64_16w_decode.cpp:47-123)
 * also records every block header and the states it enters the block with, and the plan — one chain per block and per checkpoint —
 * and its group list are assembled on the device behind it.  HSRANS_E_FORMAT with d_out COMPLETE and *indexed NULL: the stream
 * holds more than decoded_len / 4096 + 16 blocks, or ends in a single-symbol block with a partial group behind it — the cases in
 * which hsrans_index_build returns 0; decode it with the walk plan.  HSRANS_INDEX_ASSEMBLE_ON_HOST=1 (read at hsrans_ctx_create):
 * the records come down and the host writes the same blob (mt_ and block_; the comparison path). */
int hsrans_decode_device_indexing(hsrans_ctx *ctx, hsrans_dplan *dplan, const void *d_stream, size_t stream_length, void *d_out, size_t out_capacity,
                                  uint32_t index_interval, void *hip_stream, hsrans_dplan **indexed);

/* The first decode of many streams that came without an index, in one call: the many-streams form of hsrans_decode_device_indexing.
 * The walks of different block_ streams, and the blocks of mt_ base plans, are independent: each is one wavefront of one launch.
 *
 * Member equivalence.  Member k gets exactly what hsrans_decode_device_indexing(ctx, dplan, d_stream, stream_length, d_out,
 * out_capacity, index_interval, hip_stream, &indexed) gives it: the same bytes at d_out, the same plan blob byte for byte
 * (hsrans_dplan_read_plan; hence the blob hsrans_index_build returns), the same group list (hence the same hsrans_dplan_launch_info)
 * and the same rc.
 * Mixing.  HSRANS_BLOCK walk plans and HSRANS_MT base plans may share one call, with 32 and 64 states, 10-15 bits and different
 * intervals.  count is 1..65,536.
 * Validation before launch.  Every member is checked with the single call's rules before anything is launched or allocated.  Besides:
 * a dplan appears at most once; no two members' [d_out, d_out + decoded_len) overlap; no output overlaps any member's stream
 * [d_stream, d_stream + stream_length); a raw member (and an mt_ plan that carries its histogram, which the single call also indexes on
 * the host) is an argument error here: raw streams are indexed on the host and gain nothing from the batch.  Any violation returns
 * HSRANS_E_ARG or HSRANS_E_FORMAT as the single call would, with nothing launched, no byte written, every rc set to that code and every
 * `indexed` NULL.  (NULL ctx or members, count == 0 or > 65,536: HSRANS_E_ARG, members untouched.)
 * Failure on the device is per member.  A member whose pass sets its status word gets rc = HSRANS_E_DEVICE, indexed = NULL and its
 * status word cleared.  A member whose walk overflows the block list or ends short gets rc = HSRANS_E_FORMAT, indexed = NULL and d_out
 * COMPLETE.  In both cases the other members complete normally.  The call returns the first non-OK rc in member order, else HSRANS_OK.
 * (HSRANS_E_HIP: the runtime failed; every rc is HSRANS_E_HIP.)
 * Synchronisation.  One hipStreamSynchronize of hip_stream, plus one more only when some member's status word has to be cleared.  All
 * members' results, status words and (64 states) group lists come down in front of that one synchronisation.
 * Launch count.  Independent of count: the recording pass launches at most once per private table layout present (<= 11 bits, 12 bits,
 * 13-15 bits: at most 3), count and fill each at most once per kind (walk, mt_: at most 4); stats->launches <= 7, plus one upload,
 * one memset and the copies down.  Its tasks (a walk, or one mt_ block) are ordered by descending work: the decoded bytes of a walk, of
 * an mt_ block its member's average block length.
 * Host work per member: its validation and parameter records, and one plan allocation with its memset (as the single call).  The
 * members' checkpoints are carved out of the context's checkpoint buffer, which grows to the sum over all members.
 * HSRANS_INDEX_ASSEMBLE_ON_HOST=1 (read at hsrans_ctx_create): the single call's body runs member by member behind the same validation
 * (the comparison path): the same results, stats->launches == 0.  Calls on one context are serialised. */
typedef struct hsrans_indexing_member
{
  hsrans_dplan *dplan;      /* base plan, as hsrans_decode_device_indexing takes it: a block_ walk plan or an mt_ base plan (no checkpoints) */
  const void *d_stream;     /* device, 16-byte aligned */
  size_t stream_length;
  void *d_out;              /* device, 4-byte aligned */
  size_t out_capacity;
  uint32_t index_interval;  /* multiple of 4, != 0; members may differ */
  int rc;                   /* out: what the single call would have returned for this member */
  hsrans_dplan *indexed;    /* out: the plan with checkpoints, NULL unless rc == HSRANS_OK */
} hsrans_indexing_member;
typedef struct hsrans_indexing_batch_stats
{
  uint32_t launches, walk_members, mt_members, tasks; /* kernels launched; members by kind; wavefront tasks of the recording pass */
} hsrans_indexing_batch_stats;
int hsrans_decode_device_indexing_batch(hsrans_ctx *ctx, hsrans_indexing_member *members, uint32_t count, void *hip_stream,
                                        hsrans_indexing_batch_stats *stats /* may be NULL */);

/* GPU encoder: mt_ stream with fixed blocks of `block_size` symbols (multiple of 64), each block
 * encoded independently by one wavefront (HSRANS_ENC_INDEPENDENT_BLOCKS layout).  d_in / d_out are device pointers (16-byte
 * aligned); d_out needs hsrans_capacity(HSRANS_MT, states, length) bytes.  Synchronises `hip_stream`; returns the stream
 * size, 0 on failure.  Byte-identical to hsrans_encode_ex(HSRANS_MT, ..., {block_size, index_interval, flags =
 * HSRANS_ENC_INDEPENDENT_BLOCKS}), stream and plan.
 * out_dplan != NULL: the stream's decode plan is written on the device as well — one chain per block plus one per
 * checkpoint every `index_interval` groups inside the blocks (multiple of 4; 0 = block starts only), the encoder passes
 * through exactly those states — and returned as a device plan for hsrans_decode_device (hsrans_dplan_read_plan fetches
 * the blob).  Nothing leaves HBM between encode and decode. */
size_t hsrans_encode_device(hsrans_ctx *ctx, int container, int states, uint32_t bits, const void *d_in, size_t length, void *d_out, size_t out_capacity,
                            uint32_t block_size, uint32_t index_interval, void *hip_stream, hsrans_dplan **out_dplan);

/* Every format hsrans_encode_ex writes, on the GPU: the same arguments, the same stream bytes at d_out, the same plan blob at
 * opts->plan_out (opts->plan_size set) when opts asks for an index; out_dplan != NULL also returns that plan as a device plan for
 * hsrans_decode_device.  What hsrans_encode_ex refuses, this call refuses too (0, nothing launched).  d_in / d_out are device
 * pointers, 16-byte aligned; `hist` is used by HSRANS_RAW only (as hsrans_encode_ex).  Synchronises `hip_stream`.
 *   HSRANS_RAW: hsrans_encode_device_raw.  HSRANS_MT with fixed HSRANS_ENC_INDEPENDENT_BLOCKS and no index: hsrans_encode_device.
 *   Otherwise (block_ and mt_, the reference's adaptive blocks with block_size == 0 or fixed blocks, the states carried from block
 *   to block as the reference's encoders carry them): the per-unit byte counts are taken on the device, the host walks the block
 *   policy over them (the host encoder's own code), and ONE wavefront codes the blocks back to front — the carried states make the
 *   whole input one dependent chain, like the raw format.
 *   Independent mt_ blocks with index_interval also take the one-wave-per-block launch (its plan is copied back); with index_groups
 *   they take the one-wavefront chain (fresh states per block): about 1 GB/s instead of hundreds.
 * Limits: length <= 2^31 - 2^16 (as hsrans_encode_device_raw); index_groups with fixed blocks need block_size / states to be a
 * multiple of 4 (checkpoints are taken between sets of four groups); both refused with 0.  Any block_size that is a multiple of 64
 * is accepted (one longer than the input makes one block). */
size_t hsrans_encode_device_ex(hsrans_ctx *ctx, int container, int states, uint32_t bits, const void *d_in, size_t length, void *d_out, size_t out_capacity,
                               const hsrans_hist *hist, hsrans_encode_opts *opts, void *hip_stream, hsrans_dplan **out_dplan);
/* The block choice behind block_ / mt_ streams (block_size 0: the reference's adaptive policy; else fixed blocks), as the host
 * encoder makes it and as hsrans_encode_device_ex makes it from device-side unit summaries: blocks in stream order, `counts` the
 * normalised histogram a block is coded with (zero for single-symbol blocks).  Returns the number of blocks (only the first
 * `capacity` are written), 0 on bad arguments.  For inspection and tests; the device variant synchronises `hip_stream`. */
typedef struct hsrans_block_choice
{
  uint64_t begin, end;
  uint32_t single, symbol;
  uint16_t counts[256];
} hsrans_block_choice;
size_t hsrans_block_choices(int container, int states, uint32_t bits, const void *in, size_t length, uint32_t block_size, hsrans_block_choice *out, size_t capacity);
size_t hsrans_block_choices_device(hsrans_ctx *ctx, int container, int states, uint32_t bits, const void *d_in, size_t length, uint32_t block_size,
                                   hsrans_block_choice *out, size_t capacity, void *hip_stream);

/* The raw format on the GPU (replaces src/rANS32x64_16w.cpp:34-166 `rANS32x64_16w_encode_scalar_N` / src/rANS32x32_16w.cpp for
 * data that lives in HBM): the format carries every coder state from the last symbol to the first, so it
 * is ONE wavefront's work — about 3.5x one host core, not a throughput kernel; mt_ (hsrans_encode_device) is the format to encode
 * at HBM rates.  `hist` NULL: the histogram of the input is counted and normalised on the device (what make_hist gives); else the
 * caller's normalised counts are used (they must sum to 1 << bits), as the reference's encode signature passes them.
 * The sidecar index: a checkpoint every `index_interval` groups, or at `index_groups` (hsrans_index_boundaries) when
 * n_index_groups != 0; the plan goes to plan_out (host; *plan_size receives its size; hsrans_plan_capacity[_chains]) and/or is
 * returned as a device plan.  Stream and plan are byte-identical to hsrans_encode_ex's.  length <= 2^31 - 2^16.
 * hsrans_encode_device(HSRANS_RAW, ...) is this call with hist = NULL and a uniform interval.  Returns the stream length, 0 on failure. */
size_t hsrans_encode_device_raw(hsrans_ctx *ctx, int states, uint32_t bits, const void *d_in, size_t length, void *d_out, size_t out_capacity, const hsrans_hist *hist,
                                uint32_t index_interval, const uint64_t *index_groups, size_t n_index_groups, uint8_t *plan_out, size_t plan_capacity,
                                size_t *plan_size, void *hip_stream, hsrans_dplan **out_dplan);

/* Many independent streams encoded on the GPU at once: the encode-side twin of hsrans_decode_device_batch.
 *
 * Member equivalence.  Member k gets exactly what it would get from its single call on `hip_stream`: the same stream bytes at d_out,
 * the same stream_length, and in out_dplans[k] (when out_dplans != NULL) the device plan that call returns in *out_dplan (NULL where
 * it returns none).
 *   HSRANS_RAW: hsrans_encode_device_raw(ctx, states, bits, d_in, length, d_out, out_capacity, hist, index_interval, index_groups,
 *               n_index_groups, NULL, 0, NULL, hip_stream, out_dplans ? &p : NULL) — a plan only with an index (interval or groups).
 *   HSRANS_MT:  hsrans_encode_device(ctx, HSRANS_MT, states, bits, d_in, length, d_out, out_capacity, block_size, index_interval,
 *               hip_stream, out_dplans ? &p : NULL) — fixed blocks of block_size symbols, each from fresh states.
 * Mixing.  Raw and mt_ members, 32 and 64 states and every bit width may share one call; count is 1..65,536.
 * Validation before launch.  Every member is checked with its single call's rules before anything is launched; besides, no two
 * members' output ranges [d_out, d_out + out_capacity) may overlap, and no output range may overlap any member's input range
 * [d_in, d_in + length).  hist, index_groups and n_index_groups belong to HSRANS_RAW members (NULL / 0 otherwise), block_size to
 * HSRANS_MT members (0 for raw).  HSRANS_BLOCK members, mt_ members with carried states or adaptive blocks (block_size 0) and anything
 * else a check refuses: HSRANS_E_ARG, nothing launched, no output byte changed, every stream_length 0.
 * Failure on the device.  The only one: a raw member whose caller hist gives no slot to a byte that occurs.  That member gets
 * stream_length 0 and a NULL plan; the others complete; the call returns HSRANS_E_DEVICE.  (HSRANS_E_HIP: the runtime failed.)
 * Synchronisation.  Synchronises hip_stream: every output is complete on return (twice when mt_ plans are made: their chain counts
 * are needed before the plans are written on the device; and once more per mt_ plan with checkpoints, whose group list is read back
 * as the single call reads it).
 * Launch count.  Independent of count: each kernel kind launches at most once per (kind, state count, chunk variant) present —
 * the raw histograms, the mt_ block histograms, the raw coding wavefronts per state count, the mt_ coding wavefronts per state count
 * (one chunk variant for the whole batch, chosen from its total block count), the mt_ size scan (only for members of more than 4,096
 * blocks), the mt_ gather, the raw image copy, and the mt_ plans (only when asked for): at most 10 kernels, plus one memset and the
 * copies of the members' parameters and results.  stats->launches counts the kernels.
 * Host work per member: its validation and parameter record; with out_dplans, per raw member with an index its plan is assembled on
 * the host (as the single call does) and uploaded by hsrans_dplan_create (one device allocation), and per mt_ member one plan
 * allocation, one memset and one header upload; raw members' headers and checkpoints come down in one copy for all of them.
 * The members' scratch (slots, result words, checkpoints) is carved out of the context's encode buffers, which grow to the sum over
 * all members: a raw member needs about 2 x length, an mt_ member 2 x block_size per block.  Calls on one context are serialised.
 * Limits: the single calls' (raw length <= 2^31 - 2^16), and fewer than 2^24 mt_ blocks and 2^24 raw 64 KiB parts in one call. */
typedef struct hsrans_encode_member
{
  int container, states;       /* HSRANS_RAW or HSRANS_MT (fixed, independent blocks); 32 or 64 */
  uint32_t bits;               /* 10..15 */
  uint32_t block_size;         /* HSRANS_MT: symbols per block, multiple of 64; HSRANS_RAW: must be 0 */
  const void *d_in;            /* device, 16-byte aligned */
  size_t length;
  void *d_out;                 /* device, 16-byte aligned, out_capacity >= hsrans_capacity(container, states, length) */
  size_t out_capacity;
  const hsrans_hist *hist;     /* HSRANS_RAW only, may be NULL (as hsrans_encode_device_raw) */
  uint32_t index_interval;     /* checkpoints for the member's plan, multiple of 4, 0 = none */
  const uint64_t *index_groups; /* HSRANS_RAW only (e.g. hsrans_index_boundaries_batch) */
  size_t n_index_groups;
  size_t stream_length;        /* out: bytes written to d_out, 0 = this member failed */
} hsrans_encode_member;
typedef struct hsrans_encode_batch_stats
{
  uint32_t launches, raw_members, mt_members, mt_blocks;
} hsrans_encode_batch_stats;
int hsrans_encode_device_batch(hsrans_ctx *ctx, hsrans_encode_member *members, uint32_t count, void *hip_stream, hsrans_dplan **out_dplans,
                               hsrans_encode_batch_stats *stats);

/* Many block_ and carried-state mt_ streams encoded on the GPU at once: hsrans_encode_device_ex's chain path for many streams, the
 * encode-side twin of hsrans_decode_device_indexing_batch.  A stream of these formats is one dependent chain — one wavefront — at
 * any size; the chains of different streams are independent and run side by side.
 *
 * Member equivalence.  Member k gets exactly what hsrans_encode_device_ex(ctx, container, states, bits, d_in, length, d_out,
 * out_capacity, NULL, opts, hip_stream, out_dplans ? &p : NULL) gives it: the same bytes at d_out, the same returned length in
 * stream_length, the same blob at opts->plan_out with the same opts->plan_size, and in out_dplans[k] a device plan over that blob
 * (NULL where the single call returns none: no index asked for).  Stream and plan are byte for byte hsrans_encode_ex's.
 * Which members.  Those the single call sends to its chain: every HSRANS_BLOCK member; HSRANS_MT with carried states, adaptive
 * (block_size == 0) or fixed blocks; HSRANS_MT with HSRANS_ENC_INDEPENDENT_BLOCKS and listed checkpoints (index_groups).  HSRANS_RAW
 * members and independent fixed mt_ blocks with index_interval or with no index belong to hsrans_encode_device_batch and get
 * HSRANS_E_ARG here, as that call refuses these.  32 and 64 states, every bit width, adaptive and fixed blocks, members with and
 * without an index may share one call; count is 1..65,536.
 * Validation before launch.  Every member is checked with hsrans_encode_device_ex's rules (length <= 2^31 - 2^16; index_groups with
 * fixed blocks need block_size / states to be a multiple of 4; ...).  Besides: no two members' [d_out, d_out + out_capacity) may
 * overlap, no output may overlap any member's [d_in, d_in + length), and no two members may share an opts object or a plan_out range.
 * Any violation: HSRANS_E_ARG, nothing launched, no output byte changed, every stream_length 0, every rc HSRANS_E_ARG, every
 * plan_size 0, every out_dplans[k] NULL.  A NULL ctx or members, count == 0 or count > 65,536: HSRANS_E_ARG (the members are left
 * untouched where they cannot be read).
 * Failure after launch is per member.  A member whose plan does not fit plan_capacity — known after its walk — gets rc =
 * HSRANS_E_ARG, stream_length 0, plan_size 0, a NULL plan, and is left out of the coding launch: its d_out stays untouched.  A member
 * whose result words report an internal inconsistency gets HSRANS_E_DEVICE.  The others complete.  The call returns the first rc
 * that is not HSRANS_OK, in member order.  HSRANS_E_HIP: the runtime failed; every rc is HSRANS_E_HIP, and the call returns after
 * everything it queued has drained.
 * Synchronisation.  Two hipStreamSynchronize(hip_stream), whatever count: behind the summaries (the host walks need them) and behind
 * the coding and gather.  The image sizes and offsets, block states, checkpoint states and positions of all members lie next to each
 * other and come down in front of the second one in two copies; no blocking copy per member.  With out_dplans, each member with an
 * index costs one hsrans_dplan_create (one allocation, one upload), as the single call does.
 * Launch count.  Independent of count, at most 5 kernels: the unit summaries (one launch over all (member, unit) tasks), the unit
 * costs (one over the adaptive members' whole units; none when no member is adaptive or none has a whole unit), the coding wavefronts (one per state count
 * present: a workgroup of one wavefront per member, the longest first), the gather (one over all (member, block, part) tasks);
 * plus one upload of the members' records in front of each phase and the copies down.  stats->launches counts the kernels.
 * Host work.  The block walks run member by member on the calling thread (stats->walk_us).  With HSRANS_DEBUG_STAMPS=1 (read at
 * hsrans_ctx_create) the call prints one line with its four phase times.
 * Memory.  The context's encode buffers grow to the sum over all members: slots of about 2 x length each, 1,040 bytes per summary
 * unit, the per-block records and checkpoints.  Calls on one context are serialised.
 * Limits: the single call's, and fewer than 2^24 summary units and 2^24 gather workgroups in one call (HSRANS_E_ARG). */
typedef struct hsrans_encode_ex_member
{
  int container, states;      /* HSRANS_BLOCK or HSRANS_MT; 32 or 64 */
  uint32_t bits;              /* 10..15 */
  const void *d_in;           /* device, 16-byte aligned */
  size_t length;
  void *d_out;                /* device, 16-byte aligned, out_capacity >= hsrans_capacity(container, states, length) */
  size_t out_capacity;
  hsrans_encode_opts *opts;   /* as hsrans_encode_device_ex takes it; may be NULL (adaptive blocks, no index); plan_size is set */
  size_t stream_length;       /* out: bytes written to d_out, 0 = this member failed */
  int rc;                     /* out: HSRANS_OK, or why stream_length is 0 */
} hsrans_encode_ex_member;
typedef struct hsrans_encode_ex_batch_stats
{
  uint32_t launches, block_members, mt_members, units, blocks; /* kernels launched; members by container; summary units; coded + single-symbol blocks */
  double summaries_us, walk_us, chain_us, plans_us;            /* host clock: up to the first synchronisation; the host walks; up to the second; the plans */
} hsrans_encode_ex_batch_stats;
int hsrans_encode_device_ex_batch(hsrans_ctx *ctx, hsrans_encode_ex_member *members, uint32_t count, void *hip_stream,
                                  hsrans_dplan **out_dplans /* [count] or NULL */, hsrans_encode_ex_batch_stats *stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------------------------
 * Multi-byte elements coded as byte planes.  What lies in HBM is mostly tensors of 2-, 4- or 8-byte elements; coded as they lie,
 * bytes of very different statistics share one histogram (a bf16 value's sign/exponent byte carries ~2.6 bits, its mantissa byte
 * ~8).  Each byte position coded as a stream of its own never costs entropy (entropy is concave in the histogram) and usually
 * gains.
 *
 * Layout.  An element is W = elem_size bytes, W in {2, 4, 8}.  Plane p is the byte at memory offset p of every element, in
 * element order: plane[p][i] = in[i * W + p].  Memory order: the library takes no view on endianness or dtype.
 * A frame is ONE device buffer that holds the W planes at offsets known before encoding:
 *   offset[p] = p * up256(hsrans_capacity(HSRANS_MT, states, elements))        (up256: rounded up to a multiple of 256)
 * A plane is coded — an mt_ stream of independent fixed blocks, exactly what hsrans_encode_device(HSRANS_MT, ...) writes for the
 * plane's bytes — or stored: its `elements` bytes verbatim (stored_mask).
 * Decision: the descriptor is a host struct and the frame carries no header of its own; keeping or serialising the descriptor is
 * the caller's business, like the plan blobs.
 *
 * The split (elements -> planes) and the merge (planes -> elements) are streaming kernels of their own, in front of the existing
 * batch encoder and behind the existing batch decoder: neither codec kernel changes, and hsrans_decode_device_planes costs one
 * pass over the decoded bytes more than hsrans_decode_device_batch of the same plans.
 * ---------------------------------------------------------------------------------------------------------- */
#define HSRANS_PLANES_MAX 8
#define HSRANS_PLANES_STORE_INCOMPRESSIBLE 1u /* flags: a plane whose stream is not shorter than its bytes is stored verbatim */
typedef struct hsrans_planes_desc
{
  uint32_t elem_size, states, bits, block_size, index_interval;
  uint32_t stored_mask; /* bit p: plane p is stored, not coded */
  uint64_t elements;
  uint64_t offset[HSRANS_PLANES_MAX], length[HSRANS_PLANES_MAX]; /* inside the frame; entries >= elem_size are 0 */
  uint64_t frame_length;                                         /* end of the last plane's data */
} hsrans_planes_desc;
/* host arithmetic, no device; 0 on bad arguments (elem_size not 2, 4 or 8; states not 32 or 64; elements 0) */
size_t hsrans_planes_capacity(uint32_t elem_size, int states, size_t elements); /* the frame's bytes */
size_t hsrans_planes_workspace_bytes(uint32_t elem_size, size_t elements);      /* elem_size * up256(elements) */
/* the layout on the host, in plain C++: planes[p] (elements bytes each) <-> in / out (elem_size * elements bytes); HSRANS_OK or HSRANS_E_ARG */
int hsrans_planes_split(uint32_t elem_size, const void *in, size_t elements, uint8_t *const *planes);
int hsrans_planes_merge(uint32_t elem_size, const uint8_t *const *planes, size_t elements, void *out);
/* the two kernels alone.  d_planes: a HOST array of elem_size device pointers.  Asynchronous on `hip_stream`, no allocation, no
 * synchronisation.  Every pointer is 16-byte aligned; the planes must not overlap each other or the element buffer. */
int hsrans_planes_split_device(hsrans_ctx *ctx, uint32_t elem_size, const void *d_in, size_t elements, void *const *d_planes, void *hip_stream);
int hsrans_planes_merge_device(hsrans_ctx *ctx, uint32_t elem_size, const void *const *d_planes, size_t elements, void *d_out, void *hip_stream);
/* d_in (elem_size * elements bytes) -> a frame at d_frame: one split launch into d_work, ONE hsrans_encode_device_batch of the
 * elem_size planes as mt_ members, and with HSRANS_PLANES_STORE_INCOMPRESSIBLE a device-to-device copy over every plane whose
 * stream_length >= elements (exactly this comparison; without the flag nothing is stored).  *desc describes the frame;
 * out_dplans[p] (when out_dplans != NULL) is plane p's device plan, NULL for a stored plane.  Returns desc->frame_length, 0 on
 * failure.  Synchronises `hip_stream`, like every encoder here.  A plane that hsrans_encode_device cannot encode (its stream does not
 * fit hsrans_capacity: uniform bytes in 16 KiB blocks at 10 bits) fails the call, whatever the flags.
 * Refused before anything is launched or written (0): a NULL ctx, desc or pointer; elem_size not 2, 4 or 8; states not 32 or 64;
 * bits outside 10..15; block_size 0 or not a multiple of 64; index_interval not a multiple of 4; elements 0 or beyond
 * hsrans_encode_device's limit; unknown flags; a pointer that is not 16-byte aligned; frame_capacity < hsrans_planes_capacity or
 * work_bytes < hsrans_planes_workspace_bytes; any intersection among the element buffer, the frame and the workspace. */
size_t hsrans_encode_device_planes(hsrans_ctx *ctx, uint32_t elem_size, int states, uint32_t bits, const void *d_in, size_t elements, void *d_frame,
                                   size_t frame_capacity, uint32_t block_size, uint32_t index_interval, uint32_t flags, void *d_work, size_t work_bytes,
                                   void *hip_stream, hsrans_planes_desc *desc, hsrans_dplan **out_dplans /* [elem_size] or NULL */);
/* The decode side: a frame's descriptor bound to its planes' device plans.  dplans[p] is NULL exactly for the stored planes; every
 * other one is a plan of this context over `elements` decoded bytes and length[p] stream bytes with the descriptor's states and
 * bits, and appears once.  One hsrans_batch is made over the coded planes (none when all are stored).  The dplans must outlive
 * the object.  The descriptor's offsets may be any multiples of 16 whose ranges [offset, offset + up16(length)) do not overlap
 * and end within up16(frame_length): a caller may have compacted the frame. */
typedef struct hsrans_planes hsrans_planes;
int hsrans_planes_create(hsrans_ctx *ctx, const hsrans_planes_desc *desc, hsrans_dplan *const *dplans, hsrans_planes **out_planes);
void hsrans_planes_destroy(hsrans_planes *planes);
/* frame -> d_out (elem_size * elements bytes): hsrans_decode_device_batch of the coded planes into d_work, then ONE merge launch
 * behind it on the same stream; a stored plane is read by the merge straight from the frame (neither a decode nor a copy).
 * Asynchronous on `hip_stream`, no allocation, no synchronisation; nothing is launched unless every argument passes (pointers
 * set and 16-byte aligned; frame_length >= the descriptor's; out_capacity >= elem_size * elements; work_bytes >=
 * hsrans_planes_workspace_bytes; frame, output and workspace disjoint): HSRANS_E_ARG otherwise. */
int hsrans_decode_device_planes(hsrans_ctx *ctx, hsrans_planes *planes, const void *d_frame, size_t frame_length, void *d_out, size_t out_capacity,
                                void *d_work, size_t work_bytes, void *hip_stream);
/* hsrans_dplan_batch_status over the coded planes (synchronises `hip_stream`); stored planes report HSRANS_OK */
int hsrans_planes_status(hsrans_ctx *ctx, hsrans_planes *planes, void *hip_stream, int *plane_status /* [elem_size] or NULL */);
typedef struct hsrans_planes_info_t
{
  uint32_t coded, stored; /* planes */
  uint32_t launches;      /* kernels of one hsrans_decode_device_planes: the batch's launches + the merge */
} hsrans_planes_info_t;
int hsrans_planes_info(const hsrans_planes *planes, hsrans_planes_info_t *info);
/* ------------------------------------------------------------------------------------------------------------
 * Many tensors' frames in one call — a checkpoint's parameters, a layer's experts, the pages of a cache — as the codec
 * batches stand to their single calls: K tensors pay the split, the codec batch, the store and the merge once, not K times.
 *
 * Member equivalence.  Member k of hsrans_encode_device_planes_batch gets byte for byte what hsrans_encode_device_planes
 * gives it with the same arguments (its own frame, and its region of the workspace as d_work): the same frame bytes, the same
 * desc, the same stored planes (stream_length >= elements, by the member's own flags) and the same plans, at
 * out_dplans[HSRANS_PLANES_MAX * k + p] — NULL for a stored plane and for p >= elem_size.  frame_length is desc.frame_length.
 * elem_size, states, bits, block_size, index_interval and flags may differ from member to member.
 * Workspace, a pure function of the shapes: member k's region starts at the sum of the earlier members'
 * hsrans_planes_workspace_bytes (multiples of 256) and holds plane p at p * up256(elements), as the single call's.
 * hsrans_planes_batch_workspace_bytes is that sum; 0 for count 0, a NULL array, a member whose own value is 0, or an overflow.
 * Tasks.  The split and the merge are one launch each over all members, one workgroup per task: member k's tasks are the
 * workgroups of its single launch, max(1, ceil(floor(elements / 16) / 256)).  hsrans_planes_batch_tasks writes their exclusive
 * prefix and total to first_task[0 .. count] (may be NULL) and returns the total; 0 for a NULL `elements`, count 0, a member
 * with 0 elements or more than 2^42, or a total of 2^31 or more (one launch's limit: the entries refuse by this same function).
 * Launches, independent of count: one split launch, ONE hsrans_encode_device_batch over all the planes as mt_ members
 * (through that public entry: its launch count, limits and synchronisations are that call's), one store launch that copies the
 * stored planes from the workspace into their frames (none when nothing is stored), one settle of the stream behind it.  The
 * member table goes up in one copy, the store's records in one more; both pass through the context's task buffers (below).
 * stats: launches = the planes kernels + the codec batch's; members; planes = the sum of elem_size; stored.
 * Validation before anything is launched or written.  HSRANS_E_ARG: a NULL ctx or members, count 0; any member that
 * hsrans_encode_device_planes refuses (see there); d_work NULL or not 16-byte aligned; work_bytes below
 * hsrans_planes_batch_workspace_bytes; more than 65,536 planes or 2^24 mt_ blocks or more in all (the codec batch's limits);
 * 2^31 tasks or more; any intersection in which a written span takes part among the members' element buffers (read), their
 * frames over frame_capacity and the workspace over work_bytes (written).  Then every frame_length is 0, every desc zero, every
 * plan NULL and no device byte has changed; rc is HSRANS_E_ARG for the members whose own arguments were refused.
 * Failure after launch.  Whatever makes hsrans_encode_device_batch return other than HSRANS_OK — a plane whose stream outgrows
 * hsrans_capacity, as in the single call; the runtime — fails the whole call with that code: every frame_length 0, every desc
 * zero, every rc that code, the plans destroyed.  The workspace and the frames may have been written.
 * Synchronisation.  hsrans_encode_device_planes_batch synchronises hip_stream, like every encoder here.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct hsrans_planes_member
{
  uint32_t elem_size;      /* 2, 4 or 8 */
  int states;              /* 32 or 64 */
  uint32_t bits;           /* 10..15 */
  uint32_t block_size, index_interval, flags; /* as hsrans_encode_device_planes */
  const void *d_in;        /* device, 16-byte aligned, elem_size * elements bytes */
  size_t elements;
  void *d_frame;           /* device, 16-byte aligned, frame_capacity >= hsrans_planes_capacity(elem_size, states, elements) */
  size_t frame_capacity;
  hsrans_planes_desc desc; /* out */
  size_t frame_length;     /* out: desc.frame_length, 0 = the call failed */
  int rc;                  /* out: HSRANS_OK, or why this member made the call fail */
} hsrans_planes_member;
typedef struct hsrans_planes_batch_stats
{
  uint32_t launches, members, planes, stored;
} hsrans_planes_batch_stats;
size_t hsrans_planes_batch_workspace_bytes(const uint32_t *elem_sizes, const size_t *elements, uint32_t count);
size_t hsrans_planes_batch_tasks(const size_t *elements, uint32_t count, uint32_t *first_task /* [count + 1] or NULL */);
int hsrans_encode_device_planes_batch(hsrans_ctx *ctx, hsrans_planes_member *members, uint32_t count, void *d_work, size_t work_bytes, void *hip_stream,
                                      hsrans_dplan **out_dplans /* [count * HSRANS_PLANES_MAX] or NULL */, hsrans_planes_batch_stats *stats /* may be NULL */);
/* The decode side: `count` descriptors bound to their planes' device plans, dplans[HSRANS_PLANES_MAX * k + p] plane p of
 * member k.  Every member is checked by hsrans_planes_create's rules (HSRANS_E_ARG); ONE hsrans_batch is made over all coded
 * planes of all members, in member and plane order (none when every plane is stored); a plan that appears twice is refused as
 * hsrans_dplan_batch_create refuses it.  The plans must outlive the set.
 * hsrans_decode_device_planes_batch: member k's frame d_frames[k] -> d_outs[k] (elem_size * elements bytes).  ONE
 * hsrans_decode_device_batch of all coded planes into d_work (the encoder's layout), then ONE merge launch over all members
 * behind it on the same stream; stored planes are read by the merge straight from their frames.  Asynchronous on hip_stream,
 * no device allocation, no synchronisation.  Launch count: the batch's + 1, as hsrans_planes_set_info reports it — not a
 * constant: the codec batch packs at most 32 grouped members into one launch (kBatchMax), so a set of many coded planes
 * takes ceil(planes / 32) grouped launches per histogram width, and members no shared kernel takes (no checkpoints) one each.
 * The per-call member table (the frames' and outputs' addresses) goes up through a region of the context's task buffers, as
 * hsrans_decode_device_planes_gather sends its tasks: the arrays are read before the call returns, no allocation beyond what
 * that buffer does, and the call is ordered with the other gathers of the context.
 * HSRANS_E_ARG, nothing launched: a NULL handle or array, a set of another context; any d_frames[k], d_outs[k] or d_work NULL
 * or not 16-byte aligned; frame_lengths[k] below the descriptor's; out_capacities[k] < elem_size * elements; work_bytes below
 * the set's (hsrans_planes_set_info: hsrans_planes_batch_workspace_bytes of its members); any intersection in which an output
 * or the workspace takes part among all frames over frame_lengths (read; frames may share), all outputs over out_capacities
 * and the workspace over work_bytes (written).  HSRANS_E_HIP (the runtime refused an upload or a launch) may leave the
 * workspace written and the outputs not.
 * hsrans_planes_set_status synchronises hip_stream; member_status[k] is the status of member k's first failing plane, or
 * HSRANS_OK; returns the first failure.  With no batch it only settles the stream.
 * Limits: the codec batches' (65,536 planes, fewer than 2^24 mt_ blocks per encode) and fewer than 2^31 tasks per launch. */
typedef struct hsrans_planes_set hsrans_planes_set;
int hsrans_planes_set_create(hsrans_ctx *ctx, const hsrans_planes_desc *descs, hsrans_dplan *const *dplans /* [count * HSRANS_PLANES_MAX] */, uint32_t count,
                             hsrans_planes_set **out);
void hsrans_planes_set_destroy(hsrans_planes_set *set);
typedef struct hsrans_planes_set_info_t
{
  uint32_t members, coded, stored; /* members; planes of all members */
  uint32_t launches;               /* kernels of one hsrans_decode_device_planes_batch: the batch's launches + the merge */
  uint32_t merge_tasks, reserved;  /* workgroups of the merge launch */
  size_t work_bytes;               /* the workspace a decode needs */
} hsrans_planes_set_info_t;
int hsrans_planes_set_info(const hsrans_planes_set *set, hsrans_planes_set_info_t *info);
int hsrans_decode_device_planes_batch(hsrans_ctx *ctx, hsrans_planes_set *set, const void *const *d_frames, const size_t *frame_lengths, void *const *d_outs,
                                      const size_t *out_capacities, void *d_work, size_t work_bytes, void *hip_stream);
int hsrans_planes_set_status(hsrans_ctx *ctx, hsrans_planes_set *set, void *hip_stream, int *member_status /* [count] or NULL */);
/* ------------------------------------------------------------------------------------------------------------
 * Many streams, or many frames, into one exact-size arena.  The encoders leave every stream in a buffer of hsrans_capacity
 * bytes and every frame in one of hsrans_planes_capacity bytes — more than the tensor, with gaps between short streams; what
 * makes the coded size the size in HBM is one more step: the streams' bytes side by side in a buffer of exactly their sum.
 * These entries are that step, in ONE launch whatever the count, where a caller would otherwise queue a device copy per
 * stream and rewrite every descriptor.  Two layers, as elsewhere: the codec's streams, and the element layer's frames.
 *
 * Streams.  Layout, a pure function of the lengths: offsets[0] = 0, offsets[k + 1] = offsets[k] + up16(lengths[k]) (up16:
 * rounded up to a multiple of 16); hsrans_pack_layout writes offsets[0 .. count] (may be NULL) and returns offsets[count], the
 * arena's exact size.  0 for a NULL array, count 0, a length of 0, more than 524,288 items (65,536 members x
 * HSRANS_PLANES_MAX, the planes sets' limit) or an overflow.
 * No slack behind the last item: no decode or gather kernel here fetches a stream byte at or beyond up16(length) of its
 * stream.  Stream words are fetched through a buffer descriptor that begins on a 16-byte boundary of the stream and whose
 * range ends at the stream's length rounded up to 16 (win_open, csrc/kernels_common.h: a 16-byte request that straddles the
 * range is dropped as a whole) — the gathers' prologues open the same window (ring_init, csrc/kernels_gather.h) — and the one
 * wavefront that loads words itself tests each against the length (csrc/kernels_single.h); histograms and block headers are
 * read only where they end within the length.  So a stream may end next to another stream or at the end of an allocation.
 * Tasks.  One launch, one workgroup per task: item k's tasks are the chunks of HSRANS_PACK_CHUNK bytes of its up16(length)
 * bytes, ceil(up16(lengths[k]) / HSRANS_PACK_CHUNK).  hsrans_pack_tasks writes their exclusive prefix and total to
 * first_task[0 .. count] (may be NULL) and returns the total; 0 under the layout's conditions and for a total of 2^31 or more
 * (one launch's limit).  The entry refuses by these same two functions.
 * hsrans_pack_device: for every k the bytes [d_srcs[k], + lengths[k]) land at (uint8_t *)d_arena + offsets[k], and the bytes
 * from there up to up16(lengths[k]) are written as zero: an arena is a pure function of its items' bytes and can be compared
 * or hashed.  No byte at or behind d_srcs[k] + lengths[k] is read; no byte of the arena outside [0, offsets[count]) is
 * written.  A caller who packs in several calls — one chunk of a checkpoint at a time — passes d_arena + its running offset.
 * Validation before anything is launched or written.  HSRANS_E_ARG: a NULL ctx, array or arena; a layout or task count of 0;
 * any d_srcs[k] or d_arena NULL or not 16-byte aligned; arena_capacity < offsets[count]; any intersection between
 * [d_arena, + arena_capacity) and a source [d_srcs[k], + lengths[k]).  Sources may overlap each other (they are only read);
 * packing in place is not supported.
 * Synchronisation.  Asynchronous on hip_stream: no synchronisation, and no device allocation beyond what the context's task
 * buffer does.  The item table goes up through a region of that buffer in one copy, as hsrans_decode_device_planes_batch
 * sends its member table: the arrays are read before the call returns, and the call is ordered with the context's gathers.
 * HSRANS_E_HIP: the runtime refused the upload or the launch; nothing was written.
 *
 * Frames.  hsrans_planes_pack_layout: out_descs[k] is descs[k] with offset[p] = the sum of up16(length[q]) over q < p (member-
 * relative, the planes in order) and frame_length = offset[W - 1] + length[W - 1]; bases[0] = 0 and bases[k + 1] = bases[k] +
 * the sum of up16(length[p]) over member k's planes.  Member k's packed frame is (uint8_t *)d_arena + bases[k] — 16-byte
 * aligned — and has out_descs[k].frame_length bytes; every entry that takes a descriptor and a frame pointer takes
 * out_descs[k] with that pointer (hsrans_planes_create, hsrans_planes_set_create, both gather creators; the plans are those
 * of the unpacked frame: a plan knows its stream, not where it lies).  Returns bases[count], the arena's bytes; out_descs and
 * bases may be NULL, and out_descs may be descs itself.  The layout is idempotent: of its own output it returns the same.
 * A descriptor is checked by hsrans_planes_create's rules without the plans — elem_size 2, 4 or 8; offsets that are multiples
 * of 16; lengths that are not 0; ranges [offset, offset + up16(length)) that do not overlap; frame_length not below the last
 * byte of a plane — and the layout returns 0, with nothing written, for anything else, for a NULL descs, count 0, more than
 * 65,536 members, or an overflow.  Every descriptor it accepts is a valid source: an encoder's, one the caller compacted, one
 * that came out of an earlier pack — packing the survivors of one arena into another is this same call.
 * hsrans_planes_pack_device: the layout, then hsrans_pack_device's launch over all planes of all members, in member and
 * plane order, plane p of member k read at (uint8_t *)d_frames[k] + descs[k].offset[p]: one launch for the whole set, stored
 * planes and coded planes alike.  out_descs and bases (may be NULL) get the layout's.  Asynchronous as above.
 * HSRANS_E_ARG with nothing launched and nothing written, and out_descs zeroed: a NULL ctx, array, arena or out_descs; a
 * layout or task count of 0; any d_frames[k] or d_arena NULL or not 16-byte aligned; frame_lengths[k] < descs[k].frame_length;
 * arena_capacity below the layout's; any intersection of [d_arena, + arena_capacity) with a frame [d_frames[k], +
 * frame_lengths[k]).  out_descs is zeroed on HSRANS_E_HIP too.
 * Limits: 524,288 items, 65,536 members, fewer than 2^31 tasks per launch.
 * ---------------------------------------------------------------------------------------------------------- */
#define HSRANS_PACK_CHUNK 8192 /* bytes one workgroup moves */
size_t hsrans_pack_layout(const size_t *lengths, uint32_t count, uint64_t *offsets /* [count + 1] or NULL */);
size_t hsrans_pack_tasks(const size_t *lengths, uint32_t count, uint32_t *first_task /* [count + 1] or NULL */);
int hsrans_pack_device(hsrans_ctx *ctx, const void *const *d_srcs, const size_t *lengths, uint32_t count, void *d_arena, size_t arena_capacity, void *hip_stream);
size_t hsrans_planes_pack_layout(const hsrans_planes_desc *descs, uint32_t count, hsrans_planes_desc *out_descs /* [count] or NULL */,
                                 uint64_t *bases /* [count + 1] or NULL */);
int hsrans_planes_pack_device(hsrans_ctx *ctx, const hsrans_planes_desc *descs, const void *const *d_frames, const size_t *frame_lengths, uint32_t count,
                              void *d_arena, size_t arena_capacity, void *hip_stream, hsrans_planes_desc *out_descs /* [count] */,
                              uint64_t *bases /* [count + 1] or NULL */);
/* ------------------------------------------------------------------------------------------------------------
 * Element ranges of a frame that stays compressed in device memory — embedding rows, one expert's slice, pages of a cache.
 * For every r < count the elements [ranges[r].offset, + ranges[r].length) of the tensor land at
 * (uint8_t *)d_out + ranges[r].dst_offset * elem_size; no other byte of d_out is written.  All three fields of hsrans_range
 * are in ELEMENTS here.  Ranges may overlap in the source; destinations that overlap are the caller's responsibility; an
 * empty range does nothing (hsrans_decode_device_gather's rules).
 * hsrans_planes_gather_create binds a hsrans_planes object to the frame it will read and makes ONE hsrans_gather_set over
 * the coded planes — member k is the k-th coded plane, its stream d_frame + desc.offset[p], desc.length[p] bytes — and none
 * when every plane is stored.  The planes object, its plans and the frame must outlive the gather object.  Returns
 * HSRANS_E_ARG: a null argument, a planes object of another context, d_frame not 16-byte aligned, frame_length below the
 * descriptor's; HSRANS_E_FORMAT: as hsrans_gather_set_create (a plan without entry points).
 * The call: one hsrans_decode_device_gather_batch on the set (count x coded rows) that fetches the coded planes' bytes into
 * d_work, then ONE merge launch behind it on the same stream that interleaves the fetched bytes with the stored planes'
 * bytes, read straight from the frame.  Asynchronous on hip_stream; `ranges` (host memory) is read before the call returns;
 * no allocation beyond what the context's task buffer does.  The merge's tasks go through that buffer like the gather's:
 * the call is ordered with the other gathers of the context.
 * Workspace layout, a pure function of the ranges: with phase = offset & 15 a non-empty range r has the slot
 * [B_r, B_r + up16(phase + length)) of every plane's region, B_r = the sum of the earlier slots; the regions lie
 * up256(sum of all slots) apart, region p at d_work + p * that; the byte of plane p of element offset + i is at
 * region p + B_r + phase + i.  A 16-element block of the tensor is thus aligned alike in the workspace and in a stored
 * plane, and every gather row is 16-byte aligned against its source (the gather's word stores).  Slot bytes outside
 * [phase, phase + length) and the regions of stored planes are never written.
 * hsrans_planes_gather_workspace_bytes = elem_size * up256(total_elements + 30 * count): enough for every `count` ranges of
 * `total_elements` elements in all; 0 for an elem_size that is not 2, 4 or 8 (or an overflow).
 * Everything is checked before anything is launched or uploaded.  HSRANS_E_ARG: a null handle or pointer, a null `ranges`
 * with count > 0; a gather object of another context; d_out or d_work not 16-byte aligned; a range beyond the descriptor's
 * elements; (dst_offset + length) * elem_size beyond out_capacity, or any 64-bit overflow in these sums; work_bytes below
 * what THIS call's layout needs (elem_size * up256(sum of slots)); count * elem_size or the merge's task total at or above
 * 2^31; any intersection among the frame, the output and the workspace.  HSRANS_OK with nothing launched: count == 0 or
 * only empty ranges.  HSRANS_E_HIP (the runtime refused an upload or a launch) may leave the workspace written and the
 * output not: the gather may have been queued before the merge failed.
 * Cost: the gather of the coded planes' bytes (hsrans_decode_device_gather_batch's cost model: each task plus at most one
 * chain in front of it) and one pass over the fetched elements.  128 MiB of bf16 / fp32, rows of 4096 elements: 49-53 us
 * for 1 % of the rows against 84-134 us for hsrans_decode_device_planes and a copy of the rows; level at 10 %.  Above about
 * a tenth of the tensor (9.3-11.1 % measured) decode the whole frame instead (README).  Destinations that are
 * only element-aligned cost the same at that size (rows of 1000 elements: 54-80 us either way).
 * hsrans_planes_gather_status: hsrans_gather_set_status mapped back to planes (synchronises hip_stream); stored planes
 * report HSRANS_OK; with every plane stored it only settles the stream, as hsrans_planes_status does.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct hsrans_planes_gather hsrans_planes_gather;
int hsrans_planes_gather_create(hsrans_ctx *ctx, hsrans_planes *planes, const void *d_frame, size_t frame_length, hsrans_planes_gather **out);
void hsrans_planes_gather_destroy(hsrans_planes_gather *pg);
size_t hsrans_planes_gather_workspace_bytes(uint32_t elem_size, uint32_t count, uint64_t total_elements);
int hsrans_decode_device_planes_gather(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *ranges /* host, in elements */, uint32_t count,
                                       void *d_out, size_t out_capacity /* bytes */, void *d_work, size_t work_bytes, void *hip_stream);
int hsrans_planes_gather_status(hsrans_ctx *ctx, hsrans_planes_gather *pg, void *hip_stream, int *plane_status /* [elem_size] or NULL */);
typedef struct hsrans_planes_gather_info_t
{
  uint32_t coded, stored; /* planes */
  /* the last hsrans_decode_device_planes_gather on the object (all 0: none yet, or it had nothing to do) */
  uint32_t rows;        /* of its hsrans_decode_device_gather_batch: count x coded */
  uint32_t merge_tasks; /* workgroups of its merge launch */
  uint32_t launches;    /* kernels: the set's launches + the merge */
} hsrans_planes_gather_info_t;
int hsrans_planes_gather_info(const hsrans_planes_gather *pg, hsrans_planes_gather_info_t *info);
/* The host-side cut of the merge, a pure function (no GPU), as hsrans_gather_tasks is for the codec gather.  One task = one
 * workgroup's work: at most 4096 elements of one range, cut on the source's 16-element grid — task t of a range covers the
 * elements [A + 4096 t, A + 4096 (t + 1)) with A = offset - phase, clipped to the range.  src (a multiple of 16, in
 * tensor coordinates) is that window's first element and work_pos (a multiple of 16, in region coordinates) where it lies
 * in a workspace region; the valid elements are [src + lo, src + hi), lo < 16 (only a range's first task has lo != 0),
 * hi <= 4096; element e goes to output element e + dst_delta.  The tasks of a range tile it in order; empty ranges
 * give no task.  Returns the tasks the ranges need and writes at most `capacity` of them (out may be NULL when capacity is
 * 0); 0 for a null `ranges` with count > 0, a range beyond `elements`, or 2^31 tasks or more (one launch's limit, which
 * hsrans_decode_device_planes_gather refuses by this same function). */
typedef struct hsrans_planes_gather_task
{
  uint64_t src, work_pos;
  int64_t dst_delta; /* elements */
  uint32_t lo, hi;
} hsrans_planes_gather_task; /* 32 bytes */
size_t hsrans_planes_gather_tasks(const hsrans_range *ranges, uint32_t count, uint64_t elements, hsrans_planes_gather_task *out, size_t capacity);
/* ------------------------------------------------------------------------------------------------------------
 * The same for ranges that are in DEVICE memory — a router's choice, a page table, a sampler — with no host round trip:
 * n = d_count ? *d_count : max_count, and for the ranges d_ranges[0 .. n) d_out receives, byte for byte, what
 * hsrans_decode_device_planes_gather writes for the same ranges in host memory; no other byte of d_out is written.
 *   - asynchronous on hip_stream: kernel launches and nothing else — no allocation, no synchronisation, no lock, no host
 *     read of device memory, no use of the context's task buffer; the last call's part of hsrans_planes_gather_info is not
 *     written.  The call can be captured into a graph: one line of kernels on one stream, no parallel branches.
 *   - d_ranges and *d_count are read when the launches RUN: a replayed graph gathers whatever they hold then and inherits
 *     nothing from the replay before it (every word the later launches read is written by every call).  Rows of
 *     d_ranges from n on are never read.
 *   - launches, in order: one cut (one workgroup: it checks the ranges, lays out their slots, counts the merge's tasks and
 *     writes the count x coded rows of the set's gather); where the frame has coded planes,
 *     hsrans_decode_device_gather_batch_indirect on the object's set, through that public entry, with those rows;
 *     one merge launch that finds each task's range in the prefix the cut left and derives the task as
 *     hsrans_planes_gather_tasks does.  With every plane stored: two kernels.  The merge's grid cannot depend on the
 *     ranges: it is the most tasks the call can have, max_count + stride / 4096, capped at the workgroups the device
 *     holds at once, and the workgroups stride over the tasks, so any total finishes.
 *   - d_work, the data workspace: the ranges cannot decide the layout, so the regions lie
 *     stride = up256(max_elements + 30 * max_count) apart, region p at d_work + p * stride, and work_bytes must be
 *     hsrans_planes_gather_workspace_bytes(elem_size, max_count, max_elements).  Inside a region the layout is the host
 *     call's (slot [B_r, B_r + up16(phase + length)), the byte of plane p of element offset + i at
 *     region p + B_r + phase + i); slot bytes outside [phase, phase + length) and the regions of stored planes are never
 *     written.  max_elements: the most elements the ranges fetch in all.
 *   - d_workspace, the control workspace: hsrans_planes_gather_indirect_workspace_bytes(elem_size, max_count) bytes,
 *     256-byte aligned, contents irrelevant; it belongs to one call in flight (calls with different workspace pairs on
 *     one object are independent of each other whatever streams they are on).  It holds a header, the tasks' prefix
 *     first_task[0 .. max_count], B_r per range, the max_count x elem_size rows of hsrans_member_range for the set with
 *     their count word, and behind them hsrans_gather_batch_workspace_bytes(elem_size, max_count x elem_size) bytes
 *     for the set's own call.
 * What only the device can see is checked there, all or nothing: *d_count > max_count, a range beyond the descriptor's
 * elements, (dst_offset + length) * elem_size beyond out_capacity, any 64-bit overflow in these sums, a sum of slots
 * above stride, a merge task total of 2^31 or more.  Then the call moves NOTHING — not one byte of d_out or d_work is
 * written — and sets bit 8 of a status word the gather object owns (no plan's word is touched):
 * hsrans_planes_gather_refused synchronises hip_stream, returns HSRANS_E_DEVICE once and clears the word; otherwise it
 * returns what hsrans_gather_set_refused returns for the object's set (whose word should never fire once the cut has
 * passed the rows; HSRANS_OK when there is no set).  A malformed histogram still reaches only its plane's plan word
 * (hsrans_planes_gather_status).
 * Returns HSRANS_E_ARG, nothing queued: a null handle or pointer (d_count may be NULL); a gather object of another
 *   context; d_out or d_work not 16-byte, d_ranges not 8-byte, d_count not 4-byte or d_workspace not 256-byte aligned;
 *   workspace_bytes or work_bytes below the two size functions, either of them returning 0, or
 *   max_elements + 30 * max_count at or above 2^48; any intersection in which a written span takes part among the frame,
 *   d_ranges[0 .. max_count), d_count (read) and d_out over out_capacity, d_work over work_bytes, d_workspace (written).
 * HSRANS_OK with nothing queued: max_count == 0.
 * hsrans_planes_gather_indirect_workspace_bytes: a pure function, sized for all planes coded (it needs no object); > 0
 *   and a multiple of 256 for elem_size 2, 4 or 8 with max_count * elem_size < 2^31, non-decreasing in max_count; 0
 *   otherwise.
 * hsrans_planes_gather_indirect_info: a pure function of the object, max_count and max_elements (no device call), through
 *   the shape function the entry uses.  HSRANS_E_ARG where the entry would refuse these sizes.
 * Cost: README and DESIGN 5b (two single-workgroup cuts stand in a line in front of the gather).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct hsrans_planes_gather_indirect_info_t
{
  uint32_t coded, stored; /* planes */
  uint32_t max_rows;      /* of the set's gather: max_count x coded */
  uint32_t merge_grid;    /* workgroups of the merge launch */
  uint32_t launches;      /* all kernels of one call: the cut, the set's, the merge (0: max_count == 0) */
  uint32_t set_launches;  /* what hsrans_gather_set_indirect_info reports + the set's cut (0: every plane stored) */
} hsrans_planes_gather_indirect_info_t;
size_t hsrans_planes_gather_indirect_workspace_bytes(uint32_t elem_size, uint32_t max_count);
int hsrans_decode_device_planes_gather_indirect(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *d_ranges /* DEVICE, 8-byte aligned, in elements */,
                                                const uint32_t *d_count /* DEVICE, or NULL = max_count */, uint32_t max_count, uint64_t max_elements, void *d_out,
                                                size_t out_capacity, void *d_work, size_t work_bytes, void *d_workspace /* DEVICE, 256-byte aligned */,
                                                size_t workspace_bytes, void *hip_stream);
int hsrans_planes_gather_refused(hsrans_ctx *ctx, hsrans_planes_gather *pg, void *hip_stream);
int hsrans_planes_gather_indirect_info(const hsrans_planes_gather *pg, uint32_t max_count, uint64_t max_elements, size_t out_capacity,
                                       hsrans_planes_gather_indirect_info_t *info);
/* ------------------------------------------------------------------------------------------------------------
 * Element ranges of MANY frames that stay compressed in device memory — rows of many experts' weights, pages of every
 * layer's cache, slices of many parameters — in one call: what hsrans_decode_device_gather_batch is to
 * hsrans_decode_device_gather, for the byte-plane layer.  A planes gather set binds the members of a hsrans_planes_set
 * to their frames once; a call then takes rows of hsrans_member_range whose `member` is the tensor's index in the planes
 * set and whose offset, length and dst_offset are in THAT member's elements: the elements [offset, offset + length) of
 * member m land at (uint8_t *)d_out + dst_offset * elem_size(m), and no other byte of d_out is written.  All rows share
 * the one d_out.  Rows may come in any member order, a member may appear many times or not at all, sources may overlap;
 * destinations that overlap are the caller's responsibility; an empty row does nothing; reserved must be 0.  For every
 * row d_out receives, byte for byte, what hsrans_decode_device_planes_gather on that member's own gather object writes
 * for the same range, and the row's merge tasks are those hsrans_planes_gather_tasks reports for it.
 * hsrans_planes_gather_set_create binds member k to d_frames[k] (16-byte aligned, frame_lengths[k] at least the
 * descriptor's frame length), makes ONE hsrans_gather_set over all coded planes of all members, in member and plane order
 * (none when every plane is stored), and uploads, once, one record per member for the merge: its element size, which
 * planes are coded and the stored planes' addresses (d_frames[k] + desc.offset[p]).  The planes set, its plans and the
 * frames must outlive the object.  Returns HSRANS_E_ARG: a null argument, a set of another context, a misaligned or short
 * frame, more than 65,536 coded planes (hsrans_gather_set_create's limit); HSRANS_E_FORMAT: as hsrans_gather_set_create.
 * The call: ONE hsrans_decode_device_gather_batch on that set, through its public entry — every non-empty row gives one
 * gather row per coded plane of its member — then ONE merge launch behind it on the same stream that interleaves rows of
 * 2-, 4- and 8-byte members alike; stored planes are read by the merge straight from their frames.  Launch count: the
 * set's (one per table layout that has tasks, at most six) + 1, whatever the number of members or rows.  Asynchronous on
 * hip_stream; `ranges` (host memory) is read before the call returns; no device allocation, no synchronisation.  The
 * merge's task list goes through the context's task buffer: the call is ordered with the other gathers of the context.
 * Workspace layout, a pure function of the rows: with phase = offset & 15 a non-empty row r has
 * slot_r = up16(phase + length) and owns W(m_r) consecutive sub-slots of slot_r bytes from C_r on, C_r = the sum of
 * W * slot over the earlier rows; the byte of plane p of element offset + i is at d_work + C_r + p * slot_r + phase + i.
 * Everything is a multiple of 16: a 16-element block of a tensor is aligned alike in the workspace and in a stored plane,
 * and every gather row is 16-byte aligned against its source.  Sub-slots of stored planes and sub-slot bytes outside
 * [phase, phase + length) are never written.  A call needs up256(sum of W * slot) bytes;
 * hsrans_planes_gather_batch_workspace_bytes = up256(max_elem_size * (total_elements + 30 * count)) bounds it for every
 * `count` rows of `total_elements` elements in all over members of at most max_elem_size bytes an element; 0 for a
 * max_elem_size that is not 2, 4 or 8 (or an overflow).
 * Everything is checked before anything is uploaded or launched.  HSRANS_E_ARG, nothing written: a null handle or pointer,
 * a null `ranges` with count > 0; an object of another context; d_out or d_work not 16-byte aligned; member >= the set's
 * members or reserved != 0; a range beyond the member's elements; (dst_offset + length) * elem_size(m) beyond
 * out_capacity, or any 64-bit overflow in these sums; work_bytes below what THIS call's layout needs; gather rows or merge
 * tasks at or above 2^31; any intersection among the frames (over frame_lengths), the output and the workspace.
 * HSRANS_OK with nothing launched: count == 0 or only empty rows.  HSRANS_E_HIP (the runtime refused an upload or a
 * launch) may leave the workspace written and the output not.
 * hsrans_planes_gather_set_status: hsrans_gather_set_status mapped back to members (synchronises hip_stream):
 * member_status[k] is the status of member k's first failing plane, or HSRANS_OK; returns the first failure.  With every
 * plane stored it only settles the stream.
 * Cost: README and DESIGN 5b.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct hsrans_planes_gather_set hsrans_planes_gather_set;
int hsrans_planes_gather_set_create(hsrans_ctx *ctx, hsrans_planes_set *set, const void *const *d_frames, const size_t *frame_lengths, hsrans_planes_gather_set **out);
void hsrans_planes_gather_set_destroy(hsrans_planes_gather_set *pgs);
size_t hsrans_planes_gather_batch_workspace_bytes(uint32_t max_elem_size, uint32_t count, uint64_t total_elements);
int hsrans_decode_device_planes_gather_batch(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, const hsrans_member_range *ranges /* host, in elements */, uint32_t count,
                                             void *d_out, size_t out_capacity /* bytes */, void *d_work, size_t work_bytes, void *hip_stream);
int hsrans_planes_gather_set_status(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, void *hip_stream, int *member_status /* [members] or NULL */);
typedef struct hsrans_planes_gather_set_info_t
{
  uint32_t members, coded, stored; /* members; planes of all members */
  /* the last hsrans_decode_device_planes_gather_batch on the object (all 0: none yet, or it had nothing to do) */
  uint32_t rows;        /* of its hsrans_decode_device_gather_batch: the coded planes of every non-empty row's member */
  uint32_t merge_tasks; /* workgroups of its merge launch */
  uint32_t launches;    /* kernels: the set's launches + the merge */
} hsrans_planes_gather_set_info_t;
int hsrans_planes_gather_set_info(const hsrans_planes_gather_set *pgs, hsrans_planes_gather_set_info_t *info);
/* The host-side cut of the merge, a pure function (no GPU): member m has elem_sizes[m]-byte elements (2, 4 or 8) and
 * elements[m] of them.  The tasks come in row order, a row's tasks are those hsrans_planes_gather_tasks gives for the row
 * alone — src, dst_delta, lo and hi as there, work_pos counted from the row's C_r — with plane_step = slot_r (plane p of
 * the task's window lies at work_pos + p * plane_step of the workspace) and the row's member.  Returns the task total and
 * writes at most `capacity` of them (out may be NULL when capacity is 0); 0 for a null `ranges` with count > 0, null
 * member arrays with members > 0, a member whose element size is not 2, 4 or 8, member >= members, reserved != 0, a
 * range beyond its member's elements, a sum of W * slot that overflows, or 2^31 tasks or more (one launch's limit);
 * hsrans_decode_device_planes_gather_batch refuses by this same function. */
typedef struct hsrans_planes_gather_batch_task
{
  uint64_t src, work_pos, plane_step;
  int64_t dst_delta; /* elements */
  uint32_t lo, hi, member, reserved;
} hsrans_planes_gather_batch_task; /* 48 bytes */
size_t hsrans_planes_gather_batch_tasks(const hsrans_member_range *ranges, uint32_t count, const uint32_t *elem_sizes, const uint64_t *elements, uint32_t members,
                                        hsrans_planes_gather_batch_task *out, size_t capacity);
/* ------------------------------------------------------------------------------------------------------------
 * The same for rows that are in DEVICE memory — a router's choice among many experts, a page table over every layer's
 * cache, a sampler — with no host round trip: n = d_count ? *d_count : max_count, and for the rows d_ranges[0 .. n) d_out
 * AND d_work receive, byte for byte, what hsrans_decode_device_planes_gather_batch writes for the same rows in host
 * memory; no other byte of either buffer is written.
 *   - asynchronous on hip_stream: kernel launches and nothing else — no allocation, no synchronisation, no lock, no host
 *     read of device memory, no use of the context's task buffer; the last call's part of hsrans_planes_gather_set_info is
 *     not written.  The call can be captured into a graph: one line of kernels on one stream, no parallel branches.
 *   - d_ranges and *d_count are read when the launches RUN: a replayed graph gathers whatever they hold then and inherits
 *     nothing from the replay before it (every word the later launches read is written by every call).  Rows of
 *     d_ranges from n on are never read.
 *   - launches, in order: one cut (one workgroup: it checks every row against its member, lays out the workspace, counts
 *     the merge's tasks and writes, for every non-empty row, one row of the set's gather per coded plane of its member,
 *     in the form the host call builds: {offset, length, C_r + p * slot_r + phase, the plane's member of the set, 0});
 *     where the set has coded planes, hsrans_decode_device_gather_batch_indirect on the object's set, through that
 *     public entry, with those rows, their count word and dst_capacity = work_bytes; one merge launch that finds each
 *     task's row in the prefix the cut left and derives the task as hsrans_planes_gather_batch_tasks does.  With every
 *     plane stored: two kernels.  The merge's grid cannot depend on the rows: it is the most tasks the call can have,
 *     max_count + work_bytes / (the smallest member's elem_size * 4096), capped at the workgroups the device holds at
 *     once, and the workgroups stride over the tasks, so any total finishes.  Pass the work_bytes the rows really need.
 *   - d_work, the data workspace: the layout is the host call's (row r owns W(m_r) sub-slots of slot_r = up16(phase +
 *     length) bytes from C_r on, C_r = the sum of W * slot over the earlier rows) — the device forms C_r by a prefix sum,
 *     so, unlike hsrans_decode_device_planes_gather_indirect, there is no stride and no max_elements.  work_bytes is the
 *     capacity: hsrans_planes_gather_batch_workspace_bytes bounds what any rows can need.
 *   - d_workspace, the control workspace: hsrans_planes_gather_batch_indirect_workspace_bytes(the set's coded planes,
 *     its largest elem_size, max_count) bytes, 256-byte aligned, contents irrelevant; it belongs to one call in flight
 *     (calls with different workspace pairs on one object are independent of each other whatever streams they are on).
 *     It holds a header, the tasks' prefix first_task[0 .. max_count], C_r per row, the position of each row's first
 *     gather row, the max_count x max_elem_size rows of hsrans_member_range for the set with their count word, and behind
 *     them hsrans_gather_batch_workspace_bytes(coded_planes, max_count x max_elem_size) bytes for the set's own call.
 * What only the device can see is checked there, all or nothing, by the rules that make the host call return
 * HSRANS_E_ARG: *d_count > max_count; member >= the set's members or reserved != 0 (of empty rows too); a range beyond
 * its member's elements; (dst_offset + length) * elem_size(m) beyond out_capacity; any 64-bit overflow in these sums;
 * up256(the sum of W * slot) above work_bytes (or above 2^48); a merge task total or a gather row total of 2^31 or more.
 * Then the call moves NOTHING — not one byte of d_out or d_work is written — and sets bit 8 of a status word the
 * gather set object owns, allocated by hsrans_planes_gather_set_create (no plan's word is touched):
 * hsrans_planes_gather_set_refused synchronises hip_stream, returns HSRANS_E_DEVICE once and clears the word; otherwise
 * it returns what hsrans_gather_set_refused returns for the object's set (whose word should never fire once the cut has
 * passed the rows; HSRANS_OK when there is no set).  A malformed histogram still reaches only its plane's plan word
 * (hsrans_planes_gather_set_status).
 * Returns HSRANS_E_ARG, nothing queued: a null handle or pointer (d_count may be NULL); an object of another context;
 *   d_out or d_work not 16-byte, d_ranges not 8-byte, d_count not 4-byte or d_workspace not 256-byte aligned;
 *   workspace_bytes below the size function (or the size function returning 0); any intersection in which a written
 *   span takes part among the frames, d_ranges[0 .. max_count), d_count (read) and d_out over out_capacity, d_work over
 *   work_bytes, d_workspace (written).
 * HSRANS_OK with nothing queued: max_count == 0.
 * hsrans_planes_gather_batch_indirect_workspace_bytes: a pure function (it needs no object); > 0 and a multiple of 256
 *   for max_elem_size 2, 4 or 8 with max_count * max_elem_size < 2^31 and coded_planes <= 65,536, non-decreasing in
 *   max_count and coded_planes; coded_planes == 0 (every plane stored) leaves out the set's part; 0 otherwise.
 * hsrans_planes_gather_set_indirect_info: a pure function of the object, max_count and work_bytes (no device call),
 *   through the shape function the entry uses.  HSRANS_E_ARG where the entry would refuse these sizes.
 * Cost: README and DESIGN 5b (two single-workgroup cuts stand in a line in front of the gather).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct hsrans_planes_gather_set_indirect_info_t
{
  uint32_t members, coded, stored; /* members; planes of all members */
  uint32_t max_rows;               /* of the set's gather: max_count x the largest elem_size (0: every plane stored) */
  uint32_t merge_grid;             /* workgroups of the merge launch */
  uint32_t launches;               /* all kernels of one call: the cut, the set's, the merge (0: max_count == 0) */
  uint32_t set_launches;           /* what hsrans_gather_set_indirect_info reports + the set's cut (0: every plane stored) */
} hsrans_planes_gather_set_indirect_info_t;
size_t hsrans_planes_gather_batch_indirect_workspace_bytes(uint32_t coded_planes, uint32_t max_elem_size, uint32_t max_count);
int hsrans_decode_device_planes_gather_batch_indirect(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs,
                                                      const hsrans_member_range *d_ranges /* DEVICE, 8-byte aligned, in elements */,
                                                      const uint32_t *d_count /* DEVICE, or NULL = max_count */, uint32_t max_count, void *d_out, size_t out_capacity,
                                                      void *d_work, size_t work_bytes, void *d_workspace /* DEVICE, 256-byte aligned */, size_t workspace_bytes,
                                                      void *hip_stream);
int hsrans_planes_gather_set_refused(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, void *hip_stream);
int hsrans_planes_gather_set_indirect_info(const hsrans_planes_gather_set *pgs, uint32_t max_count, size_t out_capacity, size_t work_bytes,
                                           hsrans_planes_gather_set_indirect_info_t *info);
/* ------------------------------------------------------------------------------------------------------------
 * Tensors coded against a base.  The tensors this layer is for are rarely alone: a checkpoint's parameters sit next to the
 * previous checkpoint's, a fine-tuned model next to its base, a layer's experts next to a shared initialisation.  XORed with a
 * close relative, a bf16 tensor's sign/exponent byte is almost always zero and its mantissa byte's upper bits mostly are: the
 * residue codes far smaller than the tensor.  XOR here, not an arithmetic difference: it is dtype-free (these entries take no view
 * on endianness or dtype), exactly invertible and needs no carries across bytes.  It pays for every carry the real difference
 * causes, though — two bf16 values one ulp apart XOR to 2^(k+1) - 1, k the low mantissa bits that flip — so a second residue rule,
 * the zigzag of the elements' wrapped integer difference, has entries of its own in the section behind this one
 * (hsrans_*_device_planes_diff); that is the one place the library reads an element as a little-endian integer.  XOR stays, for
 * callers who want no such view.
 *
 * The invariant.  A delta frame of `in` against `base` is, byte for byte, the ordinary frame of the tensor in ^ base: the same
 * frame bytes, the same descriptor, the same plans as hsrans_encode_device_planes gives for a buffer that holds in ^ base.
 * hsrans_planes_desc does not change and a frame does NOT record its base: keeping track of the base is the caller's business,
 * like the descriptor itself.  Every other entry of this layer therefore takes a delta frame unchanged and yields the residue —
 * hsrans_planes_create, hsrans_planes_pack_device, the gathers, the batches; in particular hsrans_decode_device_planes of a delta
 * frame gives in ^ base.  That is intended, not an error the library could detect.
 *
 * Cost.  The XOR rides in the split and the merge kernels, which touch every element once anyway: one more 16-byte load per 16
 * bytes moved.  No extra launch, no extra workspace, no codec kernel changes: each entry below has the launch count, the
 * workspace, the return value and the synchronisation of its plain counterpart, and checks everything that one checks.
 *
 * The base: a device buffer, 16-byte aligned, base_bytes >= elem_size * elements, element i of the base against element i of
 * the tensor.  HSRANS_E_ARG (the encoders: 0) before anything is launched or written for a NULL or misaligned base or a short
 * base_bytes.  Overlap: the base is a READ span over base_bytes.  It may coincide with other read spans — one base shared by
 * many members, or d_in == d_base (every plane is then one symbol) — and any intersection with a written span (a frame, the
 * workspace, an output) is refused.  A frame counts as one on the decode side too, where it is only read: a base that meets the
 * frame it is decoded against — in the batch any member's frame, in the gather the frame the object is bound to — is refused.
 * In place.  One exception, for the whole-tensor decodes (hsrans_planes_merge_delta_device, hsrans_decode_device_planes_delta and
 * hsrans_decode_device_planes_delta_batch): a member's output may be exactly its own base — the same address, out_capacity <=
 * base_bytes — and the delta is then applied in place: every lane reads its base bytes before it writes, and no lane reads
 * another's.  Any other overlap of an output and a base (an offset of 16 bytes, another member's base) is refused.  The gather
 * allows no aliasing at all.
 * ---------------------------------------------------------------------------------------------------------- */
/* the rule on the host, in plain C++: planes[p][i] = in[i * W + p] ^ base[i * W + p], and back (out may be base);
 * HSRANS_OK or HSRANS_E_ARG (elem_size not 2, 4 or 8; a NULL pointer) */
int hsrans_planes_split_delta(uint32_t elem_size, const void *in, const void *base, size_t elements, uint8_t *const *planes);
int hsrans_planes_merge_delta(uint32_t elem_size, const uint8_t *const *planes, const void *base, size_t elements, void *out);
/* the two kernels alone, as hsrans_planes_split_device / hsrans_planes_merge_device: asynchronous on `hip_stream`, no allocation,
 * no synchronisation.  d_base: elem_size * elements bytes, 16-byte aligned, clear of the planes; the merge's d_out may be d_base. */
int hsrans_planes_split_delta_device(hsrans_ctx *ctx, uint32_t elem_size, const void *d_in, const void *d_base, size_t elements, void *const *d_planes,
                                     void *hip_stream);
int hsrans_planes_merge_delta_device(hsrans_ctx *ctx, uint32_t elem_size, const void *const *d_planes, const void *d_base, size_t elements, void *d_out,
                                     void *hip_stream);
/* hsrans_encode_device_planes of in ^ base without the buffer that holds it: the same flow with the delta split in front, the
 * same return value, descriptor, plans, refusals and synchronisation; a stored plane holds the residue's bytes. */
size_t hsrans_encode_device_planes_delta(hsrans_ctx *ctx, uint32_t elem_size, int states, uint32_t bits, const void *d_in, const void *d_base, size_t base_bytes,
                                         size_t elements, void *d_frame, size_t frame_capacity, uint32_t block_size, uint32_t index_interval, uint32_t flags,
                                         void *d_work, size_t work_bytes, void *hip_stream, hsrans_planes_desc *desc,
                                         hsrans_dplan **out_dplans /* [elem_size] or NULL */);
/* hsrans_decode_device_planes with the delta merge behind the codec batch: d_out = (what the frame holds) ^ base.  The same
 * launch count (hsrans_planes_info) and workspace; asynchronous.  d_out may be d_base (in place, above). */
int hsrans_decode_device_planes_delta(hsrans_ctx *ctx, hsrans_planes *planes, const void *d_frame, size_t frame_length, const void *d_base, size_t base_bytes,
                                      void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream);
/* hsrans_encode_device_planes_batch with a base per member: member k is coded against d_bases[k] over base_bytes[k], or as it
 * is where d_bases[k] is NULL (base_bytes[k] is then ignored).  Member equivalence: member k gets byte for byte what
 * hsrans_encode_device_planes_delta gives it — hsrans_encode_device_planes where its base is NULL.  One delta split launch over
 * all members (the NULL-base choice is taken per workgroup), then the plain call's launches: the same stats.  A NULL d_bases or
 * base_bytes array is HSRANS_E_ARG. */
int hsrans_encode_device_planes_delta_batch(hsrans_ctx *ctx, hsrans_planes_member *members, const void *const *d_bases /* [count], entries may be NULL */,
                                            const size_t *base_bytes /* [count] */, uint32_t count, void *d_work, size_t work_bytes, void *hip_stream,
                                            hsrans_dplan **out_dplans /* [count * HSRANS_PLANES_MAX] or NULL */, hsrans_planes_batch_stats *stats /* may be NULL */);
/* hsrans_decode_device_planes_batch with ONE delta merge launch in place of the merge: the set's launch count and workspace.
 * d_outs[k] may be d_bases[k] (in place, above); it may not meet another member's base. */
int hsrans_decode_device_planes_delta_batch(hsrans_ctx *ctx, hsrans_planes_set *set, const void *const *d_frames, const size_t *frame_lengths,
                                            const void *const *d_bases /* [count], entries may be NULL */, const size_t *base_bytes /* [count] */, void *const *d_outs,
                                            const size_t *out_capacities, void *d_work, size_t work_bytes, void *hip_stream);
/* hsrans_decode_device_planes_gather (ranges in host memory) of a delta frame: element offset + i of the frame, XORed with
 * element offset + i of the base, lands at element dst_offset + i of d_out.  d_base is the WHOLE base tensor, in the frame's
 * element coordinates (base_bytes >= elem_size * the frame's elements), whatever the ranges are; heads and tails read base bytes
 * of their own elements only.  No aliasing: the base may not meet d_out or d_work. */
int hsrans_decode_device_planes_gather_delta(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *ranges, uint32_t count, const void *d_base, size_t base_bytes,
                                             void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream);
/* The other three gathers of a delta frame: each is its plain twin with the XOR in its merge kernel (hsrans_planes_gather_delta.hip)
 * — the same launch count, both workspaces and their size functions, the same *_info / *_indirect_info answers, device-side checks,
 * refused word, *_status, return codes, asynchrony, and for the two indirect forms the same "kernels and nothing else" (capturable).
 * d_work receives exactly what the plain twin writes there: the residue's plane bytes; the XOR happens behind them.  Every row of
 * d_out receives byte for byte what hsrans_decode_device_planes_gather_delta on that member's own gather object writes for the same
 * range against the same base.  (The merge's grid of an indirect delta call is sized from the delta kernel's registers and may be
 * smaller than the merge_grid that *_indirect_info reports for the plain call; the workgroups stride over the tasks either way.)
 * Added refusals, all HSRANS_E_ARG with nothing queued or written: a NULL, misaligned or short base; a base set that is NULL or of
 * another gather set or context; a base that meets d_out over out_capacity, d_work over work_bytes or d_workspace; a base that meets
 * a frame; and — reads though they are, like a frame — a base that meets d_ranges[0 .. max_count) or d_count.  Bases may coincide
 * with one another.  No gather allows in-place or any other aliasing. */
/* ranges in device memory, one frame: hsrans_decode_device_planes_gather_indirect with d_base, the WHOLE base tensor in the frame's
 * element coordinates (base_bytes >= elem_size * the frame's elements), read when the launches run */
int hsrans_decode_device_planes_gather_indirect_delta(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *d_ranges, const uint32_t *d_count, uint32_t max_count,
                                                      uint64_t max_elements, const void *d_base, size_t base_bytes, void *d_out, size_t out_capacity, void *d_work,
                                                      size_t work_bytes, void *d_workspace, size_t workspace_bytes, void *hip_stream);
/* member m of a gather set is decoded against d_bases[m] over base_bytes[m], or as it is where d_bases[m] is NULL (base_bytes[m] is
 * then ignored).  The addresses are uploaded here, once and synchronously, one uint64_t per member, so that the device-rows call
 * stays kernels and nothing else; the object keeps a host copy for the calls' overlap checks.  It is bound to ONE gather set, which
 * may have several base sets and is not modified (nor is its planes set); destroy it before that set; the bases must outlive it.
 * HSRANS_E_ARG, with nothing allocated: a NULL argument, a set of another context, a non-NULL base that is not 16-byte aligned,
 * base_bytes[m] < elem_size(m) * elements(m), a base that meets any member's frame.  Bases may coincide with each other.  All entries
 * NULL is valid: the calls then write what the plain calls write. */
typedef struct hsrans_planes_base_set hsrans_planes_base_set;
int hsrans_planes_base_set_create(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, const void *const *d_bases /* [members], entries may be NULL */,
                                  const size_t *base_bytes /* [members] */, hsrans_planes_base_set **out);
void hsrans_planes_base_set_destroy(hsrans_planes_base_set *bs); /* NULL: nothing */
/* rows of many frames on the host: hsrans_decode_device_planes_gather_batch with member m's rows XORed with its base; the task list
 * goes through the context's task buffer like the plain call's; hsrans_planes_gather_set_info answers as for the plain call */
int hsrans_decode_device_planes_gather_batch_delta(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, const hsrans_planes_base_set *bs, const hsrans_member_range *ranges,
                                                   uint32_t count, void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream);
/* rows of many frames in device memory: hsrans_decode_device_planes_gather_batch_indirect likewise; a refusal on the device is
 * reported by hsrans_planes_gather_set_refused as the plain call's is */
int hsrans_decode_device_planes_gather_batch_indirect_delta(hsrans_ctx *ctx, hsrans_planes_gather_set *pgs, const hsrans_planes_base_set *bs,
                                                            const hsrans_member_range *d_ranges, const uint32_t *d_count, uint32_t max_count, void *d_out,
                                                            size_t out_capacity, void *d_work, size_t work_bytes, void *d_workspace, size_t workspace_bytes, void *hip_stream);

/* ------------------------------------------------------------------------------------------------------------
 * Tensors coded against a base as a zigzag difference.  The second residue rule of this layer, for relatives that lie a few ulps
 * apart: a fine-tune next to its base, a checkpoint next to its predecessor.  There the XOR residue above pays for every carry
 * (one ulp across k low mantissa bits XORs to 2^(k+1) - 1); the difference does not.
 *
 * The rule.  An element is read as a LITTLE-ENDIAN UNSIGNED INTEGER of W = elem_size bytes, W in {2, 4, 8}: this is the one place
 * the library takes a view on byte order (nothing is read as a float: bf16, fp16, fp32, fp64 and the integers all go by their bit
 * patterns).  All arithmetic is modulo 2^(8 W):
 *   split:  d = in - base,  z = (d << 1) ^ (0 - (d >> (8 W - 1))),  planes[p][i] = byte p of z[i]
 *   merge:  d = (z >> 1) ^ (0 - (z & 1)),  out = base + d
 * — the wrapped difference with its sign folded into the lowest bit, so that small differences of either sign leave small z.
 * Exactly invertible for every pair of bit patterns, NaNs and values of opposite sign included.
 *
 * The invariant mirrors the delta one.  A diff frame of `in` against `base` is, byte for byte, the ordinary frame of the tensor z:
 * the same frame bytes, the same descriptor, the same plans as hsrans_encode_device_planes gives for a buffer that holds z.  A frame
 * records neither its base NOR ITS RULE.  Every other entry of this layer therefore takes a diff frame unchanged and yields z; in
 * particular hsrans_decode_device_planes of a diff frame gives z.  Decoding a diff frame with a _delta entry, or a delta frame with
 * a _diff entry, gives garbage, not an error: which rule a frame was coded by is the caller's to keep, like its base.
 *
 * Each entry below has the argument list, return value, launch count, workspace, synchronisation, refusals and overlap rule of its
 * _delta twin above, word for word — the base a 16-byte aligned device buffer of base_bytes >= elem_size * elements, a READ span
 * that may coincide with other reads and may meet nothing written nor a frame it is decoded against; the in-place exception
 * d_out == d_base (out_capacity <= base_bytes) for the three whole-tensor decodes (hsrans_planes_merge_diff_device,
 * hsrans_decode_device_planes_diff, hsrans_decode_device_planes_diff_batch: every lane reads its base elements before it writes,
 * and no lane reads another's); no aliasing at all in the gather.  The kernels are the _diff ones of hsrans_planes_base.hip: the delta
 * kernels' loads and stores with a handful of integer instructions per word between them.
 * The diff forms of the other three gathers (_gather_indirect, _gather_batch, _gather_batch_indirect) are not offered yet.
 * ---------------------------------------------------------------------------------------------------------- */
/* the rule on the host, in plain C++ (out may be base); HSRANS_OK or HSRANS_E_ARG (elem_size not 2, 4 or 8; a NULL pointer) */
int hsrans_planes_split_diff(uint32_t elem_size, const void *in, const void *base, size_t elements, uint8_t *const *planes);
int hsrans_planes_merge_diff(uint32_t elem_size, const uint8_t *const *planes, const void *base, size_t elements, void *out);
/* the two kernels alone, as hsrans_planes_split_delta_device / hsrans_planes_merge_delta_device: asynchronous on `hip_stream`, no
 * allocation, no synchronisation.  d_base: elem_size * elements bytes, 16-byte aligned, clear of the planes; the merge's d_out may
 * be d_base. */
int hsrans_planes_split_diff_device(hsrans_ctx *ctx, uint32_t elem_size, const void *d_in, const void *d_base, size_t elements, void *const *d_planes,
                                    void *hip_stream);
int hsrans_planes_merge_diff_device(hsrans_ctx *ctx, uint32_t elem_size, const void *const *d_planes, const void *d_base, size_t elements, void *d_out,
                                    void *hip_stream);
/* hsrans_encode_device_planes of z without the buffer that holds it: hsrans_encode_device_planes_delta with the diff split in front;
 * a stored plane holds z's bytes. */
size_t hsrans_encode_device_planes_diff(hsrans_ctx *ctx, uint32_t elem_size, int states, uint32_t bits, const void *d_in, const void *d_base, size_t base_bytes,
                                        size_t elements, void *d_frame, size_t frame_capacity, uint32_t block_size, uint32_t index_interval, uint32_t flags,
                                        void *d_work, size_t work_bytes, void *hip_stream, hsrans_planes_desc *desc,
                                        hsrans_dplan **out_dplans /* [elem_size] or NULL */);
/* hsrans_decode_device_planes_delta with the diff merge behind the codec batch: d_out = base + (the difference the frame holds).
 * d_out may be d_base (in place, above). */
int hsrans_decode_device_planes_diff(hsrans_ctx *ctx, hsrans_planes *planes, const void *d_frame, size_t frame_length, const void *d_base, size_t base_bytes,
                                     void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream);
/* hsrans_encode_device_planes_delta_batch under this rule: member k gets byte for byte what hsrans_encode_device_planes_diff gives
 * it — hsrans_encode_device_planes where d_bases[k] is NULL: such a member goes as it is.  A call is all-diff: XOR and diff members
 * cannot be mixed in one call. */
int hsrans_encode_device_planes_diff_batch(hsrans_ctx *ctx, hsrans_planes_member *members, const void *const *d_bases /* [count], entries may be NULL */,
                                           const size_t *base_bytes /* [count] */, uint32_t count, void *d_work, size_t work_bytes, void *hip_stream,
                                           hsrans_dplan **out_dplans /* [count * HSRANS_PLANES_MAX] or NULL */, hsrans_planes_batch_stats *stats /* may be NULL */);
/* hsrans_decode_device_planes_delta_batch under this rule: ONE diff merge launch in place of the merge.  d_outs[k] may be d_bases[k]
 * (in place, above); it may not meet another member's base. */
int hsrans_decode_device_planes_diff_batch(hsrans_ctx *ctx, hsrans_planes_set *set, const void *const *d_frames, const size_t *frame_lengths,
                                           const void *const *d_bases /* [count], entries may be NULL */, const size_t *base_bytes /* [count] */, void *const *d_outs,
                                           const size_t *out_capacities, void *d_work, size_t work_bytes, void *hip_stream);
/* hsrans_decode_device_planes_gather_delta (ranges in host memory) under this rule: base element offset + i plus the difference that
 * element offset + i of the frame holds lands at element dst_offset + i of d_out.  d_base is the WHOLE base tensor, in the frame's
 * element coordinates (base_bytes >= elem_size * the frame's elements), whatever the ranges are; heads and tails read base
 * elements of their own range only.  No aliasing: the base may not meet d_out or d_work. */
int hsrans_decode_device_planes_gather_diff(hsrans_ctx *ctx, hsrans_planes_gather *pg, const hsrans_range *ranges, uint32_t count, const void *d_base, size_t base_bytes,
                                            void *d_out, size_t out_capacity, void *d_work, size_t work_bytes, void *hip_stream);

/* Build a plan with checkpoints every `index_interval` groups for an EXISTING stream (e.g. one written by the
 * reference's encoder) by one decode pass on the GPU that records the states at the checkpoints: HSRANS_RAW (one
 * sequential wavefront), HSRANS_MT (one wavefront per block) and HSRANS_BLOCK (one sequential wavefront that also reports
 * the inline block headers it meets: the plan then has a chain per block and per checkpoint, which is what makes a block_
 * stream chunk-parallel; blocks must average >= 4 KiB).  Returns plan bytes written to plan_out (host memory), 0 on
 * failure. */
size_t hsrans_index_build(hsrans_ctx *ctx, int container, int states, uint32_t bits, const uint8_t *in, size_t in_length,
                          uint32_t index_interval, uint8_t *plan_out, size_t plan_capacity);

/* as hsrans_index_build, with checkpoints at the given ascending group indices (raw streams; hsrans_index_boundaries) */
size_t hsrans_index_build_at(hsrans_ctx *ctx, int container, int states, uint32_t bits, const uint8_t *in, size_t in_length,
                             const uint64_t *groups, size_t n_groups, uint8_t *plan_out, size_t plan_capacity);

/* ------------------------------------------------------------------------------------------------------------
 * Host buffers, PCIe legs overlapped (BASELINE config 5 shape; the GPU counterpart of the reference's thread-pool fan-out,
 * src/mt_rANS32x64_16w_decode.cpp:137-265): the plan's chains are cut into `n_slices` runs; slice k's compressed bytes go
 * up on one HIP stream while slice k-1 decodes on a second and slice k-2's output comes down on a third (page-lock `in` and
 * `out` — hipHostMalloc / hipHostRegister / hsrans_host_register — or the runtime stages the copies and the legs serialise).
 * 2^30 bytes: 22.6 ms end to end = 47.4 GB/s decoded; 100 MB: 36-39 k MiB/s for every codec.  HSRANS_HPIPE_DIRECT=1 in the
 * environment makes the decode kernels store STRAIGHT into a page-locked `out` instead (no device-side output buffer, no
 * download copies): the same rate at 2^30 bytes, 29-34 k MiB/s at 100 MB.  The three streams belong to the context.
 * The slice plans live on the device for the lifetime of the pipeline object; a pipe serves one decode at a time (calls
 * serialise on it).  hsrans_decode_host_pipelined is the one-call form: it keeps the pipeline of the plan it saw last inside
 * the context (keyed by the plan's address, size and a sampled checksum).  On any failure every entry returns only after all work it queued has drained.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct hsrans_hpipe hsrans_hpipe;
int hsrans_hpipe_create(hsrans_ctx *ctx, const uint8_t *plan, size_t plan_size, uint32_t n_slices /* 0 = by size: 2..16 slices of >= 16 MiB of output */, hsrans_hpipe **out_pipe);
size_t hsrans_hpipe_decode(hsrans_hpipe *pipe, const uint8_t *in, size_t in_length, uint8_t *out, size_t out_capacity);
void hsrans_hpipe_destroy(hsrans_hpipe *pipe);
size_t hsrans_decode_host_pipelined(hsrans_ctx *ctx, int container, int states, uint32_t bits, const uint8_t *in, size_t in_length, uint8_t *out,
                                    size_t out_capacity, const uint8_t *plan, size_t plan_size, uint32_t n_slices);
/* The encode direction: host bytes in, an mt_ stream in host memory out, on the GPU with the PCIe legs overlapped — in place of
 * hsrans_encode_ex on one core (about 0.22 GB/s), or of device buffers of the whole input and stream with upload, hsrans_encode_device
 * and download one after the other.  The input is cut into `n_slices` runs of whole blocks (0 = by size, as hsrans_hpipe_create: 2..16
 * slices of >= 16 MiB of input; never more than there are blocks); slice k's input goes up on one of the context's three pipe streams
 * while slice k-1 is encoded on the second (hsrans_encode_device's kernels, the stream position carried from slice to slice on the
 * device) and slice k-2's compressed bytes come down on the third.  2^30 bytes, 64 states, 11 bits, 64 KiB blocks, page-locked:
 * 20.2 ms = 53 GB/s of input (46 GB/s with a plan every 32 groups) against 32.3 ms for upload, hsrans_encode_device and download
 * one after the other; 100 MB: 2.3 ms, 190x the host encoder.
 * Result: the stream length, 0 on failure.  out[0, length) is exactly what hsrans_encode_ex(container, states, bits, in, length, out,
 * out_capacity, NULL, opts) writes, and with opts->index_interval != 0 so are opts->plan_out / opts->plan_size; no byte of `out` at or
 * beyond the returned length is written.
 * Accepted: container HSRANS_MT, states 32 / 64, bits 10..15, opts->flags == HSRANS_ENC_INDEPENDENT_BLOCKS, opts->block_size a non-zero
 * multiple of 64 up to 2^30, opts->index_interval 0 or a multiple of 4, opts->n_index_groups 0.  Everything else, and everything
 * hsrans_encode_ex refuses (out_capacity < hsrans_capacity, a plan_capacity the plan cannot fit in), returns 0 before anything is
 * launched, with `out` untouched.
 * `in` and `out` are host memory: page-locked (hipHostMalloc, hsrans_host_register, torch pin_memory()) for the overlap; pageable
 * memory gives the same bytes, slower.  Synchronous: the stream (and plan) are complete on return; on failure it returns after all
 * work it queued has drained.  Device memory: the context's encode buffers, sized by the slices in flight (two input and two staging
 * slices, one slice of block slots) plus the per-block records of the plan — not by the input; calls on one context serialise. */
size_t hsrans_encode_host_pipelined(hsrans_ctx *ctx, int container, int states, uint32_t bits, const uint8_t *in, size_t length, uint8_t *out,
                                    size_t out_capacity, hsrans_encode_opts *opts, uint32_t n_slices);
/* page-lock / release a caller-owned host buffer (hipHostRegister on the context's device); 0 on success */
int hsrans_host_register(hsrans_ctx *ctx, void *ptr, size_t bytes);
int hsrans_host_unregister(hsrans_ctx *ctx, void *ptr);

/* Per-device fit of the one-chain-per-wave index (hsrans_index_boundaries): the SIMDs serve their oldest wave first, so the 8
 * scheduling classes of waves decode at different rates and get chains of different lengths; the lengths compiled in were fitted
 * on one box and are a few per cent off on others.  This measures the classes' finish times on the context's own device (48 MiB
 * of synthetic enwik8-shaped bytes, encoded once on the host; `iterations` (0 = 4) rounds of index -> launches -> adjust; about
 * half a second) and keeps the best lengths in the context: hsrans_index_boundaries(ctx, ...) and the launch info use them from
 * then on.  64 states, bits 10..12 (the 8-byte-table kernel).  Returns HSRANS_OK; `report` may be NULL.  Synchronises the
 * device; call it before the context is shared between threads (it rewrites the context's geometry while it runs).  Indexes made
 * before and after stay valid on any device: the lengths only decide how evenly a launch finishes. */
typedef struct hsrans_calibration
{
  uint32_t class_weights[8];                 /* per-mille chain lengths kept */
  double class_finish_us_last_iteration[8];  /* mean finish time of each class in the last iteration measured */
  double last_wave_us_before, last_wave_us_after;       /* when the launch's last wave was done: first iteration / best iteration */
  double class_spread_us_before, class_spread_us_after; /* latest minus earliest class mean */
  uint32_t iterations, reserved;
  uint64_t bytes;
} hsrans_calibration;
int hsrans_ctx_calibrate(hsrans_ctx *ctx, uint32_t bits, uint32_t iterations, hsrans_calibration *report);
/* The same fit at another RUN LENGTH.  A wave's time is its prologue plus its groups at its class's rate, so the chain lengths that
 * make the classes finish together depend on how long the runs are (an old wave's head start counts for less in a long run):
 * hsrans_ctx_calibrate fits runs of ~96 groups (its 48 MiB stream over 8,192 waves); this call decodes `copies` (1..16) members
 * of that stream in ONE batch launch — runs of copies x 96 groups — and keeps the fitted lengths as the set of that run length.
 * hsrans_index_boundaries[_batch] and the batch dealing interpolate between the fitted run lengths (log scale; the nearest set
 * outside them); up to 4 sets per context.  E.g. copies = 2 for 100 MB streams decoded alone, 8 for four of them in one launch. */
int hsrans_ctx_calibrate_runs(hsrans_ctx *ctx, uint32_t bits, uint32_t iterations, uint32_t copies, hsrans_calibration *report);

/* kernel launch geometry of the last hsrans_decode_device call on this plan (for benchmarks / DESIGN.md tables) */
typedef struct hsrans_launch_info
{
  uint32_t grid, block, lds_bytes, waves_per_block, chains, shared_table, walk, two_level;
  uint32_t table_mode; /* decode-table layout: 0/1 packed u32, 2 two-level, 3 8-byte per slot, 4 rank byte per slot + 256 entries, 5 8-byte in global memory */
  uint32_t chains_per_wave; /* 2: the two-chains-per-wave kernel (13..15 bits with a one-chain-per-wave index) */
  uint32_t class_weights[8]; /* per-mille chain / run lengths of the 8 wave scheduling classes the launch was shaped with (fitted
                              * constants, HSRANS_*_WEIGHTS override them): which table a measurement used */
  uint32_t dynamic_groups;   /* block_/mt_ plans with checkpoints: blocks handed to workgroups by a ticket counter (1) or statically (0) */
  uint32_t spread;           /* such plans with few, large blocks: all chains dealt out evenly over the resident workgroups (1) */
} hsrans_launch_info;
int hsrans_dplan_launch_info(const hsrans_dplan *dplan, hsrans_launch_info *info);

/* The dealing of the one-round launch of block_/mt_ plans with checkpoints (k_decode_dealt), without a device (tests, planning): block k of the
 * plan = chains [block_begin[k], block_begin[k + 1]) (n_blocks + 1 entries, the last = n_chains); total_groups = the groups of S symbols the
 * plan decodes.  Every one of the launch's 512 workgroups gets chains [begin_out[b], begin_out[b + 1]) — sized by the workgroups' scheduling
 * classes (the MI355X defaults; ctx != NULL: that context's fitted ones), never reaching into a third block — and split_out[b] = how many of
 * them belong to the share's first block (0xFFFF: all).  Returns 1 when the plan suits the launch, 0 when it keeps the grouped / spread
 * launch (too few chains per wave, a block and more per workgroup slot, shares bent too far by the cuts), < 0 on bad arguments. */
int hsrans_dealt_shares(const hsrans_ctx *ctx, uint32_t bits /* the class lengths differ between the 8-byte-table loop (<= 11) and the rank-table loop (13, 14) */,
                        const uint32_t *block_begin, uint32_t n_blocks, uint32_t n_chains, uint64_t total_groups, uint32_t *begin_out /* [513] */,
                        uint16_t *split_out /* [512] */);

/* Which kernel a single-plan decode launch of a plan would run, and with what geometry, without a device (tests, planning): the launcher's
 * own decision (choose_launch in csrc/hsrans_launch.cpp), on the MI355X defaults (ctx != NULL: that context's device and switches).
 * `plan`: the plan-header fields that matter.  `facts`: what the launcher otherwise reads off the device plan it is handed.
 * Returns 0 and fills *info and kernel_name (the demangled name as a kernel trace prints it, without return type and parameter list,
 * e.g. "hsrans::k_decode_direct<3>"); 1: the launch would be refused as not supported, 2: as an invalid value (nothing is filled in);
 * < 0 on bad arguments. */
typedef struct hsrans_plan_kind
{
  uint32_t container, states, bits, flags; /* flags: 1 walk, 2 mergeable, 4 carries its histogram */
  uint64_t decoded_len;
  uint32_t n_chains, n_pieces, shared_hist, interval;
} hsrans_plan_kind;
typedef struct hsrans_launch_facts
{
  uint32_t persistent;          /* a mergeable plan (raw with an index): chains of plan->interval groups, or of any length (0) */
  uint32_t table_mode, dual;    /* ... its host-built decode table (hsrans_launch_info.table_mode; 0: none) and two chains per wave */
  uint32_t n_groups;            /* block_/mt_ plan with checkpoints: its groups (a block, or a part of one); 0: none */
  uint32_t groups_lean;         /* ... 64 states, every group a run of single-piece chains or a single-symbol block */
  uint32_t spread_min_block;    /* ... the fewest chains of a coded block that is neither first nor last; 0: k_decode_spread cannot take the plan */
  uint32_t tickets;             /* ... the launch has a ticket counter for the groups behind the first round */
  uint32_t index_pass;          /* the launch records checkpoints */
  uint32_t single_valid, single_ring_entries; /* one chain of one rANS piece (a raw stream without an index) and its ring size */
  uint32_t calibrating;         /* hsrans_ctx_calibrate's launches */
  uint32_t parts, n_parts;      /* a sharded decode's sub-runs in one launch, and how many */
  uint32_t dealt;               /* the plan has a valid dealing (hsrans_dealt_shares returned 1) */
} hsrans_launch_facts;
int hsrans_launch_choice(const hsrans_ctx *ctx /* may be NULL: MI355X defaults, as hsrans_dealt_shares */, const hsrans_plan_kind *plan, const hsrans_launch_facts *facts,
                         hsrans_launch_info *info, char *kernel_name, size_t name_capacity);

/* diagnostics: with HSRANS_DEBUG_STAMPS=1 in the environment every wavefront of a persistent / direct launch records
 * s_memtime stamps {entry, table built, stream ready, done, static share done} in 8 slots; copies up to capacity_u64 values to
 * `out`, returns the count */
size_t hsrans_debug_read_stamps(hsrans_dplan *dplan, uint64_t *out, size_t capacity_u64);

const char *hsrans_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HSRANS_HIP_H */
