/*
 * flate_hip.h -- C ABI of libflate_hip.so: the MI355X (gfx950) batch engine for
 * the deflate-fast encode path (and batch inflate) of gmlewis/moonbit-flate.
 *
 * The reference has no FFI of its own (pure MoonBit); the
 * natural seam is Compressor::enc_speed (reference deflate.mbt:236-277), which
 * takes window[:window_end] plus the persistent DeflateFast {table, cur} and
 * appends DEFLATE bytes to the sink.  This ABI generalises that seam to N
 * independent streams ("fresh Writer per stream"): for every stream i the bytes
 * produced equal  Writer::new(buf) ; write(in[in_off[i]:in_off[i+1]]) ; close()
 * (reference writer.mbt:10,45,53 -> deflate.mbt:280-294,157-183), bit for bit.
 *
 * Plain pointers and sizes only; no torch / C++ types.  One ctx per host thread;
 * calls on distinct contexts are independent.  The caller owns every buffer; the
 * library retains no pointer after a call returns.  Errors: 0 = ok, negative enum
 * below, never abort (the reference's sticky IOError / abort() become codes).
 */
#ifndef FLATE_HIP_H
#define FLATE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct flate_hip_ctx flate_hip_ctx;

/* error codes */
#define FLATE_HIP_OK 0
#define FLATE_HIP_E_INVALID (-1)        /* bad argument                               */
#define FLATE_HIP_E_OUT_TOO_SMALL (-2)  /* out_cap / slot too small                    */
#define FLATE_HIP_E_HIP (-3)            /* HIP runtime failure (see strerror)         */
#define FLATE_HIP_E_CORRUPT (-4)        /* inflate: corrupt_input_error (inflate.mbt:38) */
#define FLATE_HIP_E_NO_DEVICE (-5)      /* no usable GPU: the engine has no CPU path  */
#define FLATE_HIP_E_TOO_LARGE (-6)      /* batch calls: a stream with an LZ77 window at index 32 766
                                           (> 2 147 319 937 bytes; where the reference's `cur` reaches
                                           buffer_reset and shift_offsets runs, deflate-fast.mbt:55,
                                           130-132) or >= 2 GiB - 128 KiB with FLATE_HIP_COMPAT_GO:
                                           write such a stream with flate_hip_stream_write, which follows
                                           the reference through shift_offsets                        */
#define FLATE_HIP_E_UNEXPECTED_EOF (-7) /* inflate: err_unexpected_eof (inflate.mbt:781) */
#define FLATE_HIP_E_AGAIN (-9)          /* flate_hip_gather_end: a shard outgrew the agreed pad, or a
                                           rank holds more streams than the plan allows for; the
                                           plan has been raised on every rank: repeat this batch
                                           with flate_hip_gather_compressed                      */
#define FLATE_HIP_E_UNSUPPORTED (-10)   /* ZIP: an entry that is encrypted, patched, or of a method other than 0
                                           and 8 (that entry's status) */
#define FLATE_HIP_E_INTERNAL (-8)       /* encoder self-check failed (the reference abort()s on its
                                           invariants, deflate.mbt:111, huffman-code.mbt:118,232):
                                           packed bits != the size computed before packing;
                                           flate_hip_last_hip_error names the stream            */

/* flags */
#define FLATE_HIP_DEVICE_PTRS 0x1u /* in/out (and tokens/recs) are device pointers; offset
                                      tables are always host arrays                     */
#define FLATE_HIP_COMPAT_GO 0x2u   /* Go 1.23.1 semantics: fixes divergences D1
                                      (deflate-fast.mbt:157,310) and D2
                                      (huffman-bit-writer.mbt:527,780); default is the
                                      reference's own (MoonBit) behaviour                */
#define FLATE_HIP_LZ_SERIAL 0x4u   /* debug: single-lane match finder kernel            */
#define FLATE_HIP_SIZE_ONLY 0x8u   /* flate_hip_inflate_batch: decode without storing -- out may be
                                      NULL and out_off is ignored; out_len[i] = the bytes stream i
                                      inflates to (up to its error, if any), status / err_off as in
                                      a real pass.  The kernels count output in 32 bits: a stream
                                      that inflates to 4 GiB or more gets FLATE_HIP_E_TOO_LARGE
                                      (decode it with flate_hip_inflate_stream_read).  What a batch
                                      caller that needs sizes runs first, instead of guessing a
                                      capacity and retrying                                    */

/* -- lifecycle ------------------------------------------------------------------
 * replaces: Writer::new (writer.mbt:10) / Compressor::new (deflate.mbt:81) state
 * allocation; one ctx holds the scratch for any number of streams. */
int flate_hip_init(int device, flate_hip_ctx **ctx);
void flate_hip_destroy(flate_hip_ctx *ctx);
/* Run on the caller's HIP stream (hipStream_t passed as void*), e.g. torch's
 * current stream; NULL = the ctx's own stream. */
int flate_hip_set_stream(flate_hip_ctx *ctx, void *hip_stream);
/* Tuning knobs of the match finder's launch geometry (results never change):
 *   "guest_blocks"       extra persistent wavefronts whose hash table lives in L2 instead of LDS
 *                        (default 6 per CU: 4 LDS-table + 6 guest blocks fill the 128 LDS granules of a
 *                        CU; larger values displace LDS-table blocks and are slower; 0 = off)
 *   "resident_blocks"    persistent LDS-table wavefronts (default 4 per CU)
 *   "guest_min_streams"  batches smaller than this use one block per stream (default 5 per CU = 1280)
 *   "window_units"       1 (default): multi-window streams of a persistent launch are scheduled one
 *                        65535-byte window at a time (a stream's table rests in global memory
 *                        between its windows); 0: one block keeps a stream from start to end
 *   "host_pipeline_groups"  host-pointer calls of flate_hip_deflate_fast_batch / flate_hip_inflate_batch
 *                        on >= 64 MiB: the batch is cut into this many groups of streams (each at
 *                        least 2048 streams, for inflate 8192) and
 *                        group g is compressed while group g+1 is copied in and the output of g-1
 *                        is copied out (default 8; 0 or 1: copy in, compress, copy out).  The
 *                        groups hold equal BYTES (not equal stream counts).  Such a call starts
 *                        two copy threads (and, for the encoder, "host_pipeline_lanes" compute
 *                        threads) of its own for its duration.  If it fails part-way
 *                        (FLATE_HIP_E_OUT_TOO_SMALL, a HIP error) out and out_off are partly
 *                        written and must not be used; inflate: a failing stream does not stop
 *                        the batch, every stream's status is reported as in one pass
 *   "host_pipeline_group_streams"  smallest group of such a call (default 2048 streams)
 *   "host_pipeline_lanes"  2 (default): the groups of a host-pointer encode call alternate between two
 *                        lanes (sub-contexts with their own HIP streams and scratch, one host thread
 *                        each), so that the match finder of group g+1 fills the chip while group g's
 *                        last streams, entropy kernels and size read-back drain; 1: one lane
 *   "entropy_per_block"  -1 (default): the histogram and pack kernels run one wavefront per BLOCK
 *                        instead of per stream when the batch's streams have three or more blocks
 *                        on average; 0 = never; 1 = whenever every stream has a block
 *   "inflate_simt_min_streams"  inflate batches at least this large decode one stream per LANE
 *                        (64 per wavefront) instead of one per wavefront (default 2049)
 *   "inflate_spec"       the third decoder -- one wavefront per stream, 64 sub-blocks of the bit
 *                        stream decoded at once from guessed token starts, repeated until the
 *                        starts agree: 0 = never, 1 = for batches below
 *                        "inflate_spec_max_streams" streams (default 45056), 2 = always
 *   "inflate_spec_shape" which build of it: 0 (default) = by batch size, 1 = the small-batch one
 *                        (long token lists, 16 KiB history ring), 2 = the large-batch one
 *   "inflate_lanes"      streams per wavefront of that decoder: 0 = chosen from the batch size
 *                        (default), or 16 / 32 / 64
 *   "inflate_row_dwords" the lane-per-stream decoder's output row (64-lane form): a lane collects
 *                        this many dwords of its output in registers and stores whole aligned
 *                        pieces: 0 = every store goes straight to memory, 8 (default), 16
 *   "spin_limit_polls"   the persistent kernels' waits (a window that another block is still
 *                        producing) give up after this many
 *                        polls and the call returns FLATE_HIP_E_INTERNAL (default 8 Mi polls,
 *                        several seconds of a running wave; time spent preempted does not count)
 *   "stream_rebase_bytes"  flate_hip_stream_*: a stream longer than this moves the origin of the
 *                        32-bit positions its kernels count in (all distances stay what they were);
 *                        default 1 GiB, read when the stream is opened; results never change
 *   "zip_unit_min"       flate_hip_zip_read: 0 (default) = every entry goes to the batch decoders; v >= 1 = a deflated
 *                        entry of at least v compressed bytes is decoded through units (ZIP archives, below)
 *   "zip_piece_bytes"    flate_hip_zip_write: 0 (default) = every entry is one stream, written by one wavefront; P >= 1
 *                        = an entry longer than P bytes is written from ceil(len / P) pieces compressed in parallel
 *                        and spliced into one stream (ZIP archives, below)
 *   "gzfile_serial_max"  flate_hip_gzfile_index / _read only: 0 (default) = every member is cut into units; S >= 1
 *                        (at most 2^28 - 1, like "gzip_member_max") = a member whose header and raw stream fit in
 *                        S bytes and decode cleanly is ONE unit, decoded whole by the batch decoders.  Bytes,
 *                        out_len, status, bad_member, err_off, stream_err_off, n_members, member_off and the
 *                        trailer verdicts never change; n_units, unit_bit, out_off, member_unit and
 *                        n_candidates do (A gzip FILE of any members, below)
 *   "one_stored_units"   flate_hip_inflate_one* and flate_hip_gzfile_*: 0 (default) = a unit starts at bit 0
 *                        and at every dynamic block header; 1 = at every STORED block header too, so that a
 *                        run of stored blocks (incompressible data) is many units instead of one: it is
 *                        decoded in parallel, each unit has "one_unit_max" to itself, and seek points fall
 *                        inside it.  Bytes, status and err_off never change; unit_bit, out_off, n_units and
 *                        n_candidates do.  A seek index records the rule it was built with and is read
 *                        with that rule whatever the reading ctx's option says
 *   "debug_buffer_reset"  test hook: buffer_reset (deflate-fast.mbt:55) of the streams opened from now
 *                        on, so that the reference's shift_offsets can be reached in a few windows
 *                        instead of after 2.1 GB (0 = the reference's value)
 *   "debug_drop_window_push"  test hook: k > 0 loses the k-th window hand-over of the next
 *                        multi-window launch, so that the bounded wait can be exercised
 *   "debug_stall_batch"  test hook: k > 0 makes the k-th dense batch of every LZ77 window forget its
 *                        progress, so that the match finder's progress guard can be exercised (the
 *                        call returns FLATE_HIP_E_INTERNAL, "a match-finder batch made no progress") */
int flate_hip_set_option(flate_hip_ctx *ctx, const char *name, int64_t value);
const char *flate_hip_strerror(int code);
/* Hash of the sources this library was built from (moonbit-flate_amd/build.py: source_hash):
 * measurement files under profiles/ carry the id of the build they were collected on. */
const char *flate_hip_build_id(void);
/* Text of the last HIP runtime error seen by this ctx ("" if none). */
const char *flate_hip_last_hip_error(const flate_hip_ctx *ctx);

/* -- host buffers ---------------------------------------------------------------
 * The reference's Writer / Reader are handed host memory (writer.mbt:45, inflate.mbt:382); a host-pointer
 * call copies it over PCIe inside the call.  From PAGEABLE memory every such copy is staged through the
 * runtime's own bounce buffers; from page-locked memory it is one DMA transfer at the link's rate.  A
 * caller that keeps its buffers across calls registers them once (the page-locking itself costs about
 * as much as one copy of the buffer, and touches every page: a fresh output buffer is also faulted in
 * here instead of inside the first call) or lets the library allocate page-locked memory.  The calls
 * themselves are unchanged: they recognise registered ranges by address. */
int flate_hip_host_register(flate_hip_ctx *ctx, void *ptr, size_t bytes);
int flate_hip_host_unregister(flate_hip_ctx *ctx, void *ptr);
int flate_hip_host_alloc(flate_hip_ctx *ctx, size_t bytes, void **ptr);
int flate_hip_host_free(flate_hip_ctx *ctx, void *ptr);

/* -- encode ---------------------------------------------------------------------
 * Upper bound of the compressed size of one stream of in_len bytes. */
size_t flate_hip_deflate_bound(size_t in_len);

/* replaces: Writer::write + Writer::close (writer.mbt:45,53; deflate.mbt:280,157)
 * for n_streams independent streams.  in_off has n_streams+1 entries (host);
 * stream i is in[in_off[i] .. in_off[i+1]).  On return out holds the streams back
 * to back and out_off[0..n_streams] (host, written) their offsets. */
int flate_hip_deflate_fast_batch(flate_hip_ctx *ctx, const uint8_t *in,
                                 const uint64_t *in_off, uint32_t n_streams,
                                 uint8_t *out, uint64_t out_cap, uint64_t *out_off,
                                 uint32_t flags);

/* The same with PRESET DICTIONARIES as history: stream i is compressed as if its Writer had been handed its
 * dictionary first without producing output, and can only be read by a Reader initialised with the same dictionary
 * (&Reader::new_dict, flate_hip_inflate_batch_dict, zlib's inflateSetDictionary).  This is what the doc comment of
 * the reference's Writer::new_dict promises and Go / zlib implement; the reference's CODE (writer.mbt:25-31,
 * deflate.mbt:108-151) compresses the dictionary into the output as data, and the host mirror
 * flate_host::Writer::new_dict keeps doing that.  Exactly: d = the last 32768 bytes of the dictionary; a fresh
 * DeflateFast runs encode(d) once and its tokens are dropped (deflate-fast.mbt:123-270: the table holds what the
 * greedy parser inserts, `cur` advances by len(d)); the payload then goes through the unchanged Compressor driver
 * (65535-byte windows, enc_speed's size policy, close).  Consequences of that policy, kept as they are:
 *   - a dictionary of fewer than 17 bytes (after the cut) has no effect at all (:136-140);
 *   - a payload of fewer than 128 bytes gets nothing from its dictionary (deflate.mbt:243: it never reaches the
 *     match finder), and a final window of fewer than 128 bytes likewise;
 *   - with FLATE_HIP_COMPAT_GO matches extend into the dictionary and may run from the dictionary on into the
 *     payload (match_len's third regime, :335-341): the USEFUL mode.  Without it `prev` is empty: a
 *     candidate inside the dictionary yields a match of exactly length 4; the output is valid but usually LARGER
 *     than without a dictionary.
 * The dictionary arguments mean what they mean in flate_hip_inflate_batch_dict (a table of dictionaries,
 * dict_of[i] or FLATE_HIP_NO_DICT, dict_of == NULL = every stream uses dictionary 0, dicts host or device with
 * FLATE_HIP_DEVICE_PTRS) and get the same checks (FLATE_HIP_E_INVALID before any HIP call); everything else is
 * flate_hip_deflate_fast_batch's.  A call in which no stream has a dictionary of at least 17 bytes IS
 * flate_hip_deflate_fast_batch: same kernels, same bytes.  Every used dictionary is run through the match finder
 * ONCE per call (not once per stream); its streams start from a copy of the resulting table.
 *   FLATE_HIP_LZ_SERIAL together with such a dictionary: FLATE_HIP_E_INVALID (the debug kernel has no dictionary
 *   build).  The dictionary is window 0 of its stream, so FLATE_HIP_E_TOO_LARGE comes one window earlier for a
 *   stream with one: at 0x7ffe0000 - 65535 bytes, and without FLATE_HIP_COMPAT_GO at 32766 LZ77 windows instead of
 *   32767.  flate_hip_deflate_bound is unchanged.  A host-pointer call is copied in and out in one piece (no
 *   "host_pipeline_groups").
 * Out of scope: dictionaries for flate_hip_stream_write, flate_hip_deflate_fast_spliced, flate_hip_lz77_matches
 * and across ranks (flate_hip_gather_*). */
int flate_hip_deflate_fast_batch_dict(flate_hip_ctx *ctx, const uint8_t *in, const uint64_t *in_off,
                                      uint32_t n_streams,
                                      const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts,
                                      const uint32_t *dict_of,
                                      uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint32_t flags);

/* ONE stream written in pieces -- Writer::write as the reference behaves: compressed bytes leave
 * while later input is still to come (Compressor::write -> fill_store / enc_speed per full
 * 65535-byte window, deflate.mbt:280-294,222-229,236-277; the sink sees output every >= 240
 * bytes, huffman-bit-writer.mbt:193-196) instead of everything at close.  The concatenation of
 * the pieces' output is, bit for bit, what flate_hip_deflate_fast_batch produces for the whole
 * stream (= Writer::new; write(all); close()).  Between two pieces the stream's DeflateFast state
 * (hash table, position; deflate-fast.mbt:104-117,156) rests on the device together with the last
 * 32 KiB of input (max_match_offset) and the bits of the last incomplete output byte.
 *   n: a multiple of 65535 (whole windows) unless final; final != 0: any n (also 0), ends the
 *   stream with Writer::close's block (deflate.mbt:171-176).  in / out are HOST buffers;
 *   out_cap >= flate_hip_stream_bound(n).  Errors are sticky (Compressor.err, deflate.mbt:74):
 *   after a failed or a final write every further write fails.  The stream may be of any length;
 *   one piece is < 1 GiB.  Where the reference's `cur` reaches buffer_reset (window 32 766 of a
 *   Writer, then every 32 767 windows: deflate-fast.mbt:55,130-132) its shift_offsets runs
 *   (:366-389), and so does this: in the default compat mode `prev` is empty, so the
 *   table is CLEARED (:367-374) and the window starts without history; with FLATE_HIP_COMPAT_GO the
 *   offsets move down and every distance stays what it was.  (Independently of that the origin of
 *   the kernels' 32-bit positions moves up every "stream_rebase_bytes"; that changes no result.)
 *   One wavefront compresses one
 *   stream: this is the reference's semantics for a long stream, not the engine's fast path
 *   (batches of streams are). */
typedef struct flate_hip_stream flate_hip_stream;
int flate_hip_stream_open(flate_hip_ctx *ctx, uint32_t flags, flate_hip_stream **stream);
size_t flate_hip_stream_bound(size_t n);
int flate_hip_stream_write(flate_hip_stream *stream, const uint8_t *in, uint64_t n, int final,
                           uint8_t *out, uint64_t out_cap, uint64_t *out_len);
void flate_hip_stream_free(flate_hip_stream *stream);

/* Match-finder only (replaces DeflateFast::encode, deflate-fast.mbt:123-270), for
 * token-stream parity tests.  A stream is cut into LZ77 chunks exactly as
 * Compressor::enc_speed does (every full 65535-byte window, plus a final partial
 * window of >= 128 bytes).  For chunk c (global index, stream order):
 *   chunk_nmatch[c] matches, records at recs[2*chunk_rec_off[c] ...], each record
 *   = { position of the match start inside the chunk, token as token.mbt:76 }.
 * Literal tokens are implied: every byte not covered by a match (token.mbt:69).
 * Call with recs == NULL to query *n_chunks and *n_recs_cap. */
int flate_hip_lz77_matches(flate_hip_ctx *ctx, const uint8_t *in, const uint64_t *in_off,
                           uint32_t n_streams, uint32_t flags, uint32_t *n_chunks,
                           uint64_t *n_recs_cap, uint32_t *chunk_nmatch,
                           uint64_t *chunk_rec_off, uint32_t *recs);

/* -- decode ---------------------------------------------------------------------
 * replaces: &Reader::new + read to EOF (inflate.mbt:305,382) for n_streams
 * independent DEFLATE streams.  Stream i is in[in_off[i]..in_off[i+1]); its output
 * goes to out[out_off[i] .. out_off[i+1]) (capacity; bytes of the slot beyond out_len[i] are
 * unspecified afterwards); out_len[i] = bytes produced;
 * status[i] = 0 or a negative code; err_off[i] = input offset reported by
 * corrupt_input_error (or -1). Returns the first non-zero status.
 * With FLATE_HIP_DEVICE_PTRS a stream writes only inside its own slot -- nothing outside
 * out[out_off[0], out_off[n_streams]) is written, and nothing of another stream's slot -- and a stream that produces
 * no bytes (out_len[i] == 0) writes nothing at all.  With host pointers the slots are copied back as one range:
 * every byte of out[0, out_off[n_streams]) may be rewritten, the slot of a stream that produced nothing included, and
 * nothing behind it.  (The same holds for flate_hip_inflate_batch_dict, _spliced and _batch_framed.) */
int flate_hip_inflate_batch(flate_hip_ctx *ctx, const uint8_t *in, const uint64_t *in_off,
                            uint32_t n_streams, uint8_t *out, const uint64_t *out_off,
                            uint64_t *out_len, int32_t *status, int64_t *err_off,
                            uint32_t flags);

/* &Reader::new_dict(r, dict) (inflate.mbt:315-317) + read to EOF for n_streams independent streams: stream i
 * decodes as if its output started with its PRESET DICTIONARY, which has already been read -- the last 32768
 * bytes of it are the history (DictDecoder::new, dict-decoder.mbt:40-60), a distance may reach
 * min(32768, dict_len + bytes produced) back (:63-69, inflate.mbt:677-680), beyond that FLATE_HIP_E_CORRUPT.
 * Everything else -- in / in_off / out / out_off / out_len / status / err_off (counted from the stream's own
 * input), FLATE_HIP_SIZE_ONLY, FLATE_HIP_DEVICE_PTRS, the options -- as flate_hip_inflate_batch.
 *   dictionary j   = dicts[dict_off[j], dict_off[j+1]); dict_off: n_dicts + 1 entries, HOST array; dicts: host,
 *                    or device under FLATE_HIP_DEVICE_PTRS (like in).  An empty dictionary = none.
 *   dict_of[i]     = the dictionary of stream i, or FLATE_HIP_NO_DICT; HOST array of n_streams entries.
 *                    NULL: every stream uses dictionary 0.
 * FLATE_HIP_E_INVALID (before any HIP call): dict_off not monotone, a dict_of entry neither below n_dicts nor
 * FLATE_HIP_NO_DICT, dict_of == NULL with n_dicts == 0, dicts == NULL with non-empty dictionaries.  A call in
 * which no stream has a non-empty dictionary IS flate_hip_inflate_batch.  The used dictionaries' tails are
 * uploaded once per call; every decoder has a dictionary build, chosen when a stream of the launch has one. */
#define FLATE_HIP_NO_DICT 0xffffffffu
int flate_hip_inflate_batch_dict(flate_hip_ctx *ctx, const uint8_t *in, const uint64_t *in_off, uint32_t n_streams,
                                 const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts,
                                 const uint32_t *dict_of,
                                 uint8_t *out, const uint64_t *out_off, uint64_t *out_len,
                                 int32_t *status, int64_t *err_off, uint32_t flags);

/* ONE stream decoded in pieces -- Decompressor::read as the reference behaves (inflate.mbt:382-407): the
 * caller holds a piece of the compressed stream and room for a piece of the output, never the whole of
 * either; between two calls the decoder's state rests on the device: the 32 KiB window
 * (dict-decoder.mbt:29-60), the Huffman tables of the block in progress (h1 / h2), the bit position
 * inside the current byte (b / nb), a copy that did not fit (copy_len / copy_dist), final_flag
 * (inflate.mbt:252-290).  Results, statuses and error offsets are those of flate_hip_inflate_batch on
 * the whole stream (= the reference's), whatever the piece sizes.
 *   in[0, in_len): the next bytes of the stream, STARTING with the bytes an earlier call reported as
 *     unused (*in_used < in_len: move the rest to the front and append new data); final_in != 0: the
 *     stream has no bytes behind these.  Unless final_in is set a call stops in front of a token it cannot
 *     be sure to have whole (8 bytes; 600 bytes in front of a block header), so pieces should be a few
 *     KiB at least; a call that cannot use anything returns FLATE_HIP_OK with *in_used = *out_len = 0.
 *   out[0, out_cap): receives *out_len bytes.
 *   returns FLATE_HIP_OK: call again (more input if the rest is short, more room if *out_len == out_cap);
 *     FLATE_HIP_STREAM_END: the final block has been decoded -- reported together with the last bytes,
 *     as Decompressor::read hands out io.EOF (:394-397); a negative code: the stream's error, sticky
 *     (FLATE_HIP_E_CORRUPT with *err_off = corrupt_input_error's offset counted from the start of the
 *     stream, FLATE_HIP_E_UNEXPECTED_EOF when final_in was set and the stream is not complete); the
 *     bytes decoded in front of the error are delivered (:402-404).  in / out are HOST buffers; one
 *     call takes at most 1 GiB each way.  One wavefront decodes one stream: the reference's semantics
 *     for a long stream, not the engine's fast path (flate_hip_inflate_batch / _spliced are; batches of
 *     streams with preset dictionaries: flate_hip_inflate_batch_dict). */
typedef struct flate_hip_inflate_stream flate_hip_inflate_stream;
#define FLATE_HIP_STREAM_END 1
int flate_hip_inflate_stream_open(flate_hip_ctx *ctx, flate_hip_inflate_stream **stream);
int flate_hip_inflate_stream_read(flate_hip_inflate_stream *stream, const uint8_t *in, uint64_t in_len,
                                  int final_in, uint8_t *out, uint64_t out_cap, uint64_t *in_used,
                                  uint64_t *out_len, int64_t *err_off);
/* Decompressor::reset(r, dict) (inflate.mbt:862-884) and &Reader::new_dict(r, dict) (:315-317): the handle
 * becomes a fresh decoder (open = reset without a dictionary), optionally with a PRESET DICTIONARY: the
 * stream decodes as if its output started with `dict`, which has already been read -- the last 32768
 * bytes of it are kept as history (DictDecoder::new, dict-decoder.mbt:40-60), a distance may reach
 * min(32768, dict_len + bytes produced) back (:63-69, inflate.mbt:677-680).  dict is a HOST buffer, not
 * retained; dict_len = 0: none.  (The encoder side of ONE stream, Writer::new_dict, is outside this path: in the
 * reference it compresses the dictionary into the output as data; batches of streams that NEED their
 * dictionary to be read: flate_hip_deflate_fast_batch_dict.) */
int flate_hip_inflate_stream_reset(flate_hip_inflate_stream *stream, const uint8_t *dict, uint64_t dict_len);
void flate_hip_inflate_stream_free(flate_hip_inflate_stream *stream);

/* The same for the n_streams pieces of ONE spliced stream in[0, in_len) (as written by
 * flate_hip_deflate_fast_spliced): piece i starts at bit bit_off[i] (host array, n_streams+1
 * entries) and is decoded on its own -- the encoder's pieces never reference one another --
 * until the bit where piece i+1 starts; the last piece runs through the closing block.
 * This is what a single Reader over the whole stream produces (inflate.mbt:305,382), cut at
 * the index.  status[i] = E_CORRUPT also if the index does not point at block boundaries. */
int flate_hip_inflate_spliced(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len,
                              const uint64_t *bit_off, uint32_t n_streams, uint8_t *out,
                              const uint64_t *out_off, uint64_t *out_len, int32_t *status,
                              int64_t *err_off, uint32_t flags);

/* -- checksums for the container formats around a raw stream (optional gzip / zlib wrappers;
 * the reference has neither) ------------------------------------------------------
 * out[i] = the Adler-32 (RFC 1950 section 8.2: what a zlib stream carries behind its data, big endian) or
 * the CRC-32 (RFC 1952 section 8: what a gzip member carries, little endian, followed by the length mod
 * 2^32) of stream i = in[in_off[i], in_off[i+1]).  in: host, or device with FLATE_HIP_DEVICE_PTRS; in_off and
 * out: host.  Streams of any length: the work is cut into 64 KiB pieces, so one long stream fills the chip
 * as a batch of short ones does.  WRITING members -- header, raw stream, trailer, in place on the device -- is
 * flate_hip_deflate_fast_batch_framed / _spliced_framed below; READING them (header parsing, the check of the
 * trailer against what was decoded) is flate_hip_inflate_batch_framed. */
#define FLATE_HIP_CHECKSUM_ADLER32 1
#define FLATE_HIP_CHECKSUM_CRC32 2
int flate_hip_checksum_batch(flate_hip_ctx *ctx, const uint8_t *in, const uint64_t *in_off, uint32_t n_streams,
                             uint32_t kind, uint32_t *out, uint32_t flags);

/* -- splice ---------------------------------------------------------------------
 * SURVEY 8(f)-3; no counterpart in the reference, whose Writer makes one stream per
 * Writer.  Same compression as flate_hip_deflate_fast_batch (stream i is encoded as a
 * fresh Writer would: writer.mbt:10,45; deflate.mbt:92,280), but the whole batch comes
 * out as ONE legal DEFLATE stream that inflates to the concatenation of the inputs:
 * every block starts at the bit where the previous stream's last block ended, stored
 * blocks are padded relative to the spliced stream (write_stored_header -> flush,
 * huffman-bit-writer.mbt:474-487,139-158) and the closing block of Writer::close
 * (deflate.mbt:171-176: empty stored block, BFINAL=1) is written once, at the end.
 * All other blocks carry BFINAL=0 (deflate.mbt:251,267,269).  *out_len = bytes of the
 * stream; bit_off (host, n_streams+1 entries, may be NULL) = bit position of every
 * stream's first block (the stream index a parallel decoder needs).  out_cap must be
 * at least the result + 3 bytes (sum of flate_hip_deflate_bound is always enough). */
int flate_hip_deflate_fast_spliced(flate_hip_ctx *ctx, const uint8_t *in,
                                   const uint64_t *in_off, uint32_t n_streams, uint8_t *out,
                                   uint64_t out_cap, uint64_t *out_len, uint64_t *bit_off,
                                   uint32_t flags);

/* -- containers: zlib and gzip members, framed on the device ----------------------
 * SURVEY 8(f)-3; the reference has no container format.  flate_hip_deflate_fast_batch_framed is
 * flate_hip_deflate_fast_batch -- or, with dictionary arguments, flate_hip_deflate_fast_batch_dict: their
 * arguments, checks, limits and flags -- with every stream inside its container: member i is
 * out[out_off[i], out_off[i+1]) = header | exactly the bytes the raw call produces for stream i | trailer, the
 * members back to back.
 *   FLATE_HIP_WRAP_ZLIB (RFC 1950)  header 78 01; trailer: the Adler-32 of the INPUT of stream i, big endian.
 *   FLATE_HIP_WRAP_GZIP (RFC 1952)  header 1f 8b 08 00 00 00 00 00 04 ff (no name, no time, XFL = fastest, OS
 *                                   unknown); trailer: CRC-32, then the input's length mod 2^32, little endian.
 *   FLATE_HIP_WRAP_RAW              IS the raw call: the same kernels, the same bytes.
 *   An empty stream is header | 01 00 00 ff ff | the checksum of nothing (Adler-32 = 1, CRC-32 = 0).
 * Dictionaries (zlib only): dicts == NULL, n_dicts == 0 and dict_of == NULL together mean none; otherwise the
 * four arguments are flate_hip_deflate_fast_batch_dict's and get its FLATE_HIP_E_INVALID checks.  Stream i gets
 * the six-byte header 78 3f | DICTID (FDICT, RFC 1950 2.2) exactly when dict_of names a dictionary for it
 * (dict_of == NULL: every stream uses dictionary 0); a stream with FLATE_HIP_NO_DICT gets 78 01.  DICTID is the
 * Adler-32 of the WHOLE dictionary as given, big endian -- not of the 32 KiB tail the match finder uses, and
 * also for a dictionary too short to have any effect (an empty one: DICTID 1).  The trailer is always the
 * payload's checksum.
 *   FLATE_HIP_E_INVALID, before any HIP call: an unknown wrap; FLATE_HIP_WRAP_GZIP with any dictionary argument.
 *   out_cap: the framed total is enough, to the byte (one byte less: FLATE_HIP_E_OUT_TOO_SMALL, decided on the
 *   device by the scan, as in the raw call); sum of flate_hip_deflate_bound + n_streams *
 *   flate_hip_frame_overhead is always enough.  n_streams == 0: out_off[0] = 0, FLATE_HIP_OK.
 *   in, out, dicts: host buffers, or device buffers under FLATE_HIP_DEVICE_PTRS; out may have any byte alignment.
 *   A host-pointer call is copied in ONCE, in one piece, and out once (no "host_pipeline_groups", as
 *   flate_hip_deflate_fast_batch_dict): the checksums run on the staged copy, and for the DICTIDs the whole
 *   dictionaries are uploaded, not only their tails.
 * How: the entropy stage knows every stream's exact size before it writes, so a scan that adds header and
 * trailer places the members and the pack kernels write each raw stream straight into its member; the checksum
 * kernels run on the input where it already is, and one small kernel writes headers and trailers last.  With
 * profiling on, the checksum and frame kernels are reported as FLATE_HIP_STAGE_CHECKSUM beside the two encode
 * stages.
 *
 * flate_hip_deflate_fast_spliced_framed: out[0, *out_len) = header | exactly the stream
 * flate_hip_deflate_fast_spliced writes | trailer over the CONCATENATED input in[in_off[0], in_off[n_streams])
 * (ISIZE: that length mod 2^32) -- the one .gz / zlib blob that gzip -d or zlib's uncompress turn back into the
 * whole buffer.  bit_off (may be NULL) is counted from the first byte of the raw stream, out + header length (2
 * or 10): its values are the unframed call's, and flate_hip_inflate_spliced_framed takes the member and this index as they are.
 * n_streams == 0: header | 01 00 00 ff ff | the trailer of nothing.  out_cap >= header + raw stream + trailer is
 * enough (the unframed call's 3 spare bytes lie inside the trailer).  No dictionaries; FLATE_HIP_WRAP_RAW is the
 * unframed call; an unknown wrap: FLATE_HIP_E_INVALID.
 *
 * flate_hip_frame_overhead (host only): the bytes a member adds around its raw stream -- RAW 0; ZLIB 6, with
 * with_dict != 0: 10; GZIP 18; an unknown wrap 0.
 * Reading members: flate_hip_inflate_batch_framed and flate_hip_inflate_spliced_framed below. */
#define FLATE_HIP_WRAP_RAW 0u
#define FLATE_HIP_WRAP_ZLIB 1u /* RFC 1950 */
#define FLATE_HIP_WRAP_GZIP 2u /* RFC 1952 */
size_t flate_hip_frame_overhead(uint32_t wrap, int with_dict);
int flate_hip_deflate_fast_batch_framed(flate_hip_ctx *ctx, const uint8_t *in, const uint64_t *in_off,
                                        uint32_t n_streams, uint32_t wrap,
                                        const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts,
                                        const uint32_t *dict_of,
                                        uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint32_t flags);
int flate_hip_deflate_fast_spliced_framed(flate_hip_ctx *ctx, const uint8_t *in, const uint64_t *in_off,
                                          uint32_t n_streams, uint32_t wrap, uint8_t *out, uint64_t out_cap,
                                          uint64_t *out_len, uint64_t *bit_off, uint32_t flags);

/* GROUPED SPLICE: several spliced members in one call, so that a batch in which some members are long is written by
 * as many wavefronts as it has pieces.  The n_pieces pieces in[in_off[i], in_off[i+1]) are compressed independently;
 * group g = the pieces [group_off[g], group_off[g+1]) becomes member g = out[out_off[g], out_off[g+1]): header |
 * exactly the bytes flate_hip_deflate_fast_spliced produces for the pieces of group g under the same flags | trailer
 * over the group's (contiguous) input; FLATE_HIP_WRAP_RAW: the bare stream.  Members lie back to back; out_off
 * (n_groups + 1 entries, HOST) is never optional.
 *   group_off (HOST, n_groups + 1 entries): group_off[0] == 0, group_off[n_groups] == n_pieces, strictly increasing --
 *     every group has at least one piece; an empty member is one piece of zero bytes.  Anything else, an unknown wrap
 *     or flag, or a missing pointer: FLATE_HIP_E_INVALID before any HIP call.
 *   bit_off (HOST, n_pieces + n_groups entries, may be NULL): group g's index is
 *     bit_off[group_off[g] + g .. group_off[g+1] + g], n_g + 1 entries counted from the first byte of the member's raw
 *     stream: what flate_hip_deflate_fast_spliced_framed returns, so flate_hip_inflate_spliced_framed takes a member
 *     and its slice as they are.
 *   out_cap: the exact total is enough for ZLIB and GZIP; FLATE_HIP_WRAP_RAW needs the total + 3, as the unframed
 *     spliced call (the pack kernel stores whole dwords).  Too little: FLATE_HIP_E_OUT_TOO_SMALL, decided on the
 *     device, nothing written.
 *   flags: FLATE_HIP_DEVICE_PTRS (in and out), FLATE_HIP_COMPAT_GO.  Host pointers: one copy in, one copy out, no
 *     "host_pipeline_groups".  n_groups == 0: out_off[0] = 0, FLATE_HIP_OK.
 *   How: the positions of pieces inside a spliced stream compose as maps x -> x + a / x -> align8(x + a) + b; the end
 *     of a member -- closing block, trailer, next header -- is one more map of that form (csrc/splice_rule.h), so one
 *     scan places every piece of every member, the pack kernel writes a closing block at every group's end, and one
 *     thread per group writes header and trailer last.  Stage accounting: the framed calls'.
 *   Out of scope: dictionaries, BGZF, grouping across ranks, pieces that share history, and choosing the piece size
 *     per member.  (ZIP entries in pieces: the option "zip_piece_bytes" of flate_hip_zip_write.) */
int flate_hip_deflate_fast_grouped_framed(flate_hip_ctx *ctx, const uint8_t *in, const uint64_t *in_off,
                                          uint32_t n_pieces, const uint32_t *group_off, uint32_t n_groups,
                                          uint32_t wrap, uint8_t *out, uint64_t out_cap, uint64_t *out_off,
                                          uint64_t *bit_off, uint32_t flags);

/* ONE long raw, zlib or gzip stream WRITTEN IN PARTS through bounded buffers: flate_hip_deflate_fast_spliced_framed for
 * a caller that has neither the whole input nor room for the whole output (a 40 GB dump turned into a .gz through
 * two fixed buffers).  The handle carries the stream between calls; its state rests on the device.
 *   open: wrap = FLATE_HIP_WRAP_RAW / _ZLIB / _GZIP.  piece_bytes = P, the bytes of a piece (0: 65535; P must be below
 *     0x7ffe0000).  flags: a subset of FLATE_HIP_DEVICE_PTRS | FLATE_HIP_COMPAT_GO, fixed for the handle's life.
 *     Anything else: FLATE_HIP_E_INVALID before any HIP call.
 *   THE STREAM: with T the total input of all calls, the concatenation of every call's out[0, *out_len) is, byte for
 *     byte, what flate_hip_deflate_fast_spliced_framed writes for that input with in_off = {0, P, 2P, ..., T} (ceil(T /
 *     P) pieces; T == 0: n_streams == 0), the same wrap and the same flags; the concatenation of every call's bit_off
 *     is that call's bit_off, counted from the raw stream's first byte.  Both hold for ANY cut of the input into parts:
 *     the pieces are independent, and where a piece's blocks fall depends on the start position only modulo 8.
 *   write: in[0, in_len) begins with the bytes the last call left unused (flate_hip_one_reader_read's convention).  A
 *     call that is not final consumes k = floor(in_len / P) whole pieces, *in_used = k * P; with in_len < P it returns
 *     FLATE_HIP_OK with *in_used = *out_len = 0 and launches nothing (the header is written only by a call with k >= 1
 *     or a final one).  A final call (final_in != 0) consumes everything -- the last piece is shorter, and there may
 *     be no piece at all.  The first call that writes anything starts with the container's header; a final call ends
 *     with the closing block and the trailer (CRC-32 or Adler-32 and ISIZE over all T bytes, ISIZE mod 2^32).  A call
 *     delivers the whole bytes that are finished: the 0..7 bits of the last, incomplete byte stay in the handle on the
 *     device and share the next call's first byte; a final call delivers everything.  *n_pieces = k.  bit_off: NULL,
 *     or a HOST array with room for in_len / P + 2 entries: the k pieces' start bits and, on a final call, one entry
 *     more, the end bit, where the closing block starts.  Returns FLATE_HIP_OK, or FLATE_HIP_STREAM_END for a final
 *     call that succeeded; after that every write is FLATE_HIP_E_INVALID until reset.
 *   Room: out_cap >= *out_len is enough to the byte; flate_hip_one_writer_bound(in_len, P) (host only) is enough for
 *     any call on at most in_len bytes, first and final included.  Too little: FLATE_HIP_E_OUT_TOO_SMALL with *out_len =
 *     the bytes needed, nothing written to out, the handle unchanged -- the same call repeated with room delivers the
 *     same bytes.  Nothing outside out[0, *out_len) is ever written, with device pointers too: the pack kernels (whole
 *     dwords, OR into shared ones) write into the handle's own device buffer, and exactly *out_len bytes are copied
 *     from it -- device pointers: a copy kernel that reads the length on the device; host pointers: one download.
 *   Errors: FLATE_HIP_E_INVALID (a NULL handle or pointer; decided before any HIP call), FLATE_HIP_E_OUT_TOO_SMALL,
 *     FLATE_HIP_E_TOO_LARGE (in_len >= 2^32, or the limits of flate_hip_deflate_fast_spliced on the pieces a call
 *     consumes) and FLATE_HIP_E_HIP in front of the commit point are repeatable and change nothing.  Behind the
 *     commit point -- the launch of the one kernel that moves the handle's state -- every failure is sticky until
 *     reset.  The stream itself may be of any length: positions are 64-bit.
 *   Host waits per call: one read-back of the result words (device pointers), plus the download (host pointers).  The
 *     carry byte, the running checksum, the length and the emitted byte count never pass through the host.
 *   Out of scope: pieces that share history, dictionaries, several members (BGZF in parts: flate_hip_bgzf_writer_*),
 *     overlapping the upload of part k + 1 with the compression of part k, range reads through the writer's index, the MoonBit binding. */
typedef struct flate_hip_one_writer flate_hip_one_writer;
size_t flate_hip_one_writer_bound(size_t in_len, size_t piece_bytes);
int flate_hip_one_writer_open(flate_hip_ctx *ctx, uint32_t wrap, uint64_t piece_bytes, uint32_t flags,
                              flate_hip_one_writer **writer);
int flate_hip_one_writer_write(flate_hip_one_writer *writer, const uint8_t *in, uint64_t in_len, int final_in,
                               uint8_t *out, uint64_t out_cap, uint64_t *in_used, uint64_t *out_len, uint64_t *bit_off,
                               uint32_t *n_pieces);
int flate_hip_one_writer_reset(flate_hip_one_writer *writer);
void flate_hip_one_writer_free(flate_hip_one_writer *writer);

/* READING members: flate_hip_inflate_batch -- its output slots, out_len, status, return value (the first non-zero
 * status), FLATE_HIP_DEVICE_PTRS, options and size limits -- for n_streams zlib or gzip members, member i =
 * in[in_off[i], in_off[i+1]) = header | raw stream | trailer.  Header parsing, decoding and the check of the trailer
 * against what was decoded all happen on the device, in one call, on one HIP stream: no host pass over member bytes, no
 * host synchronisation between decode and verification.
 *   Header, FLATE_HIP_WRAP_ZLIB (RFC 1950 2.2): CM = 8, CINFO <= 7, (CMF * 256 + FLG) % 31 == 0.  Without FDICT it is
 *     2 bytes; with FDICT 6, and the member's dictionary is the FIRST j whose Adler-32 over the whole of dictionary j
 *     equals DICTID (an empty dictionary has id 1).  FDICT with n_dicts == 0, or with an id that no dictionary has,
 *     is a bad header.  The trailer is 4 bytes.
 *   Header, FLATE_HIP_WRAP_GZIP (RFC 1952 2.3): 1f 8b, CM = 8, the reserved FLG bits zero; FEXTRA, FNAME, FCOMMENT and
 *     FHCRC are skipped, in that order (the scan for a terminating NUL ends at the member's end).  The trailer is 8
 *     bytes.  One range is one member: a file of several members is several ranges (a BGZF file:
 *     flate_hip_bgzf_read below finds them itself).
 *   A member too short for its header plus trailer has a bad header.
 *   The raw stream is exactly [member + header length, member end - trailer length): a stream that needs more bytes
 *     than that is FLATE_HIP_E_UNEXPECTED_EOF -- the decoder does not run on into the trailer.  Bytes between the end
 *     of the final block and the trailer are not examined: the trailer is the member's last 4 or 8 bytes.
 *   The verdict, in this order:
 *     1. a bad header: FLATE_HIP_E_CORRUPT, err_off = 0, out_len = 0;
 *     2. the decoder's own non-zero status: status and err_off as flate_hip_inflate_batch reports them for the raw
 *        stream alone (err_off counted from the raw stream's first byte); out_len = the bytes produced, delivered;
 *     3. a checksum that is not the trailer's -- zlib: the Adler-32 of the out_len[i] bytes produced, big endian;
 *        gzip: their CRC-32, little endian -- or, gzip, out_len mod 2^32 != ISIZE: FLATE_HIP_E_CORRUPT, err_off = the
 *        member's length; the bytes are delivered.
 *   dicts / dict_off / n_dicts (zlib only): the table of dictionaries of flate_hip_inflate_batch_dict (dict_off a HOST
 *     array of n_dicts + 1 entries, dicts host or device like in); all NULL / 0: none.  There is no dict_of: every
 *     member names its dictionary itself.  dict_used (HOST array of n_streams entries, may be NULL): entry i = the
 *     dictionary chosen for member i, or FLATE_HIP_NO_DICT.  The tail of EVERY non-empty dictionary is staged per call
 *     (which ones are used is known on the device only), and the decoders' dictionary build runs whenever a non-empty
 *     dictionary is passed.
 *   FLATE_HIP_SIZE_ONLY: as in flate_hip_inflate_batch -- and since nothing is stored, nothing can be summed: status
 *     covers the header and the decode only, NOT the trailer's checksum or ISIZE.
 *   FLATE_HIP_E_INVALID, before any HIP call: flate_hip_inflate_batch's checks; an unknown wrap; FLATE_HIP_WRAP_GZIP or
 *     FLATE_HIP_WRAP_RAW with any dictionary argument; dict_off not monotone; dicts == NULL with non-empty dictionaries.
 *   FLATE_HIP_WRAP_RAW (without dictionaries) IS flate_hip_inflate_batch: the same kernels, the same results (dict_used:
 *     FLATE_HIP_NO_DICT throughout).  n_streams == 0: FLATE_HIP_OK.  A host-pointer call is copied in ONCE, in one
 *     piece, and out once (no "host_pipeline_groups", as the framed write calls).
 * How: the DICTIDs are the checksum kernels over the whole dictionaries; a parse kernel (one thread per member) checks
 * the header, finds the raw stream, reads the trailer and matches the DICTID; the batch decoders read every stream's
 * range and dictionary from what it wrote; the checksum kernels then run over 64 KiB pieces planned over the output
 * SLOTS and clipped on the device to out_len[i]; a verdict kernel merges.  With profiling on, FLATE_HIP_STAGE_INFLATE is
 * the decoder alone and FLATE_HIP_STAGE_CHECKSUM the contiguous run of output checksums plus verdict (0 for a size-only
 * pass's sums: only the verdict kernel); the DICTID sums and the parse kernel run in front of the decoder's first
 * event and are counted in NO stage. */
int flate_hip_inflate_batch_framed(flate_hip_ctx *ctx, const uint8_t *in, const uint64_t *in_off,
                                   uint32_t n_streams, uint32_t wrap,
                                   const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts,
                                   uint8_t *out, const uint64_t *out_off, uint64_t *out_len,
                                   int32_t *status, int64_t *err_off, uint32_t *dict_used,
                                   uint32_t flags);

/* READING ONE member around a spliced stream: flate_hip_inflate_spliced -- its index, output slots (capacities: a
 * piece may produce less than its slot holds), out_len, status, err_off, FLATE_HIP_DEVICE_PTRS and slot-write
 * guarantees -- for in[0, in_len) = header | the raw spliced stream | trailer, as flate_hip_deflate_fast_spliced_framed
 * writes it or any other zlib / gzip writer around the same raw stream.  bit_off (HOST array, n_streams + 1 entries) is
 * counted from the first byte of the RAW stream, exactly as flate_hip_deflate_fast_spliced_framed returns it: the
 * header's length is found on the device, and no caller parses it.  Header parsing, decoding and the check of the
 * trailer against what was decoded all happen on the device, in one call, on one HIP stream: no host pass over member
 * bytes, no host synchronisation between decode and verification; host pointers mean one copy in and one copy out.
 *   Header: the rules of flate_hip_inflate_batch_framed (the same parse kernel over one range).  gzip: FEXTRA, FNAME,
 *     FCOMMENT and FHCRC are skipped.  zlib: FDICT is a bad header -- the spliced writer has no dictionaries and this
 *     call takes none.  A member too short for its header plus trailer has a bad header.
 *   The raw stream is exactly [header end, in_len - trailer length): a piece that needs bytes behind that range is
 *     FLATE_HIP_E_UNEXPECTED_EOF, and no decoder reads the trailer.  An index entry that lies behind that range once
 *     the header's length is added (a header longer than the shortest) is clamped to its end: the piece sees no input
 *     and reports FLATE_HIP_E_UNEXPECTED_EOF.
 *   The verdict, in this order (member_status and member_err_off may each be NULL):
 *     1. a bad header: every piece gets status FLATE_HIP_E_CORRUPT, err_off 0, out_len 0 and nothing is written to
 *        out; *member_status = FLATE_HIP_E_CORRUPT, *member_err_off = 0; returns FLATE_HIP_E_CORRUPT;
 *     2. a piece's own non-zero status: out_len, status and err_off are what flate_hip_inflate_spliced reports for the
 *        raw stream alone (err_off counted from the raw stream's first byte), the bytes are delivered;
 *        *member_status = the first non-zero piece status, *member_err_off = -1, no checksum is judged; returns that
 *        status;
 *     3. every piece 0, but the checksum of the logical concatenation out[out_off[i], out_off[i] + out_len[i]), i = 0
 *        .. n_streams - 1 -- zlib: Adler-32, big endian; gzip: CRC-32, little endian -- is not the trailer's, or, gzip,
 *        the sum of out_len mod 2^32 is not ISIZE: the statuses stay 0 and the bytes are delivered;
 *        *member_status = FLATE_HIP_E_CORRUPT, *member_err_off = in_len; returns FLATE_HIP_E_CORRUPT;
 *     otherwise *member_status = 0, *member_err_off = -1, FLATE_HIP_OK.
 *   FLATE_HIP_E_INVALID, before any HIP call: flate_hip_inflate_spliced's checks; an unknown wrap; bit_off not
 *     monotone; bit_off[n_streams] > 8 * (in_len - trailer length - shortest header: 6 bytes zlib, 18 gzip), or in_len
 *     below those; FLATE_HIP_SIZE_ONLY (the spliced calls have no size-only pass).  FLATE_HIP_E_TOO_LARGE as in the raw
 *     call (a piece of 2^30 bits or more).  n_streams == 0: FLATE_HIP_OK, nothing is read.
 *   FLATE_HIP_WRAP_RAW IS flate_hip_inflate_spliced: the same kernels, the same results; the member's two words are
 *     derived on the host as in case 2 and the last row.
 * How: the parse kernel measures the header; a rebase kernel (one thread per index entry) adds it to the uploaded
 * index, clamps, and on a bad header collapses every piece to an empty range; the spliced decoders then run unchanged
 * on the member up to its trailer (whole bytes are added: stored blocks keep their alignment); the checksum kernels
 * leave one finished sum per piece, a join kernel (one workgroup, a running count of the bytes behind every piece)
 * turns them into the concatenation's sum and length, and a verdict kernel applies the cases.  With profiling on,
 * FLATE_HIP_STAGE_INFLATE is the decoder alone and FLATE_HIP_STAGE_CHECKSUM the output sums plus the join plus the
 * verdict; the parse and rebase kernels are counted in NO stage. */
int flate_hip_inflate_spliced_framed(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint32_t wrap,
                                     const uint64_t *bit_off, uint32_t n_streams,
                                     uint8_t *out, const uint64_t *out_off, uint64_t *out_len,
                                     int32_t *status, int64_t *err_off,
                                     int32_t *member_status, int64_t *member_err_off, uint32_t flags);

/* -- BGZF files: written and read in one call each ------------------------------------
 * BGZF is the blocked gzip of the SAM/BAM specification (section 4.1; what bgzip, htslib and tabix read and write): a
 * gzip file (RFC 1952) of members of at most 65536 bytes, each of which carries its own size in an extra subfield
 * ('B' 'C', BSIZE = size - 1) and its output size in ISIZE, ended by a canonical empty member.  Such a file is its own
 * index, so it is the one form of multi-member gzip FILE this engine reads without a side index: member boundaries and
 * output slots are found on the device from the file's bytes.  gzip -d and every gzip reader read what is written
 * here.  (Multi-member files WITHOUT 'BC' subfields stay out of scope: several ranges for
 * flate_hip_inflate_batch_framed.)
 *
 * flate_hip_bgzf_write: block k = in[k * block_bytes, min((k + 1) * block_bytes, in_len)), n_blocks = ceil(in_len /
 * block_bytes); block_bytes 0 = FLATE_HIP_BGZF_BLOCK_DEFAULT, else 1 .. 65535 (one LZ77 window), anything else
 * FLATE_HIP_E_INVALID.  Member k = 1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 (htslib's) | BSIZE, little endian |
 * exactly the bytes flate_hip_deflate_fast_batch produces for block k under the same flags | the block's CRC-32 and
 * length, little endian; the members back to back, then the 28-byte EOF marker (the same 16 bytes, 1b 00 03 00, eight
 * zero bytes).  in_len == 0: the marker alone.  *out_len = the file's size; member_off (HOST, n_blocks + 1 entries,
 * may be NULL): where every member starts, member_off[n_blocks] = where the marker starts.
 *   This is the framed encode path: the scan adds 18 + 8 bytes per member and the marker, the pack kernels write into
 *   the members, the checksums run on the input where it is, the frame kernel writes headers, trailers and the marker.
 *   A member of more than 65536 bytes cannot be expressed (incompressible blocks near 65535 bytes): decided on the
 *   device by the scan, FLATE_HIP_E_TOO_LARGE, flate_hip_last_hip_error names the first such block, out must not be
 *   used.  out_cap: the exact total is enough, to the byte (less: FLATE_HIP_E_OUT_TOO_SMALL); flate_hip_bgzf_bound
 *   (host only; 0 for a refused block_bytes) always is.  FLATE_HIP_DEVICE_PTRS and FLATE_HIP_COMPAT_GO as in
 *   flate_hip_deflate_fast_batch_framed; other flags: FLATE_HIP_E_INVALID.  Host pointers: one copy in, one copy out.
 *
 * flate_hip_bgzf_index (discovery only): a member at offset p has all of: 1f 8b 08; FLG with FEXTRA set and the
 * reserved bits zero; XLEN >= 6; inside the XLEN bytes a well-formed run of subfields, the first of which with SI = 'B'
 * 'C' and SLEN = 2 gives BSIZE; total = BSIZE + 1 >= 12 + XLEN + 8; p + total <= in_len.  The first member is at 0,
 * member k + 1 starts where member k ends, the file ends where a member ends at in_len.  FNAME, FCOMMENT and FHCRC are
 * not examined here (the parse kernel handles them at decode time).  Anything else: FLATE_HIP_E_CORRUPT, *err_off = the
 * offset at which no member could be read, *n_members = the well-formed members in front of it, *out_bytes = 0.
 *   On success member_off[0 .. n] (member_off[n] = in_len) and out_off[0 .. n] (the exclusive prefix sum of the
 *   members' ISIZE, out_off[n] = *out_bytes) are exactly what flate_hip_inflate_batch_framed(FLATE_HIP_WRAP_GZIP) takes
 *   as in_off and out_off; *eof_marker = 1 if the last member is the canonical 28 bytes; *err_off = -1.  Both arrays
 *   are HOST arrays of index_cap entries, or both NULL: a query that returns only the counts.  index_cap < n + 1:
 *   FLATE_HIP_E_OUT_TOO_SMALL with the counts set.  in_len == 0: FLATE_HIP_OK, zero members.  More candidates than 32
 *   bits count: FLATE_HIP_E_TOO_LARGE.  eof_marker and err_off may be NULL.  in: host, or device under
 *   FLATE_HIP_DEVICE_PTRS (any alignment); nothing outside in[0, in_len) is read.
 *   How (bgzf_kernels.hip): every offset that passes the rule is a candidate (one pass with 16-byte loads, compacted in
 *   file order); every candidate finds the candidate at offset + total by binary search; the chain from offset 0 is
 *   ranked by pointer doubling -- log2 rounds instead of one dependent miss per member.  The result equals the serial
 *   walk on every input, also where compressed bytes look like member headers.  The kernels are counted in no
 *   profiling stage.
 *
 * flate_hip_bgzf_read: index, then flate_hip_inflate_batch_framed(FLATE_HIP_WRAP_GZIP) over every member into the
 * dense slots out_off, fed with the index the device has just produced (it comes back to the host once, 16 bytes per
 * member, behind its counts: decoder routing and checksum planning are host code).  Host pointers: the file is
 * uploaded once -- index and decode use the same staged copy -- and out[0, *out_len) downloaded once.
 *   A malformed chain: flate_hip_bgzf_index's return value and *err_off, *bad_member = the count of good members,
 *   *out_len = 0, nothing is written.  A total above out_cap: FLATE_HIP_E_OUT_TOO_SMALL, *out_len = the size needed,
 *   nothing is decoded.  Otherwise every member is decoded (a failing member does not stop the others), *out_len =
 *   out_off[n], and the return value is the first non-zero member status as flate_hip_inflate_batch_framed defines it
 *   (FLATE_HIP_E_CORRUPT: bad header, CRC or ISIZE mismatch; FLATE_HIP_E_UNEXPECTED_EOF: the raw stream is cut short;
 *   FLATE_HIP_E_OUT_TOO_SMALL: the member produces more than its ISIZE) with *bad_member = its index and *err_off =
 *   its file offset; on success 0xffffffff and -1.  n_members, bad_member, err_off and eof_marker may each be NULL.
 *   The slot-write guarantees of flate_hip_inflate_batch hold. */
#define FLATE_HIP_BGZF_BLOCK_DEFAULT 65280u /* 0xff00, what bgzip cuts at */
#define FLATE_HIP_BGZF_MEMBER_MAX 65536u
#define FLATE_HIP_BGZF_EOF_BYTES 28u
size_t flate_hip_bgzf_bound(uint64_t in_len, uint32_t block_bytes);
int flate_hip_bgzf_write(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint32_t block_bytes,
                         uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *member_off, uint32_t flags);
int flate_hip_bgzf_index(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint64_t index_cap,
                         uint64_t *member_off, uint64_t *out_off, uint32_t *n_members, uint64_t *out_bytes,
                         int *eof_marker, int64_t *err_off, uint32_t flags);
int flate_hip_bgzf_read(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap,
                        uint64_t *out_len, uint32_t *n_members, uint32_t *bad_member, int64_t *err_off,
                        int *eof_marker, uint32_t flags);

/* -- BGZF random access: byte and virtual-offset ranges in one call --------------------
 * BGZF exists for random access: a BAM, tabix or CSI index stores VIRTUAL FILE OFFSETS (coffset << 16 | uoffset: the
 * file offset of a member, and a position in that member's output), and a region query is a list of chunks [v_begin,
 * v_end); bgzip -b/-s does the same with plain byte positions.  flate_hip_bgzf_read_ranges takes a batch of such ranges,
 * decodes the members they touch -- each ONCE, however many ranges touch it -- and delivers the requested bytes back to
 * back.
 *
 * Notation: U = the file's uncompressed bytes (what flate_hip_bgzf_read delivers), T their count, member_off[0 .. n]
 * and out_off_m[0 .. n] what flate_hip_bgzf_index defines, ISIZE[k] = out_off_m[k + 1] - out_off_m[k].
 * begin, end: HOST arrays of n_ranges entries.  out_off: HOST array of n_ranges + 1 entries, written.  range_status:
 * HOST array of n_ranges entries, written, may be NULL.  (Offset tables are always host arrays in this ABI.)  n_members,
 * n_decoded, bad_member and err_off may each be NULL.  in / out: host, or device under FLATE_HIP_DEVICE_PTRS.
 *
 * Positions.  FLATE_HIP_BGZF_POS_BYTES: range r is U[min(begin[r], T), min(end[r], T)) -- it reads short at the end of
 * the file, as pread does.  FLATE_HIP_BGZF_POS_VIRTUAL: v = (c << 16) | u is VALID iff c == member_off[k] for some k in
 * [0, n] (k == n: c == in_len, the end of the file; a c that merely passes the member rule, such as a decoy inside a
 * stored block, is not valid) and u <= ISIZE[k], with only u == 0 allowed for k == n.  Its position is p(v) =
 * out_off_m[k] + u, and range r is U[p(begin[r]), p(end[r])).  A range with an invalid end point is decided on the
 * device: range_status[r] = FLATE_HIP_E_INVALID, and it delivers zero bytes.
 *
 * Touched members.  Member k is touched iff ISIZE[k] > 0 and [out_off_m[k], out_off_m[k + 1]) intersects some valid,
 * non-empty range.  Every touched member is decoded once per call, whole, and verified exactly as
 * flate_hip_inflate_batch_framed(FLATE_HIP_WRAP_GZIP) verifies it: header, raw stream up to the trailer, CRC-32, ISIZE.
 * Untouched members are neither decoded nor verified.  The CHAIN is always validated whole: discovery runs as in
 * flate_hip_bgzf_read.  *n_members = n, *n_decoded = the number of touched members.
 *
 * Output.  out[out_off[r], out_off[r + 1]) = the bytes of range r: the ranges lie back to back in the order given,
 * out_off[0] = 0, out_off[n_ranges] = the total.  Ranges may overlap, repeat, be empty and come in any order.  Bytes
 * that come from a member whose status is non-zero are unspecified; everything else is exact.  Device pointers: nothing
 * outside out[0, out_off[n_ranges]) is written.  Host pointers: that range is copied back once, nothing behind it is
 * written.
 *
 * Verdict, in this order.
 *  1. FLATE_HIP_E_INVALID before any HIP call: NULL ctx / in (with in_len > 0) / begin / end / out_off (with n_ranges >
 *     0); out == NULL with out_cap > 0; an unknown pos_kind; flags other than FLATE_HIP_DEVICE_PTRS; begin[r] > end[r]
 *     numerically for any r, in either kind (for valid virtual offsets numeric order is position order).
 *  2. n_ranges == 0: out_off[0] = 0 if out_off is given, FLATE_HIP_OK, nothing is read.
 *  3. A malformed chain: the return value and *err_off are flate_hip_bgzf_index's, *bad_member = the count of good
 *     members, every out_off entry is 0, every range_status[r] = FLATE_HIP_E_CORRUPT; nothing is decoded or written.
 *  4. A total above out_cap: FLATE_HIP_E_OUT_TOO_SMALL; out_off is fully written (out_off[n_ranges] = the size needed),
 *     nothing is decoded or written.  out == NULL with out_cap == 0 is the size query -- unless the total is 0, which
 *     is FLATE_HIP_OK.
 *  5. Otherwise everything is decoded and delivered.  range_status[r] = FLATE_HIP_E_INVALID as above, else the first
 *     non-zero status among the members r touches in file order, else 0.  The return value is the first non-zero status
 *     among the decoded members in file order, with *bad_member = its index in the file and *err_off = its file offset;
 *     otherwise FLATE_HIP_E_INVALID if any range was invalid, else FLATE_HIP_OK with *bad_member = 0xffffffff and
 *     *err_off = -1.
 * in_len == 0: zero members, T = 0; every byte range is empty, virtual offset 0 is the only valid one.
 *
 * Host pointers: the file is uploaded once -- index, selection and decode share the staged copy, as in
 * flate_hip_bgzf_read -- and the delivered bytes come down once.  A caller with many queries keeps the file on the
 * device and uses FLATE_HIP_DEVICE_PTRS.
 *   How (bgzf_range_kernels.hip), all on the ctx's stream behind discovery, no host pass over file bytes: LOCATE, one
 *   thread per range (the rule is bgzf_range_rule.h: byte positions clamped, virtual offsets found in member_off by
 *   binary search); SELECT, +1 / -1 per range into a difference array over the members, a scan, the mask ISIZE > 0, one
 *   scan for rank and scratch offset, compaction in file order -- no walk over a range's span; ONE read-back of the
 *   selected members' index and the ranges' layout (the synchronisation flate_hip_bgzf_read has between index and
 *   decode); DECODE of the selected members, which are not consecutive in the file, through the framed gzip read into a
 *   dense scratch; GATHER of every range's one contiguous run of that scratch into out: pieces of at most 64 KiB,
 *   16-byte stores on the destination's grid with the source realigned in registers, heads and tails byte-exact.
 *   Locate, select and gather are counted in no profiling stage; FLATE_HIP_STAGE_INFLATE / _CHECKSUM mean what they
 *   mean in flate_hip_bgzf_read.  A failed scratch allocation is FLATE_HIP_E_HIP, never a truncated result.
 *   Out of scope: a caller-supplied index; uploading only the touched members from host memory; caching the index
 *   across calls; decoding straight into out for whole-member spans. */
#define FLATE_HIP_BGZF_POS_BYTES   0u  /* begin/end: positions in the file's uncompressed bytes       */
#define FLATE_HIP_BGZF_POS_VIRTUAL 1u  /* begin/end: BGZF virtual offsets, coffset << 16 | uoffset     */
int flate_hip_bgzf_read_ranges(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint32_t pos_kind,
                               const uint64_t *begin, const uint64_t *end, uint32_t n_ranges,
                               uint8_t *out, uint64_t out_cap, uint64_t *out_off, int32_t *range_status,
                               uint32_t *n_members, uint32_t *n_decoded, uint32_t *bad_member,
                               int64_t *err_off, uint32_t flags);

/* -- BGZF files in PARTS: read and written through bounded buffers ---------------------
 * BAM, bgzipped VCF and tabix-indexed tables run to hundreds of gigabytes; these handles stream one through two fixed
 * buffers.  A handle is a few host words: nothing of it lives on the device or in the ctx's scratch, so any other call
 * on the ctx may run between two calls of a handle.  `flags` is fixed at open.
 *
 * flate_hip_bgzf_reader_read -- one call is flate_hip_bgzf_read on the part in[0, in_len); the conventions are
 * flate_hip_gzfile_reader_read's.  `in` begins with the bytes the last call left unused (*in_used says how many were
 * used); final_in != 0: the file ends with this part.  flags: a subset of FLATE_HIP_DEVICE_PTRS.
 *   THE CONTRACT.  Let F be the concatenation of everything consumed.  The serial walk of flate_hip_bgzf_index over F
 *     defines the members.  The concatenation of every call's out[0, *out_len) is the output of F's members IN FRONT OF
 *     THE FIRST FAILURE in file order, for every cut and every out_cap.  A failure is a position where no member can
 *     stand, or a member that does not decode or verify (status per member as flate_hip_inflate_batch_framed defines
 *     it).  The call that reaches the failure delivers the good members in front of it, returns the error, sets
 *     *bad_member to the member's number counted over the FILE and *err_off to its FILE offset (or to the offset where
 *     no member could be read), and *in_used = 0.  THE ONE DIFFERENCE from flate_hip_bgzf_read: the whole call delivers
 *     nothing for a broken chain and everything around a bad member; only "everything in front" can be the same for
 *     every cut.  On success the *in_used of all calls sum to F's length.
 *   The part's end.  A member that the part cuts is left unused: *in_used stops in front of it.  Where the walk finds
 *     no member at offset p of the part: p == in_len is a boundary; on a final part, or with in_len - p >=
 *     FLATE_HIP_BGZF_MEMBER_MAX (a member is at most that long: no continuation can put one there), it is
 *     FLATE_HIP_E_CORRUPT at p; else nothing is wrong yet and the next part begins at p.  No finer test of a cut header
 *     is made: every cut gives the same bytes and the same final verdict, a malformed file is only reported one call
 *     later.  THE PROGRESS RULE: a part of at least 65536 bytes, or a final one, always makes progress or gives a
 *     verdict (given room for its first member).
 *   Delivery.  Of the whole members of the part a call delivers the longest prefix whose output fits out_cap (the sums
 *     of ISIZE) and whose index fits index_cap; empty members are delivered as far as they go.  *n_members = that
 *     count.  If not even the first fits: FLATE_HIP_E_OUT_TOO_SMALL with *out_len = its ISIZE and *in_used = 0 --
 *     repeatable, nothing changes.  Nothing outside out[0, *out_len of a clean call) is written, with device pointers
 *     too, and that is at most out_cap.
 *   Returns FLATE_HIP_OK: call again.  FLATE_HIP_STREAM_END: a final call that delivered every member up to in_len
 *     (an empty file -- a final call without bytes on a fresh handle -- included); sticky.  The file's error: sticky,
 *     every later call returns it with the same words, *in_used = 0 and *out_len = 0.  Repeatable and changing
 *     nothing: FLATE_HIP_E_INVALID (a NULL handle or pointer, one index array without the other, index_cap == 0 with
 *     arrays; decided before any HIP call), FLATE_HIP_E_OUT_TOO_SMALL as above, FLATE_HIP_E_HIP.  The repeatable codes
 *     leave *bad_member = 0xffffffff: a sticky FLATE_HIP_E_OUT_TOO_SMALL (a member produced more than its ISIZE)
 *     names the member.  *eof_marker = 1 if the last member delivered so far is the canonical 28 bytes.
 *   The file's index while streaming.  member_off and out_off: both NULL, or HOST arrays of index_cap entries.  A call
 *     that delivers k members writes k + 1 entries in FILE coordinates -- compressed and uncompressed offsets, what a
 *     .gzi holds and the halves of a virtual offset; the last entry of one call equals the first of the next (a call
 *     that delivers nothing, a sticky one included, writes the one entry where the file stands).
 *     index_cap < k + 1 clips the delivery to index_cap - 1 members, exactly as out_cap does.
 *   Out of scope: ranges in parts; overlapping the upload of part k + 1 with the work on part k; a .gzi or .bai
 *     writer (the arrays are there, the file formats are not); the MoonBit binding. */
typedef struct flate_hip_bgzf_reader flate_hip_bgzf_reader;
int flate_hip_bgzf_reader_open(flate_hip_ctx *ctx, uint32_t flags, flate_hip_bgzf_reader **reader);
int flate_hip_bgzf_reader_read(flate_hip_bgzf_reader *reader, const uint8_t *in, uint64_t in_len, int final_in,
                               uint8_t *out, uint64_t out_cap, uint64_t *in_used, uint64_t *out_len,
                               uint64_t index_cap, uint64_t *member_off, uint64_t *out_off, uint32_t *n_members,
                               uint32_t *bad_member, int64_t *err_off, int *eof_marker);
int flate_hip_bgzf_reader_reset(flate_hip_bgzf_reader *reader);
void flate_hip_bgzf_reader_free(flate_hip_bgzf_reader *reader);

/* flate_hip_bgzf_writer_write -- the conventions are flate_hip_one_writer_write's; block_bytes and flags are
 * flate_hip_bgzf_write's.  A call that is not final consumes the k = in_len / block_bytes whole blocks its part holds
 * (*in_used = k * block_bytes; with in_len < block_bytes: FLATE_HIP_OK, nothing written, nothing launched) and writes
 * NO marker.  A final call consumes everything and ends with the 28-byte marker; without bytes it writes the marker
 * alone.  It returns FLATE_HIP_STREAM_END; after that every write is FLATE_HIP_E_INVALID until reset.  *n_blocks = the
 * members written (the marker not counted; may be NULL).
 *   THE FILE: the concatenation of every call's out[0, *out_len) is, byte for byte, what flate_hip_bgzf_write writes
 *     for the whole input with the same block_bytes and flags, for ANY cut: the blocks are independent.
 *   member_off: NULL, or a HOST array with room for in_len / block_bytes + 2 entries: the members' FILE offsets and
 *     where the next member, or the marker, starts.
 *   Room: flate_hip_bgzf_writer_bound(in_len, block_bytes) always holds a call's output.  Too little:
 *     FLATE_HIP_E_OUT_TOO_SMALL; a block that 65536 bytes cannot express: FLATE_HIP_E_TOO_LARGE, as in the whole call.
 *     Both, FLATE_HIP_E_INVALID and FLATE_HIP_E_HIP are repeatable and leave the handle unchanged.
 *   Out of scope: overlapping the upload of part k + 1 with the work on part k; a .gzi or .bai writer; the MoonBit
 *     binding. */
typedef struct flate_hip_bgzf_writer flate_hip_bgzf_writer;
size_t flate_hip_bgzf_writer_bound(uint64_t in_len, uint32_t block_bytes);
int flate_hip_bgzf_writer_open(flate_hip_ctx *ctx, uint32_t block_bytes, uint32_t flags, flate_hip_bgzf_writer **writer);
int flate_hip_bgzf_writer_write(flate_hip_bgzf_writer *writer, const uint8_t *in, uint64_t in_len, int final_in,
                                uint8_t *out, uint64_t out_cap, uint64_t *in_used, uint64_t *out_len,
                                uint64_t *member_off, uint32_t *n_blocks);
int flate_hip_bgzf_writer_reset(flate_hip_bgzf_writer *writer);
void flate_hip_bgzf_writer_free(flate_hip_bgzf_writer *writer);

/* -- Plain multi-member gzip files: indexed and read in one call each -----------------
 * The gzip files people have -- `cat a.gz b.gz`, rotated logs, Hadoop part files, WARC / WET records, the concatenated
 * members flate_hip_deflate_fast_batch_framed(FLATE_HIP_WRAP_GZIP) writes -- carry no index: member k + 1 starts where
 * member k's DEFLATE stream ends, plus 8 bytes, and nothing in a header says where that is.  These two calls find the
 * members on the device, from the file's bytes alone.  The rule and the walk are written once, csrc/gzip_rule.h; the
 * kernels are csrc/gzip_kernels.hip.
 *
 * THE RULE.  A member can start at offset p iff in[p, E), E = min(in_len, p + M), begins with a gzip header as
 * flate_hip_inflate_batch_framed accepts it: 1f 8b 08; FLG with the reserved bits zero; the 10 fixed bytes; FEXTRA,
 * FNAME, FCOMMENT, FHCRC skipped in that order, every NUL below E; and 8 bytes left for the trailer.  M is the option
 * "gzip_member_max" (flate_hip_set_option): 2^28 - 1 by default, which is also the most -- the bit positions of the
 * decoder are 32 bits wide -- so it can only be lowered.  Every such p is a CANDIDATE.  Its raw stream is decoded
 * size-only over in[p + header, E - 8): status s, the size z it inflates to, and `used`, the bytes up to and including
 * the one that holds the last bit of the final block.  s == 0: the member is in[p, e), e = p + header + used + 8.
 *
 * THE WALK that defines every result starts at p = 0.  p == in_len: success (in_len == 0: zero members).  No header at
 * p: FLATE_HIP_E_CORRUPT, *err_off = p.  s != 0: the walk ends with *err_off = p and s -- FLATE_HIP_E_CORRUPT,
 * FLATE_HIP_E_UNEXPECTED_EOF, or FLATE_HIP_E_TOO_LARGE for a member that inflates to 4 GiB or more -- except that
 * FLATE_HIP_E_UNEXPECTED_EOF in a range that M clipped (p + M < in_len) is FLATE_HIP_E_TOO_LARGE: such a member is read
 * with flate_hip_inflate_one, which decodes a single long member in parallel, or in pieces with
 * flate_hip_inflate_stream_read.
 * Otherwise p = e.  The file must end exactly where a member ends: padding or
 * garbage behind the last member, zero bytes included, is FLATE_HIP_E_CORRUPT at its offset.
 *
 * flate_hip_gzip_index has flate_hip_bgzf_index's conventions.  On success member_off[0 .. n] (member_off[n] = in_len)
 * and out_off[0 .. n] (the exclusive prefix sum of what the members ACTUALLY inflate to, never of ISIZE: a wrong ISIZE
 * is that member's failure at read time, not a misplaced slot) are exactly what
 * flate_hip_inflate_batch_framed(FLATE_HIP_WRAP_GZIP) takes as in_off and out_off; *out_bytes = out_off[n]; *err_off =
 * -1.  Both arrays are HOST arrays of index_cap entries, or both NULL: a query that returns only the counts.
 * index_cap < n + 1: FLATE_HIP_E_OUT_TOO_SMALL with the counts set.  A broken chain: the return value and *err_off are
 * the walk's, *n_members = the good members in front, *out_bytes = 0, and the first n_members + 1 entries of both arrays
 * are still filled if they fit -- a caller can salvage the good prefix through the framed batch call.  *n_candidates
 * (may be NULL, as may err_off): how many offsets were decoded speculatively.  flags: FLATE_HIP_DEVICE_PTRS or 0,
 * anything else is FLATE_HIP_E_INVALID before any HIP call.  More candidates than 32 bits count: FLATE_HIP_E_TOO_LARGE.
 * Nothing outside in[0, in_len) is read, at any alignment of in.
 *   How: every offset that passes the rule is a candidate (one pass with 16-byte loads, the 3-byte magic and the FLG
 *   mask tested in LDS, the rule run from global memory on the rare hit, compacted in file order); the count comes
 *   back to the host; ONE size-only launch of the batch decoders runs over all candidates -- it stores nothing, so a
 *   decoy can write nothing --; every candidate finds the candidate at its end by binary search; the chain from offset
 *   0 is ranked by pointer doubling.  A decoy (a gzip member inside a stored block, a header inside a file name) is a
 *   candidate like any other, gets a successor like any other, and is simply not on the path from candidate 0.  The
 *   discovery kernels are counted in no profiling stage.
 *   The work: the sum, over the candidates, of the bytes each consumes before its stream ends or fails, each at most M
 *   -- the members themselves once, plus the decoys; and every false hit's header rule, a NUL scan of at most M bytes.
 *   1f 8b 08 and three zero FLG bits have probability 2^-27 per offset of random bytes, about eight per GiB (arithmetic,
 *   not a measurement), and a garbage stream dies within a few blocks.  Both are properties of the method: a file
 *   built to hold many long decoys costs their sum, and no further guard exists.
 *
 * flate_hip_gzip_read: the discovery, then flate_hip_bgzf_read's tail -- one read-back of the index, the framed gzip
 * decode of every member into the dense slots out_off, CRC-32 and ISIZE judged on the device.  Host pointers: the file
 * is uploaded once, shared by discovery and decode, and out[0, *out_len) is downloaded once.
 *   A broken chain: the walk's code and *err_off, *bad_member = the count of good members, *out_len = 0, nothing is
 *   written.  A total above out_cap: FLATE_HIP_E_OUT_TOO_SMALL, *out_len = the size needed, nothing is decoded (out ==
 *   NULL with out_cap == 0 is the size query).  Otherwise every member is decoded, *out_len = out_off[n], and the return
 *   value is the first non-zero member status as flate_hip_inflate_batch_framed defines it, with *bad_member = its index
 *   and *err_off = its file offset; on success 0xffffffff and -1.  n_members, bad_member and err_off may each be NULL.
 *   The slot-write guarantees of flate_hip_inflate_batch hold.  With profiling on, FLATE_HIP_STAGE_INFLATE and
 *   FLATE_HIP_STAGE_CHECKSUM are the decode pass's, as in flate_hip_bgzf_read: the size-only pass of the discovery is in
 *   neither.
 *   Out of scope: zero or garbage padding behind the last member; members of M bytes or more (flate_hip_gzfile_read
 *   reads them); running a clipped
 *   candidate again unclipped; caching the index across calls; salvage inside flate_hip_gzip_read; zlib or raw
 *   concatenations. */
int flate_hip_gzip_index(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint64_t index_cap,
                         uint64_t *member_off, uint64_t *out_off, uint32_t *n_members, uint64_t *out_bytes,
                         uint32_t *n_candidates, int64_t *err_off, uint32_t flags);
int flate_hip_gzip_read(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap,
                        uint64_t *out_len, uint32_t *n_members, uint32_t *bad_member, int64_t *err_off,
                        uint32_t flags);

/* -- One long stream: its block starts found on the device ----------------------------
 * The most common compressed file there is carries nothing that cuts it into independent pieces: ONE .gz, zlib or raw
 * DEFLATE stream as gzip, zlib or pigz write it -- one member, many blocks.  flate_hip_inflate_one_index finds where
 * its dynamic-Huffman blocks start, at bit granularity, from the stream's bits alone.  The rule is written once,
 * csrc/deflate_block_rule.h; the kernels are csrc/one_kernels.hip and csrc/one_probe_kernel.inc.
 *
 * The input is ONE stream: wrap = FLATE_HIP_WRAP_RAW, _ZLIB or _GZIP, with exactly the header rules of
 * flate_hip_inflate_spliced_framed (FEXTRA, FNAME, FCOMMENT and FHCRC skipped; zlib's FDICT, or a member too short for
 * header plus trailer, is a bad header: *status = FLATE_HIP_E_CORRUPT, *err_off = 0, no units).  Bits and offsets below
 * are counted from the RAW stream's first byte.
 *
 * UNITS.  A unit starts at bit 0 and at every dynamic block header (BTYPE = 2) the serial decode reaches; stored and
 * fixed blocks belong to the unit in front of them, so a stream made only of them is one unit.  With the option
 * "one_stored_units" at 1 UNITS reads: bit 0, every dynamic header and every STORED header (BTYPE = 0) that the serial
 * decode reaches; only fixed blocks then belong to the unit in front of them, a stream of stored blocks of any total
 * length is accepted (the limit below is per unit), and a unit of zero output bytes -- an empty stored block of
 * Z_SYNC_FLUSH, Z_FULL_FLUSH or pigz -- is a unit like any other.  A stored header is found by its LEN / NLEN pair
 * (csrc/deflate_block_rule.h: BTYPE = 0, the padding bits unread, four bytes inside the stream, LEN == ~NLEN), so up to
 * 8 bit offsets in front of one aligned pair are candidates, at most one of them on the path.  On success
 * unit_bit[0 .. n] (unit_bit[n] = the bit behind the final block) and out_off[0 .. n] (the exclusive prefix sum of what
 * the units inflate to) describe the stream; *out_bytes = out_off[n]; *status = 0; *err_off = -1.
 *
 * THE VERDICT is the serial decoder's, as far as it does not depend on history: the bits a DEFLATE stream consumes never
 * depend on the bytes it has produced, so *status and *err_off equal what flate_hip_inflate_batch reports for the raw
 * stream -- FLATE_HIP_E_CORRUPT with its offset, FLATE_HIP_E_UNEXPECTED_EOF with -1 -- except for a distance that reaches
 * in front of the stream and for the container's trailer, which only a decode can judge: neither is looked at here.  A
 * unit whose input spans 2^28 bytes or more (option "one_unit_max", which can only be lowered) is FLATE_HIP_E_TOO_LARGE:
 * the decoders count positions inside one unit in 32 bits; such a stream is read with flate_hip_inflate_stream_read.
 * Exactly: a unit is too large iff its reader, counting from the byte that holds the unit's first bit, takes more than
 * that many bytes before the unit ends (the three bits of the next block header included).  A
 * stream that fails: *n_units = the good units in front of the failing one, *out_bytes = 0, and the first n_units + 1
 * entries of both arrays are still filled if they fit (unit_bit[n_units]: where the failing unit starts).
 *
 * Conventions: flate_hip_gzip_index's.  Both arrays are HOST arrays of index_cap entries, or both NULL: a query that
 * returns only the counts.  index_cap < n + 1: FLATE_HIP_E_OUT_TOO_SMALL with the counts set.  The return value is
 * *status when that is not 0.  *n_candidates (may be NULL, as may err_off): how many bit offsets were decoded
 * speculatively, bit 0 included.  flags: FLATE_HIP_DEVICE_PTRS or 0, anything else -- or a wrap above _GZIP -- is
 * FLATE_HIP_E_INVALID before any HIP call.  in_len == 0: a bad header for zlib and gzip, FLATE_HIP_E_UNEXPECTED_EOF for
 * raw.  More candidates than 32 bits count: FLATE_HIP_E_TOO_LARGE.  Nothing outside in[0, in_len) is read, at any
 * alignment of in; nothing is written to device memory the caller owns.
 *   How, all on the ctx's stream, no host pass over stream bytes: FIND, one thread per BIT offset of the raw stream
 *   tests the rule -- exactly what the decoder's header reader accepts: BTYPE = 2 with either BFINAL, at most 286
 *   literal/length and 30 distance codes, a code-length code the decoder takes, every repeat inside the counts, both
 *   codes taken, all inside the raw stream; nothing stricter, or a true header would be missed -- the counts and the
 *   code-length code first, in LDS; hits are compacted in bit order and the count comes back to the host.  PROBE, one
 *   wavefront per candidate, decodes from the candidate's bit without history, window or stores -- a decoy can write
 *   nothing -- up to the next header with BTYPE = 2 or through the final block: end bit, bytes produced, status.  LINK /
 *   RANK / SCAN as for gzip members: every candidate finds the candidate at its end bit by binary search, the chain
 *   from bit 0 is ranked by pointer doubling, a scan of the sizes gives out_off.  A chain that stops at a header with
 *   BTYPE = 2 that is no candidate takes its verdict from one more probe at that bit.  A decoy (a stream inside a
 *   stored block, compressed bits that look like a header) is a candidate like any other and is simply not on the path
 *   from bit 0.  Counted in no profiling stage.
 *
 * flate_hip_inflate_one: the discovery, then the units DECODED IN PARALLEL.  in / out are host buffers, or device buffers
 * under FLATE_HIP_DEVICE_PTRS (any other flag: FLATE_HIP_E_INVALID before any HIP call), at any alignment.  *status,
 * *err_off and *out_len are what the serial decoder reports for the same bytes as one stream
 * (flate_hip_inflate_batch_framed; flate_hip_inflate_batch for a raw stream): err_off counted from the raw stream's
 * first byte, the bytes in front of an error delivered, a distance that reaches in front of the stream
 * FLATE_HIP_E_CORRUPT at the serial offset, a trailer mismatch (CRC-32 or ISIZE, Adler-32) FLATE_HIP_E_CORRUPT with
 * err_off = in_len.  The return value is *status when that is not 0.  The total is known after discovery: above out_cap
 * it is FLATE_HIP_E_OUT_TOO_SMALL with *out_len = the size needed and nothing decoded (out == NULL with out_cap == 0 is
 * the size query); with device pointers nothing outside out[0, total) is written.  Host pointers: the stream is
 * uploaded once, shared by discovery and decode, and out[0, *out_len) is downloaded once.  err_off, n_units and
 * n_candidates may be NULL.
 *   How: in rounds of at most "one_round_units" units (flate_hip_set_option; 4096 by default, 160 KiB of scratch per
 *   unit: two buffers of tail functions and the windows).  TAIL: the probe's decoder with a SYMBOLIC 32 KiB window in
 *   LDS (16-bit entries: a literal byte, or "byte j of the 32 KiB in front of this unit"; csrc/window_compose.h), one
 *   wavefront per unit; copies move entries as they move bytes, and only the unit's final window is stored: its tail
 *   function, with the shifted pass-through of a unit shorter than 32 KiB.  COMPOSE: the functions are scanned over the
 *   round in ceil(log2(units)) dependent launches and resolved against the last window of the round in front (nothing
 *   for round 0: entries in front of the stream resolve to 0, and no valid stream reads them).  DECODE: the round's
 *   units go through the lane-per-stream dictionary decoder as spliced pieces with dictionaries: piece k starts at the
 *   unit's bit and ends where the next unit starts, its dictionary is its resolved history, dict_len = min(32768,
 *   out_off[k]), and its output slot is out + out_off[k] with exactly the unit's size.
 *   TAIL and DECODE apply the distance rule with the history the unit really has, min(32768, out_off[k] + bytes
 *   produced), so the one history-dependent verdict comes out where the serial decoder has it; the first failing unit's
 *   slot ends at its failure and the units behind it get an empty one: nothing behind an error is written.  VERIFY:
 *   the checksum kernels over out[0, total) in 64 KiB pieces and a verdict kernel.  No kernel waits for another
 *   workgroup.  Profiling: FLATE_HIP_STAGE_INFLATE is DECODE (of several rounds the last),
 *   FLATE_HIP_STAGE_CHECKSUM is VERIFY; FIND, PROBE, LINK, TAIL and COMPOSE are counted in no stage.
 *   Out of scope: finding fixed block starts (a fixed block has no header beyond its three bits, so there is nothing
 *   to test: runs of them stay serial inside one unit; stored block starts: option "one_stored_units"); fusing
 *   PROBE with TAIL; routing long members of flate_hip_gzip_read here; multi-member input (flate_hip_gzfile_read);
 *   caching the index across calls (the seek index below is what a caller keeps). */
int flate_hip_inflate_one(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint32_t wrap, uint8_t *out,
                          uint64_t out_cap, uint64_t *out_len, int32_t *status, int64_t *err_off, uint32_t *n_units,
                          uint32_t *n_candidates, uint32_t flags);
int flate_hip_inflate_one_index(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint32_t wrap,
                                uint64_t index_cap, uint64_t *unit_bit, uint64_t *out_off, uint32_t *n_units,
                                uint64_t *out_bytes, uint32_t *n_candidates, int32_t *status, int64_t *err_off,
                                uint32_t flags);

/* -- One long stream read in PARTS: flate_hip_inflate_one through bounded buffers ------
 * For a caller that holds a long raw, zlib or gzip stream a piece at a time (a Reader over a multi-gigabyte .gz): the
 * conventions of flate_hip_inflate_stream_read, the speed of flate_hip_inflate_one.  One call IS flate_hip_inflate_one
 * on the part in[0, in_len) of the stream, started where the last call stopped; between calls the handle keeps the bit
 * where the next unit starts, the 32 KiB window in front of it (on the device) and the running checksum (on the device).
 *
 * open: wrap is FLATE_HIP_WRAP_RAW / _ZLIB / _GZIP with flate_hip_inflate_one's header rules; flags is 0 or
 * FLATE_HIP_DEVICE_PTRS (in and out of every read are device buffers), fixed for the handle's life; anything else, or a
 * NULL ctx or result pointer, is FLATE_HIP_E_INVALID before any HIP call.  The handle records the unit rule (option
 * "one_stored_units") and "one_unit_max" as the ctx has them at open and uses them whatever the ctx says later, as a
 * seek index does.  reset: a fresh stream on the same handle, same wrap, flags and options.  The ctx must outlive it.
 *
 * read: in[0, in_len) BEGINS with the bytes the last call left unused (*in_used < in_len: move them to the front and
 * append); final_in != 0: no bytes follow.  Returns FLATE_HIP_OK (call again), FLATE_HIP_STREAM_END (the final block
 * decoded and the trailer judged, reported with the last bytes; sticky) or a negative status, which is sticky -- every
 * later call returns it with the same *err_off -- except FLATE_HIP_E_OUT_TOO_SMALL, FLATE_HIP_E_INVALID (NULL reader /
 * in with in_len > 0 / out with out_cap > 0 / in_used / out_len, before any HIP call) and a failure of the runtime or of
 * an allocation (FLATE_HIP_E_HIP) in front of the point where the call begins to move the handle's device words: such a
 * call has changed nothing and may be repeated.  Behind that point -- the part's checksum, the join, the result words,
 * the window's carry, the download -- FLATE_HIP_E_HIP and FLATE_HIP_E_INTERNAL end the handle (sticky), because running
 * sum or window may be ahead of the host's state; reset makes it usable again.  err_off and n_units may be NULL.
 *   ONE CALL.  Discovery runs over the part with the chain's root at the carried bit b0 (0..7) of the part's first raw
 *   byte: that bit is candidate 0, the bits in front of it in that byte are none.  Every unit whose end lies inside the
 *   part -- the next unit's header, or the final block -- is COMPLETE.  The unit that the part's end cuts is not: on a
 *   part that is not final it is left for the next call; on a final part it is judged as the whole call judges it,
 *   FLATE_HIP_E_UNEXPECTED_EOF with the bytes in front delivered.  FLATE_HIP_E_CORRUPT inside a part is the stream's
 *   verdict (the bits read are true stream bits) and comes with the bytes in front of it, as in the whole call.  The
 *   call delivers the longest prefix of complete units whose bytes fit out_cap (with the part's verdict behind them, if
 *   everything in front of it fits), decoded in rounds through the unchanged TAIL / COMPOSE / RESOLVE / DECODE with the
 *   handle's window as R[0] of the first round (zeros on the first part); the window behind the last delivered unit
 *   goes back into the handle.  *in_used = the byte that holds the first bit of the first undelivered unit, whose place
 *   in that byte becomes b0; *out_len = the bytes delivered; *n_units = the complete units delivered.  Units that did not
 *   fit, and the cut unit, are simply discovered again by the next call.
 *     At least one complete unit and not even the first fits: FLATE_HIP_E_OUT_TOO_SMALL with *out_len = the first
 *     unit's size, the state unchanged.  No complete unit on a part that is not final: FLATE_HIP_OK with *in_used =
 *     *out_len = 0, the caller appends more; the same with in_len >= "one_unit_max", or a unit beyond it, is
 *     FLATE_HIP_E_TOO_LARGE.  A RUN OF FIXED BLOCKS -- or of stored blocks with "one_stored_units" at 0 -- IS ONE UNIT:
 *     it needs a part that holds it whole (and the three bits of the header behind it).
 *   HISTORY.  The distance rule uses what the STREAM has produced, not the part: TAIL and DECODE see min(32768,
 *   produced before the part + out_off[k] + bytes produced), so a distance that reaches in front of the stream in a
 *   later part of a stream that has produced less than 32 KiB fails at the serial offset.
 *   OFFSETS.  *err_off counts from the raw stream's first byte over all parts; a trailer that does not match reports
 *   the member's length in bytes, as the whole call reports in_len.
 *   CONTAINER.  The header is read on the first part; a header that is refused only because the part ends inside it is
 *   FLATE_HIP_OK with nothing used on a part that is not final (csrc/one_parts_rule.h: the rule's third answer), and a
 *   bad header on a final one.  On a final part the trailer's bytes are cut off the raw range as in the whole call; on
 *   any other part the raw range runs to the part's end.  When the final block lies in a part but the 4 or 8 trailer
 *   bytes do not lie in it whole, the call delivers the bytes, *in_used points behind the final block rounded up to a
 *   byte, it returns FLATE_HIP_OK, and the next call judges the trailer once it has the bytes (final_in with too few:
 *   FLATE_HIP_E_UNEXPECTED_EOF).  The checksum of each part's delivered bytes is computed by the checksum kernels and
 *   joined to the running sum on the device (as two pieces, of the bytes produced before and of *out_len); the verdict
 *   kernel compares the joined sum, and for gzip the total length mod 2^32, with the trailer.  Bytes behind the trailer
 *   are not looked at: *in_used stops behind it.
 *   Host pointers: the part is uploaded once and out[0, *out_len) downloaded once per call.  With device pointers
 *   nothing outside out[0, *out_len) is written.  Per call the host waits for the discovery's two read-backs and one
 *   read-back of the result words.
 *   Out of scope: a file of several members read in parts (that is flate_hip_gzfile_reader_*, below); overlapping
 *   the copy of part k + 1 with the decode of part k.  (The parallel writer in parts: flate_hip_one_writer_*.) */
typedef struct flate_hip_one_reader flate_hip_one_reader;
int flate_hip_one_reader_open(flate_hip_ctx *ctx, uint32_t wrap, uint32_t flags, flate_hip_one_reader **reader);
int flate_hip_one_reader_read(flate_hip_one_reader *reader, const uint8_t *in, uint64_t in_len, int final_in,
                              uint8_t *out, uint64_t out_cap, uint64_t *in_used, uint64_t *out_len, int64_t *err_off,
                              uint32_t *n_units);
int flate_hip_one_reader_reset(flate_hip_one_reader *reader);
void flate_hip_one_reader_free(flate_hip_one_reader *reader);

/* -- Seek index for one long stream: build once, read ranges --------------------------
 * flate_hip_inflate_one pays the whole discovery on every call.  A SEEK INDEX keeps it: flate_hip_inflate_one_seek_index
 * builds one, flate_hip_inflate_one_ranges reads byte ranges of the stream's output through it and decodes only the
 * units they need.  The rule and the layout are written once, csrc/seek_index_rule.h; the kernels are
 * csrc/one_seek_kernels.hip.
 *
 * Notation: n, unit_bit[0 .. n] and out_off[0 .. n] are exactly what flate_hip_inflate_one_index defines; T =
 * out_off[n]; U[0, T) is what the stream inflates to.
 *
 * THE POINT RULE.  Unit k is a POINT iff k == 0 or out_off[k] / span > out_off[k - 1] / span (integer division).  span
 * >= 1; span == 0 means FLATE_HIP_SEEK_SPAN_DEFAULT; FLATE_HIP_SEEK_SPAN_NONE leaves unit 0 as the only point: the
 * index then holds no window at all and is simply the cached discovery; span == 1 makes every unit that produces output
 * behind a non-empty predecessor a point.  pstart(k) is the last point at or in front of k; a SEGMENT is a point and the
 * units behind it up to the next point.
 *
 * TWO BUFFERS.  index: a HOST array of 64-bit words (offset tables are always host arrays in this ABI):
 *   word 0 the magic "FONESIDX" (little endian), 1 the version (1), 2 wrap, 3 in_len, 4 the raw stream's first byte, 5
 *   the byte behind it, 6 T, 7 span, 8 n, 9 n_points, 10 / 11 the container's trailer words as the device parses them
 *   (the checksum as a number and ISIZE; 0 for raw), 12 the unit rule the index was built with (0: dynamic headers
 *   start units; 1: dynamic and stored headers, option "one_stored_units" -- flate_hip_inflate_one_ranges walks the units
 *   by THIS word and ignores its ctx's option; any other value: FLATE_HIP_E_INVALID), 13 .. 15 zero;
 *   then unit_bit[n + 1], out_off[n + 1], point_unit[n_points] (rising, point_unit[0] = 0):
 *   16 + 2 (n + 1) + n_points words.
 * windows: host, or device under FLATE_HIP_DEVICE_PTRS like in, at any byte alignment: n_points - 1 blocks of 32768
 * bytes; block p - 1 is the 32 KiB of output in front of unit point_unit[p], in stream order, bytes in front of the
 * stream 0.  Point 0 needs no window.  The windows are neither compressed nor checksummed.
 *
 * flate_hip_inflate_one_seek_index: BUILD.  Conventions are flate_hip_inflate_one's: the wrap rules, flags
 * FLATE_HIP_DEVICE_PTRS or 0, FLATE_HIP_E_INVALID before any HIP call (NULL ctx / in with in_len > 0 / index_words /
 * windows_bytes / n_units / n_points / out_bytes / status; index == NULL with index_cap_words > 0, windows == NULL with
 * windows_cap > 0; a wrap above _GZIP; any other flag); host pointers are uploaded once.  n_candidates and err_off may
 * be NULL.  Both sizes are known after POINTS, in front of TAIL: a too-small index_cap_words or windows_cap -- both
 * buffers NULL with capacity 0 is the size query -- returns FLATE_HIP_E_OUT_TOO_SMALL with every count set
 * (*index_words, *windows_bytes, *n_units, *n_points, *out_bytes = T) and nothing written; the query costs the
 * discovery only.
 * Verdict: *status / *err_off are flate_hip_inflate_one's for the same bytes, EXCEPT THAT THE TRAILER IS NOT JUDGED:
 * nothing is decoded to output, so there is nothing to sum.  The history-independent verdict comes from the discovery;
 * a distance that reaches in front of the stream comes from TAIL at the serial offset, which therefore runs over every
 * unit whatever the span (a size query returns in front of it and reports the discovery's verdict).  A caller who wants
 * the trailer judged calls flate_hip_inflate_one once.  A stream whose status is not 0 gets no index: *index_words =
 * *windows_bytes = 0, *n_points = 0, the return value is the status; what `windows` holds then is unspecified, nothing
 * outside windows[0, windows_cap) is ever written.
 *   How: discovery as in flate_hip_inflate_one_index; POINTS, one thread per unit, the rule from two neighbouring
 *   out_off entries, a scan and a compaction; per round of "one_round_units" TAIL and COMPOSE / RESOLVE exactly as
 *   flate_hip_inflate_one runs them; in DECODE's place PACK, the resolved window in front of every point unit of the
 *   round into its block by the gather kernel of the BGZF range call.  No kernel waits for another workgroup.
 *
 * flate_hip_inflate_one_ranges: READ.  begin, end: HOST arrays of n_ranges positions in U; range r is U[min(begin[r], T),
 * min(end[r], T)) -- it reads short at the end, as FLATE_HIP_BGZF_POS_BYTES does.  out_off (HOST, n_ranges + 1, written),
 * range_status (HOST, n_ranges, written, may be NULL), the output's layout, overlapping, repeated and empty ranges and
 * what is written where are flate_hip_bgzf_read_ranges's.  n_decoded and bad_unit may be NULL.
 * Unit k is TOUCHED iff it produces output and its output range intersects a non-empty range.  The DECODED set is the
 * union, over touched k, of [pstart(k), k]: units behind the last touched unit of a segment are not decoded.
 * *n_decoded is the size of that set.
 * Verdict, in this order.
 *  1. FLATE_HIP_E_INVALID before any HIP call: any of flate_hip_bgzf_read_ranges's argument refusals; a wrap above
 *     _GZIP; windows == NULL with windows_bytes > 0; an index that fails seek_index_ok (host, O(n)): a wrong magic or
 *     version; wrap or in_len not the call's; a word count or windows_bytes that is not what the counts imply; unit_bit
 *     not strictly increasing from 0 inside the raw stream, or a unit of more than 2^28 bytes of input; out_off not
 *     non-decreasing from 0 to T; point_unit not exactly the point rule's set for the stored span.
 *  2. n_ranges == 0: out_off[0] = 0 if out_off is given, FLATE_HIP_OK, nothing is read.
 *  3. The stream is not the one the index was built from -- the raw stream's range or the trailer words, parsed on the
 *     device, differ from the head's: FLATE_HIP_E_CORRUPT, every range_status FLATE_HIP_E_CORRUPT, every out_off 0,
 *     nothing decoded.
 *  4. A total above out_cap: FLATE_HIP_E_OUT_TOO_SMALL, out_off fully written, nothing decoded.  out == NULL with out_cap
 *     == 0 is the size query -- unless the total is 0, which is FLATE_HIP_OK.
 *  5. Decode and deliver.  A decoded unit is GOOD iff its piece ends with status 0 and produces exactly out_off[k + 1] -
 *     out_off[k] bytes; anything else means that the index does not fit the stream: the decoder's status, or
 *     FLATE_HIP_E_CORRUPT if only the size differs.  range_status[r] is the first non-zero status, in stream order,
 *     among the units [pstart(first), last] decoded for range r (first / last: its first and last touched unit), else
 *     0.  The return value is the first non-zero status among all decoded units in stream order, with *bad_unit = that
 *     unit; otherwise FLATE_HIP_OK and *bad_unit = 0xffffffff.  Bytes from units behind a bad unit of the same segment
 *     are unspecified; everything else is exact.  A wrong byte inside `windows` cannot be detected: ranges carry no
 *     checksum.
 * Host pointers: the stream is uploaded once, at most the windows of the selected points are uploaded (the host has
 * the selection after the read-back), the delivered bytes come down once.
 *   How, all on the ctx's stream, no host pass over stream bytes: LOCATE, one thread per range, binary search in
 *   out_off, +1 at pstart(first) and -1 behind last into a difference array over the units.  SELECT: its scan marks the
 *   decoded units, a second scan gives each its rank and its place in a dense scratch, compaction in stream order gives
 *   the unit list; ONE read-back of counts and layout (the synchronisation flate_hip_bgzf_read_ranges has).  Rounds of
 *   "one_round_units" over the list: TAIL through the list; a SEGMENTED scan -- every unit of the round carries the
 *   round-local place of its seed, the nearest selected point at or in front of it, or place 0 when its segment
 *   continues from the round in front; the stride-s step composes only when k - s is not in front of that seed;
 *   RESOLVE applies each unit's composed function to its seed's window: the point's stored one, copied from `windows`
 *   into the round's slots first, or the carried one -- and DECODE: the units as spliced pieces with dictionaries, each
 *   with its own end, straight into the dense scratch, every unit in a slot of exactly its size.  CHECK per unit, then
 *   GATHER: every range's one run of the scratch into out.  Locate, select and gather are counted in no profiling
 *   stage; FLATE_HIP_STAGE_INFLATE is DECODE (of several rounds the last).
 *   Out of scope: delivering the output or judging the trailer from the build call (packed windows: below);
 *   importing or exporting other tools' index formats (multi-member input: flate_hip_gzfile_seek_index below); an index
 *   cached inside the ctx; uploading
 *   only the touched part of the stream from host memory; stored and fixed block starts as units; skipping TAIL for
 *   units whose tail function nobody reads. */
#define FLATE_HIP_SEEK_SPAN_DEFAULT (1ull << 20)
#define FLATE_HIP_SEEK_SPAN_NONE 0xffffffffffffffffull
#define FLATE_HIP_SEEK_WINDOW_BYTES 32768u
int flate_hip_inflate_one_seek_index(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint32_t wrap,
                                     uint64_t span, uint64_t *index, uint64_t index_cap_words, uint64_t *index_words,
                                     uint8_t *windows, uint64_t windows_cap, uint64_t *windows_bytes, uint32_t *n_units,
                                     uint32_t *n_points, uint64_t *out_bytes, uint32_t *n_candidates, int32_t *status,
                                     int64_t *err_off, uint32_t flags);
int flate_hip_inflate_one_ranges(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint32_t wrap,
                                 const uint64_t *index, uint64_t index_words, const uint8_t *windows,
                                 uint64_t windows_bytes, const uint64_t *begin, const uint64_t *end, uint32_t n_ranges,
                                 uint8_t *out, uint64_t out_cap, uint64_t *out_off, int32_t *range_status,
                                 uint32_t *n_decoded, uint32_t *bad_unit, uint32_t flags);

/* -- Seek index: sparse, compressed windows packed and read on the device --------------
 * The windows of a seek index are 32 KiB of raw output per point: at a small span they outweigh the file.  Three opt-in
 * calls PACK them, UNPACK them and READ ranges straight through the packed form; the two calls above, the index (version
 * 1) and the raw windows stay what they are.  The rule is written once, csrc/seek_pack_rule.h; the kernels are
 * csrc/seek_pack_mark_kernel.inc (on the shared block reader) and csrc/seek_pack_kernels.hip.
 *
 * THE KEEP RULE (FLATE_HIP_SEEK_PACK_SPARSE).  Let P0 be the output offset of point p and [P0, P1) its segment.  A byte
 * of block p - 1 is NEEDED iff some copy at output position q in [P0, min(P1, P0 + 32768)) has a source byte a in
 * [q - dist, q - dist + len) with a < P0.  Later copies cannot reach the block (dist <= 32768); copies of copies are
 * covered, because the first copy was counted where it happened.  A sparse block has every other byte set to zero: a
 * read through it delivers the same bytes, because zeroed bytes are never read.
 * THE EMPTY-BLOCK RULE.  A block all of whose bytes are zero (after sparsifying, or as it came) is stored as NO bytes and
 * read back by zero fill without a decode.  Every other block is ONE raw DEFLATE stream: byte for byte what
 * flate_hip_deflate_fast_batch writes under flags 0 for the block's 32768 bytes.
 * THE PACK INDEX: a HOST array of 64-bit words: 0 the magic "FONESWPK" (little endian), 1 the version (1), 2 mode, 3
 * n_blocks = n_points - 1, 4 packed_bytes, 5 kept_bytes (SPARSE: the needed bytes; else n_blocks * 32768), 6 .. 10 the
 * binding to the seek index (its words 3, 6, 7, 8, 12: in_len, T, span, n, the unit rule), 11 .. 15 zero, then
 * off[n_blocks + 1]: byte offsets into `packed`, off[0] = 0, non-decreasing, block b = packed[off[b], off[b + 1]):
 * 17 + n_blocks words.  seek_pack_ok (host, O(n_blocks)) is seek_index_ok's counterpart.
 *
 * flate_hip_seek_windows_pack: PACK.  index / windows: what the build call returned.  in, windows and packed are host
 * buffers, or device buffers under FLATE_HIP_DEVICE_PTRS, at any byte alignment; `in` may be NULL without SPARSE (the
 * stream is only walked to mark; in_len and wrap are still the index's).  mode: FLATE_HIP_SEEK_PACK_COMPRESS, or
 * _COMPRESS | _SPARSE.  Verdict, in this order.
 *  1. FLATE_HIP_E_INVALID before any HIP call, nothing written: NULL ctx / pack_words / packed_bytes / kept_bytes; any
 *     other mode; any flag but FLATE_HIP_DEVICE_PTRS; a wrap above _GZIP; SPARSE with in == NULL and in_len > 0; windows
 *     == NULL with windows_bytes > 0, pack_index == NULL with pack_cap_words > 0, packed == NULL with packed_cap > 0; an
 *     index that fails seek_index_ok or names an unknown unit rule.
 *  2. pack_cap_words < 17 + n_blocks: FLATE_HIP_E_OUT_TOO_SMALL with *pack_words set.  (n_blocks == 0: the head and off =
 *     {0}, *packed_bytes = 0, FLATE_HIP_OK; nothing is walked.)
 *  3. With SPARSE: the stream is not the index's -- verdict 3 of flate_hip_inflate_one_ranges, or a walk that fails,
 *     meets a distance in front of the stream, or ends a segment anywhere but at the segment's end bit with exactly the
 *     segment's bytes: FLATE_HIP_E_CORRUPT.
 *  4. packed_cap below the total: FLATE_HIP_E_OUT_TOO_SMALL with *packed_bytes = the bytes needed (the encoder's scan
 *     knows every size before it packs).  The exact total is enough; flate_hip_seek_windows_pack_bound(n_blocks) =
 *     n_blocks * flate_hip_deflate_bound(32768) (host only) is always enough; nothing outside packed[0, packed_cap) is
 *     ever written.
 *  5. FLATE_HIP_OK: pack_index, packed[0, *packed_bytes), *pack_words, *kept_bytes.
 *   How: MARK + SPARSIFY, one wavefront per point p >= 1: a token walk from unit_bit[point_unit[p]] through block and
 *   unit headers alike (the unit rule does not matter) that stops once 32768 bytes of output have passed, at the
 *   segment's end bit, or behind the final block; no window, no store of the stream's output; the keep mask is 4 KiB of
 *   bits in LDS; then the same workgroup reads the raw block, zeroes what is not kept, writes a dense scratch slot and
 *   records "has a non-zero byte" and the kept count.  Without SPARSE only the non-zero test runs.  ONE read-back of the
 *   per-block records; the non-empty blocks, compacted in order, go as one batch through the unchanged encode path
 *   straight into `packed` or its staged copy; the host spreads the batch's offsets over off[].  Every loop consumes
 *   input bits or ends.  A segment whose first 32768 bytes of output take more than 2^30 bytes of input is refused as
 *   corrupt.
 *
 * flate_hip_seek_windows_unpack: (pack_index, packed) -> all n_blocks blocks in the raw layout: the sparsified windows,
 * or with COMPRESS alone the original windows byte for byte -- what the unchanged flate_hip_inflate_one_ranges takes.
 * FLATE_HIP_E_INVALID before any HIP call (NULL ctx / windows_bytes, a flag but FLATE_HIP_DEVICE_PTRS, a NULL buffer with
 * a size, a pack index that fails seek_pack_self_ok); windows_cap < n_blocks * 32768: FLATE_HIP_E_OUT_TOO_SMALL with
 * *windows_bytes set (the size query too); a block that does not inflate with status 0 to exactly 32768 bytes:
 * FLATE_HIP_E_CORRUPT with *bad_block (may be NULL) the first one, every other block exact.
 *
 * flate_hip_inflate_one_ranges_packed: flate_hip_inflate_one_ranges with (pack_index, pack_words, packed, packed_bytes)
 * in the place of (windows, windows_bytes).  Everything else is that call's: the arguments and the verdict order,
 * out_off, range_status, n_decoded, bad_unit and what is written where; verdict 1 additionally runs seek_pack_ok against
 * the index.  Between SELECT's read-back and the rounds the selected points' blocks are made: the non-empty ones by ONE
 * launch of the batch decoders into a dense stage of 32 KiB per SELECTED point, the empty ones by zero fill; the
 * rounds' window copy reads the stage through a point -> slot table, so device scratch for windows grows with the
 * selection, not with n_points, and with host pointers only the selected blocks' streams are uploaded.  A block that
 * does not inflate with status 0 to exactly 32768 bytes makes its point's unit a bad unit of status
 * FLATE_HIP_E_CORRUPT: the call returns the first bad unit's status in stream order with *bad_unit, every range that
 * decodes that unit gets that range_status and unspecified bytes, every other range is exact.  Delivered bytes equal
 * the raw call's for both modes.
 *   Out of scope: the gzfile seek index (its block numbering differs; the pack head's binding leaves room); building the
 *   packed form without the raw windows ever existing; checksums over windows; other tools' index formats; the MoonBit
 *   binding. */
#define FLATE_HIP_SEEK_PACK_COMPRESS 1u /* every block one raw DEFLATE stream */
#define FLATE_HIP_SEEK_PACK_SPARSE 2u   /* with _COMPRESS: unread bytes become zero first */
size_t flate_hip_seek_windows_pack_bound(uint64_t n_blocks);
int flate_hip_seek_windows_pack(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint32_t wrap,
                                const uint64_t *index, uint64_t index_words, const uint8_t *windows,
                                uint64_t windows_bytes, uint32_t mode, uint64_t *pack_index, uint64_t pack_cap_words,
                                uint64_t *pack_words, uint8_t *packed, uint64_t packed_cap, uint64_t *packed_bytes,
                                uint64_t *kept_bytes, uint32_t flags);
int flate_hip_seek_windows_unpack(flate_hip_ctx *ctx, const uint64_t *pack_index, uint64_t pack_words,
                                  const uint8_t *packed, uint64_t packed_bytes, uint8_t *windows, uint64_t windows_cap,
                                  uint64_t *windows_bytes, uint32_t *bad_block, uint32_t flags);
int flate_hip_inflate_one_ranges_packed(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint32_t wrap,
                                        const uint64_t *index, uint64_t index_words, const uint64_t *pack_index,
                                        uint64_t pack_words, const uint8_t *packed, uint64_t packed_bytes,
                                        const uint64_t *begin, const uint64_t *end, uint32_t n_ranges, uint8_t *out,
                                        uint64_t out_cap, uint64_t *out_off, int32_t *range_status, uint32_t *n_decoded,
                                        uint32_t *bad_unit, uint32_t flags);

/* -- Any gzip file: units found across member boundaries ------------------------------
 * RFC 1952 makes a gzip file a series of members, and everyday files are a few long members, or long and short ones
 * mixed (rotated logs concatenated after compression, pigz -i, dumps appended to).  WHICH CALL FOR WHICH FILE:
 * flate_hip_gzip_read for files of many small members (every member serial on one wavefront, no search over bits: the
 * fastest call there, members below "gzip_member_max" only); flate_hip_inflate_one for exactly one member;
 * flate_hip_gzfile_read for everything else and for files of unknown make-up: it cuts EVERY member into the units of
 * flate_hip_inflate_one_index and decodes them in parallel, and pays the search over every bit for it.  The link rule
 * between members is written once, csrc/gzfile_rule.h; the kernels are csrc/gzfile_kernels.hip.
 *
 * THE WALK that defines every result.  in[0, in_len) is the file; BITS ARE COUNTED FROM THE FILE'S FIRST BYTE.  p = 0.
 * p == in_len: success (in_len == 0: zero members, zero units, FLATE_HIP_OK).  The header rule at p is
 * flate_hip_gzip_index's over in[p, in_len), never clipped by "gzip_member_max"; no header at p: FLATE_HIP_E_CORRUPT,
 * the chain breaks at p.  The member's raw stream starts at byte r = p + header length and the serial decoder reads it
 * over [r, in_len - 8) -- the last 8 bytes of a file can only be a trailer; a stream that needs more is
 * FLATE_HIP_E_UNEXPECTED_EOF.  A non-zero status ends the walk in this member.  Otherwise b is the bit behind the final
 * block, the member is in[p, e) with e = ceil(b / 8) + 8, and p = e.  Anything behind the last member, zero bytes
 * included, is FLATE_HIP_E_CORRUPT at its offset.
 * UNITS are flate_hip_inflate_one_index's, per member: one starts at bit 8 r of every member whatever block type is
 * there, and at every dynamic block header the serial decode of that member reaches; every member has at least one
 * unit.  Unit k starts a member iff k == 0 or the unit in front of it on the chain ended with BFINAL.  HISTORY NEVER
 * CROSSES A MEMBER: unit k of a member whose first unit is f has min(32768, out_off[k] - out_off[f] + bytes produced)
 * bytes of history, and a distance beyond that is FLATE_HIP_E_CORRUPT at the serial offset, also when an earlier
 * member's output lies right in front of it in out.  Limits are per unit ("one_unit_max"); there is no per-member one.
 *
 * flate_hip_gzfile_index (discovery only).  Conventions: flate_hip_inflate_one_index's and flate_hip_gzip_index's.  The
 * four index arrays are HOST arrays; unit_bit / out_off (index_cap entries) and member_off / member_unit (member_cap
 * entries) are each both given or both NULL (both NULL: a count query); a pair that is too small is
 * FLATE_HIP_E_OUT_TOO_SMALL with every count set.  flags: FLATE_HIP_DEVICE_PTRS or 0, anything else is
 * FLATE_HIP_E_INVALID before any HIP call.  Nothing outside in[0, in_len) is read, at any alignment of in; nothing is
 * written to device memory the caller owns.  n_candidates, bad_member, err_off and stream_err_off may be NULL.
 * On success: unit_bit[0 .. n] (unit_bit[n]: the bit behind the last member's final block; a unit ends where the next
 * one starts, a member's last unit with its final block), out_off[0 .. n] (the exclusive prefix sum of what the units
 * inflate to; *out_bytes = out_off[n]), member_off[0 .. m] (file offsets, member_off[m] = in_len), member_unit[0 .. m]
 * (the first unit of each member, member_unit[m] = n); *status = 0, *bad_member = 0xffffffff, both offsets -1.
 * A broken chain: *status and the return value are the walk's code; *bad_member = the whole good members in front;
 * *err_off = the file offset where the failing member starts, or where no member could start; *stream_err_off = the
 * serial decoder's error offset counted from that member's raw stream's first byte (-1 for
 * FLATE_HIP_E_UNEXPECTED_EOF and FLATE_HIP_E_TOO_LARGE, and when no header was found); *n_units = the good units in
 * front of the failing one, those of the failing member included; *n_members = *bad_member; *out_bytes = 0; the good
 * prefix of all four arrays is still filled if it fits (unit_bit[n_units]: where the failing unit starts;
 * member_off[n_members] = *err_off; member_unit[n_members]: the failing member's first unit, or n_units when no header
 * was found).  The verdict is history-free and trailer-free, exactly as flate_hip_inflate_one_index's is.
 * *n_candidates: the nodes probed -- every bit offset that passes the dynamic-header rule (bit 0 included) and one per
 * byte offset that passes the header rule.
 *
 * flate_hip_gzfile_read: what zcat gives, the members' bytes back to back.  The total is known after discovery: above
 * out_cap it is FLATE_HIP_E_OUT_TOO_SMALL with *out_len = the size needed and nothing decoded (out == NULL with
 * out_cap == 0 is the size query).  Host pointers: the file is uploaded once and out[0, *out_len) downloaded once;
 * device pointers: nothing outside out[0, *out_len) is written.  THE VERDICT, in this order.  (1) A chain that breaks
 * (a header, a decode error, a unit too large, a distance in front of its member -- found by TAIL, reported at its
 * serial offset): *status, *bad_member, *err_off and *stream_err_off as in the index call; delivered are every good
 * member in front, whole, and the failing member's bytes in front of its failure (a unit that is too large delivers
 * nothing of itself); nothing behind the failure is written; *out_len is that count; no trailer is judged.  (2) Chain
 * good, a trailer wrong: every member is decoded and delivered, *out_len is the total, *status = FLATE_HIP_E_CORRUPT
 * for the first member in file order whose CRC-32 or ISIZE (mod 2^32) is not its trailer's, *bad_member its index,
 * *err_off its file offset, *stream_err_off that member's length (flate_hip_inflate_batch_framed's convention).
 * (3) Otherwise 0, 0xffffffff, -1, -1.  The return value is *status when that is not 0.
 *   How, all on the ctx's stream, no host pass over file bytes, no kernel waits for another workgroup.  CANDIDATES:
 *   list A, flate_hip_inflate_one_index's FIND over the whole file (decoys inside headers and trailers are candidates
 *   like any other); list B, flate_hip_gzip_index's header pass, each hit a node at bit 8 * (p + header length); one
 *   read-back of the two counts.  Both lists stay sorted in one node array; a bit that is in both is two nodes, and
 *   the path takes the one its predecessor names.  PROBE as in flate_hip_inflate_one_index, limited to
 *   [.., in_len - 8).  LINK: a node that stops in front of a dynamic header searches list A; one that ends with BFINAL
 *   takes THE HOP (csrc/gzfile_rule.h): e = ceil(b / 8) + 8; e == in_len: the terminal node; no header at e: the dead
 *   node, FLATE_HIP_E_CORRUPT at e; else the list B node of the header at e.  RANK, the out-size scan and the tail
 *   probe as there; a second scan over the path's "starts a member" marks gives member_unit and member_off.  DECODE in
 *   rounds of "one_round_units": TAIL with ooff = out_off[k] - out_off[first unit of k's member], the SEGMENTED compose
 *   / resolve of the seek index with every member's first unit as a seed (its dict_len is 0), pieces through the
 *   lane-per-stream dictionary decoder with a per-piece end.  VERIFY: one checksum launch planned over the members'
 *   output ranges, a thread per trailer, an ordered min.  Profiling: FLATE_HIP_STAGE_INFLATE is DECODE (of several
 *   rounds the last), FLATE_HIP_STAGE_CHECKSUM is VERIFY; the rest is counted in no stage.
 *   Out of scope: zlib or raw concatenations; routing
 *   flate_hip_gzip_read or flate_hip_inflate_one here automatically; fixed block starts as units (stored ones: option
 *   "one_stored_units"; a member's first unit starts
 *   behind its header whatever block is there, and the hop behind BFINAL is unchanged); caching across calls.
 *
 * SHORT MEMBERS DECODED WHOLE: the option "gzfile_serial_max" = S (0, the default: off -- both calls launch the
 * kernels above in that order, nothing more).  With S >= 1 a member whose header and raw stream fit in S bytes and
 * decode cleanly is a WHOLE member, ONE unit of the chain (the rule: csrc/gzfile_serial_rule.h).  For the member whose
 * header starts at byte p and is hl bytes long, the serial range is in[p + hl, E), E = min(in_len - 8, p + S); the
 * member is whole iff a size-only serial decode over that range ends its final block with status 0 and p + hl + used
 * <= E.  It is never searched for block headers and never walked symbolically; flate_hip_gzfile_read decodes all whole
 * members with ONE batch of the batch decoders (routed like flate_hip_inflate_batch from their count and S) straight
 * into their places in out, in front of the rounds.  Every other member -- longer, failing for any reason, the one the
 * chain breaks in -- is cut into units exactly as with S = 0.
 *   What never changes with the option: the delivered bytes, *out_len, *status, *bad_member, *err_off,
 *   *stream_err_off, *n_members, member_off and the trailer verdicts.  What DOES change: *n_units, unit_bit, out_off,
 *   member_unit and *n_candidates (which is why the default stays 0, as for "one_stored_units" and "zip_unit_min").  The
 *   units are S = 0's units without every unit of a whole member that is not that member's first; unit_bit and out_off
 *   of the kept units are S = 0's values; member_unit is renumbered; unit_bit[n_units], when the last good unit is a
 *   whole member, is the BYTE-ROUNDED bit behind its final block, 8 * (p + hl + used).  *n_candidates counts List B and
 *   the part of List A that was searched; it never exceeds S = 0's count.  "one_unit_max" and "one_round_units" apply
 *   to ordinary units only: a whole member is bounded by S (with "one_unit_max" lowered below S, a whole member may
 *   hold a unit that S = 0 refuses as too large).
 *   How: PHASE 1 -- List B, then ONE size-only launch of the batch decoders over the serial ranges of all B candidates
 *   (as flate_hip_gzip_index does), the whole test, the hop links of the whole candidates, and a pointer-doubling walk
 *   from the member at offset 0 for as long as the members it reaches are whole: find_from = the offset of the first
 *   member on that walk that is not whole, or in_len when the walk reaches the file's end, a dead hop or a file that
 *   starts with no member.  PHASE 2, only if find_from < in_len -- FIND (list A) over in[find_from, in_len) alone; PROBE
 *   over A and the B nodes that are not whole.  The chain, the scans and VERIFY are unchanged; the rounds run over the
 *   runs of units between whole members (a run starts with a member's first unit, a seed).  The whole-member batch is
 *   counted in FLATE_HIP_STAGE_INFLATE.  Device pointers: nothing at or behind out + T is written, T being what the
 *   size query reports; T == *out_len except when TAIL alone finds the failure (a distance in front of its member):
 *   whole members behind the failing one have been decoded by then, so out[*out_len, T) is unspecified in that case
 *   (with S = 0 it is untouched); the delivered bytes out[0, *out_len) are the same.
 *   Recommended: S = 1 MiB (1 GiB of S-text at zlib level 6 on one MI355X): a file of 16 384 members
 *   of 64 KiB reads in 21.1 ms instead of 1246.1 (flate_hip_gzip_read: 20.8), one of 1024 members of 1 MiB in 32.6
 *   instead of 883.6; what a file of long members pays is the size-only probe of each long member up to its clip,
 *   + 23 ms on one 1 GiB member (862.5 -> 885.5; S = 64 KiB: + 1.8, 256 KiB: + 4.8, 4 MiB: + 98.9), and S = 256 KiB
 *   or less leaves the 1 MiB members (about 410 KiB compressed) to the units.
 *   The option is ignored by flate_hip_gzfile_seek_index / _ranges, flate_hip_inflate_one*, flate_hip_gzip_* and the ZIP
 *   calls.  Out of scope: FIND in windows between long members (the search runs from the first long member to the
 *   file's end); running a clipped candidate again unclipped.
 * flate_hip_gzfile_last_route: what the last flate_hip_gzfile_index or flate_hip_gzfile_read on this ctx did --
 * *serial_members = the whole members among the discovery's good units, *unit_members = the discovery's other good
 * members (n_members - serial_members; the member a chain breaks in is counted in neither), *find_from as above (0
 * with the option off or an empty file: the search ran from the file's first byte; == in_len: no bit-offset search
 * ran).  Every pointer is required (else FLATE_HIP_E_INVALID); no HIP call. */
int flate_hip_gzfile_index(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint64_t index_cap,
                           uint64_t *unit_bit, uint64_t *out_off, uint64_t member_cap, uint64_t *member_off,
                           uint64_t *member_unit, uint32_t *n_units, uint32_t *n_members, uint64_t *out_bytes,
                           uint32_t *n_candidates, int32_t *status, uint32_t *bad_member, int64_t *err_off,
                           int64_t *stream_err_off, uint32_t flags);
int flate_hip_gzfile_read(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap,
                          uint64_t *out_len, uint32_t *n_members, uint32_t *n_units, uint32_t *n_candidates,
                          int32_t *status, uint32_t *bad_member, int64_t *err_off, int64_t *stream_err_off,
                          uint32_t flags);
int flate_hip_gzfile_last_route(const flate_hip_ctx *ctx, uint32_t *serial_members, uint32_t *unit_members,
                                uint64_t *find_from);

/* -- Any gzip file read in PARTS: members and units through bounded buffers ------------
 * flate_hip_gzfile_read wants the whole file; flate_hip_one_reader_* reads ONE member in parts.  A
 * flate_hip_gzfile_reader reads a file of ANY members through two bounded buffers: every call is flate_hip_gzfile_read
 * on the part of the file it is given -- its units cross member boundaries inside the part, the trailers of the members
 * that end in it are judged in it -- and between two calls the handle holds where the file stands (the rule:
 * csrc/gzfile_parts_rule.h; the chain's kernels are the whole call's, csrc/gzfile_kernels.hip, which run the whole file
 * as the part that is final and starts at a BOUNDARY; a part's decode words: csrc/gzfile_parts_kernels.hip).
 *
 * open: flags is 0 or FLATE_HIP_DEVICE_PTRS (in and out of every read are device buffers); anything else, or a NULL ctx
 * or result pointer, is FLATE_HIP_E_INVALID before any HIP call.  The handle records "one_stored_units" and
 * "one_unit_max" as the ctx has them at open.  reset: a fresh file on the same handle.  The ctx must outlive it.
 *
 * read: in[0, in_len) BEGINS with the bytes the last call left unused; final_in != 0: no bytes follow.  Returns
 * FLATE_HIP_OK (call again), FLATE_HIP_STREAM_END (a final call whose walk reached the file's end; sticky), the file's
 * error (sticky: every later call returns it with the same *bad_member, *err_off and *stream_err_off, *in_used = 0), or
 * one of the repeatable codes, which follow flate_hip_one_reader_read's rule: FLATE_HIP_E_OUT_TOO_SMALL with *out_len =
 * the first unit's size, FLATE_HIP_E_INVALID (NULL reader / in with in_len > 0 / out with out_cap > 0 / in_used /
 * out_len, before any HIP call), and FLATE_HIP_E_HIP in front of the point where the call begins to move the handle's
 * device words -- such a call has changed nothing; behind that point it is sticky.  n_members, n_units, bad_member,
 * err_off and stream_err_off may be NULL.  An empty file -- a final call without bytes on a fresh handle -- is
 * FLATE_HIP_STREAM_END with nothing.
 *   THE CONTRACT.  Let F be the concatenation of everything the calls consumed.  THE WALK of flate_hip_gzfile_read over
 *   F (above) defines the members, the units, the bytes and the offsets, and the reader's results are independent of
 *   where the parts are cut and of out_cap.  The concatenation of every call's out[0, *out_len) is F's output up to the
 *   first failure in file order: a failing unit of member j comes before j's trailer; a chain break delivers the good
 *   members in front whole and the failing member's bytes in front of its failure, as the whole call; a wrong trailer
 *   delivers up to and including that member's last byte and nothing behind it.  The sticky status and words are the
 *   whole call's for that failure: *bad_member counts members over the file, *err_off is the member's FILE offset (or
 *   the offset where no member could start), *stream_err_off counts from that member's raw stream's first byte across
 *   parts, and a wrong trailer gives the member's length.  ONE DIFFERENCE from flate_hip_gzfile_read: of a file with a
 *   wrong trailer in front of a chain break the reader reports the wrong trailer -- the whole call judges no trailer
 *   once the chain breaks and reports the break, but only the reader's answer can be the same for every cut.  On
 *   success the *in_used of all calls sum to F's length; *n_members of a call is the number of members whose trailers
 *   it judged good, *n_units the complete units it delivered.
 *   STATE.  Between two calls the reader stands at a BOUNDARY (the next part's first byte is where a header must stand,
 *   or the file's end) or INSIDE a member (the next unit starts at bit b0 of the next part's first byte; the device
 *   holds the 32 KiB window and the member's running CRC-32).  There is no "trailer pending" state: on EVERY part the
 *   probes read in[.., in_len - 8), so a final block that is complete has its trailer inside the part; a unit that needs
 *   more is cut, which is a verdict only on a final part (FLATE_HIP_E_UNEXPECTED_EOF, as the whole call).
 *   ROOT.  INSIDE: FIND's PARTS build with candidate 0 at bit b0.  BOUNDARY: the header at byte 0 -- a byte that fails
 *   is FLATE_HIP_E_CORRUPT at the file offset; a header the part cuts, or one with fewer than 8 bytes behind it, uses
 *   nothing on a part that is not final and is the whole call's FLATE_HIP_E_CORRUPT on a final one.
 *   THE PARTS HOP behind a final block at bit b, e = ceil(b / 8) + 8 <= in_len: e == in_len is the file's end on a
 *   final part, else a BOUNDARY stop; a header at e (the header rule over in[e, in_len)) is the next member; otherwise
 *   the chain is dead on a final part, and on any other part only where a byte of in[e, in_len) fails already -- else a
 *   BOUNDARY stop at e.
 *   DELIVERY is flate_hip_one_reader_read's: the longest prefix of complete units that fits out_cap, with the part's
 *   own verdict behind them when everything in front fits.  A call that delivers no unit and has no verdict uses
 *   nothing (in_len >= "one_unit_max": FLATE_HIP_E_TOO_LARGE).  *in_used is the byte of the first undelivered unit's
 *   first bit; if that unit is a member's first, the trailer and the header in front of it are used.  A BOUNDARY stop
 *   gives *in_used = e.
 *   HISTORY never crosses a member: a unit of the continued member sees min(32768, the member's bytes before the part +
 *   its offset inside the part's share of the member + the bytes produced), every other unit flate_hip_gzfile_read's
 *   value.
 *   CHECKSUMS.  One checksum launch is planned over the members' ranges inside the delivered bytes; the first range is
 *   joined to the carried sum on the device; a thread per member that ends among the delivered units holds CRC-32 and
 *   ISIZE against the trailer in the part.  The window behind the last delivered unit goes back into the handle once
 *   the result words are good.
 *   Host pointers: one upload and one download per call.  Device pointers: nothing outside out[0, planned total) is
 *   written, planned total <= out_cap, and nothing outside out[0, *out_len) except in a call that reports a wrong
 *   trailer, where out[*out_len, planned total) is unspecified.  Per call the host waits for the discovery's two
 *   read-backs and one read-back of the result words.
 *   SHORT MEMBERS WHOLE (flate_hip_gzfile_reader_set_serial_max, S >= 1; the rule: csrc/gzfile_parts_serial_rule.h, the
 *   kernels: csrc/gzfile_parts_serial_kernels.hip, which run the whole call's phase 1 too).
 *   The ctx option "gzfile_serial_max" is ignored by the reader: the setting is the handle's.
 *   With S = 0, the default, a call launches exactly what is described above.  With S >= 1 a member that lies whole
 *   inside the part, fits in S bytes and decodes cleanly is ONE unit: it is never searched for
 *   block headers and never walked symbolically, and the call decodes all such members with one batch of the batch
 *   decoders, in front of the rounds (counted in FLATE_HIP_STAGE_INFLATE).  Every offset p that passes the header rule
 *   over in[p, in_len) gets the serial range of flate_hip_gzfile_read's option with the PART's in_len, E = min(in_len -
 *   8, p + S), and one size-only launch of the batch decoders runs over all ranges.  THREE VERDICTS: WHOLE -- the whole
 *   test holds and the member inflates to at most out_cap bytes; OPEN -- the part is not final, the range was clipped
 *   by the part and not by S (in_len - 8 < p + S) and the decode ran out of input there (FLATE_HIP_E_UNEXPECTED_EOF, or
 *   the header alone did not fit in front of E): more bytes could make it whole; LONG -- everything else (longer than
 *   S, corrupt, 4 GiB or more, larger than out_cap): cut into units exactly as with S = 0, so a bounded output buffer
 *   always makes the progress S = 0 makes.  A final part has no OPEN verdict.  THE WALK and find_from: INSIDE a member
 *   find_from = 0 -- the continued member is units, FIND runs in its PARTS build over the part, whole members behind it
 *   are still single nodes.  At a BOUNDARY the walk goes from the member at byte 0 along THE PARTS HOP for as long as
 *   members are WHOLE: a LONG member at p gives find_from = p; an OPEN member at p > 0 ends the chain with a BOUNDARY
 *   stop at p and find_from = in_len; an OPEN member at the root is treated as LONG (find_from = 0), so the reader
 *   never needs a part of a minimum size; the file's end, a dead hop or a stop give find_from = in_len.  Everywhere in
 *   the chain a hop that lands on the header of an OPEN member is a BOUNDARY stop there.  FIND runs over in[find_from,
 *   in_len) only, or not at all.  STATE: with S >= 1 a call whose first undelivered unit is a member's first unit stops
 *   at the BOUNDARY in front of that member's HEADER (*in_used = the header's offset), so that the next part judges the
 *   member as a root; no window leaves a call whose last delivered unit is a whole member.  THE CONTRACT holds for every
 *   cut, every out_cap and every S: the bytes, the sticky status and words and the sum of *in_used are the walk's;
 *   *n_units and *in_used of a single call depend on S, and the *n_units of a file's calls sum to the walk's units
 *   minus every unit of a whole member that is not its first.  A whole member is a checksum segment of one unit; the
 *   guarantee about out[0, planned total) is unchanged (the batch's last slot ends at the planned total).
 *   set_serial_max: S is 0 .. 2^28 - 1 and the handle must be FRESH -- behind open or reset, before any call has
 *   consumed a byte -- else FLATE_HIP_E_INVALID, as for a NULL handle; no HIP call; reset keeps S, as it keeps the unit
 *   rule.  last_route reports on the last read that ran a discovery: *serial_members = the whole members among the units
 *   it delivered, *open_stop = 1 when its chain ended at a BOUNDARY stop in front of an OPEN member, *find_from = the
 *   part offset FIND started at (that call's in_len: no bit-offset search ran; 0 with S = 0).  Every pointer is
 *   required (else FLATE_HIP_E_INVALID); no HIP call.
 *   Out of scope: FIND in windows between long members (the search runs from find_from to the part's end, so "INSIDE,
 *   then many short members in the same part" pays FIND over the part); zlib or raw concatenations; overlapping the
 *   upload of part k + 1 with the decode of part k; a seek index built in parts; the MoonBit binding. */
typedef struct flate_hip_gzfile_reader flate_hip_gzfile_reader;
int flate_hip_gzfile_reader_open(flate_hip_ctx *ctx, uint32_t flags, flate_hip_gzfile_reader **reader);
int flate_hip_gzfile_reader_read(flate_hip_gzfile_reader *reader, const uint8_t *in, uint64_t in_len, int final_in,
                                 uint8_t *out, uint64_t out_cap, uint64_t *in_used, uint64_t *out_len,
                                 uint32_t *n_members, uint32_t *n_units, uint32_t *bad_member, int64_t *err_off,
                                 int64_t *stream_err_off);
int flate_hip_gzfile_reader_reset(flate_hip_gzfile_reader *reader);
void flate_hip_gzfile_reader_free(flate_hip_gzfile_reader *reader);
int flate_hip_gzfile_reader_set_serial_max(flate_hip_gzfile_reader *reader, uint64_t serial_max);
int flate_hip_gzfile_reader_last_route(const flate_hip_gzfile_reader *reader, uint32_t *serial_members,
                                       uint32_t *open_stop, uint64_t *find_from);

/* -- Seek index for any gzip file: build once, read ranges across members -------------
 * flate_hip_gzfile_read pays the whole discovery on every call and delivers everything.  flate_hip_gzfile_seek_index
 * keeps the discovery of a file of ANY members, flate_hip_gzfile_ranges reads byte ranges of what zcat gives through it
 * and decodes only the units they need.  The rule and the layout are written once, csrc/gzfile_seek_rule.h; the new
 * kernels are csrc/gzfile_seek_kernels.hip; everything else is the two sections above, unchanged.
 *
 * Notation is flate_hip_gzfile_index's: n units, unit_bit[0 .. n] with bits counted from the FILE's first byte,
 * out_off[0 .. n], T = out_off[n], m members, member_off[0 .. m], member_unit[0 .. m]; f(k) is the first unit of unit
 * k's member; U[0, T) is what zcat gives.
 *
 * THE POINT RULE.  Unit k is a POINT iff k == 0, or k starts a member, or out_off[k] / span > out_off[k - 1] / span.
 * span is flate_hip_inflate_one_seek_index's (0: FLATE_HIP_SEEK_SPAN_DEFAULT); with FLATE_HIP_SEEK_SPAN_NONE the points
 * are exactly the member starts and the index is the cached discovery.  pstart(k) and segments are defined as there,
 * so a segment never crosses a member.
 * WINDOWS.  A point that starts a member has NO window: history never crosses a member.  Every other point p with unit
 * u has one block of 32768 bytes, block number p - j with j = the members whose first unit is at or in front of u
 * (derived, not stored): n_points - m blocks.  A block is the 32 KiB of ITS MEMBER's output in front of unit u, in
 * stream order; bytes in front of the member's first byte are 0 -- never the bytes of the member in front, although
 * those lie right there in U.  `windows` is host, or device under FLATE_HIP_DEVICE_PTRS like in, at any byte alignment.
 * INDEX: a HOST array of 64-bit words: word 0 the magic "FGZFSIDX" (little endian), 1 the version (1), 2 in_len, 3 T,
 * 4 span, 5 n, 6 m, 7 n_points, 8 the unit rule the index was built with (0 or 1 as in word 12 of the one-stream index:
 * flate_hip_gzfile_ranges walks by it, any other value is FLATE_HIP_E_INVALID), 9 .. 15 zero; then unit_bit[n + 1],
 * out_off[n + 1], member_off[m + 1],
 * member_unit[m + 1], point_unit[n_points]: 16 + 2 (n + 1) + 2 (m + 1) + n_points words.  The empty file (in_len == 0):
 * the 16 head words alone, n = m = n_points = 0, no windows.
 *
 * flate_hip_gzfile_seek_index: BUILD.  Conventions are flate_hip_inflate_one_seek_index's: flags FLATE_HIP_DEVICE_PTRS
 * or 0, FLATE_HIP_E_INVALID before any HIP call (NULL ctx / in with in_len > 0 / index_words / windows_bytes / n_units /
 * n_members / n_points / out_bytes / status; index == NULL with index_cap_words > 0, windows == NULL with windows_cap >
 * 0; any other flag); host pointers are uploaded once.  n_candidates, bad_member, err_off and stream_err_off may be
 * NULL.  Both sizes are known after POINTS, in front of TAIL: a too-small index_cap_words or windows_cap -- both
 * buffers NULL with capacity 0 is the size query -- returns FLATE_HIP_E_OUT_TOO_SMALL with every count set
 * (*index_words, *windows_bytes, *n_units, *n_members, *n_points, *out_bytes = T) and nothing written.  Nothing outside
 * windows[0, windows_cap) is ever written.
 * Verdict: *status, *bad_member, *err_off and *stream_err_off are flate_hip_gzfile_index's for the same bytes; in
 * addition a distance that reaches in front of its member is found by TAIL, which runs over every unit whatever the
 * span, and reported at its serial offset as flate_hip_gzfile_read reports it (*n_units, *n_members: the good ones in
 * front).  TRAILERS ARE NOT JUDGED: nothing is decoded to output, so there is nothing to sum; a caller who wants them
 * judged calls flate_hip_gzfile_read once.  A file whose status is not 0 gets no index: *index_words = *windows_bytes
 * = 0, *n_points = 0, *out_bytes = 0, the return value is the status; what `windows` holds then is unspecified.
 * in_len == 0: FLATE_HIP_OK, the 16 head words alone.
 *   How: flate_hip_gzfile_index's discovery; POINTS, one workgroup, the rule with the discovery's member-start mark
 *   per unit, a scan that counts points and windows, a compaction; ONE read-back of the index arrays; per round of
 *   "one_round_units" TAIL over EVERY unit with out_off[k] - out_off[f(k)] as its offset and the segmented COMPOSE /
 *   RESOLVE with every member's first unit as a seed, exactly as flate_hip_gzfile_read runs them, over slots zeroed
 *   first so that a member's first window is zeros; in DECODE's place PACK: the round's points as runs for the gather
 *   kernel of the BGZF range call, a member start being a run of no bytes, so that every window lands in its block.
 *
 * flate_hip_gzfile_ranges: READ.  Ranges, out_off, range_status, the layout, the TOUCHED set and *bad_unit are
 * flate_hip_inflate_one_ranges's over U; a range may cross members.  The DECODED set is the union, over the non-empty
 * ranges, of [pstart(first), last] (first / last: the range's first and last touched unit): the union over touched k
 * of [pstart(k), k] and, between two touched units of one range, the units that produce no output -- an empty member
 * is a segment of its own that no touched unit names, and costs one empty piece.  *n_decoded is its size.  Verdict, in
 * this order.
 *  1. FLATE_HIP_E_INVALID before any HIP call: any of flate_hip_bgzf_read_ranges's argument refusals; windows == NULL
 *     with windows_bytes > 0; an index that fails gzfile_seek_index_ok (host, O(n + m), reads nothing outside the
 *     words): a wrong magic or version; in_len not the call's; a word count or windows_bytes that is not what the counts
 *     imply; not (n >= 1, 1 <= m <= n, m <= n_points <= n, span >= 1) and not the empty file's head with in_len = 0 and
 *     T = 0; unit_bit not strictly increasing; out_off not non-decreasing from 0 to T; member_off not strictly
 *     increasing from 0 to in_len; member_unit not strictly increasing from 0 to n; a member whose units do not lie
 *     inside it (unit_bit[member_unit[j]] >= 8 (member_off[j] + 10), unit_bit[member_unit[j + 1] - 1] < 8
 *     (member_off[j + 1] - 8)); a unit of more than 2^28 bytes of input, a member's last unit measured to 8
 *     (member_off[j + 1] - 8); point_unit not exactly the point rule's set for the stored span.
 *  2. n_ranges == 0: out_off[0] = 0 if out_off is given, FLATE_HIP_OK, nothing is read.
 *  3. The file is not the one the index was built from -- some member's header, parsed on the device, does not end
 *     where the index has that member's first unit: FLATE_HIP_E_CORRUPT, every range_status FLATE_HIP_E_CORRUPT, every
 *     out_off 0, nothing decoded.
 *  4. A total above out_cap: FLATE_HIP_E_OUT_TOO_SMALL, out_off fully written, nothing decoded.  out == NULL with out_cap
 *     == 0 is the size query -- unless the total is 0, which is FLATE_HIP_OK.
 *  5. Decode and deliver, as verdict 5 there: a decoded unit is GOOD iff its piece ends with status 0 and fills exactly
 *     out_off[k + 1] - out_off[k]; range_status, the return value and *bad_unit as there.
 * The decoders read in[0, in_len - 8) with bits counted from the file's first byte; a unit runs to BFINAL iff the next
 * unit starts a member or there is none, and its history is min(32768, out_off[k] - out_off[f(k)]) bytes.  Host
 * pointers: the file is uploaded once, only the blocks of the selected window-bearing points are uploaded, the
 * delivered bytes come down once; the host reads no file byte and waits once before decoding.
 *   How: MEMBERS, one thread per member, the header rule at member_off[j] against unit_bit[member_unit[j]], an ordered
 *   min; REL, one thread per unit; LOCATE, SELECT, LAYOUT and ONE read-back as in flate_hip_inflate_one_ranges; rounds
 *   over the unit list: SEED (the piece from the index), LOAD (the stored window of each of the round's points into
 *   its slot by the block formula, ZEROS for a member start, the carried window left alone), TAIL, the segmented scan,
 *   RESOLVE, DECODE, CHECK; GATHER.  Profiling stages are flate_hip_inflate_one_ranges's.  No kernel waits for another
 *   workgroup.
 *   Out of scope: judging trailers from either call; an index of the good prefix of a broken file; zlib or raw
 *   concatenations; compressed windows; other tools' index formats; caching in the ctx. */
int flate_hip_gzfile_seek_index(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint64_t span, uint64_t *index,
                                uint64_t index_cap_words, uint64_t *index_words, uint8_t *windows, uint64_t windows_cap,
                                uint64_t *windows_bytes, uint32_t *n_units, uint32_t *n_members, uint32_t *n_points,
                                uint64_t *out_bytes, uint32_t *n_candidates, int32_t *status, uint32_t *bad_member,
                                int64_t *err_off, int64_t *stream_err_off, uint32_t flags);
int flate_hip_gzfile_ranges(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, const uint64_t *index,
                            uint64_t index_words, const uint8_t *windows, uint64_t windows_bytes, const uint64_t *begin,
                            const uint64_t *end, uint32_t n_ranges, uint8_t *out, uint64_t out_cap, uint64_t *out_off,
                            int32_t *range_status, uint32_t *n_decoded, uint32_t *bad_unit, uint32_t flags);

/* -- ZIP archives ----------------------------------------------------------------
 * The everyday container of a batch of independent DEFLATE streams (.zip, .npz, .jar, .whl, .docx; PKWARE APPNOTE
 * 6.3), and the one whose own index, the central directory, makes writing and reading parallel.  The format rule is
 * written once, csrc/zip_rule.h; the kernels are csrc/zip_kernels.hip.
 *
 * WRITING: entry i is in[in_off[i], in_off[i+1]), named names[name_off[i], name_off[i+1]) (UTF-8; names and name_off
 * are HOST arrays always, like every offset table).  Its data is exactly the bytes the raw batch call produces for
 * stream i under the same flags (an empty entry: 01 00 00 ff ff).  Local headers carry CRC-32 and both sizes (no data
 * descriptors), flags 0x0800, method 8, time 0, date 0x0021; a central record carries a Zip64 extra exactly when its
 * header offset >= 0xffffffff, and the Zip64 end record and locator appear exactly when n >= 65535 or the directory's
 * offset or size >= 0xffffffff.  entry_off (host, n + 1, may be NULL) receives the local header offsets, [n] = where
 * the directory starts.  Refused before any HIP call with FLATE_HIP_E_INVALID: a name of 0 or more than 65535 bytes,
 * name_off not monotone, NULLs, flags other than FLATE_HIP_DEVICE_PTRS | FLATE_HIP_COMPAT_GO.  out_cap: the exact
 * total is enough to the byte, one byte less is FLATE_HIP_E_OUT_TOO_SMALL (decided on the device by the scan); the
 * bound below is always enough.  n == 0 gives the 22-byte empty archive.  Host pointers: one copy in, one copy out.
 *   How: a scan over 30 + name + raw size places the members and gives the pack kernels their offsets; the CRC-32s
 *   run on the input where it is; one thread per entry writes its local header and its central record behind the
 *   pack kernel, one thread the end records -- all queued on the ctx's stream, the checksum and writer kernels
 *   counted as FLATE_HIP_STAGE_CHECKSUM.
 *
 * READING.  Absolute offsets, one disk.  The end record is the HIGHEST p in [max(0, in_len - 65557), in_len - 22] with
 * its signature and p + 22 + comment length == in_len; a Zip64 locator at p - 20 moves the values to the Zip64 end
 * record.  The directory is exactly n records chained from its offset and ending exactly at offset + size.  Sizes and
 * CRC-32 always come from the directory (data descriptors need no pass), data_off from the LOCAL header's lengths.
 * The archive's verdict is FLATE_HIP_E_CORRUPT with err_off = in_len (no end record), the end record's offset (a
 * refused end record, Zip64 record or directory range) or the offset at which a record was expected (a record that
 * cannot be read, bytes left behind n records, the directory's end reached early); n_entries = the well-formed
 * records in front of it.  An entry's status at index time: FLATE_HIP_E_UNSUPPORTED for flag bit 0, 5 or 6 or a
 * method other than 0 and 8; FLATE_HIP_E_CORRUPT for a local header without its signature or not in front of the
 * directory, data that runs into the directory, or a stored entry whose two sizes differ.
 *   How: the end record by one thread per offset of the tail window and an atomic max; the directory as BGZF members
 *   are found (every offset tested with 16-byte loads, hits compacted in file order, each linked to the candidate at
 *   its own end by binary search, the chain ranked by pointer doubling); one thread per record reads the record and
 *   its local header; a scan of the sizes.  No host pass over file bytes; nothing outside in[0, in_len) is read, at
 *   any alignment of in.
 *
 * READING LONG ENTRIES: the option "zip_unit_min".  The batch decoders give an entry one lane or one wavefront, the
 * right shape for .jar, .whl and .docx and the wrong one for an .npz of a few large arrays or a .zip of one large CSV.
 * With "zip_unit_min" = v >= 1 (0, the default: off -- the same kernels, no new launch, no new allocation) a selected
 * deflated entry with comp_size >= v is LONG and is decoded as flate_hip_gzfile_read decodes a long member: in UNITS
 * found on the device, all long entries as ONE chain.  The rule is written once, csrc/zip_units_rule.h; the kernels are
 * csrc/zip_units_kernels.hip.  The set L: the selection slots, in ascending order, whose entry has index status 0,
 * method 8, comp_size >= v, is not FLATE_HIP_E_TOO_LARGE, is the first occurrence of its entry number in sel, and
 * whose data range overlaps no other such entry's range (archives whose records share data exist; those go to the
 * batch decoders).  FIND runs over the HULL of L's data ranges only, and every bit of the unit path is counted from
 * the hull's first byte.  A unit of entry X links to the unit that starts where it stops, inside X's range; a unit
 * that ends with BFINAL at or before X's end links to the first unit of the next L entry, which starts at 8 * data_off
 * whatever block type is there; anything else ends the chain.  An L entry is GOOD iff its chain reaches BFINAL
 * inside its range, its units' output sums to exactly `size`, and every unit passes TAIL and the decode round's
 * check.  With g = the L entries in front of the first that is not GOOD, L[0, g) are served by units -- unit k of
 * entry j writes at out_off[j] + (what j's units in front of k produce), with min(32768, that) bytes of history,
 * never another entry's -- and L[g] and every L entry behind it go to the batch decoders in the same call: a broken
 * archive costs what it costs with the option off.  CRC-32 and size of every entry are judged by the same kernels.
 * RESULTS ARE THOSE OF THE OPTION AT 0 for every archive, selection, pointer kind and alignment: out[0,
 * out_off[n_sel]), out_off, out_len, status, err_off, n_entries, archive_err_off and the return value (the slot of an
 * entry whose status is not 0 excepted: empty or as far as it came).  The size query and FLATE_HIP_E_OUT_TOO_SMALL are
 * decided before any discovery.  The options "one_stored_units", "one_unit_max" and "one_round_units" apply as in
 * flate_hip_gzfile_read.  Which path ran: flate_hip_zip_last_route.
 *   How: L is host code over the index that comes back anyway, O(|L| log |L|).  FIND's count pass over the hull, ONE
 *   read-back of the count; fill, the B nodes' bits from the directory, PROBE of every node, link, pointer doubling,
 *   finish, out-scan, the entry scan, the entry-relative offsets, ONE read-back of the head words and every entry's
 *   first unit; rounds of TAIL, pieces in ZIP's slots (between two entries' slots a piece of no bits, so that every
 *   unit's slot is exactly its size), the segmented COMPOSE / RESOLVE with every entry's first unit as a seed, DECODE,
 *   CHECK; ONE small read-back (g); then ONE batch-decoder launch over the short and the fallback entries, the stored
 *   copies, the checksums and the verdict as before.  Stages: discovery is counted in no stage, as in
 *   flate_hip_gzfile_read; FLATE_HIP_STAGE_INFLATE is the batch launch, or the last round's decoder launch when no
 *   entry is left for the batch decoders.  No kernel waits for another workgroup.
 * WRITING LONG ENTRIES: the option "zip_piece_bytes".  flate_hip_zip_write gives an entry one wavefront, the wrong shape
 * for an .npz of one large array.  With "zip_piece_bytes" = P >= 1 (0, the default: off) an entry longer than P bytes is
 * cut into ceil(len / P) pieces of P bytes, the last one shorter (zip_pieces_plan, csrc/splice_rule.h); the pieces of
 * an entry are one group of a grouped splice (flate_hip_deflate_fast_grouped_framed, above), so the entry's data is ONE
 * legal DEFLATE stream -- exactly what flate_hip_deflate_fast_spliced writes for those pieces -- and its sizes and
 * CRC-32 in the local header and the central record are the entry's own: an ordinary ZIP archive.  Entries of at most P
 * bytes are groups of one piece and their bytes are what they are with the option off.  When no entry is longer than P
 * the call takes the route of the option at 0: the same kernels, no new launch, no new allocation, the same bytes.
 * Everything the call refuses with the option off it refuses with it on; more than 2^32 - 2 pieces, or an entry whose
 * stream reaches 4 GiB: FLATE_HIP_E_TOO_LARGE.  Pieces share no history, so the archive grows as P shrinks (at P =
 * 65535 a piece is one window of the plain stream with its own first block).  flate_hip_zip_bound does not know P: it
 * covers every P >= 65535; below that add flate_hip_deflate_bound(0) per piece beyond the first of each entry (the
 * room is judged on the device either way: too little is FLATE_HIP_E_OUT_TOO_SMALL, nothing written).  Which path ran:
 * flate_hip_zip_write_last_route.  Out of scope: choosing P per entry, pieces that share history.
 * Out of scope: archives with prepended data, several disks, encryption, methods other than 0 and 8, comments on
 * write; uploading only the selected entries from host memory; caching the index across calls; entries of 4 GiB or
 * more through units; a seek index for entries; independent chains per entry. */
typedef struct flate_hip_zip_entry {
  uint64_t name_off;    /* the name's place in the archive (the directory's copy), name_len bytes */
  uint64_t header_off;  /* the local header */
  uint64_t data_off;    /* the entry's data (0 where the local header cannot be used) */
  uint64_t comp_size, size;
  uint32_t crc32;
  uint16_t name_len, method, flags, reserved;
  int32_t status;
  uint32_t reserved2;
} flate_hip_zip_entry; /* 64 bytes: 60 of fields and 4 of padding behind them */
/* room that is always enough for the archive of these entries; 0 for offsets or names that would be refused */
size_t flate_hip_zip_bound(const uint64_t *in_off, uint32_t n, const uint64_t *name_off);
int flate_hip_zip_write(flate_hip_ctx *ctx, const uint8_t *in, const uint64_t *in_off, uint32_t n,
                        const uint8_t *names, const uint64_t *name_off, uint8_t *out, uint64_t out_cap,
                        uint64_t *out_len, uint64_t *entry_off, uint32_t flags);
/* Discovery only.  entries / out_off: host arrays of index_cap / index_cap + 1 entries, both NULL for a count query;
 * too small is FLATE_HIP_E_OUT_TOO_SMALL with the counts set.  out_off = the exclusive prefix sum of size over the
 * entries with status 0 (the others get empty slots), *out_bytes its last entry.  More than 2^32 - 2 entries:
 * FLATE_HIP_E_TOO_LARGE.  flags: FLATE_HIP_DEVICE_PTRS or 0. */
int flate_hip_zip_index(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, uint64_t index_cap,
                        flate_hip_zip_entry *entries, uint64_t *out_off, uint32_t *n_entries, uint64_t *out_bytes,
                        int64_t *err_off, uint32_t flags);
/* Index, one read-back, then decode and verify.  sel (host, n_sel entry numbers in any order, duplicates allowed) or
 * NULL = every entry; n_cap = the capacity of out_off (n_cap + 1), out_len, status and err_off (host arrays).  The
 * selected entries' bytes lie back to back in out in the order given; out_off (n_sel + 1) is written.  Method 8 runs
 * through the batch decoders, method 0 through a copy kernel; the CRC-32 of what was produced is judged on the device.
 * An entry's verdict, in order: its index status; the decoder's own status with err_off counted from data_off;
 * FLATE_HIP_E_OUT_TOO_SMALL if it produces more than size; FLATE_HIP_E_CORRUPT with err_off = comp_size if it produced
 * another length than size or another CRC-32.  An entry of 4 GiB or more (or of 2 GiB or more of compressed data) is
 * FLATE_HIP_E_TOO_LARGE for that entry.  A failing entry does not stop the others and gets an empty slot or leaves
 * its slot as far as it came.
 * Returns: the archive's verdict (with *archive_err_off, nothing written); FLATE_HIP_E_INVALID for a sel entry >= n or
 * n_sel > n_cap, before decoding (sel == NULL takes n_sel == 0, and more entries than n_cap are
 * FLATE_HIP_E_OUT_TOO_SMALL with *n_entries set); an entry's err_off is -1 unless stated; FLATE_HIP_E_OUT_TOO_SMALL with out_off fully written and nothing decoded when the
 * total exceeds out_cap (out == NULL and out_cap == 0 is the size query); else the first non-zero entry status in the
 * order given.  With device pointers nothing outside out[0, out_off[n_sel]) is written. */
int flate_hip_zip_read(flate_hip_ctx *ctx, const uint8_t *in, uint64_t in_len, const uint32_t *sel, uint32_t n_sel,
                       uint32_t n_cap, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint64_t *out_len,
                       int32_t *status, int64_t *err_off, uint32_t *n_entries, int64_t *archive_err_off,
                       uint32_t flags);
/* What the last flate_hip_zip_read on this ctx did with the option "zip_unit_min": *unit_entries = the selection slots
 * served by units; *fallback_entries = the slots that qualified by size but went to the batch decoders (a duplicate,
 * an overlapping range, at or behind the first entry that is not GOOD); *n_units = the units on the served entries'
 * path; *n_candidates = FIND's candidates in the hull.  All zero when the option is 0, and after a call that decoded
 * nothing.  Results are identical by design: this is how a caller sees which path ran.  No HIP call. */
int flate_hip_zip_last_route(const flate_hip_ctx *ctx, uint32_t *unit_entries, uint32_t *fallback_entries,
                             uint32_t *n_units, uint32_t *n_candidates);

/* What the last flate_hip_zip_write on this ctx did with the option "zip_piece_bytes": *long_entries = the entries
 * written from more than one piece, *n_pieces = the pieces of the whole call.  Both zero on the unchanged route (the
 * option at 0, or no entry longer than it) and after a call that failed.  No HIP call. */
int flate_hip_zip_write_last_route(const flate_hip_ctx *ctx, uint32_t *long_entries, uint32_t *n_pieces);

/* -- exchange step (multi-GPU) ---------------------------------------------------
 * SURVEY 8(e) / section 5; no counterpart in the reference (single-threaded, no communication
 * layer).  Independent streams shard by contiguous index range, one process and one ctx per
 * GPU, no collective in the compress path; this step concatenates the compressed shards on
 * every rank over RCCL (xGMI inside a node).  A host in the reference's language drives it
 * through these entry points; moonbit-flate_amd/shard.py is a thin caller.
 *
 * A flate_hip_comm wraps one RCCL communicator (created here from a unique id that rank 0
 * makes and the host distributes -- or an existing ncclComm_t) together with the exchange's
 * own HIP stream and the sticky plan {pad, largest stream count} all ranks agree on. */
/* Verification status: with ONE rank the calls below run over RCCL on the GPU; with TWO ranks their
 * control flow (peer sizes, rank_base placement, the grouped send / receive loop, refusals and plan
 * overflows decided alike on every rank) has run over the tests' rehearsal transport -- two processes
 * on one card, host shared memory in place of RCCL (tests/test_gather_abi.py).  Over RCCL itself
 * more than one rank has not run yet: the build boxes have one GPU (a test gated on two devices is in
 * the suite). */
typedef struct flate_hip_comm flate_hip_comm;
#define FLATE_HIP_UNIQUE_ID_BYTES 128
#define FLATE_HIP_GATHER_ALLGATHER 0u /* payloads padded to `pad`, one ncclAllGather; rank r at out + r*pad */
#define FLATE_HIP_GATHER_SENDRECV 1u  /* exact sizes, grouped ncclSend/ncclRecv to all peers at once;
                                         shards back to back in rank order                          */
int flate_hip_comm_unique_id(uint8_t id[FLATE_HIP_UNIQUE_ID_BYTES]);
int flate_hip_comm_init(flate_hip_ctx *ctx, const uint8_t id[FLATE_HIP_UNIQUE_ID_BYTES], int rank,
                        int world, flate_hip_comm **comm);
/* An existing ncclComm_t (passed as void*, not owned) of the ctx's device. */
int flate_hip_comm_wrap(flate_hip_ctx *ctx, void *nccl_comm, int rank, int world, flate_hip_comm **comm);
void flate_hip_comm_destroy(flate_hip_comm *comm);
/* The plan: payload slot size of the padded form (a multiple of 1 MiB) and the largest per-rank
 * stream count.  It only grows.  set_plan must be given the same values on every rank. */
int flate_hip_comm_plan(flate_hip_comm *comm, uint64_t *pad, uint32_t *max_streams);
int flate_hip_comm_set_plan(flate_hip_comm *comm, uint64_t pad, uint32_t max_streams);
/* Host arithmetic of the layout alone (no GPU, no RCCL): pad = largest shard rounded up to
 * pad_to, rank_base[r] = where rank r's shard starts in out, *out_bytes = room out needs. */
int flate_hip_gather_layout(uint32_t world, const uint64_t *rank_bytes, uint64_t pad_to, uint32_t mode,
                            uint64_t *pad, uint64_t *rank_base, uint64_t *out_bytes);
/* Blocking exchange.  local (device, local_cap readable bytes) holds this rank's k streams back
 * to back, local_off[k+1] (host) their offsets (local_off[0] = 0) -- what
 * flate_hip_deflate_fast_batch returned.  On return out (device) holds every rank's shard and,
 * for the *total_streams streams of all ranks in rank-major order, stream j is
 * out[stream_off[j] .. + stream_len[j]) (host arrays of index_cap entries).  Every rank must
 * call with the same mode; FLATE_HIP_E_OUT_TOO_SMALL is returned on every rank if any rank's out
 * is too small (decided from gathered values: no rank is left waiting in a collective). */
int flate_hip_gather_compressed(flate_hip_comm *comm, const uint8_t *local, uint64_t local_cap,
                                const uint64_t *local_off, uint32_t k, uint8_t *out, uint64_t out_cap,
                                uint64_t *stream_off, uint64_t *stream_len, uint64_t index_cap,
                                uint64_t *total_streams, uint32_t mode);
/* Overlapped exchange (padded form, plan required: one blocking call or set_plan first).
 * begin returns at once: the exchange starts when the work queued so far on the ctx's stream
 * (the compression that wrote local) is done and runs on the communicator's own stream, beside
 * the next batch's compression.  local and out must stay untouched until end, which waits for
 * the exchange and fills the index; FLATE_HIP_E_AGAIN = a shard outgrew the pad or a rank holds more
 * streams than the plan's max_streams (both raised now, on every rank alike: the condition travels
 * through the exchange itself, no rank refuses alone).  begin's own refusals -- no plan
 * (FLATE_HIP_E_INVALID), out_cap < world * pad (FLATE_HIP_E_OUT_TOO_SMALL) -- depend only on the plan
 * and on out_cap, which the caller must keep EQUAL on all ranks: then they too are taken by every
 * rank or by none.  The metadata copies use pinned host memory of the communicator, so begin does not
 * wait for the compression queued in front of it (tests/test_gather_abi.py times that). */
int flate_hip_gather_begin(flate_hip_comm *comm, const uint8_t *local, uint64_t local_cap,
                           const uint64_t *local_off, uint32_t k, uint8_t *out, uint64_t out_cap);
int flate_hip_gather_end(flate_hip_comm *comm, uint64_t *stream_off, uint64_t *stream_len,
                         uint64_t index_cap, uint64_t *total_streams);

/* -- measurement ----------------------------------------------------------------
 * With profiling on, every kernel launch of the next call is bracketed by HIP
 * events on the launch stream; flate_hip_last_timing returns the per-stage
 * milliseconds of the last call (stage names via flate_hip_stage_name). */
#define FLATE_HIP_STAGE_LZ77 0
#define FLATE_HIP_STAGE_HUFF_PACK 1
#define FLATE_HIP_STAGE_CHECKSUM 2 /* flate_hip_checksum_batch; the checksum and frame kernels of the *_framed calls
                                      (flate_hip_inflate_batch_framed: output checksums + verdict) */
#define FLATE_HIP_STAGE_INFLATE 3
#define FLATE_HIP_STAGE_COUNT 4
int flate_hip_set_profiling(flate_hip_ctx *ctx, int on);
/* How the last encode call's persistent match-finder launch split its stream queue:
 * *resident_streams taken by the LDS-table blocks out of *queued_streams (the rest went to the
 * L2-table guest blocks); both 0 if the launch was not persistent.  With the option
 * "profile_split_streams" = K the split is fixed (first K queue entries to the LDS-table blocks)
 * instead of dynamic: a profiler that serialises the two kernels (rocprofv3 --pmc) then still
 * sees each of them do its share -- how profiles/r02/lz77_traffic.json was collected. */
int flate_hip_last_resident_share(flate_hip_ctx *ctx, uint32_t *resident_streams,
                                  uint32_t *queued_streams);
int flate_hip_last_timing(flate_hip_ctx *ctx, float *ms, int n);
const char *flate_hip_stage_name(int stage);

/* -- synthetic workloads (host side, no GPU needed) --------------------------------
 * Bit-reproducible generators for the benchmark inputs of BASELINE.md section 3.
 * Fills n_streams streams of stream_len bytes each, back to back, into out (host). */
#define FLATE_SYNTH_RAMP 0 /* byte[i] = i & 127 (deflate-fast_test.mbt:15-24) */
#define FLATE_SYNTH_TEXT 1 /* Zipf word text, the headline workload          */
#define FLATE_SYNTH_RAND 2 /* uniform random bytes                            */
#define FLATE_SYNTH_ZERO 3 /* all zero                                        */
int flate_hip_synth_fill(int kind, uint64_t seed, uint64_t first_stream,
                         uint32_t n_streams, uint64_t stream_len, uint8_t *out,
                         int nthreads);

#ifdef __cplusplus
}
#endif
#endif
