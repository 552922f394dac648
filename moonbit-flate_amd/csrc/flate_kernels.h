// flate_kernels.h -- kernel parameter blocks and launch entry points (internal).
#pragma once

#include "bgzf_parts_rule.h"
#include "chain_rule.h"
#include "flate_common.h"
#include "flate_hip.h"

namespace flate {

// A container's constants (RFC 1950 / RFC 1952), for the kernels of frame_kernels.hip and every host site.
// wrap: FLATE_HIP_WRAP_ZLIB / _GZIP.  The header as this library WRITES it (a member that is read may carry a longer
// gzip header: frame_parse_kernel); with_dict: zlib's FDICT + DICTID.
// kWrapBgzf: the members of a BGZF file (flate_hip_bgzf_write) -- gzip members with the 18-byte header that carries
// BSIZE, followed by the 28-byte EOF marker.  INTERNAL: the public *_framed calls refuse every wrap above _GZIP.
constexpr uint32_t kWrapBgzf = 3u;
// kWrapBgzfOpen: the same members WITHOUT the marker -- a part of a file that goes on (flate_hip_bgzf_writer_write, a
// call that is not final).  It differs from kWrapBgzf in nothing else.
constexpr uint32_t kWrapBgzfOpen = 4u;
FLATE_HD bool frame_is_bgzf(uint32_t wrap) { return wrap == kWrapBgzf || wrap == kWrapBgzfOpen; }
FLATE_HD uint32_t frame_header_len(uint32_t wrap, bool with_dict) {
  return frame_is_bgzf(wrap) ? 18u : wrap == FLATE_HIP_WRAP_GZIP ? 10u : (with_dict ? 6u : 2u);
}
FLATE_HD uint32_t frame_trailer_len(uint32_t wrap) { return (wrap == FLATE_HIP_WRAP_GZIP || frame_is_bgzf(wrap)) ? 8u : 4u; }
// the shortest member: the header without a dictionary, nothing, the trailer
FLATE_HD uint32_t frame_min_len(uint32_t wrap) { return frame_header_len(wrap, false) + frame_trailer_len(wrap); }
FLATE_HD uint32_t frame_sum_kind(uint32_t wrap) {
  return (wrap == FLATE_HIP_WRAP_GZIP || frame_is_bgzf(wrap)) ? (uint32_t)FLATE_HIP_CHECKSUM_CRC32
                                                            : (uint32_t)FLATE_HIP_CHECKSUM_ADLER32;
}

}  // namespace flate

#if defined(__HIPCC__)  // (what follows needs the HIP compiler; the constants above are also compiled as plain C++)
namespace flate {

// A stream is cut into LZ77 chunks as Compressor::enc_speed does (reference
// deflate.mbt:236-277): every full 65535-byte window plus a final partial window
// of >= 128 bytes.  chunk_base[i] .. chunk_base[i+1] are stream i's chunks; chunk c
// owns match records [c * kMatchCapPerChunk, (c+1) * kMatchCapPerChunk).
// device-side status words that the host turns into FLATE_HIP_E_INTERNAL with a message
// (a range of their own: no device-only word may alias a public FLATE_HIP_E_* code, which some status
// words are -- FLATE_HIP_E_OUT_TOO_SMALL from the scan kernels -- and which a caller may be handed raw;
// every value <= kStatusUqTimeout is an internal condition, the pack self-check's -(0x100000 + stream) too)
constexpr int kStatusUqTimeout = -0x1001;    // uq_pop: the unit with my ticket was never pushed
constexpr int kStatusGateTimeout = -0x1002;  // (retired with the overlapped entropy stage; the number stays reserved)
constexpr int kStatusBadIndex = -0x1003;     // an index outside the scratch it addresses (never expected)
constexpr int kStatusLanesLost = -0x1004;    // a persistent loop is running without all 64 lanes
constexpr int kStatusNoProgress = -0x1005;   // lz77_stream: a batch left the parser where it found it
static_assert(kStatusUqTimeout < -64 && kStatusNoProgress > -0x100000, "device-only status words: their own range");

struct LzParams {
  const uint8_t *in;
  const uint64_t *in_off;      // n_streams + 1
  const uint32_t *chunk_base;  // n_streams + 1
  const uint32_t *stream_ids;  // streams handled by this launch (or null = identity)
  const uint16_t *scan_off;    // probe offsets of the skip schedule
  int scan_len;
  uint2 *matches;          // {pos in chunk, token}
  uint32_t *chunk_nmatch;  // per chunk
  uint32_t *chunk_ntok;    // per chunk: literals + matches (DeflateFast::encode's token count)
  uint32_t compat_go;
  uint64_t *debug;  // diagnostic builds only (8 u64 per chunk), else null
  // guest kernel only
  void *gtables;        // one table per guest block
  uint32_t *queue;      // next index into stream_ids
  uint32_t queue_end;
  uint32_t gtable_blocks;  // tables behind `gtables` (a guest block beyond them does nothing)
  uint32_t spin_limit;     // polls before a bounded wait gives up
  uint32_t inject_drop_push;  // test hook (option debug_drop_window_push): drop that hand-over
  uint32_t inject_stall;      // test hook (option debug_stall_batch): that dense batch of every chunk undoes its progress
  // resumable single-stream launches (flate_hip_stream_write): the stream's first LZ77 window in this
  // launch has absolute index win0 (in / in_off then describe the stream through a virtual base:
  // in + absolute position is valid for the 32 KiB of history and the new bytes); 0 otherwise
  uint32_t win0;
  // measurement aid: the launch counts the streams it took from the queue here (null = off)
  uint32_t *taken;
  // Window-granular scheduling of multi-window streams (persistent MULTI launches): the unit of
  // work is one LZ77 window of one stream.  uq_ready[k] = (queue entry + 1) << 15 | window of the
  // k-th unit to run (0 = not pushed yet); uq_ctr = {head, tail}; the table of a stream between
  // two of its windows lives in uq_tables (32 KiB per queue entry), its sweep clock in uq_sweep.
  uint32_t *uq_ready;
  uint32_t *uq_ctr;
  uint32_t uq_units;
  uint16_t *uq_tables;
  uint32_t *uq_sweep;
  int *status;
};

// Preset dictionaries of a match-finder launch (the *_dict_kernel builds; flate_hip_deflate_fast_batch_dict).
// A slot is one USED dictionary: the last dict_len (17 .. 32768) bytes of it sit at dict_buf + dict_at[slot],
// followed by at least 16 readable bytes.  lz77_dict_prime_kernel leaves every slot's table and sweep clock in
// tables / clocks; the stream kernels start stream i from the snapshot of slot_of[i].
struct LzDictParams {
  const uint8_t *dict_buf;
  const uint64_t *dict_at;   // per slot
  const uint32_t *dict_len;  // per slot
  const uint32_t *slot_of;   // per stream of the batch (read for the streams of the launch only)
  uint16_t *tables;          // per slot: kTableSize slots
  uint32_t *clocks;          // per slot
};

// Entropy stage.  Blocks are the units enc_speed writes: every full 65535-byte window plus the
// tail (blk_base[i] .. blk_base[i+1] are stream i's blocks; the first chunk_base[i+1]-chunk_base[i]
// of them are LZ77 chunks).
struct HuffParams {
  const uint8_t *in;
  const uint64_t *in_off;
  const uint32_t *chunk_base;
  const uint32_t *blk_base;  // n_streams + 1
  const uint2 *matches;
  const uint32_t *chunk_nmatch;
  const uint32_t *chunk_ntok;
  uint32_t *blk_hist;  // per block 320 u32: literal/length histogram [0,286), offsets [288,318)
  uint32_t *blk_cl;    // per block 320 u32: (len << 16) | bit-reversed code, same layout
  uint32_t *blk_hdr;   // per block 704 u32: dynamic-header items (nbits << 16) | value
  uint8_t *tile_meta;  // input / 4 bytes: one byte per lane and 256-position tile, written by
                       // huff_hist_kernel and read by huff_pack_kernel (see TileTok::pack)
  uint4 *blk_meta;     // per block {kind 0 stored / 1 huffman-only / 2 dynamic, header items, start bit lo, hi}
  // spliced mode (one DEFLATE stream for the whole batch, splice_kernels.hip); 0/NULL otherwise
  uint32_t spliced;
  uint64_t *stream_sum;          // per stream {a, b}: written by huff_code_kernel
  const uint64_t *stream_bit;    // n_streams + 1: read by huff_pack_kernel
  uint64_t *out_len;   // exact compressed bytes per stream (huff_code_kernel)
  const uint64_t *out_off;  // exclusive scan of out_len
  uint8_t *out;
  int *status;
  uint32_t n_streams;
  uint32_t compat_go;
  const uint32_t *blk_sid;  // per-block launches (huff_*_block_kernel): stream of every block, else null
  uint32_t no_close;  // spliced mode: the batch's last stream does not write Writer::close's block
                      // (a stream that continues in a later call: flate_hip_stream_write)
  // grouped mode (huff_pack_grouped_kernel only; splice_rule.h): the streams are the pieces of SEVERAL spliced streams.
  // Piece i belongs to group piece_group[i]; the last piece of group g ends at bit group_end_bit[g] and writes the
  // group's closing block.  NULL otherwise.
  const uint32_t *piece_group;
  const uint64_t *group_end_bit;
};

struct CompactParams {
  const uint64_t *out_len;
  uint64_t *out_off;  // n_streams + 1 (device), exclusive scan of out_len
  uint64_t out_cap;
  uint32_t n_streams;
  int *status;  // set to FLATE_HIP_E_OUT_TOO_SMALL if the total exceeds out_cap
};

struct InfParams {
  const uint8_t *in;
  const uint64_t *in_off;   // n_streams + 1
  uint8_t *out;
  const uint64_t *out_off;  // n_streams + 1: slot of every stream's output (capacity)
  uint64_t *out_len;
  int32_t *status;
  int64_t *err_off;
  uint32_t n_streams;
  // spliced input (inflate_simt_kernel, inflate_spec_kernel): the n_streams pieces of ONE DEFLATE stream in[0, in_len);
  // piece i starts at bit bit_off[i] and ends where piece i+1 starts; the last one runs to BFINAL.
  // NULL: independent streams given by in_off.
  const uint64_t *bit_off;
  uint64_t in_len;
  // inflate_simt_kernel, spliced: nonzero = the pieces are a part of a longer stream (a round of
  // flate_hip_inflate_one): the last piece does not run to BFINAL, it ends at bit_off[n_streams] like the others
  uint32_t closed;
  // inflate_simt_kernel, spliced: pieces that are NOT consecutive in the stream (flate_hip_inflate_one_ranges: the
  // selected units): piece i ends at bit bit_end[i], or runs to BFINAL where that is ~0; bit_off then has n_streams
  // entries and `closed` is not read.  NULL: piece i ends where piece i+1 starts, `closed` as above.
  const uint64_t *bit_end;
  uint32_t size_only;  // inflate_kernel: decode and count, store nothing (FLATE_HIP_SIZE_ONLY)
  uint32_t *simt_lens; // inflate_simt_kernel: per-lane scratch of the header being parsed (inflate_simt_lens_bytes)
  uint32_t sid0;       // inflate_simt_kernel: first stream of this launch (a batch of several rounds)
  // preset dictionaries (the *_dict_kernel instantiations only): stream i's history starts with the
  // dict_len[i] (<= 32768, 0 = none) bytes at dict_buf + dict_at[i], the tail of its dictionary; every
  // tail is followed by at least 16 readable bytes.  Output byte k of the stream sits at history
  // position dict_len[i] + k.
  const uint8_t *dict_buf;
  const uint64_t *dict_at;
  const uint32_t *dict_len;
  // members of a container (flate_hip_inflate_batch_framed): stream i is in[in_off[i], in_end[i]) -- its trailer
  // follows, and the next stream's header.  NULL: stream i ends at in_off[i + 1].  Independent streams only.
  const uint64_t *in_end;
  // inflate_kernel, inflate_spec_kernel (what a size-only pass routes to): per stream, the bytes consumed from the
  // stream's first byte up to and including the byte that holds the last bit of the final block; meaningful when the
  // status is 0 (gzip member discovery: where the member's trailer starts).  NULL: not reported.
  uint64_t *used;
};

__global__ void lz77_serial_kernel(LzParams P);
// HOOKS: the build that carries the test hooks (inject_stall, inject_drop_push); see lz77_hooks_build, deflate_plan.h
template <bool MULTI, bool HOOKS>
__global__ void lz77_wave_kernel(LzParams P);
template <bool MULTI, bool HOOKS>
__global__ void lz77_guest_kernel(LzParams P);
// one stream continued from an earlier launch: table and sweep clock come from / go back to `table_io`,
// `clock_io`; runs the nwin windows from P.win0 on
// rebase != 0: every position the table and the clock hold is first moved down by that many bytes
// (the stream's origin was moved up: what shift_offsets does for the reference, deflate-fast.mbt:366-389)
// forget != 0: the first window of the launch starts on an empty table (shift_offsets with an empty
// `prev`, deflate-fast.mbt:367-374: what the reference does in its default compat mode)
__global__ void lz77_resume_kernel(LzParams P, uint16_t *table_io, uint32_t *clock_io, uint32_t nwin,
                                   uint32_t rebase, uint32_t forget);
// preset dictionaries: one block per slot primes its table; the stream kernels' dictionary builds (P.win0 = 1)
__global__ void lz77_dict_prime_kernel(LzParams P, LzDictParams DP);
template <bool HOOKS>
__global__ void lz77_wave_dict_kernel(LzParams P, LzDictParams DP);
template <bool HOOKS>
__global__ void lz77_guest_dict_kernel(LzParams P, LzDictParams DP);
__global__ void huff_hist_kernel(HuffParams P);
__global__ void huff_code_kernel(HuffParams P);
__global__ void huff_pack_kernel(HuffParams P);
// one wavefront per block instead of per stream (multi-window streams)
__global__ void huff_hist_block_kernel(HuffParams P);
__global__ void huff_zero_edges_kernel(HuffParams P, uint32_t n_blocks);
__global__ void huff_pack_block_kernel(HuffParams P);
__global__ void uq_init_kernel(uint32_t *ready, uint32_t *ctr, uint32_t n_streams, uint32_t n_units);
__global__ void scan_sizes_kernel(CompactParams P);
// small index arrays between pinned host staging and the device (see compact_kernels.hip)
__global__ void copy_ctl_kernel(uint32_t *dst, const uint32_t *src, size_t nwords);
__global__ void inflate_kernel(InfParams P);
// the same decoders with preset dictionaries (InfParams::dict_*): the no-dictionary kernels keep their code
__global__ void inflate_dict_kernel(InfParams P);
// one wavefront per stream, 64 sub-blocks of the bit stream decoded at once (inflate_spec_kernel.inc):
// <bits per sub-block, tokens per list, bytes of history ring>
template <int SUB, int CAP, int RING>
__global__ void inflate_spec_kernel(InfParams P);
template <int SUB, int CAP, int RING>
__global__ void inflate_spec_dict_kernel(InfParams P);
#ifndef FLATE_SPEC_SMALL
#define FLATE_SPEC_SMALL 288, 61, 8192  // batches up to one wavefront per SIMD (31.4 KiB of LDS)
#endif
#ifndef FLATE_SPEC_LARGE
#define FLATE_SPEC_LARGE 224, 47, 512  // 19.9 KiB of LDS: two wavefronts per SIMD
#endif
template <int LPW, int ROWD>  // ROWD: dwords of the lane's output row (0 = none), see inflate_kernels.hip
__global__ void inflate_simt_kernel(InfParams P);
template <int LPW, int ROWD>
__global__ void inflate_simt_dict_kernel(InfParams P);
// one long stream decoded in pieces (inflate_stream_kernel.inc): the decoder's state -- the 32 KiB
// window, the tables of the block in progress, the bit carry, a copy that did not fit -- rests in
// `state` (inflate_stream_state_bytes()) between launches; its first 64 bytes are InfStreamResult
struct InfStreamResult {
  uint64_t total_in, total_out;
  int64_t err_off;
  int32_t status;  // 0 = call again, 1 = the final block is done, < 0 = error (sticky)
  uint32_t in_used, out_len, bit_in_byte;
};
size_t inflate_stream_state_bytes();
__global__ void inflate_stream_init_kernel(void *state, const uint8_t *dict, uint32_t dict_len);
__global__ void inflate_stream_kernel(void *state, const uint8_t *in, uint32_t in_len, uint32_t final_in,
                                      uint8_t *out, uint32_t out_cap);

// splice (splice_kernels.hip): bit positions of the streams inside one spliced DEFLATE stream
struct SpliceParams {
  const uint64_t *sum;    // per stream {a, b} written by huff_code_kernel (see splice_kernels.hip)
  uint64_t *stream_bit;   // n_streams + 1
  uint64_t *total_bytes;  // size of the spliced stream
  uint64_t out_cap;
  int *status;            // -2 if total_bytes > out_cap
  uint32_t n_streams;
  uint64_t start_bit;     // bit position of the first stream's first block (0; a continued stream: its carry)
  uint32_t no_close;      // no closing block behind the last stream: total_bytes = ceil(end bit / 8)
};
__global__ void splice_scan_kernel(SpliceParams P);
__global__ void splice_zero_kernel(SpliceParams P, uint8_t *out);

// grouped splice (splice_kernels.hip, splice_rule.h; flate_hip_deflate_fast_grouped_framed): SEVERAL spliced streams
// in one output, group g = the pieces [group_off[g], group_off[g + 1]) inside header_len bytes in front and
// trailer_len bytes behind.  Every position is absolute: bits (bytes) counted from out[0].
struct ZipWriteHead;  // (zip_kernels.h)
struct GroupParams {
  const uint64_t *sum;          // per piece {a, b} written by huff_code_kernel
  const uint32_t *group_off;    // n_groups + 1
  const uint32_t *piece_group;  // per piece: its group
  const uint32_t *header_len;   // per group; null: header_len_all for every group
  uint32_t header_len_all;
  uint32_t trailer_len;
  uint64_t *stream_bit;         // n_pieces + 1: piece i's first block (entry n_pieces: 8 * total)
  uint64_t *end_bit;            // per group: where its last piece ends and its closing block starts
  uint64_t *payload_off;        // per group: the first byte of its raw stream
  uint64_t *member_off;         // n_groups + 1: payload_off[g] - header length; entry n_groups: the total
  uint64_t *bit_idx;            // n_pieces + n_groups, or null: group g's index at [group_off[g] + g, group_off[g + 1] + g],
                                // counted from the first byte of its raw stream
  uint64_t *total_bytes;
  uint64_t out_cap;
  uint32_t slack;               // bytes behind the total that must fit as well (3 where nothing follows the last
                                // closing block: the pack kernel stores whole dwords)
  int *status;                  // -2 if total + slack > out_cap
  uint32_t n_pieces, n_groups;
  // the members of a ZIP archive (flate_hip_zip_write with "zip_piece_bytes"; header_len[g] = 30 + name length): the
  // scan also produces zip_scan_kernel's result words -- k0, the directory's place and size, the archive's total, which
  // is then what is judged against out_cap -- and refuses a raw stream of 2^32 bytes or more (FLATE_HIP_E_TOO_LARGE).
  // zip_name_off: n_groups + 1, DEVICE.  NULL otherwise.
  ZipWriteHead *zip_head;
  const uint64_t *zip_name_off;
};
__global__ void group_scan_kernel(GroupParams P);
__global__ void group_zero_kernel(GroupParams P, uint8_t *out);
// huff_pack_kernel over the pieces of a grouped call (HuffParams::piece_group)
__global__ void huff_pack_grouped_kernel(HuffParams P);

// headers and trailers of the groups' members, one thread per group, behind the pack kernel (frame_kernels.hip)
struct GroupFrameParams {
  const uint64_t *member_off;   // n_groups + 1 (group_scan_kernel)
  const uint64_t *payload_off;  // per group
  const uint64_t *end_bit;      // per group
  const uint32_t *group_off;    // n_groups + 1
  const uint64_t *in_off;       // n_pieces + 1: the pieces' input (gzip: ISIZE of the group's contiguous input)
  const uint32_t *sums;         // per group: the checksum of its input
  uint8_t *out;
  uint64_t out_cap;
  uint32_t n_groups;
  uint32_t wrap;                // FLATE_HIP_WRAP_ZLIB / _GZIP
  const int *status;
};
__global__ void group_frame_write_kernel(GroupFrameParams P);

// Containers around the raw streams (frame_kernels.hip; flate_hip_deflate_fast_*_framed): member i of a batch is
// header | raw stream i | trailer, the members back to back.  wrap = FLATE_HIP_WRAP_ZLIB: two header bytes, or six
// (FDICT + DICTID) for a stream that names a dictionary, and the Adler-32 of the input, big endian; _GZIP: ten
// header bytes, the CRC-32 and the input's length mod 2^32, little endian.
struct FrameParams {
  const uint64_t *out_len;  // per stream: bytes of its raw stream (huff_code_kernel)
  uint64_t *member_off;     // n_streams + 1: where every member starts (frame_scan_kernel writes it); null: ONE member
                            // at out[0] whose raw stream has out_len[0] bytes (the spliced form)
  uint64_t *payload_off;    // n_streams + 1: member_off[i] + header length = HuffParams::out_off (frame_scan_kernel)
  const uint64_t *in_off;   // n_streams + 1: the streams' input (gzip: ISIZE); one member: unused
  uint64_t one_len;         // one member: bytes of its input
  const uint32_t *sums;     // per member: the checksum of its input
  const uint32_t *dict_of;  // per stream: its dictionary or FLATE_HIP_NO_DICT; null: no member carries a DICTID
  const uint32_t *dict_id;  // per dictionary: its Adler-32
  uint8_t *out;             // any byte alignment
  uint64_t out_cap;
  uint32_t n_streams;
  uint32_t wrap;
  int *status;              // frame_scan_kernel: FLATE_HIP_E_OUT_TOO_SMALL if the members exceed out_cap; kWrapBgzf:
                            // FLATE_HIP_E_TOO_LARGE if a member exceeds 65536 bytes, status[1] = the first such block
};
// scan_sizes_kernel for members: exclusive scan of header + out_len + trailer
__global__ void frame_scan_kernel(FrameParams P);
// headers and trailers, byte by byte (one thread per member); launched AFTER the pack kernel, whose spliced form
// stores whole dwords around its stream
__global__ void frame_write_kernel(FrameParams P);

// Reading members (flate_hip_inflate_batch_framed): member i = in[in_off[i], in_off[i + 1]) = header | raw stream |
// trailer.  frame_parse_kernel (one thread per member) checks the header, finds the raw stream -- pay_off / pay_end:
// what the decoders read as InfParams::in_off / in_end --, reads the trailer and, for a zlib member with FDICT, looks
// its DICTID up among dict_id (the first match) and hands the decoders that dictionary's staged tail.  A bad member
// gets an empty raw stream.  frame_verdict_kernel (one thread per member, behind the decoder and the sums of what it
// produced) merges header verdict, decoder status, checksum and ISIZE into status / err_off / out_len.
struct FrameReadParams {
  const uint8_t *in;
  const uint64_t *in_off;   // n_streams + 1: the members
  const uint64_t *in_end;   // per member: where it ends; null (the public call): member i ends at in_off[i + 1].  Members
                            // that are NOT consecutive in `in` (flate_hip_bgzf_read_ranges: the touched ones of a file)
  uint32_t n_streams;
  uint32_t wrap;            // FLATE_HIP_WRAP_ZLIB / _GZIP
  const uint32_t *dict_id;  // per dictionary: the Adler-32 of the whole of it (n_dicts == 0: unused)
  uint32_t n_dicts;
  const uint64_t *tail_at;  // per dictionary: where its tail lies in InfParams::dict_buf ...
  const uint32_t *tail_len; // ... and its length (0: an empty dictionary)
  uint64_t *pay_off;        // n_streams + 1 (entry n_streams: in_off[n_streams])
  uint64_t *pay_end;        // per member
  uint32_t *want;           // per member: the trailer's checksum
  uint32_t *isize;          // per member: gzip's ISIZE
  uint32_t *bad;            // per member: 1 = bad header
  uint32_t *dict_used;      // per member: its dictionary or FLATE_HIP_NO_DICT
  uint64_t *dict_at;        // per member: InfParams::dict_at / dict_len (null when n_dicts == 0)
  uint32_t *dict_len;
  // frame_verdict_kernel
  const uint32_t *sums;     // per member: the checksum of what it produced; null: nothing was stored (FLATE_HIP_SIZE_ONLY)
  uint64_t *out_len;
  int32_t *status;
  int64_t *err_off;
};
__global__ void frame_parse_kernel(FrameReadParams P);
__global__ void frame_verdict_kernel(FrameReadParams P);

// Reading ONE member whose raw stream is spliced (flate_hip_inflate_spliced_framed): in[0, in_len) = header | the
// n_pieces pieces of one DEFLATE stream | trailer, the index counted from the raw stream's first byte.
// frame_parse_kernel runs over the one range {0, in_len} and fills a FrameOne; frame_rebase_kernel (one thread per
// index entry) then moves the index to the member's first byte -- bit_in[i] + 8 * header length, never beyond the
// raw stream's end: a piece that would start behind it gets no input (the decoders compute in_len - start unsigned)
// -- so that the spliced decoders run unchanged on InfParams::in = the member, in_len = raw_end.  Whole bytes are
// added: the bit alignment that stored blocks need is kept.  A bad header collapses every piece to the empty range
// at raw_end.  frame_verdict_spliced_kernel (one workgroup, behind the decoder, the pieces' sums and their join)
// applies the three cases of flate_hip.h to every piece and writes the member's two words.
struct FrameOne {
  uint64_t in_off[2];       // {0, in_len}: uploaded
  uint64_t pay_off[2];      // frame_parse_kernel: [0] = the header's length
  uint64_t pay_end;
  uint64_t total;           // checksum_join_kernel: bytes of the concatenation
  int64_t member_err_off;   // frame_verdict_spliced_kernel
  uint32_t want, isize, bad, dict_used;  // frame_parse_kernel
  uint32_t sum;             // checksum_join_kernel
  int32_t member_status;    // frame_verdict_spliced_kernel
  uint32_t b0;              // one_part_init_kernel (a stream read in parts): the first unit starts at this bit of the raw
                            // range's first byte; 0 everywhere else (one_init_kernel, gzfile_init_kernel)
};
struct FrameSplicedParams {
  FrameOne *one;
  const uint64_t *bit_in;   // n_pieces + 1: counted from the raw stream's first byte
  uint64_t *bit_out;        // n_pieces + 1: counted from the member's first byte (InfParams::bit_off)
  uint32_t *piece_bad;      // per piece: the member's header verdict (checksum_device_clipped's d_bad)
  uint32_t n_pieces;
  uint32_t wrap;
  uint64_t in_len;          // the member's bytes
  uint64_t raw_end;         // in_len - trailer length
  // frame_verdict_spliced_kernel
  uint64_t *out_len;
  int32_t *status;
  int64_t *err_off;
};
__global__ void frame_rebase_kernel(FrameSplicedParams P);
__global__ void frame_verdict_spliced_kernel(FrameSplicedParams P);

// THE DISCOVERY SKELETON (chain_walk.h, chain_rule.h, chain_kernels.hip), shared by the four formats below.  Every
// offset of the input that passes a format's rule is a CANDIDATE; the candidates are compacted in file order (count per
// 4 KiB tile, chain_scan_kernel, fill), every candidate finds the one at its own end by binary search (the end of the
// file: the terminal node n_cand; nothing there: the dead node n_cand + 1; both absorb), and the chain from candidate 0
// is ranked by pointer doubling (chain_round_kernel).  All loops are bounded by values the host computed before the
// launches; no kernel waits for another workgroup.
struct BgzfHead {          // the result words, read back as one block
  uint64_t out_bytes;      // sum of the members' ISIZE (0 unless rc == 0)
  int64_t err_off;         // the offset at which no member could be read, or -1
  uint32_t n_members;      // well-formed members from offset 0
  int32_t rc;              // 0 or FLATE_HIP_E_CORRUPT
  uint32_t eof_marker;     // the last member is the canonical 28 bytes
  uint32_t n_cand;         // candidates counted (saturating); above cap: nothing else here is valid, run again
};
struct ChainParams {       // what the shared code reads
  const uint8_t *in;       // any byte alignment
  uint64_t in_len;
  uint32_t n_tiles;        // 4 KiB tiles on the 16-byte grid of in's ADDRESS
  uint32_t cap;            // candidates the arrays hold
  uint32_t path_len;       // a power of two >= cap + 2
  uint32_t *tile_cnt;      // n_tiles + 1: candidates per tile, then their exclusive scan
  uint64_t *cand_off;      // cap: where the candidates start
  uint32_t *jump[2];       // cap + 2 each: the successor after 2^j steps, double-buffered
  uint32_t *path;          // path_len: node r steps from candidate 0
  uint64_t *member_off;    // cap + 1: where the chain's members start
  uint64_t *out_off;       // cap + 1: where their output goes
  BgzfHead *head;
};
__global__ void chain_scan_kernel(ChainParams C);
__global__ void chain_round_kernel(ChainParams C, uint32_t j);

// BGZF member discovery (bgzf_kernels.hip; flate_hip_bgzf_index / _read): the members of a file form a linked list
// through their BSIZE fields; a candidate is an offset that passes the member rule (bgzf_rule.h), and it ends at
// offset + total.  ZIP's directory is linked by the same kernel (zip_kernels.h).
struct BgzfParams {
  ChainParams C;
  uint32_t *cand_total;    // cap
  uint32_t *isize;         // cap: per member
};
__global__ void bgzf_count_kernel(BgzfParams P);
__global__ void bgzf_fill_kernel(BgzfParams P);
__global__ void bgzf_link_kernel(BgzfParams P);
__global__ void bgzf_finish_kernel(BgzfParams P);
__global__ void bgzf_out_scan_kernel(BgzfParams P);

// A PART of a BGZF file (bgzf_parts_kernels.hip; flate_hip_bgzf_reader_read): the count, scan, fill, link and round
// kernels above over the part, then the part's own finish (THE PART STOP of bgzf_parts_rule.h where the chain's
// successor is the dead node) and out-scan (the ISIZE scan, DELIVERY, the result words, the FILE-absolute index).
struct BgzfPartParams {
  BgzfParams B;
  BgzfPartFound *found;      // the result words, read back as one block
  uint64_t out_cap;
  uint64_t base_in;          // the part's file offset ...
  uint64_t base_out;         // ... and the output bytes in front of it
  uint64_t *idx_member_off;  // cap + 1: base_in + member_off
  uint64_t *idx_out_off;     // cap + 1: base_out + out_off
  uint32_t k_max;            // bgzf_part_k_max
  uint32_t final_in;
};
__global__ void bgzf_part_finish_kernel(BgzfPartParams Q);
__global__ void bgzf_part_out_scan_kernel(BgzfPartParams Q);

// BGZF random access (bgzf_range_kernels.hip; flate_hip_bgzf_read_ranges): behind the discovery kernels, on the index
// where they left it.  Locate: one thread per range (bgzf_range_rule.h) -- b, length, status, the first and the last
// member with bytes inside it -- and +1 / -1 into a difference array over the members.  Select: its scan says which
// members some range covers; masked with ISIZE > 0, one scan of (1, ISIZE) gives every selected member its rank and its
// place in the dense scratch, and the members are compacted in file order.  Layout: the scan of the ranges' lengths
// (their places in `out`), and where every range's ONE run starts in the scratch.  Gather: the runs into `out`.
struct BgzfRangeHead {     // the result words, read back in front of the arrays
  uint64_t out_total;      // bytes of all ranges
  uint64_t scratch_total;  // bytes of all selected members
  uint32_t n_sel;          // selected (touched) members
  uint32_t any_invalid;    // some range had an invalid end point
};
struct BgzfSel {           // one selected member, in file order
  uint64_t in_off, in_end; // its bytes in the file
  uint64_t scratch_off;    // where its output goes in the dense scratch
  uint32_t member;         // its index in the file
  uint32_t isize;
};
struct BgzfRangeParams {
  // the index (BgzfParams), n = head->n_members of a well-formed chain
  const uint64_t *member_off;
  const uint64_t *out_off_m;
  const uint32_t *isize;
  uint32_t n_members;
  uint32_t n_ranges;
  uint32_t pos_kind;
  const uint64_t *begin;   // n_ranges each (device copies of the caller's arrays)
  const uint64_t *end;
  int32_t *diff;           // n_members + 1, zeroed: +1 at a range's first member, -1 behind its last
  uint32_t *rank;          // n_members: selected members in front of member k
  uint64_t *scratch_at;    // n_members: selected bytes in front of member k
  // per range
  uint64_t *r_b;           // locate: where it starts in U
  uint64_t *r_len;         // locate: its length
  uint32_t *r_first;       // locate: its first / last member, or kBgzfNoMember
  uint32_t *r_last;
  uint64_t *r_src;         // layout: where its run starts in the scratch
  // what the host reads back, one block: head | r_out_off (n_ranges + 1) | r_status | r_rank_lo | r_rank_hi | sel
  BgzfRangeHead *head;
  uint64_t *r_out_off;
  int32_t *r_status;
  uint32_t *r_rank_lo;     // the selected members [r_rank_lo, r_rank_hi) are the ones the range touches
  uint32_t *r_rank_hi;
  BgzfSel *sel;            // n_members entries of room, head->n_sel used
};
__global__ void bgzf_range_locate_kernel(BgzfRangeParams P);
__global__ void bgzf_range_select_kernel(BgzfRangeParams P);
__global__ void bgzf_range_layout_kernel(BgzfRangeParams P);
// The gather: range r's run scratch[r_src[r], + len) -> out[r_out_off[r], + len), both sides at any byte alignment.
// Work is cut by COST = bytes + kBgzfGatherRangeCost per range: workgroup j owns the cost window [j, j + 1) *
// kBgzfGatherWindow, so one huge range fills the chip in 64 KiB pieces and many tiny ranges share a workgroup.  The
// scratch must be a 16-byte aligned allocation with 32 readable bytes behind its last run.
struct BgzfGatherParams {
  const uint8_t *scratch;
  uint8_t *out;
  const uint64_t *r_out_off;  // n_ranges + 1
  const uint64_t *r_src;      // n_ranges
  uint32_t n_ranges;
};
constexpr uint32_t kBgzfGatherWindow = 65536;
constexpr uint32_t kBgzfGatherRangeCost = 256;
__global__ void bgzf_gather_kernel(BgzfGatherParams P);

// Plain multi-member gzip files (gzip_kernels.hip; flate_hip_gzip_index / _read): the skeleton for members that do not
// carry their size.  A candidate is an offset that passes the header rule (gzip_rule.h) over the range it is given --
// in[p, min(in_len, p + member_max)); frame_parse_kernel and ONE size-only launch of the batch decoders run over all
// candidates (InfParams::used) between the fill and the link, and a candidate ends behind its trailer -- or, when its
// decode failed, nowhere: the dead node.  gzip_finish_kernel and gzip_out_scan_kernel turn the ranks into member_off /
// out_off and the walk's verdict (gzip_serial_walk).  C.cap is the exact candidate count: the host reads it back
// behind the scan.
struct GzipParams {
  ChainParams C;
  uint64_t member_max;     // option "gzip_member_max"
  uint64_t *cand_end;      // cap: where candidate c's range ends; C.cand_off has cap + 1 entries (the last: in_len)
  // what frame_parse_kernel and the decoders left, per candidate
  const uint64_t *pay_off; // where the raw stream starts
  const uint32_t *bad;     // (never 1: the candidates passed the same rule)
  const int32_t *status;
  const uint64_t *out_len;
  const uint64_t *used;
  uint64_t *msize;         // cap: per member of the chain, what it inflates to
};
__global__ void gzip_count_kernel(GzipParams P);
__global__ void gzip_fill_kernel(GzipParams P);
__global__ void gzip_link_kernel(GzipParams P);
__global__ void gzip_finish_kernel(GzipParams P);
__global__ void gzip_out_scan_kernel(GzipParams P);

// One long DEFLATE stream (one_kernels.hip, one_probe_kernel.inc; flate_hip_inflate_one_index): the skeleton one level
// down.  A candidate is bit 0 of the raw stream or a bit offset that passes the dynamic-header rule
// (deflate_block_rule.h); one_probe_kernel decodes every candidate without history or stores up to the next dynamic
// header (OneProbe) between the fill and the link, and a candidate ends at that header's bit (a final block: the
// terminal node; a failed probe: the dead node).  one_finish_kernel and one_out_scan_kernel turn the ranks into
// unit_bit / out_off; a chain that stops at a dynamic header the rule refused takes its verdict from one more probe
// there (one_probe_kernel, tail form).  C.in is the whole input, C.cand_off the candidates' bits, C.member_off the
// units' bits (both counted from the raw stream's first byte).  C.cap is the exact candidate count.
// With OneParams::stored_units (option "one_stored_units") read "dynamic or stored header" for "dynamic header"
// throughout: the stored-header rule adds candidates, and the walk stops in front of a stored header too.
struct OneProbe {          // what a candidate's probe left
  uint64_t end_bit;        // where it stopped: in front of a dynamic header, or behind the final block
  uint64_t out;            // bytes it inflates to
  int64_t err_off;         // counted from the raw stream's first byte, or -1
  int32_t status;          // 0, FLATE_HIP_E_CORRUPT / _UNEXPECTED_EOF / _TOO_LARGE
  uint32_t final_block;    // it ended with BFINAL
};
struct OneHead {           // the result words, read back as one block; C.head = &h
  BgzfHead h;              // n_members: the units; rc / err_off: the serial decoder's verdict
  uint64_t tail_bit;       // tail != 0: the chain stopped here, at a dynamic header that is no candidate
  uint32_t tail;
  uint32_t bad;            // the container's header verdict (frame_parse_kernel)
  uint64_t raw_off, raw_len;  // the raw stream inside the input
  uint64_t prefix_bytes;   // what the good units inflate to (out_off[n_members]), of a stream that fails too
  uint64_t fail_out;       // a unit that fails behind its header: the bytes it produced in front of the failure
  uint32_t fail_unit;      // ... and 1: that unit is decoded too, so that those bytes are delivered
  uint32_t pad;
};
struct OneParams {
  ChainParams C;
  FrameOne *one;           // one_init_kernel, frame_parse_kernel: pay_off[0] .. pay_end is the raw stream
  OneHead *head;
  OneProbe *probe;         // cap
  uint64_t *usize;         // cap: per unit of the chain, what it inflates to
  uint64_t unit_max;       // option "one_unit_max": a unit's input spans fewer bytes than this
  uint32_t stored_units;   // option "one_stored_units": 1 = a stored header starts a unit too: the host launches the
                           // <true> builds of FIND and PROBE
};
// The decode of the units (flate_hip_inflate_one), in rounds of `count` units from unit u0.  one_tail_kernel (TAIL)
// decodes every unit of the round with a SYMBOLIC window (window_compose.h) and stores its tail function into F[0];
// one_compose_kernel scans the functions over the round (Hillis-Steele, ceil(log2(count)) launches between F[0] and
// F[1]); one_resolve_kernel turns them into the byte windows R[1 .. count] from the seed R[0]; one_pieces_kernel
// writes the round as spliced pieces with dictionaries (InfParams: bit_off = unit_bit + u0, dict = R[i], dict_len =
// min(32768, out_off[k]), slot = out + out_off[k]) and the lane-per-stream dictionary decoder (DECODE) decodes them
// straight into the output; one_check_kernel holds what it reports against the discovery.  TAIL and DECODE apply the
// distance rule of the serial decoder (history = min(32768, out_off[k] + bytes produced)): the first unit that fails
// is dh->first_bad; its slot ends at the failure and the units behind it get an empty slot (nothing is written).
struct OneDecHead {        // the call's result words
  uint64_t out_len;
  int64_t err_off;
  int32_t status;
  uint32_t first_bad;      // 0xffffffff: none
  uint32_t decode_bad;     // 0xffffffff: none; else a good unit DECODE did not decode as TAIL did (E_INTERNAL)
  uint32_t pad;
};
struct OneDecParams {
  const uint8_t *in;
  const FrameOne *one;
  const uint64_t *unit_bit;  // n_dec + 1 (OneParams::C.member_off)
  const uint64_t *out_off;   // n_dec + 1
  uint32_t u0, count;
  // one_tail_kernel: the round's units are unit_list[u0 .. u0 + count) -- not consecutive in the stream
  // (flate_hip_inflate_one_ranges) -- every one of them is walked, and status / err_off / produced are indexed by the
  // place in the list.  NULL: the units u0 .. u0 + count - 1.
  const uint32_t *unit_list;
  uint64_t total;            // nothing at or behind out + total is written
  uint64_t unit_max;
  uint16_t *F[2];            // count * 32768 entries each
  uint8_t *R;                // (count + 1) * 32768 bytes: R[i] = the window in front of unit u0 + i
  OneDecHead *dh;
  int32_t *status;           // per unit (TAIL)
  int64_t *err_off;
  uint64_t *produced;
  // the round's pieces (one_pieces_kernel -> InfParams) and what DECODE reports for them (one_check_kernel)
  uint64_t *p_out_off;       // count + 1: piece i's slot is [p_out_off[i], p_out_off[i + 1]) of the output
  uint64_t *p_dict_at;       // count: where in R piece i's dict_len bytes of history start
  uint32_t *p_dict_len;      // count
  const int32_t *d_status;   // count
  const uint64_t *d_out_len; // count
  // one_verdict_kernel
  const OneHead *head;
  const uint32_t *sum;       // the checksum of out[0, total), or null
  uint32_t wrap;
  // TAIL's unit rule, the word that goes with unit_max: what the units were cut by (OneParams::stored_units, or a seek
  // index's rule word); the host launches that build of one_tail_kernel.  (It stands in the padding behind `wrap`: no
  // other field moves, so the default build's parameter loads are the ones it had.)
  uint32_t stored_units;
  uint64_t in_len;
  // one_pieces_kernel: bytes of history in front of out_off[0], at most 32768 -- what a stream read in parts produced
  // before this part (the handle's window holds them); 0 in every other call
  uint64_t hist_base;
};
template <bool STORED>  // (the unit rule of D.stored_units; both builds: one_probe_kernel.inc)
__global__ void one_tail_kernel(OneDecParams D);
__global__ void one_pieces_kernel(OneDecParams D);
__global__ void one_check_kernel(OneDecParams D);
__global__ void one_compose_kernel(const uint16_t *src, uint16_t *dst, uint32_t count, uint32_t s);
__global__ void one_resolve_kernel(const uint16_t *F, uint8_t *R, uint32_t count);
__global__ void one_verdict_kernel(OneDecParams D);
__global__ void one_init_kernel(FrameOne *one, uint64_t in_len);
// (STORED: the unit rule, one_find_kernel.inc -- <false>, dynamic headers alone, is instantiated in one_kernels.hip;
// <true>, dynamic and stored headers, in one_stored_kernels.hip.  PARTS: the root of the chain is bit FrameOne::b0 of
// the raw range's first byte, not bit 0 -- a stream read in parts; both unit rules in one_parts_kernels.hip)
template <bool STORED, bool PARTS = false>
__global__ void one_count_kernel(OneParams P);
template <bool STORED, bool PARTS = false>
__global__ void one_fill_kernel(OneParams P);
template <bool STORED>  // (the unit rule of P.stored_units; both builds: one_probe_kernel.inc)
__global__ void one_probe_kernel(OneParams P, uint32_t tail);
__global__ void one_link_kernel(OneParams P);
__global__ void one_finish_kernel(OneParams P);
__global__ void one_out_scan_kernel(OneParams P);

// ONE stream read in PARTS (flate_hip_one_reader_*; one_parts_kernels.hip; the rule: one_parts_rule.h).  A call is the
// discovery and the rounds above over one part of the stream, between three small kernels of its own:
//   one_part_init_kernel   in one_init_kernel's and frame_parse_kernel's place: the part's raw range (the header on the
//                          first part only, with the rule's third answer in FrameOne::bad; the trailer cut off on a
//                          final part only) and b0
//   one_part_link_kernel   one_link_kernel with the chain's root at candidate 0 = bit b0 (FIND's PARTS build masks the
//                          bits in front of it out of that byte)
//   one_part_hist_kernel   TAIL's offsets: out_off[k] + hist_base, so that the distance rule sees what the STREAM has
//                          produced (unit_rounds: tail_out_off)
//   one_part_carry_kernel  behind the rounds: the part's verdict words (one_verdict_kernel's cases without the trailer)
//                          and the two pieces of the checksum join -- the running sum over produced_before bytes, the
//                          part's over its own
//   one_part_verdict_kernel  behind the join: the joined sum becomes the running one, and -- trailer != null -- it and
//                          the total length are held against the trailer's words
// The window behind the last delivered unit, R[count] of the last round, goes into OnePartState::window by a copy on
// the stream, as the round driver's own carry does.
struct OnePartState {        // per handle, in device memory
  uint8_t window[32768];     // the 32 KiB in front of the next unit (zeros in front of the stream)
  uint64_t slot_off[3];      // checksum_join_device: {0, produced_before, produced_before + out_len}
  uint64_t produced[2];      // ... {produced_before, out_len}
  uint64_t total;            // ... its length word
  uint32_t sums[2];          // the running sum, the part's
  uint32_t joined;
  uint32_t trailer_bad;      // res.status is a trailer mismatch (err_off is counted from the member's first byte)
  OneDecHead res;            // the call's result words, read back
};
struct OnePartParams {
  OnePartState *st;
  uint64_t produced_before;
  uint64_t total;            // bytes the call delivers if nothing fails
  int32_t term_rc;           // the discovery's verdict when the call delivers everything in front of it, else 0
  uint32_t wrap;
  int64_t term_err_off;
  const uint8_t *trailer;    // the trailer's bytes when this call judges it, or null
  uint64_t member_len;       // ... and the member's length with it: err_off of a mismatch
};
__global__ void one_part_init_kernel(FrameOne *one, const uint8_t *in, uint64_t in_len, uint32_t wrap, uint32_t first,
                                     uint32_t final_in, uint32_t b0);
__global__ void one_part_link_kernel(OneParams P);
__global__ void one_part_hist_kernel(const uint64_t *out_off, uint64_t *tail_off, uint32_t n, uint64_t hist_base);
__global__ void one_part_carry_kernel(OnePartParams Q, OneDecParams D);
__global__ void one_part_verdict_kernel(OnePartParams Q);

// ONE stream written in PARTS (flate_hip_one_writer_*; one_writer_kernels.hip; the rule: one_writer_rule.h).  A call is
// the whole call's match finder and entropy stage over the pieces it consumes, the scan started at the carried bit
// (SpliceParams::start_bit) and closed only by a final call (no_close), between four small kernels of its own:
//   one_writer_begin_kernel   behind splice_zero_kernel, in front of the pack kernel: the header, or the carried bits
//   one_writer_index_kernel   the scan's positions as bits of the raw stream
//   one_writer_commit_kernel  behind the pack kernel and the part's checksum: room, closing block of a call without
//                             pieces, trailer, the checksum join, the new carry, the result words
//   one_writer_copy_kernel    device callers: the handle's buffer to `out`, the length read on the device
struct OneWriterResult {     // the call's result words, read back
  int32_t status;            // FLATE_HIP_OK, FLATE_HIP_STREAM_END, FLATE_HIP_E_OUT_TOO_SMALL (out_len: the bytes needed),
                             // or the encoder's status word
  uint32_t n_pieces;
  uint64_t out_len;
  uint64_t end_bit;          // of the raw stream: where the next piece, or the closing block, starts
};
struct OneWriterState {      // per handle, in device memory; written by one_writer_commit_kernel alone
  uint64_t emitted;          // bytes of the member delivered so far
  uint64_t total_in;         // bytes of input consumed so far
  uint32_t sum;              // their checksum
  uint32_t carry;            // the last, incomplete byte ...
  uint32_t carry_bits;       // ... and how many of its bits count (0..7)
  uint32_t part_sum;         // the checksum of the call's input (checksum_device)
  OneWriterResult res;
};
struct OneWriterParams {
  OneWriterState *st;
  uint8_t *buf;               // the handle's buffer: the call's bytes from byte 0
  const uint64_t *stream_bit; // n_pieces + 1: splice_scan_kernel's positions in buf (not read when n_pieces == 0)
  uint64_t *bit_idx;          // n_pieces + 1: the same as bits of the raw stream
  const int *status;          // the encoder's status word
  uint64_t start_bit;         // SpliceParams::start_bit
  uint64_t in_used;           // bytes of input the call consumes
  uint64_t out_cap;
  uint32_t n_pieces;
  uint32_t wrap;
  uint32_t header;            // the call's bytes start with the container's header
  uint32_t close;             // ... and end with the closing block and the trailer
};
struct X2n;  // (checksum_clip.h)
__global__ void one_writer_begin_kernel(OneWriterParams Q);
__global__ void one_writer_index_kernel(OneWriterParams Q);
__global__ void one_writer_commit_kernel(OneWriterParams Q, X2n T);
__global__ void one_writer_copy_kernel(const OneWriterState *st, const uint8_t *buf, uint8_t *out);

// The seek index of one long stream (one_seek_kernels.hip; flate_hip_inflate_one_seek_index / _ranges; the rule and
// the index's layout: seek_index_rule.h).
// BUILD.  one_seek_points_kernel (POINTS, one workgroup): mark by the point rule, scan, compact -> point_unit, n_points.
// Per round of flate_hip_inflate_one's TAIL / COMPOSE / RESOLVE, one_seek_pack_kernel lists the round's point units as
// runs of R for bgzf_gather_kernel (PACK): run j = R[point_unit[p_lo + j] - u0] -> block p_lo + j - 1 of the windows.
struct OneSeekPointsParams {
  const uint64_t *out_off;   // n + 1
  uint32_t n;
  uint64_t span;             // >= 1
  uint64_t *point_unit;      // n entries of room
  uint32_t *n_points;
};
__global__ void one_seek_points_kernel(OneSeekPointsParams P);
__global__ void one_seek_pack_kernel(const uint64_t *point_unit, uint32_t p_lo, uint32_t np, uint32_t u0,
                                     uint64_t *r_out_off, uint64_t *r_src);
// READ.  Locate: one thread per range (seek_locate) and +1 at pstart(first) / -1 behind last into a difference array
// over the units.  Select: its scan marks the DECODED units; one scan of (1, size) gives each its rank and its place in
// the dense scratch; compacted in stream order (sel_unit, sel_at).  Layout: the scan of the ranges' lengths, where
// every range's ONE run starts in the scratch, and the ranks [r_rank_lo, r_rank_hi) of the units [pstart(first), last].
struct OneSeekHead {         // the result words, read back in front of the arrays
  uint64_t out_total;        // bytes of all ranges
  uint64_t scratch_total;    // bytes of all decoded units
  uint32_t n_sel;            // decoded units
  uint32_t pad;
};
struct OneSeekParams {
  const uint64_t *unit_bit;  // n + 1: the index, uploaded
  const uint64_t *out_off;   // n + 1
  const uint64_t *point_unit;  // n_points
  uint32_t n, n_points;
  uint64_t span;
  uint32_t n_ranges;
  const uint64_t *begin;     // n_ranges each (device copies of the caller's arrays)
  const uint64_t *end;
  int32_t *diff;             // n + 1, zeroed
  uint32_t *rank;            // n: decoded units in front of unit k
  uint64_t *scratch_at;      // n: decoded bytes in front of unit k
  uint64_t *r_b, *r_len;     // per range (locate)
  uint32_t *r_first, *r_last, *r_seg;
  uint64_t *r_src;           // layout: where the range's run starts in the scratch
  // what the host reads back, one block: head | r_out_off (n_ranges + 1) | r_rank_lo | r_rank_hi | sel_unit
  OneSeekHead *head;
  uint64_t *r_out_off;
  uint32_t *r_rank_lo, *r_rank_hi;
  uint32_t *sel_unit;        // n entries of room, head->n_sel used: the decoded units in stream order
  uint64_t *sel_at;          // n + 1 entries of room: their places in the scratch, then scratch_total
};
__global__ void one_seek_locate_kernel(OneSeekParams P);
__global__ void one_seek_select_kernel(OneSeekParams P);
__global__ void one_seek_layout_kernel(OneSeekParams P);
// A round of `count` units of the list from place i0.  one_seek_seed_kernel: per unit its SEED -- the round-local
// place of the nearest point at or in front of it, or 0 when its segment continues from the round in front (R[0] is
// the carried window then) -- and its piece for the decoder.  one_seek_load_kernel: the stored windows of the round's
// points from `windows` (any alignment) into their R slots (point 0: zeros).  one_tail_kernel through
// OneDecParams::unit_list.  one_seek_compose_kernel: the SEGMENTED scan step, dst[k] = src[k] o src[k - s] only when
// k - s is not in front of k's seed.  one_seek_resolve_kernel: R[k + 1] = the composed function of k applied to
// R[seed[k]], unless k + 1 is a point (its slot holds the stored window).  one_seek_check_kernel: a unit is good iff
// its piece ends with status 0 and fills its slot exactly.
struct OneSeekRoundParams {
  OneSeekParams Q;
  uint32_t i0, count;
  const uint8_t *windows;    // device
  uint8_t *R;                // (count + 1) * 32768
  uint32_t *seed;            // count
  uint64_t *p_bit_off;       // count
  uint64_t *p_bit_end;       // count
  uint64_t *p_dict_at;       // count
  uint32_t *p_dict_len;      // count
  const int32_t *d_status;   // count: what DECODE reports
  const uint64_t *d_out_len;
  int32_t *u_status;         // n_sel: per decoded unit
};
__global__ void one_seek_seed_kernel(OneSeekRoundParams S);
__global__ void one_seek_load_kernel(OneSeekRoundParams S);
__global__ void one_seek_compose_kernel(const uint16_t *src, uint16_t *dst, const uint32_t *seed, uint32_t count, uint32_t s);
__global__ void one_seek_resolve_kernel(const uint16_t *F, uint8_t *R, const uint32_t *seed, uint32_t count);
__global__ void one_seek_check_kernel(OneSeekRoundParams S);

// The PACKED windows of that index (seek_pack_rule.h; flate_hip_seek_windows_pack / _unpack,
// flate_hip_inflate_one_ranges_packed).  seek_pack_mark_kernel (seek_pack_mark_kernel.inc, on the shared reader): MARK +
// SPARSIFY, one wavefront per block b = point b + 1 -- the token walk from the point's bit over at most 32768 bytes of
// output, the keep mask in LDS, then the raw block with everything else zeroed into slot b of `dense`.
// seek_pack_flags_kernel: the non-zero test alone (COMPRESS without SPARSE).  seek_pack_load_kernel: one_seek_load_kernel
// with the unpacked blocks of the SELECTED points in a dense stage, through the point -> slot table.
struct SeekPackBlock {       // per block, read back once
  uint32_t nonzero;          // the (sparsified) block has a non-zero byte
  uint32_t kept;             // bytes the keep rule marks (whole blocks: 32768)
  int32_t status;            // 0, or FLATE_HIP_E_CORRUPT: the walk failed or left the segment anywhere but at its end
  uint32_t pad;
};
struct SeekMarkParams {
  const uint8_t *in;         // the whole input (device)
  uint64_t in_len;
  const FrameOne *one;       // the raw stream's range as this input has it
  const uint64_t *unit_bit;  // n + 1: the index, uploaded
  const uint64_t *out_off;   // n + 1
  const uint64_t *point_unit;  // n_points
  uint32_t n, n_points;
  const uint8_t *windows;    // n_points - 1 blocks, any alignment
  uint8_t *dense;            // n_points - 1 slots of 32768 bytes, 16-byte aligned
  SeekPackBlock *blk;        // n_points - 1
};
__global__ void seek_pack_mark_kernel(SeekMarkParams M);
__global__ void seek_pack_flags_kernel(const uint8_t *windows, uint32_t n_blocks, SeekPackBlock *blk);
__global__ void seek_pack_load_kernel(OneSeekRoundParams S, const uint32_t *slot_of_point);

// A gzip FILE of any members, long ones included (gzfile_kernels.hip; flate_hip_gzfile_index / _read; the rule:
// gzfile_rule.h).  The units of ALL members form one chain over the file's bits: the raw stream of OneParams is
// in[0, in_len - 8), so every bit and every error offset is counted from the file's first byte.  The nodes are two
// lists in one array: A, the n_a bit offsets of one_count_kernel / one_fill_kernel (the dynamic-header rule at every
// bit of the file; sorted), then B, one node per byte offset that passes the gzip header rule (gzip_count_kernel /
// gzip_fill_kernel without a clip; hdr_off sorted), at the bit behind that header.  one_probe_kernel probes every node.
// A node that stops in front of a dynamic header links into A as the units of one stream do; one that ends with
// BFINAL takes THE HOP into B; so the first unit of a member is always a B node and every other unit an A node, and a
// bit that is in both lists is two nodes of which the path takes the one its predecessor names.
struct GzFileHead {        // the discovery's verdict, read back as one block with the OneHead in front of it
  int64_t err_off;         // where the failing member starts, or where no member could start; -1
  int64_t stream_err_off;  // the serial decoder's offset, counted from that member's raw stream; -1
  uint32_t n_members;      // whole good members
  uint32_t no_header;      // the chain broke where a header had to be
  uint32_t pad[2];
};
struct GzFileParams {
  OneParams O;             // the chain: O.C.cap = n_a + n_b nodes, O.C.member_off = unit_bit
  uint32_t n_a, n_b;
  const uint64_t *hdr_off; // n_b + 1: List B's byte offsets
  uint64_t *u_start;       // cap + 1, per unit: its member's header offset + 1 when it starts a member, else 0
  uint32_t *u_final;       // cap, per good unit: it ends with BFINAL
  uint32_t *u_member;      // cap + 1, per unit: its member
  uint64_t *rel_off;       // cap + 1, per unit: out_off[k] - out_off[its member's first unit]
  uint64_t *member_off;    // n_b + 2, per member: its header's offset; behind the last: in_len
  uint64_t *member_unit;   // n_b + 2: its first unit; behind the last: the unit count
  uint64_t *member_out;    // n_b + 2: out_off[member_unit]
  GzFileHead *gh;
};
// THE FORM of a discovery.  A file reaches these kernels whole or in parts (below), and the whole file is the part that
// is final and starts at a BOUNDARY: GzFileMode{} with final_in = 1.  What a part adds -- the root INSIDE a member, THE
// PARTS HOP of a part that is not final, the carried count, the OPEN stop -- is stated once, in the kernels that take
// the mode; `part` alone says what no value of the others does: whose result words the call reports.
struct GzFileMode {
  uint32_t part;            // a reader's call: the root's header verdict is taken; the member words are the host's
  uint32_t inside;          // the chain's root is FIND's candidate 0 (bit b0), not the member at offset 0
  uint32_t final_in;        // the file ends with in[0, in_len)
  uint64_t hist;            // what the continued member produced in front of the part, saturated at the window
  const uint32_t *verdict;  // n_b, or null: List B's three verdicts (gzfile_parts_serial_rule.h); null = all LONG
};
__global__ void gzfile_init_kernel(FrameOne *one, const uint8_t *in, uint64_t in_len, GzFileMode M, uint32_t b0);
__global__ void gzfile_bits_kernel(GzFileParams P);
__global__ void gzfile_link_kernel(GzFileParams P, GzFileMode M);
__global__ void gzfile_finish_kernel(GzFileParams P, GzFileMode M);
__global__ void gzfile_members_kernel(GzFileParams P);
__global__ void gzfile_rel_kernel(GzFileParams P, GzFileMode M);
// The decode (flate_hip_gzfile_read): flate_hip_inflate_one's rounds with every member's first unit as a SEED of the
// segmented scan (one_seek_compose_kernel / one_seek_resolve_kernel): TAIL runs with rel_off as its out_off, and a
// piece's history is min(32768, what its own member has produced in front of it).  gzfile_trailer_kernel: one thread
// per member, CRC-32 and ISIZE against the trailer, an ordered min; gzfile_verdict_kernel: the call's words.
struct GzFileVerdict {
  uint64_t out_len;
  int64_t err_off, stream_err_off;
  int32_t status;
  uint32_t bad_member;
  uint32_t n_members, n_units;
  uint32_t bad_trailer;    // 0xffffffff: none (set by the host's fill)
  uint32_t pad;
};
struct GzFileDecParams {
  OneDecParams D;          // D.out_off = the file's out_off
  GzFileParams P;
  uint32_t n_good;         // the discovery's good units
  uint32_t n_members;      // ... and whole members (gzfile_trailer_kernel)
  uint32_t *seed;          // count
  uint64_t *p_bit_off;     // count
  uint64_t *p_bit_end;     // count: ~0 = the piece runs to BFINAL
  const uint32_t *sums;    // per member: the CRC-32 of its output
  GzFileVerdict *v;
};
__global__ void gzfile_pieces_kernel(GzFileDecParams G, uint64_t hist);
__global__ void gzfile_trailer_kernel(GzFileDecParams G);
__global__ void gzfile_verdict_kernel(GzFileDecParams G);

// A gzip file read in PARTS (flate_hip_gzfile_reader_*; gzfile_parts_kernels.hip; the rule: gzfile_parts_rule.h).  A
// call is the discovery and the rounds above over one part of the file.  FIND (its PARTS build: candidate 0 at bit
// FrameOne::b0), PROBE, the chain rounds, the out-scan, the tail probe, gzfile_bits_kernel, gzfile_members_kernel,
// TAIL, COMPOSE, RESOLVE, DECODE, the check and the checksum kernels run as they are, and so do the kernels that take
// a GzFileMode, with the part's: the root's header verdict in FrameOne::bad, a BOUNDARY stop into the terminal sink and
// how the chain ended into GzFileHead::pad[0], the units in front of the part's first header (u_member == 0xffffffff)
// at the carried count and seeded by R[0], the handle's window.  The part's own:
//   gzfile_part_trailer_kernel  a thread per member that ends among the delivered units: CRC-32 (the continued member's
//                               is the joined sum) and ISIZE against the trailer in the part, an ordered min
//   gzfile_part_carry_kernel    the result words in file order, and the unfinished member's sum back into the handle
constexpr uint32_t kGzPartEndFile = 0, kGzPartEndStop = 1, kGzPartEndDead = 2;  // GzFileHead::pad[0]
struct GzPartSeg;            // (gzfile_parts_rule.h)
struct GzPartState {         // per handle, in device memory
  uint8_t window[32768];     // the 32 KiB in front of the next unit of the member in progress
  uint64_t total;            // checksum_join_device's length word
  uint32_t sum;              // the running CRC-32 of the member in progress (0: of nothing)
  uint32_t joined;
  GzFileVerdict res;         // the call's result words, read back: err_off counts from the part's first byte,
                             // bad_member is the UNIT that TAIL failed in, bad_trailer the segment
};
struct GzPartParams {
  GzPartState *st;
  const uint8_t *in;
  const GzPartSeg *segs;     // the members among the decoded units (uploaded)
  const uint32_t *sums;      // [0]: the running sum as the call found it; [1 + i]: segment i's bytes of this call
  uint32_t n_segs;
  uint32_t n_end;            // the first n_end segments end among the delivered units
  uint32_t sum0_mode;        // segment 0's sum: 0 = its own, 1 = the running one (no bytes in this call), 2 = joined
  uint32_t keep_sum;         // the last segment goes on behind the call: its sum is the handle's next running sum
  uint32_t n_del;            // complete units delivered if nothing fails
  int32_t term_rc;           // the chain's verdict when the call delivers everything in front of it, else 0
  int64_t term_err_off;
  uint64_t total;
};
__global__ void gzfile_part_trailer_kernel(GzPartParams Q, OneDecParams D);
__global__ void gzfile_part_carry_kernel(GzPartParams Q, OneDecParams D);

// Short members decoded WHOLE (gzfile_serial_kernels.hip, gzfile_parts_serial_kernels.hip; the option
// "gzfile_serial_max" and flate_hip_gzfile_reader_set_serial_max = S >= 1; the rules: gzfile_serial_rule.h,
// gzfile_parts_serial_rule.h).  With S = 0 none of this is launched and the structures above are what they were.
// PHASE 1 runs over List B alone, in front of FIND: gzfile_serial_ranges_kernel gives every B candidate its serial
// range, ONE size-only launch of the batch decoders runs over them (InfParams::used), gzfile_serial_nodes_kernel
// gives each THE THREE VERDICTS -- a WHOLE candidate gets its record and links by THE PARTS HOP, every other node
// absorbs --, gzfile_serial_round_kernel doubles the pointers and gzfile_serial_from_kernel reads find_from where the
// walk from candidate 0 came to rest (INSIDE a member: 0; in front of an OPEN member: nowhere, and GzSerialHead::pad).
// The whole file is the part GzPartSerialIn{1, 0, ~0, null}: its verdicts are WHOLE where the whole test holds and
// LONG elsewhere, its hop is THE HOP.  PHASE 2: FIND runs over in[find_from, in_len) only (or not at all);
// gzfile_serial_base_kernel moves its bits to the file's origin; gzfile_serial_bits_kernel is gzfile_bits_kernel,
// except that a whole candidate's bit is the raw stream's end, so that PROBE leaves it at once;
// gzfile_serial_keep_kernel puts a whole candidate's bit and its phase-1 record back behind PROBE.  Link, rounds,
// finish, the scans and the rel kernel then run over the combined nodes as they are: a whole member is a unit that
// ends with BFINAL.  gzfile_serial_marks_kernel: per path rank, is the unit a whole member, and where its stream ends;
// gzfile_serial_list_kernel (one workgroup): the whole members among the first units compacted into the streams of
// ONE batch -- in_off, in_end, the slots and their sizes; the whole call launches it behind the out-scan over the good
// units (the last slot ends at out_off[n_units]), a reader's call behind the host's plan over the units it decodes
// (the last slot ends at the planned total).  A part's chain has no list behind it but
// gzfile_part_serial_stop_kernel: did it end in front of an OPEN member (GzSerialHead::pad).
// gzfile_serial_check_kernel, behind that batch in the read: status 0 and exactly the size the discovery found, else
// OneDecHead::decode_bad.
struct GzSerialHead {
  uint64_t find_from;      // phase 1: where FIND starts; in_len = nowhere
  uint32_t n_whole;        // gzfile_serial_list_kernel: the whole members among the good units
  uint32_t pad;
};
struct GzSerialParams {
  const uint8_t *in;
  uint64_t in_len;
  uint64_t serial_max;     // S
  uint32_t n_a, n_b;
  const uint64_t *hdr_off; // n_b + 1: List B's byte offsets
  uint64_t *pay_off;       // n_b + 1: the serial ranges
  uint64_t *pay_end;       // n_b
  const int32_t *status;   // n_b each: what the size-only decode left
  const uint64_t *out_len;
  const uint64_t *used;
  OneProbe *rec;           // n_b: a whole candidate's record
  uint32_t *whole;         // n_b
  uint32_t *jump[2];       // n_b + 2: the walk's links; n_b = the file's end, n_b + 1 = a dead hop
  GzSerialHead *head;
  // behind the chain (sized for its n_a + n_b nodes)
  uint32_t *u_whole;       // cap + 1, per unit
  uint64_t *u_end;         // cap + 1, per whole unit: the byte behind its final block
  // the batch of whole members
  uint64_t *w_in_off;      // n_b + 1
  uint64_t *w_in_end;      // n_b
  uint64_t *w_out_off;     // n_b + 1
  uint64_t *w_size;        // n_b
  uint32_t *w_unit;        // n_b
};
struct GzPartSerialIn {      // phase 1's form (the chain's: GzFileMode)
  uint32_t final_in, inside;
  uint64_t out_cap;          // a member that inflates to more is not WHOLE
  uint32_t *verdict;         // n_b, or null: kGzPartLong / kGzPartWhole / kGzPartOpen, kept for the chain's link
};
__global__ void gzfile_serial_ranges_kernel(GzSerialParams S);
__global__ void gzfile_serial_nodes_kernel(GzSerialParams S, GzPartSerialIn A);
__global__ void gzfile_serial_round_kernel(const uint32_t *src, uint32_t *dst, uint32_t n);
__global__ void gzfile_serial_from_kernel(GzSerialParams S, GzPartSerialIn A, const uint32_t *jump);
__global__ void gzfile_serial_base_kernel(uint64_t *cand_off, uint32_t n, uint64_t base_bits);
__global__ void gzfile_serial_bits_kernel(GzFileParams P, GzSerialParams S);
__global__ void gzfile_serial_keep_kernel(GzFileParams P, GzSerialParams S);
__global__ void gzfile_serial_marks_kernel(GzFileParams P, GzSerialParams S);
// from_head: the unit count and the total are the chain's head's (n_dec and total are not read), else the host's
__global__ void gzfile_serial_list_kernel(GzFileParams P, GzSerialParams S, uint32_t from_head, uint32_t n_dec, uint64_t total);
__global__ void gzfile_serial_check_kernel(GzSerialParams S, uint32_t n_whole, const int32_t *d_status,
                                           const uint64_t *d_out_len, OneDecHead *dh);
__global__ void gzfile_part_serial_stop_kernel(GzFileParams P, GzSerialParams S);

// The seek index of a gzip FILE (gzfile_seek_kernels.hip; flate_hip_gzfile_seek_index / _ranges; the rule and the
// index's layout: gzfile_seek_rule.h).  Locate, select, layout, compose, resolve, check, TAIL and the gather are the
// kernels above, unchanged: they see the file's units as the units of one stream.
// BUILD.  gzfile_seek_points_kernel (POINTS, one workgroup): the point rule with the discovery's member-start mark per
// unit, scan, compact -> point_unit, counts[0] = points, counts[1] = windows.  gzfile_seek_pack_kernel (PACK): the
// round's points p_lo .. p_lo + np - 1 as runs of R for bgzf_gather_kernel; a member start is a run of NO bytes, so the
// window-bearing points land one behind the other from block gzfile_seek_blocks_before(p_lo) on (r_out_off counts from
// that block; entry np: np_all == p_lo + np ? all windows : the blocks in front of point p_lo + np).
struct GzSeekPointsParams {
  const uint64_t *out_off;   // n + 1
  const uint64_t *u_start;   // n: != 0 where the unit starts a member (GzFileParams::u_start)
  uint32_t n;
  uint64_t span;             // >= 1
  uint64_t *point_unit;      // n entries of room
  uint32_t *counts;          // 2
};
struct GzSeekPackParams {
  const uint64_t *point_unit;
  const uint64_t *member_unit;  // m + 1
  uint32_t m, n_points;
  uint32_t p_lo, np, u0;
  uint64_t *r_out_off;       // np + 1
  uint64_t *r_src;           // np
};
__global__ void gzfile_seek_points_kernel(GzSeekPointsParams P);
__global__ void gzfile_seek_pack_kernel(GzSeekPackParams P);
// READ.  gzfile_seek_members_kernel: one thread per member, its header must end where the index has its first unit --
// an ordered min of the members that miss into *bad_member (0xffffffff: none).  gzfile_seek_rel_kernel: one thread per
// unit, rel[k] = out_off[k] - out_off[f(k)]: TAIL's out_off.  Per round of the unit list: gzfile_seek_seed_kernel
// (one_seek_seed_kernel's seed; the piece from the index, its end ~0 where the unit runs to BFINAL, its history
// min(32768, rel)) and gzfile_seek_load_kernel (the stored window of each of the round's points into its R slot by the
// block formula; a member start's slot is ZERO-FILLED; place 0 of a segment that continues is left alone).
struct GzSeekParams {
  OneSeekParams Q;           // the file's units as one stream's
  const uint8_t *in;
  uint64_t in_len;
  const uint64_t *member_off;   // m + 1
  const uint64_t *member_unit;  // m + 1
  uint32_t m;
  uint64_t *rel;             // n + 1
  uint32_t *bad_member;
};
struct GzSeekRoundParams {
  OneSeekRoundParams S;
  const uint64_t *member_unit;  // m + 1
  uint32_t m;
  const uint64_t *rel;       // n + 1
};
__global__ void gzfile_seek_members_kernel(GzSeekParams G);
__global__ void gzfile_seek_rel_kernel(GzSeekParams G);
__global__ void gzfile_seek_seed_kernel(GzSeekRoundParams S);
__global__ void gzfile_seek_load_kernel(GzSeekRoundParams S);

size_t inflate_simt_lds_bytes(int lanes_per_wave);  // dynamic LDS of that launch
size_t inflate_simt_lens_bytes(uint32_t blocks);    // global scratch of that launch (InfParams::simt_lens)

}  // namespace flate

// the ctx as the other host-side files of the library see it (gather.hip)
#include <string>
struct flate_hip_ctx;
namespace flate {
hipStream_t ctx_stream(flate_hip_ctx *c);
int ctx_device(flate_hip_ctx *c);
void ctx_set_error(flate_hip_ctx *c, const std::string &msg);
uint32_t ctx_num_cus(flate_hip_ctx *c);
// one stage's kernels between two events of the ctx (when profiling is on); ctx_stage_collect after the
// stream has been synchronised: stage_ms[stage] from them, every other stage zero
void ctx_stage_begin(flate_hip_ctx *c, int stage);
void ctx_stage_end(flate_hip_ctx *c, int stage);
int ctx_stage_collect(flate_hip_ctx *c, int stage);
// grow-only device scratch owned by the ctx (slot 0: a call's index arrays and partial results, slot 1: a
// staged copy of host input): no hipMalloc / hipFree per call -- hipFree drains the whole device
int ctx_scratch(flate_hip_ctx *c, int slot, size_t bytes, void **p);
// the ctx's pinned staging + copy kernel for small index arrays (see ctl_begin in flate_api.hip);
// ctx_ctl_finish after the stream has been synchronised
int ctx_ctl_begin(flate_hip_ctx *c, size_t up_bytes, size_t down_bytes);
int ctx_ctl_up(flate_hip_ctx *c, void *dev_dst, const void *host_src, size_t bytes);
int ctx_ctl_down(flate_hip_ctx *c, void *host_dst, const void *dev_src, size_t bytes);
void ctx_ctl_finish(flate_hip_ctx *c);
// flate_hip_checksum_batch without its two ends (checksum.hip): d_in is DEVICE memory, in_off a host array, the n sums
// stay in device memory at d_sums -- kernels queued on the ctx's stream, no read-back, no synchronise; the two
// kernels between the events of `stage` (-1: the caller brackets a longer run of kernels itself).  The caller has
// made room with ctx_ctl_begin: checksum_ctl_up_bytes(in_off, n) bytes of uploads.  Slot 0 of ctx_scratch holds the
// partial results until the kernels have run, checksum_scratch_bytes(in_off, n) bytes of it: a caller that queues
// several calls sizes the slot for the largest first, so that no call between them grows (frees) it.
size_t checksum_ctl_up_bytes(const uint64_t *in_off, uint32_t n);
size_t checksum_scratch_bytes(const uint64_t *in_off, uint32_t n);
int checksum_device(flate_hip_ctx *c, const uint8_t *d_in, const uint64_t *in_off, uint32_t n, uint32_t kind,
                    uint32_t *d_sums, int stage);
// The sums of what a batch decoder PRODUCED (flate_hip_inflate_batch_framed): stream i's bytes are
// d_out[slot_off[i], slot_off[i] + d_out_len[i]) -- slot_off a host array, out_len known on the device only.  The 64 KiB
// pieces are planned over the slots and clipped on the device (checksum_clip.h); a stream whose d_status or d_bad
// entry is non-zero is not summed (its entry of d_sums is the sum of nothing).  No events: the caller brackets.
// Room: checksum_ctl_up_bytes(slot_off, n) and checksum_scratch_bytes(slot_off, n), as for checksum_device.
int checksum_device_clipped(flate_hip_ctx *c, const uint8_t *d_out, const uint64_t *slot_off, uint32_t n, uint32_t kind,
                            const uint64_t *d_out_len, const int32_t *d_status, const uint32_t *d_bad,
                            uint32_t *d_sums);
// Behind it, for ONE member whose raw stream is spliced (flate_hip_inflate_spliced_framed): the n sums of d_sums
// joined into the checksum of the concatenation of d_out[slot_off[i], slot_off[i] + min(out_len[i], slot)), i = 0 ..
// n - 1, left at *d_sum with its length at *d_total (checksum_join_kernel, one workgroup; d_slot_off is the DEVICE
// copy of slot_off).  A piece with a status was summed as nothing but keeps its length here: a member with such a
// piece is never judged by its checksum.
int checksum_join_device(flate_hip_ctx *c, const uint32_t *d_sums, const uint64_t *d_slot_off,
                         const uint64_t *d_out_len, uint32_t n, uint32_t kind, uint32_t *d_sum, uint64_t *d_total);
}  // namespace flate
#endif  // __HIPCC__
