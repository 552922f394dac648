// api_checks.h -- the argument checks of the C ABI's batch calls: plain C++17, no ctx and no HIP call, so that
// tests/test_api_checks.py reaches every refusal on the CPU.  The entry points test their ctx first.
#pragma once

#include <stdint.h>

#include "bgzf_parts_rule.h"
#include "flate_hip.h"
#include "gzfile_parts_rule.h"
#include "gzfile_parts_serial_rule.h"
#include "gzfile_seek_rule.h"
#include "one_parts_rule.h"
#include "one_writer_rule.h"
#include "seek_index_rule.h"
#include "seek_pack_rule.h"
#include "splice_rule.h"

namespace flate {

// flate_hip_inflate_batch(_dict, _framed): the pointers ...
inline bool inflate_batch_ptrs_ok(const uint8_t *in, const uint64_t *in_off, uint32_t n, const uint8_t *out,
                                  const uint64_t *out_off, const uint64_t *out_len, const int32_t *status,
                                  const int64_t *err_off, uint32_t flags) {
  const bool size_only = (flags & FLATE_HIP_SIZE_ONLY) != 0;
  return in_off && out_len && status && err_off && (!n || in) && (size_only || (out_off && (!n || out)));
}
// ... and the streams' offsets and sizes
inline int inflate_batch_ranges(const uint64_t *in_off, uint32_t n, const uint64_t *out_off, uint32_t flags) {
  const bool size_only = (flags & FLATE_HIP_SIZE_ONLY) != 0;
  for (uint32_t i = 0; i < n; ++i)
    if (in_off[i + 1] < in_off[i] || (!size_only && out_off[i + 1] < out_off[i])) return FLATE_HIP_E_INVALID;
  for (uint32_t i = 0; i < n; ++i)
    if (in_off[i + 1] - in_off[i] >= 0x7ffe0000ull) return FLATE_HIP_E_TOO_LARGE;
  return FLATE_HIP_OK;
}

// flate_hip_deflate_fast_batch(_dict, _framed): the pointers (out_off receives the index, so it is never optional)
inline bool deflate_batch_ptrs_ok(const uint8_t *in, const uint64_t *in_off, uint32_t n, const uint8_t *out,
                                  const uint64_t *out_off) {
  return in_off && out_off && (!n || (in && out));
}
// flate_hip_deflate_fast_spliced(_framed): one stream comes out even of no input, so `out` and out_len are never optional
// (the bit index is)
inline bool deflate_spliced_ptrs_ok(const uint8_t *in, const uint64_t *in_off, uint32_t n, const uint8_t *out,
                                    const uint64_t *out_len) {
  return in_off && out && out_len && (!n || in);
}

// flate_hip_deflate_fast_grouped_framed: everything that is refused before any HIP call -- the spliced call's pointers
// (out_off receives the members' index, so it is never optional), an unknown wrap or flag, the groups (grouped_args_ok,
// splice_rule.h) and pieces that run backwards
inline int deflate_grouped_args(const uint8_t *in, const uint64_t *in_off, uint32_t n_pieces, const uint32_t *group_off,
                                uint32_t n_groups, uint32_t wrap, const uint8_t *out, const uint64_t *out_off, uint32_t flags) {
  if (!in_off || !out_off || !group_off || (n_pieces && !in) || (n_groups && !out)) return FLATE_HIP_E_INVALID;
  if (wrap > FLATE_HIP_WRAP_GZIP || (flags & ~(FLATE_HIP_DEVICE_PTRS | FLATE_HIP_COMPAT_GO))) return FLATE_HIP_E_INVALID;
  if (!grouped_args_ok(group_off, n_groups, n_pieces)) return FLATE_HIP_E_INVALID;
  for (uint32_t i = 0; i < n_pieces; ++i)
    if (in_off[i + 1] < in_off[i]) return FLATE_HIP_E_INVALID;
  return FLATE_HIP_OK;
}

// The dictionary table of a call (flate_hip_inflate_batch_framed needs no more: its members choose by DICTID) ...
inline bool dict_table_ok(const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts) {
  if (n_dicts && !dict_off) return false;
  for (uint32_t j = 0; j < n_dicts; ++j)
    if (dict_off[j + 1] < dict_off[j]) return false;
  return !(n_dicts && dict_off[n_dicts] > dict_off[0] && !dicts);
}
// ... and with the streams' choices (flate_hip_inflate_batch_dict / flate_hip_deflate_fast_batch_dict)
inline bool dict_args_ok(const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts, const uint32_t *dict_of,
                         uint32_t n) {
  if (!dict_of && n_dicts == 0) return false;
  if (!dict_table_ok(dicts, dict_off, n_dicts)) return false;
  if (dict_of)
    for (uint32_t i = 0; i < n; ++i)
      if (dict_of[i] >= n_dicts && dict_of[i] != FLATE_HIP_NO_DICT) return false;
  return true;
}

// The index of a spliced stream of in_len bytes (flate_hip_inflate_spliced; _spliced_framed: frame_bytes =
// frame_min_len(wrap), the shortest header and the trailer, which must fit and which the index must leave room for).
inline int spliced_index_check(const uint64_t *bit_off, uint32_t n, const uint64_t *out_off, uint64_t in_len,
                               uint64_t frame_bytes) {
  if (in_len < frame_bytes) return FLATE_HIP_E_INVALID;
  for (uint32_t i = 0; i < n; ++i) {
    if (bit_off[i + 1] < bit_off[i] || out_off[i + 1] < out_off[i] || bit_off[i + 1] > 8 * (in_len - frame_bytes))
      return FLATE_HIP_E_INVALID;
    if (bit_off[i + 1] - bit_off[i] >= (1ull << 30)) return FLATE_HIP_E_TOO_LARGE;  // piece < 128 MiB
  }
  return FLATE_HIP_OK;
}

// ---- BGZF files (flate_hip_bgzf_write / _index / _read / _read_ranges) ----

// block_bytes as the caller passes it -> the block size in use (0 = the default), or 0: not 1 .. 65535, one LZ77 window
inline uint32_t bgzf_block_bytes(uint32_t block_bytes) {
  if (block_bytes == 0) return FLATE_HIP_BGZF_BLOCK_DEFAULT;
  return block_bytes <= 65535u ? block_bytes : 0u;
}
inline uint64_t bgzf_n_blocks(uint64_t in_len, uint32_t bb) { return in_len / bb + (in_len % bb ? 1u : 0u); }
// room that is always enough for the file: every block at its raw bound inside 18 + 8 bytes, and the EOF marker
// (bound: flate_hip_deflate_bound); 0 for a block size that is refused
inline uint64_t bgzf_file_bound(uint64_t in_len, uint32_t block_bytes, size_t (*bound)(size_t)) {
  const uint32_t bb = bgzf_block_bytes(block_bytes);
  if (!bb) return 0;
  const uint64_t full = in_len / bb, tail = in_len % bb;
  return full * ((uint64_t)bound(bb) + 26u) + (tail ? (uint64_t)bound((size_t)tail) + 26u : 0u) + FLATE_HIP_BGZF_EOF_BYTES;
}
inline int bgzf_write_args(const uint8_t *in, uint64_t in_len, uint32_t block_bytes, const uint8_t *out,
                           const uint64_t *out_len, uint32_t flags) {
  if (!out || !out_len || (in_len && !in)) return FLATE_HIP_E_INVALID;
  if (flags & ~(FLATE_HIP_DEVICE_PTRS | FLATE_HIP_COMPAT_GO)) return FLATE_HIP_E_INVALID;
  const uint32_t bb = bgzf_block_bytes(block_bytes);
  if (!bb) return FLATE_HIP_E_INVALID;
  if (bgzf_n_blocks(in_len, bb) > 0xfffffffeull) return FLATE_HIP_E_TOO_LARGE;
  return FLATE_HIP_OK;
}
// member_off and out_off come together or not at all (the query form)
inline int bgzf_index_args(const uint8_t *in, uint64_t in_len, const uint64_t *member_off, const uint64_t *out_off,
                           const uint32_t *n_members, const uint64_t *out_bytes, uint32_t flags) {
  if (!n_members || !out_bytes || (in_len && !in) || (!member_off != !out_off)) return FLATE_HIP_E_INVALID;
  return (flags & ~FLATE_HIP_DEVICE_PTRS) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}
inline int bgzf_read_args(const uint8_t *in, uint64_t in_len, const uint8_t *out, uint64_t out_cap,
                          const uint64_t *out_len, uint32_t flags) {
  if (!out_len || (in_len && !in) || (out_cap && !out)) return FLATE_HIP_E_INVALID;
  return (flags & ~FLATE_HIP_DEVICE_PTRS) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}
// flate_hip_bgzf_read_ranges: everything that is refused before any HIP call.  begin, end and out_off are HOST arrays;
// begin[r] > end[r] numerically is refused in either kind of position (for valid virtual offsets numeric order is
// position order).
inline int bgzf_ranges_args(const uint8_t *in, uint64_t in_len, uint32_t pos_kind, const uint64_t *begin,
                            const uint64_t *end, uint32_t n_ranges, const uint8_t *out, uint64_t out_cap,
                            const uint64_t *out_off, uint32_t flags) {
  if ((in_len && !in) || (out_cap && !out)) return FLATE_HIP_E_INVALID;
  if (n_ranges && (!begin || !end || !out_off)) return FLATE_HIP_E_INVALID;
  if (pos_kind != FLATE_HIP_BGZF_POS_BYTES && pos_kind != FLATE_HIP_BGZF_POS_VIRTUAL) return FLATE_HIP_E_INVALID;
  if (flags & ~FLATE_HIP_DEVICE_PTRS) return FLATE_HIP_E_INVALID;
  for (uint32_t r = 0; r < n_ranges; ++r)
    if (begin[r] > end[r]) return FLATE_HIP_E_INVALID;
  return FLATE_HIP_OK;
}
// flate_hip_bgzf_reader_* / flate_hip_bgzf_writer_* (bgzf_parts_rule.h): everything that is refused before any HIP
// call.  member_off and out_off come together or not at all, and then with room for one entry at least; a writer that
// has ended (a successful final call) refuses every write until reset.
inline int bgzf_reader_open_args(const void *ctx, uint32_t flags, const void *reader) {
  return bgzf_parts_reader_open_args(ctx, flags, FLATE_HIP_DEVICE_PTRS, reader) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}
inline int bgzf_reader_read_args(const void *reader, const uint8_t *in, uint64_t in_len, const uint8_t *out, uint64_t out_cap,
                                 const uint64_t *in_used, const uint64_t *out_len, uint64_t index_cap,
                                 const uint64_t *member_off, const uint64_t *out_off) {
  return bgzf_parts_reader_read_args(reader, in, in_len, out, out_cap, in_used, out_len, index_cap, member_off, out_off)
             ? FLATE_HIP_E_INVALID
             : FLATE_HIP_OK;
}
inline int bgzf_writer_open_args(const void *ctx, uint32_t block_bytes, uint32_t flags, const void *writer) {
  return bgzf_parts_writer_open_args(ctx, bgzf_block_bytes(block_bytes), flags, FLATE_HIP_DEVICE_PTRS | FLATE_HIP_COMPAT_GO, writer)
             ? FLATE_HIP_E_INVALID
             : FLATE_HIP_OK;
}
inline int bgzf_writer_write_args(const void *writer, const uint8_t *in, uint64_t in_len, const uint8_t *out,
                                  const uint64_t *in_used, const uint64_t *out_len, bool ended) {
  return bgzf_parts_writer_write_args(writer, in, in_len, out, in_used, out_len, ended) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}
// how many candidates the discovery arrays hold on the first attempt (real files: one member per tens of KiB; a file
// of nothing but empty members has one per 28 bytes and takes the second attempt, sized from the count)
inline uint32_t bgzf_first_cap(uint64_t in_len) {
  const uint64_t c = in_len / 1024u + 4096u;
  return c > 0xfffffff0ull ? 0xfffffff0u : (uint32_t)c;
}
// the pointer-doubling rounds for that many candidates: the smallest R with 2^R >= cap + 2
inline uint32_t bgzf_rounds(uint32_t cap) {
  uint32_t r = 1;
  while (r < 32u && (1ull << r) < (uint64_t)cap + 2u) ++r;
  return r;
}

// ---- plain multi-member gzip files (flate_hip_gzip_index / _read) ----

// the option "gzip_member_max": the range a candidate is given, 1 .. 2^28 - 1 bytes (the default, which a caller can
// only lower: the sub-block decoder's bit positions are 32 bits wide)
inline bool gzip_member_max_ok(int64_t value) { return value >= 1 && value <= (1ll << 28) - 1; }
// member_off and out_off come together or not at all (the count query)
inline int gzip_index_args(const uint8_t *in, uint64_t in_len, const uint64_t *member_off, const uint64_t *out_off,
                           const uint32_t *n_members, const uint64_t *out_bytes, uint32_t flags) {
  if (!n_members || !out_bytes || (in_len && !in) || (!member_off != !out_off)) return FLATE_HIP_E_INVALID;
  return (flags & ~FLATE_HIP_DEVICE_PTRS) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}
inline int gzip_read_args(const uint8_t *in, uint64_t in_len, const uint8_t *out, uint64_t out_cap,
                          const uint64_t *out_len, uint32_t flags) {
  if (!out_len || (in_len && !in) || (out_cap && !out)) return FLATE_HIP_E_INVALID;
  return (flags & ~FLATE_HIP_DEVICE_PTRS) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}

// ---- one long stream (flate_hip_inflate_one_index) ----

// the option "one_unit_max": the bytes a unit's input spans at most, 1 .. 2^28 (the default, which a caller can only
// lower: the decoders' positions inside one unit are 32 bits wide)
inline bool one_unit_max_ok(int64_t value) { return value >= 1 && value <= (1ll << 28); }
// the option "one_stored_units": the unit rule, 0 (dynamic headers start units: the default) or 1 (stored headers too)
inline bool one_stored_units_ok(int64_t value) { return value == 0 || value == 1; }
// unit_bit and out_off come together or not at all (the count query); the input is ONE raw, zlib or gzip stream
inline int one_index_args(const uint8_t *in, uint64_t in_len, uint32_t wrap, const uint64_t *unit_bit,
                          const uint64_t *out_off, const uint32_t *n_units, const uint64_t *out_bytes,
                          const int32_t *status, uint32_t flags) {
  if (!n_units || !out_bytes || !status || (in_len && !in) || (!unit_bit != !out_off)) return FLATE_HIP_E_INVALID;
  if (wrap > FLATE_HIP_WRAP_GZIP) return FLATE_HIP_E_INVALID;
  return (flags & ~FLATE_HIP_DEVICE_PTRS) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}

// the option "one_round_units": the units flate_hip_inflate_one decodes per round, 1 .. 65536 (scratch: 160 KiB each)
inline bool one_round_units_ok(int64_t value) { return value >= 1 && value <= 65536; }
// flate_hip_inflate_one: out == NULL with out_cap == 0 is the size query
inline int one_args(const uint8_t *in, uint64_t in_len, uint32_t wrap, const uint8_t *out, uint64_t out_cap,
                    const uint64_t *out_len, const int32_t *status, uint32_t flags) {
  if (!out_len || !status || (in_len && !in) || (out_cap && !out)) return FLATE_HIP_E_INVALID;
  if (wrap > FLATE_HIP_WRAP_GZIP) return FLATE_HIP_E_INVALID;
  return (flags & ~FLATE_HIP_DEVICE_PTRS) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}

// flate_hip_one_reader_open / _read (one_parts_rule.h holds the checks; its status words are this header's)
static_assert(kPartsInvalid == FLATE_HIP_E_INVALID && kPartsOutTooSmall == FLATE_HIP_E_OUT_TOO_SMALL &&
                  kPartsCorrupt == FLATE_HIP_E_CORRUPT && kPartsTooLarge == FLATE_HIP_E_TOO_LARGE &&
                  kPartsEof == FLATE_HIP_E_UNEXPECTED_EOF && kPartsStreamEnd == FLATE_HIP_STREAM_END &&
                  kPartsGzip == FLATE_HIP_WRAP_GZIP && kPartsZlib == FLATE_HIP_WRAP_ZLIB,
              "one_parts_rule.h restates flate_hip.h");
inline int one_reader_open_args(const void *ctx, uint32_t wrap, uint32_t flags, const void *reader) {
  return one_parts_open_args(ctx, wrap, flags, FLATE_HIP_DEVICE_PTRS, reader);
}
inline int one_reader_read_args(const void *reader, const uint8_t *in, uint64_t in_len, const uint8_t *out, uint64_t out_cap,
                                const uint64_t *in_used, const uint64_t *out_len) {
  return one_parts_read_args(reader, in, in_len, out, out_cap, in_used, out_len);
}

// flate_hip_gzfile_reader_open / _read (gzfile_parts_rule.h; a read's pointers are checked as the one reader's)
inline int gzfile_reader_open_args(const void *ctx, uint32_t flags, const void *reader) {
  return gzfile_parts_open_args(ctx, flags, FLATE_HIP_DEVICE_PTRS, reader);
}
inline int gzfile_reader_read_args(const void *reader, const uint8_t *in, uint64_t in_len, const uint8_t *out,
                                   uint64_t out_cap, const uint64_t *in_used, const uint64_t *out_len) {
  return one_parts_read_args(reader, in, in_len, out, out_cap, in_used, out_len);
}

// flate_hip_gzfile_reader_set_serial_max / _last_route (gzfile_parts_serial_rule.h).  S: gzfile_serial_max_ok's range;
// fresh: the handle stands behind open or reset and no call has consumed a byte.
inline bool gzfile_serial_max_ok(int64_t value);
inline int gzfile_reader_set_serial_max_args(const void *reader, uint64_t serial_max, bool fresh) {
  if (serial_max > (uint64_t)INT64_MAX || !gzfile_serial_max_ok((int64_t)serial_max)) return FLATE_HIP_E_INVALID;
  return gzfile_parts_serial_set_args(reader, serial_max, fresh);
}
inline int gzfile_reader_last_route_args(const void *reader, const uint32_t *serial_members, const uint32_t *open_stop,
                                         const uint64_t *find_from) {
  return gzfile_parts_route_args(reader, serial_members, open_stop, find_from);
}

// flate_hip_one_writer_open / _write (one_writer_rule.h holds the checks and what a call decides; its words are this
// header's)
static_assert(kWriterInvalid == FLATE_HIP_E_INVALID && kWriterOutTooSmall == FLATE_HIP_E_OUT_TOO_SMALL &&
                  kWriterTooLarge == FLATE_HIP_E_TOO_LARGE && kWriterStreamEnd == FLATE_HIP_STREAM_END &&
                  kWriterGzip == FLATE_HIP_WRAP_GZIP && kWriterZlib == FLATE_HIP_WRAP_ZLIB && kWriterRaw == FLATE_HIP_WRAP_RAW,
              "one_writer_rule.h restates flate_hip.h");
inline int one_writer_open_check(const void *ctx, uint32_t wrap, uint64_t piece_bytes, uint32_t flags, const void *writer) {
  return one_writer_open_args(ctx, wrap, piece_bytes, flags, FLATE_HIP_DEVICE_PTRS | FLATE_HIP_COMPAT_GO, writer);
}
inline int one_writer_write_check(const void *writer, const uint8_t *in, uint64_t in_len, const uint8_t *out, uint64_t out_cap,
                                  const uint64_t *in_used, const uint64_t *out_len, const uint32_t *n_pieces) {
  return one_writer_write_args(writer, in, in_len, out, out_cap, in_used, out_len, n_pieces);
}

// ---- a gzip file of any members (flate_hip_gzfile_index / _read) ----

// unit_bit / out_off and member_off / member_unit: each pair comes together or not at all (both absent: the count query)
inline int gzfile_index_args(const uint8_t *in, uint64_t in_len, const uint64_t *unit_bit, const uint64_t *out_off,
                             const uint64_t *member_off, const uint64_t *member_unit, const uint32_t *n_units,
                             const uint32_t *n_members, const uint64_t *out_bytes, const int32_t *status, uint32_t flags) {
  if (!n_units || !n_members || !out_bytes || !status || (in_len && !in)) return FLATE_HIP_E_INVALID;
  if ((!unit_bit != !out_off) || (!member_off != !member_unit)) return FLATE_HIP_E_INVALID;
  return (flags & ~FLATE_HIP_DEVICE_PTRS) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}
// out == NULL with out_cap == 0 is the size query
inline int gzfile_read_args(const uint8_t *in, uint64_t in_len, const uint8_t *out, uint64_t out_cap,
                            const uint64_t *out_len, const int32_t *status, uint32_t flags) {
  if (!out_len || !status || (in_len && !in) || (out_cap && !out)) return FLATE_HIP_E_INVALID;
  return (flags & ~FLATE_HIP_DEVICE_PTRS) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}

// ---- the seek index of one long stream (flate_hip_inflate_one_seek_index / _ranges; seek_index_rule.h) ----

// the build: index and windows are each a buffer with its capacity, or NULL with 0 (both NULL: the size query)
inline int one_seek_index_args(const uint8_t *in, uint64_t in_len, uint32_t wrap, const uint64_t *index,
                               uint64_t index_cap_words, const uint64_t *index_words, const uint8_t *windows,
                               uint64_t windows_cap, const uint64_t *windows_bytes, const uint32_t *n_units,
                               const uint32_t *n_points, const uint64_t *out_bytes, const int32_t *status, uint32_t flags) {
  if (!index_words || !windows_bytes || !n_units || !n_points || !out_bytes || !status) return FLATE_HIP_E_INVALID;
  if ((in_len && !in) || (index_cap_words && !index) || (windows_cap && !windows)) return FLATE_HIP_E_INVALID;
  if (wrap > FLATE_HIP_WRAP_GZIP) return FLATE_HIP_E_INVALID;
  return (flags & ~FLATE_HIP_DEVICE_PTRS) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}
// the read: flate_hip_bgzf_read_ranges's refusals for byte positions, then the index itself (seek_index_ok, O(n))
inline int one_ranges_args(const uint8_t *in, uint64_t in_len, uint32_t wrap, const uint64_t *index, uint64_t index_words,
                           const uint8_t *windows, uint64_t windows_bytes, const uint64_t *begin, const uint64_t *end,
                           uint32_t n_ranges, const uint8_t *out, uint64_t out_cap, const uint64_t *out_off, uint32_t flags) {
  const int rc = bgzf_ranges_args(in, in_len, FLATE_HIP_BGZF_POS_BYTES, begin, end, n_ranges, out, out_cap, out_off, flags);
  if (rc) return rc;
  if (wrap > FLATE_HIP_WRAP_GZIP || (windows_bytes && !windows)) return FLATE_HIP_E_INVALID;
  return seek_index_ok(index, index_words, windows_bytes, wrap, in_len) && seek_index_rule_ok(index) ? FLATE_HIP_OK
                                                                                                     : FLATE_HIP_E_INVALID;
}

// ---- the packed windows of that index (flate_hip_seek_windows_pack / _unpack, flate_hip_inflate_one_ranges_packed;
// ---- seek_pack_rule.h) ----

// the pack: the mode, the result words, every buffer with its size, then the index itself (seek_index_ok, O(n)); `in`
// may be NULL without FLATE_HIP_SEEK_PACK_SPARSE, for the stream is only walked to mark
inline int seek_pack_args(const uint8_t *in, uint64_t in_len, uint32_t wrap, const uint64_t *index, uint64_t index_words,
                          const uint8_t *windows, uint64_t windows_bytes, uint32_t mode, const uint64_t *pack_index,
                          uint64_t pack_cap_words, const uint64_t *pack_words, const uint8_t *packed, uint64_t packed_cap,
                          const uint64_t *packed_bytes, const uint64_t *kept_bytes, uint32_t flags) {
  if (!pack_words || !packed_bytes || !kept_bytes || !seek_pack_mode_ok(mode)) return FLATE_HIP_E_INVALID;
  if ((flags & ~FLATE_HIP_DEVICE_PTRS) || wrap > FLATE_HIP_WRAP_GZIP) return FLATE_HIP_E_INVALID;
  if ((mode & kSeekPackSparse) && in_len && !in) return FLATE_HIP_E_INVALID;
  if ((windows_bytes && !windows) || (pack_cap_words && !pack_index) || (packed_cap && !packed)) return FLATE_HIP_E_INVALID;
  return seek_index_ok(index, index_words, windows_bytes, wrap, in_len) && seek_index_rule_ok(index) ? FLATE_HIP_OK
                                                                                                     : FLATE_HIP_E_INVALID;
}
// the unpack: the pack index by itself (seek_pack_self_ok, O(n_blocks))
inline int seek_unpack_args(const uint64_t *pack_index, uint64_t pack_words, const uint8_t *packed, uint64_t packed_bytes,
                            const uint8_t *windows, uint64_t windows_cap, const uint64_t *windows_bytes, uint32_t flags) {
  if (!windows_bytes || (flags & ~FLATE_HIP_DEVICE_PTRS)) return FLATE_HIP_E_INVALID;
  if ((packed_bytes && !packed) || (windows_cap && !windows)) return FLATE_HIP_E_INVALID;
  return seek_pack_self_ok(pack_index, pack_words, packed_bytes) ? FLATE_HIP_OK : FLATE_HIP_E_INVALID;
}
// the read: one_ranges_args with the windows the pack index stands for, then seek_pack_ok against the index
inline int one_ranges_packed_args(const uint8_t *in, uint64_t in_len, uint32_t wrap, const uint64_t *index,
                                  uint64_t index_words, const uint64_t *pack_index, uint64_t pack_words,
                                  const uint8_t *packed, uint64_t packed_bytes, const uint64_t *begin, const uint64_t *end,
                                  uint32_t n_ranges, const uint8_t *out, uint64_t out_cap, const uint64_t *out_off,
                                  uint32_t flags) {
  const int rc = bgzf_ranges_args(in, in_len, FLATE_HIP_BGZF_POS_BYTES, begin, end, n_ranges, out, out_cap, out_off, flags);
  if (rc) return rc;
  if (wrap > FLATE_HIP_WRAP_GZIP || (packed_bytes && !packed)) return FLATE_HIP_E_INVALID;
  if (!index || index_words < kSeekHeadWords) return FLATE_HIP_E_INVALID;
  if (!seek_index_ok(index, index_words, seek_windows_bytes(index[kSeekPointsAt]), wrap, in_len) || !seek_index_rule_ok(index))
    return FLATE_HIP_E_INVALID;
  return seek_pack_ok(pack_index, pack_words, packed_bytes, index) ? FLATE_HIP_OK : FLATE_HIP_E_INVALID;
}

// ---- the seek index of a gzip file of any members (flate_hip_gzfile_seek_index / _ranges; gzfile_seek_rule.h) ----

// the build: index and windows are each a buffer with its capacity, or NULL with 0 (both NULL: the size query)
inline int gzfile_seek_index_args(const uint8_t *in, uint64_t in_len, const uint64_t *index, uint64_t index_cap_words,
                                  const uint64_t *index_words, const uint8_t *windows, uint64_t windows_cap,
                                  const uint64_t *windows_bytes, const uint32_t *n_units, const uint32_t *n_members,
                                  const uint32_t *n_points, const uint64_t *out_bytes, const int32_t *status,
                                  uint32_t flags) {
  if (!index_words || !windows_bytes || !n_units || !n_members || !n_points || !out_bytes || !status)
    return FLATE_HIP_E_INVALID;
  if ((in_len && !in) || (index_cap_words && !index) || (windows_cap && !windows)) return FLATE_HIP_E_INVALID;
  return (flags & ~FLATE_HIP_DEVICE_PTRS) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}
// the read: flate_hip_bgzf_read_ranges's refusals for byte positions, then the index itself (gzfile_seek_index_ok,
// O(n + m))
inline int gzfile_ranges_args(const uint8_t *in, uint64_t in_len, const uint64_t *index, uint64_t index_words,
                              const uint8_t *windows, uint64_t windows_bytes, const uint64_t *begin, const uint64_t *end,
                              uint32_t n_ranges, const uint8_t *out, uint64_t out_cap, const uint64_t *out_off,
                              uint32_t flags) {
  const int rc = bgzf_ranges_args(in, in_len, FLATE_HIP_BGZF_POS_BYTES, begin, end, n_ranges, out, out_cap, out_off, flags);
  if (rc) return rc;
  if (windows_bytes && !windows) return FLATE_HIP_E_INVALID;
  return gzfile_seek_index_ok(index, index_words, windows_bytes, in_len) && gzfile_seek_index_rule_ok(index)
             ? FLATE_HIP_OK
             : FLATE_HIP_E_INVALID;
}

// the option "gzfile_serial_max": 0 (the default) = every member is cut into units; S >= 1 = a member whose header and
// raw stream fit in S bytes and decode cleanly is decoded whole (gzfile_serial_rule.h); at most 2^28 - 1, the range of
// the size-only decoders' bit positions, as for "gzip_member_max"
inline bool gzfile_serial_max_ok(int64_t value) { return value >= 0 && value <= (1ll << 28) - 1; }
// flate_hip_gzfile_last_route: every result pointer is required
inline int gzfile_last_route_args(const void *ctx, const uint32_t *serial_members, const uint32_t *unit_members,
                                  const uint64_t *find_from) {
  return (!ctx || !serial_members || !unit_members || !find_from) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}

// ---- ZIP archives (flate_hip_zip_write / _index / _read) ----

// everything flate_hip_zip_write refuses before any HIP call
inline int zip_write_args(const uint8_t *in, const uint64_t *in_off, uint32_t n, const uint8_t *names,
                          const uint64_t *name_off, const uint8_t *out, const uint64_t *out_len, uint32_t flags) {
  if (!in_off || !name_off || !out || !out_len || (n && (!in || !names))) return FLATE_HIP_E_INVALID;
  if (flags & ~(FLATE_HIP_DEVICE_PTRS | FLATE_HIP_COMPAT_GO)) return FLATE_HIP_E_INVALID;
  for (uint32_t i = 0; i < n; ++i) {
    if (in_off[i + 1] < in_off[i] || name_off[i + 1] <= name_off[i]) return FLATE_HIP_E_INVALID;  // (a name of 0 bytes)
    if (name_off[i + 1] - name_off[i] > 65535u) return FLATE_HIP_E_INVALID;
  }
  return FLATE_HIP_OK;
}
// room that is always enough for the archive: every entry at its raw bound (bound: flate_hip_deflate_bound) behind its
// local header, every central record with its Zip64 extra, all three end records; 0 for arguments that are refused
inline uint64_t zip_archive_bound(const uint64_t *in_off, uint32_t n, const uint64_t *name_off, size_t (*bound)(size_t)) {
  if (!in_off || !name_off) return 0;
  uint64_t total = 22u + 56u + 20u;
  for (uint32_t i = 0; i < n; ++i) {
    if (in_off[i + 1] < in_off[i] || name_off[i + 1] <= name_off[i] || name_off[i + 1] - name_off[i] > 65535u) return 0;
    total += 30u + 46u + 12u + 2u * (name_off[i + 1] - name_off[i]) + (uint64_t)bound((size_t)(in_off[i + 1] - in_off[i]));
  }
  return total;
}
// entries and out_off come together or not at all (the count query)
inline int zip_index_args(const uint8_t *in, uint64_t in_len, const void *entries, const uint64_t *out_off,
                          const uint32_t *n_entries, const uint64_t *out_bytes, uint32_t flags) {
  if (!n_entries || !out_bytes || (in_len && !in) || (!entries != !out_off)) return FLATE_HIP_E_INVALID;
  return (flags & ~FLATE_HIP_DEVICE_PTRS) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}
inline int zip_read_args(const uint8_t *in, uint64_t in_len, const uint32_t *sel, uint32_t n_sel, uint32_t n_cap,
                         const uint8_t *out, uint64_t out_cap, const uint64_t *out_off, const uint64_t *out_len,
                         const int32_t *status, const int64_t *err_off, uint32_t flags) {
  if ((in_len && !in) || (out_cap && !out) || !out_off) return FLATE_HIP_E_INVALID;
  if (n_cap && (!out_len || !status || !err_off)) return FLATE_HIP_E_INVALID;
  if (sel ? n_sel > n_cap : n_sel != 0) return FLATE_HIP_E_INVALID;  // (sel == NULL: every entry, n_sel is 0)
  return (flags & ~FLATE_HIP_DEVICE_PTRS) ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
}
// the option "zip_unit_min": 0 (the default) = every entry goes to the batch decoders; v >= 1 = a deflated entry of
// at least v compressed bytes is decoded through units (zip_units_rule.h)
inline bool zip_unit_min_ok(int64_t value) { return value >= 0; }
// the option "zip_piece_bytes": 0 (the default) = every entry is one stream; P >= 1 = an entry longer than P bytes is
// written from pieces of P bytes (zip_pieces_plan, splice_rule.h)
inline bool zip_piece_bytes_ok(int64_t value) { return value >= 0; }
// how many candidates the directory's discovery arrays hold on the first attempt: the records the end record promises
// and some decoys (names or extras that look like records); never more than fit the directory, 4 bytes apart
inline uint32_t zip_first_cap(uint64_t n, uint64_t cd_size) {
  const uint64_t fit = cd_size / 4u + 1u, want = n + 4096u;
  const uint64_t c = want < fit ? want : fit;
  return c > 0xfffffff0ull ? 0xfffffff0u : (uint32_t)c;
}

// what a decode call returns when it has run: FLATE_HIP_OK or the first non-zero status of a stream
inline bool is_stream_status(int rc) {
  return rc == FLATE_HIP_OK || rc == FLATE_HIP_E_OUT_TOO_SMALL || rc == FLATE_HIP_E_CORRUPT || rc == FLATE_HIP_E_UNEXPECTED_EOF;
}

}  // namespace flate
