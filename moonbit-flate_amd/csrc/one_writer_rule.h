// one_writer_rule.h -- ONE long stream written in PARTS (flate_hip_one_writer_*), what a call decides, written ONCE:
// plain C++17 without HIP, compiled into the library's host code (api_checks.h), into the writer's kernels
// (one_writer_kernels.hip) and into tests/host_model/one_writer_rule_model.cpp, which compares it with
// tests/one_writer_ref.py.
//
// A call is flate_hip_deflate_fast_spliced over the whole pieces of P bytes that in[0, in_len) holds (a final call:
// over everything, the last piece shorter), continued at the bit the call before it stopped at.  The pieces are
// independent, and the position maps of splice_rule.h depend on the start position only modulo 8, so the bits are those
// of one call over the whole input whatever the cut.  This file says which pieces a call consumes, whether it writes
// the container's header and the closing block with the trailer, at which bit of the call's own buffer the scan
// starts, and -- from the bit the scan ends at -- which bytes the call delivers and what stays in the handle.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define ONE_WRITER_HD __host__ __device__ inline
#else
#define ONE_WRITER_HD inline
#endif

namespace flate {

// the wraps, the flags and the status words (FLATE_HIP_WRAP_* / FLATE_HIP_E_*; this header is compiled without
// flate_hip.h, api_checks.h holds the two against each other)
constexpr uint32_t kWriterRaw = 0, kWriterZlib = 1, kWriterGzip = 2;
constexpr int kWriterOk = 0, kWriterStreamEnd = 1, kWriterInvalid = -1, kWriterOutTooSmall = -2, kWriterTooLarge = -6;
constexpr uint64_t kWriterPieceDefault = 65535;      // "zip_piece_bytes"' measured best
constexpr uint64_t kWriterPieceLimit = 0x7ffe0000ull;  // a piece is one stream of the batch encoder (make_plan)

ONE_WRITER_HD uint32_t one_writer_header_len(uint32_t wrap) { return wrap == kWriterGzip ? 10u : wrap == kWriterZlib ? 2u : 0u; }
ONE_WRITER_HD uint32_t one_writer_trailer_len(uint32_t wrap) { return wrap == kWriterGzip ? 8u : wrap == kWriterZlib ? 4u : 0u; }
ONE_WRITER_HD uint64_t one_writer_piece(uint64_t piece_bytes) { return piece_bytes ? piece_bytes : kWriterPieceDefault; }

// ---- the arguments ----
ONE_WRITER_HD int one_writer_open_args(const void *ctx, uint32_t wrap, uint64_t piece_bytes, uint32_t flags, uint32_t allowed,
                                       const void *writer) {
  if (!ctx || !writer || wrap > kWriterGzip || piece_bytes >= kWriterPieceLimit || (flags & ~allowed)) return kWriterInvalid;
  return kWriterOk;
}
ONE_WRITER_HD int one_writer_write_args(const void *writer, const uint8_t *in, uint64_t in_len, const uint8_t *out, uint64_t out_cap,
                                        const uint64_t *in_used, const uint64_t *out_len, const uint32_t *n_pieces) {
  if (!writer || !in_used || !out_len || !n_pieces || (in_len && !in) || (out_cap && !out)) return kWriterInvalid;
  return kWriterOk;
}

// ---- what the host remembers between two calls (everything else rests on the device) ----
struct OneWriterHost {
  uint32_t started;     // some call has delivered bytes: the header lies behind
  uint32_t carry_bits;  // bits of the last, incomplete byte (0..7): the end bit of the last call, modulo 8
  int32_t status;       // sticky: 0, FLATE_HIP_STREAM_END or an error behind the commit point
};
ONE_WRITER_HD OneWriterHost one_writer_fresh() { return OneWriterHost{0, 0, 0}; }

// ---- one call ----
constexpr uint32_t kWriterRun = 0;      // launch: n_pieces pieces, header / close as said
constexpr uint32_t kWriterNothing = 1;  // FLATE_HIP_OK with nothing used and nothing launched: the caller appends more
constexpr uint32_t kWriterReturn = 2;   // `status` without a launch

struct OneWriterPlan {
  uint32_t action;
  int32_t status;
  uint64_t n_pieces;   // k
  uint64_t in_used;
  uint32_t header;     // the call's bytes start with the container's header
  uint32_t close;      // ... and end with the closing block and the trailer
  uint64_t start_bit;  // where the scan starts in the call's buffer: behind the header, or at the carry
};

ONE_WRITER_HD OneWriterPlan one_writer_plan(const OneWriterHost &s, uint64_t in_len, bool final_in, uint64_t piece_bytes,
                                            uint32_t wrap) {
  OneWriterPlan p{kWriterRun, 0, 0, 0, 0, 0, 0};
  const uint64_t P = one_writer_piece(piece_bytes);
  if (s.status) {  // the stream has ended (every write is invalid until reset), or it is dead
    p.action = kWriterReturn, p.status = s.status == kWriterStreamEnd ? kWriterInvalid : s.status;
    return p;
  }
  if (in_len >= (1ull << 32)) {
    p.action = kWriterReturn, p.status = kWriterTooLarge;
    return p;
  }
  p.n_pieces = final_in ? (in_len + P - 1) / P : in_len / P;
  p.in_used = final_in ? in_len : p.n_pieces * P;
  if (!final_in && p.n_pieces == 0) {
    p.action = kWriterNothing;
    return p;
  }
  if (p.n_pieces >= 0xffffffffull) {  // (the index arrays count the pieces in 32 bits, one entry more than there are)
    p.action = kWriterReturn, p.status = kWriterTooLarge;
    return p;
  }
  p.header = s.started ? 0u : 1u;
  p.close = final_in ? 1u : 0u;
  p.start_bit = s.started ? s.carry_bits : 8ull * one_writer_header_len(wrap);
  return p;
}

// Behind the scan: end_bit is where the last piece ends in the call's buffer (no piece: the start bit).  A call that
// is not final delivers the whole bytes in front of that bit and keeps the rest of the last byte; a final one adds the
// closing block (3 bits, the padding to a byte, LEN, NLEN) and the trailer and keeps nothing.
struct OneWriterEnd {
  uint64_t whole;       // bytes delivered = bytes needed
  uint32_t carry_bits;
  uint32_t fits;
};
ONE_WRITER_HD OneWriterEnd one_writer_end(uint64_t end_bit, bool close, uint32_t wrap, uint64_t out_cap) {
  OneWriterEnd e;
  e.whole = close ? ((end_bit + 3u + 7u) >> 3) + 4u + one_writer_trailer_len(wrap) : end_bit >> 3;
  e.carry_bits = close ? 0u : (uint32_t)(end_bit & 7u);
  e.fits = e.whole <= out_cap ? 1u : 0u;
  return e;
}

// The bit of the RAW stream that bit x of the call's buffer is: byte 0 of the buffer is byte `emitted` of the member
// (what the calls before have delivered), and the raw stream starts behind the header.
ONE_WRITER_HD uint64_t one_writer_abs_bit(uint64_t x, uint64_t emitted, uint32_t wrap) {
  return x + 8ull * emitted - 8ull * one_writer_header_len(wrap);
}

// Room for any call on at most in_len bytes, first and final included: every piece within the batch encoder's bound
// for a stream of its length (flate_hip_deflate_bound: two bytes per byte, 320 per window, 16), header, the carried
// byte, closing block and trailer.
ONE_WRITER_HD uint64_t one_writer_bound(uint64_t in_len, uint64_t piece_bytes) {
  const uint64_t P = one_writer_piece(piece_bytes);
  const uint64_t pieces = in_len / P + 1u;
  return 2u * in_len + 320u * (in_len / 65535u + pieces) + 16u * pieces + 32u;
}

}  // namespace flate
