// one_writer_kernels.hip -- ONE long stream written in PARTS (flate_hip_one_writer_*; flate_kernels.h: OneWriterState,
// OneWriterParams; the rule: one_writer_rule.h).  A call runs the whole call's match finder, histogram, code, scan,
// zero and pack kernels over the pieces it consumes, with the scan started at the carried bit and without a closing
// block unless the call is final; what is the writer's own stands here, four small kernels around them:
//   one_writer_begin_kernel   between the zero and the pack kernel: the container's header (first call), or the carried
//                             bits OR-ed into byte 0 of the handle's buffer -- the zero kernel has cleared exactly the
//                             dwords that this kernel and the pack kernel's OR both touch
//   one_writer_index_kernel   one thread per piece: the scan's positions in the buffer as bits of the raw stream
//   one_writer_commit_kernel  behind pack and checksum: room, the closing block of a call without pieces, the trailer,
//                             the join of the part's checksum to the running one, the new carry, the result words.  It
//                             is the only kernel that writes the handle's state, and it writes it whole or not at all
//   one_writer_copy_kernel    device callers: buffer -> out, exactly out_len bytes, the length read on the device
// The pack kernels store whole dwords around the stream; they do that in the handle's buffer, never in the caller's.
// No kernel waits for another workgroup; no loop is longer than the bytes it copies.
#include <hip/hip_runtime.h>

#include "checksum_clip.h"
#include "flate_hip.h"
#include "flate_kernels.h"
#include "one_writer_rule.h"

namespace flate {

namespace {

// the header as frame_write_kernel writes it: gzip ID1 ID2, CM = 8, FLG = 0, MTIME = 0, XFL = 4, OS = 255; zlib CMF =
// 0x78, FLG = 0x01
__device__ inline uint8_t header_byte(uint32_t wrap, uint32_t k) {
  if (wrap == FLATE_HIP_WRAP_GZIP) return k == 0 ? 0x1f : k == 1 ? 0x8b : k == 2 ? 8 : k == 8 ? 4 : k == 9 ? 255 : 0;
  return k == 0 ? 0x78 : 0x01;
}

// destination chunk j = the 16 bytes from dword Q, bit b of the aligned source chunk j on (b = 0, 8, 16, 24; Q and b
// both 0: the chunk itself)
template <int Q>
__device__ inline void copy_body(uint4 *d, const uint4 *sa, uint32_t b, uint64_t chunks, uint64_t t, uint64_t lanes) {
  for (uint64_t j = t; j < chunks; j += lanes) {
    const uint4 lo = sa[j];
    if (Q == 0 && b == 0) {
      d[j] = lo;
      continue;
    }
    const uint4 hi = sa[j + 1];
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = b ? (w[Q + k] >> b) | (w[Q + k + 1] << (32u - b)) : w[Q + k];
    d[j] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

}  // namespace

__global__ void one_writer_begin_kernel(OneWriterParams Q) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || *Q.status != 0) return;
  if (Q.header) {
    const uint32_t hl = one_writer_header_len(Q.wrap);
    for (uint32_t k = 0; k < hl; ++k) Q.buf[k] = header_byte(Q.wrap, k);
  } else {
    Q.buf[0] |= (uint8_t)(Q.st->carry & ((1u << Q.st->carry_bits) - 1u));
  }
}

// n_pieces + 1 entries: the pieces' first bits and the end bit (where a final call's closing block starts).  It runs in
// front of the commit kernel: st->emitted is still what the calls before have delivered.
__global__ __launch_bounds__(256) void one_writer_index_kernel(OneWriterParams Q) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i > Q.n_pieces || *Q.status != 0) return;
  const uint64_t x = Q.n_pieces ? Q.stream_bit[i] : Q.start_bit;
  Q.bit_idx[i] = one_writer_abs_bit(x, Q.st->emitted, Q.wrap);
}

__global__ void one_writer_commit_kernel(OneWriterParams Q, X2n T) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  OneWriterState *st = Q.st;
  OneWriterResult r{};
  r.n_pieces = Q.n_pieces;
  const int status = *Q.status;
  if (status != 0 && status != FLATE_HIP_E_OUT_TOO_SMALL) {  // the encoder's own word: nothing is delivered
    r.status = status;
    st->res = r;
    return;
  }
  // (a scan status of -2: the handle's own buffer was too small for the scan's total, which the host's bound excludes;
  // the bytes needed are still what the positions say, and nothing has been packed)
  const uint64_t end_bit = Q.n_pieces ? Q.stream_bit[Q.n_pieces] : Q.start_bit;
  const OneWriterEnd e = one_writer_end(end_bit, Q.close != 0u, Q.wrap, Q.out_cap);
  if (status != 0 || !e.fits) {
    r.status = FLATE_HIP_E_OUT_TOO_SMALL;
    r.out_len = e.whole;
    st->res = r;
    return;
  }
  uint8_t *buf = Q.buf;
  const uint32_t tl = one_writer_trailer_len(Q.wrap);
  if (Q.close && Q.n_pieces == 0) {
    // nothing was packed: the header or the carry, then the closing block of Writer::close by hand -- BFINAL = 1,
    // BTYPE = 00 at the end bit, zeros to the byte's end, LEN = 0, NLEN = 0xffff
    const uint64_t b0 = end_bit >> 3, b1 = (end_bit + 3u + 7u) >> 3;
    uint8_t first = 0;
    if (Q.header) {
      for (uint32_t k = 0; k < one_writer_header_len(Q.wrap); ++k) buf[k] = header_byte(Q.wrap, k);
    } else {
      first = (uint8_t)(st->carry & ((1u << st->carry_bits) - 1u));
    }
    buf[b0] = (uint8_t)(first | (1u << (end_bit & 7u)));
    if (b1 - b0 == 2) buf[b0 + 1] = 0;
    buf[b1] = 0, buf[b1 + 1] = 0, buf[b1 + 2] = 0xff, buf[b1 + 3] = 0xff;
  }
  // the running checksum and length: the part's sum joined behind them (checksum_clip.h)
  const uint64_t total = st->total_in + Q.in_used;
  uint32_t sum = st->sum;
  if (Q.wrap == FLATE_HIP_WRAP_GZIP && Q.in_used) {
    sum = crc_join(T, sum, (uint32_t)Q.in_used, st->part_sum);
  } else if (Q.wrap == FLATE_HIP_WRAP_ZLIB && Q.in_used) {
    const AdlerTerm a = adler_concat_term(sum, st->total_in, Q.in_used);
    const AdlerTerm b = adler_concat_term(st->part_sum, Q.in_used, 0);
    sum = adler_concat_finish((uint64_t)a.d1 + b.d1, (uint64_t)a.d2 + b.d2, total);
  }
  if (Q.close && tl) {  // the trailer behind the closing block, byte by byte
    uint8_t *t = buf + (e.whole - tl);
    if (Q.wrap == FLATE_HIP_WRAP_GZIP) {
      for (uint32_t k = 0; k < 4; ++k) t[k] = (uint8_t)(sum >> (8 * k)), t[4 + k] = (uint8_t)((uint32_t)total >> (8 * k));
    } else {
      for (uint32_t k = 0; k < 4; ++k) t[k] = (uint8_t)(sum >> (24 - 8 * k));
    }
  }
  r.status = Q.close ? FLATE_HIP_STREAM_END : FLATE_HIP_OK;
  r.out_len = e.whole;
  r.end_bit = one_writer_abs_bit(end_bit, st->emitted, Q.wrap);
  st->carry_bits = e.carry_bits;
  st->carry = e.carry_bits ? (uint32_t)buf[e.whole] & ((1u << e.carry_bits) - 1u) : 0u;
  st->emitted += e.whole;
  st->total_in = total;
  st->sum = sum;
  st->res = r;
}

// buf[0, out_len) -> out, for a call that delivered (status 0 or FLATE_HIP_STREAM_END): byte stores up to the
// destination's 16-byte grid and behind its last whole chunk, 16-byte stores between, the source read in aligned
// 16-byte chunks and shifted (buf is 16-byte aligned and has 16 readable bytes behind out_len).  Grid-stride.
__global__ __launch_bounds__(256) void one_writer_copy_kernel(const OneWriterState *st, const uint8_t *buf, uint8_t *out) {
  if (st->res.status < 0) return;
  const uint64_t len = st->res.out_len;
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x, lanes = (uint64_t)gridDim.x * 256u;
  uint64_t head = (16u - (reinterpret_cast<uintptr_t>(out) & 15u)) & 15u;
  if (head > len) head = len;
  const uint64_t chunks = (len - head) >> 4;
  const uint64_t tail_at = head + 16u * chunks;
  const uint64_t edge = head + (len - tail_at);  // the bytes off the destination's grid: at most 30
  if (t < edge) {
    const uint64_t at = t < head ? t : tail_at + (t - head);
    out[at] = buf[at];
  }
  uint4 *d = reinterpret_cast<uint4 *>(out + head);
  const uint4 *sa = reinterpret_cast<const uint4 *>(buf);  // chunk j of the destination is buf[head + 16 j, + 16)
  const uint32_t b = 8u * (uint32_t)(head & 3u);
  switch (head >> 2) {  // (uniform over the launch)
    case 0: copy_body<0>(d, sa, b, chunks, t, lanes); break;
    case 1: copy_body<1>(d, sa, b, chunks, t, lanes); break;
    case 2: copy_body<2>(d, sa, b, chunks, t, lanes); break;
    default: copy_body<3>(d, sa, b, chunks, t, lanes); break;
  }
}

}  // namespace flate
