// frame_kernels.hip -- zlib (RFC 1950) and gzip (RFC 1952) members around the raw streams of a batch, written on
// the device (flate_hip_deflate_fast_batch_framed / _spliced_framed; SURVEY 8f-3: the reference has neither).
//
// Member i = header | raw DEFLATE stream i | trailer.  The entropy stage knows the exact size of every raw stream
// before a byte of it is written (huff_code_kernel), so the members' places follow from a scan like the raw
// form's, and the pack kernels write every stream straight into its member:
//   frame_scan_kernel   scan_sizes_kernel with header + trailer added to every size (scan_range of block_scan.h):
//                       member offsets (returned to the caller) and payload offsets (= member offset + header
//                       length: what the pack kernels read as HuffParams::out_off);
//   frame_write_kernel  the header and trailer bytes of every member, one thread each, byte by byte -- a member
//                       starts at any alignment, and an empty stream's member (11 or 23 bytes) shares its dwords
//                       with its neighbours.  It runs AFTER the pack kernel: in the spliced form that kernel works
//                       on the dword grid around the raw stream (it ORs into the dword that holds the header's last
//                       bytes and stores the whole last dword, up to 3 bytes into the trailer); what is written
//                       last is right by construction.
// The checksums are checksum.hip's, left in device memory (checksum_device).  Neither kernel matters for the time
// of a call: 18 bytes per member against the member itself.
// READING members (flate_hip_inflate_batch_framed) is the other half of the file: frame_parse_kernel in front of the
// batch decoders (header rules, the raw stream's range, the trailer's values, the DICTID's dictionary) and
// frame_verdict_kernel behind them and behind the checksums of what they produced (flate_kernels.h: FrameReadParams).
// ONE member around a spliced stream (flate_hip_inflate_spliced_framed): the same parse kernel over one range, then
// frame_rebase_kernel (the index moved behind the header) and frame_verdict_spliced_kernel (FrameSplicedParams).
#include <hip/hip_runtime.h>

#include "bgzf_rule.h"
#include "block_scan.h"
#include "flate_hip.h"
#include "flate_kernels.h"
#include "gzip_rule.h"

namespace flate {

namespace {

// bytes in front of / behind stream i's raw stream
__device__ inline uint32_t header_len(const FrameParams &P, uint32_t i) {
  return frame_header_len(P.wrap, P.wrap == FLATE_HIP_WRAP_ZLIB && P.dict_of && P.dict_of[i] != FLATE_HIP_NO_DICT);
}
__device__ inline uint32_t trailer_len(const FrameParams &P) { return frame_trailer_len(P.wrap); }

__device__ inline void put_be32(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}
__device__ inline void put_le32(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}

}  // namespace

// Exclusive scan of the members' sizes (one workgroup, block_scan.h; scan_sizes_kernel's status word).
__global__ __launch_bounds__(1024) void frame_scan_kernel(FrameParams P) {
  __shared__ uint64_t wtot[16];
  __shared__ uint32_t big_s;  // kWrapBgzf: the first member that BSIZE cannot express
  const uint32_t tl = trailer_len(P);
  if (threadIdx.x == 0) big_s = 0xffffffffu;
  __syncthreads();
  const uint64_t sum = scan_range<16, uint64_t>(
      P.n_streams, wtot,
      [&](uint32_t i) {
        const uint64_t v = P.out_len[i] + header_len(P, i) + tl;
        if (frame_is_bgzf(P.wrap) && v > (uint64_t)kBgzfMemberMax) atomicMin(&big_s, i);
        return v;
      },
      [&](uint32_t i, uint64_t at, uint64_t) {
        P.member_off[i] = at;
        P.payload_off[i] = at + header_len(P, i);
      });
  if (threadIdx.x == 0) {  // (behind the scan's barriers: big_s is final)
    P.member_off[P.n_streams] = sum;
    P.payload_off[P.n_streams] = sum;
    // (a BGZF file ends with the EOF marker behind its last member; kWrapBgzfOpen: the file goes on)
    const uint64_t total = sum + (P.wrap == kWrapBgzf ? (uint64_t)kBgzfEofLen : 0ull);
    if (total > P.out_cap) *P.status = FLATE_HIP_E_OUT_TOO_SMALL;
    if (big_s != 0xffffffffu) {
      P.status[1] = (int)big_s;
      *P.status = FLATE_HIP_E_TOO_LARGE;
    }
  }
}

__global__ __launch_bounds__(256) void frame_write_kernel(FrameParams P) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t members = P.member_off ? P.n_streams : 1u;
  if (*P.status != 0) return;  // (a status: the scan found the output too small -- nothing may be written)
  if (P.wrap == kWrapBgzf && i == members) {  // the EOF marker behind the last member (the scan has counted it)
    uint8_t *e = P.out + P.member_off[members];
    for (uint32_t b = 0; b < kBgzfEofLen; ++b) e[b] = bgzf_eof_byte(b);
  }
  if (i >= members) return;
  const bool one = P.member_off == nullptr;
  const uint32_t hl = one ? frame_header_len(P.wrap, false) : header_len(P, i);
  const uint64_t at = one ? 0ull : P.member_off[i];
  const uint64_t raw = P.out_len[i];
  const uint64_t in_len = one ? P.one_len : P.in_off[i + 1] - P.in_off[i];
  if (at + hl + raw + trailer_len(P) > P.out_cap) return;  // (never: the scan kernels have checked the total)
  uint8_t *h = P.out + at;
  uint8_t *t = h + hl + raw;
  const uint32_t sum = P.sums[i];
  if (frame_is_bgzf(P.wrap)) {
    // htslib's header: FEXTRA, XLEN = 6, the subfield 'B' 'C' with BSIZE = the member's size - 1 (the scan has
    // refused the call if that does not fit 16 bits)
    const uint32_t bsize = (uint32_t)(hl + raw + trailer_len(P)) - 1u;
    for (uint32_t b = 0; b < 16u; ++b) h[b] = bgzf_header_byte(b);
    h[16] = (uint8_t)bsize, h[17] = (uint8_t)(bsize >> 8);
    put_le32(t, sum);
    put_le32(t + 4, (uint32_t)in_len);
  } else if (P.wrap == FLATE_HIP_WRAP_GZIP) {
    // ID1 ID2, CM = 8, FLG = 0, MTIME = 0, XFL = 4 (fastest), OS = 255 (unknown): RFC 1952 2.3
    h[0] = 0x1f, h[1] = 0x8b, h[2] = 8, h[3] = 0;
    h[4] = h[5] = h[6] = h[7] = 0;
    h[8] = 4, h[9] = 255;
    put_le32(t, sum);
    put_le32(t + 4, (uint32_t)in_len);
  } else {
    // CMF = 0x78 (deflate, 32 KiB window); FLG: FLEVEL = 0, FDICT, FCHECK makes CMF * 256 + FLG a multiple of 31
    // (RFC 1950 2.2): 0x01 without a dictionary, 0x3f with one
    h[0] = 0x78;
    if (hl == frame_header_len(FLATE_HIP_WRAP_ZLIB, true)) {
      h[1] = 0x3f;
      put_be32(h + 2, P.dict_id[P.dict_of[i]]);
    } else {
      h[1] = 0x01;
    }
    put_be32(t, sum);
  }
}

// The members of a grouped call (flate_hip_deflate_fast_grouped_framed; group_scan_kernel has placed them): member g's
// raw stream is spliced from the pieces of group g, whose input is contiguous.  The same bytes as above, no dictionaries.
__global__ __launch_bounds__(256) void group_frame_write_kernel(GroupFrameParams P) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= P.n_groups || *P.status != 0) return;
  const uint32_t tl = frame_trailer_len(P.wrap);
  // the raw stream ends behind its closing block: 3 bits, padding, LEN, NLEN
  const uint64_t raw_end = (((P.end_bit[g] + 3 + 7) & ~7ull) + 32) >> 3;
  if (raw_end + tl > P.out_cap) return;  // (never: the scan kernel has checked the total)
  const uint64_t in_len = P.in_off[P.group_off[g + 1]] - P.in_off[P.group_off[g]];
  uint8_t *h = P.out + P.member_off[g];
  uint8_t *t = P.out + raw_end;
  const uint32_t sum = P.sums[g];
  if (P.wrap == FLATE_HIP_WRAP_GZIP) {
    h[0] = 0x1f, h[1] = 0x8b, h[2] = 8, h[3] = 0;
    h[4] = h[5] = h[6] = h[7] = 0;
    h[8] = 4, h[9] = 255;
    put_le32(t, sum);
    put_le32(t + 4, (uint32_t)in_len);
  } else {
    h[0] = 0x78, h[1] = 0x01;
    put_be32(t, sum);
  }
}

// ---- reading members (flate_hip_inflate_batch_framed) ----

namespace {
__device__ inline uint32_t get_be32(const uint8_t *p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}
__device__ inline uint32_t get_le32(const uint8_t *p) {
  return p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
}  // namespace

// The rules are the host mirrors' (parse_container_header / zlib_member_header in engine.py, container_header in
// flate_host.hpp).  Every read is below the member's end.
__global__ __launch_bounds__(256) void frame_parse_kernel(FrameReadParams P) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P.n_streams) return;
  const uint64_t a = P.in_off[i], len = (P.in_end ? P.in_end[i] : P.in_off[i + 1]) - a;
  const uint8_t *m = P.in + a;
  uint64_t hl = 0, tl = 0;
  bool ok = false;
  uint32_t used = FLATE_HIP_NO_DICT;
  if (P.wrap == FLATE_HIP_WRAP_GZIP) {
    // RFC 1952 2.3: ID1 ID2, CM = 8, the reserved FLG bits zero; FEXTRA, FNAME, FCOMMENT, FHCRC skipped in that order
    // (the rule is gzip_rule.h's: member discovery tests every offset of a file with it)
    tl = frame_trailer_len(FLATE_HIP_WRAP_GZIP);
    hl = gzip_header_len(m, len);
    ok = hl != 0;
  } else {
    // RFC 1950 2.2: CM = 8, CINFO <= 7, FCHECK; FDICT: DICTID follows, and names the FIRST dictionary with that id
    tl = frame_trailer_len(FLATE_HIP_WRAP_ZLIB);
    if (len >= frame_header_len(FLATE_HIP_WRAP_ZLIB, false) && (m[0] & 15u) == 8u && (m[0] >> 4) <= 7u && (((uint32_t)m[0] << 8) | m[1]) % 31u == 0u) {
      if (m[1] & 0x20u) {
        if (P.n_dicts && len >= frame_header_len(FLATE_HIP_WRAP_ZLIB, true)) {
          const uint32_t id = get_be32(m + 2);
          for (uint32_t j = 0; j < P.n_dicts && !ok; ++j)
            if (P.dict_id[j] == id) used = j, ok = true;
          hl = frame_header_len(FLATE_HIP_WRAP_ZLIB, true);
        }
      } else {
        ok = true;
        hl = frame_header_len(FLATE_HIP_WRAP_ZLIB, false);
      }
    }
  }
  if (ok && len < hl + tl) ok = false;  // too short for its header plus trailer
  if (!ok) used = FLATE_HIP_NO_DICT;
  // the raw stream is exactly [header's end, trailer's start): a decoder that needs more has met the stream's end
  P.pay_off[i] = ok ? a + hl : a;
  P.pay_end[i] = ok ? a + len - tl : a;
  if (i + 1 == P.n_streams) P.pay_off[i + 1] = P.in_off[i + 1];
  P.bad[i] = ok ? 0u : 1u;
  uint32_t want = 0, isize = 0;
  if (ok) {
    const uint8_t *t = m + (len - tl);
    if (P.wrap == FLATE_HIP_WRAP_GZIP) want = get_le32(t), isize = get_le32(t + 4);
    else want = get_be32(t);
  }
  P.want[i] = want;
  P.isize[i] = isize;
  P.dict_used[i] = used;
  if (P.dict_at) {
    P.dict_at[i] = used != FLATE_HIP_NO_DICT ? P.tail_at[used] : 0ull;
    P.dict_len[i] = used != FLATE_HIP_NO_DICT ? P.tail_len[used] : 0u;
  }
}

// In this order: a bad header; the decoder's own status (left as it is, with its err_off and the bytes it produced);
// a checksum -- or, gzip, a length mod 2^32 -- that is not the trailer's.
__global__ __launch_bounds__(256) void frame_verdict_kernel(FrameReadParams P) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= P.n_streams) return;
  if (P.bad[i]) {
    P.status[i] = FLATE_HIP_E_CORRUPT;
    P.err_off[i] = 0;
    P.out_len[i] = 0;
    return;
  }
  if (P.status[i] != 0 || P.sums == nullptr) return;
  const bool mismatch = P.sums[i] != P.want[i] ||
                        (P.wrap == FLATE_HIP_WRAP_GZIP && (uint32_t)P.out_len[i] != P.isize[i]);
  if (mismatch) {
    P.status[i] = FLATE_HIP_E_CORRUPT;
    P.err_off[i] = (int64_t)((P.in_end ? P.in_end[i] : P.in_off[i + 1]) - P.in_off[i]);
  }
}

// ---- reading one member whose raw stream is spliced (flate_hip_inflate_spliced_framed; FrameSplicedParams) ----

__global__ __launch_bounds__(256) void frame_rebase_kernel(FrameSplicedParams P) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > P.n_pieces) return;
  const bool bad = P.one->bad != 0;
  const uint64_t end_bit = 8ull * P.raw_end;
  // (a good header ends at or below raw_end -- frame_parse_kernel -- and the host has kept bit_in below 2^61)
  const uint64_t bit = P.bit_in[i] + 8ull * P.one->pay_off[0];
  P.bit_out[i] = (bad || bit > end_bit) ? end_bit : bit;
  if (i < P.n_pieces) P.piece_bad[i] = bad ? 1u : 0u;
}

// One workgroup: the cases per piece, the first piece with a status of its own, then the member's two words.
__global__ __launch_bounds__(1024) void frame_verdict_spliced_kernel(FrameSplicedParams P) {
  __shared__ uint32_t first_s;
  const uint32_t tid = threadIdx.x;
  if (tid == 0) first_s = 0xffffffffu;
  __syncthreads();
  FrameOne &O = *P.one;
  const bool bad = O.bad != 0;
  const int64_t hl = (int64_t)O.pay_off[0];
  uint32_t first = 0xffffffffu;
  for (uint32_t i = tid; i < P.n_pieces; i += 1024u) {
    if (bad) {
      P.status[i] = FLATE_HIP_E_CORRUPT;
      P.err_off[i] = 0;
      P.out_len[i] = 0;
    } else {
      // a piece whose start was clamped has no input: to the decoders one that ends where it starts is an empty
      // piece, so the end of the stream is reported here (the last piece, which has no end, meets it by itself)
      if (P.status[i] == 0 && P.bit_in[i] + 8ull * (uint64_t)hl > 8ull * P.raw_end) {
        P.status[i] = FLATE_HIP_E_UNEXPECTED_EOF;
        P.err_off[i] = -1;
        P.out_len[i] = 0;
      }
      if (P.status[i] != 0) {
        if (first == 0xffffffffu) first = i;
        // (the decoders count from InfParams::in, the member's first byte)
        if (P.err_off[i] >= 0) P.err_off[i] = P.err_off[i] >= hl ? P.err_off[i] - hl : 0;
      }
    }
  }
  if (first != 0xffffffffu) atomicMin(&first_s, first);
  __syncthreads();
  if (tid != 0) return;
  // (the trailer's two tests are folded into one flag with plain arithmetic before anything branches on them, and
  // the error offset is chosen by that flag alone: written as `a || (gzip && b)` in the chain of cases below, the
  // compiler in use kept the offset at -1 on the path where only the ISIZE differs)
  const uint32_t isize_off = P.wrap == FLATE_HIP_WRAP_GZIP ? ((uint32_t)O.total ^ O.isize) : 0u;
  const bool mismatch = ((O.sum ^ O.want) | isize_off) != 0u;
  const uint32_t first_bad = first_s;
  int32_t ms = 0;
  int64_t me = -1;
  if (bad) {
    ms = FLATE_HIP_E_CORRUPT;
    me = 0;
  } else if (first_bad != 0xffffffffu) {
    ms = P.status[first_bad];
  } else if (mismatch) {
    ms = FLATE_HIP_E_CORRUPT;
    me = (int64_t)P.in_len;
  }
  O.member_status = ms;
  O.member_err_off = me;
}

}  // namespace flate
