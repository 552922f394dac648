// frame_kernels.hip -- zlib (RFC 1950) and gzip (RFC 1952) members around the raw streams of a batch, written on
// the device (flate_hip_deflate_fast_batch_framed / _spliced_framed; SURVEY 8f-3: the reference has neither).
//
// Member i = header | raw DEFLATE stream i | trailer.  The entropy stage knows the exact size of every raw stream
// before a byte of it is written (huff_code_kernel), so the members' places follow from a scan like the raw
// form's, and the pack kernels write every stream straight into its member:
//   frame_scan_kernel   scan_sizes_kernel with header + trailer added to every size: member offsets (returned to
//                       the caller) and payload offsets (= member offset + header length: what the pack kernels
//                       read as HuffParams::out_off);
//   frame_write_kernel  the header and trailer bytes of every member, one thread each, byte by byte -- a member
//                       starts at any alignment, and an empty stream's member (11 or 23 bytes) shares its dwords
//                       with its neighbours.  It runs AFTER the pack kernel: in the spliced form that kernel works
//                       on the dword grid around the raw stream (it ORs into the dword that holds the header's last
//                       bytes and stores the whole last dword, up to 3 bytes into the trailer); what is written
//                       last is right by construction.
// The checksums are checksum.hip's, left in device memory (checksum_device).  Neither kernel matters for the time
// of a call: 18 bytes per member against the member itself.
#include <hip/hip_runtime.h>

#include "flate_hip.h"
#include "flate_kernels.h"

namespace flate {

namespace {

// bytes in front of / behind stream i's raw stream
__device__ inline uint32_t header_len(const FrameParams &P, uint32_t i) {
  if (P.wrap == FLATE_HIP_WRAP_GZIP) return 10u;
  return (P.dict_of && P.dict_of[i] != FLATE_HIP_NO_DICT) ? 6u : 2u;
}
__device__ inline uint32_t trailer_len(const FrameParams &P) { return P.wrap == FLATE_HIP_WRAP_GZIP ? 8u : 4u; }

__device__ inline void put_be32(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}
__device__ inline void put_le32(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}

}  // namespace

// Exclusive scan of the members' sizes (one workgroup, as scan_sizes_kernel; the same status word).
__global__ __launch_bounds__(1024) void frame_scan_kernel(FrameParams P) {
  __shared__ uint64_t wtot[16];
  __shared__ uint64_t carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t hi = P.n_streams;
  const uint32_t tl = trailer_len(P);
  if (tid == 0) carry_s = 0ull;
  __syncthreads();
  for (uint32_t base = 0; base < hi; base += 1024) {
    const uint32_t i = base + (uint32_t)tid;
    const uint32_t hl = i < hi ? header_len(P, i) : 0u;
    const uint64_t v = i < hi ? P.out_len[i] + hl + tl : 0ull;
    uint64_t x = v;
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t o = __shfl_up(x, d);
      if (lane >= d) x += o;
    }
    if (lane == 63) wtot[wid] = x;
    __syncthreads();
    uint64_t woff = 0;
    for (int w = 0; w < wid; ++w) woff += wtot[w];
    const uint64_t carry = carry_s;
    if (i < hi) {
      const uint64_t at = carry + woff + x - v;
      P.member_off[i] = at;
      P.payload_off[i] = at + hl;
    }
    __syncthreads();
    if (tid == 1023) carry_s = carry + woff + x;
    __syncthreads();
  }
  if (tid == 0) {
    P.member_off[P.n_streams] = carry_s;
    P.payload_off[P.n_streams] = carry_s;
    if (carry_s > P.out_cap) *P.status = FLATE_HIP_E_OUT_TOO_SMALL;
  }
}

__global__ __launch_bounds__(256) void frame_write_kernel(FrameParams P) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t members = P.member_off ? P.n_streams : 1u;
  if (i >= members || *P.status != 0) return;  // (a status: the scan found the output too small -- nothing may be written)
  const bool one = P.member_off == nullptr;
  const uint32_t hl = one ? (P.wrap == FLATE_HIP_WRAP_GZIP ? 10u : 2u) : header_len(P, i);
  const uint64_t at = one ? 0ull : P.member_off[i];
  const uint64_t raw = P.out_len[i];
  const uint64_t in_len = one ? P.one_len : P.in_off[i + 1] - P.in_off[i];
  if (at + hl + raw + trailer_len(P) > P.out_cap) return;  // (never: the scan kernels have checked the total)
  uint8_t *h = P.out + at;
  uint8_t *t = h + hl + raw;
  const uint32_t sum = P.sums[i];
  if (P.wrap == FLATE_HIP_WRAP_GZIP) {
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
    if (hl == 6u) {
      h[1] = 0x3f;
      put_be32(h + 2, P.dict_id[P.dict_of[i]]);
    } else {
      h[1] = 0x01;
    }
    put_be32(t, sum);
  }
}

}  // namespace flate
