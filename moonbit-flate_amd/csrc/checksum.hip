// checksum.hip -- Adler-32 and CRC-32 of a batch of streams, for the container formats that wrap a raw
// DEFLATE stream ("optional gzip/zlib wrappers (absent from reference)"; RFC 1950 section 8.2,
// RFC 1952 section 8).  The reference has neither; the checker is oracle/checksum.c, pinned against zlib.
//
// Both checksums are linear in the right sense, so the work is cut into PIECES of 64 KiB regardless of how
// long a stream is (one stream of 1 GiB and 16384 streams of 64 KiB fill the chip alike):
//   checksum_piece_kernel  one wavefront per piece.  A FULL piece is read in 64 coalesced rows of 1 KiB, lane
//       L taking bytes [16 L, 16 L + 16) of every row:
//       CRC-32   the lane carries the raw (zero-initialised, hence linear) CRC of its sixteen-byte pieces as if
//                they were contiguous: per row a multiplication by x^(8 * 1008) (the gap; four table lookups)
//                and slicing-by-4 over the row's four dwords (sixteen lookups; eight 1 KiB tables in LDS); at
//                the end a multiplication by x^(8 * bytes behind the lane's last piece), XOR over the lanes,
//                and the pre-/post-inversion as a term that depends on the length only
//                (crc(A || B) = crc(A) * x^(8 |B|) + crc(B): zlib's crc32_combine);
//       Adler-32 sum of the bytes and sum of (index * byte) per lane (v_dot4), added over the lanes.
//       The last, shorter piece of a stream: lane L takes bytes [1024 L, 1024 L + 1024) of it instead;
//   checksum_fold_kernel   one wavefront per stream folds its pieces: 64 runs of consecutive pieces, one per
//       lane, then the lanes;
//   checksum_join_kernel   one workgroup joins the finished sums of the pieces of a spliced stream into the sum of
//       their concatenation (flate_hip_inflate_spliced_framed).
// One read of the input; what bounds the kernels is stated in DESIGN 4.7.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <stdexcept>
#include <vector>

#include <string>

#include "block_scan.h"
#include "carve.h"
#include "checksum_clip.h"
#include "flate_hip.h"
#include "flate_kernels.h"

namespace flate {

namespace {

constexpr uint32_t kPiece = kSumPiece;  // bytes per wavefront and step (checksum_clip.h)
constexpr uint32_t kChunk = 1024;   // bytes per lane of it
constexpr uint32_t kPoly = kSumPoly;
constexpr uint32_t kAdlerMod = kSumAdlerMod;

struct PieceParams {
  const uint8_t *in;
  const uint64_t *piece_off;  // absolute offset of every piece in `in`
  const uint32_t *piece_len;  // 1 .. kPiece; 0: a piece planned over a slot, beyond what its stream produced
  uint32_t n_pieces;
  uint32_t want_crc, want_adler;
  uint32_t *crc;      // per piece
  uint32_t *asum;     // per piece: sum of its bytes
  uint64_t *wsum;     // per piece: sum of (index inside the piece) * byte
  X2n x2n;
};

__device__ inline uint32_t ld32u(const uint8_t *p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// my bytes [1024 L, 1024 L + 1024) of a piece shorter than kPiece (a stream's last one)
__device__ inline void short_piece(const PieceParams &P, const uint32_t (*T)[256], uint32_t pc, int lane) {
  const uint32_t len = P.piece_len[pc];
  const uint8_t *src = P.in + P.piece_off[pc];
  const uint32_t start = kChunk * (uint32_t)lane;
  const uint32_t clen = len > start ? (len - start < kChunk ? len - start : kChunk) : 0u;
  const uint8_t *p = src + start;
  uint32_t c = 0xffffffffu;
  uint32_t a = 0;  // sum of my bytes (<= 1024 * 255)
  uint32_t w = 0;  // sum of (index inside my chunk) * byte (< 2^28)
  uint32_t i = 0;
  for (; i + 16 <= clen; i += 16) {
    uint4 q;
    __builtin_memcpy(&q, p + i, 16);
    const uint32_t d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (P.want_crc) {
        c ^= d[k];
        c = T[3][c & 255u] ^ T[2][(c >> 8) & 255u] ^ T[1][(c >> 16) & 255u] ^ T[0][c >> 24];
      }
      if (P.want_adler) {
        const uint32_t s4 = __builtin_amdgcn_udot4(d[k], 0x01010101u, 0u, false);
        a += s4;
        w = __builtin_amdgcn_udot4(d[k], 0x03020100u, w, false) + (i + 4u * k) * s4;
      }
    }
  }
  for (; i < clen; ++i) {
    const uint32_t b = p[i];
    if (P.want_crc) c = T[0][(c ^ b) & 255u] ^ (c >> 8);
    a += b;
    w += i * b;
  }
  if (P.want_crc) {
    c = clen ? c ^ 0xffffffffu : 0u;  // (the CRC of no bytes is 0)
    if (clen) c = multmodp(x2nmodp(P.x2n, len - (start + clen), 3), c);
    for (int d = 32; d >= 1; d >>= 1) c ^= (uint32_t)__shfl_xor((int)c, d);
    if (lane == 0) P.crc[pc] = c;
  }
  if (P.want_adler) {
    uint64_t ww = (uint64_t)w + (uint64_t)start * a;
    uint32_t aa = a;
    for (int d = 32; d >= 1; d >>= 1) {
      aa += (uint32_t)__shfl_xor((int)aa, d);
      ww += (uint64_t)__shfl_xor((long long)ww, d);
    }
    if (lane == 0) {
      P.asum[pc] = aa;
      P.wsum[pc] = ww;
    }
  }
}

__global__ __launch_bounds__(256) void checksum_piece_kernel(PieceParams P) {
  // T: slicing-by-4 tables (RFC 1952 section 8's table and three shifted copies); S: the same four byte
  // positions multiplied by x^(8 * 1008) -- the bytes between two of a lane's sixteen-byte pieces
  __shared__ uint32_t T[4][256], S[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  {
    uint32_t c = (uint32_t)tid;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? kPoly ^ (c >> 1) : c >> 1;
    T[0][tid] = c;
    __syncthreads();
    uint32_t v = c;
    for (int k = 1; k < 4; ++k) {
      v = (v >> 8) ^ T[0][v & 255u];
      T[k][tid] = v;
    }
    if (P.want_crc) {
      const uint32_t xgap = x2nmodp(P.x2n, kChunk - 16u, 3);
      for (int k = 0; k < 4; ++k) S[k][tid] = multmodp(xgap, (uint32_t)tid << (8 * k));
    }
    __syncthreads();
  }
  // x^(8 * bytes behind my last sixteen-byte piece of a full piece), and the inversions' term of a full piece
  const uint32_t xlane = P.want_crc ? x2nmodp(P.x2n, 16u * (uint32_t)(63 - lane), 3) : 0u;
  const uint32_t inv_full = P.want_crc ? multmodp(x2nmodp(P.x2n, kPiece, 3), 0xffffffffu) ^ 0xffffffffu : 0u;
  const uint32_t waves = gridDim.x * 4u;
  for (uint32_t pc = blockIdx.x * 4u + (uint32_t)wid; pc < P.n_pieces; pc += waves) {
    if (P.piece_len[pc] != kPiece) {
      short_piece(P, T, pc, lane);
      continue;
    }
    const uint8_t *src = P.in + P.piece_off[pc] + 16u * (uint32_t)lane;
    uint32_t c = 0;            // raw CRC of my pieces so far, as if contiguous
    uint32_t a = 0;            // sum of my bytes (<= 64 * 16 * 255)
    uint32_t w1 = 0, w2 = 0;   // sum over rows of row * (row's bytes); sum of (index inside the 16) * byte
#pragma unroll 4
    for (uint32_t r = 0; r < kPiece / kChunk; ++r) {
      uint4 q;
      __builtin_memcpy(&q, src + kChunk * r, 16);
      const uint32_t d[4] = {q.x, q.y, q.z, q.w};
      if (P.want_crc) {
        c = S[0][c & 255u] ^ S[1][(c >> 8) & 255u] ^ S[2][(c >> 16) & 255u] ^ S[3][c >> 24];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          c ^= d[k];
          c = T[3][c & 255u] ^ T[2][(c >> 8) & 255u] ^ T[1][(c >> 16) & 255u] ^ T[0][c >> 24];
        }
      }
      if (P.want_adler) {
        uint32_t ar = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t s4 = __builtin_amdgcn_udot4(d[k], 0x01010101u, 0u, false);
          ar += s4;
          w2 = __builtin_amdgcn_udot4(d[k], 0x03020100u, w2, false) + 4u * k * s4;
        }
        a += ar;
        w1 += r * ar;
      }
    }
    if (P.want_crc) {
      c = multmodp(xlane, c);
      for (int d = 32; d >= 1; d >>= 1) c ^= (uint32_t)__shfl_xor((int)c, d);
      if (lane == 0) P.crc[pc] = c ^ inv_full;
    }
    if (P.want_adler) {
      uint64_t ww = (uint64_t)kChunk * w1 + (uint64_t)(16u * (uint32_t)lane) * a + w2;
      uint32_t aa = a;
      for (int d = 32; d >= 1; d >>= 1) {
        aa += (uint32_t)__shfl_xor((int)aa, d);
        ww += (uint64_t)__shfl_xor((long long)ww, d);
      }
      if (lane == 0) {
        P.asum[pc] = aa;
        P.wsum[pc] = ww;
      }
    }
  }
}

struct FoldParams {
  const uint64_t *in_off;      // n_streams + 1
  const uint32_t *piece_base;  // n_streams + 1: first piece of every stream
  const uint32_t *piece_len;
  const uint32_t *crc;
  const uint32_t *asum;
  const uint64_t *wsum;
  uint32_t *out;  // per stream
  uint32_t n_streams;
  uint32_t want_crc;  // else Adler-32
  uint32_t max_pieces;  // pieces of the longest stream
  const uint64_t *n_len;  // per stream: its bytes where the pieces were planned over slots and clipped on the device
                          // (checksum_clip_kernel); null: in_off[s + 1] - in_off[s]
  X2n x2n;
};

// One wavefront per stream: lane L folds the run of pieces [p0 + L r, p0 + (L + 1) r), then the lanes are
// folded (every piece but a stream's last is kPiece long, so a run's place in the stream is known).
__global__ __launch_bounds__(256) void checksum_fold_kernel(FoldParams P) {
  // K[k][b] = (b << 8k) * x^(8 * kPiece) mod P: a full piece's step of the CRC fold as four lookups instead of
  // a 32-step multiplication (one long stream: 16384 pieces, 256 per lane)
  __shared__ uint32_t K[4][256];
  const int lane = threadIdx.x & 63;
  const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
  const bool tables = P.want_crc && P.max_pieces > 256u;  // (uniform: worth the 1024 multiplications per block)
  if (tables) {
    const uint32_t xp = x2nmodp(P.x2n, kPiece, 3);
    for (int k = 0; k < 4; ++k) K[k][threadIdx.x] = multmodp(xp, (uint32_t)threadIdx.x << (8 * k));
    __syncthreads();
  }
  if (s >= P.n_streams) return;
  const uint32_t p0 = P.piece_base[s], p1 = P.piece_base[s + 1];
  const uint64_t n = P.n_len ? P.n_len[s] : P.in_off[s + 1] - P.in_off[s];
  // (clipped pieces: a piece may be empty and a run may lie beyond the data -- fold_run keeps `start` within n)
  const FoldRun R = fold_run(p1 - p0, (uint32_t)lane, n);
  const uint32_t k0 = p0 + R.k0, k1 = p0 + R.k1;
  if (P.want_crc) {
    const uint32_t xpiece = x2nmodp(P.x2n, kPiece, 3);
    uint32_t c = 0;
    uint64_t end = R.start;  // bytes of the stream in front of my run, then behind its pieces
    for (uint32_t k = k0; k < k1; ++k) {
      const uint32_t len = P.piece_len[k];
      if (len == kPiece && tables)
        c = K[0][c & 255u] ^ K[1][(c >> 8) & 255u] ^ K[2][(c >> 16) & 255u] ^ K[3][c >> 24];
      else
        c = multmodp(len == kPiece ? xpiece : x2nmodp(P.x2n, len, 3), c);
      c ^= P.crc[k];
      end += len;
    }
    if (k1 > k0) c = crc_place(P.x2n, c, n - end);
    for (int d = 32; d >= 1; d >>= 1) c ^= (uint32_t)__shfl_xor((int)c, d);
    if (lane == 0) P.out[s] = c;
  } else {
    // s1 = 1 + sum b;  s2 = n + sum (n - i) b_i = n + n * sum b - sum i b_i   (all mod 65521, RFC 1950 8.2)
    uint64_t sa = 0, sib = 0, base = R.start;
    for (uint32_t k = k0; k < k1; ++k) {
      const uint64_t a = P.asum[k];
      sa = (sa + a) % kAdlerMod;
      sib = (sib + (base % kAdlerMod) * (a % kAdlerMod) + P.wsum[k] % kAdlerMod) % kAdlerMod;
      base += P.piece_len[k];
    }
    for (int d = 32; d >= 1; d >>= 1) {
      sa += (uint64_t)__shfl_xor((long long)sa, d);
      sib += (uint64_t)__shfl_xor((long long)sib, d);
    }
    if (lane == 0) P.out[s] = adler_finish(sa, sib, n);
  }
}

// Pieces planned over output SLOTS (flate_hip_inflate_batch_framed: what a stream produced is known on the device
// only): one wavefront per stream clips its pieces to the bytes produced -- never more than the slot holds -- and
// leaves that length for the fold.  A stream with a verdict already (a bad header, a decoder status) needs no sum:
// its pieces are empty.
struct ClipParams {
  const uint64_t *slot_off;    // n_streams + 1
  const uint32_t *piece_base;  // n_streams + 1
  const uint64_t *produced;    // per stream: out_len of the decoder
  const int32_t *status;       // per stream: the decoder's
  const uint32_t *bad;         // per stream: non-zero = bad header
  uint32_t *piece_len;
  uint64_t *n_len;
  uint32_t n_streams;
};
__global__ __launch_bounds__(256) void checksum_clip_kernel(ClipParams P) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (s >= P.n_streams) return;
  const uint64_t slot = P.slot_off[s + 1] - P.slot_off[s];
  uint64_t n = P.produced[s] < slot ? P.produced[s] : slot;
  if (P.status[s] != 0 || P.bad[s] != 0) n = 0;
  const uint32_t p0 = P.piece_base[s], np = P.piece_base[s + 1] - p0;
  for (uint32_t k = lane; k < np; k += 64u) P.piece_len[p0 + k] = clip_piece_len(n, k);
  if (lane == 0) P.n_len[s] = n;
}

// The sum of a CONCATENATION (flate_hip_inflate_spliced_framed): the n pieces of a spliced stream each left a finished
// sum (checksum_fold_kernel) of the L_i = min(out_len[i], slot) bytes they produced; the member's checksum is that of
// the L_i-byte runs one after another.  Piece i's term needs the bytes BEHIND it, n_bytes - (L_0 + .. + L_i): one
// workgroup first adds up n_bytes, then walks the pieces with a running prefix (scan_range of block_scan.h, as
// frame_scan_kernel walks sizes); every thread keeps the XOR (CRC-32) or the two sums mod 65521 (Adler-32) of its
// terms, folded over the workgroup at the end.  The arithmetic is checksum_clip.h's.  2^20 pieces: 1024 chunks of at
// most ~40 multmodp per thread -- nothing against the decode in front of it.
struct JoinParams {
  const uint32_t *sums;      // per piece: its finished Adler-32 / CRC-32
  const uint64_t *slot_off;  // n_pieces + 1
  const uint64_t *produced;  // per piece: out_len of the decoder
  uint32_t n_pieces;
  uint32_t want_crc;  // else Adler-32
  uint32_t *sum;      // the whole's
  uint64_t *total;    // its bytes (gzip: ISIZE is this mod 2^32)
  X2n x2n;
};
__global__ __launch_bounds__(1024) void checksum_join_kernel(JoinParams P) {
  __shared__ uint64_t wtot[16], wd1[16], wd2[16];
  __shared__ uint32_t wcrc[16];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const uint32_t hi = P.n_pieces;
  auto len_of = [&](uint32_t i) { return clip_to_slot(P.produced[i], P.slot_off[i + 1] - P.slot_off[i]); };
  // the whole's bytes
  uint64_t mine = 0;
  for (uint32_t i = (uint32_t)tid; i < hi; i += 1024u) mine += len_of(i);
  for (int d = 32; d >= 1; d >>= 1) mine += (uint64_t)__shfl_xor((long long)mine, d);
  if (lane == 0) wtot[wid] = mine;
  __syncthreads();
  uint64_t n_bytes = 0;
  for (int w = 0; w < 16; ++w) n_bytes += wtot[w];
  __syncthreads();
  // the terms
  uint32_t c = 0;
  uint64_t d1 = 0, d2 = 0;
  (void)scan_range<16, uint64_t>(hi, wtot, len_of, [&](uint32_t i, uint64_t before, uint64_t v) {
    const uint64_t upto = before + v;  // L_0 + .. + L_i: never more than n_bytes
    const uint64_t behind = n_bytes - upto;
    if (P.want_crc) {
      c ^= crc_concat_term(P.x2n, P.sums[i], v, behind);
    } else {
      const AdlerTerm t = adler_concat_term(P.sums[i], v, behind);
      d1 = (d1 + t.d1) % kAdlerMod;
      d2 = (d2 + t.d2) % kAdlerMod;
    }
  });
  for (int d = 32; d >= 1; d >>= 1) {
    c ^= (uint32_t)__shfl_xor((int)c, d);
    d1 += (uint64_t)__shfl_xor((long long)d1, d);
    d2 += (uint64_t)__shfl_xor((long long)d2, d);
  }
  if (lane == 0) wcrc[wid] = c, wd1[wid] = d1, wd2[wid] = d2;
  __syncthreads();
  if (tid == 0) {
    c = 0, d1 = 0, d2 = 0;
    for (int w = 0; w < 16; ++w) c ^= wcrc[w], d1 += wd1[w], d2 += wd2[w];
    *P.sum = P.want_crc ? c : adler_concat_finish(d1, d2, n_bytes);
    *P.total = n_bytes;
  }
}

}  // namespace

}  // namespace flate

using namespace flate;

namespace {
// checksum_device's arrays in slot 0 of the ctx's scratch, for np pieces of n streams; bytes: of all of them
struct Arrays {
  uint64_t *poff, *wsum, *ioff, *nlen;
  uint32_t *plen, *pbase, *crc, *asum;
  size_t bytes;
  Arrays(void *base, size_t np, size_t n) {
    flate_host::Carve k{base};
    k.take(poff, np), k.take(wsum, np), k.take(ioff, n + 1), k.take(plen, np + 1);
    k.take(pbase, n + 2), k.take(crc, np), k.take(asum, np), k.take(nlen, n + 1);
    bytes = k.at;
  }
};
size_t count_pieces(const uint64_t *in_off, uint32_t n) {
  uint64_t np = 0;
  for (uint32_t i = 0; i < n; ++i) np += (in_off[i + 1] - in_off[i] + kPiece - 1) / kPiece;
  return (size_t)np;
}
}  // namespace

size_t flate::checksum_scratch_bytes(const uint64_t *in_off, uint32_t n) { return Arrays(nullptr, count_pieces(in_off, n), n).bytes; }

// uploads of one checksum_device call through the ctx's staging: piece offsets and lengths, piece_base, in_off
size_t flate::checksum_ctl_up_bytes(const uint64_t *in_off, uint32_t n) {
  return count_pieces(in_off, n) * 12 + ((size_t)n + 1) * 12 + 4 * 512;
}

// The kernels of flate_hip_checksum_batch on input that is on the device already; the sums stay there (flate_kernels.h).
namespace {
// what the decoder left on the device for checksum_device_clipped (null: the pieces are the streams')
struct Produced {
  const uint64_t *out_len;
  const int32_t *status;
  const uint32_t *bad;
};
int checksum_run(flate_hip_ctx *c, const uint8_t *d_in, const uint64_t *in_off, uint32_t n, uint32_t kind,
                 uint32_t *d_sums, int stage, const Produced *clip);
}  // namespace

int flate::checksum_device(flate_hip_ctx *c, const uint8_t *d_in, const uint64_t *in_off, uint32_t n, uint32_t kind,
                           uint32_t *d_sums, int stage) {
  return checksum_run(c, d_in, in_off, n, kind, d_sums, stage, nullptr);
}

// The same over what a decoder PRODUCED in its output slots (flate_kernels.h): the pieces are planned over the slots
// slot_off, which the host knows, and clipped on the device to out_len[i].
int flate::checksum_device_clipped(flate_hip_ctx *c, const uint8_t *d_out, const uint64_t *slot_off, uint32_t n,
                                   uint32_t kind, const uint64_t *d_out_len, const int32_t *d_status,
                                   const uint32_t *d_bad, uint32_t *d_sums) {
  const Produced clip{d_out_len, d_status, d_bad};
  return checksum_run(c, d_out, slot_off, n, kind, d_sums, -1, &clip);
}

// The pieces' sums joined into the sum of their concatenation (flate_kernels.h); queued behind checksum_device_clipped.
int flate::checksum_join_device(flate_hip_ctx *c, const uint32_t *d_sums, const uint64_t *d_slot_off,
                                const uint64_t *d_out_len, uint32_t n, uint32_t kind, uint32_t *d_sum,
                                uint64_t *d_total) {
  JoinParams J{};
  J.sums = d_sums;
  J.slot_off = d_slot_off;
  J.produced = d_out_len;
  J.n_pieces = n;
  J.want_crc = kind == FLATE_HIP_CHECKSUM_CRC32;
  J.sum = d_sum;
  J.total = d_total;
  J.x2n = make_x2n();
  hipLaunchKernelGGL(checksum_join_kernel, dim3(1), dim3(1024), 0, ctx_stream(c), J);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    ctx_set_error(c, std::string("checksum join kernel: ") + hipGetErrorString(e));
    return FLATE_HIP_E_HIP;
  }
  return FLATE_HIP_OK;
}

namespace {
int checksum_run(flate_hip_ctx *c, const uint8_t *d_in, const uint64_t *in_off, uint32_t n, uint32_t kind,
                 uint32_t *d_sums, int stage, const Produced *clip) {
  if (n == 0) return FLATE_HIP_OK;
  auto hip_fail = [&](const char *what) -> int {
    ctx_set_error(c, std::string(what) + ": " + hipGetErrorString(hipGetLastError()));
    return FLATE_HIP_E_HIP;
  };
  hipStream_t st = ctx_stream(c);
  // pieces.  (The vectors may throw: nothing may cross the extern "C" boundary -- see the catch at the end.)
  try {
  std::vector<uint64_t> poff;
  std::vector<uint32_t> plen, pbase(n + 1, 0);
  for (uint32_t i = 0; i < n; ++i) {
    pbase[i] = (uint32_t)plen.size();
    for (uint64_t o = in_off[i]; o < in_off[i + 1]; o += kPiece) {
      poff.push_back(o);
      plen.push_back((uint32_t)(in_off[i + 1] - o < kPiece ? in_off[i + 1] - o : kPiece));
      if (plen.size() >= 0xfffffff0u) return FLATE_HIP_E_TOO_LARGE;
    }
  }
  pbase[n] = (uint32_t)plen.size();
  const uint32_t np = (uint32_t)plen.size();
  // one grow-only scratch of the ctx, carved into the call's arrays (round 4 did nine hipMalloc / hipFree
  // pairs per call: hipFree drains the whole device, i.e. every other context and the host pipelines' lanes)
  void *base = nullptr;
  {
    const int rc = ctx_scratch(c, 0, Arrays(nullptr, np, n).bytes, &base);
    if (rc != FLATE_HIP_OK) return rc;
  }
  const Arrays d(base, np, n);
  // the index arrays travel through the ctx's pinned staging and its copy kernel, not through DMA
  // commands that queue behind whatever bulk copy another thread has in flight (flate_api.hip: ctl_up)
  {
    int rc = ctx_ctl_up(c, d.poff, poff.data(), (size_t)np * 8);
    if (rc == FLATE_HIP_OK && !clip) rc = ctx_ctl_up(c, d.plen, plen.data(), (size_t)np * 4);
    if (rc == FLATE_HIP_OK) rc = ctx_ctl_up(c, d.pbase, pbase.data(), ((size_t)n + 1) * 4);
    if (rc == FLATE_HIP_OK) rc = ctx_ctl_up(c, d.ioff, in_off, ((size_t)n + 1) * 8);
    if (rc != FLATE_HIP_OK) return rc;
  }
  if (clip) {  // the pieces' lengths come from what the decoder produced
    ClipParams K{};
    K.slot_off = d.ioff;
    K.piece_base = d.pbase;
    K.produced = clip->out_len;
    K.status = clip->status;
    K.bad = clip->bad;
    K.piece_len = d.plen;
    K.n_len = d.nlen;
    K.n_streams = n;
    hipLaunchKernelGGL(checksum_clip_kernel, dim3((n + 3) / 4), dim3(256), 0, st, K);
  }
  const X2n x2n = make_x2n();
  if (np) {
    PieceParams P{};
    P.in = d_in;
    P.piece_off = d.poff;
    P.piece_len = d.plen;
    P.n_pieces = np;
    P.want_crc = kind == FLATE_HIP_CHECKSUM_CRC32;
    P.want_adler = kind == FLATE_HIP_CHECKSUM_ADLER32;
    P.crc = d.crc;
    P.asum = d.asum;
    P.wsum = d.wsum;
    P.x2n = x2n;
    uint32_t blocks = (np + 3) / 4;
    const uint32_t cap = 8u * (uint32_t)ctx_num_cus(c);  // 32 wavefronts per CU
    if (blocks > cap) blocks = cap;
    if (stage >= 0) ctx_stage_begin(c, stage);
    hipLaunchKernelGGL(checksum_piece_kernel, dim3(blocks), dim3(256), 0, st, P);
  } else {
    if (stage >= 0) ctx_stage_begin(c, stage);
  }
  FoldParams F{};
  F.in_off = d.ioff;
  F.piece_base = d.pbase;
  F.piece_len = d.plen;
  F.crc = d.crc;
  F.asum = d.asum;
  F.wsum = d.wsum;
  F.out = d_sums;
  F.n_streams = n;
  F.want_crc = kind == FLATE_HIP_CHECKSUM_CRC32;
  F.max_pieces = 0;
  for (uint32_t i = 0; i < n; ++i) F.max_pieces = pbase[i + 1] - pbase[i] > F.max_pieces ? pbase[i + 1] - pbase[i] : F.max_pieces;
  F.n_len = clip ? d.nlen : nullptr;
  F.x2n = x2n;
  hipLaunchKernelGGL(checksum_fold_kernel, dim3((n + 3) / 4), dim3(256), 0, st, F);
  if (stage >= 0) ctx_stage_end(c, stage);
  if (hipGetLastError() != hipSuccess) return hip_fail("checksum kernels");
  return FLATE_HIP_OK;
  } catch (const std::bad_alloc &) {
    ctx_set_error(c, "out of host memory (checksum piece index)");
    return FLATE_HIP_E_HIP;
  } catch (const std::exception &e) {
    ctx_set_error(c, e.what());
    return FLATE_HIP_E_INTERNAL;
  }
}
}  // namespace

extern "C" int flate_hip_checksum_batch(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n,
                                        uint32_t kind, uint32_t *out, uint32_t flags) {
  if (!c || !in_off || (n && !out) || (kind != FLATE_HIP_CHECKSUM_ADLER32 && kind != FLATE_HIP_CHECKSUM_CRC32))
    return FLATE_HIP_E_INVALID;
  for (uint32_t i = 0; i < n; ++i)
    if (in_off[i + 1] < in_off[i]) return FLATE_HIP_E_INVALID;
  if (n == 0) return FLATE_HIP_OK;
  const uint64_t total = in_off[n];
  if (total && !in) return FLATE_HIP_E_INVALID;
  ctx_set_error(c, "");
  auto hip_fail = [&](const char *what) -> int {
    ctx_set_error(c, std::string(what) + ": " + hipGetErrorString(hipGetLastError()));
    return FLATE_HIP_E_HIP;
  };
  if (hipSetDevice(ctx_device(c)) != hipSuccess) return hip_fail("hipSetDevice");
  hipStream_t st = ctx_stream(c);
  const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
  // the sums, and a staged copy of host input, in slot 1 of the ctx's scratch (slot 0 is checksum_device's)
  const size_t sums_bytes = ((size_t)n * 4 + 4 + 255) & ~(size_t)255;
  void *aux = nullptr;
  int rc = ctx_scratch(c, 1, sums_bytes + (dev ? 0 : total + 16), &aux);
  if (rc != FLATE_HIP_OK) return rc;
  uint32_t *d_sums = (uint32_t *)aux;
  const uint8_t *d_in = dev ? in : (const uint8_t *)aux + sums_bytes;
  if ((rc = ctx_ctl_begin(c, checksum_ctl_up_bytes(in_off, n), (size_t)n * 4 + 512)) != FLATE_HIP_OK) return rc;
  if (!dev && total && hipMemcpyAsync((void *)d_in, in, total, hipMemcpyHostToDevice, st) != hipSuccess)
    return hip_fail("hipMemcpyAsync (checksum input)");
  if ((rc = checksum_device(c, d_in, in_off, n, kind, d_sums, FLATE_HIP_STAGE_CHECKSUM)) != FLATE_HIP_OK) return rc;
  if ((rc = ctx_ctl_down(c, out, d_sums, (size_t)n * 4)) != FLATE_HIP_OK) return rc;
  if (hipStreamSynchronize(st) != hipSuccess) return hip_fail("checksum read-back");
  ctx_ctl_finish(c);
  return ctx_stage_collect(c, FLATE_HIP_STAGE_CHECKSUM);
}
