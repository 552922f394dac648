// checksum_clip.h -- the index arithmetic of checksum.hip's pieces and folds, shared by the kernels and by a CPU
// test (tests/test_checksum_clip.py compiles this header with g++): which bytes a piece holds when a stream's pieces
// were planned over its output SLOT and the stream then produced fewer bytes (flate_hip_inflate_batch_framed), where a
// lane's run of pieces starts, and the arithmetic that joins per-piece sums.  No HIP type, no device builtin.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FLATE_CLIP_HD __host__ __device__
#else
#define FLATE_CLIP_HD
#endif

namespace flate {

constexpr uint32_t kSumPiece = 65536;  // bytes per piece
constexpr uint32_t kSumPoly = 0xedb88320u;
constexpr uint32_t kSumAdlerMod = 65521u;

// pieces planned for `bytes` bytes (a stream, or the slot of one)
FLATE_CLIP_HD inline uint64_t sum_pieces(uint64_t bytes) { return (bytes + kSumPiece - 1) / kSumPiece; }

// Piece k of a stream (counted from the stream's first piece) covers [k * 64 KiB, (k + 1) * 64 KiB); of a stream of
// n bytes it holds the part below n: 64 KiB, the stream's last bytes, or nothing (a piece planned over a slot that
// the stream did not fill).
FLATE_CLIP_HD inline uint32_t clip_piece_len(uint64_t n, uint64_t k) {
  const uint64_t at = k * kSumPiece;
  if (at >= n) return 0u;
  return n - at < kSumPiece ? (uint32_t)(n - at) : kSumPiece;
}

// The fold gives lane L the run of pieces [L r, (L + 1) r) of a stream's np pieces, r = ceil(np / 64).  k0, k1: the
// run, counted from the stream's first piece (k0 == k1: none).  start: the bytes of the stream in front of the run.
// Every piece in front of a run is full or lies beyond the data, so that is k0 * 64 KiB, but never more than n:
// what follows (n - start - the run's bytes = the bytes behind the run) cannot wrap.
struct FoldRun {
  uint32_t k0, k1;
  uint64_t start;
};
FLATE_CLIP_HD inline FoldRun fold_run(uint32_t np, uint32_t lane, uint64_t n) {
  const uint32_t run = (np + 63u) / 64u;
  FoldRun r;
  r.k0 = (uint64_t)run * lane < np ? run * lane : np;
  r.k1 = np - r.k0 > run ? r.k0 + run : np;
  const uint64_t at = (uint64_t)r.k0 * kSumPiece;
  r.start = at < n ? at : n;
  return r;
}

// a(x) * b(x) mod P in the reflected representation (bit 31 = x^0); zlib's multmodp
FLATE_CLIP_HD inline uint32_t multmodp(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) {
      p ^= b;
      if ((a & (m - 1u)) == 0) break;
    }
    m >>= 1;
    b = (b & 1u) ? (b >> 1) ^ kSumPoly : b >> 1;
  }
  return p;
}

struct X2n {
  uint32_t t[32];  // x^(2^n) mod P
};
inline X2n make_x2n() {
  X2n r;
  uint32_t p = 1u << 30;  // x^1
  r.t[0] = p;
  for (int n = 1; n < 32; ++n) r.t[n] = p = multmodp(p, p);
  return r;
}

// x^(n * 2^k) mod P
FLATE_CLIP_HD inline uint32_t x2nmodp(const X2n &T, uint64_t n, unsigned k) {
  uint32_t p = 1u << 31;  // x^0
  while (n) {
    if (n & 1u) p = multmodp(T.t[k & 31u], p);
    n >>= 1;
    ++k;
  }
  return p;
}

// CRC-32: a run's value so far, joined with its next piece (len bytes, CRC crc; an empty piece: len = 0, crc = 0
// changes nothing) -- crc(A || B) = crc(A) * x^(8 |B|) + crc(B)
FLATE_CLIP_HD inline uint32_t crc_join(const X2n &T, uint32_t c, uint32_t len, uint32_t crc) {
  return multmodp(x2nmodp(T, len, 3), c) ^ crc;
}
// ... and a finished run moved to its place: `behind` bytes of the stream follow it
FLATE_CLIP_HD inline uint32_t crc_place(const X2n &T, uint32_t c, uint64_t behind) {
  return multmodp(x2nmodp(T, behind, 3), c);
}

// Adler-32 from sa = sum of the bytes and sib = sum of (index * byte), both mod 65521, of a stream of n bytes:
// s1 = 1 + sum b;  s2 = n + sum (n - i) b_i = n + n * sum b - sum i b_i   (RFC 1950 8.2).  n = 0: 1.
FLATE_CLIP_HD inline uint32_t adler_finish(uint64_t sa, uint64_t sib, uint64_t n) {
  sa %= kSumAdlerMod;
  sib %= kSumAdlerMod;
  const uint64_t nm = n % kSumAdlerMod;
  const uint32_t s1 = (uint32_t)((1u + sa) % kSumAdlerMod);
  const uint32_t s2 = (uint32_t)((nm + nm * sa + (uint64_t)kSumAdlerMod * kSumAdlerMod - sib) % kSumAdlerMod);
  return (s2 << 16) | s1;
}

// ---- the sums of a CONCATENATION from the finished sums of its pieces (flate_hip_inflate_spliced_framed: the
// member's checksum is that of what the pieces of the spliced stream produced, one after another; checksum_join_kernel
// and tests/test_checksum_join.py).  Piece i has `len` bytes and `behind` bytes of the whole follow it.

// CRC-32: crc(whole) = XOR over the pieces of crc_i * x^(8 behind_i); an empty piece (crc 0) adds nothing, and the
// CRC of no piece at all is 0
FLATE_CLIP_HD inline uint32_t crc_concat_term(const X2n &T, uint32_t crc, uint64_t len, uint64_t behind) {
  return len ? crc_place(T, crc, behind) : 0u;
}

// Adler-32: with (a1, a2) the halves of piece i's sum, a1 - 1 = sum of its bytes and a2 - len = sum of
// (len - k) * byte k.  In the whole, byte k of piece i weighs (behind + len - k), hence
//   s1 = 1 + sum of d1,  d1 = a1 - 1;      s2 = n + sum of d2,  d2 = (a2 - len) + behind * d1      (mod 65521).
// An empty piece (sum 1) gives d1 = d2 = 0; no piece at all: 1.
struct AdlerTerm {
  uint32_t d1, d2;  // both below 65521
};
FLATE_CLIP_HD inline AdlerTerm adler_concat_term(uint32_t adler, uint64_t len, uint64_t behind) {
  const uint64_t M = kSumAdlerMod;
  const uint64_t a1 = (adler & 0xffffu) % M, a2 = (adler >> 16) % M;
  AdlerTerm t;
  t.d1 = (uint32_t)((a1 + M - 1u) % M);
  t.d2 = (uint32_t)((a2 + M - len % M + (behind % M) * t.d1) % M);
  return t;
}
// d1, d2: the terms' sums (any multiple of 65521 may have been taken out on the way); n: bytes of the whole
FLATE_CLIP_HD inline uint32_t adler_concat_finish(uint64_t d1, uint64_t d2, uint64_t n) {
  const uint32_t s1 = (uint32_t)((1u + d1 % kSumAdlerMod) % kSumAdlerMod);
  const uint32_t s2 = (uint32_t)((n % kSumAdlerMod + d2 % kSumAdlerMod) % kSumAdlerMod);
  return (s2 << 16) | s1;
}

// what piece i counts: what its decoder produced, never more than its slot holds (checksum_clip_kernel's rule)
FLATE_CLIP_HD inline uint64_t clip_to_slot(uint64_t produced, uint64_t slot) { return produced < slot ? produced : slot; }

}  // namespace flate
