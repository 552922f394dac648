// checksum_clip_model.cpp -- host model of checksum.hip's clipped pieces and fold (tests/test_checksum_clip.py).
// The index arithmetic and the joining arithmetic are the kernels' own: moonbit-flate_amd/csrc/checksum_clip.h.  What
// is modelled here is only what surrounds them: a piece's sums (checksum_piece_kernel: CRC-32 of the piece, sum of its
// bytes, sum of index * byte) computed the plain way, and checksum_fold_kernel's 64 lanes run one after another.
#include <cstdint>
#include <vector>

#include "checksum_clip.h"

using namespace flate;

namespace {
uint32_t g_table[256];
const uint8_t *g_data = nullptr;
std::vector<uint32_t> g_crc, g_asum;  // of the FULL pieces of g_data
std::vector<uint64_t> g_wsum;

struct Sums {
  uint32_t crc, asum;
  uint64_t wsum;
};
Sums piece_sums(const uint8_t *p, uint32_t len) {
  Sums s{0, 0, 0};
  uint32_t c = 0xffffffffu;
  for (uint32_t i = 0; i < len; ++i) {
    c = g_table[(c ^ p[i]) & 255u] ^ (c >> 8);
    s.asum += p[i];
    s.wsum += (uint64_t)i * p[i];
  }
  s.crc = len ? c ^ 0xffffffffu : 0u;  // (the CRC of no bytes is 0)
  return s;
}
}  // namespace

// data[0, bytes): the bytes every later call sums a prefix of
extern "C" void clip_prepare(const uint8_t *data, uint64_t bytes) {
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? kSumPoly ^ (c >> 1) : c >> 1;
    g_table[i] = c;
  }
  g_data = data;
  const uint64_t full = bytes / kSumPiece;
  g_crc.resize(full), g_asum.resize(full), g_wsum.resize(full);
  for (uint64_t k = 0; k < full; ++k) {
    const Sums s = piece_sums(data + k * kSumPiece, kSumPiece);
    g_crc[k] = s.crc, g_asum[k] = s.asum, g_wsum[k] = s.wsum;
  }
}

// Pieces planned over a slot of `slot` bytes, a stream that produced `produced` (<= slot) of them.  Returns 0, or
// 1: the clipped pieces do not tile [0, produced); 2: a lane's "bytes behind my run" would wrap.
extern "C" int clip_fold(uint64_t slot, uint64_t produced, uint32_t *adler, uint32_t *crc) {
  const uint32_t np = (uint32_t)sum_pieces(slot);
  const uint64_t n = produced;
  std::vector<uint32_t> plen(np), pcrc(np), pasum(np);
  std::vector<uint64_t> pwsum(np);
  uint64_t covered = 0;
  for (uint32_t k = 0; k < np; ++k) {
    const uint32_t len = clip_piece_len(n, k);
    if (len && (uint64_t)k * kSumPiece != covered) return 1;  // a gap or an overlap
    if (len > kSumPiece) return 1;
    covered += len;
    plen[k] = len;
    Sums s;
    if (len == kSumPiece) s = {g_crc[k], g_asum[k], g_wsum[k]};
    else s = piece_sums(g_data + (uint64_t)k * kSumPiece, len);
    pcrc[k] = s.crc, pasum[k] = s.asum, pwsum[k] = s.wsum;
  }
  if (covered != n) return 1;
  const X2n T = make_x2n();
  uint32_t call = 0;
  uint64_t sa_all = 0, sib_all = 0;
  for (uint32_t lane = 0; lane < 64; ++lane) {
    const FoldRun R = fold_run(np, lane, n);
    // CRC-32 (checksum_fold_kernel, want_crc)
    uint32_t c = 0;
    uint64_t end = R.start;
    for (uint32_t k = R.k0; k < R.k1; ++k) {
      c = crc_join(T, c, plen[k], pcrc[k]);
      end += plen[k];
    }
    if (end > n) return 2;
    if (R.k1 > R.k0) c = crc_place(T, c, n - end);
    call ^= c;
    // Adler-32
    uint64_t sa = 0, sib = 0, base = R.start;
    for (uint32_t k = R.k0; k < R.k1; ++k) {
      const uint64_t a = pasum[k];
      sa = (sa + a) % kSumAdlerMod;
      sib = (sib + (base % kSumAdlerMod) * (a % kSumAdlerMod) + pwsum[k] % kSumAdlerMod) % kSumAdlerMod;
      base += plen[k];
    }
    sa_all += sa, sib_all += sib;
  }
  *crc = call;
  *adler = adler_finish(sa_all, sib_all, n);
  return 0;
}
