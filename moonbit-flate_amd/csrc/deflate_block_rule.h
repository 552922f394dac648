// deflate_block_rule.h -- where a dynamic-Huffman block of a DEFLATE stream (RFC 1951 3.2.7) can start, at BIT
// granularity, written ONCE: plain C++17 without HIP, compiled into the discovery kernels (one_kernels.hip), into the
// library's host code and into tests/host_model/deflate_block_rule_model.cpp, which compares it with the restatement in
// tests/one_ref.py.
//
// One long stream has no index: its blocks start wherever the previous one ended.  So every bit offset whose next bits
// are a dynamic block header THAT THE DECODER WOULD TAKE is a candidate (flate_hip_inflate_one_index); each candidate is
// decoded without history up to the next dynamic header, linked to the candidate at its end, and the chain from bit 0
// is the serial decode cut at those headers.  The rule must therefore accept EXACTLY what read_tables(typ == 2) of
// inflate_kernels.hip accepts -- a true header that is refused leaves a hole in the chain; a decoy that is accepted only
// costs its probe --: BTYPE = 2 with either BFINAL; HLIT + 257 <= 286; HDIST + 1 <= 30; a code-length code
// HuffmanDecoder::initialize takes (complete, or one code of one bit); every code-length symbol decodable, the repeat
// symbol 16 never first, no repeat beyond HLIT + HDIST + 258 lengths; the literal/length and the distance code each
// taken by initialize (complete, one code of one bit, or EMPTY); every bit inside the raw range.  Nothing else: an
// end-of-block code of length 0 is accepted here as it is there (the block then fails at its first symbol).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define DBLK_HD __host__ __device__ inline
#else
#define DBLK_HD inline
#endif

namespace flate {

// LSB-first bit reader over p[0, ...): the bits [pos, end), counted from p's first bit; no byte that holds none of the
// requested bits is read
struct DblkBits {
  const uint8_t *p;
  uint64_t pos, end;
};
// n = 1 .. 16 bits; false: the range ends first (the decoder's FLATE_HIP_E_UNEXPECTED_EOF)
DBLK_HD bool dblk_get(DblkBits &r, uint32_t n, uint32_t &v) {
  if (r.pos > r.end || r.end - r.pos < n) return false;
  const uint64_t b = r.pos >> 3, last = (r.pos + n - 1) >> 3;
  uint32_t w = r.p[b];
  if (b + 1 <= last) w |= (uint32_t)r.p[b + 1] << 8;
  if (b + 2 <= last) w |= (uint32_t)r.p[b + 2] << 16;
  v = (w >> (r.pos & 7u)) & ((1u << n) - 1u);
  r.pos += n;
  return true;
}

// HuffmanDecoder::initialize's verdict (inflate.mbt:143-161; dec_init of inflate_kernels.hip) on a code with count[l]
// codes of length l = 1 .. 15: the empty code, a complete code, or the one code of one bit
DBLK_HD bool dblk_code_ok(const uint16_t *count) {
  int mn = 0, mx = 0;
  for (int l = 1; l < 16; ++l)
    if (count[l]) {
      if (!mn) mn = l;
      mx = l;
    }
  if (!mx) return true;
  uint32_t code = 0;
  for (int l = mn; l <= mx; ++l) code = (code << 1) + count[l];
  return code == (1u << mx) || (code == 1u && mx == 1);
}

// The cheapest rejection, on the first 13 bits of a header (w: LSB first; BFINAL is either): BTYPE = 2, HLIT <= 29,
// HDIST <= 29.  It refuses about 25 of 32 random offsets before a reader exists.
DBLK_HD bool dblk_quick_ok(uint32_t w) {
  return ((w >> 1) & 3u) == 2u && ((w >> 3) & 31u) <= 29u && ((w >> 8) & 31u) <= 29u;
}

// The first 17 bits at r.pos: BTYPE, HLIT, HDIST, HCLEN.  true: nlit / ndist / nclen are the three counts (257 .. 286,
// 1 .. 30, 4 .. 19) and r stands behind them.
DBLK_HD bool dblk_counts(DblkBits &r, uint32_t &nlit, uint32_t &ndist, uint32_t &nclen) {
  uint32_t h, v;
  if (!dblk_get(r, 3, h) || (h >> 1) != 2u) return false;
  if (!dblk_get(r, 14, v)) return false;
  nlit = (v & 31u) + 257u;
  ndist = ((v >> 5) & 31u) + 1u;
  nclen = ((v >> 10) & 15u) + 4u;
  return dblk_quick_ok(h | (v << 3));
}

// The code-length code behind the counts: its 3-bit lengths in the order of RFC 1951 into cl[19]; true: initialize takes
// it and it is not empty (an empty one decodes no symbol, and there are at least 258 to decode).  At most 57 bits.
DBLK_HD bool dblk_clen_code(DblkBits &r, uint32_t nclen, uint8_t *cl) {
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint16_t count[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 19; ++i) cl[i] = 0;
  for (uint32_t i = 0; i < nclen; ++i) {
    uint32_t v;
    if (!dblk_get(r, 3, v)) return false;
    cl[order[i]] = (uint8_t)v;
    if (v) ++count[v];
  }
  bool any = false;
  for (int l = 1; l < 8; ++l) any = any || count[l] != 0;
  return any && dblk_code_ok(count);
}

// what the discovery pass tests at every bit offset before it looks further: the counts and the code-length code, at
// most 74 bits from `bit` on
DBLK_HD bool dblk_head_ok(const uint8_t *p, uint64_t end_bit, uint64_t bit) {
  DblkBits r{p, bit, end_bit};
  uint32_t nlit, ndist, nclen;
  uint8_t cl[19];
  return dblk_counts(r, nlit, ndist, nclen) && dblk_clen_code(r, nclen, cl);
}

// THE RULE.  raw[0, raw_len): the raw DEFLATE stream; bit: counted from its first byte.  true: read_tables(typ == 2)
// behind read_block_header returns 0 for the block header at `bit`.  No byte at or behind raw + raw_len is read.
DBLK_HD bool deflate_dyn_header_ok(const uint8_t *raw, uint64_t raw_len, uint64_t bit) {
  DblkBits r{raw, bit, 8u * raw_len};
  uint32_t nlit, ndist, nclen;
  uint8_t cl[19];
  if (!dblk_counts(r, nlit, ndist, nclen) || !dblk_clen_code(r, nclen, cl)) return false;
  // the code-length code in canonical form: count per length, the symbols ordered by (length, symbol)
  uint16_t ccount[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint8_t csym[19];
  for (int s = 0; s < 19; ++s) ++ccount[cl[s]];
  ccount[0] = 0;
  {
    uint32_t at[8], a = 0;
    for (int l = 1; l < 8; ++l) at[l] = a, a += ccount[l];
    for (int s = 0; s < 19; ++s)
      if (cl[s]) csym[at[cl[s]]++] = (uint8_t)s;
  }
  uint16_t lit[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  uint16_t dist[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t total = nlit + ndist;
  uint32_t i = 0, prev = 0, kraft_lit = 0, kraft_dist = 0;  // the codes' Kraft sums in units of 2^-15
  while (i < total) {
    // one symbol, bit by bit: a proper prefix of a code word is none, so a range that ends inside one decodes nothing
    uint32_t code = 0, first = 0, index = 0;
    int sym = -1;
    for (int l = 1; l < 8 && sym < 0; ++l) {
      uint32_t b;
      if (!dblk_get(r, 1, b)) return false;
      code |= b;
      const uint32_t cnt = ccount[l];
      if (code - first < cnt) sym = csym[index + (code - first)];
      index += cnt;
      first = (first + cnt) << 1;
      code <<= 1;
    }
    if (sym < 0) return false;  // (the one code of one bit, and the other bit)
    uint32_t rep = 1, len = (uint32_t)sym, extra;
    if (sym == 16) {
      if (i == 0 || !dblk_get(r, 2, extra)) return false;
      rep = 3u + extra, len = prev;
    } else if (sym == 17) {
      if (!dblk_get(r, 3, extra)) return false;
      rep = 3u + extra, len = 0;
    } else if (sym == 18) {
      if (!dblk_get(r, 7, extra)) return false;
      rep = 11u + extra, len = 0;
    }
    if (i + rep > total) return false;
    for (uint32_t k = 0; k < rep; ++k, ++i) {
      if (!len) continue;
      // (an over-subscribed code can never become one that initialize takes: the same verdict as at the end, early --
      // bits that are no header run into this within a few dozen lengths instead of after three hundred)
      uint32_t &kraft = i < nlit ? kraft_lit : kraft_dist;
      kraft += 1u << (15u - len);
      if (kraft > (1u << 15)) return false;
      ++(i < nlit ? lit : dist)[len];
    }
    prev = len;
  }
  return dblk_code_ok(lit) && dblk_code_ok(dist);
}

// THE STORED RULE (option "one_stored_units").  true: read_block_header followed by read_stored_len of
// inflate_kernels.hip take the block header at `bit` as a stored block's -- BTYPE = 0 with either BFINAL; behind the
// header's three bits the reader drops the rest of their byte UNREAD, so the padding bits are not examined here either
// (a rule that asked for zeros would refuse a true header and leave a hole in the chain); the four bytes from
// q = (bit + 3 + 7) / 8 on lie inside the raw range, and LEN (the first two) is the complement of NLEN.  LEN = 0 is a
// header.  Whether the LEN data bytes lie inside the stream is not judged: the probe reports
// FLATE_HIP_E_UNEXPECTED_EOF there, as the serial decoder does.  No byte at or behind raw + raw_len is read.
// A consequence: up to 8 bit offsets in front of ONE aligned LEN / NLEN pair pass -- the bits 5 .. 7 of byte q - 2 and
// 0 .. 4 of byte q - 1, wherever the two bits behind them are 0.  At most one of them is on the path; the others are
// decoys like any other.
DBLK_HD bool deflate_stored_header_ok(const uint8_t *raw, uint64_t raw_len, uint64_t bit) {
  if (bit > ~0ull - 10u) return false;
  const uint64_t b = bit >> 3, q = (bit + 3u + 7u) >> 3;
  if (q > raw_len || raw_len - q < 4u) return false;  // (b < q: the header's bits lie inside as well)
  uint32_t w = raw[b];
  if (b + 1u < q) w |= (uint32_t)raw[b + 1u] << 8;  // (bits 6 and 7 of a byte: BTYPE reaches into the next one)
  if (((w >> ((bit & 7u) + 1u)) & 3u) != 0u) return false;
  const uint32_t len = raw[q] | ((uint32_t)raw[q + 1u] << 8), nlen = raw[q + 2u] | ((uint32_t)raw[q + 3u] << 8);
  return (len ^ nlen) == 0xffffu;
}

// A unit's input spans less than this many bytes (option "one_unit_max" lowers it): the wave decoders count bytes of
// one stream in 32 bits and the lane decoders bits
constexpr uint64_t kOneUnitMax = 1ull << 28;

}  // namespace flate
