// one_parts_rule.h -- ONE long stream read in PARTS (flate_hip_one_reader_*), what a call decides, written ONCE: plain
// C++17 without HIP, compiled into the library's host code, into the part kernels (one_parts_kernels.hip) and into
// tests/host_model/one_parts_rule_model.cpp, which compares it with tests/one_parts_ref.py.
//
// A call is flate_hip_inflate_one on the part in[0, in_len) of the stream, started at bit b0 of the part's first raw
// byte.  The discovery over the part yields the COMPLETE units (those that end inside the part, at the next unit's
// header or behind the final block), their sizes, and a verdict: 0 (the chain reaches the final block), or what ended
// it.  This file says what the container's header is on a part that may end inside it, which raw range the part has,
// which units the call delivers, and what the handle remembers for the next call.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define ONE_PARTS_HD __host__ __device__ inline
#else
#define ONE_PARTS_HD inline
#endif

namespace flate {

// the wraps and the status words (FLATE_HIP_WRAP_* / FLATE_HIP_E_*; this header is compiled without flate_hip.h)
constexpr uint32_t kPartsRaw = 0, kPartsZlib = 1, kPartsGzip = 2;
constexpr int kPartsOk = 0, kPartsStreamEnd = 1, kPartsInvalid = -1, kPartsOutTooSmall = -2, kPartsCorrupt = -4,
              kPartsTooLarge = -6, kPartsEof = -7;

ONE_PARTS_HD uint32_t one_parts_trailer_len(uint32_t wrap) { return wrap == kPartsGzip ? 8u : wrap == kPartsZlib ? 4u : 0u; }

// ---- the header: good, bad, or refused only because the part ends here ----
constexpr uint32_t kPartsHdrGood = 0, kPartsHdrBad = 1, kPartsHdrMore = 2;

// m[0, len): the part's bytes.  Good: *hl = the header's length (<= len).  The verdicts are frame_parse_kernel's for a
// member without dictionaries (zlib: CM = 8, CINFO <= 7, FCHECK, FDICT is bad; gzip: gzip_rule.h's header rule), except
// that nothing is asked of the bytes behind the header, and that a header every byte of which passes so far is "more".
// (The gzip walk restates gzip_rule.h's gzip_header_len, which has two answers and asks for the trailer's room; it is not
// shared so that the discovery kernels that compile that function stay what they are.  The stand-alone model program
// holds the two against each other on every header it is given.)
ONE_PARTS_HD uint32_t one_parts_header(uint32_t wrap, const uint8_t *m, uint64_t len, uint64_t *hl) {
  *hl = 0;
  if (wrap == kPartsRaw) return kPartsHdrGood;
  if (wrap == kPartsZlib) {
    if (len >= 1 && ((m[0] & 15u) != 8u || (m[0] >> 4) > 7u)) return kPartsHdrBad;
    if (len < 2) return kPartsHdrMore;
    if ((((uint32_t)m[0] << 8) | m[1]) % 31u != 0u || (m[1] & 0x20u)) return kPartsHdrBad;
    *hl = 2;
    return kPartsHdrGood;
  }
  const uint8_t magic[3] = {0x1f, 0x8b, 8};
  for (uint32_t k = 0; k < 3u && k < len; ++k)
    if (m[k] != magic[k]) return kPartsHdrBad;
  if (len >= 4 && (m[3] & 0xe0u)) return kPartsHdrBad;
  if (len < 10) return kPartsHdrMore;
  const uint32_t flg = m[3];
  uint64_t p = 10;
  if (flg & 4u) {  // FEXTRA
    if (len < p + 2) return kPartsHdrMore;
    p += 2u + (uint64_t)(m[p] | ((uint32_t)m[p + 1] << 8));
  }
  for (uint32_t bit = 8u; bit <= 16u; bit <<= 1) {  // FNAME, FCOMMENT: zero-terminated
    if (!(flg & bit)) continue;
    while (p < len && m[p]) ++p;
    if (p >= len) return kPartsHdrMore;
    ++p;
  }
  if (flg & 2u) p += 2;  // FHCRC
  if (p > len) return kPartsHdrMore;
  *hl = p;
  return kPartsHdrGood;
}

// The raw range of a part.  first: the part starts the stream (its header is here); final_in: no bytes follow, so the
// trailer is the part's last bytes and the raw stream ends in front of them -- a decoder that needs more has met the
// stream's end, as in the whole call -- and a header that is refused for want of bytes, or that leaves no room for
// the trailer, is bad.  On a part that is not final the raw range runs to the part's end: where the trailer starts is
// known only once the final block has been decoded.
struct OnePartFrame {
  uint32_t hdr;               // kPartsHdr*
  uint64_t raw_off, raw_end;  // the raw range [raw_off, raw_end) of the part (empty unless hdr is good)
};
ONE_PARTS_HD OnePartFrame one_parts_frame(uint32_t wrap, bool first, bool final_in, const uint8_t *m, uint64_t len) {
  OnePartFrame f{kPartsHdrGood, 0, 0};
  const uint64_t tl = one_parts_trailer_len(wrap);
  if (first) {
    uint64_t hl = 0;
    f.hdr = one_parts_header(wrap, m, len, &hl);
    if (final_in && (f.hdr == kPartsHdrMore || (f.hdr == kPartsHdrGood && len < hl + tl))) f.hdr = kPartsHdrBad;
    if (f.hdr != kPartsHdrGood) return f;
    f.raw_off = hl;
  }
  f.raw_end = final_in ? (len >= f.raw_off + tl ? len - tl : f.raw_off) : len;
  return f;
}

// ---- which units a call delivers ----
constexpr uint32_t kPartsDecode = 0;   // decode n_del units (and, with_fail, the failing one) into out[0, total)
constexpr uint32_t kPartsNothing = 1;  // FLATE_HIP_OK with nothing used: the caller appends more
constexpr uint32_t kPartsReturn = 2;   // `status` without a decode (need: *out_len of FLATE_HIP_E_OUT_TOO_SMALL)

struct OnePartsPlan {
  uint32_t action;
  int32_t status;
  uint64_t need;
  uint32_t n_del;      // complete units delivered: the longest prefix that fits
  uint32_t with_fail;  // ... and the unit the stream fails in, as far as it came
  uint32_t terminal;   // everything up to the discovery's verdict is delivered, and that verdict is the stream's: 0 =
                       // the final block, else its error (rc at err_off)
  uint64_t total;      // bytes delivered if every unit decodes as discovered
};

// n_units complete units with the sizes out_off[k + 1] - out_off[k]; rc: the discovery's verdict over the part;
// fail_unit / fail_out: the unit behind them fails behind its header, after fail_out bytes.  The verdict is the STREAM's
// when it does not come from the part's end: 0 and FLATE_HIP_E_CORRUPT always (the bits read are true stream bits), the
// end of input on a final part.  On a part that is not final the end of input only says that the unit is cut, and a
// unit beyond unit_max stays in front of the next call, which has no complete unit then and returns that status.
ONE_PARTS_HD OnePartsPlan one_parts_plan(uint32_t n_units, const uint64_t *out_off, int rc, uint32_t fail_unit,
                                         uint64_t fail_out, bool final_in, uint64_t out_cap, uint64_t in_len,
                                         uint64_t unit_max) {
  OnePartsPlan p{kPartsDecode, 0, 0, 0, 0, 0, 0};
  if (rc != 0 && rc != kPartsCorrupt && rc != kPartsEof && rc != kPartsTooLarge) {  // (FLATE_HIP_E_INTERNAL)
    p.action = kPartsReturn, p.status = rc;
    return p;
  }
  const bool verdict = rc == 0 || rc == kPartsCorrupt || (rc == kPartsEof && final_in);
  const uint64_t prefix = out_off[n_units];
  const uint64_t all = prefix + (verdict && fail_unit ? fail_out : 0ull);
  if (verdict && all <= out_cap) {
    p.n_del = n_units, p.with_fail = fail_unit ? 1u : 0u, p.terminal = 1u, p.total = all;
    return p;
  }
  uint32_t k = 0;
  while (k < n_units && out_off[k + 1] <= out_cap) ++k;
  if (k) {
    p.n_del = k, p.total = out_off[k];
    return p;
  }
  if (n_units || verdict) {  // a first unit, or what the failing one produced, that does not fit
    p.action = kPartsReturn, p.status = kPartsOutTooSmall, p.need = n_units ? out_off[1] : all;
    return p;
  }
  if (rc == kPartsTooLarge || in_len >= unit_max) p.action = kPartsReturn, p.status = kPartsTooLarge;
  else p.action = kPartsNothing;
  return p;
}

// ---- what the handle remembers ----
struct OnePartsState {
  uint64_t produced;         // bytes delivered so far
  uint64_t raw_base;         // bytes of the RAW stream in front of the next part's first byte (err_off counts from there)
  uint64_t consumed;         // bytes of the member used so far: the sum of *in_used
  uint32_t b0;               // the next unit starts at this bit of the next part's first byte
  uint32_t header_done;      // the container's header lies behind
  uint32_t trailer_pending;  // the final block is delivered, the trailer is not judged yet
  int32_t status;            // sticky: 0, FLATE_HIP_STREAM_END or the stream's error
  int64_t err_off;           // ... and its offset
};
ONE_PARTS_HD OnePartsState one_parts_fresh() { return OnePartsState{0, 0, 0, 0, 0, 0, 0, -1}; }

// Behind a call that delivered `delivered` bytes up to bit next_bit (counted from the part's first raw byte, raw_off):
// *in_used = the byte that holds the first undelivered bit, whose place in that byte becomes b0.  ended: the final block
// was delivered -- the rest of its last byte is used too, and the trailer behind it if the part holds it whole
// (*trailer_now: it is judged in this call); else it stays for the next call.
ONE_PARTS_HD void one_parts_advance(OnePartsState &s, uint32_t wrap, uint64_t raw_off, uint64_t next_bit,
                                    uint64_t delivered, bool ended, uint64_t in_len, uint64_t *in_used,
                                    bool *trailer_now) {
  const uint64_t tl = one_parts_trailer_len(wrap);
  uint64_t used = raw_off + (ended ? (next_bit + 7u) / 8u : next_bit / 8u);
  s.raw_base += used - raw_off;
  s.b0 = ended ? 0u : (uint32_t)(next_bit & 7u);
  s.produced += delivered;
  s.header_done = 1u;
  *trailer_now = false;
  if (ended) {
    if (in_len - used >= tl) used += tl, *trailer_now = true;
    else s.trailer_pending = 1u;
  }
  s.consumed += used;
  *in_used = used;
}

// ---- the arguments (api_checks.h hands them on) ----
ONE_PARTS_HD int one_parts_open_args(const void *ctx, uint32_t wrap, uint32_t flags, uint32_t device_ptrs, const void *r) {
  if (!ctx || !r || wrap > kPartsGzip || (flags & ~device_ptrs)) return kPartsInvalid;
  return kPartsOk;
}
ONE_PARTS_HD int one_parts_read_args(const void *r, const uint8_t *in, uint64_t in_len, const uint8_t *out, uint64_t out_cap,
                                     const uint64_t *in_used, const uint64_t *out_len) {
  if (!r || !in_used || !out_len || (in_len && !in) || (out_cap && !out)) return kPartsInvalid;
  return kPartsOk;
}

}  // namespace flate
