// zip_rule.h -- what a ZIP archive is for this library (PKWARE APPNOTE 6.3: local headers, the central directory, the
// end record, their Zip64 forms), written ONCE: plain C++17 without HIP, compiled into the kernels (zip_kernels.hip),
// into the library's host code (flate_api_zip.hip) and into tests/host_model/zip_rule_model.cpp, which compares it with
// tests/zip_ref.py and with Python's zipfile.  The serial functions at the end are the specification of
// flate_hip_zip_write / _index: the kernels must equal them on every input.
//
// WRITING.  version needed / made-by 20 (45 where a Zip64 field is used), flags 0x0800 (names are UTF-8), method 8,
// time 0, date 0x0021, CRC-32 and both sizes in the LOCAL header, no data descriptor, no local extra, no comments, disk
// numbers and attributes 0.  A central record carries the 12-byte Zip64 extra (id 1, size 8, the header offset) exactly
// when its local header offset >= 0xffffffff; offsets are monotone, so these records are a suffix that starts at the
// first such entry k0, and the place of record i is a closed form (zip_central_place).  The Zip64 end record and its
// locator appear exactly when n >= 65535 or the directory's offset or size >= 0xffffffff; the count, size and offset
// fields of the end record then hold all ones.  An entry's sizes never need Zip64: a batch stream is < 2 GiB.
//
// READING.  Absolute offsets, one disk, no prepended data; sizes and the CRC-32 always come from the directory.
#pragma once

#include <stdint.h>

#include "flate_hip.h"

#if defined(__HIPCC__)
#define ZIP_HD __host__ __device__ inline
#else
#define ZIP_HD inline
#endif

namespace flate {

constexpr uint32_t kZipLocalLen = 30;     // + name (+ extra, in archives of others)
constexpr uint32_t kZipCentralLen = 46;   // + name + extra + comment
constexpr uint32_t kZipEndLen = 22;       // + comment
constexpr uint32_t kZip64EndLen = 56;
constexpr uint32_t kZip64LocLen = 20;
constexpr uint32_t kZip64ExtraLen = 12;   // id 1, size 8, the header offset
constexpr uint64_t kZipAll32 = 0xffffffffull;
constexpr uint32_t kZipTailWindow = 65557;  // the end record and the longest comment
constexpr uint16_t kZipFlagsWritten = 0x0800;
constexpr uint16_t kZipFlagsRefused = 0x0061;  // bit 0 encrypted, bit 5 patched data, bit 6 strong encryption

ZIP_HD void zip_put16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8); }
ZIP_HD void zip_put32(uint8_t *p, uint32_t v) { zip_put16(p, v), zip_put16(p + 2, v >> 16); }
ZIP_HD void zip_put64(uint8_t *p, uint64_t v) { zip_put32(p, (uint32_t)v), zip_put32(p + 4, (uint32_t)(v >> 32)); }
ZIP_HD uint32_t zip_get16(const uint8_t *p) { return p[0] | ((uint32_t)p[1] << 8); }
ZIP_HD uint32_t zip_get32(const uint8_t *p) { return zip_get16(p) | (zip_get16(p + 2) << 16); }
ZIP_HD uint64_t zip_get64(const uint8_t *p) { return zip_get32(p) | ((uint64_t)zip_get32(p + 4) << 32); }
ZIP_HD bool zip_sig(const uint8_t *p, uint32_t b2, uint32_t b3) { return p[0] == 0x50 && p[1] == 0x4b && p[2] == b2 && p[3] == b3; }

// ---- writing ----

// The local header of an entry and its name: 30 + name_len bytes at d.
ZIP_HD uint32_t zip_put_local(uint8_t *d, const uint8_t *name, uint32_t name_len, uint32_t crc, uint32_t comp_size, uint32_t size) {
  d[0] = 0x50, d[1] = 0x4b, d[2] = 3, d[3] = 4;
  zip_put16(d + 4, 20), zip_put16(d + 6, kZipFlagsWritten), zip_put16(d + 8, 8);
  zip_put16(d + 10, 0), zip_put16(d + 12, 0x0021);
  zip_put32(d + 14, crc), zip_put32(d + 18, comp_size), zip_put32(d + 22, size);
  zip_put16(d + 26, name_len), zip_put16(d + 28, 0);
  for (uint32_t b = 0; b < name_len; ++b) d[kZipLocalLen + b] = name[b];
  return kZipLocalLen + name_len;
}

ZIP_HD bool zip_central_has_extra(uint64_t header_off) { return header_off >= kZipAll32; }
ZIP_HD uint32_t zip_central_len(uint32_t name_len, uint64_t header_off) {
  return kZipCentralLen + name_len + (zip_central_has_extra(header_off) ? kZip64ExtraLen : 0u);
}
// The central record of an entry: zip_central_len bytes at d.
ZIP_HD uint32_t zip_put_central(uint8_t *d, const uint8_t *name, uint32_t name_len, uint32_t crc, uint32_t comp_size, uint32_t size,
                                uint64_t header_off) {
  const bool z = zip_central_has_extra(header_off);
  const uint32_t ver = z ? 45u : 20u;
  d[0] = 0x50, d[1] = 0x4b, d[2] = 1, d[3] = 2;
  zip_put16(d + 4, ver), zip_put16(d + 6, ver), zip_put16(d + 8, kZipFlagsWritten), zip_put16(d + 10, 8);
  zip_put16(d + 12, 0), zip_put16(d + 14, 0x0021);
  zip_put32(d + 16, crc), zip_put32(d + 20, comp_size), zip_put32(d + 24, size);
  zip_put16(d + 28, name_len), zip_put16(d + 30, z ? kZip64ExtraLen : 0u), zip_put16(d + 32, 0);
  zip_put16(d + 34, 0), zip_put16(d + 36, 0), zip_put32(d + 38, 0);
  zip_put32(d + 42, z ? (uint32_t)kZipAll32 : (uint32_t)header_off);
  for (uint32_t b = 0; b < name_len; ++b) d[kZipCentralLen + b] = name[b];
  if (z) {
    uint8_t *x = d + kZipCentralLen + name_len;
    zip_put16(x, 1), zip_put16(x + 2, 8), zip_put64(x + 4, header_off);
  }
  return zip_central_len(name_len, header_off);
}

// Where record i starts inside the directory, in closed form: names_before = the bytes of the names of the entries in
// front of i; k0 = the first entry whose header offset >= 0xffffffff (n: none).  (i == n: the directory's size.)
ZIP_HD uint64_t zip_central_place(uint64_t i, uint64_t names_before, uint64_t k0) {
  return (uint64_t)kZipCentralLen * i + names_before + (i > k0 ? (uint64_t)kZip64ExtraLen * (i - k0) : 0ull);
}

ZIP_HD bool zip_needs_zip64_end(uint64_t n, uint64_t cd_off, uint64_t cd_size) {
  return n >= 65535u || cd_off >= kZipAll32 || cd_size >= kZipAll32;
}
ZIP_HD uint32_t zip_end_len(uint64_t n, uint64_t cd_off, uint64_t cd_size) {
  return kZipEndLen + (zip_needs_zip64_end(n, cd_off, cd_size) ? kZip64EndLen + kZip64LocLen : 0u);
}
// What follows the directory: [the Zip64 end record, its locator,] the end record; zip_end_len bytes at d, which is
// archive offset cd_off + cd_size.
ZIP_HD uint32_t zip_put_end(uint8_t *d, uint64_t n, uint64_t cd_off, uint64_t cd_size) {
  const bool z = zip_needs_zip64_end(n, cd_off, cd_size);
  if (z) {
    d[0] = 0x50, d[1] = 0x4b, d[2] = 6, d[3] = 6;
    zip_put64(d + 4, kZip64EndLen - 12u), zip_put16(d + 12, 45), zip_put16(d + 14, 45);
    zip_put32(d + 16, 0), zip_put32(d + 20, 0);
    zip_put64(d + 24, n), zip_put64(d + 32, n), zip_put64(d + 40, cd_size), zip_put64(d + 48, cd_off);
    d += kZip64EndLen;
    d[0] = 0x50, d[1] = 0x4b, d[2] = 6, d[3] = 7;
    zip_put32(d + 4, 0), zip_put64(d + 8, cd_off + cd_size), zip_put32(d + 16, 1);
    d += kZip64LocLen;
  }
  d[0] = 0x50, d[1] = 0x4b, d[2] = 5, d[3] = 6;
  zip_put16(d + 4, 0), zip_put16(d + 6, 0);
  zip_put16(d + 8, z ? 0xffffu : (uint32_t)n), zip_put16(d + 10, z ? 0xffffu : (uint32_t)n);
  zip_put32(d + 12, z ? (uint32_t)kZipAll32 : (uint32_t)cd_size), zip_put32(d + 16, z ? (uint32_t)kZipAll32 : (uint32_t)cd_off);
  zip_put16(d + 20, 0);
  return zip_end_len(n, cd_off, cd_size);
}

// ---- reading: the end record ----

struct ZipEnd {
  uint64_t end_off;   // p: where the end record lies
  uint64_t rec_off;   // where the record the values come from lies (the Zip64 end record, or p): the directory ends
                      // at or in front of it
  uint64_t n, cd_off, cd_size;
  uint32_t zip64;
};

// the lowest offset an end record can have
ZIP_HD uint64_t zip_tail_lo(uint64_t in_len) { return in_len > kZipTailWindow ? in_len - kZipTailWindow : 0ull; }

// Is p (<= in_len - 22) the place of a consistent end record?  The archive's end record is the HIGHEST such p in
// [zip_tail_lo(in_len), in_len - 22]; a signature inside the comment or the data that fails the equation is none.
ZIP_HD bool zip_end_candidate(const uint8_t *in, uint64_t in_len, uint64_t p) {
  return zip_sig(in + p, 5, 6) && p + kZipEndLen + zip_get16(in + p + 20) == in_len;
}

// The values of the end record at p (a candidate).  Returns 0 or FLATE_HIP_E_CORRUPT: a refused end record or Zip64
// record or directory range.
ZIP_HD int zip_end_read(const uint8_t *in, uint64_t in_len, uint64_t p, ZipEnd *E) {
  (void)in_len;
  const uint8_t *e = in + p;
  E->end_off = p, E->rec_off = p, E->zip64 = 0;
  uint64_t disk, cd_disk, here;
  if (p >= kZip64LocLen && zip_sig(e - kZip64LocLen, 6, 7)) {
    const uint8_t *l = e - kZip64LocLen;
    const uint64_t r = zip_get64(l + 8);
    if (zip_get32(l + 4) != 0u || zip_get32(l + 16) != 1u) return FLATE_HIP_E_CORRUPT;
    if (p < kZip64LocLen + kZip64EndLen || r > p - (kZip64LocLen + kZip64EndLen) || !zip_sig(in + r, 6, 6)) return FLATE_HIP_E_CORRUPT;
    const uint8_t *z = in + r;
    disk = zip_get32(z + 16), cd_disk = zip_get32(z + 20), here = zip_get64(z + 24);
    E->n = zip_get64(z + 32), E->cd_size = zip_get64(z + 40), E->cd_off = zip_get64(z + 48);
    E->rec_off = r, E->zip64 = 1;
  } else {
    disk = zip_get16(e + 4), cd_disk = zip_get16(e + 6), here = zip_get16(e + 8);
    E->n = zip_get16(e + 10), E->cd_size = zip_get32(e + 12), E->cd_off = zip_get32(e + 16);
  }
  if (disk != 0 || cd_disk != 0 || here != E->n) return FLATE_HIP_E_CORRUPT;
  if (E->cd_off > E->rec_off || E->cd_size > E->rec_off - E->cd_off) return FLATE_HIP_E_CORRUPT;
  return FLATE_HIP_OK;
}

// ---- reading: the central directory ----

struct ZipCentral {
  uint64_t size, comp_size, header_off;
  uint32_t crc, total;  // total: 46 + name + extra + comment
  uint16_t flags, method, name_len;
};

// THE RECORD RULE.  m: the bytes at a directory offset; avail: how many bytes are left up to the directory's end.
// Returns the record's length, or 0: no record can be read here.  A Zip64 extra (the first subfield with id 1 in a
// well-formed run of subfields) supplies, in this order, size, compressed size and header offset, each only if its
// 32-bit field is all ones; a wanted value that is missing makes the record unreadable.  No byte at or behind
// m + avail is read.
ZIP_HD uint32_t zip_central_read(const uint8_t *m, uint64_t avail, ZipCentral *R) {
  if (avail < kZipCentralLen || !zip_sig(m, 1, 2)) return 0;
  const uint32_t nl = zip_get16(m + 28), xl = zip_get16(m + 30), cl = zip_get16(m + 32);
  const uint32_t total = kZipCentralLen + nl + xl + cl;
  if (total > avail) return 0;
  R->flags = (uint16_t)zip_get16(m + 8), R->method = (uint16_t)zip_get16(m + 10);
  R->crc = zip_get32(m + 16);
  R->comp_size = zip_get32(m + 20), R->size = zip_get32(m + 24), R->header_off = zip_get32(m + 42);
  R->name_len = (uint16_t)nl, R->total = total;
  const bool w_size = R->size == kZipAll32, w_comp = R->comp_size == kZipAll32, w_off = R->header_off == kZipAll32;
  if (w_size || w_comp || w_off) {
    const uint8_t *x = m + kZipCentralLen + nl;
    uint32_t q = 0, have = 0;
    const uint8_t *v = nullptr;
    while (q + 4u <= xl) {
      const uint32_t id = zip_get16(x + q), sl = zip_get16(x + q + 2);
      if (q + 4u + sl > xl) break;  // a subfield running past the extra field: nothing behind it is looked at
      if (id == 1u) {
        v = x + q + 4, have = sl;
        break;
      }
      q += 4u + sl;
    }
    uint32_t at = 0;
    if (w_size) {
      if (at + 8u > have) return 0;
      R->size = zip_get64(v + at), at += 8;
    }
    if (w_comp) {
      if (at + 8u > have) return 0;
      R->comp_size = zip_get64(v + at), at += 8;
    }
    if (w_off) {
      if (at + 8u > have) return 0;
      R->header_off = zip_get64(v + at), at += 8;
    }
  }
  return total;
}

// THE ENTRY VERDICT at index time, from the record at directory offset rec_off and the local header it names: the
// whole entry of the index.  Sizes, CRC-32, flags and method are the directory's; data_off uses the LOCAL header's
// name and extra lengths (0 where the local header cannot be used).
ZIP_HD void zip_entry_make(const uint8_t *in, uint64_t cd_off, uint64_t rec_off, const ZipCentral &R, flate_hip_zip_entry *e) {
  e->name_off = rec_off + kZipCentralLen, e->header_off = R.header_off, e->data_off = 0;
  e->comp_size = R.comp_size, e->size = R.size, e->crc32 = R.crc;
  e->name_len = R.name_len, e->method = R.method, e->flags = R.flags, e->reserved = 0, e->reserved2 = 0;
  e->status = FLATE_HIP_OK;
  if ((R.flags & kZipFlagsRefused) || (R.method != 0 && R.method != 8)) {
    e->status = FLATE_HIP_E_UNSUPPORTED;
    return;
  }
  e->status = FLATE_HIP_E_CORRUPT;
  if (R.header_off > cd_off || cd_off - R.header_off < kZipLocalLen || !zip_sig(in + R.header_off, 3, 4)) return;
  const uint8_t *l = in + R.header_off;
  e->data_off = R.header_off + kZipLocalLen + zip_get16(l + 26) + zip_get16(l + 28);
  if (e->data_off > cd_off || R.comp_size > cd_off - e->data_off) return;
  if (R.method == 0 && R.comp_size != R.size) return;
  e->status = FLATE_HIP_OK;
}

// ---- the serial forms: the specification ----

// The end record by the rule: its offset, or -1.
inline int64_t zip_find_end(const uint8_t *in, uint64_t in_len) {
  if (in_len < kZipEndLen) return -1;
  for (uint64_t p = in_len - kZipEndLen + 1; p-- > zip_tail_lo(in_len);)
    if (zip_end_candidate(in, in_len, p)) return (int64_t)p;
  return -1;
}

// flate_hip_zip_index as a serial walk.  Returns 0 or FLATE_HIP_E_CORRUPT with *err_off (else -1); *n = the
// well-formed records in front of it.  entries (may be null): room for E->n of them.
inline int zip_serial_index(const uint8_t *in, uint64_t in_len, ZipEnd *E, flate_hip_zip_entry *entries, uint64_t *n,
                            int64_t *err_off) {
  *n = 0, *err_off = -1;
  *E = ZipEnd{};
  const int64_t p = zip_find_end(in, in_len);
  if (p < 0) {
    *err_off = (int64_t)in_len;
    return FLATE_HIP_E_CORRUPT;
  }
  if (zip_end_read(in, in_len, (uint64_t)p, E)) {
    *err_off = p;
    return FLATE_HIP_E_CORRUPT;
  }
  const uint64_t cd_end = E->cd_off + E->cd_size;
  uint64_t at = E->cd_off;
  for (uint64_t k = 0; k < E->n; ++k) {
    ZipCentral R;
    const uint32_t t = zip_central_read(in + at, cd_end - at, &R);  // (at == cd_end: the directory's end, early)
    if (!t) {
      *err_off = (int64_t)at;
      return FLATE_HIP_E_CORRUPT;
    }
    if (entries) zip_entry_make(in, E->cd_off, at, R, entries + k);
    at += t, *n = k + 1;
  }
  if (at != cd_end) {  // bytes left behind n records
    *err_off = (int64_t)at;
    return FLATE_HIP_E_CORRUPT;
  }
  return FLATE_HIP_OK;
}

// The bytes flate_hip_zip_write produces from the raw streams of a batch (raw[raw_off[i], raw_off[i + 1]), the
// CRC-32s and sizes of what they hold): the archive at out (zip_serial_size bytes); entry_off (may be null): n + 1.
inline uint64_t zip_serial_size(const uint64_t *raw_off, const uint64_t *name_off, uint64_t n) {
  uint64_t at = 0, k0 = n;
  for (uint64_t i = 0; i < n; ++i) {
    if (k0 == n && zip_central_has_extra(at)) k0 = i;
    at += kZipLocalLen + (name_off[i + 1] - name_off[i]) + (raw_off[i + 1] - raw_off[i]);
  }
  const uint64_t cd = zip_central_place(n, name_off[n] - name_off[0], k0);
  return at + cd + zip_end_len(n, at, cd);
}
inline uint64_t zip_serial_write(const uint8_t *raw, const uint64_t *raw_off, const uint32_t *crc, const uint64_t *size,
                                 const uint8_t *names, const uint64_t *name_off, uint64_t n, uint8_t *out, uint64_t *entry_off) {
  uint64_t at = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t nl = (uint32_t)(name_off[i + 1] - name_off[i]);
    const uint64_t cs = raw_off[i + 1] - raw_off[i];
    if (entry_off) entry_off[i] = at;
    at += zip_put_local(out + at, names + name_off[i], nl, crc[i], (uint32_t)cs, (uint32_t)size[i]);
    for (uint64_t b = 0; b < cs; ++b) out[at + b] = raw[raw_off[i] + b];
    at += cs;
  }
  if (entry_off) entry_off[n] = at;
  const uint64_t cd_off = at;
  uint64_t h = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t nl = (uint32_t)(name_off[i + 1] - name_off[i]);
    const uint64_t cs = raw_off[i + 1] - raw_off[i];
    at += zip_put_central(out + at, names + name_off[i], nl, crc[i], (uint32_t)cs, (uint32_t)size[i], h);
    h += kZipLocalLen + nl + cs;
  }
  at += zip_put_end(out + at, n, cd_off, at - cd_off);
  return at;
}

}  // namespace flate
