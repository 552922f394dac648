// zip_kernels.h -- the parameter blocks of zip_kernels.hip (flate_hip_zip_write / _index / _read) and the host entry
// points of the two drivers those calls run through (private).  The format itself is zip_rule.h.
#pragma once

#include <stdint.h>

#include "flate_hip.h"
#include "flate_kernels.h"
#include "zip_units_rule.h"

namespace flate {

// ---- writing: the members placed by a scan, headers and directory behind the pack kernels ----
struct ZipWriteHead {     // the scan's result words
  uint64_t cd_off;        // where the directory starts = the sum of the members
  uint64_t cd_size;
  uint64_t total;         // the archive's bytes
  uint32_t k0, pad;       // the first entry whose header offset >= 0xffffffff (n: none)
};
struct ZipWriteParams {
  const uint64_t *out_len;   // per stream: the raw stream's bytes (huff_code_kernel)
  const uint64_t *in_off;    // n + 1: the entries' input
  const uint64_t *name_off;  // n + 1, DEVICE copy
  const uint8_t *names;      // DEVICE copy
  uint64_t *entry_off;       // n + 1: the local headers, [n] = cd_off
  uint64_t *payload_off;     // n + 1: what the pack kernels read as HuffParams::out_off
  const uint32_t *sums;      // the entries' CRC-32
  uint8_t *out;
  uint64_t out_cap;
  uint32_t n;
  int *status;               // scan_sizes_kernel's status word
  ZipWriteHead *head;
  // entries written in pieces (the option "zip_piece_bytes"; group_scan_kernel has placed them): entry i is the pieces
  // [group_off[i], group_off[i + 1]) of in_off, its raw size the next entry's start minus its own payload start, and
  // out_len is not read.  NULL: every entry is one stream.
  const uint32_t *group_off;
};

// ---- reading: the end record ----
struct ZipEndHead {       // read back as one block
  uint64_t end_p1;        // the highest consistent end record's offset + 1 (atomic max; 0: none)
  uint64_t n, cd_off, cd_size, rec_off;
  int64_t err_off;
  int32_t rc;
  uint32_t zip64;
};

// ---- reading: the directory.  The discovery skeleton (flate_kernels.h) over the directory: the tiles count from
// (cd_off + A) & ~15, the candidates' offsets from cd_off, and bgzf_link_kernel links them as the members of a file of
// cd_size bytes. ----
struct ZipDirHead {       // read back as one block
  uint64_t out_bytes;     // the sum of size over the entries with status 0 (rc == 0 only)
  int64_t err_off;
  uint32_t n_entries;     // well-formed records in front of err_off
  int32_t rc;
};
struct ZipDirParams {
  ChainParams C;          // in / in_len: the archive; n_tiles: over the directory; cand_off: counted from cd_off;
                          // member_off: unused; head: n_cand alone
  uint64_t cd_off, cd_size;
  uint32_t n;             // records the end record promises
  uint32_t ent_cap;       // min(n, cap): entries / C.out_off hold that many (+ 1)
  uint32_t *cand_total;   // cap
  ZipDirHead *head;
  flate_hip_zip_entry *entries;
};

// ---- reading: behind the decoders ----
struct ZipSel {           // one selected entry, built by the host from the index it has read back
  uint64_t src;           // data_off
  uint64_t comp_size, size;
  uint32_t crc;
  int32_t status;         // the index status (or FLATE_HIP_E_TOO_LARGE)
  uint32_t method, pad;
};
struct ZipCopyPiece {     // at most kZipCopyPiece bytes of a stored entry
  uint64_t dst, src;
  uint32_t len, pad;
};
constexpr uint32_t kZipCopyPiece = 65536;
struct ZipReadParams {
  const uint8_t *in;
  uint8_t *out;
  const ZipSel *sel;
  const ZipCopyPiece *pieces;
  uint32_t n_sel, n_pieces;
  uint64_t *out_len;      // per selected entry: the decoders', then the verdict's
  int32_t *status;
  int64_t *err_off;
  uint32_t *bad;          // per selected entry: not to be summed
  const uint32_t *sums;   // the CRC-32 of what was produced
  uint32_t decoded;       // the decoders have run (0: no entry of method 8 was selected)
};

// ---- reading: LONG entries through units (zip_units_kernels.hip; the option "zip_unit_min"; the rule:
// zip_units_rule.h).  The units of all L entries form ONE chain over the HULL's bits: OneParams' raw stream is the hull
// (O.C.in = the archive + the hull's start, one_init_kernel over the hull's length), so every bit and byte offset here
// is counted from the hull's first byte.  The nodes are two lists in one array: A, the n_a FIND candidates of the
// hull, then B, one node per L entry in chain order at bit 8 * L[i].lo.  one_probe_kernel probes every node; the link
// is zip_units_next. ----
struct ZipUnitsHead {      // read back with the OneHead in front of it
  uint32_t n_complete;     // the leading L entries whose units are all good and end with BFINAL
  uint32_t first_unfit;    // the first of them whose units do not sum to the directory's size (0xffffffff: none)
};
struct ZipUnitsParams {
  OneParams O;             // the chain: O.C.cap = n_a + n_b nodes, O.C.member_off = unit_bit
  uint32_t n_a, n_b;
  const ZuEntry *L;        // n_b, chain order
  const ZuRange *R;        // n_b, sorted by file position
  uint32_t *u_start;       // cap + 1, per unit: its L entry + 1 when it starts an entry, else 0
  uint32_t *u_final;       // cap, per unit: it ends with BFINAL
  uint32_t *u_entry;       // cap + 1, per good unit: its L entry
  uint64_t *rel_off;       // cap + 1, per good unit: out_off[k] - out_off[its entry's first unit]
  uint64_t *entry_unit;    // n_b + 1, per L entry the chain reached: its first unit; behind the last: the unit count
  ZipUnitsHead *zh;
};
// The decode: flate_hip_gzfile_read's rounds with every entry's first unit as a SEED.  The round's `count` units
// become n_pieces = count + (entry starts behind the round's first unit) pieces: in front of every such start lies a
// GAP piece of no bits whose slot is the bytes between the two entries' slots in `out`, so that every unit's slot has
// exactly the unit's size and nothing is written between them.  Unit i of the round is piece i + u_entry[u0 + i] -
// u_entry[u0].
struct ZipUnitsDecParams {
  OneDecParams D;          // D.out_off = the chain's out_off; p_out_off / p_dict_* hold 2 * count + 1 pieces
  ZipUnitsParams P;
  uint32_t *seed;          // count
  uint64_t *p_bit_off;     // per piece
  uint64_t *p_bit_end;     // per piece: ~0 = the piece runs to BFINAL
  const int32_t *dp_status;    // per piece: what DECODE reports
  const uint64_t *dp_out_len;
  int32_t *du_status;      // count: the same per unit (zip_units_fold_kernel), for one_check_kernel
  uint64_t *du_out_len;
  // zip_units_verdict_kernel: the served entries L[0, g) into the read's per-slot arrays
  uint32_t g;
  uint64_t *z_out_len;
  int32_t *z_status;
  int64_t *z_err_off;
};

#if defined(__HIPCC__)
__global__ void zip_units_bits_kernel(ZipUnitsParams P);
__global__ void zip_units_link_kernel(ZipUnitsParams P);
__global__ void zip_units_finish_kernel(ZipUnitsParams P);
__global__ void zip_units_entries_kernel(ZipUnitsParams P);
__global__ void zip_units_rel_kernel(ZipUnitsParams P);
__global__ void zip_units_pieces_kernel(ZipUnitsDecParams G);
__global__ void zip_units_fold_kernel(ZipUnitsDecParams G);
__global__ void zip_units_verdict_kernel(ZipUnitsDecParams G);
__global__ void zip_scan_kernel(ZipWriteParams P);
__global__ void zip_write_kernel(ZipWriteParams P);
__global__ void zip_end_find_kernel(const uint8_t *in, uint64_t in_len, ZipEndHead *head);
__global__ void zip_end_read_kernel(const uint8_t *in, uint64_t in_len, ZipEndHead *head);
__global__ void zip_dir_count_kernel(ZipDirParams P);
__global__ void zip_dir_scan_kernel(ZipDirParams P);
__global__ void zip_dir_fill_kernel(ZipDirParams P);
__global__ void zip_entry_kernel(ZipDirParams P);
__global__ void zip_out_scan_kernel(ZipDirParams P);
__global__ void zip_prep_kernel(ZipReadParams P);
__global__ void zip_copy_kernel(ZipReadParams P);
__global__ void zip_verdict_kernel(ZipReadParams P);
#endif

}  // namespace flate

#if defined(__HIPCC__)
namespace flate_host {
// flate_api_deflate.hip: flate_hip_zip_write after its checks (n > 0) -- the encode driver with the ZIP container
int zip_deflate(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n, const uint8_t *names,
                const uint64_t *name_off, uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *entry_off,
                uint32_t flags);
// the same for entries written in pieces ("zip_piece_bytes"): entry i = the pieces [group_off[i], group_off[i + 1]) of
// piece_in_off (zip_pieces_plan, splice_rule.h)
int zip_deflate_pieces(flate_hip_ctx *c, const uint8_t *in, const uint64_t *piece_in_off, uint32_t n_pieces,
                       const uint32_t *group_off, uint32_t n, const uint8_t *names, const uint64_t *name_off, uint8_t *out,
                       uint64_t out_cap, uint64_t *out_len, uint64_t *entry_off, uint32_t flags);
// flate_api_inflate.hip: the batch decoders over raw streams that are not consecutive in DEVICE memory: stream i =
// d_in[in_off[i], in_end[i]) into d_out[out_off[i], out_off[i + 1]).  The results reach the host arrays and stay in the
// ctx's d_out_len / d_istatus / d_ierr.  Returns FLATE_HIP_OK or the first non-zero stream status.
int inflate_ranges_device(flate_hip_ctx *c, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_end, uint32_t n,
                          uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len, int32_t *status, int64_t *err_off);
// flate_api_units.hip: the LONG entries of flate_hip_zip_read through units (the option "zip_unit_min"): the two-list
// discovery (unit_discovery.h, with ZIP's bits, link, finish, entries and rel kernels as its hooks) over the hull
// d_in[hull_lo, hull_hi), the decode rounds into d_out, and the read-back of what they served.  L / R:
// zip_units_form + zip_units_hull (L not empty).  On return *g = the entries L[0, *g) that are decoded and GOOD (the
// caller gives every other one to the batch decoders), G what zip_units_verdict_kernel needs once the caller has set
// g and the three z_ arrays, and *n_units / *n_cand the route report's counts.  Discovery is counted in no profiling
// stage; the rounds' decoder launches in FLATE_HIP_STAGE_INFLATE (of several the last one's time).  Returns what is
// no verdict: FLATE_HIP_OK, FLATE_HIP_E_HIP, _TOO_LARGE, _INTERNAL.
int zip_units_decode(flate_hip_ctx *c, const uint8_t *d_in, uint64_t hull_lo, uint64_t hull_hi,
                     const std::vector<flate::ZuEntry> &L, const std::vector<flate::ZuRange> &R, uint8_t *d_out,
                     uint64_t total, uint32_t *g, flate::ZipUnitsDecParams &G, uint32_t *n_units, uint32_t *n_cand);
}  // namespace flate_host
#endif
