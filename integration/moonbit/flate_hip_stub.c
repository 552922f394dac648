/*
 * flate_hip_stub.c -- the few lines of C the MoonBit native backend needs next to
 * libflate_hip.so.  MoonBit's `extern "C"` cannot take
 * a pointer-to-pointer and has no null test for an #external type, so the four constructors
 * (ctx, comm, stream, inflate stream) and their null tests are wrapped, the size-only inflate pass fixes its
 * NULL arguments and the piecewise read packs its three results into one array; everything else binds
 * include/flate_hip.h directly.  UNVERIFIED with moon (not available in the build image); this file
 * itself is compiled by tests/test_library_abi.py to keep it in step with the header.
 */
#include "flate_hip.h"

/* -> flate_hip_ctx* or NULL; *rc_out (optional) receives the error code */
flate_hip_ctx *flate_hip_mbt_ctx_new(int device) {
  flate_hip_ctx *c = 0;
  if (flate_hip_init(device, &c) != FLATE_HIP_OK) return 0;
  return c;
}

/* MoonBit has no null test for an #external type */
int flate_hip_mbt_ctx_is_null(const flate_hip_ctx *c) { return c == 0; }

/* (FixedArray[Byte] / FixedArray[UInt64] / FixedArray[Int] arrive as plain pointers, so
 * flate_hip_deflate_fast_batch, flate_hip_inflate_batch, flate_hip_deflate_fast_spliced,
 * flate_hip_stream_write and the gather calls are bound by the .mbt file directly: no wrapper.) */

/* -- exchange step (multi-GPU): the communicator constructor returns its pointer instead of
 * writing it through a pointer-to-pointer; the gather calls bind include/flate_hip.h directly. -- */
flate_hip_comm *flate_hip_mbt_comm_new(flate_hip_ctx *c, const uint8_t *unique_id, int rank, int world) {
  flate_hip_comm *cm = 0;
  if (flate_hip_comm_init(c, unique_id, rank, world, &cm) != FLATE_HIP_OK) return 0;
  return cm;
}

int flate_hip_mbt_comm_is_null(const flate_hip_comm *cm) { return cm == 0; }

/* -- one long stream written in pieces; the size-only inflate pass -- */
flate_hip_stream *flate_hip_mbt_stream_new(flate_hip_ctx *c, uint32_t flags) {
  flate_hip_stream *st = 0;
  if (flate_hip_stream_open(c, flags, &st) != FLATE_HIP_OK) return 0;
  return st;
}

int flate_hip_mbt_stream_is_null(const flate_hip_stream *st) { return st == 0; }

int flate_hip_mbt_inflate_sizes(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n,
                                uint64_t *out_len, int32_t *status, int64_t *err_off) {
  return flate_hip_inflate_batch(c, in, in_off, n, 0, 0, out_len, status, err_off, FLATE_HIP_SIZE_ONLY);
}

/* -- one long stream decoded in pieces: constructor + null test, and the three results of a read
 * packed into one array (MoonBit passes no pointers to scalars) -- */
flate_hip_inflate_stream *flate_hip_mbt_inflate_stream_new(flate_hip_ctx *c) {
  flate_hip_inflate_stream *st = 0;
  if (flate_hip_inflate_stream_open(c, &st) != FLATE_HIP_OK) return 0;
  return st;
}

int flate_hip_mbt_inflate_stream_is_null(const flate_hip_inflate_stream *st) { return st == 0; }

/* res[0] = bytes of `in` used, res[1] = bytes written to out, res[2] = err_off (int64 bits) */
int flate_hip_mbt_inflate_stream_read(flate_hip_inflate_stream *st, const uint8_t *in, uint64_t in_len, int final_in,
                                      uint8_t *out, uint64_t out_cap, uint64_t *res) {
  int64_t eoff = -1;
  const int rc = flate_hip_inflate_stream_read(st, in, in_len, final_in, out, out_cap, &res[0], &res[1], &eoff);
  res[2] = (uint64_t)eoff;
  return rc;
}

/* -- zlib / gzip members framed on the device: MoonBit has no null FixedArray, so the batch call without
 * preset dictionaries gets an entry of its own (flate_hip_deflate_fast_spliced_framed takes no optional
 * arrays and is bound by the .mbt file directly) -- */
int flate_hip_mbt_deflate_batch_framed(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n,
                                       uint32_t wrap, uint8_t *out, uint64_t out_cap, uint64_t *out_off,
                                       uint32_t flags) {
  return flate_hip_deflate_fast_batch_framed(c, in, in_off, n, wrap, 0, 0, 0, 0, out, out_cap, out_off, flags);
}

/* ... and so does the read side without preset dictionaries and without the per-member dictionary report (with
 * dictionaries every array exists, and the .mbt file binds flate_hip_inflate_batch_framed directly) */
int flate_hip_mbt_inflate_batch_framed(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n,
                                       uint32_t wrap, uint8_t *out, const uint64_t *out_off, uint64_t *out_len,
                                       int32_t *status, int64_t *err_off, uint32_t flags) {
  return flate_hip_inflate_batch_framed(c, in, in_off, n, wrap, 0, 0, 0, out, out_off, out_len, status, err_off, 0,
                                        flags);
}

/* -- ONE member around a spliced stream, read in one call: the member's two words packed into one array (MoonBit
 * passes no pointers to scalars): res[0] = member status, res[1] = member_err_off -- */
int flate_hip_mbt_inflate_spliced_framed(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t wrap,
                                         const uint64_t *bit_off, uint32_t n, uint8_t *out, const uint64_t *out_off,
                                         uint64_t *out_len, int32_t *status, int64_t *err_off, int64_t *res,
                                         uint32_t flags) {
  int32_t ms = 0;
  int64_t me = -1;
  const int rc = flate_hip_inflate_spliced_framed(c, in, in_len, wrap, bit_off, n, out, out_off, out_len, status,
                                                  err_off, &ms, &me, flags);
  res[0] = ms;
  res[1] = me;
  return rc;
}

/* -- BGZF files (flate_hip_bgzf_write / _read): the scalar results packed into one array (MoonBit passes no pointers
 * to scalars).  write: res[0] = the file's size.  read: res[0] = out_len, res[1] = n_members, res[2] = bad_member
 * (-1: none), res[3] = err_off, res[4] = eof_marker.  query: res[0] = out_bytes, res[1] = n_members, res[2] =
 * eof_marker, res[3] = err_off -- the size a caller needs before it can make room for flate_hip_mbt_bgzf_read -- */
uint64_t flate_hip_mbt_bgzf_bound(uint64_t in_len, uint32_t block_bytes) {
  return (uint64_t)flate_hip_bgzf_bound(in_len, block_bytes);
}
int flate_hip_mbt_bgzf_write(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t block_bytes, uint8_t *out,
                             uint64_t out_cap, int64_t *res, uint32_t flags) {
  uint64_t len = 0;
  const int rc = flate_hip_bgzf_write(c, in, in_len, block_bytes, out, out_cap, &len, 0, flags);
  res[0] = (int64_t)len;
  return rc;
}
int flate_hip_mbt_bgzf_query(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, int64_t *res) {
  uint32_t n = 0;
  uint64_t bytes = 0;
  int eof = 0;
  int64_t err = -1;
  const int rc = flate_hip_bgzf_index(c, in, in_len, 0, 0, 0, &n, &bytes, &eof, &err, 0);
  res[0] = (int64_t)bytes;
  res[1] = n;
  res[2] = eof;
  res[3] = err;
  return rc;
}
int flate_hip_mbt_bgzf_read(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap,
                            int64_t *res) {
  uint64_t len = 0;
  uint32_t n = 0, bad = 0xffffffffu;
  int64_t err = -1;
  int eof = 0;
  const int rc = flate_hip_bgzf_read(c, in, in_len, out, out_cap, &len, &n, &bad, &err, &eof, 0);
  res[0] = (int64_t)len;
  res[1] = n;
  res[2] = bad == 0xffffffffu ? -1 : (int64_t)bad;
  res[3] = err;
  res[4] = eof;
  return rc;
}

/* -- ZIP reads (flate_hip_zip_read with the option "zip_unit_min"): which path the last read on this ctx took, the
 * four counts of flate_hip_zip_last_route packed into one array: res[0] = unit_entries, res[1] = fallback_entries,
 * res[2] = n_units, res[3] = n_candidates -- */
int flate_hip_mbt_zip_last_route(const flate_hip_ctx *c, int64_t *res) {
  uint32_t w[4] = {0, 0, 0, 0};
  const int rc = flate_hip_zip_last_route(c, &w[0], &w[1], &w[2], &w[3]);
  for (int k = 0; k < 4; ++k) res[k] = w[k];
  return rc;
}

/* -- the write side's route query (the option "zip_piece_bytes"): res[0] = long_entries, res[1] = n_pieces.
 * (flate_hip_deflate_fast_grouped_framed takes its optional index as an array and is bound by the .mbt file directly.) -- */
int flate_hip_mbt_zip_write_last_route(const flate_hip_ctx *c, int64_t *res) {
  uint32_t w[2] = {0, 0};
  const int rc = flate_hip_zip_write_last_route(c, &w[0], &w[1]);
  res[0] = w[0], res[1] = w[1];
  return rc;
}
