// flate_api_zip.hip -- ZIP archives in the C ABI (see include/flate_hip.h): flate_hip_zip_bound, _zip_write, _zip_index,
// _zip_read.  The format is zip_rule.h, the kernels zip_kernels.hip, the argument checks api_checks.h.  Writing runs
// through the encode driver (flate_api_deflate.hip: zip_deflate), reading through the decode driver
// (flate_api_inflate.hip: inflate_ranges_device) between the discovery in front of it and the verdict behind it.
#include "flate_ctx.h"

#include <cstring>
#include <exception>
#include <stdexcept>

#include "api_checks.h"
#include "zip_rule.h"
#include "zip_units_rule.h"

using namespace flate;
using namespace flate_host;

static_assert(sizeof(flate_hip_zip_entry) == 64, "flate_hip_zip_entry is part of the ABI: 64 bytes of plain integers");
static_assert(sizeof(ZipSel) == 40 && sizeof(ZipCopyPiece) == 24, "device records");

namespace {

// What discovery leaves: the archive's verdict and, when it is FLATE_HIP_OK, the index in device memory.
struct ZipFound {
  int rc = FLATE_HIP_OK;
  int64_t err_off = -1;
  uint32_t n = 0;            // rc == 0: the entries; else the well-formed records in front of err_off
  uint64_t out_bytes = 0;
  const flate_hip_zip_entry *d_entries = nullptr;  // n
  const uint64_t *d_out_off = nullptr;              // n + 1
};

// The discovery kernels over d_in[0, in_len) (DEVICE memory), queued on the ctx's stream, with two read-backs of a few
// words: the end record's values (the directory's range sizes everything behind it), then the verdict.  The arrays are
// sized for zip_first_cap candidates; a directory with more decoys takes a second attempt sized from the count.
// Returns what is no verdict (FLATE_HIP_E_HIP, _TOO_LARGE, _INTERNAL); counted in no profiling stage.
int zip_discover(flate_hip_ctx *c, const uint8_t *d_in, uint64_t in_len, ZipFound &F) {
  int rc;
  F = ZipFound{};
  if (in_len < kZipEndLen) {
    F.rc = FLATE_HIP_E_CORRUPT, F.err_off = (int64_t)in_len;
    return FLATE_HIP_OK;
  }
  if ((rc = ensure(c, c->d_zip_end, sizeof(ZipEndHead)))) return rc;
  ZipEndHead *d_end = (ZipEndHead *)c->d_zip_end.p;
  ZipEndHead EH{};
  const uint64_t window = in_len - kZipEndLen + 1u - zip_tail_lo(in_len);
  HIP_TRY(c, hipMemsetAsync(d_end, 0, sizeof(ZipEndHead), c->stream));
  hipLaunchKernelGGL(zip_end_find_kernel, dim3((uint32_t)((window + 255u) / 256u)), dim3(256), 0, c->stream, d_in, in_len, d_end);
  hipLaunchKernelGGL(zip_end_read_kernel, dim3(1), dim3(64), 0, c->stream, d_in, in_len, d_end);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&EH, d_end, sizeof EH, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (EH.rc) {
    F.rc = EH.rc, F.err_off = EH.err_off;
    return FLATE_HIP_OK;
  }
  if (EH.n > 0xfffffffeull) return FLATE_HIP_E_TOO_LARGE;
  if (EH.n == 0 || EH.cd_size == 0) {  // no record to look for: the serial walk's first step decides
    if (EH.n != 0 || EH.cd_size != 0) F.rc = FLATE_HIP_E_CORRUPT, F.err_off = (int64_t)EH.cd_off;
    return FLATE_HIP_OK;
  }
  ZipDirParams P{};
  ChainParams &C = P.C;
  C.in = d_in;
  C.in_len = in_len;
  P.cd_off = EH.cd_off;
  P.cd_size = EH.cd_size;
  P.n = (uint32_t)EH.n;
  if ((rc = tiles_for(d_in, EH.cd_off, EH.cd_size, &C.n_tiles))) return rc;
  uint32_t cap = zip_first_cap(EH.n, EH.cd_size);
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = chain_size(C, cap))) return rc;
    P.ent_cap = P.n < cap ? P.n : cap;
    rc = carve(c, c->d_zip_dir, [&](Carve &k) {
      k.take(P.head, 1);
      k.take(C.head, 1);
      k.take(C.tile_cnt, (size_t)C.n_tiles + 1);
      k.take(C.cand_off, cap);
      k.take(P.cand_total, cap);
      k.take(C.jump[0], (size_t)cap + 2);
      k.take(C.jump[1], (size_t)cap + 2);
      k.take(C.path, C.path_len);
      k.take(P.entries, (size_t)P.ent_cap + 1);
      k.take(C.out_off, (size_t)P.ent_cap + 1);
    });
    if (rc) return rc;
    BgzfParams L{C, P.cand_total, nullptr};  // bgzf_link_kernel: the directory as a file of cd_size bytes that starts at 0
    L.C.in_len = EH.cd_size;
    hipLaunchKernelGGL(zip_dir_count_kernel, dim3(C.n_tiles), dim3(256), 0, c->stream, P);
    hipLaunchKernelGGL(zip_dir_scan_kernel, dim3(1), dim3(1024), 0, c->stream, P);
    hipLaunchKernelGGL(zip_dir_fill_kernel, dim3(C.n_tiles), dim3(256), 0, c->stream, P);
    if ((rc = chain_tail(c, C, bgzf_link_kernel, L, zip_entry_kernel, zip_out_scan_kernel, P))) return rc;
    ZipDirHead H{};
    BgzfHead BH{};
    HIP_TRY(c, hipMemcpyAsync(&H, P.head, sizeof H, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&BH, C.head, sizeof BH, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (BH.n_cand <= cap) {
      F.rc = H.rc, F.err_off = H.err_off, F.n = H.n_entries, F.out_bytes = H.out_bytes;
      F.d_entries = P.entries, F.d_out_off = C.out_off;
      return FLATE_HIP_OK;
    }
    // more candidates than the arrays hold: nothing behind the scan has run; once more, sized from the count
    cap = BH.n_cand;
  }
  c->hip_err = "ZIP discovery: the candidate count changed between two passes";
  return FLATE_HIP_E_INTERNAL;
}

}  // namespace

extern "C" {

size_t flate_hip_zip_bound(const uint64_t *in_off, uint32_t n, const uint64_t *name_off) {
  return (size_t)zip_archive_bound(in_off, n, name_off, flate_hip_deflate_bound);
}

int flate_hip_zip_write(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n, const uint8_t *names,
                        const uint64_t *name_off, uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *entry_off,
                        uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  const int rc = zip_write_args(in, in_off, n, names, name_off, out, out_len, flags);
  if (rc) return rc;
  c->hip_err.clear();
  *out_len = 0;
  c->zip_write_route[0] = c->zip_write_route[1] = 0;
  if (n == 0) {  // the empty archive: the end record alone
    uint8_t end[kZipEndLen];
    (void)zip_put_end(end, 0, 0, 0);
    if (out_cap < kZipEndLen) return FLATE_HIP_E_OUT_TOO_SMALL;
    if (flags & FLATE_HIP_DEVICE_PTRS) {
      HIP_TRY(c, hipSetDevice(c->device));
      HIP_TRY(c, hipMemcpyAsync(out, end, kZipEndLen, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else {
      memcpy(out, end, kZipEndLen);
    }
    if (entry_off) entry_off[0] = 0;
    *out_len = kZipEndLen;
    return FLATE_HIP_OK;
  }
  // the option "zip_piece_bytes": with at least one entry longer than P the entries are the groups of a grouped call;
  // otherwise today's route -- the same kernels, no new launch, no new allocation
  if (c->zip_piece_bytes) {
    uint32_t long_entries = 0;
    const uint64_t pieces = zip_pieces_count(in_off, n, c->zip_piece_bytes, &long_entries);
    if (long_entries) {
      if (pieces > 0xfffffffeull) return FLATE_HIP_E_TOO_LARGE;
      for (uint32_t i = 0; i < n; ++i)  // (what the plain route refuses: an entry's sizes are 32-bit fields)
        if (in_off[i + 1] - in_off[i] >= 0x7ffe0000ull) return FLATE_HIP_E_TOO_LARGE;
      try {
        std::vector<uint64_t> piece_in_off((size_t)pieces + 1);
        std::vector<uint32_t> group_off((size_t)n + 1);
        zip_pieces_plan(in_off, n, c->zip_piece_bytes, piece_in_off.data(), group_off.data());
        const int r = zip_deflate_pieces(c, in, piece_in_off.data(), (uint32_t)pieces, group_off.data(), n, names, name_off, out,
                                         out_cap, out_len, entry_off, flags);
        if (r == FLATE_HIP_OK) c->zip_write_route[0] = long_entries, c->zip_write_route[1] = (uint32_t)pieces;
        return r;
      } catch (const std::exception &e) {  // (out of host memory in an index vector)
        c->hip_err = e.what();
        return FLATE_HIP_E_INTERNAL;
      }
    }
  }
  return zip_deflate(c, in, in_off, n, names, name_off, out, out_cap, out_len, entry_off, flags);
}

int flate_hip_zip_index(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint64_t index_cap, flate_hip_zip_entry *entries,
                        uint64_t *out_off, uint32_t *n_entries, uint64_t *out_bytes, int64_t *err_off, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = zip_index_args(in, in_len, entries, out_off, n_entries, out_bytes, flags);
  if (rc) return rc;
  c->hip_err.clear();
  *n_entries = 0, *out_bytes = 0;
  if (err_off) *err_off = -1;
  const uint8_t *d_in = nullptr;
  if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
  ZipFound F;
  if ((rc = zip_discover(c, d_in, in_len, F))) return rc;
  *n_entries = F.n;
  if (F.rc) {
    if (err_off) *err_off = F.err_off;
    return F.rc;
  }
  *out_bytes = F.out_bytes;
  if (!entries) return FLATE_HIP_OK;
  if (index_cap < F.n) return FLATE_HIP_E_OUT_TOO_SMALL;
  out_off[F.n] = F.out_bytes;
  if (F.n == 0) return FLATE_HIP_OK;
  HIP_TRY(c, hipMemcpyAsync(entries, F.d_entries, (size_t)F.n * sizeof(flate_hip_zip_entry), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(out_off, F.d_out_off, ((size_t)F.n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FLATE_HIP_OK;
}

int flate_hip_zip_read(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, const uint32_t *sel, uint32_t n_sel,
                       uint32_t n_cap, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint64_t *out_len, int32_t *status,
                       int64_t *err_off, uint32_t *n_entries, int64_t *archive_err_off, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = zip_read_args(in, in_len, sel, n_sel, n_cap, out, out_cap, out_off, out_len, status, err_off, flags);
  if (rc) return rc;
  c->hip_err.clear();
  for (uint32_t &w : c->zip_route) w = 0;
  if (n_entries) *n_entries = 0;
  if (archive_err_off) *archive_err_off = -1;
  out_off[0] = 0;
  try {
    const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
    const uint8_t *d_in = nullptr;
    if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
    for (int k = 0; k < FLATE_HIP_STAGE_COUNT; ++k) c->stage_ms[k] = 0;
    ZipFound F;
    if ((rc = zip_discover(c, d_in, in_len, F))) return rc;
    if (n_entries) *n_entries = F.n;
    if (F.rc) {  // a malformed archive: nothing is decoded, nothing is written
      if (archive_err_off) *archive_err_off = F.err_off;
      return F.rc;
    }
    const uint32_t n = F.n, ns = sel ? n_sel : n;
    if (ns > n_cap) return sel ? FLATE_HIP_E_INVALID : FLATE_HIP_E_OUT_TOO_SMALL;
    if (sel)
      for (uint32_t j = 0; j < ns; ++j)
        if (sel[j] >= n) return FLATE_HIP_E_INVALID;
    if (ns == 0) return FLATE_HIP_OK;

    // the index comes back once, 64 bytes per entry: the selection, the decoders' routing and the checksum plan are
    // host code over it
    std::vector<flate_hip_zip_entry> ent(n);
    HIP_TRY(c, hipMemcpyAsync(ent.data(), F.d_entries, (size_t)n * sizeof(flate_hip_zip_entry), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<ZipSel> zs(ns);
    std::vector<ZipCopyPiece> pieces;
    std::vector<uint64_t> soff((size_t)ns + 1), send(ns);
    uint32_t n_deflate = 0;
    for (uint32_t j = 0; j < ns; ++j) {
      const flate_hip_zip_entry &e = ent[sel ? sel[j] : j];
      ZipSel &s = zs[j];
      s = ZipSel{e.data_off, e.comp_size, e.size, e.crc32, e.status, e.method, 0};
      if (!s.status && (e.size > 0xffffffffull || (e.method == 8 && e.comp_size >= 0x7ffe0000ull))) s.status = FLATE_HIP_E_TOO_LARGE;
      if (!s.status && (e.data_off > in_len || e.comp_size > in_len - e.data_off)) {
        c->hip_err = "ZIP read: an entry with status 0 outside the archive";
        return FLATE_HIP_E_INTERNAL;
      }
      out_off[j + 1] = out_off[j] + (s.status ? 0ull : e.size);
      const bool deflate = !s.status && e.method == 8;
      soff[j] = deflate ? e.data_off : 0ull, send[j] = deflate ? e.data_off + e.comp_size : 0ull;
      n_deflate += deflate ? 1u : 0u;
      if (!s.status && e.method == 0)
        for (uint64_t at = 0; at < e.size; at += kZipCopyPiece)
          pieces.push_back({out_off[j] + at, e.data_off + at, (uint32_t)(e.size - at < kZipCopyPiece ? e.size - at : kZipCopyPiece), 0});
    }
    soff[ns] = in_len;
    const uint64_t total = out_off[ns];
    if (total > out_cap) return FLATE_HIP_E_OUT_TOO_SMALL;  // (the size query too: nothing is decoded)
    if (pieces.size() > 0x7fffffffull) return FLATE_HIP_E_TOO_LARGE;
    uint8_t *d_out = out;
    if (!dev) {
      if ((rc = ensure(c, c->d_out, total + 16))) return rc;
      d_out = (uint8_t *)c->d_out.p;
    }

    // the option "zip_unit_min": the LONG entries (zip_units_rule.h: the set L) as one chain of units over their hull,
    // decoded straight into their slots; the entries L[0, g) that come out GOOD are an empty range to the batch
    // decoders, every other one is theirs as with the option off
    uint32_t g = 0;
    ZipUnitsDecParams UG{};
    if (c->zip_unit_min) {
      std::vector<ZuEntry> L;
      std::vector<ZuRange> LR;
      uint32_t fallback = 0, n_units = 0, n_cand = 0;
      zip_units_form(ent.data(), n, sel, ns, out_off, c->zip_unit_min, L, LR, &fallback);
      if (!L.empty()) {
        uint64_t hull_lo = 0, hull_hi = 0;
        zip_units_hull(L, LR, &hull_lo, &hull_hi);
        if ((rc = zip_units_decode(c, d_in, hull_lo, hull_hi, L, LR, d_out, total, &g, UG, &n_units, &n_cand))) return rc;
        for (uint32_t e = 0; e < g; ++e) soff[L[e].slot] = send[L[e].slot] = 0ull;
        n_deflate -= g;
      }
      c->zip_route[0] = g, c->zip_route[1] = fallback + ((uint32_t)L.size() - g);
      c->zip_route[2] = n_units, c->zip_route[3] = n_cand;
    }

    // the batch decoders over the entries of method 8 (every other entry is an empty range to them, and its result is
    // replaced by zip_prep_kernel)
    if (n_deflate) {
      rc = inflate_ranges_device(c, d_in, soff.data(), send.data(), ns, d_out, out_off, out_len, status, err_off);
      if (!is_stream_status(rc)) return rc;
    } else {
      if ((rc = ensure(c, c->d_out_len, (size_t)ns * 8 + 8))) return rc;
      if ((rc = ensure(c, c->d_istatus, (size_t)ns * 4 + 4))) return rc;
      if ((rc = ensure(c, c->d_ierr, (size_t)ns * 8 + 8))) return rc;
    }

    // behind them: stored entries, the CRC-32 of what was produced, the verdict
    const size_t o_pieces = ((size_t)ns * sizeof(ZipSel) + 255) & ~(size_t)255;
    if ((rc = ensure(c, c->d_zip_sel, o_pieces + pieces.size() * sizeof(ZipCopyPiece) + 256))) return rc;
    if ((rc = ensure(c, c->d_rd_bad, (size_t)ns * 4 + 4))) return rc;
    if ((rc = ensure(c, c->d_frame_sums, (size_t)ns * 4 + 8))) return rc;
    if ((rc = ctl_begin(c, checksum_ctl_up_bytes(out_off, ns) + 1024, (size_t)ns * 20 + 64))) return rc;
    uint8_t *zb = (uint8_t *)c->d_zip_sel.p;
    HIP_TRY(c, hipMemcpyAsync(zb, zs.data(), (size_t)ns * sizeof(ZipSel), hipMemcpyHostToDevice, c->stream));
    if (!pieces.empty())
      HIP_TRY(c, hipMemcpyAsync(zb + o_pieces, pieces.data(), pieces.size() * sizeof(ZipCopyPiece), hipMemcpyHostToDevice, c->stream));
    ZipReadParams R{};
    R.in = d_in;
    R.out = d_out;
    R.sel = (const ZipSel *)zb;
    R.pieces = (const ZipCopyPiece *)(zb + o_pieces);
    R.n_sel = ns;
    R.n_pieces = (uint32_t)pieces.size();
    R.out_len = (uint64_t *)c->d_out_len.p;
    R.status = (int32_t *)c->d_istatus.p;
    R.err_off = (int64_t *)c->d_ierr.p;
    R.bad = (uint32_t *)c->d_rd_bad.p;
    R.sums = (const uint32_t *)c->d_frame_sums.p;
    R.decoded = n_deflate ? 1u : 0u;
    {
      StageTimer t(c, FLATE_HIP_STAGE_CHECKSUM);
      hipLaunchKernelGGL(zip_prep_kernel, dim3((ns + 255) / 256), dim3(256), 0, c->stream, R);
      if (g) {  // the entries the units served: judged by the same checksums and the same verdict as every other
        UG.g = g;
        UG.z_out_len = R.out_len, UG.z_status = R.status, UG.z_err_off = R.err_off;
        hipLaunchKernelGGL(zip_units_verdict_kernel, dim3((g + 255) / 256), dim3(256), 0, c->stream, UG);
      }
      if (R.n_pieces) hipLaunchKernelGGL(zip_copy_kernel, dim3(R.n_pieces), dim3(256), 0, c->stream, R);
      if ((rc = checksum_device_clipped(c, d_out, out_off, ns, FLATE_HIP_CHECKSUM_CRC32, R.out_len, R.status, R.bad,
                                        (uint32_t *)c->d_frame_sums.p)))
        return rc;
      hipLaunchKernelGGL(zip_verdict_kernel, dim3((ns + 255) / 256), dim3(256), 0, c->stream, R);
    }
    HIP_TRY(c, hipGetLastError());
    if ((rc = ctl_down(c, out_len, R.out_len, (size_t)ns * 8))) return rc;
    if ((rc = ctl_down(c, status, R.status, (size_t)ns * 4))) return rc;
    if ((rc = ctl_down(c, err_off, R.err_off, (size_t)ns * 8))) return rc;
    if (!dev && total) HIP_TRY(c, hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ctl_finish(c);
    const float inflate_ms = c->stage_ms[FLATE_HIP_STAGE_INFLATE];  // (the decode driver has collected its own)
    // (units alone: the inflate stage is the last round's decoder launch, whose events nothing has collected yet)
    const bool units_alone = g != 0 && n_deflate == 0;
    const bool used[FLATE_HIP_STAGE_COUNT] = {false, false, true, units_alone};
    if ((rc = collect_timing(c, used))) return rc;
    if (!units_alone) c->stage_ms[FLATE_HIP_STAGE_INFLATE] = inflate_ms;
    for (uint32_t j = 0; j < ns; ++j)
      if (status[j]) return status[j];
    return FLATE_HIP_OK;
  } catch (const std::exception &e) {  // (out of host memory in an index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

}  // extern "C"
