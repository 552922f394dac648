// flate_api_units.hip -- the decode calls of the C ABI that cut long DEFLATE data into parallel UNITS (see
// include/flate_hip.h): flate_hip_inflate_one*, flate_hip_gzfile_* and the long entries of flate_hip_zip_read
// (flate_host::zip_units_decode).  The batch calls, BGZF, plain gzip members and the piecewise stream are
// flate_api_inflate.hip's; the decoders' launch (launch_decoders) is shared through flate_ctx.h.
#include "flate_ctx.h"

#include <cstring>
#include <exception>
#include <stdexcept>

#include "api_checks.h"
#include "bgzf_range_rule.h"
#include "gzfile_parts_rule.h"
#include "gzfile_parts_serial_rule.h"
#include "gzfile_rule.h"
#include "gzip_rule.h"
#include "unit_discovery.h"
#include "unit_rounds.h"

using namespace flate;
using namespace flate_host;

// ---- one long stream: block discovery (one_kernels.hip, one_probe_kernel.inc) ----
namespace {

// The container around ONE stream as the device reads it: one_init_kernel leaves the raw stream's range {0, in_len} in
// `one`, and for zlib / gzip frame_parse_kernel moves it behind the header and in front of the trailer, by the header
// rules of flate_hip_inflate_spliced_framed (no dictionaries: FDICT is bad).
void one_parse_launch(flate_hip_ctx *c, const uint8_t *d_in, uint64_t in_len, FrameOne *one, uint32_t wrap) {
  hipLaunchKernelGGL(one_init_kernel, dim3(1), dim3(64), 0, c->stream, one, in_len);
  if (wrap == FLATE_HIP_WRAP_RAW) return;
  FrameReadParams R{};
  R.in = d_in;
  R.in_off = one->in_off;
  R.n_streams = 1;
  R.wrap = wrap;
  R.pay_off = one->pay_off;
  R.pay_end = &one->pay_end;
  R.want = &one->want;
  R.isize = &one->isize;
  R.bad = &one->bad;
  R.dict_used = &one->dict_used;
  hipLaunchKernelGGL(frame_parse_kernel, dim3(1), dim3(256), 0, c->stream, R);
}

// The discovery over the ONE stream d_in[0, in_len) (DEVICE memory) on the ctx's stream: the container's header, count
// and scan, ONE read-back of the candidate count (the launches behind it have a thread or a wavefront per candidate),
// then fill, probe, link, rounds, finish, out-scan, the tail probe and ONE read-back of the result words H with the
// index (P.C.member_off / P.C.out_off on the device; null when the header is bad).  Counted in no
// profiling stage.
// index_cap != 0: the first min(index_cap, candidates + 1) entries of unit_bit / out_off come back into `index` (the
// two arrays one after the other) in the same read-back as H -- the units are a subset of the candidates, so what fits
// the caller's arrays is known before the chain is.
// part != null: d_in[0, in_len) is one PART of a stream read in parts (flate_hip_one_reader_read) -- the handle's unit
// rule, one_part_init_kernel in the parse kernels' place, the chain's root at bit part->b0.
struct OnePart {
  uint64_t unit_max;      // the handle's "one_unit_max" and "one_stored_units", recorded at open
  uint32_t stored_units;
  uint32_t b0, first, final_in;
};
int one_discover(flate_hip_ctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t wrap, uint64_t index_cap, OneHead &H,
                 OneParams &P, std::vector<uint64_t> &index, const OnePart *part = nullptr) {
  int rc;
  P = OneParams{};
  ChainParams &C = P.C;
  C.in = d_in;
  C.in_len = in_len;
  P.unit_max = part ? part->unit_max : c->one_unit_max;
  P.stored_units = part ? part->stored_units : c->one_stored_units;
  if ((rc = tiles_for(d_in, 0, in_len, &C.n_tiles))) return rc;
  rc = carve(c, c->d_one_tiles, [&](Carve &k) {
    k.take(P.head, 1);
    k.take(P.one, 1);
    k.take(C.tile_cnt, (size_t)C.n_tiles + 1);
  });
  if (rc) return rc;
  C.head = &P.head->h;
  if (part)
    hipLaunchKernelGGL(one_part_init_kernel, dim3(1), dim3(64), 0, c->stream, P.one, d_in, in_len, wrap, part->first,
                       part->final_in, part->b0);
  else
    one_parse_launch(c, d_in, in_len, P.one, wrap);
  find_count(c, P, part != nullptr);
  if ((rc = find_counts_back(c, P.head, H))) return rc;
  const uint32_t cap = H.h.n_cand;
  if ((rc = chain_size(C, cap))) return rc;  // (the count saturates at 2^32 - 1)
  if (cap == 0) return FLATE_HIP_OK;  // (a bad header: the scan kernel has left FLATE_HIP_E_CORRUPT at offset 0)

  const size_t n = cap;
  if ((rc = carve(c, c->d_one, [&](Carve &k) { chain_nodes_take(k, P, n, [](Carve &) {}); }))) return rc;
  one_find_launch(c, false, C.n_tiles, P, part != nullptr);
  one_probe_launch(c, cap, P, 0u);
  if ((rc = chain_tail(c, C, part ? one_part_link_kernel : one_link_kernel, P, one_finish_kernel, one_out_scan_kernel, P)))
    return rc;
  one_probe_launch(c, 1, P, 1u);
  HIP_TRY(c, hipGetLastError());
  // ONE read-back behind the count: the result words, then 16 bytes per unit
  const size_t take = (size_t)(index_cap < n + 1 ? index_cap : n + 1);
  index.assign(2 * take, 0);
  HIP_TRY(c, hipMemcpyAsync(&H, P.head, sizeof H, hipMemcpyDeviceToHost, c->stream));
  if (take) {
    HIP_TRY(c, hipMemcpyAsync(index.data(), P.C.member_off, take * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(index.data() + take, P.C.out_off, take * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FLATE_HIP_OK;
}

// ---- what the two reads through a seek index share (flate_hip_inflate_one_ranges, flate_hip_gzfile_ranges) ----

// c->d_one_dec for rounds over the ns selected units: per round the seeds, the pieces and what DECODE reports for
// them, and per selected unit the status the check kernel folds
int seek_rounds_carve(flate_hip_ctx *c, OneDecParams &D, OneSeekRoundParams &S, UnitResults &dec, uint32_t ns, uint32_t per_round) {
  const int rc = unit_rounds_carve(c, D, ns, per_round, [&](Carve &k) {
    k.take(S.seed, per_round);
    k.take(S.p_bit_off, per_round);
    k.take(S.p_bit_end, per_round);
    k.take(D.p_dict_at, per_round);
    k.take(D.p_dict_len, per_round);
    dec.take(k, per_round);
    k.take(S.u_status, ns);
  });
  if (rc) return rc;
  S.p_dict_at = D.p_dict_at;  // (the kernels of the rounds read these through S)
  S.p_dict_len = D.p_dict_len;
  S.R = D.R;
  S.d_status = dec.status;
  S.d_out_len = dec.out_len;
  return FLATE_HIP_OK;
}
// the workgroups of a load kernel: 16 of a round's 256-entry blocks each
uint32_t seek_load_blocks(uint32_t count) {
  return ((uint32_t)(((uint64_t)count * kWinEntries + 255) / 256) + 15u) / 16u;
}

// where a read through a seek index delivers, and the ranges' layout as the host has read it back
struct SeekRangesOut {
  uint8_t *out;
  uint32_t nr;
  uint64_t out_total, scratch_total;  // bytes of all ranges, of all decoded units
  const uint32_t *r_lo, *r_hi;        // range r touches the selected units [r_lo[r], r_hi[r])
  const uint32_t *sel;                // the selected units
  int32_t *range_status;
  uint32_t *bad_unit;
  bool dev;
  // packed windows: the places in the list of the points whose block did not inflate -- FLATE_HIP_E_CORRUPT there
  const uint32_t *bad_place = nullptr;
  uint32_t n_bad_place = 0;
};

// The rounds over the ns selected units and what follows them: `seeds` (the caller's seed and load kernels, which set
// S.i0 / S.count) in front of TAIL, the segmented scan, DECODE of the round's units as spliced pieces of in[0, in_len)
// with dictionaries, each with its own end, into their dense slots, the per-unit check; then the gather of every
// range's run of the scratch to its place in out, ONE read-back and the statuses.
template <class Seeds>
int seek_ranges_decode(flate_hip_ctx *c, OneDecParams &D, OneSeekRoundParams &S, const UnitResults &dec, uint32_t per_round,
                       uint32_t ns, const uint8_t *in, uint64_t in_len, const SeekRangesOut &O, Seeds seeds) {
  int rc;
  if ((rc = ensure(c, c->d_one_seek_dense, O.scratch_total + 64))) return rc;
  uint8_t *d_dense = (uint8_t *)c->d_one_seek_dense.p;
  uint8_t *d_out;
  if ((rc = unit_out_buffer(c, O.out, O.dev, O.out_total, d_out))) return rc;
  auto decode = [&](uint32_t i0, uint32_t count) {
    const int r = unit_decode(c, unit_decode_params(D, in, in_len, S.p_bit_off, S.p_bit_end, false, count, d_dense,
                                                    S.Q.sel_at + i0, dec));
    if (r) return r;
    hipLaunchKernelGGL(one_seek_check_kernel, dim3((count + 255u) / 256u), dim3(256), 0, c->stream, S);
    return FLATE_HIP_OK;
  };
  if ((rc = unit_rounds(c, D, nullptr, S.seed, 0, ns, ns, per_round, seeds, unit_no_hook, decode))) return rc;
  if ((rc = ranges_gather(c, d_dense, d_out, S.Q.r_out_off, S.Q.r_src, O.nr, O.out_total))) return rc;
  HIP_TRY(c, hipGetLastError());
  std::vector<int32_t> st(ns);
  HIP_TRY(c, hipMemcpyAsync(st.data(), S.u_status, (size_t)ns * 4, hipMemcpyDeviceToHost, c->stream));
  if (!O.dev) HIP_TRY(c, hipMemcpyAsync(O.out, d_out, O.out_total, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  bool used[FLATE_HIP_STAGE_COUNT] = {false, false, false, false};
  used[FLATE_HIP_STAGE_INFLATE] = true;
  if (c->profiling && (rc = collect_timing(c, used))) return rc;
  for (uint32_t j = 0; j < O.n_bad_place; ++j) st[O.bad_place[j]] = FLATE_HIP_E_CORRUPT;
  const uint32_t bad = range_statuses(st.data(), ns, O.r_lo, O.r_hi, O.nr, O.range_status, nullptr);
  if (bad == ns) return FLATE_HIP_OK;
  if (O.bad_unit) *O.bad_unit = O.sel[bad];
  return st[bad];
}

}  // namespace

extern "C" {

int flate_hip_inflate_one_index(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t wrap, uint64_t index_cap,
                                uint64_t *unit_bit, uint64_t *out_off, uint32_t *n_units, uint64_t *out_bytes,
                                uint32_t *n_candidates, int32_t *status, int64_t *err_off, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = one_index_args(in, in_len, wrap, unit_bit, out_off, n_units, out_bytes, status, flags);
  if (rc) return rc;
  c->hip_err.clear();
  *n_units = 0, *out_bytes = 0, *status = 0;
  if (n_candidates) *n_candidates = 0;
  if (err_off) *err_off = -1;
  OneHead H{};
  try {
    OneParams P{};
    std::vector<uint64_t> index;
    if (in_len == 0) {  // no header at all, or a raw stream that ends in front of its first block header
      H.h.rc = wrap == FLATE_HIP_WRAP_RAW ? FLATE_HIP_E_UNEXPECTED_EOF : FLATE_HIP_E_CORRUPT;
      H.h.err_off = wrap == FLATE_HIP_WRAP_RAW ? -1 : 0;
    } else {
      const uint8_t *d_in = nullptr;
      if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
      if ((rc = one_discover(c, d_in, in_len, wrap, unit_bit ? index_cap : 0, H, P, index))) return rc;
    }
    *n_units = H.h.n_members;
    if (n_candidates) *n_candidates = H.h.n_cand;
    *status = H.h.rc;
    if (err_off) *err_off = H.h.rc ? H.h.err_off : -1;
    *out_bytes = H.h.out_bytes;  // (0 unless the chain reaches the final block)
    // the index -- of a stream that fails its good prefix, if that fits: the verdict is the serial decoder's either way
    const uint64_t entries = (uint64_t)H.h.n_members + 1;
    if (unit_bit && index_cap >= entries) {
      if (index.size() >= 2 * entries) {
        memcpy(unit_bit, index.data(), entries * 8);
        memcpy(out_off, index.data() + index.size() / 2, entries * 8);
      } else {  // (a bad header or no input: zero units in front of offset 0)
        unit_bit[0] = 0, out_off[0] = 0;
      }
    }
    if (H.h.rc) return H.h.rc;
    return unit_bit && index_cap < entries ? FLATE_HIP_E_OUT_TOO_SMALL : FLATE_HIP_OK;
  } catch (const std::exception &e) {  // (out of host memory in the index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

// The whole call: discovery, then the units decoded in parallel in rounds of "one_round_units" -- TAIL (symbolic
// windows), COMPOSE (a scan of the tail functions), DECODE (the units again, each with its resolved 32 KiB of history,
// straight into out + out_off[k]) --, then the checksum of out[0, total) and the verdict.  Behind the discovery's two
// read-backs the host reads nothing but the result words.
int flate_hip_inflate_one(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t wrap, uint8_t *out, uint64_t out_cap,
                          uint64_t *out_len, int32_t *status, int64_t *err_off, uint32_t *n_units, uint32_t *n_candidates,
                          uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = one_args(in, in_len, wrap, out, out_cap, out_len, status, flags);
  if (rc) return rc;
  c->hip_err.clear();
  *out_len = 0, *status = 0;
  if (err_off) *err_off = -1;
  if (n_units) *n_units = 0;
  if (n_candidates) *n_candidates = 0;
  auto verdict = [&](int st, int64_t eo) {
    *status = st;
    if (err_off) *err_off = st ? eo : -1;
    return st;
  };
  if (in_len == 0)
    return wrap == FLATE_HIP_WRAP_RAW ? verdict(FLATE_HIP_E_UNEXPECTED_EOF, -1) : verdict(FLATE_HIP_E_CORRUPT, 0);
  try {
    const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
    const uint8_t *d_in = nullptr;
    if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
    OneHead H{};
    OneParams P{};
    std::vector<uint64_t> none;
    if ((rc = one_discover(c, d_in, in_len, wrap, 0, H, P, none))) return rc;
    if (n_units) *n_units = H.h.n_members;
    if (n_candidates) *n_candidates = H.h.n_cand;
    if (H.h.n_cand == 0) return verdict(H.h.rc, H.h.err_off);  // a bad header
    if (H.h.rc == FLATE_HIP_E_TOO_LARGE || H.h.rc == FLATE_HIP_E_INTERNAL) return verdict(H.h.rc, H.h.err_off);
    // the units to decode: the good ones and, so that the bytes in front of an error are delivered, a unit that fails
    // behind its header; the total is known here
    const uint32_t n_dec = H.h.n_members + (H.fail_unit ? 1u : 0u);
    const uint64_t total = H.prefix_bytes + (H.fail_unit ? H.fail_out : 0ull);
    *out_len = total;
    if (total > out_cap) return FLATE_HIP_E_OUT_TOO_SMALL;  // (nothing is decoded; out == NULL: the size query)
    uint8_t *d_out;
    if ((rc = unit_out_buffer(c, out, dev, total, d_out))) return rc;
    const uint32_t per_round = unit_per_round(c, n_dec);
    OneDecParams D{};
    uint32_t *d_sum;
    UnitResults dec;
    rc = unit_rounds_carve(
        c, D, n_dec, per_round, [&](Carve &k) { unit_pieces_take(k, D, &dec, per_round); },
        [&](Carve &k) { k.take(d_sum, 4); });  // (the checksum's words stand in front of the function arrays)
    if (rc) return rc;
    if ((rc = unit_dec_params(c, D, d_in, P.one, P.C.member_off, P.C.out_off, P.stored_units, true))) return rc;
    unit_verdict_params(D, total, dec, P.head, wrap, in_len);
    // DECODE: the round's units as spliced pieces with dictionaries, through the lane-per-stream decoder.  The
    // stream's last piece runs to BFINAL (or to its failure); every other round's last piece ends where the next
    // unit starts, and so does the last unit of a chain that stopped at a header the decoder refuses.
    auto decode = [&](uint32_t u0, uint32_t count) {
      const bool closed = u0 + count < n_dec || (H.h.rc != 0 && !H.fail_unit);
      return unit_decode_chain(c, D, d_in + H.raw_off, H.raw_len, u0, count, closed, d_out, dec);
    };
    if ((rc = unit_rounds(c, D, nullptr, nullptr, 0, n_dec, n_dec, per_round, unit_no_hook, unit_no_hook, decode))) return rc;
    bool used[FLATE_HIP_STAGE_COUNT] = {false, false, false, false};
    used[FLATE_HIP_STAGE_INFLATE] = n_dec != 0;
    bool ctl = false;
    if (wrap != FLATE_HIP_WRAP_RAW && total) {
      const uint64_t whole[2] = {0, total};
      if ((rc = ctl_begin(c, checksum_ctl_up_bytes(whole, 1), 0))) return rc;
      ctl = true;
      D.sum = d_sum;
      if ((rc = checksum_device(c, d_out, whole, 1, frame_sum_kind(wrap), d_sum, FLATE_HIP_STAGE_CHECKSUM)))
        return rc;
      used[FLATE_HIP_STAGE_CHECKSUM] = true;
    }
    hipLaunchKernelGGL(one_verdict_kernel, dim3(1), dim3(64), 0, c->stream, D);
    HIP_TRY(c, hipGetLastError());
    OneDecHead R{};
    HIP_TRY(c, hipMemcpyAsync(&R, D.dh, sizeof R, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (ctl) ctl_finish(c);
    if ((rc = unit_deliver(c, out, d_out, dev, R.out_len, total, out_len))) return rc;
    if (c->profiling && (rc = collect_timing(c, used))) return rc;
    return verdict(R.status, R.err_off);
  } catch (const std::exception &e) {
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

// The seek index: discovery, POINTS, then per round TAIL / COMPOSE / RESOLVE as above and, in DECODE's place, PACK: the
// windows in front of the round's point units into their blocks.  Nothing is decoded to output.
int flate_hip_inflate_one_seek_index(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t wrap, uint64_t span,
                                     uint64_t *index, uint64_t index_cap_words, uint64_t *index_words, uint8_t *windows,
                                     uint64_t windows_cap, uint64_t *windows_bytes, uint32_t *n_units, uint32_t *n_points,
                                     uint64_t *out_bytes, uint32_t *n_candidates, int32_t *status, int64_t *err_off,
                                     uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = one_seek_index_args(in, in_len, wrap, index, index_cap_words, index_words, windows, windows_cap, windows_bytes,
                               n_units, n_points, out_bytes, status, flags);
  if (rc) return rc;
  c->hip_err.clear();
  *index_words = 0, *windows_bytes = 0, *n_units = 0, *n_points = 0, *out_bytes = 0, *status = 0;
  if (n_candidates) *n_candidates = 0;
  if (err_off) *err_off = -1;
  auto verdict = [&](int st, int64_t eo) {  // a stream that fails gets no index
    *status = st;
    if (err_off) *err_off = st ? eo : -1;
    if (st) *index_words = 0, *windows_bytes = 0, *n_points = 0, *out_bytes = 0;
    return st;
  };
  if (in_len == 0)
    return wrap == FLATE_HIP_WRAP_RAW ? verdict(FLATE_HIP_E_UNEXPECTED_EOF, -1) : verdict(FLATE_HIP_E_CORRUPT, 0);
  span = seek_span(span);
  try {
    const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
    const uint8_t *d_in = nullptr;
    if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
    OneHead H{};
    OneParams P{};
    std::vector<uint64_t> found;  // unit_bit, then out_off: one entry per candidate and one more, the units in front
    if ((rc = one_discover(c, d_in, in_len, wrap, ~0ull, H, P, found))) return rc;
    const uint32_t n = H.h.n_members;
    *n_units = n;
    if (n_candidates) *n_candidates = H.h.n_cand;
    if (H.h.n_cand == 0) return verdict(H.h.rc, H.h.err_off);  // a bad header
    if (H.h.rc == FLATE_HIP_E_TOO_LARGE || H.h.rc == FLATE_HIP_E_INTERNAL) return verdict(H.h.rc, H.h.err_off);
    const bool sound = H.h.rc == 0;  // (a stream that fails is still walked: an earlier unit's distance may fail first)
    const uint32_t n_dec = n + (H.fail_unit ? 1u : 0u);
    const uint32_t per_round = unit_per_round(c, n_dec);

    // POINTS: mark, scan, compact; the sizes are known here, in front of TAIL
    OneSeekPointsParams PP{};
    uint64_t *d_r_out_off, *d_r_src;
    rc = carve(c, c->d_one_seek, [&](Carve &k) {
      k.take(PP.n_points, 1);
      k.take(PP.point_unit, (size_t)n + 1);
      k.take(d_r_out_off, (size_t)per_round + 1);
      k.take(d_r_src, per_round);
    });
    if (rc) return rc;
    std::vector<uint64_t> points;
    FrameOne one{};
    uint32_t np = 0;
    uint64_t need_words = 0, need_bytes = 0;
    if (sound) {
      PP.out_off = P.C.out_off;
      PP.n = n;
      PP.span = span;
      hipLaunchKernelGGL(one_seek_points_kernel, dim3(1), dim3(1024), 0, c->stream, PP);
      HIP_TRY(c, hipGetLastError());
      points.assign(n, 0);
      HIP_TRY(c, hipMemcpyAsync(&np, PP.n_points, 4, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(points.data(), PP.point_unit, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(&one, P.one, sizeof one, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      if (np < 1u || np > n || found.size() < 2 * ((size_t)n + 1)) {
        c->hip_err = "seek index: the point count does not fit the units";
        return FLATE_HIP_E_INTERNAL;
      }
      need_words = seek_index_words(n, np);
      need_bytes = seek_windows_bytes(np);
      *index_words = need_words, *windows_bytes = need_bytes, *n_points = np, *out_bytes = H.h.out_bytes;
      if (index_cap_words < need_words || windows_cap < need_bytes) return FLATE_HIP_E_OUT_TOO_SMALL;  // (the size query too)
    }
    uint8_t *d_windows = windows;
    if (sound && !dev && need_bytes) {
      if ((rc = ensure(c, c->d_one_seek_win, need_bytes + 16))) return rc;
      d_windows = (uint8_t *)c->d_one_seek_win.p;
    }

    OneDecParams D{};
    if ((rc = unit_rounds_carve(c, D, n_dec, per_round, [](Carve &) {}))) return rc;
    if ((rc = unit_dec_params(c, D, d_in, P.one, P.C.member_off, P.C.out_off, P.stored_units, true))) return rc;
    uint32_t p_next = 1;  // the first point whose window is not packed yet (point 0 has none)
    // PACK: R[i] of the round's point units -> their blocks, which lie one behind the other in `windows`
    auto pack = [&](uint32_t u0, uint32_t count) {
      uint32_t p_hi = p_next;
      while (p_hi < np && points[p_hi] < (uint64_t)u0 + count) ++p_hi;
      if (p_hi == p_next) return FLATE_HIP_OK;
      const uint32_t cnt = p_hi - p_next;
      hipLaunchKernelGGL(one_seek_pack_kernel, dim3((cnt + 1u + 255u) / 256u), dim3(256), 0, c->stream, PP.point_unit, p_next,
                         cnt, u0, d_r_out_off, d_r_src);
      uint8_t *blocks = d_windows + (uint64_t)(p_next - 1u) * kSeekWindow;
      p_next = p_hi;
      return ranges_gather(c, D.R, blocks, d_r_out_off, d_r_src, cnt, (uint64_t)cnt * kSeekWindow);
    };
    if ((rc = unit_rounds(c, D, nullptr, nullptr, 0, n_dec, n_dec, per_round, unit_no_hook, unit_no_hook, pack))) return rc;
    OneDecHead bad{};
    if ((rc = unit_first_bad(c, D, n_dec, bad))) return rc;
    // TAIL's verdict: the serial decoder's, at the serial offset
    if (bad.first_bad != 0xffffffffu) return verdict(bad.status ? bad.status : FLATE_HIP_E_INTERNAL, bad.err_off);
    if (!sound) return verdict(H.h.rc, H.h.err_off);
    if (p_next != np) return FLATE_HIP_E_INTERNAL;
    if (!dev && need_bytes) {
      HIP_TRY(c, hipMemcpyAsync(windows, d_windows, need_bytes, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    for (uint32_t k = 0; k < kSeekHeadWords; ++k) index[k] = 0;
    index[kSeekMagicAt] = kSeekMagic;
    index[kSeekVersionAt] = kSeekVersion;
    index[kSeekWrapAt] = wrap;
    index[kSeekInLenAt] = in_len;
    index[kSeekRawOffAt] = H.raw_off;
    index[kSeekRawEndAt] = H.raw_off + H.raw_len;
    index[kSeekTotalAt] = H.h.out_bytes;
    index[kSeekSpanAt] = span;
    index[kSeekUnitsAt] = n;
    index[kSeekPointsAt] = np;
    index[kSeekWantAt] = one.want;
    index[kSeekIsizeAt] = one.isize;
    index[kSeekRuleAt] = P.stored_units ? kSeekRuleStored : kSeekRuleDynamic;  // a read walks by this rule
    uint64_t *w = index + kSeekHeadWords;
    memcpy(w, found.data(), ((size_t)n + 1) * 8);
    memcpy(w + (n + 1), found.data() + found.size() / 2, ((size_t)n + 1) * 8);
    memcpy(w + 2 * ((size_t)n + 1), points.data(), (size_t)np * 8);
    return FLATE_HIP_OK;
  } catch (const std::exception &e) {
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

}  // extern "C"

namespace {

// The windows of the selected points as the rounds of a read load them: the raw blocks (d_slot_of == null: block p - 1
// of d_windows), or a dense stage of the SELECTED points' blocks with the point -> slot table (packed windows).
struct OneRangesWin {
  const uint8_t *d_windows = nullptr;
  const uint32_t *d_slot_of = nullptr;
  std::vector<uint32_t> bad_place;  // packed: the places in the list of the points whose block did not inflate
};

// Random access through the seek index, behind the argument checks: locate, select, layout (one_seek_kernels.hip), ONE
// read-back (the parsed container, the ranges' layout, the unit list), win(sel, ns, h_point, np, W) -- the windows of
// the selected points, once the host has the selection --, rounds of TAIL / segmented scan / DECODE over the list into
// a dense scratch, the per-unit check, the gather.
template <class Win>
int one_ranges_run(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t wrap, const uint64_t *index,
                   const uint64_t *begin, const uint64_t *end, uint32_t n_ranges, uint8_t *out, uint64_t out_cap,
                   uint64_t *out_off, int32_t *range_status, uint32_t *n_decoded, uint32_t *bad_unit, uint32_t flags, Win win) {
  int rc;
  c->hip_err.clear();
  if (n_decoded) *n_decoded = 0;
  if (bad_unit) *bad_unit = 0xffffffffu;
  if (n_ranges == 0) {
    if (out_off) out_off[0] = 0;
    return FLATE_HIP_OK;
  }
  const uint32_t nr = n_ranges;
  try {
    const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
    const uint8_t *d_in = nullptr;
    if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
    const uint32_t n = (uint32_t)index[kSeekUnitsAt], np = (uint32_t)index[kSeekPointsAt];
    const uint64_t raw_off = index[kSeekRawOffAt], raw_end = index[kSeekRawEndAt];
    const uint64_t *h_point = index + kSeekHeadWords + 2 * ((size_t)n + 1);
    const size_t idx_words = 2 * ((size_t)n + 1) + np;

    OneSeekParams Q{};
    Q.n = n, Q.n_points = np, Q.span = index[kSeekSpanAt], Q.n_ranges = nr;
    uint64_t *d_idx, *d_begin, *d_end;
    FrameOne *d_one;
    size_t o_back = 0, o_end = 0;
    rc = carve(c, c->d_one_seek, [&](Carve &k) {
      k.take(d_idx, idx_words);
      k.take(d_begin, nr);
      k.take(d_end, nr);
      k.take(Q.diff, (size_t)n + 1);
      k.take(Q.rank, n);
      k.take(Q.scratch_at, n);
      k.take(Q.r_b, nr);
      k.take(Q.r_len, nr);
      k.take(Q.r_first, nr);
      k.take(Q.r_last, nr);
      k.take(Q.r_seg, nr);
      k.take(Q.r_src, nr);
      k.take(Q.sel_at, (size_t)n + 1);
      o_back = k.at;
      k.take(Q.head, 1);
      k.take(d_one, 1);
      k.take(Q.r_out_off, (size_t)nr + 1);
      k.take(Q.r_rank_lo, nr);
      k.take(Q.r_rank_hi, nr);
      k.take(Q.sel_unit, n);
      o_end = k.at;
    });
    if (rc) return rc;
    Q.unit_bit = d_idx, Q.out_off = d_idx + (n + 1), Q.point_unit = d_idx + 2 * ((size_t)n + 1);
    Q.begin = d_begin, Q.end = d_end;
    const size_t back_bytes = o_end - o_back;
    const uint8_t *d_back = (const uint8_t *)c->d_one_seek.p + o_back;
    HIP_TRY(c, hipMemcpyAsync(d_idx, index + kSeekHeadWords, idx_words * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_begin, begin, (size_t)nr * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_end, end, (size_t)nr * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(Q.diff, 0, ((size_t)n + 1) * 4, c->stream));
    // the container as this stream has it: the raw stream's range and the trailer's words
    one_parse_launch(c, d_in, in_len, d_one, wrap);
    hipLaunchKernelGGL(one_seek_locate_kernel, dim3((nr + 255u) / 256u), dim3(256), 0, c->stream, Q);
    hipLaunchKernelGGL(one_seek_select_kernel, dim3(1), dim3(1024), 0, c->stream, Q);
    hipLaunchKernelGGL(one_seek_layout_kernel, dim3(1), dim3(1024), 0, c->stream, Q);
    HIP_TRY(c, hipGetLastError());
    std::vector<uint8_t> back(back_bytes);
    HIP_TRY(c, hipMemcpyAsync(back.data(), d_back, back_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    auto got = [&](const auto *d) { return (decltype(d))(back.data() + ((const uint8_t *)d - d_back)); };  // d's host copy
    const OneSeekHead RH = *got(Q.head);
    const FrameOne one = *got(d_one);
    const uint32_t *r_lo = got(Q.r_rank_lo), *r_hi = got(Q.r_rank_hi), *sel = got(Q.sel_unit);
    const uint32_t ns = RH.n_sel;
    if (one.bad || one.pay_off[0] != raw_off || one.pay_end != raw_end || one.want != index[kSeekWantAt] ||
        one.isize != index[kSeekIsizeAt]) {  // not the stream the index was built from: nothing is decoded
      for (uint32_t r = 0; r <= nr; ++r) out_off[r] = 0;
      if (range_status)
        for (uint32_t r = 0; r < nr; ++r) range_status[r] = FLATE_HIP_E_CORRUPT;
      return FLATE_HIP_E_CORRUPT;
    }
    if (ns > n) {
      c->hip_err = "seek ranges: more units selected than the stream has";
      return FLATE_HIP_E_INTERNAL;
    }
    memcpy(out_off, got(Q.r_out_off), ((size_t)nr + 1) * 8);
    if (n_decoded) *n_decoded = ns;
    if (range_status)
      for (uint32_t r = 0; r < nr; ++r) range_status[r] = 0;
    if (RH.out_total > out_cap) return FLATE_HIP_E_OUT_TOO_SMALL;  // (the size query too: nothing is decoded)
    if (ns == 0 || RH.out_total == 0) return FLATE_HIP_OK;        // (no range holds a byte)

    OneRangesWin W;
    if ((rc = win(sel, ns, h_point, np, W))) return rc;

    const uint32_t per_round = unit_per_round(c, ns);
    OneDecParams D{};
    OneSeekRoundParams S{};
    UnitResults dec;
    if ((rc = seek_rounds_carve(c, D, S, dec, ns, per_round))) return rc;
    // TAIL by the index's rule, not the context's option
    const uint32_t stored = index[kSeekRuleAt] == kSeekRuleStored ? 1u : 0u;
    if ((rc = unit_dec_params(c, D, d_in, d_one, Q.unit_bit, Q.out_off, stored, false))) return rc;
    D.unit_list = Q.sel_unit;
    S.Q = Q;
    S.windows = W.d_windows;
    auto seeds = [&](uint32_t i0, uint32_t count) {
      S.i0 = i0, S.count = count;
      hipLaunchKernelGGL(one_seek_seed_kernel, dim3((count + 255u) / 256u), dim3(256), 0, c->stream, S);
      if (W.d_slot_of)
        hipLaunchKernelGGL(seek_pack_load_kernel, dim3(seek_load_blocks(count)), dim3(256), 0, c->stream, S, W.d_slot_of);
      else
        hipLaunchKernelGGL(one_seek_load_kernel, dim3(seek_load_blocks(count)), dim3(256), 0, c->stream, S);
      return FLATE_HIP_OK;
    };
    SeekRangesOut O{out, nr, RH.out_total, RH.scratch_total, r_lo, r_hi, sel, range_status, bad_unit, dev};
    O.bad_place = W.bad_place.data();
    O.n_bad_place = (uint32_t)W.bad_place.size();
    return seek_ranges_decode(c, D, S, dec, per_round, ns, d_in + raw_off, raw_end - raw_off, O, seeds);
  } catch (const std::exception &e) {
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

// the selected points behind point 0, rising, with their places in the list
void selected_points(const uint32_t *sel, uint32_t ns, const uint64_t *h_point, uint32_t np, std::vector<uint32_t> &ps,
                     std::vector<uint32_t> *places = nullptr) {
  uint32_t p = 1;
  for (uint32_t i = 0; i < ns && p < np; ++i) {
    while (p < np && h_point[p] < sel[i]) ++p;
    if (p < np && h_point[p] == sel[i]) {
      ps.push_back(p);
      if (places) places->push_back(i);
    }
  }
}

}  // namespace

extern "C" {

int flate_hip_inflate_one_ranges(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t wrap, const uint64_t *index,
                                 uint64_t index_words, const uint8_t *windows, uint64_t windows_bytes, const uint64_t *begin,
                                 const uint64_t *end, uint32_t n_ranges, uint8_t *out, uint64_t out_cap, uint64_t *out_off,
                                 int32_t *range_status, uint32_t *n_decoded, uint32_t *bad_unit, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  const int rc0 = one_ranges_args(in, in_len, wrap, index, index_words, windows, windows_bytes, begin, end, n_ranges, out,
                                  out_cap, out_off, flags);
  if (rc0) return rc0;
  const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
  // the windows: the caller's device buffer, or the blocks of the selected points uploaded into a staged copy
  auto win = [&](const uint32_t *sel, uint32_t ns, const uint64_t *h_point, uint32_t np, OneRangesWin &W) -> int {
    W.d_windows = windows;
    if (dev || !windows_bytes) return FLATE_HIP_OK;
    int rc;
    if ((rc = ensure(c, c->d_one_seek_win, windows_bytes + 16))) return rc;
    uint8_t *stage = (uint8_t *)c->d_one_seek_win.p;
    W.d_windows = stage;
    std::vector<uint32_t> ps;
    selected_points(sel, ns, h_point, np, ps);
    for (size_t a = 0; a < ps.size();) {  // neighbours in the index travel as one copy
      size_t b = a + 1;
      while (b < ps.size() && ps[b] == ps[b - 1] + 1u) ++b;
      const uint64_t at = (uint64_t)(ps[a] - 1u) * kSeekWindow, len = (uint64_t)(b - a) * kSeekWindow;
      HIP_TRY(c, hipMemcpyAsync(stage + at, windows + at, len, hipMemcpyHostToDevice, c->stream));
      a = b;
    }
    return FLATE_HIP_OK;
  };
  return one_ranges_run(c, in, in_len, wrap, index, begin, end, n_ranges, out, out_cap, out_off, range_status, n_decoded,
                        bad_unit, flags, win);
}

}  // extern "C"

// ---- the PACKED windows of the seek index (seek_pack_rule.h; seek_pack_mark_kernel.inc, seek_pack_kernels.hip) ----
namespace {

// The non-empty blocks among the nb of a pack index, rising, and the batch decoders' view of them: stream i is
// packed[off[b_i], off[b_i + 1]) -- the empty blocks between two of them have no bytes, so the streams lie back to back.
struct PackedBlocks {
  std::vector<uint32_t> b;
  std::vector<uint64_t> in_off;
};
PackedBlocks packed_blocks(const uint64_t *off, uint32_t nb) {
  PackedBlocks P;
  for (uint32_t b = 0; b < nb; ++b)
    if (off[b + 1] > off[b]) {
      P.b.push_back(b);
      P.in_off.push_back(off[b]);
    }
  P.in_off.push_back(off[nb]);
  return P;
}

// One launch of the batch decoders: stream i of d_streams (in_off, n + 1) into slot i of 32768 bytes of d_slots.
// good[i]: it inflates with status 0 to exactly 32768 bytes.
int inflate_blocks(flate_hip_ctx *c, const uint8_t *d_streams, const std::vector<uint64_t> &in_off, uint8_t *d_slots,
                   const std::vector<uint64_t> &slot_off, std::vector<uint8_t> &good) {
  const uint32_t n = (uint32_t)in_off.size() - 1u;
  std::vector<uint64_t> out_len(n, 0);
  std::vector<int32_t> status(n, 0);
  std::vector<int64_t> err_off(n, -1);
  good.assign(n, 0);
  if (n == 0) return FLATE_HIP_OK;
  const int rc = flate_hip_inflate_batch(c, d_streams, in_off.data(), n, d_slots, slot_off.data(), out_len.data(), status.data(),
                                         err_off.data(), FLATE_HIP_DEVICE_PTRS);
  int first = 0;  // (the batch call returns its first failing stream's status: that is a verdict per block, not the call's)
  for (uint32_t i = 0; i < n && !first; ++i) first = status[i];
  if (rc && rc != first) return rc;
  for (uint32_t i = 0; i < n; ++i) good[i] = status[i] == 0 && out_len[i] == kSeekWindow;
  return FLATE_HIP_OK;
}

}  // namespace

extern "C" {

size_t flate_hip_seek_windows_pack_bound(uint64_t n_blocks) { return (size_t)n_blocks * flate_hip_deflate_bound(kSeekWindow); }

// MARK + SPARSIFY (or the non-zero test alone), ONE read-back of the per-block records, the non-empty blocks compacted
// in order as one batch through the encoder, the batch's out_off spread over off[].
int flate_hip_seek_windows_pack(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t wrap, const uint64_t *index,
                                uint64_t index_words, const uint8_t *windows, uint64_t windows_bytes, uint32_t mode,
                                uint64_t *pack_index, uint64_t pack_cap_words, uint64_t *pack_words, uint8_t *packed,
                                uint64_t packed_cap, uint64_t *packed_bytes, uint64_t *kept_bytes, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = seek_pack_args(in, in_len, wrap, index, index_words, windows, windows_bytes, mode, pack_index, pack_cap_words,
                          pack_words, packed, packed_cap, packed_bytes, kept_bytes, flags);
  if (rc) return rc;
  c->hip_err.clear();
  const uint32_t n = (uint32_t)index[kSeekUnitsAt], np = (uint32_t)index[kSeekPointsAt], nb = np - 1u;
  const bool sparse = (mode & kSeekPackSparse) != 0, dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
  *pack_words = seek_pack_words(nb), *packed_bytes = 0, *kept_bytes = 0;
  if (pack_cap_words < seek_pack_words(nb)) return FLATE_HIP_E_OUT_TOO_SMALL;
  uint64_t *off = pack_index + kSeekPackHeadWords;
  if (nb == 0) {  // no block: nothing is walked
    seek_pack_head(pack_index, index, mode, 0, 0);
    off[0] = 0;
    return FLATE_HIP_OK;
  }
  try {
    HIP_TRY(c, hipSetDevice(c->device));
    const uint8_t *d_windows = windows;
    if (!dev) {
      if ((rc = ensure(c, c->d_one_seek_win, windows_bytes + 16))) return rc;
      HIP_TRY(c, hipMemcpyAsync(c->d_one_seek_win.p, windows, windows_bytes, hipMemcpyHostToDevice, c->stream));
      d_windows = (const uint8_t *)c->d_one_seek_win.p;
    }
    const size_t idx_words = 2 * ((size_t)n + 1) + np;
    uint64_t *d_idx, *d_r_out_off, *d_r_src;
    FrameOne *d_one;
    SeekPackBlock *d_blk;
    rc = carve(c, c->d_seek_pack, [&](Carve &k) {
      k.take(d_idx, sparse ? idx_words : 0);
      k.take(d_r_out_off, (size_t)nb + 1);
      k.take(d_r_src, nb);
      k.take(d_one, 1);
      k.take(d_blk, nb);
    });
    if (rc) return rc;
    FrameOne one{};
    const uint8_t *d_src = d_windows;  // what the encoder reads: the raw blocks, or the sparsified ones
    if (sparse) {
      const uint8_t *d_in = nullptr;
      if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
      if ((rc = ensure(c, c->d_seek_pack_dense, (size_t)nb * kSeekWindow + 16))) return rc;
      HIP_TRY(c, hipMemcpyAsync(d_idx, index + kSeekHeadWords, idx_words * 8, hipMemcpyHostToDevice, c->stream));
      one_parse_launch(c, d_in, in_len, d_one, wrap);  // the container as this stream has it
      SeekMarkParams M{};
      M.in = d_in, M.in_len = in_len, M.one = d_one;
      M.unit_bit = d_idx, M.out_off = d_idx + (n + 1), M.point_unit = d_idx + 2 * ((size_t)n + 1);
      M.n = n, M.n_points = np;
      M.windows = d_windows;
      M.dense = (uint8_t *)c->d_seek_pack_dense.p;
      M.blk = d_blk;
      hipLaunchKernelGGL(seek_pack_mark_kernel, dim3(nb), dim3(64), 0, c->stream, M);
      d_src = M.dense;
    } else {
      hipLaunchKernelGGL(seek_pack_flags_kernel, dim3(nb), dim3(256), 0, c->stream, d_windows, nb, d_blk);
    }
    HIP_TRY(c, hipGetLastError());
    std::vector<SeekPackBlock> blk(nb);
    HIP_TRY(c, hipMemcpyAsync(blk.data(), d_blk, (size_t)nb * sizeof(SeekPackBlock), hipMemcpyDeviceToHost, c->stream));
    if (sparse) HIP_TRY(c, hipMemcpyAsync(&one, d_one, sizeof one, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint64_t kept = 0;
    std::vector<uint32_t> ne;  // the non-empty blocks, in order
    for (uint32_t b = 0; b < nb; ++b) {
      if (blk[b].status) return FLATE_HIP_E_CORRUPT;  // (not the index's stream: the walk failed or left its segment)
      kept += blk[b].kept;
      if (blk[b].nonzero) ne.push_back(b);
    }
    if (sparse && (one.bad || one.pay_off[0] != index[kSeekRawOffAt] || one.pay_end != index[kSeekRawEndAt] ||
                   one.want != index[kSeekWantAt] || one.isize != index[kSeekIsizeAt]))
      return FLATE_HIP_E_CORRUPT;
    const uint32_t m = (uint32_t)ne.size();
    std::vector<uint64_t> e_in(m + 1), e_out(m + 1, 0);
    for (uint32_t i = 0; i <= m; ++i) e_in[i] = (uint64_t)i * kSeekWindow;
    if (m && m < nb) {  // some block is empty: the others move together (the encoder's streams lie back to back)
      if ((rc = ensure(c, c->d_seek_pack_stage, (size_t)m * kSeekWindow + 16))) return rc;
      std::vector<uint64_t> src(m);
      for (uint32_t i = 0; i < m; ++i) src[i] = (uint64_t)ne[i] * kSeekWindow;
      HIP_TRY(c, hipMemcpyAsync(d_r_out_off, e_in.data(), ((size_t)m + 1) * 8, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(c, hipMemcpyAsync(d_r_src, src.data(), (size_t)m * 8, hipMemcpyHostToDevice, c->stream));
      if ((rc = ranges_gather(c, d_src, (uint8_t *)c->d_seek_pack_stage.p, d_r_out_off, d_r_src, m, (uint64_t)m * kSeekWindow)))
        return rc;
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the uploads' host arrays end with this scope)
      d_src = (const uint8_t *)c->d_seek_pack_stage.p;
    }
    uint64_t total = 0;
    if (m) {
      // straight into the caller's device buffer, or into a staged copy no larger than the bound
      uint8_t *d_out = packed;
      uint64_t cap = packed_cap;
      if (!dev) {
        const uint64_t bound = flate_hip_seek_windows_pack_bound(m);
        cap = packed_cap < bound ? packed_cap : bound;
        if ((rc = ensure(c, c->d_seek_pack_out, cap + 16))) return rc;
        d_out = (uint8_t *)c->d_seek_pack_out.p;
      }
      rc = flate_hip_deflate_fast_batch(c, d_src, e_in.data(), m, d_out, cap, e_out.data(), FLATE_HIP_DEVICE_PTRS);
      if (rc == FLATE_HIP_E_OUT_TOO_SMALL) *packed_bytes = e_out[m];  // (the scan knows every size before the pack)
      if (rc) return rc;
      total = e_out[m];
      if (!dev) {
        HIP_TRY(c, hipMemcpyAsync(packed, d_out, total, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
      }
    }
    for (uint32_t b = 0, i = 0; b < nb; ++b) {
      off[b] = e_out[i];
      if (i < m && ne[i] == b) ++i;
    }
    off[nb] = total;
    const uint64_t kept_all = sparse ? kept : (uint64_t)nb * kSeekWindow;
    seek_pack_head(pack_index, index, mode, total, kept_all);
    *packed_bytes = total, *kept_bytes = kept_all;
    return FLATE_HIP_OK;
  } catch (const std::exception &e) {
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

// All blocks in the raw layout: the non-empty ones by ONE launch of the batch decoders, the empty ones by zero fill.
int flate_hip_seek_windows_unpack(flate_hip_ctx *c, const uint64_t *pack_index, uint64_t pack_words, const uint8_t *packed,
                                  uint64_t packed_bytes, uint8_t *windows, uint64_t windows_cap, uint64_t *windows_bytes,
                                  uint32_t *bad_block, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = seek_unpack_args(pack_index, pack_words, packed, packed_bytes, windows, windows_cap, windows_bytes, flags);
  if (rc) return rc;
  c->hip_err.clear();
  const uint32_t nb = (uint32_t)pack_index[kSeekPackBlocksAt];
  const uint64_t need = (uint64_t)nb * kSeekWindow;
  *windows_bytes = need;
  if (bad_block) *bad_block = 0xffffffffu;
  if (windows_cap < need) return FLATE_HIP_E_OUT_TOO_SMALL;  // (the size query too)
  if (nb == 0) return FLATE_HIP_OK;
  try {
    HIP_TRY(c, hipSetDevice(c->device));
    const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
    const uint64_t *off = pack_index + kSeekPackHeadWords;
    const uint8_t *d_packed = packed;
    uint8_t *d_win = windows;
    if (!dev) {
      if ((rc = ensure(c, c->d_seek_pack_stage, packed_bytes + 16))) return rc;
      if ((rc = ensure(c, c->d_one_seek_win, need + 16))) return rc;
      if (packed_bytes) HIP_TRY(c, hipMemcpyAsync(c->d_seek_pack_stage.p, packed, packed_bytes, hipMemcpyHostToDevice, c->stream));
      d_packed = (const uint8_t *)c->d_seek_pack_stage.p;
      d_win = (uint8_t *)c->d_one_seek_win.p;
    }
    const PackedBlocks P = packed_blocks(off, nb);
    const uint32_t m = (uint32_t)P.b.size();
    // (a slot runs to the next non-empty block: what a bad stream writes behind its 32768 bytes is zero-filled below)
    std::vector<uint64_t> slot_off(m + 1);
    for (uint32_t i = 0; i < m; ++i) slot_off[i] = (uint64_t)P.b[i] * kSeekWindow;
    slot_off[m] = m ? slot_off[m - 1] + kSeekWindow : 0;
    std::vector<uint8_t> good;
    if ((rc = inflate_blocks(c, d_packed, P.in_off, d_win, slot_off, good))) return rc;
    for (uint32_t b = 0, i = 0; b < nb;) {  // the runs of empty blocks
      if (i < m && P.b[i] == b) {
        ++b, ++i;
        continue;
      }
      const uint32_t e = i < m ? P.b[i] : nb;
      HIP_TRY(c, hipMemsetAsync(d_win + (uint64_t)b * kSeekWindow, 0, (size_t)(e - b) * kSeekWindow, c->stream));
      b = e;
    }
    if (!dev) HIP_TRY(c, hipMemcpyAsync(windows, d_win, need, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < m; ++i)
      if (!good[i]) {
        if (bad_block) *bad_block = P.b[i];
        return FLATE_HIP_E_CORRUPT;
      }
    return FLATE_HIP_OK;
  } catch (const std::exception &e) {
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

// flate_hip_inflate_one_ranges with the selected points' blocks made between SELECT's read-back and the rounds: the
// non-empty ones by ONE launch of the batch decoders into a dense stage of 32 KiB per SELECTED point, the empty ones by
// zero fill; the rounds' load reads the stage through the point -> slot table.
int flate_hip_inflate_one_ranges_packed(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t wrap,
                                        const uint64_t *index, uint64_t index_words, const uint64_t *pack_index,
                                        uint64_t pack_words, const uint8_t *packed, uint64_t packed_bytes, const uint64_t *begin,
                                        const uint64_t *end, uint32_t n_ranges, uint8_t *out, uint64_t out_cap,
                                        uint64_t *out_off, int32_t *range_status, uint32_t *n_decoded, uint32_t *bad_unit,
                                        uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  const int rc0 = one_ranges_packed_args(in, in_len, wrap, index, index_words, pack_index, pack_words, packed, packed_bytes,
                                         begin, end, n_ranges, out, out_cap, out_off, flags);
  if (rc0) return rc0;
  const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
  const uint64_t *off = pack_index + kSeekPackHeadWords;
  auto win = [&](const uint32_t *sel, uint32_t ns, const uint64_t *h_point, uint32_t np, OneRangesWin &W) -> int {
    int rc;
    std::vector<uint32_t> ps, places;
    selected_points(sel, ns, h_point, np, ps, &places);
    const uint32_t m = (uint32_t)ps.size();
    if (m == 0) return FLATE_HIP_OK;  // (only point 0 is selected: no window is read)
    uint32_t *d_slot_of;
    uint64_t *d_r_out_off, *d_r_src;
    rc = carve(c, c->d_seek_pack, [&](Carve &k) {
      k.take(d_r_out_off, (size_t)m + 1);
      k.take(d_r_src, m);
      k.take(d_slot_of, np);
    });
    if (rc) return rc;
    if ((rc = ensure(c, c->d_seek_pack_sel, (size_t)m * kSeekWindow + 16))) return rc;
    uint8_t *stage = (uint8_t *)c->d_seek_pack_sel.p;
    // the selected blocks' streams, compacted: slot j of the stage is point ps[j]'s
    std::vector<uint32_t> slot_of(np, 0), s_slot;  // (s_slot: the slots of the non-empty ones)
    std::vector<uint64_t> s_in(1, 0), s_src;
    for (uint32_t j = 0; j < m; ++j) {
      const uint32_t b = ps[j] - 1u;
      slot_of[ps[j]] = j;
      if (off[b + 1] > off[b]) {
        s_slot.push_back(j);
        s_src.push_back(off[b]);
        s_in.push_back(s_in.back() + (off[b + 1] - off[b]));
      }
    }
    const uint32_t k = (uint32_t)s_slot.size();
    HIP_TRY(c, hipMemcpyAsync(d_slot_of, slot_of.data(), (size_t)np * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(stage, 0, (size_t)m * kSeekWindow, c->stream));  // (the empty blocks; a bad block's rest)
    std::vector<uint8_t> good;
    if (k) {
      if ((rc = ensure(c, c->d_seek_pack_stage, s_in[k] + 16))) return rc;
      uint8_t *d_streams = (uint8_t *)c->d_seek_pack_stage.p;
      if (dev) {
        HIP_TRY(c, hipMemcpyAsync(d_r_out_off, s_in.data(), ((size_t)k + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d_r_src, s_src.data(), (size_t)k * 8, hipMemcpyHostToDevice, c->stream));
        if ((rc = ranges_gather(c, packed, d_streams, d_r_out_off, d_r_src, k, s_in[k]))) return rc;
        HIP_TRY(c, hipGetLastError());
      } else {  // only the selected blocks' streams are uploaded
        for (uint32_t i = 0; i < k; ++i)
          HIP_TRY(c, hipMemcpyAsync(d_streams + s_in[i], packed + s_src[i], s_in[i + 1] - s_in[i], hipMemcpyHostToDevice, c->stream));
      }
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      // ONE launch: every non-empty block into its own slot.  The decoders' slots lie back to back, so with empty blocks
      // in between a slot runs on to the next non-empty one
      if (k == m) {
        std::vector<uint64_t> slot_off(k + 1);
        for (uint32_t i = 0; i <= k; ++i) slot_off[i] = (uint64_t)i * kSeekWindow;
        if ((rc = inflate_blocks(c, d_streams, s_in, stage, slot_off, good))) return rc;
      } else {
        std::vector<uint64_t> slot_off(k + 1);
        for (uint32_t i = 0; i < k; ++i) slot_off[i] = (uint64_t)s_slot[i] * kSeekWindow;
        slot_off[k] = slot_off[k - 1] + kSeekWindow;
        if ((rc = inflate_blocks(c, d_streams, s_in, stage, slot_off, good))) return rc;
        // what a bad stream wrote behind its 32768 bytes lies in the empty blocks' slots: zero them again
        for (uint32_t j = 0, i = 0; j < m; ++j) {
          if (i < k && s_slot[i] == j) {
            ++i;
            continue;
          }
          HIP_TRY(c, hipMemsetAsync(stage + (uint64_t)j * kSeekWindow, 0, kSeekWindow, c->stream));
        }
      }
      for (uint32_t i = 0; i < k; ++i)
        if (!good[i]) W.bad_place.push_back(places[s_slot[i]]);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (the uploads' host arrays end with this scope)
    W.d_windows = stage;
    W.d_slot_of = d_slot_of;
    return FLATE_HIP_OK;
  };
  return one_ranges_run(c, in, in_len, wrap, index, begin, end, n_ranges, out, out_cap, out_off, range_status, n_decoded,
                        bad_unit, flags, win);
}

}  // extern "C"

// ---- ONE stream read in PARTS (one_parts_rule.h, one_parts_kernels.hip) ----

// Between two calls the stream's state rests in the handle: on the device the 32 KiB window and the running checksum
// (OnePartState), on the host the rule's words (OnePartsState: the carried bit, the bytes produced and consumed, the
// sticky status).  The unit rule and "one_unit_max" are the ctx's at open, whatever it says later (UnitReader).
struct flate_hip_one_reader : UnitReader {
  uint32_t wrap = 0;
  OnePartsState s = one_parts_fresh();
};

namespace {

// a fresh stream: a window of zeros, the sum of nothing
int one_reader_fresh(flate_hip_one_reader *r) {
  flate_hip_ctx *c = r->ctx;
  OnePartState *st = (OnePartState *)r->state.p;
  const uint32_t empty = r->wrap == FLATE_HIP_WRAP_ZLIB ? 1u : 0u;
  HIP_TRY(c, hipMemsetAsync(st, 0, sizeof(OnePartState), c->stream));
  HIP_TRY(c, hipMemcpyAsync(&st->sums[0], &empty, 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  r->s = one_parts_fresh();
  return FLATE_HIP_OK;
}

// the call's result words, behind everything queued so far
int one_reader_result(flate_hip_ctx *c, const OnePartState *st, OneDecHead &R, uint32_t &trailer_bad) {
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&R, &st->res, sizeof R, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&trailer_bad, &st->trailer_bad, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FLATE_HIP_OK;
}

}  // namespace

extern "C" {

int flate_hip_one_reader_open(flate_hip_ctx *c, uint32_t wrap, uint32_t flags, flate_hip_one_reader **out) {
  // every check before any HIP call
  if (one_reader_open_args(c, wrap, flags, out)) return FLATE_HIP_E_INVALID;
  auto fresh = [wrap](flate_hip_one_reader *r) {
    r->wrap = wrap;
    return one_reader_fresh(r);
  };
  return unit_reader_open(c, flags, sizeof(OnePartState), fresh, out);
}

int flate_hip_one_reader_reset(flate_hip_one_reader *r) { return unit_reader_reset(r, one_reader_fresh); }

void flate_hip_one_reader_free(flate_hip_one_reader *r) { unit_reader_free(r); }

// One call: flate_hip_inflate_one on the part in[0, in_len), its chain rooted at the carried bit -- discovery (the
// index comes back with the result words: the host picks the units that fit, one_parts_plan), the rounds over those
// units with the handle's window as R[0] and the stream's history in the distance rule, the part's checksum joined to
// the running one, the verdict; then the window behind the last delivered unit goes back into the handle.
int flate_hip_one_reader_read(flate_hip_one_reader *r, const uint8_t *in, uint64_t in_len, int final_in, uint8_t *out,
                              uint64_t out_cap, uint64_t *in_used, uint64_t *out_len, int64_t *err_off,
                              uint32_t *n_units) {
  // every check before any HIP call
  if (one_reader_read_args(r, in, in_len, out, out_cap, in_used, out_len)) return FLATE_HIP_E_INVALID;
  *in_used = 0, *out_len = 0;
  if (n_units) *n_units = 0;
  OnePartsState &s = r->s;
  if (err_off) *err_off = s.status < 0 ? s.err_off : -1;
  if (s.status) return s.status;  // sticky: the stream's end, or its error
  flate_hip_ctx *c = r->ctx;
  c->hip_err.clear();
  auto fail = [&](int st, int64_t eo) {
    s.status = st, s.err_off = eo;
    if (err_off) *err_off = eo;
    return st;
  };
  const uint32_t wrap = r->wrap, tl = one_parts_trailer_len(wrap);
  const bool dev = (r->flags & FLATE_HIP_DEVICE_PTRS) != 0, fin = final_in != 0;
  try {
    int rc;
    HIP_TRY(c, hipSetDevice(c->device));
    OnePartState *st = (OnePartState *)r->state.p;
    const uint8_t *d_in = nullptr;
    OneDecHead R{};
    uint32_t trailer_bad = 0;
    OnePartParams Q{};
    Q.st = st;
    Q.produced_before = s.produced;
    Q.wrap = wrap;

    if (s.trailer_pending) {  // the final block lies behind; these bytes are the trailer's
      if (in_len < tl) return fin ? fail(FLATE_HIP_E_UNEXPECTED_EOF, -1) : FLATE_HIP_OK;
      if ((rc = stage_input(c, in, tl, r->flags, &d_in))) return rc;
      HIP_TRY(c, hipMemsetAsync(&st->res, 0, sizeof st->res, c->stream));
      Q.trailer = d_in;
      Q.member_len = s.consumed + tl;
      hipLaunchKernelGGL(one_part_verdict_kernel, dim3(1), dim3(64), 0, c->stream, Q);
      if ((rc = one_reader_result(c, st, R, trailer_bad))) return rc;
      *in_used = tl;
      s.consumed += tl;
      s.trailer_pending = 0;
      if (R.status) return fail(R.status, R.err_off);
      s.status = FLATE_HIP_STREAM_END;
      return FLATE_HIP_STREAM_END;
    }
    if (in_len == 0) {
      if (!fin) return FLATE_HIP_OK;
      // no bytes at all: a bad header, as in the whole call; else the stream ends in front of a block
      if (!s.header_done && wrap != FLATE_HIP_WRAP_RAW) return fail(FLATE_HIP_E_CORRUPT, 0);
      return fail(FLATE_HIP_E_UNEXPECTED_EOF, -1);
    }

    if ((rc = stage_input(c, in, in_len, r->flags, &d_in))) return rc;
    const OnePart part{r->unit_max, r->stored_units, s.b0, s.header_done ? 0u : 1u, fin ? 1u : 0u};
    OneHead H{};
    OneParams P{};
    std::vector<uint64_t> index;  // unit_bit, then out_off
    if ((rc = one_discover(c, d_in, in_len, wrap, ~0ull, H, P, index, &part))) return rc;
    if (H.h.n_cand == 0) {
      if (H.bad == kPartsHdrBad) return fail(FLATE_HIP_E_CORRUPT, 0);
      // the header is refused only because the part ends here, or no raw byte stands behind it: more is needed
      return fin ? fail(FLATE_HIP_E_UNEXPECTED_EOF, -1) : FLATE_HIP_OK;
    }
    const uint32_t n = H.h.n_members;
    if (index.size() < 2 * ((size_t)n + 1)) {
      c->hip_err = "one reader: the index does not hold the units";
      return FLATE_HIP_E_INTERNAL;
    }
    const uint64_t *unit_bit = index.data(), *ooff = index.data() + index.size() / 2;
    const OnePartsPlan plan =
        one_parts_plan(n, ooff, H.h.rc, H.fail_unit, H.fail_out, fin, out_cap, in_len, r->unit_max);
    if (plan.action == kPartsNothing) return FLATE_HIP_OK;
    if (plan.action == kPartsReturn) {
      if (plan.status == FLATE_HIP_E_OUT_TOO_SMALL) {  // (not sticky: the state is unchanged)
        *out_len = plan.need;
        return FLATE_HIP_E_OUT_TOO_SMALL;
      }
      return fail(plan.status, H.h.err_off >= 0 ? (int64_t)s.raw_base + H.h.err_off : -1);
    }

    const uint32_t n_dec = plan.n_del + plan.with_fail;
    const uint64_t total = plan.total;
    uint8_t *d_out;
    if ((rc = unit_out_buffer(c, out, dev, total, d_out))) return rc;
    // the history in front of the part, as far as the distance rule can see it (it saturates at the window)
    const uint64_t hist = s.produced < (uint64_t)kWinEntries ? s.produced : (uint64_t)kWinEntries;
    const uint32_t per_round = unit_per_round(c, n_dec);
    OneDecParams D{};
    UnitResults dec;
    uint64_t *t_off;
    rc = unit_rounds_carve(c, D, n_dec, per_round, [&](Carve &k) {
      unit_pieces_take(k, D, &dec, per_round);
      k.take(t_off, (size_t)n_dec + 1);
    });
    if (rc) return rc;
    if ((rc = unit_dec_params(c, D, d_in, P.one, P.C.member_off, P.C.out_off, P.stored_units, false))) return rc;
    D.unit_max = r->unit_max;
    D.hist_base = hist;
    unit_verdict_params(D, total, dec, P.head, wrap, in_len);
    if ((rc = unit_window_seed(c, D, st->window))) return rc;
    // the last piece runs to BFINAL or to its failure only where the part's verdict is delivered with it
    const bool open_last = plan.terminal && (H.h.rc == 0 || H.fail_unit);
    auto decode = [&](uint32_t u0, uint32_t count) {
      return unit_decode_chain(c, D, d_in + H.raw_off, H.raw_len, u0, count, u0 + count < n_dec || !open_last, d_out, dec);
    };
    bool used[FLATE_HIP_STAGE_COUNT] = {false, false, false, false};
    if (n_dec) {
      hipLaunchKernelGGL(one_part_hist_kernel, dim3((n_dec + 255u) / 256u), dim3(256), 0, c->stream, P.C.out_off, t_off, n_dec,
                         hist);
      if ((rc = unit_rounds(c, D, t_off, nullptr, 0, n_dec, n_dec, per_round, unit_no_hook, unit_no_hook, decode))) return rc;
      used[FLATE_HIP_STAGE_INFLATE] = true;
    }
    bool ctl = false;
    // From here on the call queues work that moves the handle's device words (the running sum, the window): a failure
    // of the runtime behind this point leaves them ahead of the host's state, so it ends the handle -- sticky, as the
    // stream's own errors are.  (In front of it nothing of the handle has been touched, and a call may be repeated.)
    auto dead = [&](int e) {
      if (ctl) ctl_finish(c);
      return fail(e, -1);
    };
    const bool summed = wrap != FLATE_HIP_WRAP_RAW && total != 0;
    if (summed) {
      const uint64_t whole[2] = {0, total};
      if ((rc = ctl_begin(c, checksum_ctl_up_bytes(whole, 1), 0))) return rc;
      ctl = true;
      if ((rc = checksum_device(c, d_out, whole, 1, frame_sum_kind(wrap), &st->sums[1], FLATE_HIP_STAGE_CHECKSUM)))
        return dead(rc);
      used[FLATE_HIP_STAGE_CHECKSUM] = true;
    }
    // what the handle holds behind this call if nothing fails, and whether the trailer is judged now
    const bool ended = plan.terminal && H.h.rc == 0;
    OnePartsState next = s;
    uint64_t used_in = 0;
    bool trailer_now = false;
    one_parts_advance(next, wrap, H.raw_off, unit_bit[plan.n_del], total, ended, in_len, &used_in, &trailer_now);
    Q.total = total;
    Q.term_rc = plan.terminal ? H.h.rc : 0;
    Q.term_err_off = H.h.err_off;
    if (trailer_now && tl) {
      Q.trailer = d_in + (used_in - tl);
      Q.member_len = next.consumed;
    }
    hipLaunchKernelGGL(one_part_carry_kernel, dim3(1), dim3(64), 0, c->stream, Q, D);
    if (summed && s.produced &&
        (rc = checksum_join_device(c, st->sums, st->slot_off, st->produced, 2, frame_sum_kind(wrap), &st->joined, &st->total)))
      return dead(rc);
    hipLaunchKernelGGL(one_part_verdict_kernel, dim3(1), dim3(64), 0, c->stream, Q);
    if ((rc = one_reader_result(c, st, R, trailer_bad))) return dead(rc);
    if (ctl) ctl_finish(c);
    ctl = false;
    if ((rc = unit_reader_deliver(c, D, st->window, n_dec, per_round, R.status == 0, out, d_out, dev, R.out_len, total, out_len)))
      return dead(rc);
    if (c->profiling && (rc = collect_timing(c, used))) return dead(rc);
    if (n_units) *n_units = plan.n_del;
    if (R.status)  // (a trailer's mismatch counts from the member's first byte, everything else from the raw stream's)
      return fail(R.status, trailer_bad || R.err_off < 0 ? R.err_off : (int64_t)s.raw_base + R.err_off);
    s = next;
    *in_used = used_in;
    if (ended && trailer_now) {
      s.status = FLATE_HIP_STREAM_END;
      return FLATE_HIP_STREAM_END;
    }
    return FLATE_HIP_OK;
  } catch (const std::exception &e) {
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

}  // extern "C"

// ---- a gzip file of any members: the units of all members as one chain (gzfile_kernels.hip, gzfile_rule.h) ----
namespace {

// A PART of a file read in parts (flate_hip_gzfile_reader_read): the handle's unit rule, where the last call stopped
// (inside a member at bit b0, or at a header), whether the file ends with the part, the history in front of it, and --
// with whole members -- the handle's S and the call's out_cap.
struct GzPartIn {
  uint64_t unit_max;
  uint32_t stored_units;
  uint32_t inside, b0, final_in;
  uint64_t hist;
  uint64_t serial_max, out_cap;
};
// the kernels' word for it; the whole file is the part that is final and starts at a BOUNDARY (flate_kernels.h)
GzFileMode gzfile_mode(const GzPartIn *part, const uint32_t *verdict) {
  if (!part) return GzFileMode{0u, 0u, 1u, 0ull, verdict};
  return GzFileMode{1u, part->inside, part->final_in, part->hist, verdict};
}
// What the discovery's last read-back fetches beside the result words H / G.  The whole file: member_out, the members'
// places in the output (n_b + 2 entries of which G.n_members + 1 count).  A part: the INDEX -- unit_bit, out_off and
// u_start (cap + 1 entries each) in one vector of 64-bit words, one array behind the other, and u_final (cap).
struct GzFileBack {
  std::vector<uint64_t> *mout = nullptr;
  std::vector<uint64_t> *index = nullptr;
  std::vector<uint32_t> *u_final = nullptr;
  std::vector<uint32_t> *u_whole = nullptr;  // (a part with whole members: the per-unit marks, cap + 1)
};
// "gzfile_serial_max": phase 1's words (gzfile_discover_serial) for the chain behind it
struct GzSerialIn {
  GzSerialParams &S;
  GzSerialHead &SH;
  uint64_t find_from;
  const uint32_t *verdict = nullptr;  // a part: the three verdicts of List B (gzfile_parts_serial_rule.h)
  bool parts_find = false;            // a part INSIDE a member: FIND's PARTS build, over the whole part
};

// The chain of a file's discovery, behind the counts na / nb of the two lists (unit_discovery.h): the size rule, the
// carve of c->d_gzfile, the fills and the B nodes' bits, the probe of every node, link, rounds, finish, out-scan, the
// member scan, the tail probe, the member words and ONE read-back of H / G with what `back` names.
//   part  link, finish and rel run in the part's form (GzFileMode), FIND in its PARTS build
//   ser   List B was filled and sized by phase 1, whose arrays hold hdr_off; FIND's fill runs over the suffix PA names
//         and one small kernel moves its bits to the file's origin; a whole B node is parked at the raw stream's end for
//         PROBE and gets its phase-1 record back behind it; the marks between finish and out-scan, the list of whole
//         members at the end, SH in the read-back
//   both  a part of a handle with flate_hip_gzfile_reader_set_serial_max: the link stops in front of an OPEN member;
//         FIND's build is the PARTS one only INSIDE a member (then over the whole part); no list of whole members -- the
//         call lays out its batch behind its plan -- but whether the chain ended in front of an OPEN member, and the
//         per-unit marks in the read-back
int gzfile_chain(flate_hip_ctx *c, GzFileParams &P, OneParams &PA, GzipParams &PB, uint32_t na, uint32_t nb,
                 const GzPartIn *part, const GzSerialIn *ser, OneHead &H, GzFileHead &G, const GzFileBack &back) {
  int rc;
  ChainParams &C = P.O.C;
  if ((rc = two_list_size(C, PA.C, ser ? nullptr : &PB.C, na, nb))) return rc;
  P.n_a = na;
  P.n_b = nb;
  const size_t n = C.cap;
  rc = unit_nodes_carve(
      c, c->d_gzfile, P, P.u_member, n,
      [&](Carve &k) {
        if (ser) return;
        k.take(PB.C.cand_off, (size_t)nb + 1);
        k.take(PB.cand_end, nb);
      },
      [&](Carve &k) {
        k.take(P.member_off, (size_t)nb + 2);
        k.take(P.member_unit, (size_t)nb + 2);
        k.take(P.member_out, (size_t)nb + 2);
      });
  if (rc) return rc;
  PA.C.cand_off = C.cand_off;
  if (ser) {
    GzSerialParams &S = ser->S;
    S.n_a = na;
    rc = carve(c, part ? c->d_gzfile_parts_serial_units : c->d_gzfile_serial_units, [&](Carve &k) {
      k.take(S.u_whole, n + 1);
      k.take(S.u_end, n + 1);
    });
    if (rc) return rc;
    if (ser->find_from < C.in_len) {
      one_find_launch(c, false, PA.C.n_tiles, PA, ser->parts_find);
      if (na)
        hipLaunchKernelGGL(gzfile_serial_base_kernel, dim3((na + 255u) / 256u), dim3(256), 0, c->stream, C.cand_off, na,
                           8u * ser->find_from);
    }
    if (nb) hipLaunchKernelGGL(gzfile_serial_bits_kernel, dim3((nb + 255) / 256), dim3(256), 0, c->stream, P, S);
  } else {
    P.hdr_off = PB.C.cand_off;
    one_find_launch(c, false, C.n_tiles, PA, part != nullptr);
    if (nb) {
      hipLaunchKernelGGL(gzip_fill_kernel, dim3(C.n_tiles), dim3(256), 0, c->stream, PB);
      hipLaunchKernelGGL(gzfile_bits_kernel, dim3((nb + 255) / 256), dim3(256), 0, c->stream, P);
    }
  }
  if (n) one_probe_launch(c, C.cap, P.O, 0u);
  if (ser && nb) hipLaunchKernelGGL(gzfile_serial_keep_kernel, dim3((nb + 255) / 256), dim3(256), 0, c->stream, P, ser->S);
  const GzFileMode M = gzfile_mode(part, ser ? ser->verdict : nullptr);
  auto link = [&](dim3 g) { hipLaunchKernelGGL(gzfile_link_kernel, g, dim3(256), 0, c->stream, P, M); };
  auto finish = [&](dim3 g) { hipLaunchKernelGGL(gzfile_finish_kernel, g, dim3(256), 0, c->stream, P, M); };
  auto marks = [&](uint32_t node_blocks) {
    if (ser) hipLaunchKernelGGL(gzfile_serial_marks_kernel, dim3(node_blocks), dim3(256), 0, c->stream, P, ser->S);
  };
  auto behind = [&](uint32_t node_blocks) {
    hipLaunchKernelGGL(gzfile_members_kernel, dim3(1), dim3(1024), 0, c->stream, P);
    one_probe_launch(c, 1, P.O, 1u);
    hipLaunchKernelGGL(gzfile_rel_kernel, dim3(node_blocks), dim3(256), 0, c->stream, P, M);
    if (ser && part) hipLaunchKernelGGL(gzfile_part_serial_stop_kernel, dim3(1), dim3(64), 0, c->stream, P, ser->S);
    else if (ser) hipLaunchKernelGGL(gzfile_serial_list_kernel, dim3(1), dim3(1024), 0, c->stream, P, ser->S, 1u, 0u, 0ull);
  };
  return unit_chain(c, P.O, link, finish, marks, behind, H, G, P.gh, [&]() -> int {
    if (ser) HIP_TRY(c, hipMemcpyAsync(&ser->SH, ser->S.head, sizeof ser->SH, hipMemcpyDeviceToHost, c->stream));
    if (back.mout) {
      back.mout->assign((size_t)nb + 2, 0);
      HIP_TRY(c, hipMemcpyAsync(back.mout->data(), P.member_out, ((size_t)nb + 2) * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (back.index) {  // 28 bytes per node
      back.index->assign(3 * (n + 1), 0);
      back.u_final->assign(n + 1, 0);
      uint64_t *x = back.index->data();
      HIP_TRY(c, hipMemcpyAsync(x, C.member_off, (n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(x + (n + 1), C.out_off, (n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(x + 2 * (n + 1), P.u_start, (n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
      if (n) HIP_TRY(c, hipMemcpyAsync(back.u_final->data(), P.u_final, n * 4, hipMemcpyDeviceToHost, c->stream));
      if (back.u_whole) {
        back.u_whole->assign(n + 1, 0);
        if (ser) HIP_TRY(c, hipMemcpyAsync(back.u_whole->data(), ser->S.u_whole, (n + 1) * 4, hipMemcpyDeviceToHost, c->stream));
      }
    }
    return FLATE_HIP_OK;
  });
}

// The words the two count passes leave and List B's parameters, for a discovery over all of d_in[0, in_len) (P.O.C
// holds it): c->d_gzfile_tiles, sized before the candidates are counted; `more` takes what "gzfile_serial_max" adds,
// a_tiles is List A's tile count at most.
template <class More>
int gzfile_tiles_carve(flate_hip_ctx *c, GzFileParams &P, OneParams &PA, GzipParams &PB, OneHead *&head_a, size_t a_tiles,
                       More more) {
  ChainParams &C = P.O.C;
  BgzfHead *head_b;
  const int rc = carve(c, c->d_gzfile_tiles, [&](Carve &k) {
    k.take(P.O.head, 1);
    k.take(P.gh, 1);
    k.take(P.O.one, 1);
    k.take(head_a, 1);
    k.take(head_b, 1);
    more(k);
    k.take(PA.C.tile_cnt, a_tiles + 1);
    k.take(PB.C.tile_cnt, (size_t)C.n_tiles + 1);
  });
  if (rc) return rc;
  C.head = &P.O.head->h;
  PB.C.in = C.in;
  PB.C.in_len = C.in_len;
  PB.C.n_tiles = C.n_tiles;
  PB.C.head = head_b;
  PB.member_max = ~0ull;  // a member's range is never clipped
  return FLATE_HIP_OK;
}

// The discovery over the file d_in[0, in_len) (DEVICE memory, in_len != 0) on the ctx's stream, or -- part != null --
// over one PART of it: the two count passes and their scans, ONE read-back of the two candidate counts, then
// gzfile_chain.  The index stays on the device (P).  Counted in no profiling stage.  A part's root may be a header that
// cannot be judged yet: *root_bad is the count pass's verdict (HA.bad), and anything but 0 ends the discovery there.
int gzfile_discover(flate_hip_ctx *c, const uint8_t *d_in, uint64_t in_len, const GzPartIn *part, OneHead &H, GzFileHead &G,
                    GzFileParams &P, uint32_t *root_bad, const GzFileBack &back) {
  int rc;
  P = GzFileParams{};
  OneParams PA{};
  GzipParams PB{};
  ChainParams &C = P.O.C;
  C.in = d_in;
  C.in_len = in_len;
  if ((rc = tiles_for(d_in, 0, in_len, &C.n_tiles))) return rc;
  OneHead *head_a;
  if ((rc = gzfile_tiles_carve(c, P, PA, PB, head_a, C.n_tiles, [](Carve &) {}))) return rc;
  P.O.unit_max = part ? part->unit_max : c->one_unit_max;
  P.O.stored_units = part ? part->stored_units : c->one_stored_units;
  find_params(PA, P.O, head_a);
  hipLaunchKernelGGL(gzfile_init_kernel, dim3(1), dim3(64), 0, c->stream, P.O.one, d_in, in_len, gzfile_mode(part, nullptr),
                     part ? part->b0 : 0u);
  find_count(c, PA, part != nullptr);
  hipLaunchKernelGGL(gzip_count_kernel, dim3(C.n_tiles), dim3(256), 0, c->stream, PB);
  hipLaunchKernelGGL(chain_scan_kernel, dim3(1), dim3(1024), 0, c->stream, PB.C);
  OneHead HA{};
  BgzfHead HB{};
  if ((rc = find_counts_back(c, head_a, HA, PB.C.head, &HB))) return rc;
  if (part && (*root_bad = HA.bad)) return FLATE_HIP_OK;
  if ((rc = gzfile_chain(c, P, PA, PB, HA.h.n_cand, HB.n_cand, part, nullptr, H, G, back))) return rc;
  return !part && G.n_members > P.n_b ? FLATE_HIP_E_INTERNAL : FLATE_HIP_OK;
}

// The same discovery with short members decoded WHOLE (S >= 1: the option "gzfile_serial_max", or -- part != null --
// flate_hip_gzfile_reader_set_serial_max; gzfile_serial_rule.h, gzfile_parts_serial_rule.h and their kernel files).
// PHASE 1 over List B alone: count, scan, a read-back of the B count, fill, the serial ranges, ONE size-only launch of
// the batch decoders over all B candidates, the verdicts with the hop links, pointer doubling over those links, and
// a read-back of find_from.  PHASE 2, only when find_from < in_len: FIND over in[find_from, in_len) -- the pass runs on
// d_in + find_from with a FrameOne of its own, and one small kernel moves its bits to the file's origin -- and the
// read-back of its count.  PROBE runs over all nodes; a whole B node is parked at the raw stream's end for it and gets
// its phase-1 record back behind it.  Link, rounds, finish, the scans and the rel kernel are gzfile_discover's.  SH =
// find_from and the whole members among the good units; S = their batch, on the device.
// A PART differs in this: the root's verdict comes back with the B count (*root_bad: anything but 0 ends the discovery
// there); the ranges end with the PART and the three verdicts are kept for the chain's link; INSIDE a member find_from
// is 0 and FIND is its PARTS build over the whole part, whose candidate 0 is the chain's root; SH.pad = the chain
// ended in front of an OPEN member, and there is no list of whole members.
int gzfile_discover_serial(flate_hip_ctx *c, const uint8_t *d_in, uint64_t in_len, const GzPartIn *part, OneHead &H,
                           GzFileHead &G, GzFileParams &P, GzSerialParams &S, GzSerialHead &SH, uint32_t *root_bad,
                           const GzFileBack &back) {
  int rc;
  P = GzFileParams{};
  S = GzSerialParams{};
  SH = GzSerialHead{};
  OneParams PA{};
  GzipParams PB{};
  ChainParams &C = P.O.C;
  C.in = d_in;
  C.in_len = in_len;
  if ((rc = tiles_for(d_in, 0, in_len, &C.n_tiles))) return rc;
  const uint32_t n_tiles = C.n_tiles;
  OneHead *head_a;
  FrameOne *one_a;
  rc = gzfile_tiles_carve(c, P, PA, PB, head_a, (size_t)n_tiles + 1, [&](Carve &k) {  // (a suffix at another alignment:
    k.take(one_a, 1);                                                                  // at most one tile more)
    k.take(S.head, 1);
  });
  if (rc) return rc;
  BgzfHead *head_b = PB.C.head;
  P.O.unit_max = part ? part->unit_max : c->one_unit_max;
  P.O.stored_units = part ? part->stored_units : c->one_stored_units;
  hipLaunchKernelGGL(gzfile_init_kernel, dim3(1), dim3(64), 0, c->stream, P.O.one, d_in, in_len, gzfile_mode(part, nullptr),
                     part ? part->b0 : 0u);
  hipLaunchKernelGGL(gzip_count_kernel, dim3(n_tiles), dim3(256), 0, c->stream, PB);
  hipLaunchKernelGGL(chain_scan_kernel, dim3(1), dim3(1024), 0, c->stream, PB.C);
  HIP_TRY(c, hipGetLastError());
  BgzfHead HB{};
  FrameOne root{};
  HIP_TRY(c, hipMemcpyAsync(&HB, head_b, sizeof HB, hipMemcpyDeviceToHost, c->stream));
  if (part) HIP_TRY(c, hipMemcpyAsync(&root, P.O.one, sizeof root, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (part && (*root_bad = root.bad)) return FLATE_HIP_OK;
  const uint32_t nb = HB.n_cand;
  if (nb > 0x7ffffff0u) return FLATE_HIP_E_TOO_LARGE;  // (the count saturates at 2^32 - 1)
  if ((rc = chain_size(PB.C, nb))) return rc;

  // PHASE 1
  uint64_t *hdr_off;
  InfParams I{};  // size-only: no output buffer, no slots
  GzPartSerialIn A{1u, 0u, ~0ull, nullptr};  // the whole file: the part that is final and starts at a BOUNDARY
  if (part) A = GzPartSerialIn{part->final_in, part->inside, part->out_cap, nullptr};
  rc = carve(c, part ? c->d_gzfile_parts_serial : c->d_gzfile_serial, [&](Carve &k) {
    k.take(hdr_off, (size_t)nb + 1);
    k.take(PB.cand_end, nb);
    k.take(S.pay_off, (size_t)nb + 1);
    k.take(S.pay_end, nb);
    k.take(I.out_len, nb);
    k.take(I.status, nb);
    k.take(I.err_off, nb);
    k.take(I.used, nb);
    k.take(S.rec, nb);
    k.take(S.whole, nb);
    if (part) k.take(A.verdict, nb);
    k.take(S.jump[0], (size_t)nb + 2);
    k.take(S.jump[1], (size_t)nb + 2);
    k.take(S.w_in_off, (size_t)nb + 1);
    k.take(S.w_in_end, nb);
    k.take(S.w_out_off, (size_t)nb + 1);
    k.take(S.w_size, nb);
    k.take(S.w_unit, nb);
  });
  if (rc) return rc;
  PB.C.cand_off = hdr_off;
  P.hdr_off = hdr_off;
  P.n_b = nb;
  S.in = d_in;
  S.in_len = in_len;
  S.serial_max = part ? part->serial_max : c->gzfile_serial_max;
  S.n_b = nb;
  S.hdr_off = hdr_off;
  S.status = I.status;
  S.out_len = I.out_len;
  S.used = I.used;
  // (no candidate: no member at offset 0, nothing to search; INSIDE, the continued member is units)
  uint64_t find_from = part && part->inside ? 0ull : in_len;
  if (nb) {
    const uint32_t b_blocks = (nb + 255u) / 256u, w_blocks = (uint32_t)(((uint64_t)nb + 2 + 255) / 256);
    // every range is at most S < 2^28 bytes: the sub-block decoder at any batch size, or -- switched off -- the scalar
    // walk; both report `used`
    const uint64_t longest = in_len < S.serial_max ? in_len : S.serial_max;
    const InflateRoute route = inflate_route(c->inflate, c->num_cus, nb, longest, false, true);
    if (route.decoder == kDecodeSimt) {
      c->hip_err = part ? "gzfile reader: a size-only pass was routed to the lane-per-stream decoder"
                        : "gzfile discovery: a size-only pass was routed to the lane-per-stream decoder";
      return FLATE_HIP_E_INTERNAL;
    }
    I.in = d_in;
    I.in_off = S.pay_off;
    I.in_end = S.pay_end;
    I.n_streams = nb;
    I.in_len = in_len;
    I.size_only = 1u;
    hipLaunchKernelGGL(gzip_fill_kernel, dim3(n_tiles), dim3(256), 0, c->stream, PB);
    hipLaunchKernelGGL(gzfile_serial_ranges_kernel, dim3(b_blocks), dim3(256), 0, c->stream, S);
    HIP_TRY(c, hipGetLastError());
    if ((rc = launch_decoders(c, route, I, false))) return rc;
    hipLaunchKernelGGL(gzfile_serial_nodes_kernel, dim3(w_blocks), dim3(256), 0, c->stream, S, A);
    int cur = 0;
    for (uint64_t s = 1; s < (uint64_t)nb + 2; s <<= 1, cur ^= 1)
      hipLaunchKernelGGL(gzfile_serial_round_kernel, dim3(w_blocks), dim3(256), 0, c->stream, S.jump[cur], S.jump[cur ^ 1],
                         nb + 2u);
    hipLaunchKernelGGL(gzfile_serial_from_kernel, dim3(1), dim3(64), 0, c->stream, S, A, S.jump[cur]);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&SH, S.head, sizeof SH, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    find_from = SH.find_from;
    if (find_from > in_len || (part && part->inside && find_from)) return FLATE_HIP_E_INTERNAL;
  } else {
    SH.find_from = find_from;
    HIP_TRY(c, hipMemcpyAsync(S.head, &SH, sizeof SH, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (SH is the caller's: the copy has read it)
  }

  // PHASE 2: FIND over the bytes from find_from on (a member's header stands there), or over the part INSIDE a member
  uint32_t na = 0;
  const bool parts_find = part && part->inside;
  if (find_from < in_len) {
    find_params(PA, P.O, head_a);
    if (!parts_find) {
      PA.C.in = d_in + find_from;
      PA.C.in_len = in_len - find_from;
      PA.one = one_a;
      if ((rc = tiles_for(PA.C.in, 0, PA.C.in_len, &PA.C.n_tiles))) return rc;
      if (PA.C.n_tiles > n_tiles + 1u) return FLATE_HIP_E_INTERNAL;
      hipLaunchKernelGGL(gzfile_init_kernel, dim3(1), dim3(64), 0, c->stream, one_a, PA.C.in, PA.C.in_len,
                         gzfile_mode(nullptr, nullptr), 0u);
    }
    find_count(c, PA, parts_find);
    OneHead HA{};
    if ((rc = find_counts_back(c, head_a, HA))) return rc;
    na = HA.h.n_cand;
  }
  GzSerialIn ser{S, SH, find_from};
  ser.verdict = A.verdict;
  ser.parts_find = parts_find;
  if ((rc = gzfile_chain(c, P, PA, PB, na, nb, part, &ser, H, G, back))) return rc;
  if (SH.find_from != find_from) return FLATE_HIP_E_INTERNAL;
  if (part ? SH.pad > 1u : G.n_members > nb || SH.n_whole > nb || SH.n_whole > G.n_members) return FLATE_HIP_E_INTERNAL;
  return FLATE_HIP_OK;
}

// the discovery of flate_hip_gzfile_index / _read by the ctx's option, and what flate_hip_gzfile_last_route reports
int gzfile_discover_routed(flate_hip_ctx *c, const uint8_t *d_in, uint64_t in_len, OneHead &H, GzFileHead &G,
                           GzFileParams &P, GzSerialParams &S, GzSerialHead &SH, std::vector<uint64_t> *mout) {
  c->gzfile_route[0] = c->gzfile_route[1] = 0;
  c->gzfile_route_from = 0;
  int rc;
  GzFileBack back;
  back.mout = mout;
  if (!c->gzfile_serial_max) {
    S = GzSerialParams{};
    SH = GzSerialHead{};
    if ((rc = gzfile_discover(c, d_in, in_len, nullptr, H, G, P, nullptr, back))) return rc;
  } else if ((rc = gzfile_discover_serial(c, d_in, in_len, nullptr, H, G, P, S, SH, nullptr, back))) {
    return rc;
  }
  c->gzfile_route[0] = SH.n_whole;
  c->gzfile_route[1] = G.n_members - SH.n_whole;
  c->gzfile_route_from = SH.find_from;
  return FLATE_HIP_OK;
}

}  // namespace

extern "C" {

int flate_hip_gzfile_index(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint64_t index_cap, uint64_t *unit_bit,
                           uint64_t *out_off, uint64_t member_cap, uint64_t *member_off, uint64_t *member_unit,
                           uint32_t *n_units, uint32_t *n_members, uint64_t *out_bytes, uint32_t *n_candidates,
                           int32_t *status, uint32_t *bad_member, int64_t *err_off, int64_t *stream_err_off,
                           uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = gzfile_index_args(in, in_len, unit_bit, out_off, member_off, member_unit, n_units, n_members, out_bytes, status,
                             flags);
  if (rc) return rc;
  c->hip_err.clear();
  *n_units = 0, *n_members = 0, *out_bytes = 0, *status = 0;
  if (n_candidates) *n_candidates = 0;
  if (bad_member) *bad_member = 0xffffffffu;
  if (err_off) *err_off = -1;
  if (stream_err_off) *stream_err_off = -1;
  try {
    OneHead H{};
    GzFileHead G{};
    GzFileParams P{};
    GzSerialParams SP{};
    GzSerialHead SH{};
    G.err_off = G.stream_err_off = -1;
    c->gzfile_route[0] = c->gzfile_route[1] = 0;
    c->gzfile_route_from = 0;
    if (in_len) {  // (no bytes: zero members, zero units)
      const uint8_t *d_in = nullptr;
      if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
      if ((rc = gzfile_discover_routed(c, d_in, in_len, H, G, P, SP, SH, nullptr))) return rc;
    }
    *n_units = H.h.n_members;
    *n_members = G.n_members;
    if (n_candidates) *n_candidates = H.h.n_cand;
    *status = H.h.rc;
    *out_bytes = H.h.out_bytes;  // (0 on a broken chain)
    if (H.h.rc) {
      if (bad_member) *bad_member = G.n_members;
      if (err_off) *err_off = G.err_off;
      if (stream_err_off) *stream_err_off = G.stream_err_off;
    }
    // the index -- of a broken chain its good prefix, where that fits: the verdict is the walk's either way
    const uint64_t ue = (uint64_t)H.h.n_members + 1, me = (uint64_t)G.n_members + 1;
    const bool u_fits = unit_bit && index_cap >= ue, m_fits = member_off && member_cap >= me;
    if (in_len) {
      if (u_fits) {
        HIP_TRY(c, hipMemcpyAsync(unit_bit, P.O.C.member_off, ue * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(out_off, P.O.C.out_off, ue * 8, hipMemcpyDeviceToHost, c->stream));
      }
      if (m_fits) {
        HIP_TRY(c, hipMemcpyAsync(member_off, P.member_off, me * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(member_unit, P.member_unit, me * 8, hipMemcpyDeviceToHost, c->stream));
      }
      if (u_fits || m_fits) HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else {
      if (u_fits) unit_bit[0] = 0, out_off[0] = 0;
      if (m_fits) member_off[0] = 0, member_unit[0] = 0;
    }
    if (H.h.rc) return H.h.rc;
    return ((unit_bit && !u_fits) || (member_off && !m_fits)) ? FLATE_HIP_E_OUT_TOO_SMALL : FLATE_HIP_OK;
  } catch (const std::exception &e) {  // (out of host memory)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

// The whole call: discovery, then flate_hip_inflate_one's rounds over the units of all members -- TAIL with the
// member-relative offsets, the SEGMENTED compose / resolve with every member's first unit as a seed, DECODE straight
// into out + out_off[k] with a history that never crosses a member --, then one checksum launch planned over the
// members' output ranges, the trailers and the verdict.
int flate_hip_gzfile_read(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap,
                          uint64_t *out_len, uint32_t *n_members, uint32_t *n_units, uint32_t *n_candidates,
                          int32_t *status, uint32_t *bad_member, int64_t *err_off, int64_t *stream_err_off,
                          uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = gzfile_read_args(in, in_len, out, out_cap, out_len, status, flags);
  if (rc) return rc;
  c->hip_err.clear();
  *out_len = 0, *status = 0;
  if (n_members) *n_members = 0;
  if (n_units) *n_units = 0;
  if (n_candidates) *n_candidates = 0;
  if (bad_member) *bad_member = 0xffffffffu;
  if (err_off) *err_off = -1;
  if (stream_err_off) *stream_err_off = -1;
  c->gzfile_route[0] = c->gzfile_route[1] = 0;
  c->gzfile_route_from = 0;
  if (in_len == 0) return FLATE_HIP_OK;
  try {
    const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
    const uint8_t *d_in = nullptr;
    if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
    OneHead H{};
    GzFileHead G{};
    GzFileParams P{};
    GzSerialParams SP{};
    GzSerialHead SH{};
    std::vector<uint64_t> mout;
    if ((rc = gzfile_discover_routed(c, d_in, in_len, H, G, P, SP, SH, &mout))) return rc;
    if (n_members) *n_members = G.n_members;
    if (n_units) *n_units = H.h.n_members;
    if (n_candidates) *n_candidates = H.h.n_cand;
    // the units to decode: the good ones and, so that the bytes in front of an error are delivered, a unit that fails
    // behind its header; the total is known here
    const uint32_t n_dec = H.h.n_members + (H.fail_unit ? 1u : 0u);
    const uint64_t total = H.prefix_bytes + (H.fail_unit ? H.fail_out : 0ull);
    *out_len = total;
    if (total > out_cap) return FLATE_HIP_E_OUT_TOO_SMALL;  // (nothing is decoded; out == NULL: the size query)
    uint8_t *d_out;
    if ((rc = unit_out_buffer(c, out, dev, total, d_out))) return rc;
    const uint32_t n_mem = H.h.rc == 0 ? G.n_members : 0u;  // the members whose trailers are judged
    // the runs of units the rounds go over: all of them, or (option "gzfile_serial_max") what lies between the whole
    // members -- a run starts with a member's first unit, a seed, and ends where a member does
    const uint32_t n_whole = SH.n_whole;
    std::vector<std::pair<uint32_t, uint32_t>> runs;
    uint32_t longest_run = n_dec;
    if (n_whole) {
      std::vector<uint32_t> whole(n_dec);
      HIP_TRY(c, hipMemcpyAsync(whole.data(), SP.u_whole, (size_t)n_dec * 4, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      longest_run = 0;
      for (uint32_t a = 0; a < n_dec;) {
        uint32_t b = a;
        while (b < n_dec && !whole[b]) ++b;
        if (b > a) runs.emplace_back(a, b);
        if (b - a > longest_run) longest_run = b - a;
        a = b + 1u;
      }
    } else if (n_dec) {
      runs.emplace_back(0u, n_dec);
    }
    const uint32_t per_round = unit_per_round(c, longest_run);
    GzFileDecParams GD{};
    OneDecParams &D = GD.D;
    uint32_t *d_sums;
    UnitResults dec;
    rc = unit_rounds_carve(c, D, n_dec, per_round, [&](Carve &k) { unit_pieces_take(k, D, &dec, per_round); });
    if (rc) return rc;
    rc = carve(c, c->d_gzfile_dec, [&](Carve &k) {
      k.take(GD.v, 1);
      k.take(GD.seed, per_round);
      k.take(GD.p_bit_off, per_round);
      k.take(GD.p_bit_end, per_round);
      k.take(d_sums, (size_t)n_mem + 1);
    });
    if (rc) return rc;
    if ((rc = unit_dec_params(c, D, d_in, P.O.one, P.O.C.member_off, P.O.C.out_off, P.O.stored_units, false))) return rc;
    unit_verdict_params(D, total, dec, P.O.head, FLATE_HIP_WRAP_GZIP, in_len);
    GD.P = P;
    GD.n_good = H.h.n_members;
    GD.n_members = n_mem;
    GD.sums = d_sums;
    HIP_TRY(c, hipMemsetAsync(GD.v, 0xff, sizeof(GzFileVerdict), c->stream));  // bad_trailer: none
    if ((rc = unit_zero_seed(c, D))) return rc;
    bool used[FLATE_HIP_STAGE_COUNT] = {false, false, false, false};
    if (n_whole && total) {
      // the WHOLE members: ONE batch of independent streams straight into their places, IN FRONT of the rounds.  A slot
      // ends at the next whole member's start (the last at the end of the good units' output), so it may span the units
      // between them: whatever the batch leaves there is overwritten by the units that own those bytes
      InfParams W{};
      rc = carve(c, c->d_gzfile_serial_dec, [&](Carve &k) {
        k.take(W.out_len, n_whole);
        k.take(W.status, n_whole);
        k.take(W.err_off, n_whole);
      });
      if (rc) return rc;
      W.in = d_in;
      W.in_off = SP.w_in_off;
      W.in_end = SP.w_in_end;
      W.n_streams = n_whole;
      W.in_len = in_len;
      W.out = d_out;
      W.out_off = SP.w_out_off;
      const uint64_t longest = in_len < SP.serial_max ? in_len : SP.serial_max;
      if ((rc = launch_decoders(c, inflate_route(c->inflate, c->num_cus, n_whole, longest, false, false), W, false))) return rc;
      hipLaunchKernelGGL(gzfile_serial_check_kernel, dim3((n_whole + 255u) / 256u), dim3(256), 0, c->stream, SP, n_whole,
                         W.status, W.out_len, D.dh);
      used[FLATE_HIP_STAGE_INFLATE] = true;
      HIP_TRY(c, hipGetLastError());
    }
    // the pieces and the seeds of the round (every member's first unit is one)
    auto pieces = [&](uint32_t, uint32_t count) {
      hipLaunchKernelGGL(gzfile_pieces_kernel, dim3((count + 1u + 255u) / 256u), dim3(256), 0, c->stream, GD, 0ull);
      return FLATE_HIP_OK;
    };
    // DECODE: the round's units as pieces with dictionaries and their own ends, through the lane-per-stream decoder
    auto decode = [&](uint32_t, uint32_t count) {
      return unit_decode_members(c, D, d_in, H.raw_len, GD.p_bit_off, GD.p_bit_end, count, d_out, dec);
    };
    // TAIL with the member-relative offsets: a unit's history is what its own member has produced in front of it
    for (const auto &run : runs) {
      rc = unit_rounds(c, D, P.rel_off, GD.seed, run.first, run.second, n_dec, per_round, unit_no_hook, pieces, decode);
      if (rc) return rc;
      used[FLATE_HIP_STAGE_INFLATE] = true;
    }
    bool ctl = false;
    if (n_mem) {  // VERIFY: one launch planned over the members' output ranges, then a thread per trailer
      if (mout.size() < (size_t)n_mem + 1) return FLATE_HIP_E_INTERNAL;
      if ((rc = ctl_begin(c, checksum_ctl_up_bytes(mout.data(), n_mem), 0))) return rc;
      ctl = true;
      if ((rc = checksum_device(c, d_out, mout.data(), n_mem, FLATE_HIP_CHECKSUM_CRC32, d_sums, FLATE_HIP_STAGE_CHECKSUM)))
        return rc;
      used[FLATE_HIP_STAGE_CHECKSUM] = true;
      hipLaunchKernelGGL(gzfile_trailer_kernel, dim3((n_mem + 255) / 256), dim3(256), 0, c->stream, GD);
    }
    hipLaunchKernelGGL(gzfile_verdict_kernel, dim3(1), dim3(64), 0, c->stream, GD);
    HIP_TRY(c, hipGetLastError());
    GzFileVerdict V{};
    HIP_TRY(c, hipMemcpyAsync(&V, GD.v, sizeof V, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (ctl) ctl_finish(c);
    if ((rc = unit_deliver(c, out, d_out, dev, V.out_len, total, out_len))) return rc;
    if (c->profiling && (rc = collect_timing(c, used))) return rc;
    if (n_members) *n_members = V.n_members;
    if (n_units) *n_units = V.n_units;
    *status = V.status;
    if (V.status) {
      if (bad_member) *bad_member = V.bad_member;
      if (err_off) *err_off = V.err_off;
      if (stream_err_off) *stream_err_off = V.stream_err_off;
    }
    return V.status;
  } catch (const std::exception &e) {
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

// The seek index of a file of any members: the file's discovery, POINTS with every member's first unit as a point,
// then flate_hip_gzfile_read's rounds of TAIL / segmented COMPOSE / RESOLVE and, in DECODE's place, PACK: the windows
// in front of the round's window-bearing points into their blocks.  Nothing is decoded to output, no trailer is judged.
int flate_hip_gzfile_seek_index(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint64_t span, uint64_t *index,
                                uint64_t index_cap_words, uint64_t *index_words, uint8_t *windows, uint64_t windows_cap,
                                uint64_t *windows_bytes, uint32_t *n_units, uint32_t *n_members, uint32_t *n_points,
                                uint64_t *out_bytes, uint32_t *n_candidates, int32_t *status, uint32_t *bad_member,
                                int64_t *err_off, int64_t *stream_err_off, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = gzfile_seek_index_args(in, in_len, index, index_cap_words, index_words, windows, windows_cap, windows_bytes,
                                  n_units, n_members, n_points, out_bytes, status, flags);
  if (rc) return rc;
  c->hip_err.clear();
  *index_words = 0, *windows_bytes = 0, *n_units = 0, *n_members = 0, *n_points = 0, *out_bytes = 0, *status = 0;
  if (n_candidates) *n_candidates = 0;
  if (bad_member) *bad_member = 0xffffffffu;
  if (err_off) *err_off = -1;
  if (stream_err_off) *stream_err_off = -1;
  auto fail = [&](int st, uint32_t bm, int64_t eo, int64_t seo) {  // a file that fails gets no index
    *status = st;
    *index_words = 0, *windows_bytes = 0, *n_points = 0, *out_bytes = 0;
    if (bad_member) *bad_member = bm;
    if (err_off) *err_off = eo;
    if (stream_err_off) *stream_err_off = seo;
    return st;
  };
  span = seek_span(span);
  auto head = [&](uint64_t T, uint64_t n, uint64_t m, uint64_t np) {
    for (uint32_t k = 0; k < kGzSeekHeadWords; ++k) index[k] = 0;
    index[kGzSeekMagicAt] = kGzSeekMagic;
    index[kGzSeekVersionAt] = kGzSeekVersion;
    index[kGzSeekInLenAt] = in_len;
    index[kGzSeekTotalAt] = T;
    index[kGzSeekSpanAt] = span;
    index[kGzSeekUnitsAt] = n;
    index[kGzSeekMembersAt] = m;
    index[kGzSeekPointsAt] = np;
    index[kGzSeekRuleAt] = c->one_stored_units ? kSeekRuleStored : kSeekRuleDynamic;  // a read walks by this rule
  };
  if (in_len == 0) {  // no bytes: zero members, zero units, the head alone
    *index_words = gzfile_seek_index_words(0, 0, 0);
    if (index_cap_words < *index_words) return FLATE_HIP_E_OUT_TOO_SMALL;
    head(0, 0, 0, 0);
    return FLATE_HIP_OK;
  }
  try {
    const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
    const uint8_t *d_in = nullptr;
    if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
    OneHead H{};
    GzFileHead G{};
    GzFileParams P{};
    if ((rc = gzfile_discover(c, d_in, in_len, nullptr, H, G, P, nullptr, GzFileBack{}))) return rc;
    const uint32_t n = H.h.n_members, m = G.n_members;
    *n_units = n;
    *n_members = m;
    if (n_candidates) *n_candidates = H.h.n_cand;
    auto found = [&]() { return fail(H.h.rc, G.n_members, G.err_off, G.stream_err_off); };  // the discovery's verdict
    if (H.h.rc == FLATE_HIP_E_TOO_LARGE || H.h.rc == FLATE_HIP_E_INTERNAL) return found();
    const bool sound = H.h.rc == 0;  // (a file that fails is still walked: an earlier unit's distance may fail first)
    const uint32_t n_dec = n + (H.fail_unit ? 1u : 0u);
    if (n_dec == 0) return found();
    if (sound && (n < 1u || m < 1u || m > n)) return FLATE_HIP_E_INTERNAL;
    const uint32_t per_round = unit_per_round(c, n_dec);

    // POINTS: mark, scan, compact; the sizes are known here, in front of TAIL
    GzSeekPointsParams PP{};
    GzSeekPackParams K{};
    rc = carve(c, c->d_one_seek, [&](Carve &k) {
      k.take(PP.counts, 2);
      k.take(PP.point_unit, (size_t)n + 1);
      k.take(K.r_out_off, (size_t)per_round + 1);
      k.take(K.r_src, per_round);
    });
    if (rc) return rc;
    std::vector<uint64_t> ubit, ooff, moff, munit, points;
    uint32_t np = 0;
    uint64_t need_words = 0, need_bytes = 0;
    if (sound) {
      PP.out_off = P.O.C.out_off;
      PP.u_start = P.u_start;
      PP.n = n;
      PP.span = span;
      hipLaunchKernelGGL(gzfile_seek_points_kernel, dim3(1), dim3(1024), 0, c->stream, PP);
      HIP_TRY(c, hipGetLastError());
      uint32_t counts[2] = {0, 0};
      ubit.assign((size_t)n + 1, 0), ooff.assign((size_t)n + 1, 0), points.assign(n, 0);
      moff.assign((size_t)m + 1, 0), munit.assign((size_t)m + 1, 0);
      HIP_TRY(c, hipMemcpyAsync(counts, PP.counts, 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(points.data(), PP.point_unit, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(ubit.data(), P.O.C.member_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(ooff.data(), P.O.C.out_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(moff.data(), P.member_off, ((size_t)m + 1) * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(munit.data(), P.member_unit, ((size_t)m + 1) * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      np = counts[0];
      if (np < m || np > n || counts[1] != np - m || munit[0] != 0u || munit[m] != n) {
        c->hip_err = "gzfile seek index: the point count does not fit the units and members";
        return FLATE_HIP_E_INTERNAL;
      }
      need_words = gzfile_seek_index_words(n, m, np);
      need_bytes = gzfile_seek_windows_bytes(np, m);
      *index_words = need_words, *windows_bytes = need_bytes, *n_points = np, *out_bytes = H.h.out_bytes;
      if (index_cap_words < need_words || windows_cap < need_bytes) return FLATE_HIP_E_OUT_TOO_SMALL;  // (the size query too)
    }
    uint8_t *d_windows = windows;
    if (sound && !dev && need_bytes) {
      if ((rc = ensure(c, c->d_one_seek_win, need_bytes + 16))) return rc;
      d_windows = (uint8_t *)c->d_one_seek_win.p;
    }

    GzFileDecParams GD{};
    OneDecParams &D = GD.D;
    rc = unit_rounds_carve(c, D, n_dec, per_round, [&](Carve &k) { unit_pieces_take(k, D, nullptr, per_round); });
    if (rc) return rc;
    rc = carve(c, c->d_gzfile_dec, [&](Carve &k) {
      k.take(GD.seed, per_round);
      k.take(GD.p_bit_off, per_round);
      k.take(GD.p_bit_end, per_round);
    });
    if (rc) return rc;
    if ((rc = unit_dec_params(c, D, d_in, P.O.one, P.O.C.member_off, P.O.C.out_off, P.O.stored_units, false))) return rc;
    D.total = H.prefix_bytes + (H.fail_unit ? H.fail_out : 0ull);
    GD.P = P;
    GD.n_good = n;
    K.point_unit = PP.point_unit;
    K.member_unit = P.member_unit;
    K.m = m;
    K.n_points = np;
    uint32_t p_next = 0;  // the first point whose round has not come yet
    // a member's first unit is a seed that RESOLVE never writes: zeros in front of every member, so that a stored
    // window holds nothing of the member in front (slot 0 is the carried window unless the round starts a member)
    auto zeros = [&](uint32_t u0, uint32_t count) {
      if (!sound) return FLATE_HIP_OK;
      const bool starts = munit[bgzf_upper_bound(munit.data(), m, u0) - 1u] == u0;
      uint8_t *from = D.R + (starts ? 0 : kWinEntries);
      HIP_TRY(c, hipMemsetAsync(from, 0, ((size_t)count + (starts ? 1 : 0)) * kWinEntries, c->stream));
      return FLATE_HIP_OK;
    };
    auto seeds = [&](uint32_t, uint32_t count) {
      hipLaunchKernelGGL(gzfile_pieces_kernel, dim3((count + 1u + 255u) / 256u), dim3(256), 0, c->stream, GD, 0ull);
      return FLATE_HIP_OK;
    };
    // PACK: R[i] of the round's window-bearing points -> their blocks, which lie one behind the other in `windows`
    auto pack = [&](uint32_t u0, uint32_t count) {
      uint32_t p_hi = p_next;
      while (p_hi < np && points[p_hi] < (uint64_t)u0 + count) ++p_hi;
      if (p_hi == p_next) return FLATE_HIP_OK;
      const uint32_t cnt = p_hi - p_next;
      const uint32_t b_lo = gzfile_seek_blocks_before(munit.data(), m, p_next, (uint32_t)points[p_next]);
      const uint32_t b_hi = p_hi < np ? gzfile_seek_blocks_before(munit.data(), m, p_hi, (uint32_t)points[p_hi]) : np - m;
      K.p_lo = p_next, K.np = cnt, K.u0 = u0;
      p_next = p_hi;
      if (b_hi <= b_lo) return FLATE_HIP_OK;
      hipLaunchKernelGGL(gzfile_seek_pack_kernel, dim3((cnt + 1u + 255u) / 256u), dim3(256), 0, c->stream, K);
      return ranges_gather(c, D.R, d_windows + (uint64_t)b_lo * kSeekWindow, K.r_out_off, K.r_src, cnt,
                           (uint64_t)(b_hi - b_lo) * kSeekWindow);
    };
    // TAIL with the member-relative offsets: a unit's history is what its own member has produced in front of it
    if ((rc = unit_rounds(c, D, P.rel_off, GD.seed, 0, n_dec, n_dec, per_round, zeros, seeds, pack))) return rc;
    OneDecHead bad{};
    uint32_t bm = 0;
    if ((rc = unit_first_bad(c, D, n_dec, bad, P.u_member, &bm))) return rc;
    if (bad.first_bad != 0xffffffffu) {  // TAIL's verdict: the serial decoder's, at the serial offset, in its member
      const uint32_t fb = bad.first_bad;
      if (bm >= P.n_b) return FLATE_HIP_E_INTERNAL;
      uint64_t at = 0, first = 0, bit = 0;
      HIP_TRY(c, hipMemcpyAsync(&at, P.member_off + bm, 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(&first, P.member_unit + bm, 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      if (first > fb) return FLATE_HIP_E_INTERNAL;
      HIP_TRY(c, hipMemcpyAsync(&bit, P.O.C.member_off + first, 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      *n_members = bm;
      *n_units = fb;
      const int64_t seo = (bad.status == FLATE_HIP_E_CORRUPT && bad.err_off >= 0) ? bad.err_off - (int64_t)(bit >> 3) : -1;
      return fail(bad.status ? bad.status : FLATE_HIP_E_INTERNAL, bm, (int64_t)at, seo);
    }
    if (!sound) return found();
    if (p_next != np) return FLATE_HIP_E_INTERNAL;
    if (!dev && need_bytes) {
      HIP_TRY(c, hipMemcpyAsync(windows, d_windows, need_bytes, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    head(H.h.out_bytes, n, m, np);
    uint64_t *w = index + kGzSeekHeadWords;
    memcpy(w, ubit.data(), ((size_t)n + 1) * 8), w += (size_t)n + 1;
    memcpy(w, ooff.data(), ((size_t)n + 1) * 8), w += (size_t)n + 1;
    memcpy(w, moff.data(), ((size_t)m + 1) * 8), w += (size_t)m + 1;
    memcpy(w, munit.data(), ((size_t)m + 1) * 8), w += (size_t)m + 1;
    memcpy(w, points.data(), (size_t)np * 8);
    return FLATE_HIP_OK;
  } catch (const std::exception &e) {
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

// Random access through the file's seek index: the "same file" check per member, rel, locate, select, layout, ONE
// read-back (the check's word, the ranges' layout, the unit list), rounds of TAIL / segmented scan / DECODE over the
// list into a dense scratch, the per-unit check, the gather.
int flate_hip_gzfile_ranges(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, const uint64_t *index, uint64_t index_words,
                            const uint8_t *windows, uint64_t windows_bytes, const uint64_t *begin, const uint64_t *end,
                            uint32_t n_ranges, uint8_t *out, uint64_t out_cap, uint64_t *out_off, int32_t *range_status,
                            uint32_t *n_decoded, uint32_t *bad_unit, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = gzfile_ranges_args(in, in_len, index, index_words, windows, windows_bytes, begin, end, n_ranges, out, out_cap,
                              out_off, flags);
  if (rc) return rc;
  c->hip_err.clear();
  if (n_decoded) *n_decoded = 0;
  if (bad_unit) *bad_unit = 0xffffffffu;
  if (n_ranges == 0) {
    if (out_off) out_off[0] = 0;
    return FLATE_HIP_OK;
  }
  const uint32_t nr = n_ranges;
  if (index[kGzSeekUnitsAt] == 0) {  // the empty file: every range is empty
    for (uint32_t r = 0; r <= nr; ++r) out_off[r] = 0;
    if (range_status)
      for (uint32_t r = 0; r < nr; ++r) range_status[r] = 0;
    return FLATE_HIP_OK;
  }
  try {
    const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
    const uint8_t *d_in = nullptr;
    if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
    const uint32_t n = (uint32_t)index[kGzSeekUnitsAt], m = (uint32_t)index[kGzSeekMembersAt],
                   np = (uint32_t)index[kGzSeekPointsAt];
    const size_t idx_words = (size_t)(index_words - kGzSeekHeadWords);
    const uint64_t *h_munit = index + kGzSeekHeadWords + 2 * ((size_t)n + 1) + ((size_t)m + 1);
    const uint64_t *h_point = h_munit + ((size_t)m + 1);

    GzSeekParams GS{};
    OneSeekParams &Q = GS.Q;
    Q.n = n, Q.n_points = np, Q.span = index[kGzSeekSpanAt], Q.n_ranges = nr;
    uint64_t *d_idx, *d_begin, *d_end;
    FrameOne *d_one;
    size_t o_back = 0, o_end = 0;
    rc = carve(c, c->d_one_seek, [&](Carve &k) {
      k.take(d_idx, idx_words);
      k.take(d_begin, nr);
      k.take(d_end, nr);
      k.take(GS.rel, (size_t)n + 1);
      k.take(d_one, 1);
      k.take(Q.diff, (size_t)n + 1);
      k.take(Q.rank, n);
      k.take(Q.scratch_at, n);
      k.take(Q.r_b, nr);
      k.take(Q.r_len, nr);
      k.take(Q.r_first, nr);
      k.take(Q.r_last, nr);
      k.take(Q.r_seg, nr);
      k.take(Q.r_src, nr);
      k.take(Q.sel_at, (size_t)n + 1);
      o_back = k.at;
      k.take(Q.head, 1);
      k.take(GS.bad_member, 1);
      k.take(Q.r_out_off, (size_t)nr + 1);
      k.take(Q.r_rank_lo, nr);
      k.take(Q.r_rank_hi, nr);
      k.take(Q.sel_unit, n);
      o_end = k.at;
    });
    if (rc) return rc;
    Q.unit_bit = d_idx, Q.out_off = d_idx + ((size_t)n + 1);
    GS.member_off = Q.out_off + ((size_t)n + 1), GS.member_unit = GS.member_off + ((size_t)m + 1);
    Q.point_unit = GS.member_unit + ((size_t)m + 1);
    Q.begin = d_begin, Q.end = d_end;
    GS.in = d_in, GS.in_len = in_len, GS.m = m;
    const size_t back_bytes = o_end - o_back;
    const uint8_t *d_back = (const uint8_t *)c->d_one_seek.p + o_back;
    HIP_TRY(c, hipMemcpyAsync(d_idx, index + kGzSeekHeadWords, idx_words * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_begin, begin, (size_t)nr * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_end, end, (size_t)nr * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(Q.diff, 0, ((size_t)n + 1) * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(GS.bad_member, 0xff, 4, c->stream));  // none
    hipLaunchKernelGGL(gzfile_init_kernel, dim3(1), dim3(64), 0, c->stream, d_one, d_in, in_len, gzfile_mode(nullptr, nullptr), 0u);
    hipLaunchKernelGGL(gzfile_seek_members_kernel, dim3((m + 255u) / 256u), dim3(256), 0, c->stream, GS);
    hipLaunchKernelGGL(gzfile_seek_rel_kernel, dim3((n + 1u + 255u) / 256u), dim3(256), 0, c->stream, GS);
    hipLaunchKernelGGL(one_seek_locate_kernel, dim3((nr + 255u) / 256u), dim3(256), 0, c->stream, Q);
    hipLaunchKernelGGL(one_seek_select_kernel, dim3(1), dim3(1024), 0, c->stream, Q);
    hipLaunchKernelGGL(one_seek_layout_kernel, dim3(1), dim3(1024), 0, c->stream, Q);
    HIP_TRY(c, hipGetLastError());
    std::vector<uint8_t> back(back_bytes);
    HIP_TRY(c, hipMemcpyAsync(back.data(), d_back, back_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    auto got = [&](const auto *d) { return (decltype(d))(back.data() + ((const uint8_t *)d - d_back)); };  // d's host copy
    const OneSeekHead RH = *got(Q.head);
    const uint32_t missed = *got(GS.bad_member);
    const uint32_t *r_lo = got(Q.r_rank_lo), *r_hi = got(Q.r_rank_hi), *sel = got(Q.sel_unit);
    const uint32_t ns = RH.n_sel;
    if (missed != 0xffffffffu) {  // some member's header is not where the index has it: nothing is decoded
      for (uint32_t r = 0; r <= nr; ++r) out_off[r] = 0;
      if (range_status)
        for (uint32_t r = 0; r < nr; ++r) range_status[r] = FLATE_HIP_E_CORRUPT;
      return FLATE_HIP_E_CORRUPT;
    }
    if (ns > n) {
      c->hip_err = "gzfile ranges: more units selected than the file has";
      return FLATE_HIP_E_INTERNAL;
    }
    memcpy(out_off, got(Q.r_out_off), ((size_t)nr + 1) * 8);
    if (n_decoded) *n_decoded = ns;
    if (range_status)
      for (uint32_t r = 0; r < nr; ++r) range_status[r] = 0;
    if (RH.out_total > out_cap) return FLATE_HIP_E_OUT_TOO_SMALL;  // (the size query too: nothing is decoded)
    if (ns == 0 || RH.out_total == 0) return FLATE_HIP_OK;        // (no range holds a byte)

    // the windows: the caller's device buffer, or the blocks of the selected window-bearing points uploaded into a
    // staged copy
    const uint8_t *d_windows = windows;
    if (!dev && windows_bytes) {
      if ((rc = ensure(c, c->d_one_seek_win, windows_bytes + 16))) return rc;
      uint8_t *stage = (uint8_t *)c->d_one_seek_win.p;
      d_windows = stage;
      std::vector<uint32_t> bs;  // the blocks of the selected points, rising
      uint32_t p = 0, j = 0;     // j: the members whose first unit is at or in front of the point's
      for (uint32_t i = 0; i < ns && p < np; ++i) {
        while (p < np && h_point[p] < sel[i]) ++p;
        if (p >= np || h_point[p] != sel[i]) continue;
        while (j < m && h_munit[j] <= sel[i]) ++j;
        if (h_munit[j - 1u] != sel[i]) bs.push_back(p - j);
      }
      for (size_t a = 0; a < bs.size();) {  // neighbours in the index travel as one copy
        size_t b = a + 1;
        while (b < bs.size() && bs[b] == bs[b - 1] + 1u) ++b;
        const uint64_t at = (uint64_t)bs[a] * kSeekWindow, len = (uint64_t)(b - a) * kSeekWindow;
        HIP_TRY(c, hipMemcpyAsync(stage + at, windows + at, len, hipMemcpyHostToDevice, c->stream));
        a = b;
      }
    }

    const uint32_t per_round = unit_per_round(c, ns);
    OneDecParams D{};
    GzSeekRoundParams Z{};
    OneSeekRoundParams &S = Z.S;
    UnitResults dec;
    if ((rc = seek_rounds_carve(c, D, S, dec, ns, per_round))) return rc;
    // TAIL by the index's rule, not the context's option; a unit's history is what its own member has produced in front
    // of it (rel)
    const uint32_t stored = index[kGzSeekRuleAt] == kSeekRuleStored ? 1u : 0u;
    if ((rc = unit_dec_params(c, D, d_in, d_one, Q.unit_bit, GS.rel, stored, false))) return rc;
    D.unit_list = Q.sel_unit;
    S.Q = Q;
    S.windows = d_windows;
    Z.member_unit = GS.member_unit;
    Z.m = m;
    Z.rel = GS.rel;
    auto seeds = [&](uint32_t i0, uint32_t count) {
      S.i0 = i0, S.count = count;
      hipLaunchKernelGGL(gzfile_seek_seed_kernel, dim3((count + 255u) / 256u), dim3(256), 0, c->stream, Z);
      hipLaunchKernelGGL(gzfile_seek_load_kernel, dim3(seek_load_blocks(count)), dim3(256), 0, c->stream, Z);
      return FLATE_HIP_OK;
    };
    // (bits are counted from the file's first byte and nothing at or behind the last trailer is read)
    const SeekRangesOut O{out, nr, RH.out_total, RH.scratch_total, r_lo, r_hi, sel, range_status, bad_unit, dev};
    return seek_ranges_decode(c, D, S, dec, per_round, ns, d_in, in_len - kGzipTrailerLen, O, seeds);
  } catch (const std::exception &e) {
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

}  // extern "C"

// ---- a gzip file of any members read in PARTS (gzfile_parts_rule.h, gzfile_parts_kernels.hip) ----

// Between two calls the file's state rests in the handle: on the device the 32 KiB window and the running CRC-32 of
// the member in progress (GzPartState), on the host the rule's words (GzPartsState).  The unit rule and "one_unit_max"
// are the ctx's at open, whatever it says later (UnitReader); "gzfile_serial_max" is not read: the handle has a setting
// of its own (flate_hip_gzfile_reader_set_serial_max; gzfile_parts_serial_rule.h), which reset keeps as it keeps the
// unit rule, and the words of flate_hip_gzfile_reader_last_route.
struct flate_hip_gzfile_reader : UnitReader {
  GzPartsState s = gzfile_parts_fresh();
  uint64_t serial_max = 0;
  uint32_t route_members = 0, route_open = 0;
  uint64_t route_from = 0;
};

namespace {

// a fresh file: a window of zeros, the sum of nothing
int gzfile_reader_fresh(flate_hip_gzfile_reader *r) {
  flate_hip_ctx *c = r->ctx;
  HIP_TRY(c, hipMemsetAsync(r->state.p, 0, sizeof(GzPartState), c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  r->s = gzfile_parts_fresh();
  r->route_members = r->route_open = 0;
  r->route_from = 0;
  return FLATE_HIP_OK;
}

}  // namespace

extern "C" {

int flate_hip_gzfile_reader_open(flate_hip_ctx *c, uint32_t flags, flate_hip_gzfile_reader **out) {
  // every check before any HIP call
  if (gzfile_reader_open_args(c, flags, out)) return FLATE_HIP_E_INVALID;
  return unit_reader_open(c, flags, sizeof(GzPartState), gzfile_reader_fresh, out);
}

int flate_hip_gzfile_reader_reset(flate_hip_gzfile_reader *r) { return unit_reader_reset(r, gzfile_reader_fresh); }

void flate_hip_gzfile_reader_free(flate_hip_gzfile_reader *r) { unit_reader_free(r); }

int flate_hip_gzfile_reader_set_serial_max(flate_hip_gzfile_reader *r, uint64_t serial_max) {
  if (gzfile_reader_set_serial_max_args(r, serial_max, r && gzfile_parts_is_fresh(r->s))) return FLATE_HIP_E_INVALID;
  r->serial_max = serial_max;
  return FLATE_HIP_OK;
}

int flate_hip_gzfile_reader_last_route(const flate_hip_gzfile_reader *r, uint32_t *serial_members, uint32_t *open_stop,
                                       uint64_t *find_from) {
  if (gzfile_reader_last_route_args(r, serial_members, open_stop, find_from)) return FLATE_HIP_E_INVALID;
  *serial_members = r->route_members;
  *open_stop = r->route_open;
  *find_from = r->route_from;
  return FLATE_HIP_OK;
}

// One call: flate_hip_gzfile_read on the part in[0, in_len), its chain rooted where the last call stopped -- discovery
// (the index comes back with the result words: the host picks the units that fit and finds the members among them,
// gzfile_parts_call), the rounds over those units with the handle's window as R[0] of the continued member, one
// checksum launch over the members' ranges with the first joined to the running sum, the trailers of the members that
// end, the verdict; then the window behind the last delivered unit goes back into the handle.
int flate_hip_gzfile_reader_read(flate_hip_gzfile_reader *r, const uint8_t *in, uint64_t in_len, int final_in, uint8_t *out,
                                 uint64_t out_cap, uint64_t *in_used, uint64_t *out_len, uint32_t *n_members,
                                 uint32_t *n_units, uint32_t *bad_member, int64_t *err_off, int64_t *stream_err_off) {
  // every check before any HIP call
  if (gzfile_reader_read_args(r, in, in_len, out, out_cap, in_used, out_len)) return FLATE_HIP_E_INVALID;
  *in_used = 0, *out_len = 0;
  if (n_members) *n_members = 0;
  if (n_units) *n_units = 0;
  GzPartsState &s = r->s;
  auto words = [&]() {
    const bool bad = s.status < 0;
    if (bad_member) *bad_member = bad ? s.bad_member : 0xffffffffu;
    if (err_off) *err_off = bad ? s.err_off : -1;
    if (stream_err_off) *stream_err_off = bad ? s.stream_err_off : -1;
  };
  words();
  if (s.status) return s.status;  // sticky: the file's end, or its error
  flate_hip_ctx *c = r->ctx;
  c->hip_err.clear();
  // a failure that needs no decode: the member in progress, or the place where a header had to stand
  auto fail_here = [&](int st, bool no_header) {
    s.status = st;
    s.bad_member = s.members_done;
    s.err_off = (int64_t)(no_header ? s.consumed : s.member_off);
    s.stream_err_off = -1;
    words();
    return st;
  };
  const bool dev = (r->flags & FLATE_HIP_DEVICE_PTRS) != 0, fin = final_in != 0;
  try {
    int rc;
    if (in_len == 0) {
      if (!fin) return FLATE_HIP_OK;
      if (s.inside) return fail_here(FLATE_HIP_E_UNEXPECTED_EOF, false);
      s.status = FLATE_HIP_STREAM_END;  // the file ends at a member's end (an empty file: at its start)
      return FLATE_HIP_STREAM_END;
    }
    if (s.inside && in_len <= kGzipTrailerLen)  // no raw byte in front of the trailer's room: the next unit is cut
      return fin ? fail_here(FLATE_HIP_E_UNEXPECTED_EOF, false) : FLATE_HIP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    GzPartState *st = (GzPartState *)r->state.p;
    const uint8_t *d_in = nullptr;
    if ((rc = stage_input(c, in, in_len, r->flags, &d_in))) return rc;
    // the history in front of the part, as far as the distance rule can see it (it saturates at the window)
    const uint64_t hist = !s.inside ? 0ull : s.produced < (uint64_t)kWinEntries ? s.produced : (uint64_t)kWinEntries;
    const GzPartIn part{r->unit_max, r->stored_units, s.inside, s.b0, fin ? 1u : 0u, hist, r->serial_max, out_cap};
    OneHead H{};
    GzFileHead G{};
    GzFileParams P{};
    uint32_t root_bad = 0;
    std::vector<uint64_t> index;
    std::vector<uint32_t> u_final;
    GzFileBack back;
    back.index = &index, back.u_final = &u_final;
    // S >= 1: the members that lie whole inside the part are single units (gzfile_parts_serial_rule.h)
    const uint64_t S = r->serial_max;
    GzSerialParams SP{};
    GzSerialHead SH{};
    std::vector<uint32_t> u_whole;
    if (S) {
      back.u_whole = &u_whole;
      rc = gzfile_discover_serial(c, d_in, in_len, &part, H, G, P, SP, SH, &root_bad, back);
    } else {
      rc = gzfile_discover(c, d_in, in_len, &part, H, G, P, &root_bad, back);
    }
    if (rc) return rc;
    if (root_bad == kPartsHdrBad || (root_bad && fin)) return fail_here(FLATE_HIP_E_CORRUPT, true);
    if (root_bad) {  // the header is refused only because the part ends here: more is needed
      if (in_len >= r->unit_max) return fail_here(FLATE_HIP_E_TOO_LARGE, true);
      return FLATE_HIP_OK;
    }
    const size_t n1 = index.size() / 3;
    GzPartsIndex X{};
    X.n = H.h.n_members;
    if ((size_t)X.n + 1 > n1) {
      c->hip_err = "gzfile reader: the index does not hold the units";
      return FLATE_HIP_E_INTERNAL;
    }
    X.unit_bit = index.data(), X.out_off = index.data() + n1, X.u_start = index.data() + 2 * n1;
    X.u_final = u_final.data();
    X.rc = H.h.rc, X.err_off = H.h.err_off, X.fail_unit = H.fail_unit, X.fail_out = H.fail_out, X.no_header = G.no_header;
    if (S && u_whole.size() < (size_t)X.n + 1) return FLATE_HIP_E_INTERNAL;
    r->route_members = 0;
    r->route_open = S ? SH.pad : 0u;
    r->route_from = S ? SH.find_from : 0ull;
    const GzPartsCall call = gzfile_parts_serial_call(s, X, in_len, fin, out_cap, r->unit_max, S);
    const OnePartsPlan &plan = call.plan;
    auto fail = [&](const GzPartsFail &f) {
      gzfile_parts_fail(s, X, call, f);
      words();
      return f.status;
    };
    if (plan.action == kPartsNothing) return FLATE_HIP_OK;
    if (plan.action == kPartsReturn) {
      if (plan.status == FLATE_HIP_E_OUT_TOO_SMALL) {  // (not sticky: the state is unchanged)
        *out_len = plan.need;
        return FLATE_HIP_E_OUT_TOO_SMALL;
      }
      return fail(GzPartsFail{plan.status, 0xffffffffu, 0xffffffffu, -1});
    }

    const uint32_t n_dec = plan.n_del + plan.with_fail, n_segs = (uint32_t)call.segs.size();
    const uint64_t total = plan.total;
    uint8_t *d_out;
    if ((rc = unit_out_buffer(c, out, dev, total, d_out))) return rc;
    // the runs of units the rounds go over: all of them, or what lies between the whole members -- a run starts with the
    // continued member's unit or with a member's first unit, and ends where a member does
    const uint32_t n_whole = S ? gzfile_parts_serial_count(u_whole.data(), n_dec) : 0u;
    std::vector<std::pair<uint32_t, uint32_t>> runs;
    uint32_t longest_run = n_dec;
    if (n_whole) {
      longest_run = 0;
      for (uint32_t a = 0; a < n_dec;) {
        uint32_t b = a;
        while (b < n_dec && !u_whole[b]) ++b;
        if (b > a) runs.emplace_back(a, b);
        if (b - a > longest_run) longest_run = b - a;
        a = b + 1u;
      }
    } else if (n_dec) {
      runs.emplace_back(0u, n_dec);
    }
    // the units whose window the handle carries: the last run's, unless a whole member is the last unit (a BOUNDARY)
    const uint32_t carry_units = runs.empty() || runs.back().second != n_dec ? 0u : n_dec - runs.back().first;
    const uint32_t per_round = unit_per_round(c, longest_run);
    GzFileDecParams GD{};
    OneDecParams &D = GD.D;
    UnitResults dec;
    rc = unit_rounds_carve(c, D, n_dec, per_round, [&](Carve &k) { unit_pieces_take(k, D, &dec, per_round); });
    if (rc) return rc;
    GzPartParams Q{};
    GzPartSeg *d_segs;
    uint32_t *d_sums;
    uint64_t *d_join;  // checksum_join_device's slot_off (3) and out_len (2)
    rc = carve(c, c->d_gzfile_dec, [&](Carve &k) {
      k.take(GD.seed, per_round);
      k.take(GD.p_bit_off, per_round);
      k.take(GD.p_bit_end, per_round);
      k.take(d_join, 6);
      k.take(d_segs, (size_t)n_segs + 1);
      k.take(d_sums, (size_t)n_segs + 2);
    });
    if (rc) return rc;
    if ((rc = unit_dec_params(c, D, d_in, P.O.one, P.O.C.member_off, P.O.C.out_off, P.O.stored_units, false))) return rc;
    D.unit_max = r->unit_max;
    unit_verdict_params(D, total, dec, P.O.head, FLATE_HIP_WRAP_GZIP, in_len);
    GD.P = P;
    GD.n_good = plan.n_del;
    if ((rc = unit_window_seed(c, D, st->window))) return rc;
    auto pieces = [&](uint32_t, uint32_t count) {
      hipLaunchKernelGGL(gzfile_pieces_kernel, dim3((count + 1u + 255u) / 256u), dim3(256), 0, c->stream, GD, hist);
      return FLATE_HIP_OK;
    };
    auto decode = [&](uint32_t, uint32_t count) {
      return unit_decode_members(c, D, d_in, H.raw_len, GD.p_bit_off, GD.p_bit_end, count, d_out, dec);
    };
    bool used[FLATE_HIP_STAGE_COUNT] = {false, false, false, false};
    if (n_whole && total) {
      // the WHOLE members: ONE batch of independent streams straight into their places, IN FRONT of the rounds.  A slot
      // ends at the next whole member's start and the last at the planned total: whatever the batch leaves between them
      // is overwritten by the units that own those bytes, and nothing behind the planned total is written
      hipLaunchKernelGGL(gzfile_serial_list_kernel, dim3(1), dim3(1024), 0, c->stream, P, SP, 0u, n_dec, total);
      InfParams W{};
      rc = carve(c, c->d_gzfile_parts_serial_dec, [&](Carve &k) {
        k.take(W.out_len, n_whole);
        k.take(W.status, n_whole);
        k.take(W.err_off, n_whole);
      });
      if (rc) return rc;
      W.in = d_in;
      W.in_off = SP.w_in_off;
      W.in_end = SP.w_in_end;
      W.n_streams = n_whole;
      W.in_len = in_len;
      W.out = d_out;
      W.out_off = SP.w_out_off;
      const uint64_t longest = in_len < S ? in_len : S;
      if ((rc = launch_decoders(c, inflate_route(c->inflate, c->num_cus, n_whole, longest, false, false), W, false))) return rc;
      hipLaunchKernelGGL(gzfile_serial_check_kernel, dim3((n_whole + 255u) / 256u), dim3(256), 0, c->stream, SP, n_whole,
                         W.status, W.out_len, D.dh);
      used[FLATE_HIP_STAGE_INFLATE] = true;
      HIP_TRY(c, hipGetLastError());
    }
    for (const auto &run : runs) {
      rc = unit_rounds(c, D, P.rel_off, GD.seed, run.first, run.second, n_dec, per_round, unit_no_hook, pieces, decode);
      if (rc) return rc;
      used[FLATE_HIP_STAGE_INFLATE] = true;
    }
    // the members' sums: ONE launch planned over their ranges of the delivered bytes; the continued member's first
    // range is joined to the running sum
    const uint64_t size0 = n_segs ? call.segs[0].out_end - call.segs[0].out_begin : 0ull;
    Q.st = st;
    Q.in = d_in;
    Q.segs = d_segs;
    Q.sums = d_sums;
    Q.n_segs = n_segs;
    Q.n_end = call.n_end;
    Q.sum0_mode = !(call.continued && s.produced) ? 0u : size0 ? 2u : 1u;
    Q.keep_sum = n_segs && call.segs.back().trailer_at == ~0ull ? 1u : 0u;
    Q.n_del = plan.n_del;
    Q.term_rc = plan.terminal ? H.h.rc : 0;
    Q.term_err_off = H.h.err_off;
    Q.total = total;
    const uint64_t join[5] = {0, s.produced, s.produced + size0, s.produced, size0};
    size_t up = n_segs * sizeof(GzPartSeg) + sizeof join + 1024;
    if (n_segs && total) up += checksum_ctl_up_bytes(call.bounds.data(), n_segs);
    if ((rc = ctl_begin(c, up, 0))) return rc;
    if (n_segs && (rc = ctl_up(c, d_segs, call.segs.data(), n_segs * sizeof(GzPartSeg)))) return rc;
    if ((rc = ctl_up(c, d_join, join, sizeof join))) return rc;
    HIP_TRY(c, hipMemcpyAsync(d_sums, &st->sum, 4, hipMemcpyDeviceToDevice, c->stream));
    if (n_segs && total) {
      if ((rc = checksum_device(c, d_out, call.bounds.data(), n_segs, FLATE_HIP_CHECKSUM_CRC32, d_sums + 1,
                                FLATE_HIP_STAGE_CHECKSUM)))
        return rc;
      used[FLATE_HIP_STAGE_CHECKSUM] = true;
    }
    // From here on the call queues work that moves the handle's device words (the result words, the running sum, the
    // window): a failure of the runtime behind this point leaves them ahead of the host's state, so it ends the handle
    // -- sticky, as the file's own errors are.  (In front of it nothing of the handle has been touched, and a call may
    // be repeated.)
    auto dead = [&](int e) {
      s.status = e, s.bad_member = 0xffffffffu, s.err_off = -1, s.stream_err_off = -1;
      words();
      return e;
    };
    if (hipMemsetAsync(&st->res, 0xff, sizeof st->res, c->stream) != hipSuccess) return dead(FLATE_HIP_E_HIP);  // bad_trailer: none
    if (Q.sum0_mode == 2u &&
        (rc = checksum_join_device(c, d_sums, d_join, d_join + 3, 2, FLATE_HIP_CHECKSUM_CRC32, &st->joined, &st->total)))
      return dead(rc);
    if (call.n_end)
      hipLaunchKernelGGL(gzfile_part_trailer_kernel, dim3((call.n_end + 255u) / 256u), dim3(256), 0, c->stream, Q, D);
    hipLaunchKernelGGL(gzfile_part_carry_kernel, dim3(1), dim3(64), 0, c->stream, Q, D);
    GzFileVerdict V{};
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(&V, &st->res, sizeof V, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return dead(FLATE_HIP_E_HIP);
    ctl_finish(c);
    if ((rc = unit_reader_deliver(c, D, st->window, carry_units, per_round, V.status == 0, out, d_out, dev, V.out_len, total, out_len)))
      return dead(rc);
    if (c->profiling && (rc = collect_timing(c, used))) return dead(rc);
    if (n_members) *n_members = V.n_members;
    if (n_units) *n_units = V.n_units;
    if (S && V.n_units <= n_dec) r->route_members = gzfile_parts_serial_count(u_whole.data(), V.n_units);
    if (V.status) {
      if (V.status == FLATE_HIP_E_INTERNAL) return dead(V.status);
      return fail(GzPartsFail{V.status, V.bad_trailer, V.bad_member, V.err_off});
    }
    s = call.next;
    *in_used = call.in_used;
    if (call.at_end) {
      s.status = FLATE_HIP_STREAM_END;
      return FLATE_HIP_STREAM_END;
    }
    return FLATE_HIP_OK;
  } catch (const std::exception &e) {
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

}  // extern "C"

// ---- the LONG entries of a ZIP archive through units (zip_units_kernels.hip, zip_units_rule.h) ----
// The two-list discovery (unit_discovery.h) and flate_hip_gzfile_read's rounds with the format's own glue: the hull as
// the raw stream, B nodes from the directory (no count pass, no chain of their own), the link that hops from entry to
// entry, no tail probe, pieces in ZIP's slots.  Read-backs: the candidate count;
// the head words with entry_unit; the rounds' first_bad / decode_bad (g).
int flate_host::zip_units_decode(flate_hip_ctx *c, const uint8_t *d_in, uint64_t hull_lo, uint64_t hull_hi,
                                 const std::vector<ZuEntry> &L, const std::vector<ZuRange> &R, uint8_t *d_out,
                                 uint64_t total, uint32_t *g, ZipUnitsDecParams &G, uint32_t *n_units, uint32_t *n_cand) {
  int rc;
  *g = 0, *n_units = 0, *n_cand = 0;
  G = ZipUnitsDecParams{};
  ZipUnitsParams P{};
  OneParams PA{};
  ChainParams &C = P.O.C;
  const uint8_t *h_in = d_in + hull_lo;  // every offset below is counted from here
  const uint64_t hull_len = hull_hi - hull_lo;
  const uint32_t nb = (uint32_t)L.size();
  if (nb == 0 || R.size() != L.size() || hull_len == 0) return FLATE_HIP_E_INTERNAL;
  uint32_t n_tiles = 0;
  if ((rc = tiles_for(h_in, 0, hull_len, &n_tiles))) return rc;
  OneHead *head_a;
  ZuEntry *dL;
  ZuRange *dR;
  rc = carve(c, c->d_zip_units_tiles, [&](Carve &k) {
    k.take(P.O.head, 1);
    k.take(P.zh, 1);
    k.take(P.O.one, 1);
    k.take(head_a, 1);
    k.take(PA.C.tile_cnt, (size_t)n_tiles + 1);
    k.take(dL, nb);
    k.take(dR, nb);
    k.take(P.entry_unit, (size_t)nb + 2);
  });
  if (rc) return rc;
  P.L = dL, P.R = dR;
  HIP_TRY(c, hipMemcpyAsync(dL, L.data(), (size_t)nb * sizeof(ZuEntry), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(dR, R.data(), (size_t)nb * sizeof(ZuRange), hipMemcpyHostToDevice, c->stream));
  C.in = h_in;
  C.in_len = hull_len;
  C.n_tiles = n_tiles;
  C.head = &P.O.head->h;
  P.O.unit_max = c->one_unit_max;
  P.O.stored_units = c->one_stored_units;
  find_params(PA, P.O, head_a);
  hipLaunchKernelGGL(one_init_kernel, dim3(1), dim3(64), 0, c->stream, P.O.one, hull_len);  // the hull is the raw stream
  find_count(c, PA, false);
  OneHead HA{};
  if ((rc = find_counts_back(c, head_a, HA))) return rc;
  const uint32_t na = HA.h.n_cand;
  if ((rc = two_list_size(C, PA.C, nullptr, na, nb))) return rc;  // (List B is the directory's: no chain of its own)
  P.n_a = na;
  P.n_b = nb;
  *n_cand = na;

  rc = unit_nodes_carve(c, c->d_zip_units, P, P.u_entry, C.cap, [](Carve &) {}, [](Carve &) {});
  if (rc) return rc;
  PA.C.cand_off = C.cand_off;
  if (na) one_find_launch(c, false, n_tiles, PA, false);
  hipLaunchKernelGGL(zip_units_bits_kernel, dim3((nb + 255) / 256), dim3(256), 0, c->stream, P);
  one_probe_launch(c, C.cap, P.O, 0u);
  OneHead H{};
  ZipUnitsHead Z{};
  std::vector<uint64_t> entry_unit((size_t)nb + 2, 0);
  rc = unit_chain(
      c, P.O, [&](dim3 g) { hipLaunchKernelGGL(zip_units_link_kernel, g, dim3(256), 0, c->stream, P); },
      [&](dim3 g) { hipLaunchKernelGGL(zip_units_finish_kernel, g, dim3(256), 0, c->stream, P); }, [](uint32_t) {},
      [&](uint32_t node_blocks) {  // (ZIP's chain has no tail probe)
        hipLaunchKernelGGL(zip_units_entries_kernel, dim3(1), dim3(1024), 0, c->stream, P);
        hipLaunchKernelGGL(zip_units_rel_kernel, dim3(node_blocks), dim3(256), 0, c->stream, P);
      },
      H, Z, P.zh, [&]() -> int {
        HIP_TRY(c, hipMemcpyAsync(entry_unit.data(), P.entry_unit, ((size_t)nb + 2) * 8, hipMemcpyDeviceToHost, c->stream));
        return FLATE_HIP_OK;
      });
  if (rc) return rc;
  if (Z.n_complete > nb) return FLATE_HIP_E_INTERNAL;
  // the entries the discovery finds GOOD, and their units: the only ones that are decoded
  const uint32_t g_disc = Z.n_complete < Z.first_unfit ? Z.n_complete : Z.first_unfit;
  G.P = P;
  if (g_disc == 0) return FLATE_HIP_OK;
  if (entry_unit[g_disc] > H.h.n_members) return FLATE_HIP_E_INTERNAL;
  const uint32_t n_dec = (uint32_t)entry_unit[g_disc];

  const uint32_t per_round = unit_per_round(c, n_dec);
  const size_t pieces = 2 * (size_t)per_round;
  OneDecParams &D = G.D;
  UnitResults dec;
  rc = unit_rounds_carve(c, D, n_dec, per_round, [&](Carve &k) { unit_pieces_take(k, D, &dec, pieces); });
  if (rc) return rc;
  rc = carve(c, c->d_zip_units_dec, [&](Carve &k) {
    k.take(G.seed, per_round);
    k.take(G.p_bit_off, pieces);
    k.take(G.p_bit_end, pieces);
    k.take(G.du_status, per_round);
    k.take(G.du_out_len, per_round);
  });
  if (rc) return rc;
  if ((rc = unit_dec_params(c, D, h_in, P.O.one, C.member_off, C.out_off, P.O.stored_units, true))) return rc;
  unit_verdict_params(D, total, UnitResults{G.du_status, G.du_out_len, nullptr}, P.O.head, FLATE_HIP_WRAP_RAW, hull_len);
  G.dp_status = dec.status;
  G.dp_out_len = dec.out_len;
  // the pieces and the seeds of the round (every entry's first unit is one)
  auto round_pieces = [&](uint32_t, uint32_t count) {
    hipLaunchKernelGGL(zip_units_pieces_kernel, dim3((count + 1u + 255u) / 256u), dim3(256), 0, c->stream, G);
    return FLATE_HIP_OK;
  };
  uint32_t e_at = 0;  // the entry of the round's first unit
  auto decode = [&](uint32_t u0, uint32_t count) {
    // the round's pieces: its units and a gap in front of every entry that starts behind its first unit
    while (entry_unit[e_at + 1u] <= u0) ++e_at;
    uint32_t e_hi = e_at;
    while (e_hi + 1u < g_disc && entry_unit[e_hi + 1u] < (uint64_t)u0 + count) ++e_hi;
    const uint32_t n_pieces = count + (e_hi - e_at);
    const uint32_t unit_blocks = (count + 1u + 255u) / 256u;
    const int r = unit_decode(c, unit_decode_params(D, h_in, hull_len, G.p_bit_off, G.p_bit_end, false, n_pieces, d_out,
                                                    D.p_out_off, dec));
    if (r) return r;
    hipLaunchKernelGGL(zip_units_fold_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, G);
    OneDecParams K = D;  // the check: status 0 and exactly out_off[k + 1] - out_off[k] bytes
    K.p_out_off = C.out_off + u0;
    hipLaunchKernelGGL(one_check_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, K);
    return FLATE_HIP_OK;
  };
  // TAIL with the entry-relative offsets: a unit's history is what its own entry has produced in front of it
  if ((rc = unit_rounds(c, D, P.rel_off, G.seed, 0, n_dec, n_dec, per_round, unit_no_hook, round_pieces, decode))) return rc;
  // the one small read-back of g
  OneDecHead DH{};
  HIP_TRY(c, hipMemcpyAsync(&DH, D.dh, sizeof DH, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t bad_unit = DH.first_bad < DH.decode_bad ? DH.first_bad : DH.decode_bad;
  *g = zip_units_served(entry_unit.data(), g_disc, bad_unit);
  *n_units = (uint32_t)entry_unit[*g];
  return FLATE_HIP_OK;
}
