// flate_api_inflate.hip -- the decode calls of the C ABI (see include/flate_hip.h): flate_hip_inflate_batch, _batch_dict,
// _batch_framed, _spliced, _spliced_framed, the BGZF and plain gzip member files and the flate_hip_inflate_stream_*
// handle.  The calls that decode long data as parallel units are flate_api_units.hip's.
//
// One driver (inflate_common) serves the five batch calls as a sequence: stage the input and the index arrays, the
// container's part in front of the decoders, the decoders (inflate_route.h says which; launch_decoders is the only
// place that knows kernels), the container's part behind them, read back.  The argument checks are api_checks.h's; the
// ctx, its staging and the host pipeline are flate_api.hip's (flate_ctx.h).
#include "flate_ctx.h"

#include <cstring>
#include <exception>
#include <stdexcept>

#include "api_checks.h"
#include "bgzf_range_rule.h"
#include "bgzf_rule.h"
#include "gzfile_rule.h"
#include "gzip_rule.h"
#include "window_compose.h"

using namespace flate;
using namespace flate_host;

// One decode call as its entry point received and checked it.  spliced_len != 0: `in` is ONE stream (or one member
// around it) of that many bytes and in_off holds the bit positions of its n pieces.
struct InfCall {
  const uint8_t *in;
  const uint64_t *in_off;
  uint32_t n;
  uint8_t *out;
  const uint64_t *out_off;
  uint64_t *out_len;
  int32_t *status;
  int64_t *err_off;
  uint32_t flags;
  uint64_t spliced_len;
  // members of a container that are NOT consecutive in `in` (flate_hip_bgzf_read_ranges: the touched members of a file):
  // member i = in[in_off[i], in_end[i]); null: it ends at in_off[i + 1].  With an InfFrame and device pointers only.
  const uint64_t *in_end = nullptr;
};

// Preset dictionaries of a launch (flate_hip_inflate_batch_dict): the device tails and, per stream of the
// launch, where its tail starts and how long it is (0 = none); h_len: the same lengths on the host.
struct InfDict {
  const uint8_t *buf;
  const uint64_t *at;
  const uint32_t *len;
  const uint32_t *h_len;
};

// The container of flate_hip_inflate_batch_framed (frame_kernels.hip: frame_parse_kernel / frame_verdict_kernel);
// everything here is the caller's.
struct InfFrame {
  uint32_t wrap;             // FLATE_HIP_WRAP_ZLIB / _GZIP
  const uint8_t *dicts;      // the WHOLE dictionaries (host, or device under FLATE_HIP_DEVICE_PTRS) ...
  const uint64_t *dict_off;  // ... dictionary j = dicts[dict_off[j], dict_off[j+1])
  uint32_t n_dicts;
  uint32_t *dict_used;       // host, per member (may be null): the dictionary its DICTID chose
};

// The container of flate_hip_inflate_spliced_framed: ONE member around the spliced stream (frame_kernels.hip:
// frame_rebase_kernel / frame_verdict_spliced_kernel).  The member's verdict comes back here.
struct InfMember {
  uint32_t wrap;  // FLATE_HIP_WRAP_ZLIB / _GZIP
  int32_t status = 0;
  int64_t err_off = -1;
};

// ---- the decoders ----

using InfKernel = void (*)(InfParams);
static const struct {
  int decoder, shape, lanes, row;
  InfKernel k[2];  // without / with preset dictionaries
} kDecoders[] = {
    {kDecodeWave, 0, 0, 0, {inflate_kernel, inflate_dict_kernel}},
    {kDecodeSpec, 1, 0, 0, {inflate_spec_kernel<FLATE_SPEC_SMALL>, inflate_spec_dict_kernel<FLATE_SPEC_SMALL>}},
    {kDecodeSpec, 2, 0, 0, {inflate_spec_kernel<FLATE_SPEC_LARGE>, inflate_spec_dict_kernel<FLATE_SPEC_LARGE>}},
    {kDecodeSimt, 0, 16, 0, {inflate_simt_kernel<16, 0>, inflate_simt_dict_kernel<16, 0>}},
    {kDecodeSimt, 0, 32, 0, {inflate_simt_kernel<32, 0>, inflate_simt_dict_kernel<32, 0>}},
    {kDecodeSimt, 0, 64, 0, {inflate_simt_kernel<64, 0>, inflate_simt_dict_kernel<64, 0>}},
    {kDecodeSimt, 0, 64, 8, {inflate_simt_kernel<64, 8>, inflate_simt_dict_kernel<64, 8>}},
    {kDecodeSimt, 0, 64, 16, {inflate_simt_kernel<64, 16>, inflate_simt_dict_kernel<64, 16>}},
};

int flate_host::launch_decoders(flate_hip_ctx *c, const InflateRoute &rt, InfParams I, bool dict) {
  InfKernel k = nullptr;
  for (const auto &e : kDecoders)
    if (e.decoder == rt.decoder && e.shape == rt.shape && e.lanes == rt.lanes && e.row == rt.row) k = e.k[dict ? 1 : 0];
  if (!k) {
    c->hip_err = "no decoder kernel for the chosen route";
    return FLATE_HIP_E_INTERNAL;
  }
  StageTimer t(c, FLATE_HIP_STAGE_INFLATE);
  if (rt.decoder != kDecodeSimt) {  // one wavefront per stream
    hipLaunchKernelGGL(k, dim3(I.n_streams), dim3(64), 0, c->stream, I);
    return FLATE_HIP_OK;
  }
  // one lane per stream, in equal rounds (inflate_route.h)
  const uint32_t sblocks = (I.n_streams + (uint32_t)rt.lanes - 1) / (uint32_t)rt.lanes;
  const int rc = ensure(c, c->d_simt_lens, inflate_simt_lens_bytes(rt.blocks_per_launch));
  if (rc) return rc;
  I.simt_lens = (uint32_t *)c->d_simt_lens.p;
  for (uint32_t b0 = 0; b0 < sblocks; b0 += rt.blocks_per_launch) {
    const uint32_t nb = sblocks - b0 < rt.blocks_per_launch ? sblocks - b0 : rt.blocks_per_launch;
    I.sid0 = b0 * (uint32_t)rt.lanes;
    hipLaunchKernelGGL(k, dim3(nb), dim3(64), inflate_simt_lds_bytes(rt.lanes), c->stream, I);
  }
  return FLATE_HIP_OK;
}

// ---- a batch of members (flate_hip_inflate_batch_framed) ----

// members_before: the DICTIDs' checksums, the tails' places (8 + 4 bytes per dictionary)
static CtlBytes members_before_ctl(const InfFrame &FRD) {
  return {dictid_ctl_up_bytes(FRD.dict_off, FRD.n_dicts) + (size_t)FRD.n_dicts * 12 + 1024, 0};
}

// In front of the decoders: the DICTIDs, the arrays the parse kernel fills, and -- the host cannot know which
// dictionaries the members name before the device has parsed -- the tail of EVERY non-empty dictionary, staged as for
// flate_hip_inflate_batch_dict; then frame_parse_kernel.  The decoders read the raw streams' ranges and their
// dictionaries from what that kernel writes; `dict`: run their dictionary build (whenever a non-empty dictionary is
// passed).  sum_slots: what members_after's checksums will run over (null: nothing).
static int members_before(flate_hip_ctx *c, const InfFrame &FRD, const uint8_t *d_in, const uint64_t *sum_slots,
                          uint32_t n, uint32_t flags, InfParams &I, FrameReadParams &R, bool &dict) {
  int rc;
  // both runs of checksums carve slot 0 of the scratch: sized once for the larger, so that the second does not free
  // what the first's kernels are still to read
  size_t scratch = dictid_scratch_bytes(FRD.dict_off, FRD.n_dicts);
  if (sum_slots && checksum_scratch_bytes(sum_slots, n) > scratch) scratch = checksum_scratch_bytes(sum_slots, n);
  void *unused = nullptr;
  if ((rc = ctx_scratch(c, 0, scratch, &unused))) return rc;
  // (for the DICTIDs the whole dictionaries are uploaded, not only their tails)
  if ((rc = dictid_stage(c, FRD.dicts, FRD.dict_off, FRD.n_dicts, flags))) return rc;
  if ((rc = ensure(c, c->d_frame_off, ((size_t)n + 1) * 8))) return rc;
  if ((rc = ensure(c, c->d_rd_end, (size_t)n * 8 + 8))) return rc;
  if ((rc = ensure(c, c->d_rd_want, (size_t)n * 4 + 4))) return rc;
  if ((rc = ensure(c, c->d_rd_isize, (size_t)n * 4 + 4))) return rc;
  if ((rc = ensure(c, c->d_rd_bad, (size_t)n * 4 + 4))) return rc;
  if ((rc = ensure(c, c->d_rd_dict, (size_t)n * 4 + 4))) return rc;
  R.in = d_in;
  R.in_off = (const uint64_t *)c->d_in_off.p;
  R.n_streams = n;
  R.wrap = FRD.wrap;
  R.n_dicts = FRD.n_dicts;
  R.pay_off = (uint64_t *)c->d_frame_off.p;
  R.pay_end = (uint64_t *)c->d_rd_end.p;
  R.want = (uint32_t *)c->d_rd_want.p;
  R.isize = (uint32_t *)c->d_rd_isize.p;
  R.bad = (uint32_t *)c->d_rd_bad.p;
  R.dict_used = (uint32_t *)c->d_rd_dict.p;
  R.out_len = I.out_len;
  R.status = I.status;
  R.err_off = I.err_off;
  if (FRD.n_dicts) {
    std::vector<uint32_t> every(FRD.n_dicts);
    for (uint32_t j = 0; j < FRD.n_dicts; ++j) every[j] = j;
    const DictSlots S = dict_slots(FRD.dict_off, FRD.n_dicts, every.data(), FRD.n_dicts, 1);
    std::vector<uint64_t> t_at(FRD.n_dicts, 0);
    std::vector<uint32_t> t_len(FRD.n_dicts, 0);
    for (uint32_t j = 0; j < FRD.n_dicts; ++j) {
      if (S.slot_of[j] == DictSlots::kNone) continue;
      t_at[j] = S.at[S.slot_of[j]];
      t_len[j] = S.len[S.slot_of[j]];
    }
    if ((rc = dict_upload(c, S, FRD.dicts, FRD.dict_off, flags))) return rc;
    if ((rc = ensure(c, c->d_rd_tail_at, (size_t)FRD.n_dicts * 8 + 8))) return rc;
    if ((rc = ensure(c, c->d_rd_tail_len, (size_t)FRD.n_dicts * 4 + 4))) return rc;
    if ((rc = ensure(c, c->d_dict_at, (size_t)n * 8 + 8))) return rc;
    if ((rc = ensure(c, c->d_dict_len, (size_t)n * 4 + 4))) return rc;
    if ((rc = ctl_up(c, c->d_rd_tail_at.p, t_at.data(), (size_t)FRD.n_dicts * 8))) return rc;
    if ((rc = ctl_up(c, c->d_rd_tail_len.p, t_len.data(), (size_t)FRD.n_dicts * 4))) return rc;
    R.dict_id = (const uint32_t *)c->d_frame_ids.p;
    R.tail_at = (const uint64_t *)c->d_rd_tail_at.p;
    R.tail_len = (const uint32_t *)c->d_rd_tail_len.p;
    R.dict_at = (uint64_t *)c->d_dict_at.p;
    R.dict_len = (uint32_t *)c->d_dict_len.p;
    dict = !S.at.empty();
    if (dict) {
      I.dict_buf = (const uint8_t *)c->d_dicts.p;
      I.dict_at = R.dict_at;
      I.dict_len = R.dict_len;
    }
  }
  I.in_off = R.pay_off;
  I.in_end = R.pay_end;
  hipLaunchKernelGGL(frame_parse_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, R);
  return FLATE_HIP_OK;
}

// members_after: the checksums of what was produced (sum_slots: the slots, null: a size-only pass stored nothing);
// down: dict_used
static CtlBytes members_after_ctl(const uint64_t *sum_slots, uint32_t n) {
  CtlBytes b{0, (size_t)n * 4 + 256};
  if (sum_slots) b.up = checksum_ctl_up_bytes(sum_slots, n);
  return b;
}

// Behind the decoders: the sums of what every member produced (nothing is stored by a size-only pass: nothing to
// sum), then the verdict.
static int members_after(flate_hip_ctx *c, const InfFrame &FRD, const uint8_t *d_out, const uint64_t *sum_slots,
                         uint32_t n, FrameReadParams &R) {
  int rc;
  StageTimer t(c, FLATE_HIP_STAGE_CHECKSUM);
  if (sum_slots) {
    if ((rc = ensure(c, c->d_frame_sums, (size_t)n * 4 + 8))) return rc;
    if ((rc = checksum_device_clipped(c, d_out, sum_slots, n, frame_sum_kind(FRD.wrap), (const uint64_t *)c->d_out_len.p,
                                      (const int32_t *)c->d_istatus.p, (const uint32_t *)c->d_rd_bad.p,
                                      (uint32_t *)c->d_frame_sums.p)))
      return rc;
    R.sums = (const uint32_t *)c->d_frame_sums.p;
  }
  hipLaunchKernelGGL(frame_verdict_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, R);
  HIP_TRY(c, hipGetLastError());
  return FRD.dict_used ? ctl_down(c, FRD.dict_used, c->d_rd_dict.p, (size_t)n * 4) : FLATE_HIP_OK;
}

// ---- one member around a spliced stream (flate_hip_inflate_spliced_framed) ----

// member_before: the one range {0, in_len} of FrameOne
static CtlBytes member_before_ctl() { return {sizeof(FrameOne) + 1024, 0}; }

// In front of the decoders: frame_parse_kernel over the one range {0, in_len}, then frame_rebase_kernel, which moves
// the uploaded index (I.in_off, counted from the raw stream's first byte) behind the header the device has just
// measured.  The decoders read the member from its first byte up to its trailer.
static int member_before(flate_hip_ctx *c, const InfMember &SM, const uint8_t *d_in, uint64_t in_len, uint32_t n,
                         InfParams &I, FrameSplicedParams &S) {
  int rc;
  if ((rc = ensure(c, c->d_rd_one, sizeof(FrameOne) + 16))) return rc;
  if ((rc = ensure(c, c->d_frame_off, ((size_t)n + 1) * 8))) return rc;
  if ((rc = ensure(c, c->d_frame_sums, (size_t)n * 4 + 8))) return rc;
  if ((rc = ensure(c, c->d_rd_bad, (size_t)n * 4 + 4))) return rc;
  FrameOne *one = (FrameOne *)c->d_rd_one.p;
  const uint64_t range[2] = {0, in_len};
  if ((rc = ctl_up(c, one->in_off, range, sizeof range))) return rc;
  FrameReadParams R{};
  R.in = d_in;
  R.in_off = one->in_off;
  R.n_streams = 1;
  R.wrap = SM.wrap;
  R.pay_off = one->pay_off;
  R.pay_end = &one->pay_end;
  R.want = &one->want;
  R.isize = &one->isize;
  R.bad = &one->bad;
  R.dict_used = &one->dict_used;
  hipLaunchKernelGGL(frame_parse_kernel, dim3(1), dim3(256), 0, c->stream, R);
  S.one = one;
  S.bit_in = I.in_off;
  S.bit_out = (uint64_t *)c->d_frame_off.p;
  S.piece_bad = (uint32_t *)c->d_rd_bad.p;
  S.n_pieces = n;
  S.wrap = SM.wrap;
  S.in_len = in_len;
  S.raw_end = in_len - frame_trailer_len(SM.wrap);  // (the entry point has checked in_len)
  S.out_len = I.out_len;
  S.status = I.status;
  S.err_off = I.err_off;
  hipLaunchKernelGGL(frame_rebase_kernel, dim3(n / 256 + 1), dim3(256), 0, c->stream, S);
  HIP_TRY(c, hipGetLastError());
  I.bit_off = S.bit_out;
  I.in_len = S.raw_end;
  return FLATE_HIP_OK;
}

// member_after: the pieces' checksums; down: the member's two words
static CtlBytes member_after_ctl(const uint64_t *out_off, uint32_t n) { return {checksum_ctl_up_bytes(out_off, n), 1024}; }

// Behind the decoders: the sums of what every piece produced, their join into the member's, then the verdict.
static int member_after(flate_hip_ctx *c, InfMember &SM, const uint8_t *d_out, const uint64_t *out_off, uint32_t n,
                        const FrameSplicedParams &S) {
  int rc;
  StageTimer t(c, FLATE_HIP_STAGE_CHECKSUM);
  const uint32_t kind = frame_sum_kind(SM.wrap);
  if ((rc = checksum_device_clipped(c, d_out, out_off, n, kind, (const uint64_t *)c->d_out_len.p,
                                    (const int32_t *)c->d_istatus.p, (const uint32_t *)c->d_rd_bad.p,
                                    (uint32_t *)c->d_frame_sums.p)))
    return rc;
  if ((rc = checksum_join_device(c, (const uint32_t *)c->d_frame_sums.p, (const uint64_t *)c->d_slot_off.p,
                                 (const uint64_t *)c->d_out_len.p, n, kind, &S.one->sum, &S.one->total)))
    return rc;
  hipLaunchKernelGGL(frame_verdict_spliced_kernel, dim3(1), dim3(1024), 0, c->stream, S);
  HIP_TRY(c, hipGetLastError());
  if ((rc = ctl_down(c, &SM.status, &S.one->member_status, 4))) return rc;
  return ctl_down(c, &SM.err_off, &S.one->member_err_off, 8);
}

// ---- the driver of the five batch calls ----
// D != NULL: the streams' dictionaries (a launch in which a stream has one runs the decoders' dictionary build).
// FRD != NULL: the streams are members of a container, parsed in front of the decoders and checked behind them.
// SM != NULL (a spliced call): `in` is ONE member around the spliced stream and in_off is counted from the raw stream's
// first byte; the return value is the member's status.
static int inflate_common(flate_hip_ctx *c, const InfCall &A, const InfDict *D = nullptr, const InfFrame *FRD = nullptr,
                          InfMember *SM = nullptr) {
  const uint32_t n = A.n;
  const bool spliced = A.spliced_len != 0;
  const bool size_only = (A.flags & FLATE_HIP_SIZE_ONLY) != 0 && !spliced;
  const bool dev = (A.flags & FLATE_HIP_DEVICE_PTRS) != 0;
  const uint64_t in_bytes = spliced ? A.spliced_len : A.in_off[n];
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;

  // stage the input and the index arrays
  const uint64_t *out_off = A.out_off;
  std::vector<uint64_t> no_slots;
  if (size_only) {  // nothing is stored: no output buffer, no slots
    no_slots.assign((size_t)n + 1, 0);
    out_off = no_slots.data();
  }
  const uint64_t *sum_slots = size_only ? nullptr : out_off;  // (what a container's checksums run over)
  const uint8_t *d_in = A.in;
  uint8_t *d_out = A.out;
  if (!dev) {
    if ((rc = ensure(c, c->d_in, in_bytes + 16))) return rc;
    if ((rc = ensure(c, c->d_out, out_off[n] + 16))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_in.p, A.in, in_bytes, hipMemcpyHostToDevice, c->stream));
    d_in = (const uint8_t *)c->d_in.p;
    d_out = (uint8_t *)c->d_out.p;
  }
  if ((rc = ensure(c, c->d_in_off, ((size_t)n + 1) * 8))) return rc;
  if ((rc = ensure(c, c->d_slot_off, ((size_t)n + 1) * 8))) return rc;
  if ((rc = ensure(c, c->d_out_len, (size_t)n * 8 + 8))) return rc;
  if ((rc = ensure(c, c->d_istatus, (size_t)n * 4 + 4))) return rc;
  if ((rc = ensure(c, c->d_ierr, (size_t)n * 8 + 8))) return rc;
  if (A.in_end && (rc = ensure(c, c->d_in_end, (size_t)n * 8 + 8))) return rc;
  // up: in_off, out_off (the members' ends); down: out_len, status, err_off
  CtlBytes ctl{((size_t)n + 1) * 16 + (A.in_end ? (size_t)n * 8 + 8 : 0), (size_t)n * 20 + 64};
  if (FRD) {
    ctl += members_before_ctl(*FRD);
    ctl += members_after_ctl(sum_slots, n);
  }
  if (SM) {
    ctl += member_before_ctl();
    ctl += member_after_ctl(out_off, n);
  }
  if ((rc = ctl_begin(c, ctl.up, ctl.down))) return rc;
  if ((rc = ctl_up(c, c->d_in_off.p, A.in_off, ((size_t)n + 1) * 8))) return rc;
  if ((rc = ctl_up(c, c->d_slot_off.p, out_off, ((size_t)n + 1) * 8))) return rc;
  if (A.in_end && (rc = ctl_up(c, c->d_in_end.p, A.in_end, (size_t)n * 8))) return rc;
  InfParams I{};
  I.in = d_in;
  I.in_off = (const uint64_t *)c->d_in_off.p;
  I.out = d_out;
  I.out_off = (const uint64_t *)c->d_slot_off.p;
  I.out_len = (uint64_t *)c->d_out_len.p;
  I.status = (int32_t *)c->d_istatus.p;
  I.err_off = (int64_t *)c->d_ierr.p;
  I.n_streams = n;
  I.bit_off = spliced ? (const uint64_t *)c->d_in_off.p : nullptr;
  I.in_len = in_bytes;
  I.size_only = size_only ? 1u : 0u;
  bool dict = false;
  if (D) {
    I.dict_buf = D->buf;
    I.dict_at = D->at;
    I.dict_len = D->len;
    for (uint32_t i = 0; i < n && !dict; ++i) dict = D->h_len[i] != 0;
  }

  // the container in front of the decoders
  FrameReadParams R{};
  FrameSplicedParams S{};
  if (A.in_end) R.in_end = (const uint64_t *)c->d_in_end.p;
  if (A.in_end && !FRD && !SM) I.in_end = (const uint64_t *)c->d_in_end.p;  // (raw streams: inflate_ranges_device)
  if (FRD && (rc = members_before(c, *FRD, d_in, sum_slots, n, A.flags, I, R, dict))) return rc;
  if (SM && (rc = member_before(c, *SM, d_in, in_bytes, n, I, S))) return rc;

  const InflateRoute route = inflate_route(c->inflate, c->num_cus, n, longest_entry(A.in_off, A.in_end, n), spliced, size_only);
  if ((rc = launch_decoders(c, route, I, dict))) return rc;
  HIP_TRY(c, hipGetLastError());

  // the container behind them
  if (FRD && (rc = members_after(c, *FRD, d_out, sum_slots, n, R))) return rc;
  if (SM && (rc = member_after(c, *SM, d_out, out_off, n, S))) return rc;

  // read back, synchronise, fold the statuses
  if ((rc = ctl_down(c, A.out_len, c->d_out_len.p, (size_t)n * 8))) return rc;
  if ((rc = ctl_down(c, A.status, c->d_istatus.p, (size_t)n * 4))) return rc;
  if ((rc = ctl_down(c, A.err_off, c->d_ierr.p, (size_t)n * 8))) return rc;
  if (!dev && !size_only)
    HIP_TRY(c, hipMemcpyAsync(A.out, c->d_out.p, out_off[n], hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  ctl_finish(c);
  const bool used[FLATE_HIP_STAGE_COUNT] = {false, false, FRD != nullptr || SM != nullptr, true};
  if ((rc = collect_timing(c, used))) return rc;
  // A size-only pass has no capacity -- but the kernels count output in 32 bits: a stream that inflates
  // to 4 GiB or more stops there with "slot too small", which for a call without slots means "too large"
  if (size_only)
    for (uint32_t i = 0; i < n; ++i)
      if (A.status[i] == FLATE_HIP_E_OUT_TOO_SMALL) A.status[i] = FLATE_HIP_E_TOO_LARGE;
  if (SM) return SM->status;  // (the first non-zero piece status, or the trailer's verdict with every piece at 0)
  for (uint32_t i = 0; i < n; ++i)
    if (A.status[i]) return A.status[i];
  return FLATE_HIP_OK;
}

// Host-pointer inflate of independent streams, pipelined like deflate_host_pipelined: every
// stream has its own input range and output slot, so a group is a contiguous range of both.
static int inflate_host_pipelined(flate_hip_ctx *c, const InfCall &A, uint32_t G, const InfDict *D) {
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t *in_off = A.in_off, *out_off = A.out_off;
  int rc;
  if ((rc = ensure(c, c->d_in, in_off[A.n] + 16))) return rc;
  if ((rc = ensure(c, c->d_out, out_off[A.n] + 16))) return rc;
  if ((rc = host_pipe_streams(c))) return rc;
  uint8_t *d_in = (uint8_t *)c->d_in.p, *d_out = (uint8_t *)c->d_out.p;
  std::vector<uint32_t> lo(G + 1);
  std::vector<CopyJob> in_jobs(G);
  cut_by_bytes(in_off, out_off, A.n, G, lo);  // by input + output bytes (both cross PCIe)
  for (uint32_t g = 0; g < G; ++g)
    in_jobs[g] = {d_in + in_off[lo[g]], A.in + in_off[lo[g]], (size_t)(in_off[lo[g + 1]] - in_off[lo[g]])};
  const double t_call = host_now_ms();
  CopyPipe pipe(G, G);
  pipe.start(c->device, c->h2d_stream, c->d2h_stream, in_jobs);
  float stage_sum[FLATE_HIP_STAGE_COUNT] = {0, 0, 0, 0};
  std::vector<uint64_t> gin, gout;
  rc = FLATE_HIP_OK;
  int first_status = FLATE_HIP_OK;
  for (uint32_t g = 0; g < G; ++g) {
    if (!pipe.wait_in(g)) {
      rc = FLATE_HIP_E_HIP;
      break;
    }
    const uint32_t a = lo[g], cnt = lo[g + 1] - lo[g];
    gin.resize((size_t)cnt + 1);
    gout.resize((size_t)cnt + 1);
    for (uint32_t i = 0; i <= cnt; ++i) {
      gin[i] = in_off[a + i] - in_off[a];
      gout[i] = out_off[a + i] - out_off[a];
    }
    if (cnt) {
      const double ta = host_now_ms();
      InfDict gd{};  // (the group's slice of the per-stream dictionary arrays)
      if (D) gd = {D->buf, D->at + a, D->len + a, D->h_len + a};
      const InfCall GA{d_in + in_off[a], gin.data(), cnt, d_out + out_off[a], gout.data(), A.out_len + a, A.status + a,
                       A.err_off + a, A.flags | FLATE_HIP_DEVICE_PTRS, 0};
      const int r = inflate_common(c, GA, D ? &gd : nullptr);
      host_trace(t_call, "compute", g, ta, host_now_ms());
      // a stream's own failure (its status, also the return value) does not stop the batch: as in
      // one pass, every stream is decoded and the first failing status is what the call returns
      if (!is_stream_status(r)) {
        rc = r;
        break;
      }
      if (first_status == FLATE_HIP_OK) first_status = r;
      for (int k = 0; k < FLATE_HIP_STAGE_COUNT; ++k) stage_sum[k] += c->stage_ms[k];
    }
    pipe.post_out(g, {A.out + out_off[a], d_out + out_off[a], (size_t)gout[cnt]});
  }
  const std::string err = pipe.finish();
  if (rc == FLATE_HIP_OK) rc = first_status;
  if ((rc == FLATE_HIP_OK || rc == first_status) && !err.empty()) rc = FLATE_HIP_E_HIP;
  if (rc == FLATE_HIP_E_HIP && c->hip_err.empty()) c->hip_err = err;
  for (int k = 0; k < FLATE_HIP_STAGE_COUNT; ++k) c->stage_ms[k] = stage_sum[k];
  return rc;
}

// flate_hip_inflate_batch after its checks; D: the streams' dictionaries (flate_hip_inflate_batch_dict)
static int inflate_batch_run(flate_hip_ctx *c, InfCall A, const InfDict *D) {
  if (A.flags & FLATE_HIP_SIZE_ONLY) {
    A.out = nullptr, A.out_off = nullptr;
    return inflate_common(c, A, D);
  }
  // host pointers and a large batch: decode group g while g+1 is copied in and g-1 out
  if (!(A.flags & FLATE_HIP_DEVICE_PTRS) && c->host_groups > 1 &&
      A.in_off[A.n] - A.in_off[0] + A.out_off[A.n] - A.out_off[0] >= (64ull << 20)) {
    uint32_t G = (uint32_t)c->host_groups;
    const uint32_t iper = 4u * c->host_group_streams;  // (a group should still fill the lane-per-stream launch: 16384)
    if (A.n / iper < G) G = A.n / iper;
    if (G > 1) {
      try {
        return inflate_host_pipelined(c, A, G, D);
      } catch (const std::exception &e) {  // (no copy threads, out of host memory): one pass instead
        c->hip_err.clear();
      }
    }
  }
  return inflate_common(c, A, D);
}

extern "C" {

int flate_hip_inflate_batch(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n,
                            uint8_t *out, const uint64_t *out_off, uint64_t *out_len,
                            int32_t *status, int64_t *err_off, uint32_t flags) {
  if (!c || !inflate_batch_ptrs_ok(in, in_off, n, out, out_off, out_len, status, err_off, flags)) return FLATE_HIP_E_INVALID;
  c->hip_err.clear();
  if (n == 0) return FLATE_HIP_OK;
  const int rc = inflate_batch_ranges(in_off, n, out_off, flags);
  return rc ? rc : inflate_batch_run(c, {in, in_off, n, out, out_off, out_len, status, err_off, flags, 0}, nullptr);
}

int flate_hip_inflate_batch_dict(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n,
                                 const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts,
                                 const uint32_t *dict_of, uint8_t *out, const uint64_t *out_off,
                                 uint64_t *out_len, int32_t *status, int64_t *err_off, uint32_t flags) {
  // every check before any HIP call
  if (!c || !inflate_batch_ptrs_ok(in, in_off, n, out, out_off, out_len, status, err_off, flags)) return FLATE_HIP_E_INVALID;
  int rc = inflate_batch_ranges(in_off, n, out_off, flags);
  if (rc != FLATE_HIP_OK && rc != FLATE_HIP_E_TOO_LARGE) return rc;
  if (!dict_args_ok(dicts, dict_off, n_dicts, dict_of, n)) return FLATE_HIP_E_INVALID;
  // the history each stream starts with: the last kMaxMatchOffset bytes of its dictionary
  const DictSlots S = dict_slots(dict_off, n_dicts, dict_of, n, 1);
  if (S.at.empty())  // no stream has history in front of it: the plain call, its path and its results
    return flate_hip_inflate_batch(c, in, in_off, n, out, out_off, out_len, status, err_off, flags);
  c->hip_err.clear();
  if (rc) return rc;
  std::vector<uint64_t> h_at(n, 0);  // the decoders take {at, len} per stream (0 = none)
  std::vector<uint32_t> h_len(n, 0);
  for (uint32_t i = 0; i < n; ++i) {
    if (S.slot_of[i] == DictSlots::kNone) continue;
    h_at[i] = S.at[S.slot_of[i]];
    h_len[i] = S.len[S.slot_of[i]];
  }
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = dict_upload(c, S, dicts, dict_off, flags))) return rc;
  if ((rc = ensure(c, c->d_dict_at, (size_t)n * 8))) return rc;
  if ((rc = ensure(c, c->d_dict_len, (size_t)n * 4))) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->d_dict_at.p, h_at.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->d_dict_len.p, h_len.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const InfDict D{(const uint8_t *)c->d_dicts.p, (const uint64_t *)c->d_dict_at.p, (const uint32_t *)c->d_dict_len.p, h_len.data()};
  return inflate_batch_run(c, {in, in_off, n, out, out_off, out_len, status, err_off, flags, 0}, &D);
}

int flate_hip_inflate_batch_framed(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n,
                                   uint32_t wrap, const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts,
                                   uint8_t *out, const uint64_t *out_off, uint64_t *out_len, int32_t *status,
                                   int64_t *err_off, uint32_t *dict_used, uint32_t flags) {
  // every check before any HIP call
  if (!c || wrap > FLATE_HIP_WRAP_GZIP) return FLATE_HIP_E_INVALID;
  const bool with_dicts = dicts || dict_off || n_dicts;
  if (with_dicts && wrap != FLATE_HIP_WRAP_ZLIB) return FLATE_HIP_E_INVALID;  // (neither has a DICTID to choose by)
  if (!inflate_batch_ptrs_ok(in, in_off, n, out, out_off, out_len, status, err_off, flags)) return FLATE_HIP_E_INVALID;
  if (!dict_table_ok(dicts, dict_off, n_dicts)) return FLATE_HIP_E_INVALID;
  if (wrap == FLATE_HIP_WRAP_RAW) {  // the raw call: its kernels, its results
    const int rc = flate_hip_inflate_batch(c, in, in_off, n, out, out_off, out_len, status, err_off, flags);
    if (dict_used && rc != FLATE_HIP_E_INVALID && rc != FLATE_HIP_E_TOO_LARGE)
      for (uint32_t i = 0; i < n; ++i) dict_used[i] = FLATE_HIP_NO_DICT;
    return rc;
  }
  c->hip_err.clear();
  if (n == 0) return FLATE_HIP_OK;
  const int rc = inflate_batch_ranges(in_off, n, out_off, flags);
  if (rc) return rc;
  try {
    // (host pointers: one copy in, parse, decode, check, one copy out -- no "host_pipeline_groups")
    const InfFrame FRD{wrap, dicts, dict_off, n_dicts, dict_used};
    const bool size_only = (flags & FLATE_HIP_SIZE_ONLY) != 0;
    return inflate_common(c, {in, in_off, n, size_only ? nullptr : out, size_only ? nullptr : out_off, out_len, status,
                              err_off, flags, 0},
                          nullptr, &FRD);
  } catch (const std::exception &e) {  // (out of host memory in an index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

int flate_hip_inflate_spliced(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len,
                              const uint64_t *bit_off, uint32_t n, uint8_t *out,
                              const uint64_t *out_off, uint64_t *out_len, int32_t *status,
                              int64_t *err_off, uint32_t flags) {
  if (!c || !in || !in_len || !bit_off || !out_off || !out_len || !status || !err_off || (n && !out))
    return FLATE_HIP_E_INVALID;
  c->hip_err.clear();
  if (n == 0) return FLATE_HIP_OK;
  const int rc = spliced_index_check(bit_off, n, out_off, in_len, 0);
  return rc ? rc : inflate_common(c, {in, bit_off, n, out, out_off, out_len, status, err_off, flags, in_len});
}

int flate_hip_inflate_spliced_framed(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t wrap,
                                     const uint64_t *bit_off, uint32_t n, uint8_t *out, const uint64_t *out_off,
                                     uint64_t *out_len, int32_t *status, int64_t *err_off, int32_t *member_status,
                                     int64_t *member_err_off, uint32_t flags) {
  // every check before any HIP call
  if (!c || wrap > FLATE_HIP_WRAP_GZIP || (flags & FLATE_HIP_SIZE_ONLY)) return FLATE_HIP_E_INVALID;
  if (wrap == FLATE_HIP_WRAP_RAW) {  // the raw call: its kernels, its results
    const int rc = flate_hip_inflate_spliced(c, in, in_len, bit_off, n, out, out_off, out_len, status, err_off, flags);
    if (!is_stream_status(rc)) return rc;  // (refused, or failed: no verdict)
    int32_t first = 0;
    for (uint32_t i = 0; i < n && !first; ++i) first = status[i];
    if (member_status) *member_status = first;
    if (member_err_off) *member_err_off = -1;
    return rc;
  }
  if (!in || !in_len || !bit_off || !out_off || !out_len || !status || !err_off || (n && !out)) return FLATE_HIP_E_INVALID;
  c->hip_err.clear();
  if (n == 0) return FLATE_HIP_OK;
  // the shortest header and the trailer must fit, and the index must end inside what is left
  if (const int rc = spliced_index_check(bit_off, n, out_off, in_len, frame_min_len(wrap))) return rc;
  try {
    // (host pointers: one copy in, parse, decode, check, one copy out)
    InfMember SM{wrap};
    const int rc = inflate_common(c, {in, bit_off, n, out, out_off, out_len, status, err_off, flags, in_len}, nullptr,
                                  nullptr, &SM);
    if (!is_stream_status(rc)) return rc;  // (failed: no verdict was read back)
    if (member_status) *member_status = SM.status;
    if (member_err_off) *member_err_off = SM.err_off;
    return rc;
  } catch (const std::exception &e) {  // (out of host memory in an index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

}  // extern "C"

// Raw streams that are not consecutive in device memory (flate_hip_zip_read: the selected entries of an archive).
int flate_host::inflate_ranges_device(flate_hip_ctx *c, const uint8_t *d_in, const uint64_t *in_off, const uint64_t *in_end,
                                      uint32_t n, uint8_t *d_out, const uint64_t *out_off, uint64_t *out_len, int32_t *status,
                                      int64_t *err_off) {
  InfCall call{d_in, in_off, n, d_out, out_off, out_len, status, err_off, FLATE_HIP_DEVICE_PTRS, 0};
  call.in_end = in_end;
  return inflate_common(c, call);
}

// ---- BGZF files: member discovery (bgzf_kernels.hip) and the read built on it ----
namespace {

// The discovery kernels over d_in[0, in_len) (DEVICE memory), queued on the ctx's stream; H = their result words once
// the stream has drained (the call's synchronisation), P.member_off / P.out_off = the index, still on the device.  The
// arrays are sized for bgzf_first_cap candidates; a file with more (H.n_cand, counted by the first attempt) takes a
// second attempt sized from that count.  Counted in no profiling stage.
// Q (flate_hip_bgzf_reader_read): d_in is a PART of a file -- the same launches with the part's finish and out-scan
// kernels (bgzf_parts_kernels.hip), whose result words come back in *F beside H (of which n_cand alone is theirs).
int bgzf_discover(flate_hip_ctx *c, const uint8_t *d_in, uint64_t in_len, BgzfHead &H, BgzfParams &P,
                  BgzfPartParams *Q = nullptr, BgzfPartFound *F = nullptr) {
  int rc;
  P = BgzfParams{};
  ChainParams &C = P.C;
  C.in = d_in;
  C.in_len = in_len;
  if ((rc = tiles_for(d_in, 0, in_len, &C.n_tiles))) return rc;
  uint32_t cap = bgzf_first_cap(in_len);
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = chain_size(C, cap))) return rc;
    rc = carve(c, c->d_bgzf, [&](Carve &k) {
      k.take(C.head, 1);
      k.take(C.tile_cnt, (size_t)C.n_tiles + 1);
      k.take(C.cand_off, cap);
      k.take(P.cand_total, cap);
      k.take(C.jump[0], (size_t)cap + 2);
      k.take(C.jump[1], (size_t)cap + 2);
      k.take(C.path, C.path_len);
      k.take(P.isize, cap);
      k.take(C.member_off, (size_t)cap + 1);
      k.take(C.out_off, (size_t)cap + 1);
      if (Q) {
        k.take(Q->found, 1);
        k.take(Q->idx_member_off, (size_t)cap + 1);
        k.take(Q->idx_out_off, (size_t)cap + 1);
      }
    });
    if (rc) return rc;
    hipLaunchKernelGGL(bgzf_count_kernel, dim3(C.n_tiles), dim3(256), 0, c->stream, P);
    hipLaunchKernelGGL(chain_scan_kernel, dim3(1), dim3(1024), 0, c->stream, C);
    hipLaunchKernelGGL(bgzf_fill_kernel, dim3(C.n_tiles), dim3(256), 0, c->stream, P);
    if (Q) {
      Q->B = P;
      rc = chain_tail(c, C, bgzf_link_kernel, P, bgzf_part_finish_kernel, bgzf_part_out_scan_kernel, *Q);
      if (rc) return rc;
      HIP_TRY(c, hipMemcpyAsync(F, Q->found, sizeof *F, hipMemcpyDeviceToHost, c->stream));
    } else if ((rc = chain_tail(c, C, bgzf_link_kernel, P, bgzf_finish_kernel, bgzf_out_scan_kernel, P))) {
      return rc;
    }
    HIP_TRY(c, hipMemcpyAsync(&H, C.head, sizeof H, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (H.n_cand <= cap) return FLATE_HIP_OK;
    // more candidates than the arrays hold: nothing behind the scan has run; once more, sized from the count
    cap = H.n_cand;
  }
  c->hip_err = "BGZF discovery: the candidate count changed between two passes";
  return FLATE_HIP_E_INTERNAL;
}

// The tail flate_hip_bgzf_read and flate_hip_gzip_read share, behind a discovery that found a sound chain of n members
// whose output fits: d_member_off / d_out_off (n + 1 entries each) are the index, still on the device.  It comes back
// once, 16 bytes per member -- the decoders' routing and the checksum plan are host code --, then the framed gzip read
// runs over d_in (DEVICE memory: the caller's buffer or the staged copy) into the dense slots, and, for a host caller,
// out[0, out_bytes) comes down once.  Returns the first non-zero member status, with that member's index and offset
// (*bad, the reader in parts: also where its output would start and where the member in front of it lies).
struct MembersBad {
  uint32_t j = 0xffffffffu;  // the member, or 0xffffffff: none -- a non-zero return is the call's own failure
  uint64_t member_off = 0, out_off = 0, prev_off = 0;
};
int members_read(flate_hip_ctx *c, const uint8_t *d_in, uint32_t n, const uint64_t *d_member_off,
                 const uint64_t *d_out_off, uint64_t out_bytes, uint8_t *out, uint32_t flags, uint32_t *bad_member,
                 int64_t *err_off, MembersBad *bad = nullptr) {
  const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
  int rc;
  std::vector<uint64_t> moff((size_t)n + 1), ooff((size_t)n + 1), olen(n);
  std::vector<int32_t> st(n);
  std::vector<int64_t> eo(n);
  HIP_TRY(c, hipMemcpyAsync(moff.data(), d_member_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(ooff.data(), d_out_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if ((rc = inflate_batch_ranges(moff.data(), n, ooff.data(), 0))) return rc;
  uint8_t *d_out = out;
  if (!dev) {
    if ((rc = ensure(c, c->d_out, out_bytes + 16))) return rc;
    d_out = (uint8_t *)c->d_out.p;
  }
  // the framed gzip read over the staged copy, fed with the index the device has just produced
  const InfFrame FRD{FLATE_HIP_WRAP_GZIP, nullptr, nullptr, 0, nullptr};
  rc = inflate_common(c, {d_in, moff.data(), n, d_out, ooff.data(), olen.data(), st.data(), eo.data(),
                          flags | FLATE_HIP_DEVICE_PTRS, 0},
                      nullptr, &FRD);
  if (!is_stream_status(rc)) return rc;
  if (!dev && out_bytes) {
    HIP_TRY(c, hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  for (uint32_t i = 0; i < n; ++i)
    if (st[i]) {
      if (bad_member) *bad_member = i;
      if (err_off) *err_off = (int64_t)moff[i];
      if (bad) *bad = MembersBad{i, moff[i], ooff[i], i ? moff[i - 1] : 0ull};
      return st[i];
    }
  return FLATE_HIP_OK;
}

}  // namespace

// flate_hip_bgzf_reader_*: the file's state between two calls (bgzf_parts_rule.h), host words only
struct flate_hip_bgzf_reader {
  flate_hip_ctx *ctx = nullptr;
  uint32_t flags = 0;
  flate::BgzfPartsState s = flate::bgzf_parts_fresh();
};

// flate_ctx.h
int flate_host::ranges_gather(flate_hip_ctx *c, const uint8_t *scratch, uint8_t *d_out, const uint64_t *r_out_off,
                              const uint64_t *r_src, uint32_t n_ranges, uint64_t piece_bytes) {
  const uint64_t windows = (piece_bytes + (uint64_t)kBgzfGatherRangeCost * n_ranges + kBgzfGatherWindow - 1) / kBgzfGatherWindow;
  if (windows > 0x7fffffffull) return FLATE_HIP_E_TOO_LARGE;
  BgzfGatherParams G{};
  G.scratch = scratch;
  G.out = d_out;
  G.r_out_off = r_out_off;
  G.r_src = r_src;
  G.n_ranges = n_ranges;
  hipLaunchKernelGGL(bgzf_gather_kernel, dim3((uint32_t)windows), dim3(256), 0, c->stream, G);
  return FLATE_HIP_OK;
}

extern "C" {

int flate_hip_bgzf_index(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint64_t index_cap, uint64_t *member_off,
                         uint64_t *out_off, uint32_t *n_members, uint64_t *out_bytes, int *eof_marker, int64_t *err_off,
                         uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = bgzf_index_args(in, in_len, member_off, out_off, n_members, out_bytes, flags);
  if (rc) return rc;
  c->hip_err.clear();
  *n_members = 0, *out_bytes = 0;
  if (eof_marker) *eof_marker = 0;
  if (err_off) *err_off = -1;
  if (in_len == 0) {
    if (member_off && index_cap < 1) return FLATE_HIP_E_OUT_TOO_SMALL;
    if (member_off) member_off[0] = 0, out_off[0] = 0;
    return FLATE_HIP_OK;
  }
  const uint8_t *d_in = nullptr;
  if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
  BgzfHead H{};
  BgzfParams P{};
  if ((rc = bgzf_discover(c, d_in, in_len, H, P))) return rc;
  *n_members = H.n_members;
  if (H.rc) {
    if (err_off) *err_off = H.err_off;
    return H.rc;
  }
  *out_bytes = H.out_bytes;
  if (eof_marker) *eof_marker = (int)H.eof_marker;
  if (!member_off) return FLATE_HIP_OK;
  const uint64_t entries = (uint64_t)H.n_members + 1;
  if (index_cap < entries) return FLATE_HIP_E_OUT_TOO_SMALL;
  HIP_TRY(c, hipMemcpyAsync(member_off, P.C.member_off, entries * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(out_off, P.C.out_off, entries * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FLATE_HIP_OK;
}

int flate_hip_bgzf_read(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap,
                        uint64_t *out_len, uint32_t *n_members, uint32_t *bad_member, int64_t *err_off, int *eof_marker,
                        uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = bgzf_read_args(in, in_len, out, out_cap, out_len, flags);
  if (rc) return rc;
  c->hip_err.clear();
  *out_len = 0;
  if (n_members) *n_members = 0;
  if (bad_member) *bad_member = 0xffffffffu;
  if (err_off) *err_off = -1;
  if (eof_marker) *eof_marker = 0;
  if (in_len == 0) return FLATE_HIP_OK;
  try {
    const uint8_t *d_in = nullptr;
    if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
    BgzfHead H{};
    BgzfParams P{};
    if ((rc = bgzf_discover(c, d_in, in_len, H, P))) return rc;
    const uint32_t n = H.n_members;
    if (n_members) *n_members = n;
    if (H.rc) {  // a malformed chain: nothing is decoded, nothing is written
      if (bad_member) *bad_member = n;
      if (err_off) *err_off = H.err_off;
      return H.rc;
    }
    if (eof_marker) *eof_marker = (int)H.eof_marker;
    *out_len = H.out_bytes;
    if (H.out_bytes > out_cap) return FLATE_HIP_E_OUT_TOO_SMALL;
    return members_read(c, d_in, n, P.C.member_off, P.C.out_off, H.out_bytes, out, flags, bad_member, err_off);
  } catch (const std::exception &e) {  // (out of host memory in an index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

// ---- a BGZF file read in PARTS (bgzf_parts_rule.h, bgzf_parts_kernels.hip) ----
// The handle is a few host words: nothing of it lives on the device or in the ctx's scratch, so any other call on the
// ctx may run between two reads.
int flate_hip_bgzf_reader_open(flate_hip_ctx *c, uint32_t flags, flate_hip_bgzf_reader **out) {
  // every check before any HIP call (there is none)
  if (bgzf_reader_open_args(c, flags, out)) return FLATE_HIP_E_INVALID;
  flate_hip_bgzf_reader *r = new (std::nothrow) flate_hip_bgzf_reader();
  if (!r) return FLATE_HIP_E_INTERNAL;
  r->ctx = c, r->flags = flags;
  *out = r;
  return FLATE_HIP_OK;
}

int flate_hip_bgzf_reader_reset(flate_hip_bgzf_reader *r) {
  if (!r) return FLATE_HIP_E_INVALID;
  r->s = bgzf_parts_fresh();
  return FLATE_HIP_OK;
}

void flate_hip_bgzf_reader_free(flate_hip_bgzf_reader *r) { delete r; }

// One call: flate_hip_bgzf_read on the part in[0, in_len) -- the discovery with the part's finish and out-scan kernels
// (the stop behind the last whole member, the clip to out_cap and index_cap, the index in FILE coordinates), the words
// and the delivered members' index back, bgzf_parts_call, then members_read over the delivered members.
int flate_hip_bgzf_reader_read(flate_hip_bgzf_reader *r, const uint8_t *in, uint64_t in_len, int final_in, uint8_t *out,
                               uint64_t out_cap, uint64_t *in_used, uint64_t *out_len, uint64_t index_cap,
                               uint64_t *member_off, uint64_t *out_off, uint32_t *n_members, uint32_t *bad_member,
                               int64_t *err_off, int *eof_marker) {
  // every check before any HIP call
  if (bgzf_reader_read_args(r, in, in_len, out, out_cap, in_used, out_len, index_cap, member_off, out_off))
    return FLATE_HIP_E_INVALID;
  *in_used = 0, *out_len = 0;
  if (n_members) *n_members = 0;
  BgzfPartsState &s = r->s;
  if (member_off) member_off[0] = s.consumed, out_off[0] = s.produced;  // (a call that delivers nothing: where the file stands)
  auto words = [&]() {
    const bool bad = s.status < 0;
    if (bad_member) *bad_member = bad ? s.bad_member : 0xffffffffu;
    if (err_off) *err_off = bad ? s.err_off : -1;
    if (eof_marker) *eof_marker = (int)s.eof_marker;
  };
  words();
  if (s.status) return s.status;  // sticky: the file's end, or its error
  flate_hip_ctx *c = r->ctx;
  c->hip_err.clear();
  const bool fin = final_in != 0;
  if (in_len == 0) {
    if (!fin) return FLATE_HIP_OK;
    s.status = FLATE_HIP_STREAM_END;  // the file ends at a member's end (an empty file: at its start)
    return FLATE_HIP_STREAM_END;
  }
  try {
    int rc;
    const uint8_t *d_in = nullptr;
    if ((rc = stage_input(c, in, in_len, r->flags, &d_in))) return rc;
    BgzfHead H{};
    BgzfParams P{};
    BgzfPartParams Q{};
    BgzfPartFound F{};
    Q.out_cap = out_cap;
    Q.base_in = s.consumed, Q.base_out = s.produced;
    Q.k_max = bgzf_part_k_max(member_off != nullptr, index_cap);
    Q.final_in = fin ? 1u : 0u;
    if ((rc = bgzf_discover(c, d_in, in_len, H, P, &Q, &F))) return rc;
    if (F.k > F.n || F.in_end > in_len || F.out_end > out_cap) {
      c->hip_err = "BGZF reader: the part's result words do not fit the part";
      return FLATE_HIP_E_INTERNAL;
    }
    BgzfPartCall call = bgzf_parts_call(s, F, in_len, fin);
    if (call.status == FLATE_HIP_E_OUT_TOO_SMALL) {  // (not sticky: the state is unchanged)
      *out_len = call.out_len;
      return FLATE_HIP_E_OUT_TOO_SMALL;
    }
    if (member_off) {  // the delivered members' index, in FILE coordinates
      const size_t bytes = ((size_t)F.k + 1) * 8;
      HIP_TRY(c, hipMemcpyAsync(member_off, Q.idx_member_off, bytes, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(out_off, Q.idx_out_off, bytes, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    uint32_t delivered = call.decode;
    if (call.decode) {
      MembersBad bad;
      rc = members_read(c, d_in, call.decode, P.C.member_off, P.C.out_off, F.out_end, out, r->flags, nullptr, nullptr, &bad);
      if (rc && bad.j == 0xffffffffu) return rc;  // the call's own failure: nothing is committed
      if (rc) {  // member bad.j: the members in front of it are delivered, the file's error is sticky
        bool eof_before = false;
        if (bad.j && bad.member_off - bad.prev_off == kBgzfEofLen) {
          uint8_t m[kBgzfEofLen];
          HIP_TRY(c, hipMemcpyAsync(m, d_in + bad.prev_off, kBgzfEofLen, hipMemcpyDeviceToHost, c->stream));
          HIP_TRY(c, hipStreamSynchronize(c->stream));
          eof_before = bgzf_is_eof_marker(m, kBgzfEofLen);
        }
        bgzf_parts_fail(s, call, bad.j, rc, bad.member_off, bad.out_off, eof_before);
        delivered = bad.j;
      }
    }
    s = call.next;
    *in_used = call.in_used, *out_len = call.out_len;
    if (n_members) *n_members = delivered;
    words();
    return call.status;
  } catch (const std::exception &e) {  // (out of host memory in an index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

// Random access: discovery as in flate_hip_bgzf_read, then locate / select / layout (bgzf_range_kernels.hip) behind it
// on the same stream, ONE read-back (the ranges' layout and the selected members' index), the framed gzip read over
// the selected members -- which are not consecutive in the file: InfCall::in_end -- into a dense scratch, the gather.
int flate_hip_bgzf_read_ranges(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t pos_kind,
                               const uint64_t *begin, const uint64_t *end, uint32_t n_ranges, uint8_t *out,
                               uint64_t out_cap, uint64_t *out_off, int32_t *range_status, uint32_t *n_members,
                               uint32_t *n_decoded, uint32_t *bad_member, int64_t *err_off, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = bgzf_ranges_args(in, in_len, pos_kind, begin, end, n_ranges, out, out_cap, out_off, flags);
  if (rc) return rc;
  c->hip_err.clear();
  if (n_members) *n_members = 0;
  if (n_decoded) *n_decoded = 0;
  if (bad_member) *bad_member = 0xffffffffu;
  if (err_off) *err_off = -1;
  if (n_ranges == 0) {
    if (out_off) out_off[0] = 0;
    return FLATE_HIP_OK;
  }
  const uint32_t nr = n_ranges;
  if (in_len == 0) {  // no members, T = 0: the rule over the index {0}, {0}; nothing to run on the device
    const uint64_t zero = 0;
    bool invalid = false;
    out_off[0] = 0;
    for (uint32_t r = 0; r < nr; ++r) {
      const BgzfRangeLoc L = bgzf_range_locate(pos_kind, begin[r], end[r], &zero, &zero, 0);
      out_off[r + 1] = 0;
      if (range_status) range_status[r] = L.status ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
      invalid = invalid || L.status != 0;
    }
    return invalid ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
  }
  try {
    const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
    const uint8_t *d_in = nullptr;
    if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
    for (int k = 0; k < FLATE_HIP_STAGE_COUNT; ++k) c->stage_ms[k] = 0;
    BgzfHead H{};
    BgzfParams P{};
    if ((rc = bgzf_discover(c, d_in, in_len, H, P))) return rc;
    const uint32_t n = H.n_members;
    if (n_members) *n_members = n;
    if (H.rc) {  // a malformed chain: nothing is decoded, nothing is written
      if (bad_member) *bad_member = n;
      if (err_off) *err_off = H.err_off;
      for (uint32_t r = 0; r <= nr; ++r) out_off[r] = 0;
      if (range_status)
        for (uint32_t r = 0; r < nr; ++r) range_status[r] = FLATE_HIP_E_CORRUPT;
      return H.rc;
    }

    // locate, select, layout: the arrays carved from one buffer, what the host reads back as one block at its end
    BgzfRangeParams Q{};
    Q.member_off = P.C.member_off;
    Q.out_off_m = P.C.out_off;
    Q.isize = P.isize;
    Q.n_members = n;
    Q.n_ranges = nr;
    Q.pos_kind = pos_kind;
    uint64_t *d_begin, *d_end;
    size_t o_back = 0, o_end = 0;
    rc = carve(c, c->d_bgzf_rng, [&](Carve &k) {
      k.take(d_begin, nr);
      k.take(d_end, nr);
      k.take(Q.diff, (size_t)n + 1);
      k.take(Q.rank, (size_t)n + 1);
      k.take(Q.scratch_at, (size_t)n + 1);
      k.take(Q.r_b, nr);
      k.take(Q.r_len, nr);
      k.take(Q.r_first, nr);
      k.take(Q.r_last, nr);
      k.take(Q.r_src, nr);
      o_back = k.at;
      k.take(Q.head, 1);
      k.take(Q.r_out_off, (size_t)nr + 1);
      k.take(Q.r_status, nr);
      k.take(Q.r_rank_lo, nr);
      k.take(Q.r_rank_hi, nr);
      k.take(Q.sel, n, 8);
      o_end = k.at;
    });
    if (rc) return rc;
    Q.begin = d_begin, Q.end = d_end;
    const size_t back_bytes = o_end - o_back;
    const uint8_t *d_back = (const uint8_t *)c->d_bgzf_rng.p + o_back;
    HIP_TRY(c, hipMemcpyAsync(d_begin, begin, (size_t)nr * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_end, end, (size_t)nr * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(Q.diff, 0, ((size_t)n + 1) * 4, c->stream));
    hipLaunchKernelGGL(bgzf_range_locate_kernel, dim3((nr + 255u) / 256u), dim3(256), 0, c->stream, Q);
    hipLaunchKernelGGL(bgzf_range_select_kernel, dim3(1), dim3(1024), 0, c->stream, Q);
    hipLaunchKernelGGL(bgzf_range_layout_kernel, dim3(1), dim3(1024), 0, c->stream, Q);
    HIP_TRY(c, hipGetLastError());
    std::vector<uint8_t> back(back_bytes);
    HIP_TRY(c, hipMemcpyAsync(back.data(), d_back, back_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    auto got = [&](const auto *d) { return (decltype(d))(back.data() + ((const uint8_t *)d - d_back)); };  // d's host copy
    const BgzfRangeHead RH = *got(Q.head);
    const int32_t *r_status = got(Q.r_status);
    const uint32_t *r_lo = got(Q.r_rank_lo), *r_hi = got(Q.r_rank_hi);
    const BgzfSel *sel = got(Q.sel);
    const uint32_t ns = RH.n_sel;
    if (ns > n) {
      c->hip_err = "BGZF ranges: more members selected than the file has";
      return FLATE_HIP_E_INTERNAL;
    }
    memcpy(out_off, got(Q.r_out_off), ((size_t)nr + 1) * 8);
    if (n_decoded) *n_decoded = ns;
    if (range_status)
      for (uint32_t r = 0; r < nr; ++r) range_status[r] = r_status[r];
    if (RH.out_total > out_cap) return FLATE_HIP_E_OUT_TOO_SMALL;  // (the size query too: nothing is decoded)
    const int verdict = RH.any_invalid ? FLATE_HIP_E_INVALID : FLATE_HIP_OK;
    if (ns == 0 || RH.out_total == 0) return verdict;  // (no range holds a byte)

    // the framed gzip read over the selected members into the dense scratch
    std::vector<uint64_t> moff((size_t)ns + 1), mend(ns), soff((size_t)ns + 1), olen(ns);
    std::vector<int32_t> st(ns);
    std::vector<int64_t> eo(ns);
    for (uint32_t i = 0; i < ns; ++i) {
      moff[i] = sel[i].in_off, mend[i] = sel[i].in_end, soff[i] = sel[i].scratch_off;
      if (mend[i] < moff[i] || mend[i] > in_len || mend[i] - moff[i] > kBgzfMemberMax ||
          soff[i] + sel[i].isize > RH.scratch_total) {
        c->hip_err = "BGZF ranges: a selected member outside the file or the scratch";
        return FLATE_HIP_E_INTERNAL;
      }
    }
    moff[ns] = in_len, soff[ns] = RH.scratch_total;
    if ((rc = ensure(c, c->d_bgzf_dense, RH.scratch_total + 64))) return rc;
    uint8_t *d_dense = (uint8_t *)c->d_bgzf_dense.p;
    const InfFrame FRD{FLATE_HIP_WRAP_GZIP, nullptr, nullptr, 0, nullptr};
    InfCall call{d_in, moff.data(), ns, d_dense, soff.data(), olen.data(), st.data(), eo.data(),
                 flags | FLATE_HIP_DEVICE_PTRS, 0};
    call.in_end = mend.data();
    rc = inflate_common(c, call, nullptr, &FRD);
    if (!is_stream_status(rc)) return rc;

    // the gather: every range's run of the scratch to its place in out
    uint8_t *d_out = out;
    if (!dev) {
      if ((rc = ensure(c, c->d_out, RH.out_total + 16))) return rc;
      d_out = (uint8_t *)c->d_out.p;
    }
    if ((rc = ranges_gather(c, d_dense, d_out, Q.r_out_off, Q.r_src, nr, RH.out_total))) return rc;
    HIP_TRY(c, hipGetLastError());
    if (!dev) HIP_TRY(c, hipMemcpyAsync(out, d_out, RH.out_total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));

    // the statuses (a range that locate has refused keeps its status)
    const uint32_t i = range_statuses(st.data(), ns, r_lo, r_hi, nr, range_status, r_status);
    if (i < ns) {
      if (bad_member) *bad_member = sel[i].member;
      if (err_off) *err_off = (int64_t)moff[i];
      return st[i];
    }
    return verdict;
  } catch (const std::exception &e) {  // (out of host memory in an index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

}  // extern "C"

// ---- plain multi-member gzip files: member discovery (gzip_kernels.hip) and the read built on it ----
namespace {

// The discovery over d_in[0, in_len) (DEVICE memory) on the ctx's stream: count and scan, ONE read-back of the candidate
// count (the launches behind it have a thread or a wavefront per candidate), then fill, frame_parse_kernel, one
// size-only launch of the batch decoders over all candidates, link, rounds, finish, out-scan.  H = the result words once
// the stream has drained; P.C.member_off / P.C.out_off = the index, still on the device (null when the file holds no
// candidate: H then says FLATE_HIP_E_CORRUPT at offset 0).  The discovery kernels are counted in no profiling stage.
int gzip_discover(flate_hip_ctx *c, const uint8_t *d_in, uint64_t in_len, BgzfHead &H, GzipParams &P) {
  int rc;
  P = GzipParams{};
  ChainParams &C = P.C;
  C.in = d_in;
  C.in_len = in_len;
  P.member_max = c->gzip_member_max;
  if ((rc = tiles_for(d_in, 0, in_len, &C.n_tiles))) return rc;
  rc = carve(c, c->d_gzip_tiles, [&](Carve &k) {
    k.take(C.head, 1);
    k.take(C.tile_cnt, (size_t)C.n_tiles + 1);
  });
  if (rc) return rc;
  hipLaunchKernelGGL(gzip_count_kernel, dim3(C.n_tiles), dim3(256), 0, c->stream, P);
  hipLaunchKernelGGL(chain_scan_kernel, dim3(1), dim3(1024), 0, c->stream, C);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&H, C.head, sizeof H, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t cap = H.n_cand;
  if ((rc = chain_size(C, cap))) return rc;  // (the count saturates at 2^32 - 1)
  if (cap == 0) return FLATE_HIP_OK;  // (the scan kernel has left the verdict: no member can start at offset 0)

  FrameReadParams R{};
  InfParams I{};  // size-only: no output buffer, no slots
  const size_t n = cap;
  rc = carve(c, c->d_gzip, [&](Carve &k) {
    k.take(C.cand_off, n + 1);
    k.take(P.cand_end, n);
    k.take(R.pay_off, n + 1);
    k.take(R.pay_end, n);
    k.take(R.want, n);
    k.take(R.isize, n);
    k.take(R.bad, n);
    k.take(R.dict_used, n);
    k.take(I.out_len, n);
    k.take(I.status, n);
    k.take(I.err_off, n);
    k.take(I.used, n);
    k.take(C.jump[0], n + 2);
    k.take(C.jump[1], n + 2);
    k.take(C.path, C.path_len);
    k.take(P.msize, n);
    k.take(C.member_off, n + 1);
    k.take(C.out_off, n + 1);
  });
  if (rc) return rc;
  R.in = d_in;
  R.in_off = C.cand_off;
  R.in_end = P.cand_end;
  R.n_streams = cap;
  R.wrap = FLATE_HIP_WRAP_GZIP;
  I.in = d_in;
  I.in_off = R.pay_off;
  I.in_end = R.pay_end;
  I.n_streams = cap;
  I.in_len = in_len;
  I.size_only = 1u;
  P.pay_off = R.pay_off;
  P.bad = R.bad;
  P.status = I.status;
  P.out_len = I.out_len;
  P.used = I.used;
  // every candidate's range is at most member_max < 2^28 bytes: the sub-block decoder at any batch size, or -- switched
  // off -- the scalar walk; both report `used`
  const uint64_t longest = in_len < P.member_max ? in_len : P.member_max;
  const InflateRoute route = inflate_route(c->inflate, c->num_cus, cap, longest, false, true);
  if (route.decoder == kDecodeSimt) {
    c->hip_err = "gzip discovery: a size-only pass was routed to the lane-per-stream decoder";
    return FLATE_HIP_E_INTERNAL;
  }
  hipLaunchKernelGGL(gzip_fill_kernel, dim3(C.n_tiles), dim3(256), 0, c->stream, P);
  hipLaunchKernelGGL(frame_parse_kernel, dim3((cap + 255) / 256), dim3(256), 0, c->stream, R);
  HIP_TRY(c, hipGetLastError());
  if ((rc = launch_decoders(c, route, I, false))) return rc;
  if ((rc = chain_tail(c, C, gzip_link_kernel, P, gzip_finish_kernel, gzip_out_scan_kernel, P))) return rc;
  HIP_TRY(c, hipMemcpyAsync(&H, P.C.head, sizeof H, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FLATE_HIP_OK;
}

}  // namespace

extern "C" {

int flate_hip_gzip_index(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint64_t index_cap, uint64_t *member_off,
                         uint64_t *out_off, uint32_t *n_members, uint64_t *out_bytes, uint32_t *n_candidates,
                         int64_t *err_off, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = gzip_index_args(in, in_len, member_off, out_off, n_members, out_bytes, flags);
  if (rc) return rc;
  c->hip_err.clear();
  *n_members = 0, *out_bytes = 0;
  if (n_candidates) *n_candidates = 0;
  if (err_off) *err_off = -1;
  if (in_len == 0) {
    if (member_off && index_cap < 1) return FLATE_HIP_E_OUT_TOO_SMALL;
    if (member_off) member_off[0] = 0, out_off[0] = 0;
    return FLATE_HIP_OK;
  }
  const uint8_t *d_in = nullptr;
  if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
  BgzfHead H{};
  GzipParams P{};
  if ((rc = gzip_discover(c, d_in, in_len, H, P))) return rc;
  *n_members = H.n_members;
  if (n_candidates) *n_candidates = H.n_cand;
  if (err_off) *err_off = H.rc ? H.err_off : -1;
  *out_bytes = H.out_bytes;  // (0 on a broken chain)
  // the index -- of a broken chain its good prefix, if that fits: the verdict is the walk's either way
  const uint64_t entries = (uint64_t)H.n_members + 1;
  if (member_off && index_cap >= entries) {
    if (P.C.member_off) {
      HIP_TRY(c, hipMemcpyAsync(member_off, P.C.member_off, entries * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(out_off, P.C.out_off, entries * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else {  // (no candidate at all: zero members in front of offset 0)
      member_off[0] = 0, out_off[0] = 0;
    }
  }
  if (H.rc) return H.rc;
  return member_off && index_cap < entries ? FLATE_HIP_E_OUT_TOO_SMALL : FLATE_HIP_OK;
}

int flate_hip_gzip_read(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap,
                        uint64_t *out_len, uint32_t *n_members, uint32_t *bad_member, int64_t *err_off, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = gzip_read_args(in, in_len, out, out_cap, out_len, flags);
  if (rc) return rc;
  c->hip_err.clear();
  *out_len = 0;
  if (n_members) *n_members = 0;
  if (bad_member) *bad_member = 0xffffffffu;
  if (err_off) *err_off = -1;
  if (in_len == 0) return FLATE_HIP_OK;
  try {
    const uint8_t *d_in = nullptr;
    if ((rc = stage_input(c, in, in_len, flags, &d_in))) return rc;
    BgzfHead H{};
    GzipParams P{};
    if ((rc = gzip_discover(c, d_in, in_len, H, P))) return rc;
    const uint32_t n = H.n_members;
    if (n_members) *n_members = n;
    if (H.rc) {  // a broken chain: nothing is decoded, nothing is written
      if (bad_member) *bad_member = n;
      if (err_off) *err_off = H.err_off;
      return H.rc;
    }
    *out_len = H.out_bytes;
    if (H.out_bytes > out_cap) return FLATE_HIP_E_OUT_TOO_SMALL;
    return members_read(c, d_in, n, P.C.member_off, P.C.out_off, H.out_bytes, out, flags, bad_member, err_off);
  } catch (const std::exception &e) {  // (out of host memory in an index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

}  // extern "C"

// ---- one long stream decoded in pieces (Decompressor::read as the reference behaves: the caller
// ---- holds a piece of input and a piece of output, never the whole stream; inflate.mbt:382-407) ----
struct flate_hip_inflate_stream {
  flate_hip_ctx *ctx = nullptr;
  DevBuf state, in, out;
  int status = 0;           // sticky: 1 = the final block is done, < 0 = error
  int64_t err_off = -1;
  uint32_t bit_in_byte = 0; // of the byte the next call's input starts with
  uint64_t total_in = 0, total_out = 0;
};

extern "C" {

int flate_hip_inflate_stream_open(flate_hip_ctx *c, flate_hip_inflate_stream **out) {
  if (!c || !out) return FLATE_HIP_E_INVALID;
  *out = nullptr;
  c->hip_err.clear();
  HIP_TRY(c, hipSetDevice(c->device));
  flate_hip_inflate_stream *st = new flate_hip_inflate_stream();
  st->ctx = c;
  int rc = ensure(c, st->state, inflate_stream_state_bytes() + 64);
  if (rc == FLATE_HIP_OK) {
    hipLaunchKernelGGL(inflate_stream_init_kernel, dim3(1), dim3(64), 0, c->stream, st->state.p,
                       (const uint8_t *)nullptr, 0u);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) rc = FLATE_HIP_E_HIP;
  }
  if (rc != FLATE_HIP_OK) {
    delete st;
    return rc;
  }
  *out = st;
  return FLATE_HIP_OK;
}

// Decompressor::reset(r, dict) (inflate.mbt:862-884) / &Reader::new_dict (:315-317): a fresh decoder on
// the same handle, with the last 32768 bytes of `dict` as history that has already been read
// (DictDecoder::new, dict-decoder.mbt:40-60).
int flate_hip_inflate_stream_reset(flate_hip_inflate_stream *st, const uint8_t *dict, uint64_t dict_len) {
  if (!st || (dict_len && !dict)) return FLATE_HIP_E_INVALID;
  flate_hip_ctx *c = st->ctx;
  c->hip_err.clear();
  HIP_TRY(c, hipSetDevice(c->device));
  if (dict_len > (uint64_t)kMaxMatchOffset) {
    dict += dict_len - (uint64_t)kMaxMatchOffset;
    dict_len = (uint64_t)kMaxMatchOffset;
  }
  int rc;
  if ((rc = ensure(c, st->in, dict_len + 16))) return rc;
  if (dict_len) HIP_TRY(c, hipMemcpyAsync(st->in.p, dict, dict_len, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(inflate_stream_init_kernel, dim3(1), dim3(256), 0, c->stream, st->state.p,
                     (const uint8_t *)st->in.p, (uint32_t)dict_len);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  st->status = 0;
  st->err_off = -1;
  st->bit_in_byte = 0;
  st->total_in = st->total_out = 0;
  return FLATE_HIP_OK;
}

void flate_hip_inflate_stream_free(flate_hip_inflate_stream *st) {
  if (!st) return;
  (void)hipSetDevice(st->ctx->device);
  delete st;
}

int flate_hip_inflate_stream_read(flate_hip_inflate_stream *st, const uint8_t *in, uint64_t in_len, int final_in,
                                  uint8_t *out, uint64_t out_cap, uint64_t *in_used, uint64_t *out_len,
                                  int64_t *err_off) {
  if (!st || !in_used || !out_len || (in_len && !in) || (out_cap && !out)) return FLATE_HIP_E_INVALID;
  *in_used = *out_len = 0;
  if (err_off) *err_off = st->err_off;
  if (st->status) return st->status == 1 ? FLATE_HIP_STREAM_END : st->status;  // sticky (Decompressor.err, inflate.mbt:285,398)
  // the byte that holds the next unconsumed bit was reported as unused: it has to be here again
  if (st->bit_in_byte && in_len == 0) return final_in ? FLATE_HIP_E_UNEXPECTED_EOF : FLATE_HIP_OK;
  if (in_len == 0 && !final_in) return FLATE_HIP_OK;  // nothing to decode from
  flate_hip_ctx *c = st->ctx;
  c->hip_err.clear();
  HIP_TRY(c, hipSetDevice(c->device));
  // one call takes at most 1 GiB each way (32-bit positions inside the kernel); more input than that is
  // simply not all used, and not final
  const uint64_t kPiece = 1ull << 30;
  if (in_len > kPiece) {
    in_len = kPiece;
    final_in = 0;
  }
  if (out_cap > kPiece) out_cap = kPiece;
  int rc;
  if ((rc = ensure(c, st->in, in_len + 16))) return rc;
  if ((rc = ensure(c, st->out, out_cap + 16))) return rc;
  if (in_len) HIP_TRY(c, hipMemcpyAsync(st->in.p, in, in_len, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(inflate_stream_kernel, dim3(1), dim3(64), 0, c->stream, st->state.p, (const uint8_t *)st->in.p,
                     (uint32_t)in_len, final_in ? 1u : 0u, (uint8_t *)st->out.p, (uint32_t)out_cap);
  HIP_TRY(c, hipGetLastError());
  InfStreamResult r{};
  HIP_TRY(c, hipMemcpyAsync(&r, st->state.p, sizeof r, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (r.out_len > out_cap || r.in_used > in_len) return FLATE_HIP_E_INTERNAL;
  if (r.out_len) {
    HIP_TRY(c, hipMemcpyAsync(out, st->out.p, r.out_len, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  *in_used = r.in_used;
  *out_len = r.out_len;
  st->bit_in_byte = r.bit_in_byte;
  st->total_in = r.total_in;
  st->total_out = r.total_out;
  if (r.status) {
    st->status = r.status;
    st->err_off = r.err_off;
    if (err_off) *err_off = r.err_off;
    return r.status == 1 ? FLATE_HIP_STREAM_END : r.status;
  }
  return FLATE_HIP_OK;
}

}  // extern "C"
