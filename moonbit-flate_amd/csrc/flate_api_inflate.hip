// flate_api_inflate.hip -- the decode calls of the C ABI (see include/flate_hip.h): flate_hip_inflate_batch, _batch_dict,
// _batch_framed, _spliced, _spliced_framed and the flate_hip_inflate_stream_* handle.
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

// The route's kernel over the n streams of I, inside the inflate stage's events.  dict: some stream starts from a
// preset dictionary (the dictionary builds).
static int launch_decoders(flate_hip_ctx *c, const InflateRoute &rt, InfParams I, bool dict) {
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
int bgzf_discover(flate_hip_ctx *c, const uint8_t *d_in, uint64_t in_len, BgzfHead &H, BgzfParams &P) {
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
    });
    if (rc) return rc;
    hipLaunchKernelGGL(bgzf_count_kernel, dim3(C.n_tiles), dim3(256), 0, c->stream, P);
    hipLaunchKernelGGL(chain_scan_kernel, dim3(1), dim3(1024), 0, c->stream, C);
    hipLaunchKernelGGL(bgzf_fill_kernel, dim3(C.n_tiles), dim3(256), 0, c->stream, P);
    if ((rc = chain_tail(c, C, bgzf_link_kernel, P, bgzf_finish_kernel, bgzf_out_scan_kernel, P))) return rc;
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
// out[0, out_bytes) comes down once.  Returns the first non-zero member status, with that member's index and offset.
int members_read(flate_hip_ctx *c, const uint8_t *d_in, uint32_t n, const uint64_t *d_member_off,
                 const uint64_t *d_out_off, uint64_t out_bytes, uint8_t *out, uint32_t flags, uint32_t *bad_member,
                 int64_t *err_off) {
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
      return st[i];
    }
  return FLATE_HIP_OK;
}

}  // namespace

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
    const uint64_t windows = (RH.out_total + (uint64_t)kBgzfGatherRangeCost * nr + kBgzfGatherWindow - 1) / kBgzfGatherWindow;
    if (windows > 0x7fffffffull) return FLATE_HIP_E_TOO_LARGE;
    BgzfGatherParams G{};
    G.scratch = d_dense;
    G.out = d_out;
    G.r_out_off = Q.r_out_off;
    G.r_src = Q.r_src;
    G.n_ranges = nr;
    hipLaunchKernelGGL(bgzf_gather_kernel, dim3((uint32_t)windows), dim3(256), 0, c->stream, G);
    HIP_TRY(c, hipGetLastError());
    if (!dev) HIP_TRY(c, hipMemcpyAsync(out, d_out, RH.out_total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));

    // the statuses: nxt[i] = the first selected member at or behind i with a status
    std::vector<uint32_t> nxt((size_t)ns + 1);
    nxt[ns] = ns;
    for (uint32_t i = ns; i-- > 0;) nxt[i] = st[i] ? i : nxt[i + 1];
    if (range_status)
      for (uint32_t r = 0; r < nr; ++r)
        if (!r_status[r] && r_lo[r] < r_hi[r] && r_hi[r] <= ns && nxt[r_lo[r]] < r_hi[r]) range_status[r] = st[nxt[r_lo[r]]];
    if (nxt[0] < ns) {
      const uint32_t i = nxt[0];
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

// ---- one long stream: block discovery (one_kernels.hip, one_probe_kernel.inc) ----
namespace {

// FIND's count pass or fill pass over n_tiles tiles, in the build of P's unit rule (option "one_stored_units")
void one_find_launch(flate_hip_ctx *c, bool count, uint32_t n_tiles, const OneParams &P) {
  if (count && P.stored_units)
    hipLaunchKernelGGL(one_count_kernel<true>, dim3(n_tiles), dim3(256), 0, c->stream, P);
  else if (count)
    hipLaunchKernelGGL(one_count_kernel<false>, dim3(n_tiles), dim3(256), 0, c->stream, P);
  else if (P.stored_units)
    hipLaunchKernelGGL(one_fill_kernel<true>, dim3(n_tiles), dim3(256), 0, c->stream, P);
  else
    hipLaunchKernelGGL(one_fill_kernel<false>, dim3(n_tiles), dim3(256), 0, c->stream, P);
}

// PROBE over n_blocks candidates (or the one tail probe) and TAIL over a round's units, in the build of the unit rule
// their parameters carry -- the same word for both, so they stop at the same bits
void one_probe_launch(flate_hip_ctx *c, uint32_t n_blocks, const OneParams &P, uint32_t tail) {
  if (P.stored_units)
    hipLaunchKernelGGL(one_probe_kernel<true>, dim3(n_blocks), dim3(64), 0, c->stream, P, tail);
  else
    hipLaunchKernelGGL(one_probe_kernel<false>, dim3(n_blocks), dim3(64), 0, c->stream, P, tail);
}
void one_tail_launch(flate_hip_ctx *c, uint32_t n_blocks, const OneDecParams &D) {
  if (D.stored_units)
    hipLaunchKernelGGL(one_tail_kernel<true>, dim3(n_blocks), dim3(64), 0, c->stream, D);
  else
    hipLaunchKernelGGL(one_tail_kernel<false>, dim3(n_blocks), dim3(64), 0, c->stream, D);
}

// The discovery over the ONE stream d_in[0, in_len) (DEVICE memory) on the ctx's stream: the container's header, count
// and scan, ONE read-back of the candidate count (the launches behind it have a thread or a wavefront per candidate),
// then fill, probe, link, rounds, finish, out-scan, the tail probe and ONE read-back of the result words H with the
// index (P.C.member_off / P.C.out_off on the device; null when the header is bad).  Counted in no
// profiling stage.
// index_cap != 0: the first min(index_cap, candidates + 1) entries of unit_bit / out_off come back into `index` (the
// two arrays one after the other) in the same read-back as H -- the units are a subset of the candidates, so what fits
// the caller's arrays is known before the chain is.
int one_discover(flate_hip_ctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t wrap, uint64_t index_cap, OneHead &H,
                 OneParams &P, std::vector<uint64_t> &index) {
  int rc;
  P = OneParams{};
  ChainParams &C = P.C;
  C.in = d_in;
  C.in_len = in_len;
  P.unit_max = c->one_unit_max;
  P.stored_units = c->one_stored_units;
  if ((rc = tiles_for(d_in, 0, in_len, &C.n_tiles))) return rc;
  rc = carve(c, c->d_one_tiles, [&](Carve &k) {
    k.take(P.head, 1);
    k.take(P.one, 1);
    k.take(C.tile_cnt, (size_t)C.n_tiles + 1);
  });
  if (rc) return rc;
  C.head = &P.head->h;
  hipLaunchKernelGGL(one_init_kernel, dim3(1), dim3(64), 0, c->stream, P.one, in_len);
  if (wrap != FLATE_HIP_WRAP_RAW) {  // the header rules of flate_hip_inflate_spliced_framed (no dictionaries: FDICT is bad)
    FrameReadParams R{};
    R.in = d_in;
    R.in_off = P.one->in_off;
    R.n_streams = 1;
    R.wrap = wrap;
    R.pay_off = P.one->pay_off;
    R.pay_end = &P.one->pay_end;
    R.want = &P.one->want;
    R.isize = &P.one->isize;
    R.bad = &P.one->bad;
    R.dict_used = &P.one->dict_used;
    hipLaunchKernelGGL(frame_parse_kernel, dim3(1), dim3(256), 0, c->stream, R);
  }
  one_find_launch(c, true, C.n_tiles, P);
  hipLaunchKernelGGL(chain_scan_kernel, dim3(1), dim3(1024), 0, c->stream, C);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&H, P.head, sizeof H, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t cap = H.h.n_cand;
  if ((rc = chain_size(C, cap))) return rc;  // (the count saturates at 2^32 - 1)
  if (cap == 0) return FLATE_HIP_OK;  // (a bad header: the scan kernel has left FLATE_HIP_E_CORRUPT at offset 0)

  const size_t n = cap;
  rc = carve(c, c->d_one, [&](Carve &k) {
    k.take(C.cand_off, n);
    k.take(P.probe, n);
    k.take(C.jump[0], n + 2);
    k.take(C.jump[1], n + 2);
    k.take(C.path, C.path_len);
    k.take(P.usize, n);
    k.take(C.member_off, n + 1);
    k.take(C.out_off, n + 1);
  });
  if (rc) return rc;
  one_find_launch(c, false, C.n_tiles, P);
  one_probe_launch(c, cap, P, 0u);
  if ((rc = chain_tail(c, C, one_link_kernel, P, one_finish_kernel, one_out_scan_kernel, P))) return rc;
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

// TAIL, COMPOSE and RESOLVE of the round D.u0 .. D.u0 + D.count - 1 of consecutive units: the windows R[1 .. count]
// from the seed R[0] (flate_hip_inflate_one and the build of the seek index run exactly these launches).
void one_round_windows(flate_hip_ctx *c, const OneDecParams &D) {
  const uint32_t entry_blocks = (uint32_t)(((uint64_t)D.count * kWinEntries + 255) / 256);
  one_tail_launch(c, D.count, D);
  int cur = 0;
  for (uint32_t s = 1; s < D.count; s <<= 1, cur ^= 1)
    hipLaunchKernelGGL(one_compose_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.F[cur ^ 1], D.count, s);
  hipLaunchKernelGGL(one_resolve_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.R, D.count);
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
    uint8_t *d_out = out;
    if (!dev) {
      if ((rc = ensure(c, c->d_out, total + 16))) return rc;
      d_out = (uint8_t *)c->d_out.p;
    }
    const uint32_t per_round = n_dec < c->one_round_units ? (n_dec ? n_dec : 1u) : c->one_round_units;
    const size_t fentries = (size_t)per_round * kWinEntries;
    OneDecParams D{};
    uint32_t *d_sum;
    int32_t *d_ds;
    uint64_t *d_dl;
    int64_t *d_de;
    rc = carve(c, c->d_one_dec, [&](Carve &k) {
      k.take(D.dh, 1);
      k.take(d_sum, 4);
      k.take(D.F[0], fentries);
      k.take(D.F[1], fentries);
      k.take(D.R, ((size_t)per_round + 1) * kWinEntries);
      k.take(D.status, (size_t)n_dec + 1);
      k.take(D.err_off, (size_t)n_dec + 1);
      k.take(D.produced, (size_t)n_dec + 1);
      k.take(D.p_out_off, (size_t)per_round + 1);
      k.take(D.p_dict_at, per_round);
      k.take(D.p_dict_len, per_round);
      k.take(d_ds, per_round);
      k.take(d_dl, per_round);
      k.take(d_de, per_round);
    });
    if (rc) return rc;
    D.in = d_in;
    D.one = P.one;
    D.unit_bit = P.C.member_off;
    D.out_off = P.C.out_off;
    D.total = total;
    D.unit_max = P.unit_max;
    D.stored_units = P.stored_units;
    D.d_status = d_ds;
    D.d_out_len = d_dl;
    D.head = P.head;
    D.wrap = wrap;
    D.in_len = in_len;
    HIP_TRY(c, hipMemsetAsync(D.dh, 0xff, sizeof(OneDecHead), c->stream));  // first_bad, decode_bad: none
    HIP_TRY(c, hipMemsetAsync(D.R, 0, kWinEntries, c->stream));            // in front of the stream: zeros
    bool used[FLATE_HIP_STAGE_COUNT] = {false, false, false, false};
    for (uint32_t u0 = 0; u0 < n_dec; u0 += per_round) {
      D.u0 = u0;
      D.count = n_dec - u0 < per_round ? n_dec - u0 : per_round;
      const uint32_t unit_blocks = (D.count + 1u + 255u) / 256u;
      one_round_windows(c, D);
      // DECODE: the round's units as spliced pieces with dictionaries, through the lane-per-stream decoder.  The
      // stream's last piece runs to BFINAL (or to its failure); every other round's last piece ends where the next
      // unit starts, and so does the last unit of a chain that stopped at a header the decoder refuses.
      hipLaunchKernelGGL(one_pieces_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, D);
      InfParams I{};
      I.in = d_in + H.raw_off;
      I.in_len = H.raw_len;
      I.bit_off = D.unit_bit + u0;
      I.closed = (u0 + D.count < n_dec || (H.h.rc != 0 && !H.fail_unit)) ? 1u : 0u;
      I.n_streams = D.count;
      I.out = d_out;
      I.out_off = D.p_out_off;
      I.out_len = d_dl;
      I.status = d_ds;
      I.err_off = d_de;
      I.dict_buf = D.R;
      I.dict_at = D.p_dict_at;
      I.dict_len = D.p_dict_len;
      if ((rc = launch_decoders(c, inflate_route_units(c->inflate, c->num_cus, D.count), I, true))) return rc;  // (of several rounds the stage's time is the last one's)
      hipLaunchKernelGGL(one_check_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, D);
      used[FLATE_HIP_STAGE_INFLATE] = true;
      HIP_TRY(c, hipGetLastError());
      // the window behind the round's last unit seeds the next round
      if (u0 + D.count < n_dec)
        HIP_TRY(c, hipMemcpyAsync(D.R, D.R + (size_t)D.count * kWinEntries, kWinEntries, hipMemcpyDeviceToDevice, c->stream));
    }
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
    if (R.out_len > total) return FLATE_HIP_E_INTERNAL;
    *out_len = R.out_len;
    if (!dev && R.out_len) {  // the result comes down once
      HIP_TRY(c, hipMemcpyAsync(out, d_out, R.out_len, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
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
    const uint32_t per_round = n_dec < c->one_round_units ? (n_dec ? n_dec : 1u) : c->one_round_units;

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
    rc = carve(c, c->d_one_dec, [&](Carve &k) {
      k.take(D.dh, 1);
      k.take(D.F[0], (size_t)per_round * kWinEntries);
      k.take(D.F[1], (size_t)per_round * kWinEntries);
      k.take(D.R, ((size_t)per_round + 1) * kWinEntries);
      k.take(D.status, (size_t)n_dec + 1);
      k.take(D.err_off, (size_t)n_dec + 1);
      k.take(D.produced, (size_t)n_dec + 1);
    });
    if (rc) return rc;
    D.in = d_in;
    D.one = P.one;
    D.unit_bit = P.C.member_off;
    D.out_off = P.C.out_off;
    D.unit_max = P.unit_max;
    D.stored_units = P.stored_units;
    HIP_TRY(c, hipMemsetAsync(D.dh, 0xff, sizeof(OneDecHead), c->stream));  // first_bad: none
    HIP_TRY(c, hipMemsetAsync(D.R, 0, kWinEntries, c->stream));            // in front of the stream: zeros
    uint32_t p_next = 1;  // the first point whose window is not packed yet (point 0 has none)
    for (uint32_t u0 = 0; u0 < n_dec; u0 += per_round) {
      D.u0 = u0;
      D.count = n_dec - u0 < per_round ? n_dec - u0 : per_round;
      one_round_windows(c, D);
      // PACK: R[i] of the round's point units -> their blocks, which lie one behind the other in `windows`
      uint32_t p_hi = p_next;
      while (p_hi < np && points[p_hi] < (uint64_t)u0 + D.count) ++p_hi;
      if (p_hi > p_next) {
        const uint32_t cnt = p_hi - p_next;
        hipLaunchKernelGGL(one_seek_pack_kernel, dim3((cnt + 1u + 255u) / 256u), dim3(256), 0, c->stream, PP.point_unit,
                           p_next, cnt, u0, d_r_out_off, d_r_src);
        BgzfGatherParams G{};
        G.scratch = D.R;  // (R[count] lies behind the last run: the 32 bytes the gather may touch)
        G.out = d_windows + (uint64_t)(p_next - 1u) * kSeekWindow;
        G.r_out_off = d_r_out_off;
        G.r_src = d_r_src;
        G.n_ranges = cnt;
        const uint64_t pieces = ((uint64_t)cnt * (kSeekWindow + kBgzfGatherRangeCost) + kBgzfGatherWindow - 1) / kBgzfGatherWindow;
        hipLaunchKernelGGL(bgzf_gather_kernel, dim3((uint32_t)pieces), dim3(256), 0, c->stream, G);
        p_next = p_hi;
      }
      HIP_TRY(c, hipGetLastError());
      if (u0 + D.count < n_dec)
        HIP_TRY(c, hipMemcpyAsync(D.R, D.R + (size_t)D.count * kWinEntries, kWinEntries, hipMemcpyDeviceToDevice, c->stream));
    }
    OneDecHead R{};
    HIP_TRY(c, hipMemcpyAsync(&R, D.dh, sizeof R, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (R.first_bad != 0xffffffffu) {  // TAIL's verdict: the serial decoder's, at the serial offset
      if (R.first_bad >= n_dec) return FLATE_HIP_E_INTERNAL;
      int32_t st = 0;
      int64_t eo = -1;
      HIP_TRY(c, hipMemcpyAsync(&st, D.status + R.first_bad, 4, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(&eo, D.err_off + R.first_bad, 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      return verdict(st ? st : FLATE_HIP_E_INTERNAL, eo);
    }
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

// Random access through the seek index: locate, select, layout (one_seek_kernels.hip), ONE read-back (the parsed
// container, the ranges' layout, the unit list), rounds of TAIL / segmented scan / DECODE over the list into a dense
// scratch, the per-unit check, the gather.
int flate_hip_inflate_one_ranges(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t wrap, const uint64_t *index,
                                 uint64_t index_words, const uint8_t *windows, uint64_t windows_bytes, const uint64_t *begin,
                                 const uint64_t *end, uint32_t n_ranges, uint8_t *out, uint64_t out_cap, uint64_t *out_off,
                                 int32_t *range_status, uint32_t *n_decoded, uint32_t *bad_unit, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = one_ranges_args(in, in_len, wrap, index, index_words, windows, windows_bytes, begin, end, n_ranges, out, out_cap,
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
    hipLaunchKernelGGL(one_init_kernel, dim3(1), dim3(64), 0, c->stream, d_one, in_len);
    if (wrap != FLATE_HIP_WRAP_RAW) {
      FrameReadParams R{};
      R.in = d_in;
      R.in_off = d_one->in_off;
      R.n_streams = 1;
      R.wrap = wrap;
      R.pay_off = d_one->pay_off;
      R.pay_end = &d_one->pay_end;
      R.want = &d_one->want;
      R.isize = &d_one->isize;
      R.bad = &d_one->bad;
      R.dict_used = &d_one->dict_used;
      hipLaunchKernelGGL(frame_parse_kernel, dim3(1), dim3(256), 0, c->stream, R);
    }
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

    // the windows: the caller's device buffer, or the blocks of the selected points uploaded into a staged copy
    const uint8_t *d_windows = windows;
    if (!dev && windows_bytes) {
      if ((rc = ensure(c, c->d_one_seek_win, windows_bytes + 16))) return rc;
      uint8_t *stage = (uint8_t *)c->d_one_seek_win.p;
      d_windows = stage;
      std::vector<uint32_t> ps;  // the selected points behind point 0, rising
      uint32_t p = 1;
      for (uint32_t i = 0; i < ns && p < np; ++i) {
        while (p < np && h_point[p] < sel[i]) ++p;
        if (p < np && h_point[p] == sel[i]) ps.push_back(p);
      }
      for (size_t a = 0; a < ps.size();) {  // neighbours in the index travel as one copy
        size_t b = a + 1;
        while (b < ps.size() && ps[b] == ps[b - 1] + 1u) ++b;
        const uint64_t at = (uint64_t)(ps[a] - 1u) * kSeekWindow, len = (uint64_t)(b - a) * kSeekWindow;
        HIP_TRY(c, hipMemcpyAsync(stage + at, windows + at, len, hipMemcpyHostToDevice, c->stream));
        a = b;
      }
    }

    const uint32_t per_round = ns < c->one_round_units ? ns : c->one_round_units;
    const size_t fentries = (size_t)per_round * kWinEntries;
    OneDecParams D{};
    OneSeekRoundParams S{};
    int32_t *d_ds;
    uint64_t *d_dl;
    int64_t *d_de;
    rc = carve(c, c->d_one_dec, [&](Carve &k) {
      k.take(D.dh, 1);
      k.take(D.F[0], fentries);
      k.take(D.F[1], fentries);
      k.take(D.R, ((size_t)per_round + 1) * kWinEntries);
      k.take(D.status, (size_t)ns + 1);
      k.take(D.err_off, (size_t)ns + 1);
      k.take(D.produced, (size_t)ns + 1);
      k.take(S.seed, per_round);
      k.take(S.p_bit_off, per_round);
      k.take(S.p_bit_end, per_round);
      k.take(S.p_dict_at, per_round);
      k.take(S.p_dict_len, per_round);
      k.take(d_ds, per_round);
      k.take(d_dl, per_round);
      k.take(d_de, per_round);
      k.take(S.u_status, ns);
    });
    if (rc) return rc;
    if ((rc = ensure(c, c->d_one_seek_dense, RH.scratch_total + 64))) return rc;
    uint8_t *d_dense = (uint8_t *)c->d_one_seek_dense.p;
    uint8_t *d_out = out;
    if (!dev) {
      if ((rc = ensure(c, c->d_out, RH.out_total + 16))) return rc;
      d_out = (uint8_t *)c->d_out.p;
    }
    D.in = d_in;
    D.one = d_one;
    D.unit_bit = Q.unit_bit;
    D.out_off = Q.out_off;
    D.unit_max = c->one_unit_max;
    D.stored_units = index[kSeekRuleAt] == kSeekRuleStored ? 1u : 0u;  // the index's rule, not the context's option
    D.unit_list = Q.sel_unit;
    S.Q = Q;
    S.windows = d_windows;
    S.R = D.R;
    S.d_status = d_ds;
    S.d_out_len = d_dl;
    HIP_TRY(c, hipMemsetAsync(D.dh, 0xff, sizeof(OneDecHead), c->stream));
    bool used[FLATE_HIP_STAGE_COUNT] = {false, false, false, false};
    for (uint32_t i0 = 0; i0 < ns; i0 += per_round) {
      const uint32_t count = ns - i0 < per_round ? ns - i0 : per_round;
      D.u0 = S.i0 = i0;
      D.count = S.count = count;
      const uint32_t entry_blocks = (uint32_t)(((uint64_t)count * kWinEntries + 255) / 256);
      const uint32_t unit_blocks = (count + 255u) / 256u;
      hipLaunchKernelGGL(one_seek_seed_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, S);
      hipLaunchKernelGGL(one_seek_load_kernel, dim3((entry_blocks + 15u) / 16u), dim3(256), 0, c->stream, S);
      one_tail_launch(c, count, D);
      int cur = 0;
      for (uint32_t s = 1; s < count; s <<= 1, cur ^= 1)
        hipLaunchKernelGGL(one_seek_compose_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.F[cur ^ 1],
                           S.seed, count, s);
      hipLaunchKernelGGL(one_seek_resolve_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.R, S.seed, count);
      // DECODE: the round's units as spliced pieces with dictionaries, each with its own end, into their dense slots
      InfParams I{};
      I.in = d_in + raw_off;
      I.in_len = raw_end - raw_off;
      I.bit_off = S.p_bit_off;
      I.bit_end = S.p_bit_end;
      I.n_streams = count;
      I.out = d_dense;
      I.out_off = Q.sel_at + i0;
      I.out_len = d_dl;
      I.status = d_ds;
      I.err_off = d_de;
      I.dict_buf = D.R;
      I.dict_at = S.p_dict_at;
      I.dict_len = S.p_dict_len;
      if ((rc = launch_decoders(c, inflate_route_units(c->inflate, c->num_cus, count), I, true))) return rc;
      used[FLATE_HIP_STAGE_INFLATE] = true;
      hipLaunchKernelGGL(one_seek_check_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, S);
      HIP_TRY(c, hipGetLastError());
      // the window behind the round's last unit is the carried seed of a segment that continues
      if (i0 + count < ns)
        HIP_TRY(c, hipMemcpyAsync(D.R, D.R + (size_t)count * kWinEntries, kWinEntries, hipMemcpyDeviceToDevice, c->stream));
    }

    // the gather: every range's run of the scratch to its place in out
    const uint64_t pieces = (RH.out_total + (uint64_t)kBgzfGatherRangeCost * nr + kBgzfGatherWindow - 1) / kBgzfGatherWindow;
    if (pieces > 0x7fffffffull) return FLATE_HIP_E_TOO_LARGE;
    BgzfGatherParams G{};
    G.scratch = d_dense;
    G.out = d_out;
    G.r_out_off = Q.r_out_off;
    G.r_src = Q.r_src;
    G.n_ranges = nr;
    hipLaunchKernelGGL(bgzf_gather_kernel, dim3((uint32_t)pieces), dim3(256), 0, c->stream, G);
    HIP_TRY(c, hipGetLastError());
    std::vector<int32_t> st(ns);
    HIP_TRY(c, hipMemcpyAsync(st.data(), S.u_status, (size_t)ns * 4, hipMemcpyDeviceToHost, c->stream));
    if (!dev) HIP_TRY(c, hipMemcpyAsync(out, d_out, RH.out_total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->profiling && (rc = collect_timing(c, used))) return rc;

    // the statuses: nxt[i] = the first decoded unit at or behind place i with a status
    std::vector<uint32_t> nxt((size_t)ns + 1);
    nxt[ns] = ns;
    for (uint32_t i = ns; i-- > 0;) nxt[i] = st[i] ? i : nxt[i + 1];
    if (range_status)
      for (uint32_t r = 0; r < nr; ++r)
        if (r_lo[r] < r_hi[r] && r_hi[r] <= ns && nxt[r_lo[r]] < r_hi[r]) range_status[r] = st[nxt[r_lo[r]]];
    if (nxt[0] < ns) {
      if (bad_unit) *bad_unit = sel[nxt[0]];
      return st[nxt[0]];
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

// The discovery over the file d_in[0, in_len) (DEVICE memory, in_len != 0) on the ctx's stream: the two count passes
// and their scans, ONE read-back of the two candidate counts, then the fills, the B nodes' bits, the probe of every
// node, link, rounds, finish, out-scan, the member scan, the tail probe, the member words and ONE read-back of the
// result words H / G -- with member_out (the members' places in the output, n_b + 2 entries of which G.n_members + 1
// count) when `mout` is given.  The index stays on the device (P).  Counted in no profiling stage.
int gzfile_discover(flate_hip_ctx *c, const uint8_t *d_in, uint64_t in_len, OneHead &H, GzFileHead &G, GzFileParams &P,
                    std::vector<uint64_t> *mout) {
  int rc;
  P = GzFileParams{};
  OneParams PA{};
  GzipParams PB{};
  ChainParams &C = P.O.C;
  uint32_t n_tiles = 0;
  if ((rc = tiles_for(d_in, 0, in_len, &n_tiles))) return rc;
  OneHead *head_a;
  BgzfHead *head_b;
  rc = carve(c, c->d_gzfile_tiles, [&](Carve &k) {
    k.take(P.O.head, 1);
    k.take(P.gh, 1);
    k.take(P.O.one, 1);
    k.take(head_a, 1);
    k.take(head_b, 1);
    k.take(PA.C.tile_cnt, (size_t)n_tiles + 1);
    k.take(PB.C.tile_cnt, (size_t)n_tiles + 1);
  });
  if (rc) return rc;
  C.in = PA.C.in = PB.C.in = d_in;
  C.in_len = PA.C.in_len = PB.C.in_len = in_len;
  C.n_tiles = PA.C.n_tiles = PB.C.n_tiles = n_tiles;
  C.head = &P.O.head->h;
  P.O.unit_max = PA.unit_max = c->one_unit_max;
  P.O.stored_units = PA.stored_units = c->one_stored_units;
  PA.C.head = &head_a->h;
  PA.head = head_a;
  PA.one = P.O.one;
  PB.C.head = head_b;
  PB.member_max = ~0ull;  // a member's range is never clipped
  hipLaunchKernelGGL(gzfile_init_kernel, dim3(1), dim3(64), 0, c->stream, P.O.one, in_len);
  one_find_launch(c, true, n_tiles, PA);
  hipLaunchKernelGGL(chain_scan_kernel, dim3(1), dim3(1024), 0, c->stream, PA.C);
  hipLaunchKernelGGL(gzip_count_kernel, dim3(n_tiles), dim3(256), 0, c->stream, PB);
  hipLaunchKernelGGL(chain_scan_kernel, dim3(1), dim3(1024), 0, c->stream, PB.C);
  HIP_TRY(c, hipGetLastError());
  OneHead HA{};
  BgzfHead HB{};
  HIP_TRY(c, hipMemcpyAsync(&HA, head_a, sizeof HA, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&HB, head_b, sizeof HB, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t na = HA.h.n_cand, nb = HB.n_cand;
  if ((uint64_t)na + nb > 0x7ffffff0ull) return FLATE_HIP_E_TOO_LARGE;  // (the counts saturate at 2^32 - 1)
  const uint32_t cap = na + nb;
  if ((rc = chain_size(C, cap)) || (rc = chain_size(PA.C, na)) || (rc = chain_size(PB.C, nb))) return rc;
  P.n_a = na;
  P.n_b = nb;

  const size_t n = cap;
  uint64_t *hdr_off;
  rc = carve(c, c->d_gzfile, [&](Carve &k) {
    k.take(C.cand_off, n);
    k.take(hdr_off, (size_t)nb + 1);
    k.take(PB.cand_end, nb);
    k.take(P.O.probe, n);
    k.take(C.jump[0], n + 2);
    k.take(C.jump[1], n + 2);
    k.take(C.path, C.path_len);
    k.take(P.O.usize, n);
    k.take(C.member_off, n + 1);
    k.take(C.out_off, n + 1);
    k.take(P.u_start, n + 1);
    k.take(P.u_final, n);
    k.take(P.u_member, n + 1);
    k.take(P.rel_off, n + 1);
    k.take(P.member_off, (size_t)nb + 2);
    k.take(P.member_unit, (size_t)nb + 2);
    k.take(P.member_out, (size_t)nb + 2);
  });
  if (rc) return rc;
  PA.C.cand_off = C.cand_off;
  PB.C.cand_off = hdr_off;
  P.hdr_off = hdr_off;
  one_find_launch(c, false, n_tiles, PA);
  if (nb) {
    hipLaunchKernelGGL(gzip_fill_kernel, dim3(n_tiles), dim3(256), 0, c->stream, PB);
    hipLaunchKernelGGL(gzfile_bits_kernel, dim3((nb + 255) / 256), dim3(256), 0, c->stream, P);
  }
  if (cap) one_probe_launch(c, cap, P.O, 0u);
  const uint32_t node_blocks = (uint32_t)(((uint64_t)cap + 2 + 255) / 256);
  hipLaunchKernelGGL(gzfile_link_kernel, dim3(node_blocks), dim3(256), 0, c->stream, P);
  for (uint32_t j = 0; (1u << j) < C.path_len; ++j)
    hipLaunchKernelGGL(chain_round_kernel, dim3(node_blocks), dim3(256), 0, c->stream, C, j);
  hipLaunchKernelGGL(gzfile_finish_kernel, dim3((C.path_len + 255) / 256), dim3(256), 0, c->stream, P);
  hipLaunchKernelGGL(one_out_scan_kernel, dim3(1), dim3(1024), 0, c->stream, P.O);
  hipLaunchKernelGGL(gzfile_members_kernel, dim3(1), dim3(1024), 0, c->stream, P);
  one_probe_launch(c, 1, P.O, 1u);
  hipLaunchKernelGGL(gzfile_rel_kernel, dim3(node_blocks), dim3(256), 0, c->stream, P);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&H, P.O.head, sizeof H, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&G, P.gh, sizeof G, hipMemcpyDeviceToHost, c->stream));
  if (mout) {
    mout->assign((size_t)nb + 2, 0);
    HIP_TRY(c, hipMemcpyAsync(mout->data(), P.member_out, ((size_t)nb + 2) * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (G.n_members > nb || H.h.n_members > cap) return FLATE_HIP_E_INTERNAL;
  return FLATE_HIP_OK;
}

// The same discovery with the option "gzfile_serial_max" (S >= 1; gzfile_serial_rule.h, gzfile_serial_kernels.hip).
// PHASE 1 over List B alone: count, scan, a read-back of the B count, fill, the serial ranges, ONE size-only launch of
// the batch decoders over all B candidates, the whole test with the hop links, pointer doubling over those links, and
// a read-back of find_from.  PHASE 2, only when find_from < in_len: FIND over in[find_from, in_len) -- the pass runs on
// d_in + find_from with a FrameOne of its own, and one small kernel moves its bits to the file's origin -- and the
// read-back of its count.  PROBE runs over all nodes; a whole B node is parked at the raw stream's end for it and gets
// its phase-1 record back behind it.  Link, rounds, finish, the scans and the rel kernel are gzfile_discover's.  SH =
// find_from and the whole members among the good units; S = their batch, on the device.
int gzfile_discover_serial(flate_hip_ctx *c, const uint8_t *d_in, uint64_t in_len, OneHead &H, GzFileHead &G,
                           GzFileParams &P, GzSerialParams &S, GzSerialHead &SH, std::vector<uint64_t> *mout) {
  int rc;
  P = GzFileParams{};
  S = GzSerialParams{};
  SH = GzSerialHead{};
  OneParams PA{};
  GzipParams PB{};
  ChainParams &C = P.O.C;
  uint32_t n_tiles = 0;
  if ((rc = tiles_for(d_in, 0, in_len, &n_tiles))) return rc;
  OneHead *head_a;
  BgzfHead *head_b;
  FrameOne *one_a;
  rc = carve(c, c->d_gzfile_tiles, [&](Carve &k) {
    k.take(P.O.head, 1);
    k.take(P.gh, 1);
    k.take(P.O.one, 1);
    k.take(head_a, 1);
    k.take(head_b, 1);
    k.take(one_a, 1);
    k.take(S.head, 1);
    k.take(PA.C.tile_cnt, (size_t)n_tiles + 2);  // (a suffix at another alignment: at most one tile more)
    k.take(PB.C.tile_cnt, (size_t)n_tiles + 1);
  });
  if (rc) return rc;
  C.in = PB.C.in = d_in;
  C.in_len = PB.C.in_len = in_len;
  C.n_tiles = PB.C.n_tiles = n_tiles;
  C.head = &P.O.head->h;
  P.O.unit_max = PA.unit_max = c->one_unit_max;
  P.O.stored_units = PA.stored_units = c->one_stored_units;
  PB.C.head = head_b;
  PB.member_max = ~0ull;  // a member's range is never clipped
  hipLaunchKernelGGL(gzfile_init_kernel, dim3(1), dim3(64), 0, c->stream, P.O.one, in_len);
  hipLaunchKernelGGL(gzip_count_kernel, dim3(n_tiles), dim3(256), 0, c->stream, PB);
  hipLaunchKernelGGL(chain_scan_kernel, dim3(1), dim3(1024), 0, c->stream, PB.C);
  HIP_TRY(c, hipGetLastError());
  BgzfHead HB{};
  HIP_TRY(c, hipMemcpyAsync(&HB, head_b, sizeof HB, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t nb = HB.n_cand;
  if (nb > 0x7ffffff0u) return FLATE_HIP_E_TOO_LARGE;  // (the count saturates at 2^32 - 1)
  if ((rc = chain_size(PB.C, nb))) return rc;

  // PHASE 1
  uint64_t *hdr_off;
  InfParams I{};  // size-only: no output buffer, no slots
  rc = carve(c, c->d_gzfile_serial, [&](Carve &k) {
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
  S.serial_max = c->gzfile_serial_max;
  S.n_b = nb;
  S.hdr_off = hdr_off;
  S.status = I.status;
  S.out_len = I.out_len;
  S.used = I.used;
  uint64_t find_from = in_len;  // (no candidate: no member at offset 0, nothing to search)
  if (nb) {
    const uint32_t b_blocks = (nb + 255u) / 256u, w_blocks = (uint32_t)(((uint64_t)nb + 2 + 255) / 256);
    // every range is at most S < 2^28 bytes: the sub-block decoder at any batch size, or -- switched off -- the scalar
    // walk; both report `used`
    const uint64_t longest = in_len < S.serial_max ? in_len : S.serial_max;
    const InflateRoute route = inflate_route(c->inflate, c->num_cus, nb, longest, false, true);
    if (route.decoder == kDecodeSimt) {
      c->hip_err = "gzfile discovery: a size-only pass was routed to the lane-per-stream decoder";
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
    hipLaunchKernelGGL(gzfile_serial_nodes_kernel, dim3(w_blocks), dim3(256), 0, c->stream, S);
    int cur = 0;
    for (uint64_t s = 1; s < (uint64_t)nb + 2; s <<= 1, cur ^= 1)
      hipLaunchKernelGGL(gzfile_serial_round_kernel, dim3(w_blocks), dim3(256), 0, c->stream, S.jump[cur], S.jump[cur ^ 1],
                         nb + 2u);
    hipLaunchKernelGGL(gzfile_serial_from_kernel, dim3(1), dim3(64), 0, c->stream, S, S.jump[cur]);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&SH, S.head, sizeof SH, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    find_from = SH.find_from;
    if (find_from > in_len) return FLATE_HIP_E_INTERNAL;
  } else {
    SH.find_from = in_len;
    HIP_TRY(c, hipMemcpyAsync(S.head, &SH, sizeof SH, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (SH is the caller's: the copy has read it)
  }

  // PHASE 2: FIND over the bytes from find_from on
  uint32_t na = 0, n_tiles_a = 0;
  if (find_from < in_len) {
    const uint8_t *a_in = d_in + find_from;
    const uint64_t a_len = in_len - find_from;
    if ((rc = tiles_for(a_in, 0, a_len, &n_tiles_a))) return rc;
    if (n_tiles_a > n_tiles + 1u) return FLATE_HIP_E_INTERNAL;
    PA.C.in = a_in;
    PA.C.in_len = a_len;
    PA.C.n_tiles = n_tiles_a;
    PA.C.head = &head_a->h;
    PA.head = head_a;
    PA.one = one_a;
    hipLaunchKernelGGL(gzfile_init_kernel, dim3(1), dim3(64), 0, c->stream, one_a, a_len);
    one_find_launch(c, true, n_tiles_a, PA);
    hipLaunchKernelGGL(chain_scan_kernel, dim3(1), dim3(1024), 0, c->stream, PA.C);
    HIP_TRY(c, hipGetLastError());
    OneHead HA{};
    HIP_TRY(c, hipMemcpyAsync(&HA, head_a, sizeof HA, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    na = HA.h.n_cand;
  }
  if ((uint64_t)na + nb > 0x7ffffff0ull) return FLATE_HIP_E_TOO_LARGE;
  const uint32_t cap = na + nb;
  if ((rc = chain_size(C, cap)) || (rc = chain_size(PA.C, na))) return rc;
  P.n_a = S.n_a = na;

  const size_t n = cap;
  rc = carve(c, c->d_gzfile, [&](Carve &k) {
    k.take(C.cand_off, n);
    k.take(P.O.probe, n);
    k.take(C.jump[0], n + 2);
    k.take(C.jump[1], n + 2);
    k.take(C.path, C.path_len);
    k.take(P.O.usize, n);
    k.take(C.member_off, n + 1);
    k.take(C.out_off, n + 1);
    k.take(P.u_start, n + 1);
    k.take(P.u_final, n);
    k.take(P.u_member, n + 1);
    k.take(P.rel_off, n + 1);
    k.take(P.member_off, (size_t)nb + 2);
    k.take(P.member_unit, (size_t)nb + 2);
    k.take(P.member_out, (size_t)nb + 2);
  });
  if (rc) return rc;
  rc = carve(c, c->d_gzfile_serial_units, [&](Carve &k) {
    k.take(S.u_whole, n + 1);
    k.take(S.u_end, n + 1);
  });
  if (rc) return rc;
  PA.C.cand_off = C.cand_off;
  if (find_from < in_len) {
    one_find_launch(c, false, n_tiles_a, PA);
    if (na) hipLaunchKernelGGL(gzfile_serial_base_kernel, dim3((na + 255u) / 256u), dim3(256), 0, c->stream, C.cand_off, na, 8u * find_from);
  }
  if (nb) hipLaunchKernelGGL(gzfile_serial_bits_kernel, dim3((nb + 255) / 256), dim3(256), 0, c->stream, P, S);
  if (cap) one_probe_launch(c, cap, P.O, 0u);
  if (nb) hipLaunchKernelGGL(gzfile_serial_keep_kernel, dim3((nb + 255) / 256), dim3(256), 0, c->stream, P, S);
  const uint32_t node_blocks = (uint32_t)(((uint64_t)cap + 2 + 255) / 256);
  hipLaunchKernelGGL(gzfile_link_kernel, dim3(node_blocks), dim3(256), 0, c->stream, P);
  for (uint32_t j = 0; (1u << j) < C.path_len; ++j)
    hipLaunchKernelGGL(chain_round_kernel, dim3(node_blocks), dim3(256), 0, c->stream, C, j);
  hipLaunchKernelGGL(gzfile_finish_kernel, dim3((C.path_len + 255) / 256), dim3(256), 0, c->stream, P);
  hipLaunchKernelGGL(gzfile_serial_marks_kernel, dim3(node_blocks), dim3(256), 0, c->stream, P, S);
  hipLaunchKernelGGL(one_out_scan_kernel, dim3(1), dim3(1024), 0, c->stream, P.O);
  hipLaunchKernelGGL(gzfile_members_kernel, dim3(1), dim3(1024), 0, c->stream, P);
  one_probe_launch(c, 1, P.O, 1u);
  hipLaunchKernelGGL(gzfile_rel_kernel, dim3(node_blocks), dim3(256), 0, c->stream, P);
  hipLaunchKernelGGL(gzfile_serial_list_kernel, dim3(1), dim3(1024), 0, c->stream, P, S);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&H, P.O.head, sizeof H, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&G, P.gh, sizeof G, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&SH, S.head, sizeof SH, hipMemcpyDeviceToHost, c->stream));
  if (mout) {
    mout->assign((size_t)nb + 2, 0);
    HIP_TRY(c, hipMemcpyAsync(mout->data(), P.member_out, ((size_t)nb + 2) * 8, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (G.n_members > nb || H.h.n_members > cap || SH.n_whole > nb || SH.n_whole > G.n_members || SH.find_from != find_from)
    return FLATE_HIP_E_INTERNAL;
  return FLATE_HIP_OK;
}

// the discovery of flate_hip_gzfile_index / _read by the ctx's option, and what flate_hip_gzfile_last_route reports
int gzfile_discover_routed(flate_hip_ctx *c, const uint8_t *d_in, uint64_t in_len, OneHead &H, GzFileHead &G,
                           GzFileParams &P, GzSerialParams &S, GzSerialHead &SH, std::vector<uint64_t> *mout) {
  c->gzfile_route[0] = c->gzfile_route[1] = 0;
  c->gzfile_route_from = 0;
  int rc;
  if (!c->gzfile_serial_max) {
    S = GzSerialParams{};
    SH = GzSerialHead{};
    if ((rc = gzfile_discover(c, d_in, in_len, H, G, P, mout))) return rc;
  } else if ((rc = gzfile_discover_serial(c, d_in, in_len, H, G, P, S, SH, mout))) {
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
    uint8_t *d_out = out;
    if (!dev) {
      if ((rc = ensure(c, c->d_out, total + 16))) return rc;
      d_out = (uint8_t *)c->d_out.p;
    }
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
    const uint32_t per_round = longest_run < c->one_round_units ? (longest_run ? longest_run : 1u) : c->one_round_units;
    const size_t fentries = (size_t)per_round * kWinEntries;
    GzFileDecParams GD{};
    OneDecParams &D = GD.D;
    uint32_t *d_sums;
    int32_t *d_ds;
    uint64_t *d_dl;
    int64_t *d_de;
    rc = carve(c, c->d_one_dec, [&](Carve &k) {
      k.take(D.dh, 1);
      k.take(D.F[0], fentries);
      k.take(D.F[1], fentries);
      k.take(D.R, ((size_t)per_round + 1) * kWinEntries);
      k.take(D.status, (size_t)n_dec + 1);
      k.take(D.err_off, (size_t)n_dec + 1);
      k.take(D.produced, (size_t)n_dec + 1);
      k.take(D.p_out_off, (size_t)per_round + 1);
      k.take(D.p_dict_at, per_round);
      k.take(D.p_dict_len, per_round);
      k.take(d_ds, per_round);
      k.take(d_dl, per_round);
      k.take(d_de, per_round);
    });
    if (rc) return rc;
    rc = carve(c, c->d_gzfile_dec, [&](Carve &k) {
      k.take(GD.v, 1);
      k.take(GD.seed, per_round);
      k.take(GD.p_bit_off, per_round);
      k.take(GD.p_bit_end, per_round);
      k.take(d_sums, (size_t)n_mem + 1);
    });
    if (rc) return rc;
    D.in = d_in;
    D.one = P.O.one;
    D.unit_bit = P.O.C.member_off;
    D.out_off = P.O.C.out_off;
    D.total = total;
    D.unit_max = P.O.unit_max;
    D.stored_units = P.O.stored_units;
    D.d_status = d_ds;
    D.d_out_len = d_dl;
    D.head = P.O.head;
    D.wrap = FLATE_HIP_WRAP_GZIP;
    D.in_len = in_len;
    GD.P = P;
    GD.n_good = H.h.n_members;
    GD.n_members = n_mem;
    GD.sums = d_sums;
    HIP_TRY(c, hipMemsetAsync(D.dh, 0xff, sizeof(OneDecHead), c->stream));     // first_bad, decode_bad: none
    HIP_TRY(c, hipMemsetAsync(GD.v, 0xff, sizeof(GzFileVerdict), c->stream));  // bad_trailer: none
    HIP_TRY(c, hipMemsetAsync(D.R, 0, kWinEntries, c->stream));                // in front of the file: zeros
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
    for (const auto &run : runs)
    for (uint32_t u0 = run.first; u0 < run.second; u0 += per_round) {
      D.u0 = u0;
      D.count = run.second - u0 < per_round ? run.second - u0 : per_round;
      const uint32_t unit_blocks = (D.count + 1u + 255u) / 256u;
      const uint32_t entry_blocks = (uint32_t)(((uint64_t)D.count * kWinEntries + 255) / 256);
      OneDecParams T = D;  // TAIL: a unit's history is what its own member has produced in front of it
      T.out_off = P.rel_off;
      one_tail_launch(c, D.count, T);
      hipLaunchKernelGGL(gzfile_pieces_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, GD);
      int cur = 0;
      for (uint32_t s = 1; s < D.count; s <<= 1, cur ^= 1)
        hipLaunchKernelGGL(one_seek_compose_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.F[cur ^ 1],
                           GD.seed, D.count, s);
      hipLaunchKernelGGL(one_seek_resolve_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.R, GD.seed,
                         D.count);
      // DECODE: the round's units as pieces with dictionaries and their own ends, through the lane-per-stream decoder
      InfParams I{};
      I.in = d_in;
      I.in_len = H.raw_len;
      I.bit_off = GD.p_bit_off;
      I.bit_end = GD.p_bit_end;
      I.n_streams = D.count;
      I.out = d_out;
      I.out_off = D.p_out_off;
      I.out_len = d_dl;
      I.status = d_ds;
      I.err_off = d_de;
      I.dict_buf = D.R;
      I.dict_at = D.p_dict_at;
      I.dict_len = D.p_dict_len;
      if ((rc = launch_decoders(c, inflate_route_units(c->inflate, c->num_cus, D.count), I, true))) return rc;  // (of several rounds the stage's time is the last one's)
      hipLaunchKernelGGL(one_check_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, D);
      used[FLATE_HIP_STAGE_INFLATE] = true;
      HIP_TRY(c, hipGetLastError());
      // the window behind the round's last unit seeds the next round (a round that starts with a member reads none of it)
      if (u0 + D.count < n_dec)
        HIP_TRY(c, hipMemcpyAsync(D.R, D.R + (size_t)D.count * kWinEntries, kWinEntries, hipMemcpyDeviceToDevice, c->stream));
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
    if (V.out_len > total) return FLATE_HIP_E_INTERNAL;
    *out_len = V.out_len;
    if (!dev && V.out_len) {  // the result comes down once
      HIP_TRY(c, hipMemcpyAsync(out, d_out, V.out_len, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
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
    if ((rc = gzfile_discover(c, d_in, in_len, H, G, P, nullptr))) return rc;
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
    const uint32_t per_round = n_dec < c->one_round_units ? n_dec : c->one_round_units;

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

    const size_t fentries = (size_t)per_round * kWinEntries;
    GzFileDecParams GD{};
    OneDecParams &D = GD.D;
    rc = carve(c, c->d_one_dec, [&](Carve &k) {
      k.take(D.dh, 1);
      k.take(D.F[0], fentries);
      k.take(D.F[1], fentries);
      k.take(D.R, ((size_t)per_round + 1) * kWinEntries);
      k.take(D.status, (size_t)n_dec + 1);
      k.take(D.err_off, (size_t)n_dec + 1);
      k.take(D.produced, (size_t)n_dec + 1);
      k.take(D.p_out_off, (size_t)per_round + 1);
      k.take(D.p_dict_at, per_round);
      k.take(D.p_dict_len, per_round);
    });
    if (rc) return rc;
    rc = carve(c, c->d_gzfile_dec, [&](Carve &k) {
      k.take(GD.seed, per_round);
      k.take(GD.p_bit_off, per_round);
      k.take(GD.p_bit_end, per_round);
    });
    if (rc) return rc;
    D.in = d_in;
    D.one = P.O.one;
    D.unit_bit = P.O.C.member_off;
    D.out_off = P.O.C.out_off;
    D.total = H.prefix_bytes + (H.fail_unit ? H.fail_out : 0ull);
    D.unit_max = P.O.unit_max;
    D.stored_units = P.O.stored_units;
    GD.P = P;
    GD.n_good = n;
    HIP_TRY(c, hipMemsetAsync(D.dh, 0xff, sizeof(OneDecHead), c->stream));  // first_bad: none
    K.point_unit = PP.point_unit;
    K.member_unit = P.member_unit;
    K.m = m;
    K.n_points = np;
    uint32_t p_next = 0;  // the first point whose round has not come yet
    for (uint32_t u0 = 0; u0 < n_dec; u0 += per_round) {
      D.u0 = u0;
      D.count = n_dec - u0 < per_round ? n_dec - u0 : per_round;
      const uint32_t unit_blocks = (D.count + 1u + 255u) / 256u;
      const uint32_t entry_blocks = (uint32_t)(((uint64_t)D.count * kWinEntries + 255) / 256);
      if (sound) {
        // a member's first unit is a seed that RESOLVE never writes: zeros in front of every member, so that a stored
        // window holds nothing of the member in front (slot 0 is the carried window unless the round starts a member)
        const bool starts = munit[bgzf_upper_bound(munit.data(), m, u0) - 1u] == u0;
        uint8_t *from = D.R + (starts ? 0 : kWinEntries);
        HIP_TRY(c, hipMemsetAsync(from, 0, ((size_t)D.count + (starts ? 1 : 0)) * kWinEntries, c->stream));
      }
      OneDecParams T = D;  // TAIL: a unit's history is what its own member has produced in front of it
      T.out_off = P.rel_off;
      one_tail_launch(c, D.count, T);
      hipLaunchKernelGGL(gzfile_pieces_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, GD);  // (the seeds)
      int cur = 0;
      for (uint32_t s = 1; s < D.count; s <<= 1, cur ^= 1)
        hipLaunchKernelGGL(one_seek_compose_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.F[cur ^ 1],
                           GD.seed, D.count, s);
      hipLaunchKernelGGL(one_seek_resolve_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.R, GD.seed,
                         D.count);
      // PACK: R[i] of the round's window-bearing points -> their blocks, which lie one behind the other in `windows`
      uint32_t p_hi = p_next;
      while (p_hi < np && points[p_hi] < (uint64_t)u0 + D.count) ++p_hi;
      if (p_hi > p_next) {
        const uint32_t cnt = p_hi - p_next;
        const uint32_t b_lo = gzfile_seek_blocks_before(munit.data(), m, p_next, (uint32_t)points[p_next]);
        const uint32_t b_hi = p_hi < np ? gzfile_seek_blocks_before(munit.data(), m, p_hi, (uint32_t)points[p_hi]) : np - m;
        if (b_hi > b_lo) {
          K.p_lo = p_next, K.np = cnt, K.u0 = u0;
          hipLaunchKernelGGL(gzfile_seek_pack_kernel, dim3((cnt + 1u + 255u) / 256u), dim3(256), 0, c->stream, K);
          BgzfGatherParams GP{};
          GP.scratch = D.R;  // (R[count] lies behind the last run: the 32 bytes the gather may touch)
          GP.out = d_windows + (uint64_t)b_lo * kSeekWindow;
          GP.r_out_off = K.r_out_off;
          GP.r_src = K.r_src;
          GP.n_ranges = cnt;
          const uint64_t pieces = ((uint64_t)(b_hi - b_lo) * kSeekWindow + (uint64_t)cnt * kBgzfGatherRangeCost +
                                   kBgzfGatherWindow - 1) / kBgzfGatherWindow;
          hipLaunchKernelGGL(bgzf_gather_kernel, dim3((uint32_t)pieces), dim3(256), 0, c->stream, GP);
        }
        p_next = p_hi;
      }
      HIP_TRY(c, hipGetLastError());
      if (u0 + D.count < n_dec)
        HIP_TRY(c, hipMemcpyAsync(D.R, D.R + (size_t)D.count * kWinEntries, kWinEntries, hipMemcpyDeviceToDevice, c->stream));
    }
    OneDecHead R{};
    HIP_TRY(c, hipMemcpyAsync(&R, D.dh, sizeof R, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (R.first_bad != 0xffffffffu) {  // TAIL's verdict: the serial decoder's, at the serial offset, in its member
      const uint32_t fb = R.first_bad;
      if (fb >= n_dec) return FLATE_HIP_E_INTERNAL;
      int32_t st = 0;
      int64_t eo = -1;
      uint32_t bm = 0;
      HIP_TRY(c, hipMemcpyAsync(&st, D.status + fb, 4, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(&eo, D.err_off + fb, 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(&bm, P.u_member + fb, 4, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
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
      const int64_t seo = (st == FLATE_HIP_E_CORRUPT && eo >= 0) ? eo - (int64_t)(bit >> 3) : -1;
      return fail(st ? st : FLATE_HIP_E_INTERNAL, bm, (int64_t)at, seo);
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
    hipLaunchKernelGGL(gzfile_init_kernel, dim3(1), dim3(64), 0, c->stream, d_one, in_len);
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

    const uint32_t per_round = ns < c->one_round_units ? ns : c->one_round_units;
    const size_t fentries = (size_t)per_round * kWinEntries;
    OneDecParams D{};
    GzSeekRoundParams Z{};
    OneSeekRoundParams &S = Z.S;
    int32_t *d_ds;
    uint64_t *d_dl;
    int64_t *d_de;
    rc = carve(c, c->d_one_dec, [&](Carve &k) {
      k.take(D.dh, 1);
      k.take(D.F[0], fentries);
      k.take(D.F[1], fentries);
      k.take(D.R, ((size_t)per_round + 1) * kWinEntries);
      k.take(D.status, (size_t)ns + 1);
      k.take(D.err_off, (size_t)ns + 1);
      k.take(D.produced, (size_t)ns + 1);
      k.take(S.seed, per_round);
      k.take(S.p_bit_off, per_round);
      k.take(S.p_bit_end, per_round);
      k.take(S.p_dict_at, per_round);
      k.take(S.p_dict_len, per_round);
      k.take(d_ds, per_round);
      k.take(d_dl, per_round);
      k.take(d_de, per_round);
      k.take(S.u_status, ns);
    });
    if (rc) return rc;
    if ((rc = ensure(c, c->d_one_seek_dense, RH.scratch_total + 64))) return rc;
    uint8_t *d_dense = (uint8_t *)c->d_one_seek_dense.p;
    uint8_t *d_out = out;
    if (!dev) {
      if ((rc = ensure(c, c->d_out, RH.out_total + 16))) return rc;
      d_out = (uint8_t *)c->d_out.p;
    }
    D.in = d_in;
    D.one = d_one;
    D.unit_bit = Q.unit_bit;
    D.out_off = GS.rel;  // TAIL: a unit's history is what its own member has produced in front of it
    D.unit_max = c->one_unit_max;
    D.stored_units = index[kGzSeekRuleAt] == kSeekRuleStored ? 1u : 0u;  // the index's rule, not the context's option
    D.unit_list = Q.sel_unit;
    S.Q = Q;
    S.windows = d_windows;
    S.R = D.R;
    S.d_status = d_ds;
    S.d_out_len = d_dl;
    Z.member_unit = GS.member_unit;
    Z.m = m;
    Z.rel = GS.rel;
    HIP_TRY(c, hipMemsetAsync(D.dh, 0xff, sizeof(OneDecHead), c->stream));
    bool used[FLATE_HIP_STAGE_COUNT] = {false, false, false, false};
    for (uint32_t i0 = 0; i0 < ns; i0 += per_round) {
      const uint32_t count = ns - i0 < per_round ? ns - i0 : per_round;
      D.u0 = S.i0 = i0;
      D.count = S.count = count;
      const uint32_t entry_blocks = (uint32_t)(((uint64_t)count * kWinEntries + 255) / 256);
      const uint32_t unit_blocks = (count + 255u) / 256u;
      hipLaunchKernelGGL(gzfile_seek_seed_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, Z);
      hipLaunchKernelGGL(gzfile_seek_load_kernel, dim3((entry_blocks + 15u) / 16u), dim3(256), 0, c->stream, Z);
      one_tail_launch(c, count, D);
      int cur = 0;
      for (uint32_t s = 1; s < count; s <<= 1, cur ^= 1)
        hipLaunchKernelGGL(one_seek_compose_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.F[cur ^ 1],
                           S.seed, count, s);
      hipLaunchKernelGGL(one_seek_resolve_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.R, S.seed, count);
      // DECODE: the round's units as spliced pieces with dictionaries, each with its own end, into their dense slots;
      // bits are counted from the file's first byte and nothing at or behind the last trailer is read
      InfParams I{};
      I.in = d_in;
      I.in_len = in_len - kGzipTrailerLen;
      I.bit_off = S.p_bit_off;
      I.bit_end = S.p_bit_end;
      I.n_streams = count;
      I.out = d_dense;
      I.out_off = Q.sel_at + i0;
      I.out_len = d_dl;
      I.status = d_ds;
      I.err_off = d_de;
      I.dict_buf = D.R;
      I.dict_at = S.p_dict_at;
      I.dict_len = S.p_dict_len;
      if ((rc = launch_decoders(c, inflate_route_units(c->inflate, c->num_cus, count), I, true))) return rc;
      used[FLATE_HIP_STAGE_INFLATE] = true;
      hipLaunchKernelGGL(one_seek_check_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, S);
      HIP_TRY(c, hipGetLastError());
      // the window behind the round's last unit is the carried seed of a segment that continues
      if (i0 + count < ns)
        HIP_TRY(c, hipMemcpyAsync(D.R, D.R + (size_t)count * kWinEntries, kWinEntries, hipMemcpyDeviceToDevice, c->stream));
    }

    // the gather: every range's run of the scratch to its place in out
    const uint64_t pieces = (RH.out_total + (uint64_t)kBgzfGatherRangeCost * nr + kBgzfGatherWindow - 1) / kBgzfGatherWindow;
    if (pieces > 0x7fffffffull) return FLATE_HIP_E_TOO_LARGE;
    BgzfGatherParams GP{};
    GP.scratch = d_dense;
    GP.out = d_out;
    GP.r_out_off = Q.r_out_off;
    GP.r_src = Q.r_src;
    GP.n_ranges = nr;
    hipLaunchKernelGGL(bgzf_gather_kernel, dim3((uint32_t)pieces), dim3(256), 0, c->stream, GP);
    HIP_TRY(c, hipGetLastError());
    std::vector<int32_t> st(ns);
    HIP_TRY(c, hipMemcpyAsync(st.data(), S.u_status, (size_t)ns * 4, hipMemcpyDeviceToHost, c->stream));
    if (!dev) HIP_TRY(c, hipMemcpyAsync(out, d_out, RH.out_total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->profiling && (rc = collect_timing(c, used))) return rc;

    // the statuses: nxt[i] = the first decoded unit at or behind place i with a status
    std::vector<uint32_t> nxt((size_t)ns + 1);
    nxt[ns] = ns;
    for (uint32_t i = ns; i-- > 0;) nxt[i] = st[i] ? i : nxt[i + 1];
    if (range_status)
      for (uint32_t r = 0; r < nr; ++r)
        if (r_lo[r] < r_hi[r] && r_hi[r] <= ns && nxt[r_lo[r]] < r_hi[r]) range_status[r] = st[nxt[r_lo[r]]];
    if (nxt[0] < ns) {
      if (bad_unit) *bad_unit = sel[nxt[0]];
      return st[nxt[0]];
    }
    return FLATE_HIP_OK;
  } catch (const std::exception &e) {
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

}  // extern "C"

// ---- the LONG entries of a ZIP archive through units (zip_units_kernels.hip, zip_units_rule.h) ----
// gzfile_discover and flate_hip_gzfile_read's rounds with the format's own glue: the hull as the raw stream, B nodes
// from the directory, the link that hops from entry to entry, pieces in ZIP's slots.  Read-backs: the candidate count;
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
  C.in = PA.C.in = h_in;
  C.in_len = PA.C.in_len = hull_len;
  C.n_tiles = PA.C.n_tiles = n_tiles;
  C.head = &P.O.head->h;
  P.O.unit_max = PA.unit_max = c->one_unit_max;
  P.O.stored_units = PA.stored_units = c->one_stored_units;
  PA.C.head = &head_a->h;
  PA.head = head_a;
  PA.one = P.O.one;
  hipLaunchKernelGGL(one_init_kernel, dim3(1), dim3(64), 0, c->stream, P.O.one, hull_len);  // the hull is the raw stream
  one_find_launch(c, true, n_tiles, PA);
  hipLaunchKernelGGL(chain_scan_kernel, dim3(1), dim3(1024), 0, c->stream, PA.C);
  HIP_TRY(c, hipGetLastError());
  OneHead HA{};
  HIP_TRY(c, hipMemcpyAsync(&HA, head_a, sizeof HA, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t na = HA.h.n_cand;
  if ((uint64_t)na + nb > 0x7ffffff0ull) return FLATE_HIP_E_TOO_LARGE;  // (the count saturates at 2^32 - 1)
  const uint32_t cap = na + nb;
  if ((rc = chain_size(C, cap)) || (rc = chain_size(PA.C, na))) return rc;
  P.n_a = na;
  P.n_b = nb;
  *n_cand = na;

  const size_t n = cap;
  rc = carve(c, c->d_zip_units, [&](Carve &k) {
    k.take(C.cand_off, n);
    k.take(P.O.probe, n);
    k.take(C.jump[0], n + 2);
    k.take(C.jump[1], n + 2);
    k.take(C.path, C.path_len);
    k.take(P.O.usize, n);
    k.take(C.member_off, n + 1);
    k.take(C.out_off, n + 1);
    k.take(P.u_start, n + 1);
    k.take(P.u_final, n);
    k.take(P.u_entry, n + 1);
    k.take(P.rel_off, n + 1);
  });
  if (rc) return rc;
  PA.C.cand_off = C.cand_off;
  if (na) one_find_launch(c, false, n_tiles, PA);
  hipLaunchKernelGGL(zip_units_bits_kernel, dim3((nb + 255) / 256), dim3(256), 0, c->stream, P);
  one_probe_launch(c, cap, P.O, 0u);
  const uint32_t node_blocks = (uint32_t)(((uint64_t)cap + 2 + 255) / 256);
  hipLaunchKernelGGL(zip_units_link_kernel, dim3(node_blocks), dim3(256), 0, c->stream, P);
  for (uint32_t j = 0; (1u << j) < C.path_len; ++j)
    hipLaunchKernelGGL(chain_round_kernel, dim3(node_blocks), dim3(256), 0, c->stream, C, j);
  hipLaunchKernelGGL(zip_units_finish_kernel, dim3((C.path_len + 255) / 256), dim3(256), 0, c->stream, P);
  hipLaunchKernelGGL(one_out_scan_kernel, dim3(1), dim3(1024), 0, c->stream, P.O);
  hipLaunchKernelGGL(zip_units_entries_kernel, dim3(1), dim3(1024), 0, c->stream, P);
  hipLaunchKernelGGL(zip_units_rel_kernel, dim3(node_blocks), dim3(256), 0, c->stream, P);
  HIP_TRY(c, hipGetLastError());
  OneHead H{};
  ZipUnitsHead Z{};
  std::vector<uint64_t> entry_unit((size_t)nb + 2, 0);
  HIP_TRY(c, hipMemcpyAsync(&H, P.O.head, sizeof H, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&Z, P.zh, sizeof Z, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(entry_unit.data(), P.entry_unit, ((size_t)nb + 2) * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (H.h.n_members > cap || Z.n_complete > nb) return FLATE_HIP_E_INTERNAL;
  // the entries the discovery finds GOOD, and their units: the only ones that are decoded
  const uint32_t g_disc = Z.n_complete < Z.first_unfit ? Z.n_complete : Z.first_unfit;
  G.P = P;
  if (g_disc == 0) return FLATE_HIP_OK;
  if (entry_unit[g_disc] > H.h.n_members) return FLATE_HIP_E_INTERNAL;
  const uint32_t n_dec = (uint32_t)entry_unit[g_disc];

  const uint32_t per_round = n_dec < c->one_round_units ? n_dec : c->one_round_units;
  const size_t fentries = (size_t)per_round * kWinEntries, pieces = 2 * (size_t)per_round;
  OneDecParams &D = G.D;
  int32_t *d_ds;
  uint64_t *d_dl;
  int64_t *d_de;
  rc = carve(c, c->d_one_dec, [&](Carve &k) {
    k.take(D.dh, 1);
    k.take(D.F[0], fentries);
    k.take(D.F[1], fentries);
    k.take(D.R, ((size_t)per_round + 1) * kWinEntries);
    k.take(D.status, (size_t)n_dec + 1);
    k.take(D.err_off, (size_t)n_dec + 1);
    k.take(D.produced, (size_t)n_dec + 1);
    k.take(D.p_out_off, pieces + 1);
    k.take(D.p_dict_at, pieces);
    k.take(D.p_dict_len, pieces);
    k.take(d_ds, pieces);
    k.take(d_dl, pieces);
    k.take(d_de, pieces);
  });
  if (rc) return rc;
  rc = carve(c, c->d_zip_units_dec, [&](Carve &k) {
    k.take(G.seed, per_round);
    k.take(G.p_bit_off, pieces);
    k.take(G.p_bit_end, pieces);
    k.take(G.du_status, per_round);
    k.take(G.du_out_len, per_round);
  });
  if (rc) return rc;
  D.in = h_in;
  D.one = P.O.one;
  D.unit_bit = C.member_off;
  D.out_off = C.out_off;
  D.total = total;
  D.unit_max = P.O.unit_max;
  D.stored_units = P.O.stored_units;
  D.d_status = G.du_status;
  D.d_out_len = G.du_out_len;
  D.head = P.O.head;
  D.wrap = FLATE_HIP_WRAP_RAW;
  D.in_len = hull_len;
  G.dp_status = d_ds;
  G.dp_out_len = d_dl;
  HIP_TRY(c, hipMemsetAsync(D.dh, 0xff, sizeof(OneDecHead), c->stream));  // first_bad, decode_bad: none
  HIP_TRY(c, hipMemsetAsync(D.R, 0, kWinEntries, c->stream));
  uint32_t e_at = 0;  // the entry of the round's first unit
  for (uint32_t u0 = 0; u0 < n_dec; u0 += per_round) {
    D.u0 = u0;
    D.count = n_dec - u0 < per_round ? n_dec - u0 : per_round;
    // the round's pieces: its units and a gap in front of every entry that starts behind its first unit
    while (entry_unit[e_at + 1u] <= u0) ++e_at;
    uint32_t e_hi = e_at;
    while (e_hi + 1u < g_disc && entry_unit[e_hi + 1u] < (uint64_t)u0 + D.count) ++e_hi;
    const uint32_t n_pieces = D.count + (e_hi - e_at);
    const uint32_t unit_blocks = (D.count + 1u + 255u) / 256u;
    const uint32_t entry_blocks = (uint32_t)(((uint64_t)D.count * kWinEntries + 255) / 256);
    OneDecParams T = D;  // TAIL: a unit's history is what its own entry has produced in front of it
    T.out_off = P.rel_off;
    one_tail_launch(c, D.count, T);
    hipLaunchKernelGGL(zip_units_pieces_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, G);
    int cur = 0;
    for (uint32_t s = 1; s < D.count; s <<= 1, cur ^= 1)
      hipLaunchKernelGGL(one_seek_compose_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.F[cur ^ 1],
                         G.seed, D.count, s);
    hipLaunchKernelGGL(one_seek_resolve_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.R, G.seed, D.count);
    InfParams I{};
    I.in = h_in;
    I.in_len = hull_len;
    I.bit_off = G.p_bit_off;
    I.bit_end = G.p_bit_end;
    I.n_streams = n_pieces;
    I.out = d_out;
    I.out_off = D.p_out_off;
    I.out_len = d_dl;
    I.status = d_ds;
    I.err_off = d_de;
    I.dict_buf = D.R;
    I.dict_at = D.p_dict_at;
    I.dict_len = D.p_dict_len;
    if ((rc = launch_decoders(c, inflate_route_units(c->inflate, c->num_cus, n_pieces), I, true))) return rc;  // (of several rounds the stage's time is the last one's)
    hipLaunchKernelGGL(zip_units_fold_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, G);
    OneDecParams K = D;  // the check: status 0 and exactly out_off[k + 1] - out_off[k] bytes
    K.p_out_off = C.out_off + u0;
    hipLaunchKernelGGL(one_check_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, K);
    HIP_TRY(c, hipGetLastError());
    // the window behind the round's last unit seeds the next round (a round that starts with an entry reads none of it)
    if (u0 + D.count < n_dec)
      HIP_TRY(c, hipMemcpyAsync(D.R, D.R + (size_t)D.count * kWinEntries, kWinEntries, hipMemcpyDeviceToDevice, c->stream));
  }
  // the one small read-back of g
  OneDecHead DH{};
  HIP_TRY(c, hipMemcpyAsync(&DH, D.dh, sizeof DH, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t bad_unit = DH.first_bad < DH.decode_bad ? DH.first_bad : DH.decode_bad;
  *g = zip_units_served(entry_unit.data(), g_disc, bad_unit);
  *n_units = (uint32_t)entry_unit[*g];
  return FLATE_HIP_OK;
}

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
