// flate_ctx.h -- the ctx and the host-side helpers that more than one host file of the C ABI uses (private, host
// only).  Everything in flate_host but its templates is DEFINED in flate_api.hip unless its comment names another file;
// flate_api_deflate.hip (the encode calls), flate_api_inflate.hip and flate_api_units.hip (the decode calls) are the users.
// (checksum.hip and gather.hip see the ctx through the flate::ctx_* accessors of flate_kernels.h.)
#pragma once

#include "flate_hip.h"

#include <hip/hip_runtime.h>

#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "carve.h"
#include "deflate_plan.h"
#include "flate_kernels.h"
#include "inflate_route.h"
#include "zip_kernels.h"

namespace flate_host {

// Device memory that belongs to one owner (the ctx, a stream handle): grown by ensure(), freed with the owner, whose
// release function has selected the device.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

}  // namespace flate_host

struct flate_hip_ctx {
  using DevBuf = flate_host::DevBuf;
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string hip_err;
  bool profiling = false;
  float stage_ms[FLATE_HIP_STAGE_COUNT] = {0, 0, 0, 0};
  hipEvent_t ev[2 * FLATE_HIP_STAGE_COUNT] = {};
  // persistent device data
  DevBuf scan_tab;
  int scan_len = 0;
  // grow-only scratch
  DevBuf d_in, d_out, d_in_off, d_chunk_base, d_ids16, d_ids32, d_matches, d_nmatch, d_ntok;
  DevBuf d_slot_off, d_out_len, d_out_off, d_status;
  DevBuf d_blk_base, d_blk_hist, d_blk_cl, d_blk_hdr, d_blk_meta, d_tile_meta, d_blk_sid;
  DevBuf d_istatus, d_ierr, d_debug, d_gtables, d_queue, d_simt_lens;
  DevBuf d_dicts, d_dict_at, d_dict_len;  // flate_hip_inflate_batch_dict: dictionary tails, per-stream (at, len)
  // flate_hip_deflate_fast_batch_dict (it shares the three above, there per used dictionary): the streams that start
  // from a dictionary, every stream's dictionary slot, the primed tables and sweep clocks of the slots
  DevBuf d_idsD, d_lz_slot_of, d_lz_tables, d_lz_clocks;
  // the *_framed calls: member offsets, the streams' checksums, per stream its dictionary, the dictionaries' Adler-32
  // (DICTIDs) and, for host callers, the whole dictionaries
  DevBuf d_frame_off, d_frame_sums, d_frame_dict_of, d_frame_ids, d_frame_dicts;
  // flate_hip_deflate_fast_grouped_framed (it shares d_frame_off: the members' offsets, d_frame_sums: the groups' sums):
  // group_off, every piece's group, the groups' ends and payload starts, the bit indexes (GroupParams), carved from one buffer
  DevBuf d_group;
  // flate_hip_inflate_batch_framed (it shares d_frame_off: the raw streams' starts, d_frame_sums, d_frame_ids,
  // d_frame_dicts): the raw streams' ends, the trailers' sums and ISIZEs, the header verdicts, the chosen dictionaries,
  // and per dictionary where its staged tail lies and how long it is
  DevBuf d_rd_end, d_rd_want, d_rd_isize, d_rd_bad, d_rd_dict, d_rd_tail_at, d_rd_tail_len;
  // flate_hip_inflate_spliced_framed (it shares d_frame_off: the index counted from the member's first byte,
  // d_frame_sums: the pieces' sums, d_rd_bad: the header verdict per piece): the one member's words (FrameOne)
  DevBuf d_rd_one;
  // flate_hip_bgzf_index / _read: the discovery kernels' arrays (BgzfParams), carved from one buffer (carve.h)
  DevBuf d_bgzf;
  // flate_hip_bgzf_read_ranges: the range kernels' arrays (BgzfRangeParams), carved from one buffer; the dense scratch
  // the touched members are decoded into; and, for the framed read it runs over them, the members' ends
  DevBuf d_bgzf_rng, d_bgzf_dense, d_in_end;
  // flate_hip_zip_write: the names and their offsets; flate_hip_zip_index / _read: the end record's words, the
  // discovery kernels' arrays (ZipDirParams) carved from one buffer, the selected entries and the stored pieces
  // flate_hip_gzip_index / _read: the discovery kernels' arrays (GzipParams) and what the parse kernel and the size-only
  // decode leave per candidate, carved from one buffer; in front of it (sized before the candidates are counted) the
  // result words and the tiles' counts
  DevBuf d_gzip, d_gzip_tiles;
  // ... and the range a candidate is given at most (option "gzip_member_max": it can only be lowered)
  uint64_t gzip_member_max = (1ull << 28) - 1;
  // flate_hip_inflate_one_index: the block discovery's arrays (OneParams) and the probes' results, carved from one
  // buffer; in front of it (sized before the candidates are counted) the result words, the one member's words
  // (FrameOne) and the tiles' counts
  DevBuf d_one, d_one_tiles;
  // ... and the bytes a unit's input spans at most (option "one_unit_max": it can only be lowered)
  uint64_t one_unit_max = 1ull << 28;
  // ... and the unit rule (option "one_stored_units"): 0 = dynamic headers start units, 1 = stored headers too
  uint32_t one_stored_units = 0;
  // flate_hip_inflate_one: the decode's arrays of one round (OneDecParams: the tail functions twice, the windows, the
  // per-unit results), carved from one buffer; the units of a round (option "one_round_units")
  DevBuf d_one_dec;
  uint32_t one_round_units = 4096;
  // flate_hip_inflate_one_seek_index / _ranges: the point, range and selection arrays (OneSeekPointsParams,
  // OneSeekParams), carved from one buffer; a host caller's windows; the dense scratch the selected units are decoded
  // into.  Both calls carve their rounds' arrays from d_one_dec.
  DevBuf d_one_seek, d_one_seek_win, d_one_seek_dense;
  // flate_hip_seek_windows_pack / _unpack, flate_hip_inflate_one_ranges_packed: the per-block records and the uploaded
  // index; the sparsified blocks, one slot each; the non-empty blocks compacted (pack), a host caller's packed bytes or
  // the selected streams compacted (unpack, read); a host caller's encoded bytes; the read's dense stage of the
  // selected points' blocks
  DevBuf d_seek_pack, d_seek_pack_dense, d_seek_pack_stage, d_seek_pack_out, d_seek_pack_sel;
  // flate_hip_gzfile_index / _read: the two count passes' words and tile counts (sized before the candidates are
  // counted), the chain's arrays (GzFileParams), and the read's member-wise arrays beside d_one_dec's
  DevBuf d_gzfile_tiles, d_gzfile, d_gzfile_dec;
  // ... with the option "gzfile_serial_max" (0 = off, the default: none of this is touched): a member whose header and
  // raw stream fit in that many bytes and decode cleanly is one unit, decoded whole by the batch decoders
  // (gzfile_serial_rule.h).  Phase 1's arrays over List B (sized when the B count is known), the per-unit marks (sized
  // with the chain), the read's batch results; and what the last index or read call did (flate_hip_gzfile_last_route)
  uint64_t gzfile_serial_max = 0;
  DevBuf d_gzfile_serial, d_gzfile_serial_units, d_gzfile_serial_dec;
  uint32_t gzfile_route[2] = {0, 0};  // serial members, unit members
  uint64_t gzfile_route_from = 0;     // find_from
  // flate_hip_gzfile_reader_read on a handle with flate_hip_gzfile_reader_set_serial_max (0 = off, the default: none of
  // this is touched; gzfile_parts_serial_rule.h): phase 1's arrays over the part's List B with the verdicts, the
  // per-unit marks, the batch results of the whole members
  DevBuf d_gzfile_parts_serial, d_gzfile_parts_serial_units, d_gzfile_parts_serial_dec;
  DevBuf d_zip_names, d_zip_name_off, d_zip_whead, d_zip_end, d_zip_dir, d_zip_sel;
  // flate_hip_zip_read with the option "zip_unit_min" (0 = off, the default: none of this is touched): a deflated entry
  // of at least that many compressed bytes is decoded through units.  The count pass's words, L and the tile counts
  // (sized before the candidates are counted), the chain's arrays (ZipUnitsParams), the rounds' entry-wise arrays
  // beside d_one_dec's; and what the last call did (flate_hip_zip_last_route)
  uint64_t zip_unit_min = 0;
  DevBuf d_zip_units_tiles, d_zip_units, d_zip_units_dec;
  uint32_t zip_route[4] = {0, 0, 0, 0};  // unit entries, fallback entries, units, candidates
  // flate_hip_zip_write with the option "zip_piece_bytes" (0 = off, the default: the same kernels, no new launch, no new
  // allocation): an entry longer than that many bytes is written from pieces, as one group of a grouped call; and what
  // the last write did (flate_hip_zip_write_last_route)
  uint64_t zip_piece_bytes = 0;
  uint32_t zip_write_route[2] = {0, 0};  // long entries, pieces
  hipStream_t guest_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int32_t h_status_word = 0;  // landing pads of small async D2H copies
  int32_t h_status_aux = 0;   // (flate_hip_bgzf_write: the first block whose member BSIZE cannot express)
  uint64_t h_total_bytes = 0;
  uint32_t num_cus = 256;
  flate::InflateOpts inflate;  // the "inflate_*" options (inflate_route.h)
  flate::EncodeOpts enc;       // the encoder's launch options (deflate_plan.h)
  // (Rounds 2-4 carried an entropy stage OVERLAPPED with the match finder -- sub-batches gated on counters
  // the persistent launch incremented, in an even and an uneven form.  Never faster than running the two one
  // after the other (profiles/r02, r04), and a soak run of round 4 once saw the pack kernel's self-check fire
  // in the even form, not reproduced in 115 000 stress runs: removed)
  // window-granular scheduling of multi-window streams (lz77_kernels.hip, uq_*)
  DevBuf d_uq_ready, d_uq_tables, d_uq_sweep;
  DevBuf d_aux[2];  // ctx_scratch (checksum.hip)
  // measurement aid (flate_hip_last_resident_share)
  uint32_t last_count[2] = {0, 0};   // queue lengths of the last persistent launches (16-bit, multi)
  uint32_t queue_init = 0;
  uint32_t debug_chunks = 0;
  // Host-pointer calls of the batch encoder: the batch is cut into host_groups groups of streams
  // and group g is compressed while group g+1 is copied in and the output of group g-1 is copied
  // out (two copy threads on two non-blocking streams).  0 = one copy in, compress, one copy out.
  int host_groups = 8;
  uint32_t host_group_streams = 2048;  // a group holds at least this many streams (inflate: four times as many)
  uint32_t inject_drop_push = 0;  // test hook: the k-th window hand-over (1-based) is dropped
  uint32_t inject_stall = 0;      // test hook: the k-th dense batch (1-based) of every chunk makes no progress
  uint64_t stream_rebase = 1ull << 30;  // flate_hip_stream: origin moved up past this many bytes
  int64_t debug_buffer_reset = 0;       // test hook: buffer_reset (deflate-fast.mbt:55) of streams opened from now on
  hipStream_t h2d_stream = nullptr, d2h_stream = nullptr;
  // Host-pointer batches run their groups on TWO lanes (sub-contexts with their own streams and
  // scratch, driven by two host threads): the persistent match-finder launch of group g+1 fills the
  // chip while group g's last streams, its entropy kernels and its size read-back drain, which a single
  // lane leaves idle (4 groups of 4096 streams: 19.9 ms of match finding against 16.2 for the batch
  // as one launch).  0 = one lane (round 3's behaviour).
  int host_lanes = 2;
  flate_hip_ctx *lane[2] = {nullptr, nullptr};
  // pinned staging of a call's small index arrays (ctl_up / ctl_down): they travel by a copy KERNEL,
  // never through the DMA engines the bulk transfers of the host-pointer pipelines occupy
  struct CtlStage {
    uint8_t *p = nullptr;
    size_t cap = 0, used = 0;
  } ctl_up_buf, ctl_down_buf;
  struct CtlPending {
    void *host_dst;
    size_t off, bytes;
  };
  std::vector<CtlPending> ctl_pending;
};

#define HIP_TRY(ctx, expr)                                                         \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess) {                                                        \
      (ctx)->hip_err = std::string(#expr) + ": " + hipGetErrorString(e_);          \
      return FLATE_HIP_E_HIP;                                                      \
    }                                                                              \
  } while (0)

namespace flate_host {

int ensure(flate_hip_ctx *c, DevBuf &b, size_t bytes);
// b as a call's arrays: lay(k) names every array on the Carve k, in order, with its type and its count.  It runs over
// no buffer for the size, and again over b once ensure() has made that much room (a failed allocation is
// FLATE_HIP_E_HIP, never a truncated result).
template <typename Lay>
int carve(flate_hip_ctx *c, DevBuf &b, Lay lay) {
  Carve k;
  lay(k);
  const int rc = ensure(c, b, k.at);
  if (rc) return rc;
  k = Carve{b.p, 0};
  lay(k);
  return FLATE_HIP_OK;
}
// in[0, in_len) on the device: the caller's buffer, or the ctx's staged copy of it
int stage_input(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t flags, const uint8_t **d_in);
// The route's kernel over the n streams of I, inside the inflate stage's events (flate_api_inflate.hip: the only place
// that knows the decoder kernels).  dict: some stream starts from a preset dictionary (the dictionary builds).
int launch_decoders(flate_hip_ctx *c, const flate::InflateRoute &rt, flate::InfParams I, bool dict);
// The gather (bgzf_gather_kernel; flate_api_inflate.hip): range r's run scratch[r_src[r], ...) to d_out[r_out_off[r],
// r_out_off[r + 1]).  piece_bytes: the bytes of all runs, which with the ranges' fixed cost cut the work into
// workgroups -- more of them than a grid holds is FLATE_HIP_E_TOO_LARGE (for the PACK gathers of the two seek-index
// builds, which had no such check of their own, out of reach: a round's windows are at most 65536 * 32 KiB).  The caller
// checks the launch.
int ranges_gather(flate_hip_ctx *c, const uint8_t *scratch, uint8_t *d_out, const uint64_t *r_out_off, const uint64_t *r_src,
                  uint32_t n_ranges, uint64_t piece_bytes);

// ---- what the four discoveries share on the host (flate_kernels.h: THE DISCOVERY SKELETON) ----
// the tiles over the offsets [lo, lo + len) of the device buffer d_in, or FLATE_HIP_E_TOO_LARGE
int tiles_for(const uint8_t *d_in, uint64_t lo, uint64_t len, uint32_t *n_tiles);
// C.cap and C.path_len for arrays of cap candidates, or FLATE_HIP_E_TOO_LARGE
int chain_size(flate::ChainParams &C, uint32_t cap);
// The launches behind a format's fill (and whatever it runs over the candidates): its link kernel, the rounds of
// pointer doubling, its finish and out-scan kernels; one check of all launches so far.  link(grid) and finish(grid)
// launch the format's kernels over the grids they are given (256 threads a workgroup) with whatever arguments those
// take; mid(node_blocks) is the one place for a launch between finish and out-scan.
template <typename Link, typename Finish, typename Mid, typename SP>
int chain_tail_by(flate_hip_ctx *c, const flate::ChainParams &C, Link link, Finish finish, Mid mid, void (*out_scan)(SP),
                  const SP &sp) {
  const uint32_t node_blocks = (uint32_t)(((uint64_t)C.cap + 2 + 255) / 256);
  link(dim3(node_blocks));
  for (uint32_t j = 0; (1u << j) < C.path_len; ++j)
    hipLaunchKernelGGL(flate::chain_round_kernel, dim3(node_blocks), dim3(256), 0, c->stream, C, j);
  finish(dim3((C.path_len + 255) / 256));
  mid(node_blocks);
  hipLaunchKernelGGL(out_scan, dim3(1), dim3(1024), 0, c->stream, sp);
  HIP_TRY(c, hipGetLastError());
  return FLATE_HIP_OK;
}
// ... of a format whose link and finish kernels take one parameter block each and that has nothing for `mid`
template <typename LP, typename FP>
int chain_tail(flate_hip_ctx *c, const flate::ChainParams &C, void (*link)(LP), const LP &lp, void (*finish)(FP),
               void (*out_scan)(FP), const FP &fp) {
  return chain_tail_by(
      c, C, [&](dim3 g) { hipLaunchKernelGGL(link, g, dim3(256), 0, c->stream, lp); },
      [&](dim3 g) { hipLaunchKernelGGL(finish, g, dim3(256), 0, c->stream, fp); }, [](uint32_t) {}, out_scan, fp);
}

// ---- small index arrays: host <-> device through pinned staging and a copy kernel (copy_ctl_kernel) ----
// ctl_begin: room for the call's uploads / downloads (a staging buffer only grows between calls: the
// stream is drained first).  ctl_up: stage + launch.  ctl_down: launch into the staging; the bytes reach
// the caller's array in ctl_finish, after the stream has been synchronised.
int ctl_begin(flate_hip_ctx *c, size_t up_bytes, size_t down_bytes);
int ctl_up(flate_hip_ctx *c, void *dev_dst, const void *host_src, size_t bytes);  // (bytes: rounded up to 4)
int ctl_down(flate_hip_ctx *c, void *host_dst, const void *dev_src, size_t bytes);
void ctl_finish(flate_hip_ctx *c);
// what a step of a call moves through that staging (the sum of a call's steps is what ctl_begin is given)
struct CtlBytes {
  size_t up = 0, down = 0;
  void operator+=(const CtlBytes &o) { up += o.up, down += o.down; }
};

struct StageTimer {
  flate_hip_ctx *c;
  int stage;
  StageTimer(flate_hip_ctx *ctx, int s) : c(ctx), stage(s) {
    if (c->profiling) (void)hipEventRecord(c->ev[2 * stage], c->stream);
  }
  ~StageTimer() {
    if (c->profiling) (void)hipEventRecord(c->ev[2 * stage + 1], c->stream);
  }
};
int collect_timing(flate_hip_ctx *c, const bool used[FLATE_HIP_STAGE_COUNT]);

// ---- host-pointer batches, pipelined over groups of streams (flate_hip_ctx::host_groups) ----
double host_now_ms();
void host_trace(double t0, const char *what, unsigned g, double a, double b);
struct CopyJob {
  void *dst;
  const void *src;
  size_t bytes;
};
// Two copy threads beside the calling thread: one brings the groups' input to the device in
// order, the other takes every group's output back as soon as the caller posts it.  Each uses its
// own non-blocking HIP stream, so the copies run beside the kernels of the group in between.
class CopyPipe {
 public:
  CopyPipe(size_t n_in, size_t n_out) : in_ready_(n_in, 0), out_state_(n_out, 0), out_jobs_(n_out) {}
  // (not in the constructor: if the second thread cannot be created, the destructor must still run
  // to join the first)
  void start(int device, hipStream_t s_in, hipStream_t s_out, std::vector<CopyJob> in_jobs);
  // blocks until group g's input is on the device; false = its copy failed
  bool wait_in(size_t g);
  void post_out(size_t g, CopyJob j);
  // ends both threads (outputs not posted yet are dropped) and returns the first copy error
  std::string finish();
  ~CopyPipe() { (void)finish(); }

 private:
  bool run(const CopyJob &j, hipMemcpyKind kind, hipStream_t s, const char *what);
  double t0_ = host_now_ms();
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<int> in_ready_, out_state_;  // 0 pending, 1 done / posted, -1 failed / dropped
  std::vector<CopyJob> out_jobs_;
  std::string err_;
  bool stop_ = false;
  std::thread t_in_, t_out_;
};
void cut_by_bytes(const uint64_t *a, const uint64_t *b, uint32_t n, uint32_t G, std::vector<uint32_t> &lo);
int host_pipe_streams(flate_hip_ctx *c);

// The dictionaries a *_batch_dict call uses, as slots: a slot is one dictionary that some stream names and whose
// tail -- its last kMaxMatchOffset bytes, the history a stream can reach -- has at least min_len bytes.  The tails
// lie one after another in c->d_dicts, each 16-byte aligned and followed by 16 bytes that a 16-byte load may touch.
struct DictSlots {
  static constexpr uint32_t kNone = ~0u;
  std::vector<uint32_t> dict, len;  // per slot: the dictionary, the length of its tail
  std::vector<uint64_t> at;         // per slot: where the tail starts in d_dicts
  std::vector<uint32_t> slot_of;    // per stream: its slot, or kNone
  uint64_t total = 0;               // bytes of d_dicts
};
DictSlots dict_slots(const uint64_t *dict_off, uint32_t n_dicts, const uint32_t *dict_of, uint32_t n, uint32_t min_len);
int dict_upload(flate_hip_ctx *c, const DictSlots &S, const uint8_t *dicts, const uint64_t *dict_off, uint32_t flags);

// The DICTIDs of a *_framed call: the Adler-32 of every WHOLE dictionary, left in c->d_frame_ids (host callers: the
// dictionaries are uploaded to c->d_frame_dicts first).  Queued on c->stream behind a ctl_begin that covers
// dictid_ctl_up_bytes; slot 0 of the scratch must already hold dictid_scratch_bytes -- a caller that queues another
// run of checksums behind it sizes the slot ONCE for the larger of the two before either is queued, so that the
// second cannot grow (free) what the first's kernels are still to read.
size_t dictid_ctl_up_bytes(const uint64_t *dict_off, uint32_t n_dicts);
size_t dictid_scratch_bytes(const uint64_t *dict_off, uint32_t n_dicts);
int dictid_stage(flate_hip_ctx *c, const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts, uint32_t flags);

}  // namespace flate_host
