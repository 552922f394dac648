// flate_api_deflate.hip -- the encode calls of the C ABI (see include/flate_hip.h): flate_hip_deflate_fast_batch, _spliced,
// _batch_dict, _batch_framed, _spliced_framed, flate_hip_bgzf_write, the flate_hip_stream_* writer and
// flate_hip_lz77_matches.
//
// Host-side driver: plans the chunking exactly as Compressor::write / enc_speed / close stage their 65535-byte window
// (reference deflate.mbt:222-294,157-183) and launches the kernels on one HIP stream.  There is no CPU compression
// path in this library.  One driver (deflate_common) serves the batch calls as a sequence: plan, stage the input,
// ensure the scratch, the container's part in front of the match finder, the match finder, the entropy stage, the
// container's part behind it, read back.  The plan and every launch decision are deflate_plan.h's (run_lz77 and
// launch_entropy are the only places that know kernels); the argument checks are api_checks.h's; the ctx, its staging and
// the host pipeline's copy threads are flate_api.hip's (flate_ctx.h).
#include "flate_ctx.h"

#include <cstring>
#include <exception>
#include <stdexcept>

#include "api_checks.h"
#include "bgzf_rule.h"
#include "checksum_clip.h"
#include "zip_rule.h"

using namespace flate;
using namespace flate_host;

namespace {

// One encode call as its entry point received and checked it.  spliced: the whole batch becomes ONE DEFLATE stream;
// out_off then receives the bit position of every stream (may be null).  total_bytes (may be null): what the call wrote
// to `out`.
struct EncCall {
  const uint8_t *in;
  const uint64_t *in_off;
  uint32_t n;
  uint8_t *out;
  uint64_t out_cap;
  uint64_t *out_off;
  uint64_t *total_bytes;
  uint32_t flags;
  bool spliced;
  // grouped (flate_hip_deflate_fast_grouped_framed; it implies spliced): the n streams are the pieces of n_groups
  // spliced streams, group g = pieces [group_off[g], group_off[g + 1]); out_off then receives the MEMBERS' offsets
  // (n_groups + 1) and bit_idx (may be null) the groups' bit indexes (n + n_groups).  All three are HOST arrays.
  const uint32_t *group_off = nullptr;
  uint32_t n_groups = 0;
  uint64_t *bit_idx = nullptr;
};

// The preset dictionaries of an encode call (flate_hip_deflate_fast_batch_dict), already on the device.
struct DeflDict {
  LzDictParams dev;
  uint32_t n_slots;        // used dictionaries of at least kSmallHuffMin bytes (after the cut to 32768)
  const uint8_t *has;      // host, per stream: it uses one of them
};

// The container of a *_framed call (frame_kernels.hip); everything here is the caller's.
struct FrameReq {
  uint32_t wrap;            // FLATE_HIP_WRAP_ZLIB / _GZIP
  const uint32_t *dict_of;  // host, per stream: the dictionary whose DICTID its header carries, or FLATE_HIP_NO_DICT;
                            // null: no dictionaries
  const uint8_t *dicts;     // the WHOLE dictionaries (host, or device under FLATE_HIP_DEVICE_PTRS) ...
  const uint64_t *dict_off; // ... dictionary j = dicts[dict_off[j], dict_off[j+1])
  uint32_t n_dicts;
};

// The parameter blocks as far as the ctx owns what they point at (its scratch, its options); the callers add
// the input, the index arrays and what is theirs alone.
LzParams lz_params(const flate_hip_ctx *c, uint32_t flags) {
  LzParams P{};  // (value-initialised: a field added later must never reach a kernel as stack garbage)
  P.scan_off = (const uint16_t *)c->scan_tab.p;
  P.scan_len = c->scan_len;
  P.matches = (uint2 *)c->d_matches.p;
  P.chunk_nmatch = (uint32_t *)c->d_nmatch.p;
  P.chunk_ntok = (uint32_t *)c->d_ntok.p;
  P.compat_go = (flags & FLATE_HIP_COMPAT_GO) ? 1u : 0u;
  P.spin_limit = c->enc.spin_limit;
  P.status = (int *)c->d_status.p;
  return P;
}

// spliced: the streams' blocks follow one another bit by bit (summaries in d_slot_off, bit positions in d_out_off)
HuffParams huff_params(const flate_hip_ctx *c, uint32_t flags, bool spliced) {
  HuffParams H{};
  H.matches = (const uint2 *)c->d_matches.p;
  H.chunk_nmatch = (const uint32_t *)c->d_nmatch.p;
  H.chunk_ntok = (const uint32_t *)c->d_ntok.p;
  H.blk_hist = (uint32_t *)c->d_blk_hist.p;
  H.blk_cl = (uint32_t *)c->d_blk_cl.p;
  H.blk_hdr = (uint32_t *)c->d_blk_hdr.p;
  H.blk_meta = (uint4 *)c->d_blk_meta.p;
  H.tile_meta = (uint8_t *)c->d_tile_meta.p;
  H.spliced = spliced ? 1u : 0u;
  H.stream_sum = spliced ? (uint64_t *)c->d_slot_off.p : nullptr;
  H.stream_bit = spliced ? (const uint64_t *)c->d_out_off.p : nullptr;
  H.out_len = (uint64_t *)c->d_out_len.p;
  H.out_off = (const uint64_t *)c->d_out_off.p;
  H.status = (int *)c->d_status.p;
  H.compat_go = (flags & FLATE_HIP_COMPAT_GO) ? 1u : 0u;
  return H;
}

// The encoder's device status word (not 0) as the call's return code.  A word of the scan kernels is a public
// code already; everything from kStatusUqTimeout down is FLATE_HIP_E_INTERNAL, with what happened in hip_err.
int encoder_status(flate_hip_ctx *c, int word) {
  if (word > kStatusUqTimeout) return word;
  if (word == kStatusNoProgress)
    c->hip_err = "a match-finder batch made no progress (the chunk was abandoned)";
  else if (word == kStatusLanesLost)
    c->hip_err = "a persistent match-finder loop lost lanes of its wavefront (miscompiled loop?)";
  else if (word == kStatusUqTimeout)
    c->hip_err = "a match-finder block waited for a window that was never handed over";
  else if (word == kStatusBadIndex)
    c->hip_err = "a match-finder block was handed an index outside its scratch";
  else if (word <= -0x100000)  // encoder self-check (huff_pack_kernel): -(0x100000 + stream)
    c->hip_err = "packed bits differ from the computed block size in stream " +
                 std::to_string((uint32_t)(-word) - 0x100000u) + " (mod 2^20)";
  else
    c->hip_err = "device status word " + std::to_string(word);
  return FLATE_HIP_E_INTERNAL;
}

// A resident (LDS-table) kernel on c->stream and a guest (L2-table) kernel on c->guest_stream, side by side: the
// blocks of both pull the `count` entries of one queue.  R / G: the two sides' parameters; extra: what both
// kernels take after them.
// The LDS-table kernel is submitted FIRST: its blocks need 26 contiguous LDS granules each, and guests that
// reach a CU before them can leave it with room for three (measured: -1.4 % with this order, section 7 of
// profiles/r05/README.md).
template <typename... Extra>
void launch_pair(flate_hip_ctx *c, void (*resident)(LzParams, Extra...), void (*guest)(LzParams, Extra...),
                 uint32_t count, const LzParams &R, const LzParams &G, const Extra &...extra) {
  (void)hipEventRecord(c->ev_fork, c->stream);
  (void)hipStreamWaitEvent(c->guest_stream, c->ev_fork, 0);
  const uint32_t blocks = c->enc.resident_blocks < count ? c->enc.resident_blocks : count;
  hipLaunchKernelGGL(resident, dim3(blocks), dim3(64), 0, c->stream, R, extra...);
  hipLaunchKernelGGL(guest, dim3((uint32_t)c->enc.guest_blocks), dim3(64), 0, c->guest_stream, G, extra...);
  (void)hipEventRecord(c->ev_join, c->guest_stream);
  (void)hipStreamWaitEvent(c->stream, c->ev_join, 0);
}

// The match records and the windows' counts of n_chunks windows (the batch driver's and the stream writer's; a piece
// of a stream keeps room for the records of min_record_chunks windows even when it has none).
int ensure_lz_scratch(flate_hip_ctx *c, uint32_t n_chunks, uint32_t min_record_chunks = 0) {
  const uint32_t rec = n_chunks > min_record_chunks ? n_chunks : min_record_chunks;
  int rc;
  if ((rc = ensure(c, c->d_matches, (size_t)rec * kMatchCapPerChunk * sizeof(uint2) + 16))) return rc;
  if ((rc = ensure(c, c->d_nmatch, (size_t)n_chunks * 4 + 4))) return rc;
  return ensure(c, c->d_ntok, (size_t)n_chunks * 4 + 4);
}

// Upload the index arrays (lz77_ctl_up, deflate_plan.h) and run the match finder over every LZ77 chunk, as the route
// says; the caller has made room with ensure_lz_scratch.
// (the caller has checked that the launch is one persistent resident+guest launch in stream order)
// DD: the preset dictionaries of the streams in pl.idsD (null: there are none)
int run_lz77(flate_hip_ctx *c, const uint8_t *d_in, const uint64_t *in_off, const StagePlan &pl, const EncodeRoute &rt,
             uint32_t flags, const DeflDict *DD = nullptr) {
  const uint32_t n = pl.n_streams;
  int rc;
  if ((rc = ensure(c, c->d_in_off, ((size_t)n + 1) * 8))) return rc;
  if ((rc = ensure(c, c->d_chunk_base, ((size_t)n + 1) * 4))) return rc;
  if ((rc = ensure(c, c->d_ids16, pl.ids16.size() * 4 + 4))) return rc;
  if ((rc = ensure(c, c->d_ids32, pl.ids32.size() * 4 + 4))) return rc;
  if ((rc = ctl_up(c, c->d_in_off.p, in_off, ((size_t)n + 1) * 8))) return rc;
  if ((rc = ctl_up(c, c->d_chunk_base.p, pl.chunk_base.data(), ((size_t)n + 1) * 4))) return rc;
  if ((rc = ctl_up(c, c->d_ids16.p, pl.ids16.data(), pl.ids16.size() * 4))) return rc;
  if ((rc = ctl_up(c, c->d_ids32.p, pl.ids32.data(), pl.ids32.size() * 4))) return rc;
  if (!pl.idsD.empty()) {
    if (!DD || (flags & FLATE_HIP_LZ_SERIAL)) return FLATE_HIP_E_INTERNAL;
    if ((rc = ensure(c, c->d_idsD, pl.idsD.size() * 4 + 4))) return rc;
    if ((rc = ctl_up(c, c->d_idsD.p, pl.idsD.data(), pl.idsD.size() * 4))) return rc;
  }

  LzParams P = lz_params(c, flags);
  P.in = d_in;
  P.in_off = (const uint64_t *)c->d_in_off.p;
  P.chunk_base = (const uint32_t *)c->d_chunk_base.p;
  P.inject_drop_push = c->inject_drop_push;  // (the test hooks act on batch launches only)
  P.inject_stall = c->inject_stall;
  const bool hooks = lz77_hooks_build(c->inject_stall, c->inject_drop_push);  // only the HOOKS builds read the two
  c->last_count[0] = c->last_count[1] = 0;
  // multi-window streams of a persistent launch run one window at a time (EncodeRoute::uq_units) -- the one launch
  // decision the route does not settle: no memory for the scratch is whole-stream scheduling as well
  uint32_t uq_units = rt.uq_units;
  const size_t n32 = pl.ids32.size();
  if (uq_units) {
    // (grow-only scratch, 32 KiB per multi-window stream: when the device cannot give it, the
    // launch falls back to whole-stream scheduling, which needs none)
    if (ensure(c, c->d_uq_ready, (size_t)uq_units * 4 + 64) != FLATE_HIP_OK ||
        ensure(c, c->d_uq_tables, n32 * (size_t)kTableSize * 2 + 64) != FLATE_HIP_OK ||
        ensure(c, c->d_uq_sweep, n32 * 4 + 64) != FLATE_HIP_OK) {
      (void)hipGetLastError();
      c->hip_err.clear();
      uq_units = 0;
    }
  }
  if (c->enc.guest_blocks > 0) {
    if ((rc = ensure(c, c->d_gtables, (size_t)c->enc.guest_blocks * kTableSize * 2 + 64))) return rc;
    if ((rc = ensure(c, c->d_queue, 64))) return rc;
    // words: [0..1] stream queues (single-, multi-window), [2..3] the guests' queues of a fixed
    // profiling split, [4..5] what the LDS-table launches took, [6..7] window-unit head / tail
    // [8] the queue of the streams with a preset dictionary
    HIP_TRY(c, hipMemsetAsync(c->d_queue.p, 0, 40, c->stream));
  }
#if defined(FLATE_LZ_STAMPS) || defined(FLATE_LZ_FINISH)
  if ((rc = ensure(c, c->d_debug, (size_t)pl.n_chunks * 64 + 64))) return rc;
  HIP_TRY(c, hipMemsetAsync(c->d_debug.p, 0, (size_t)pl.n_chunks * 64, c->stream));
  P.debug = (uint64_t *)c->d_debug.p;
  c->debug_chunks = pl.n_chunks;
#endif
  {
    StageTimer t(c, FLATE_HIP_STAGE_LZ77);
    if (flags & FLATE_HIP_LZ_SERIAL) {
      if (!pl.ids16.empty()) {
        P.stream_ids = (const uint32_t *)c->d_ids16.p;
        hipLaunchKernelGGL(lz77_serial_kernel, dim3((uint32_t)pl.ids16.size()), dim3(64), 0,
                           c->stream, P);
      }
      if (!pl.ids32.empty()) {
        P.stream_ids = (const uint32_t *)c->d_ids32.p;
        hipLaunchKernelGGL(lz77_serial_kernel, dim3((uint32_t)pl.ids32.size()), dim3(64), 0,
                           c->stream, P);
      }
    } else {
      // single-window streams (ids16) and multi-window streams (ids32) use the same 32 KiB
      // 16-bit tables; the latter add the periodic sweep (MULTI)
      // a persistent launch: the blocks of both kernels take their streams from word `queue_word` of d_queue
      auto queued = [&](LzParams X, uint32_t queue_word, uint32_t count) {
        X.gtables = c->d_gtables.p;
        X.gtable_blocks = (uint32_t)c->enc.guest_blocks;  // d_gtables holds exactly this many tables
        X.queue = (uint32_t *)c->d_queue.p + queue_word;
        X.queue_end = count;
        return X;
      };
      auto launch = [&](const DevBuf &ids, uint32_t count, bool multi, uint32_t queue_slot, bool pair) {
        if (!count) return;
        P.stream_ids = (const uint32_t *)ids.p;
        void (*wave)(LzParams) = hooks ? (multi ? lz77_wave_kernel<true, true> : lz77_wave_kernel<false, true>)
                                       : (multi ? lz77_wave_kernel<true, false> : lz77_wave_kernel<false, false>);
        void (*guest)(LzParams) = hooks ? (multi ? lz77_guest_kernel<true, true> : lz77_guest_kernel<false, true>)
                                        : (multi ? lz77_guest_kernel<true, false> : lz77_guest_kernel<false, false>);
        if (!pair) {
          hipLaunchKernelGGL(wave, dim3(count), dim3(64), 0, c->stream, P);
          return;
        }
        LzParams G = queued(P, queue_slot, count);
        c->last_count[queue_slot] = count;
        if (multi && uq_units) {
          G.uq_ready = (uint32_t *)c->d_uq_ready.p;
          G.uq_ctr = (uint32_t *)c->d_queue.p + 6;  // {head, tail}
          G.uq_units = uq_units;
          G.uq_tables = (uint16_t *)c->d_uq_tables.p;
          G.uq_sweep = (uint32_t *)c->d_uq_sweep.p;
          c->last_count[queue_slot] = uq_units;
          hipLaunchKernelGGL(uq_init_kernel, dim3((uq_units + 255) / 256), dim3(256), 0, c->stream,
                             G.uq_ready, G.uq_ctr, count, uq_units);
        }
        LzParams R = G;  // the LDS-table launch counts what it takes
        R.taken = (uint32_t *)c->d_queue.p + 4 + queue_slot;
        if (c->enc.profile_split > 0 && c->enc.profile_split < count && !G.uq_ready) {
          // measurement aid: a fixed split instead of the shared queue, so that a profiler that
          // serialises the two kernels still sees each of them do its share of the work
          R.queue_end = c->enc.profile_split;
          G.queue = (uint32_t *)c->d_queue.p + 2 + queue_slot;
          G.stream_ids = P.stream_ids + c->enc.profile_split;
          G.queue_end = count - c->enc.profile_split;
        }
        launch_pair(c, wave, guest, count, R, G);
      };
      launch(c->d_ids16, (uint32_t)pl.ids16.size(), false, 0, rt.pair16);
      launch(c->d_ids32, (uint32_t)pl.ids32.size(), true, 1, rt.pair32);
      if (!pl.idsD.empty()) {
        // Streams with a preset dictionary: every used dictionary is primed once (one wavefront each), then the
        // dictionary builds of the stream kernels run the payloads as windows 1, 2, ... (whole-stream scheduling)
        const uint32_t count = (uint32_t)pl.idsD.size();
        LzParams Q = P;
        Q.stream_ids = (const uint32_t *)c->d_idsD.p;
        Q.win0 = 1;
        hipLaunchKernelGGL(lz77_dict_prime_kernel, dim3(DD->n_slots), dim3(64), 0, c->stream, Q, DD->dev);
        void (*wave_d)(LzParams, LzDictParams) = hooks ? lz77_wave_dict_kernel<true> : lz77_wave_dict_kernel<false>;
        void (*guest_d)(LzParams, LzDictParams) = hooks ? lz77_guest_dict_kernel<true> : lz77_guest_dict_kernel<false>;
        if (!rt.pairD) {
          hipLaunchKernelGGL(wave_d, dim3(count), dim3(64), 0, c->stream, Q, DD->dev);
        } else {
          Q = queued(Q, 8, count);
          launch_pair(c, wave_d, guest_d, count, Q, Q, DD->dev);
        }
      }
    }
  }
  // (test hook: it loses one hand-over of THIS launch, not of every later one)
  if (uq_units) c->inject_drop_push = 0;
  HIP_TRY(c, hipGetLastError());
  return FLATE_HIP_OK;
}

// The entropy stage's scratch for n_blocks blocks over in_bytes bytes of input, and the sizes and places of n streams
// (the batch driver's and the stream writer's: a piece of a stream asks for n = 3, the four slots it has always had).
int ensure_entropy_scratch(flate_hip_ctx *c, uint32_t n_blocks, uint64_t in_bytes, uint32_t n) {
  const size_t nb = (size_t)n_blocks + 1;
  int rc;
  if ((rc = ensure(c, c->d_blk_hist, nb * 320 * 4))) return rc;
  if ((rc = ensure(c, c->d_blk_cl, nb * 320 * 4))) return rc;
  if ((rc = ensure(c, c->d_blk_hdr, nb * 704 * 4))) return rc;
  if ((rc = ensure(c, c->d_blk_meta, nb * 16))) return rc;
  if ((rc = ensure(c, c->d_tile_meta, ((in_bytes >> 8) + nb + 2) * 64))) return rc;  // (tile_meta_at)
  if ((rc = ensure(c, c->d_out_len, (size_t)n * 8 + 8))) return rc;
  return ensure(c, c->d_out_off, ((size_t)n + 1) * 8);
}

// The result of a call without input: `len` fixed bytes to the caller's memory, host or device.
int emit_fixed(flate_hip_ctx *c, uint8_t *out, uint64_t out_cap, const uint8_t *bytes, uint64_t len, uint32_t flags) {
  if (out_cap < len) return FLATE_HIP_E_OUT_TOO_SMALL;
  if (flags & FLATE_HIP_DEVICE_PTRS) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(out, bytes, len, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  } else {
    memcpy(out, bytes, len);
  }
  return FLATE_HIP_OK;
}

// ---- the entropy stage ----

// The stage's index arrays (entropy_ctl_up, deflate_plan.h): blk_base, and for the per-block form the stream of every
// block.  Both go up in front of the match finder.
int blk_base_up(flate_hip_ctx *c, const StagePlan &pl) {
  const size_t bytes = ((size_t)pl.n_streams + 1) * 4;
  const int rc = ensure(c, c->d_blk_base, bytes);
  return rc ? rc : ctl_up(c, c->d_blk_base.p, pl.blk_base.data(), bytes);
}
int blk_sid_up(flate_hip_ctx *c, const StagePlan &pl) {
  int rc;
  std::vector<uint32_t> blk_sid(pl.n_blocks);
  for (uint32_t i = 0; i < pl.n_streams; ++i)
    for (uint32_t b = pl.blk_base[i]; b < pl.blk_base[i + 1]; ++b) blk_sid[b] = i;
  if ((rc = ensure(c, c->d_blk_sid, (size_t)pl.n_blocks * 4 + 4))) return rc;
  return ctl_up(c, c->d_blk_sid.p, blk_sid.data(), (size_t)pl.n_blocks * 4);
}

// The kernels of the entropy stage over the streams of H, inside the stage's events: histograms and codes, the scan
// that places the streams (a raw batch, a batch of members -- F, null for raw output -- or one spliced stream), pack.
// place_cap: the room the scan may give out.
// ZW (flate_hip_zip_write): the members of a ZIP archive, placed by zip_scan_kernel.
// GP (a grouped call): several spliced streams, placed by group_scan_kernel.
void launch_entropy(flate_hip_ctx *c, const EncodeRoute &rt, const HuffParams &H, uint32_t n_blocks, const FrameParams *F,
                    uint64_t place_cap, const ZipWriteParams *ZW = nullptr, const GroupParams *GP = nullptr) {
  const uint32_t n = H.n_streams;
  StageTimer t(c, FLATE_HIP_STAGE_HUFF_PACK);
  if (rt.per_block)
    hipLaunchKernelGGL(huff_hist_block_kernel, dim3(n_blocks), dim3(64), 0, c->stream, H);
  else
    hipLaunchKernelGGL(huff_hist_kernel, dim3(n), dim3(64), 0, c->stream, H);
  hipLaunchKernelGGL(huff_code_kernel, dim3(n), dim3(64), 0, c->stream, H);
  if (GP) {
    hipLaunchKernelGGL(group_scan_kernel, dim3(1), dim3(1024), 0, c->stream, *GP);
    hipLaunchKernelGGL(group_zero_kernel, dim3((uint32_t)(((uint64_t)n + GP->n_groups) / 256 + 1)), dim3(256), 0, c->stream, *GP,
                       H.out);
  } else if (H.spliced) {
    SpliceParams S{};
    S.sum = (const uint64_t *)c->d_slot_off.p;
    S.stream_bit = (uint64_t *)c->d_out_off.p;
    S.total_bytes = (uint64_t *)c->d_out_len.p + n;  // (d_out_len has n + 1 slots)
    S.out_cap = place_cap;
    S.status = (int *)c->d_status.p;
    S.n_streams = n;
    hipLaunchKernelGGL(splice_scan_kernel, dim3(1), dim3(1024), 0, c->stream, S);
    hipLaunchKernelGGL(splice_zero_kernel, dim3(n / 256 + 1), dim3(256), 0, c->stream, S, H.out);
  } else if (F) {
    hipLaunchKernelGGL(frame_scan_kernel, dim3(1), dim3(1024), 0, c->stream, *F);
  } else if (ZW) {
    hipLaunchKernelGGL(zip_scan_kernel, dim3(1), dim3(1024), 0, c->stream, *ZW);
  } else {
    CompactParams C{};
    C.out_len = (const uint64_t *)c->d_out_len.p;
    C.out_off = (uint64_t *)c->d_out_off.p;
    C.out_cap = place_cap;
    C.n_streams = n;
    C.status = (int *)c->d_status.p;
    hipLaunchKernelGGL(scan_sizes_kernel, dim3(1), dim3(1024), 0, c->stream, C);
  }
  if (rt.per_block) {
    hipLaunchKernelGGL(huff_zero_edges_kernel, dim3(n_blocks / 256 + 1), dim3(256), 0, c->stream, H, n_blocks);
    hipLaunchKernelGGL(huff_pack_block_kernel, dim3(n_blocks), dim3(64), 0, c->stream, H);
  } else {
    hipLaunchKernelGGL(GP ? huff_pack_grouped_kernel : huff_pack_kernel, dim3(n), dim3(64), 0, c->stream, H);
  }
}

// ---- the container of a *_framed call ----
// Every stream -- spliced: the one stream -- lies inside its container: the scan that places the streams adds header
// and trailer, the pack kernels write each raw stream into its member, then the checksum kernels run on the input where
// it is and frame_write_kernel writes headers and trailers.  sum_off / sum_n: what the checksum kernels sum -- the
// streams, or the one stream.

// frame_before: dict_of, the DICTIDs' checksums
CtlBytes frame_before_ctl(const FrameReq &FR, uint32_t n) {
  // (n_dicts == 0: every dict_of entry is FLATE_HIP_NO_DICT and dict_off may be null -- dict_args_ok)
  return {frame_before_ctl_up(n, FR.dict_of ? dictid_ctl_up_bytes(FR.dict_off, FR.n_dicts) : 0), 0};
}

// In front of the match finder, outside the checksum stage's events: the container's arrays and the DICTIDs.
int frame_before(flate_hip_ctx *c, const FrameReq &FR, uint32_t n, const uint64_t *sum_off, uint32_t sum_n, uint32_t flags) {
  int rc;
  if ((rc = ensure(c, c->d_frame_off, ((size_t)n + 1) * 8))) return rc;
  if ((rc = ensure(c, c->d_frame_sums, (size_t)n * 4 + 8))) return rc;
  if (!FR.dict_of) return FLATE_HIP_OK;
  if ((rc = ensure(c, c->d_frame_dict_of, (size_t)n * 4 + 4))) return rc;
  // the DICTIDs' checksums and the streams' (frame_after) carve slot 0 of the scratch: sized once here for the larger, so
  // that the second cannot grow it (a hipFree, which drains the device) inside the timed stage
  const size_t a = dictid_scratch_bytes(FR.dict_off, FR.n_dicts), b = checksum_scratch_bytes(sum_off, sum_n);
  void *unused = nullptr;
  if ((rc = ctx_scratch(c, 0, a > b ? a : b, &unused))) return rc;
  if ((rc = ctl_up(c, c->d_frame_dict_of.p, FR.dict_of, (size_t)n * 4))) return rc;
  // (DICTID is the Adler-32 of the whole dictionary: the tails of dict_upload are not enough)
  return dictid_stage(c, FR.dicts, FR.dict_off, FR.n_dicts, flags);
}

// one_len: the bytes of the one spliced stream's input
FrameParams frame_params(const flate_hip_ctx *c, const FrameReq &FR, const EncCall &A, uint8_t *d_out, uint64_t one_len) {
  FrameParams F{};
  F.out_len = (const uint64_t *)c->d_out_len.p + (A.spliced ? A.n : 0u);  // (spliced: total_bytes of splice_scan_kernel)
  F.member_off = A.spliced ? nullptr : (uint64_t *)c->d_frame_off.p;
  F.payload_off = (uint64_t *)c->d_out_off.p;
  F.in_off = (const uint64_t *)c->d_in_off.p;
  F.one_len = one_len;
  F.sums = (const uint32_t *)c->d_frame_sums.p;
  F.dict_of = FR.dict_of ? (const uint32_t *)c->d_frame_dict_of.p : nullptr;
  F.dict_id = (const uint32_t *)c->d_frame_ids.p;
  F.out = d_out;
  F.out_cap = A.out_cap;
  F.n_streams = A.n;
  F.wrap = FR.wrap;
  F.status = (int *)c->d_status.p;
  return F;
}

// frame_after: the streams' checksums
CtlBytes frame_after_ctl(const uint64_t *sum_off, uint32_t sum_n) { return {checksum_ctl_up_bytes(sum_off, sum_n), 0}; }

// Behind the pack kernel (its spliced form works on whole dwords around the stream): the checksums, headers and trailers.
int frame_after(flate_hip_ctx *c, const FrameReq &FR, const FrameParams &F, const uint8_t *d_in, const uint64_t *sum_off,
                uint32_t sum_n) {
  StageTimer t(c, FLATE_HIP_STAGE_CHECKSUM);
  const int rc = checksum_device(c, d_in, sum_off, sum_n, frame_sum_kind(FR.wrap), (uint32_t *)c->d_frame_sums.p, -1);
  if (rc) return rc;
  hipLaunchKernelGGL(frame_write_kernel, dim3(sum_n / 256 + 1), dim3(256), 0, c->stream, F);
  return FLATE_HIP_OK;
}

// A grouped call's members: the checksums of the groups' input, then group_frame_write_kernel.
int group_frame_after(flate_hip_ctx *c, const FrameReq &FR, const GroupParams &GP, uint8_t *d_out, const uint8_t *d_in,
                      const uint64_t *sum_off, uint32_t sum_n) {
  StageTimer t(c, FLATE_HIP_STAGE_CHECKSUM);
  const int rc = checksum_device(c, d_in, sum_off, sum_n, frame_sum_kind(FR.wrap), (uint32_t *)c->d_frame_sums.p, -1);
  if (rc) return rc;
  GroupFrameParams G{};
  G.member_off = GP.member_off;
  G.payload_off = GP.payload_off;
  G.end_bit = GP.end_bit;
  G.group_off = GP.group_off;
  G.in_off = (const uint64_t *)c->d_in_off.p;
  G.sums = (const uint32_t *)c->d_frame_sums.p;
  G.out = d_out;
  G.out_cap = GP.out_cap;
  G.n_groups = sum_n;
  G.wrap = FR.wrap;
  G.status = GP.status;
  hipLaunchKernelGGL(group_frame_write_kernel, dim3(sum_n / 256 + 1), dim3(256), 0, c->stream, G);
  return FLATE_HIP_OK;
}

// ---- the container of flate_hip_zip_write (zip_kernels.hip) ----
// The members of a ZIP archive: zip_scan_kernel places them (30 + name in front of every raw stream), the pack kernels
// write each raw stream into its member, then the CRC-32s run on the input where it is and zip_write_kernel writes the
// local headers, the central directory and the end records.
struct ZipReq {
  const uint8_t *names;      // HOST
  const uint64_t *name_off;  // HOST, n + 1
};

// zip_after: the entries' checksums; down: the archive's size
CtlBytes zip_ctl(const uint64_t *sum_off, uint32_t sum_n) { return {checksum_ctl_up_bytes(sum_off, sum_n), 64}; }

// In front of the match finder: the container's arrays, the names on the device.
int zip_before(flate_hip_ctx *c, const ZipReq &ZR, uint32_t n) {
  int rc;
  const uint64_t name_bytes = ZR.name_off[n];
  if ((rc = ensure(c, c->d_frame_off, ((size_t)n + 1) * 8))) return rc;
  if ((rc = ensure(c, c->d_frame_sums, (size_t)n * 4 + 8))) return rc;
  if ((rc = ensure(c, c->d_zip_names, name_bytes + 16))) return rc;
  if ((rc = ensure(c, c->d_zip_name_off, ((size_t)n + 1) * 8))) return rc;
  if ((rc = ensure(c, c->d_zip_whead, sizeof(ZipWriteHead)))) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->d_zip_names.p, ZR.names, name_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->d_zip_name_off.p, ZR.name_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
  return FLATE_HIP_OK;
}

// GP (entries written in pieces): the entries are its groups, placed by group_scan_kernel
ZipWriteParams zip_params(const flate_hip_ctx *c, const EncCall &A, uint8_t *d_out, const GroupParams *GP) {
  ZipWriteParams Z{};
  Z.out_len = GP ? nullptr : (const uint64_t *)c->d_out_len.p;
  Z.in_off = (const uint64_t *)c->d_in_off.p;
  Z.name_off = (const uint64_t *)c->d_zip_name_off.p;
  Z.names = (const uint8_t *)c->d_zip_names.p;
  Z.entry_off = (uint64_t *)c->d_frame_off.p;
  Z.payload_off = GP ? GP->payload_off : (uint64_t *)c->d_out_off.p;
  Z.group_off = GP ? GP->group_off : nullptr;
  Z.sums = (const uint32_t *)c->d_frame_sums.p;
  Z.out = d_out;
  Z.out_cap = A.out_cap;
  Z.n = GP ? GP->n_groups : A.n;
  Z.status = (int *)c->d_status.p;
  Z.head = (ZipWriteHead *)c->d_zip_whead.p;
  return Z;
}

// Behind the pack kernel: the CRC-32s, then headers, directory and end records.
int zip_after(flate_hip_ctx *c, const ZipWriteParams &ZW, const uint8_t *d_in, const uint64_t *sum_off, uint32_t sum_n) {
  StageTimer t(c, FLATE_HIP_STAGE_CHECKSUM);
  const int rc = checksum_device(c, d_in, sum_off, sum_n, FLATE_HIP_CHECKSUM_CRC32, (uint32_t *)c->d_frame_sums.p, -1);
  if (rc) return rc;
  hipLaunchKernelGGL(zip_write_kernel, dim3(sum_n / 256 + 1), dim3(256), 0, c->stream, ZW);
  return FLATE_HIP_OK;
}

// ---- the driver of the batch calls ----
// DD != NULL: the preset dictionaries of the streams whose encoder starts from one.
// FR != NULL (the *_framed calls; null: raw streams): the container, frame_before / frame_after.
// planned: the call's plan where the entry point has made it already (null: made here).
// ZR != NULL (flate_hip_zip_write): the ZIP container, zip_before / zip_after.
int deflate_common(flate_hip_ctx *c, const EncCall &A, const DeflDict *DD = nullptr, const FrameReq *FR = nullptr,
                   const StagePlan *planned = nullptr, const ZipReq *ZR = nullptr) {
  const uint32_t n = A.n;
  const bool dev = (A.flags & FLATE_HIP_DEVICE_PTRS) != 0;
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;

  // plan
  StagePlan made;
  if (!planned) {
    if ((rc = make_plan(A.in_off, n, made, A.flags, DD ? DD->has : nullptr))) return rc;
    planned = &made;
  }
  const StagePlan &pl = *planned;
  const bool grouped = A.group_off != nullptr;
  const uint32_t n_groups = A.n_groups;
  const EncodeRoute route = encode_route(pl, c->enc, A.flags, A.spliced, grouped);
  const uint64_t in_bytes = A.in_off[n];
  // a spliced member's fixed header and trailer; what the checksum kernels sum: the streams, or the one stream
  const uint32_t f_hl = FR ? frame_header_len(FR->wrap, false) : 0u;
  const uint32_t f_tl = FR ? frame_trailer_len(FR->wrap) : 0u;
  const uint64_t whole[2] = {A.in_off[0], A.in_off[n]};
  // (grouped: every group's input is contiguous; and every piece's group, for the kernels)
  std::vector<uint64_t> group_in;
  std::vector<uint32_t> piece_group;
  if (grouped) {
    group_in.resize((size_t)n_groups + 1);
    piece_group.resize(n);
    for (uint32_t g = 0; g < n_groups; ++g) {
      group_in[g] = A.in_off[A.group_off[g]];
      for (uint32_t i = A.group_off[g]; i < A.group_off[g + 1]; ++i) piece_group[i] = g;
    }
    group_in[n_groups] = A.in_off[n];
  }
  const uint64_t *sum_off = grouped ? group_in.data() : A.spliced ? whole : A.in_off;
  const uint32_t sum_n = grouped ? n_groups : A.spliced ? 1u : n;
  if (FR && A.spliced && !grouped && A.out_cap < (uint64_t)f_hl + f_tl) return FLATE_HIP_E_OUT_TOO_SMALL;
  CtlBytes ctl{lz77_ctl_up(pl) + entropy_ctl_up(pl), encode_ctl_down(n)};
  if (FR) {
    ctl += frame_before_ctl(*FR, n);
    ctl += frame_after_ctl(sum_off, sum_n);
  }
  if (ZR) ctl += zip_ctl(sum_off, sum_n);
  if (grouped) ctl += CtlBytes{grouped_ctl_up(n, n_groups) + (ZR ? (size_t)n_groups * 4 : 0), grouped_ctl_down(n, n_groups)};
  if ((rc = ctl_begin(c, ctl.up, ctl.down))) return rc;

  // stage the input
  const uint8_t *d_in = A.in;
  uint8_t *d_out = A.out;
  if (!dev) {
    if ((rc = ensure(c, c->d_in, in_bytes + 16))) return rc;
    if ((rc = ensure(c, c->d_out, A.out_cap + 16))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_in.p, A.in, in_bytes, hipMemcpyHostToDevice, c->stream));
    d_in = (const uint8_t *)c->d_in.p;
    d_out = (uint8_t *)c->d_out.p;
  }

  // the scratch of both stages
  if ((rc = ensure_entropy_scratch(c, pl.n_blocks, in_bytes, n))) return rc;
  if (A.spliced && (rc = ensure(c, c->d_slot_off, ((size_t)n + 1) * 16))) return rc;  // stream summaries {a, b}
  if ((rc = ensure_lz_scratch(c, pl.n_chunks))) return rc;
  if ((rc = blk_base_up(c, pl))) return rc;

  // the container in front of the match finder
  if (FR && (rc = frame_before(c, *FR, n, sum_off, sum_n, A.flags))) return rc;
  if (ZR && (rc = zip_before(c, *ZR, grouped ? n_groups : n))) return rc;
  GroupParams GP{};
  if (grouped) {
    uint32_t *d_group_off = nullptr, *d_piece_group = nullptr, *d_header_len = nullptr;
    if ((rc = carve(c, c->d_group, [&](Carve &k) {
           k.take(d_group_off, (size_t)n_groups + 1);
           k.take(d_piece_group, n);
           k.take(d_header_len, ZR ? n_groups : 0u);
           k.take(GP.end_bit, n_groups);
           k.take(GP.payload_off, n_groups);
           k.take(GP.bit_idx, (size_t)n + n_groups);
         })))
      return rc;
    if ((rc = ensure(c, c->d_frame_off, ((size_t)n + 1) * 8))) return rc;
    if ((rc = ctl_up(c, d_group_off, A.group_off, ((size_t)n_groups + 1) * 4))) return rc;
    if ((rc = ctl_up(c, d_piece_group, piece_group.data(), (size_t)n * 4))) return rc;
    if (!A.bit_idx) GP.bit_idx = nullptr;
    if (ZR) {  // an entry's header: 30 + its name
      std::vector<uint32_t> header_len(n_groups);
      for (uint32_t g = 0; g < n_groups; ++g) header_len[g] = kZipLocalLen + (uint32_t)(ZR->name_off[g + 1] - ZR->name_off[g]);
      if ((rc = ctl_up(c, d_header_len, header_len.data(), (size_t)n_groups * 4))) return rc;
      GP.header_len = d_header_len;
      GP.zip_head = (ZipWriteHead *)c->d_zip_whead.p;
      GP.zip_name_off = (const uint64_t *)c->d_zip_name_off.p;
    }
    GP.sum = (const uint64_t *)c->d_slot_off.p;
    GP.group_off = d_group_off;
    GP.piece_group = d_piece_group;
    GP.header_len_all = f_hl;
    GP.trailer_len = f_tl;
    GP.stream_bit = (uint64_t *)c->d_out_off.p;
    GP.member_off = (uint64_t *)c->d_frame_off.p;
    GP.total_bytes = (uint64_t *)c->d_out_len.p + n;  // (d_out_len has n + 1 slots)
    GP.out_cap = A.out_cap;
    GP.slack = FR || ZR ? 0u : 3u;  // (a trailer or the directory behind the last closing block takes the pack kernel's last dword)
    GP.status = (int *)c->d_status.p;
    GP.n_pieces = n;
    GP.n_groups = n_groups;
  }

  // the match finder
  HIP_TRY(c, hipMemsetAsync(c->d_status.p, 0, 8, c->stream));  // (word 1: frame_scan_kernel's first oversized BGZF member)
  if (route.per_block && (rc = blk_sid_up(c, pl))) return rc;
  if ((rc = run_lz77(c, d_in, A.in_off, pl, route, A.flags, DD))) return rc;

  // the entropy stage
  HuffParams H = huff_params(c, A.flags, A.spliced);
  H.in = d_in;
  H.in_off = (const uint64_t *)c->d_in_off.p;
  H.chunk_base = (const uint32_t *)c->d_chunk_base.p;
  H.blk_base = (const uint32_t *)c->d_blk_base.p;
  // (batch members: the header lengths are in the offsets, frame_scan_kernel; grouped: in the bit positions)
  H.out = d_out + (A.spliced && !grouped ? f_hl : 0u);
  H.piece_group = GP.piece_group;
  H.group_end_bit = GP.end_bit;
  H.n_streams = n;
  H.blk_sid = route.per_block ? (const uint32_t *)c->d_blk_sid.p : nullptr;
  FrameParams F{};
  if (FR && !grouped) F = frame_params(c, *FR, A, d_out, whole[1] - whole[0]);
  // (a spliced member: header + stream + trailer <= out_cap is enough -- the 3 bytes the pack kernel's last dword may
  // reach past the stream lie in the trailer, which is written after it)
  ZipWriteParams ZW{};
  if (ZR) ZW = zip_params(c, A, d_out, grouped ? &GP : nullptr);
  launch_entropy(c, route, H, pl.n_blocks, FR && !grouped ? &F : nullptr,
                 FR && A.spliced ? A.out_cap - f_hl - f_tl + 3 : A.out_cap, ZR ? &ZW : nullptr, grouped ? &GP : nullptr);
  HIP_TRY(c, hipGetLastError());

  // the container behind it
  if (FR && !grouped && (rc = frame_after(c, *FR, F, d_in, sum_off, sum_n))) return rc;
  if (FR && grouped && (rc = group_frame_after(c, *FR, GP, d_out, d_in, sum_off, sum_n))) return rc;
  if (ZR && (rc = zip_after(c, ZW, d_in, sum_off, sum_n))) return rc;
  HIP_TRY(c, hipGetLastError());

  // read back
  uint64_t *out_off = A.out_off;
  if (grouped) {
    if ((rc = ctl_down(c, out_off, GP.member_off, ((size_t)n_groups + 1) * 8))) return rc;
    if (A.bit_idx && (rc = ctl_down(c, A.bit_idx, GP.bit_idx, ((size_t)n + n_groups) * 8))) return rc;
  } else if (out_off && (rc = ctl_down(c, out_off, ((FR && !A.spliced) || ZR) ? c->d_frame_off.p : c->d_out_off.p, ((size_t)n + 1) * 8)))
    return rc;
  if (A.spliced && !ZR && (rc = ctl_down(c, &c->h_total_bytes, (uint64_t *)c->d_out_len.p + n, 8))) return rc;
  if (ZR && (rc = ctl_down(c, &c->h_total_bytes, &ZW.head->total, 8))) return rc;
  if ((rc = ctl_down(c, &c->h_status_word, c->d_status.p, 4))) return rc;
  const bool bgzf = FR && frame_is_bgzf(FR->wrap);
  if (bgzf && (rc = ctl_down(c, &c->h_status_aux, (int *)c->d_status.p + 1, 4))) return rc;
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  ctl_finish(c);
  if (bgzf && c->h_status_word == FLATE_HIP_E_TOO_LARGE)
    c->hip_err = "BGZF: block " + std::to_string((uint32_t)c->h_status_aux) + " compresses to a member of more than 65536 bytes";
  if (c->h_status_word) return encoder_status(c, c->h_status_word);
  // (a BGZF file: the members, then the EOF marker frame_write_kernel has put behind them)
  const uint64_t produced = ZR || grouped ? c->h_total_bytes
                            : A.spliced  ? c->h_total_bytes + f_hl + f_tl
                                        : out_off[n] + (FR && FR->wrap == kWrapBgzf ? (uint64_t)kBgzfEofLen : 0ull);
  if (A.total_bytes) *A.total_bytes = produced;
  if (!dev) {
    HIP_TRY(c, hipMemcpyAsync(A.out, c->d_out.p, produced, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  const bool used[FLATE_HIP_STAGE_COUNT] = {true, true, FR != nullptr || ZR != nullptr, false};
  return collect_timing(c, used);
}

// The launch options of the parent, as they are now, for a lane's sub-context.
void lane_options(flate_hip_ctx *dst, const flate_hip_ctx *src) {
  dst->enc = src->enc;
  dst->profiling = src->profiling;
  dst->host_groups = 0;
}

// The streams are independent, so the bytes are those of one call over the whole batch.
// Group g is compressed on lane g % lanes into its own slot of the device output (the slots are
// sized by the groups' bounds: where a group's bytes end up in `out` depends on the sizes of the
// groups before it, which the host only learns as they finish); the calling thread takes the groups
// in order, fills the index and posts each group's bytes to the copy-out thread.
int deflate_host_pipelined(flate_hip_ctx *c, const EncCall &A, uint32_t G) {
  const uint8_t *in = A.in;
  const uint64_t *in_off = A.in_off;
  const uint32_t n = A.n;
  uint8_t *out = A.out;
  const uint64_t out_cap = A.out_cap;
  uint64_t *out_off = A.out_off;
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  const int lanes = c->host_lanes > 1 ? 2 : 1;
  for (int k = 0; k < lanes; ++k) {
    if (!c->lane[k] && (rc = flate_hip_init(c->device, &c->lane[k]))) return rc;
    lane_options(c->lane[k], c);
  }
  std::vector<uint32_t> lo(G + 1);
  std::vector<CopyJob> in_jobs(G);
  cut_by_bytes(in_off, nullptr, n, G, lo);  // equal BYTES per group: copy and compute stages stay balanced
  // device slots of the groups' output
  std::vector<uint64_t> slot(G + 1, 0);
  for (uint32_t g = 0; g < G; ++g) {
    uint64_t bound = 0;
    for (uint32_t i = lo[g]; i < lo[g + 1]; ++i) bound += flate_hip_deflate_bound((size_t)(in_off[i + 1] - in_off[i]));
    if (bound > out_cap) bound = out_cap;  // (a group that needs more than that fails the call anyway)
    slot[g + 1] = slot[g] + ((bound + 255) & ~255ull);
  }
  if ((rc = ensure(c, c->d_in, in_off[n] + 16))) return rc;
  if ((rc = ensure(c, c->d_out, slot[G] + 16))) return rc;
  if ((rc = host_pipe_streams(c))) return rc;
  uint8_t *d_in = (uint8_t *)c->d_in.p, *d_out = (uint8_t *)c->d_out.p;
  for (uint32_t g = 0; g < G; ++g)
    in_jobs[g] = {d_in + in_off[lo[g]], in + in_off[lo[g]], (size_t)(in_off[lo[g + 1]] - in_off[lo[g]])};
  const double t_call = host_now_ms();
  CopyPipe pipe(G, G);
  pipe.start(c->device, c->h2d_stream, c->d2h_stream, in_jobs);

  struct GroupResult {
    std::vector<uint64_t> off;
    int rc = FLATE_HIP_OK;
    bool done = false;
    bool threw = false;  // an exception was caught in the lane's thread
    float stage[FLATE_HIP_STAGE_COUNT] = {0, 0, 0, 0};
    std::string err;
  };
  std::vector<GroupResult> res(G);
  std::mutex mu;
  std::condition_variable cv;
  bool stop = false;
  auto run_lane = [&](int k) {
    flate_hip_ctx *lc = c->lane[k];
    std::vector<uint64_t> gin;
    for (uint32_t g = (uint32_t)k; g < G; g += (uint32_t)lanes) {
      GroupResult &r = res[g];
      {
        std::lock_guard<std::mutex> l(mu);
        if (stop) r.rc = FLATE_HIP_E_INTERNAL;
      }
      // (this is a worker thread: an exception that left it would end the process.  std::bad_alloc /
      // length_error from the vectors here or inside deflate_common are recorded instead; the calling thread
      // rethrows after the join, and its caller runs the batch as one pass, as before the lanes existed)
      try {
        if (r.rc == FLATE_HIP_OK && !pipe.wait_in(g)) r.rc = FLATE_HIP_E_HIP;
        const uint32_t cnt = lo[g + 1] - lo[g];
        r.off.assign((size_t)cnt + 1, 0);
        if (r.rc == FLATE_HIP_OK && cnt) {
          gin.resize((size_t)cnt + 1);
          const uint64_t base = in_off[lo[g]];
          for (uint32_t i = 0; i <= cnt; ++i) gin[i] = in_off[lo[g] + i] - base;
          lc->hip_err.clear();
          const double a = host_now_ms();
          r.rc = deflate_common(lc, {d_in + base, gin.data(), cnt, d_out + slot[g], slot[g + 1] - slot[g], r.off.data(),
                                     nullptr, A.flags | FLATE_HIP_DEVICE_PTRS, false});
          host_trace(t_call, "compute", g, a, host_now_ms());
          for (int s = 0; s < FLATE_HIP_STAGE_COUNT; ++s) r.stage[s] = lc->stage_ms[s];
          if (r.rc != FLATE_HIP_OK) r.err = lc->hip_err;
        }
      } catch (const std::exception &e) {
        r.rc = FLATE_HIP_E_INTERNAL;
        r.threw = true;
        try {
          r.err = std::string("host pipeline lane: ") + e.what();
        } catch (...) {
        }
      } catch (...) {
        r.rc = FLATE_HIP_E_INTERNAL;
        r.threw = true;
      }
      std::lock_guard<std::mutex> l(mu);
      r.done = true;
      if (r.rc != FLATE_HIP_OK) stop = true;
      cv.notify_all();
    }
  };
  // (the calling thread only collects; a thread that cannot be started ends the others before the
  // exception travels on to the caller, which then runs the batch as one pass)
  std::thread workers[2];
  try {
    for (int k = 0; k < lanes; ++k) workers[k] = std::thread(run_lane, k);
  } catch (...) {
    {
      std::lock_guard<std::mutex> l(mu);
      stop = true;
    }
    (void)pipe.finish();
    for (auto &w : workers)
      if (w.joinable()) w.join();
    throw;
  }

  float stage_sum[FLATE_HIP_STAGE_COUNT] = {0, 0, 0, 0};
  uint64_t at = 0;
  bool lane_threw = false;
  rc = FLATE_HIP_OK;
  out_off[0] = 0;
  for (uint32_t g = 0; g < G && rc == FLATE_HIP_OK; ++g) {
    GroupResult &r = res[g];
    {
      std::unique_lock<std::mutex> l(mu);
      cv.wait(l, [&] { return r.done; });
    }
    if (r.rc != FLATE_HIP_OK) {
      rc = r.rc;
      lane_threw = r.threw;
      if (c->hip_err.empty()) c->hip_err = r.err;
      break;
    }
    const uint32_t cnt = lo[g + 1] - lo[g];
    const uint64_t bytes = r.off[cnt];
    if (at + bytes > out_cap) {
      rc = FLATE_HIP_E_OUT_TOO_SMALL;
      break;
    }
    for (uint32_t i = 1; i <= cnt; ++i) out_off[lo[g] + i] = at + r.off[i];
    pipe.post_out(g, {out + at, d_out + slot[g], (size_t)bytes});
    at += bytes;
    for (int k = 0; k < FLATE_HIP_STAGE_COUNT; ++k) stage_sum[k] += r.stage[k];
  }
  {
    std::lock_guard<std::mutex> l(mu);
    if (rc != FLATE_HIP_OK) stop = true;
  }
  for (auto &w : workers)
    if (w.joinable()) w.join();
  const std::string err = pipe.finish();
  // A lane that threw may sit behind the group the collector stopped at (lane 1 throws in group 3 and raises `stop`
  // before lane 0 has started group 2: group 2 then carries E_INTERNAL without a message): look at every group.
  for (uint32_t g = 0; g < G; ++g)
    if (res[g].threw) {
      lane_threw = true;
      if (!res[g].err.empty()) c->hip_err = res[g].err;
      break;
    }
  if (lane_threw) {
    // the one-pass fallback reuses c->d_in / c->d_out: nothing of the lanes may still be writing there
    for (int k = 0; k < lanes; ++k) {
      (void)hipStreamSynchronize(c->lane[k]->stream);
      if (c->lane[k]->guest_stream) (void)hipStreamSynchronize(c->lane[k]->guest_stream);
    }
    throw std::runtime_error(c->hip_err);  // every thread has ended: the caller falls back to one pass
  }
  if (rc == FLATE_HIP_OK && !err.empty()) rc = FLATE_HIP_E_HIP;
  if (rc == FLATE_HIP_E_HIP && c->hip_err.empty()) c->hip_err = err;
  for (int k = 0; k < FLATE_HIP_STAGE_COUNT; ++k) c->stage_ms[k] = stage_sum[k];
  return rc;
}

// flate_hip_deflate_fast_batch after its checks (n > 0)
int deflate_batch_run(flate_hip_ctx *c, const EncCall &A) {
  const uint32_t G = encode_host_groups(c->enc, c->host_groups, c->host_group_streams, A.flags, A.n, A.in_off[A.n]);
  if (G <= 1) return deflate_common(c, A);
  StagePlan pl;  // validate the whole index before any group runs (the same checks as the one-call path)
  const int rc = make_plan(A.in_off, A.n, pl, A.flags);
  if (rc) return rc;
  try {
    return deflate_host_pipelined(c, A, G);
  } catch (const std::exception &e) {  // (no copy threads, out of host memory): one pass instead
    c->hip_err.clear();
  }
  return deflate_common(c, A, nullptr, nullptr, &pl);
}

}  // namespace

extern "C" {

// Worst case of one stream: every window Huffman-coded with matches (< 15 bits per
// byte), a <= 320-byte dynamic header per window, 5 bytes per stored block.
size_t flate_hip_deflate_bound(size_t n) {
  const size_t windows = n / kMaxStoreBlockSize + 1;
  return n * 2 + windows * 320 + 16;
}

int flate_hip_deflate_fast_batch(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off,
                                 uint32_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_off,
                                 uint32_t flags) {
  if (!c || !deflate_batch_ptrs_ok(in, in_off, n, out, out_off)) return FLATE_HIP_E_INVALID;
  c->hip_err.clear();
  if (n == 0) {
    out_off[0] = 0;
    return FLATE_HIP_OK;
  }
  return deflate_batch_run(c, {in, in_off, n, out, out_cap, out_off, nullptr, flags, false});
}

int flate_hip_deflate_fast_spliced(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off,
                                   uint32_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                                   uint64_t *bit_off, uint32_t flags) {
  if (!c || !deflate_spliced_ptrs_ok(in, in_off, n, out, out_len)) return FLATE_HIP_E_INVALID;
  c->hip_err.clear();
  if (n == 0) {  // nothing but the closing block of Writer::close
    static const uint8_t closing[5] = {0x01, 0x00, 0x00, 0xff, 0xff};
    const int rc = emit_fixed(c, out, out_cap, closing, sizeof closing, flags);
    if (rc) return rc;
    *out_len = sizeof closing;
    if (bit_off) bit_off[0] = 0;
    return FLATE_HIP_OK;
  }
  return deflate_common(c, {in, in_off, n, out, out_cap, bit_off, out_len, flags, true});
}

// ---- one long stream, written in pieces (Writer::write as the reference behaves: output leaves
// ---- while later input is still to come, deflate.mbt:280-294) ---------------------------------
}  // extern "C"

struct flate_hip_stream {
  flate_hip_ctx *ctx = nullptr;
  uint32_t flags = 0;
  DevBuf table, clock, hist, stage, io, out;  // io: {lz77 in_off[2], huff in_off[2]} (u64) + chunk/blk bases
  uint64_t abs = 0;        // bytes of the stream consumed so far (a multiple of 65535 until the end)
  uint64_t pos = 0;        // the same, counted from the stream's current origin (see rebase_at)
  uint64_t rebase_at = 1ull << 30;  // origin moved up when pos passes this (option stream_rebase_bytes)
  // DeflateFast.cur as the reference counts it (deflate-fast.mbt:107,115,156): 65535 at the start,
  // + the window's length after every encode; when it reaches buffer_reset (:55,130-132) shift_offsets
  // runs -- in MoonBit `prev` is always empty, so that CLEARS the table (:367-374); in Go
  // the offsets move down and every distance stays what it was
  int64_t ref_cur = kMaxStoreBlockSize;
  int64_t buffer_reset = 2147483647ll - 2 * kMaxStoreBlockSize;
  uint32_t carry_bits = 0; // bits of the last, incomplete output byte (0..7) ...
  uint8_t carry = 0;       // ... and their value
  bool closed = false;
  int err = 0;             // sticky (Compressor.err, deflate.mbt:74)
};

namespace {
constexpr uint64_t kHist = 32768;  // max_match_offset: what a later window can still reference

int stream_write_impl(flate_hip_stream *st, const uint8_t *in, uint64_t n, bool final, uint8_t *out,
                      uint64_t out_cap, uint64_t *out_len) {
  flate_hip_ctx *c = st->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  // Positions inside the kernels are 32-bit and counted from the stream's origin.  A long stream
  // moves its origin up (the reference's shift_offsets, deflate-fast.mbt:366-389: same distances,
  // smaller numbers), so its length is not limited; one piece is (< 1 GiB).
  if (n >= (1ull << 30)) return FLATE_HIP_E_TOO_LARGE;
  uint32_t rebase = 0;
  if (st->pos >= st->rebase_at && st->pos > (uint64_t)kMaxStoreBlockSize) {
    rebase = (uint32_t)(st->pos - (uint64_t)kMaxStoreBlockSize);  // new origin: one window in front
    st->pos = kMaxStoreBlockSize;
  }
  const uint64_t W0 = st->pos;
  const uint64_t full = n / kMaxStoreBlockSize, r = n % kMaxStoreBlockSize;
  const uint32_t nch = (uint32_t)(full + (r >= (uint64_t)kSmallLzMin ? 1 : 0));
  const uint32_t nblk = (uint32_t)(full + (r > 0 ? 1 : 0));
  const uint32_t win0 = (uint32_t)(W0 / kMaxStoreBlockSize);
  int rc;
  // device staging: [the last 32 KiB of what came before][the new bytes]
  if ((rc = ensure(c, st->table, kTableSize * 2 + 64))) return rc;
  if ((rc = ensure(c, st->clock, 64))) return rc;
  if ((rc = ensure(c, st->hist, kHist + 64))) return rc;
  if ((rc = ensure(c, st->stage, kHist + n + 64))) return rc;
  if ((rc = ensure(c, st->io, 256))) return rc;
  const uint64_t cap_need = flate_hip_deflate_bound(n) + 16;
  if ((rc = ensure(c, st->out, cap_need + 16))) return rc;
  uint8_t *stage = (uint8_t *)st->stage.p;
  if (W0) HIP_TRY(c, hipMemcpyAsync(stage, st->hist.p, kHist, hipMemcpyDeviceToDevice, c->stream));
  if (n) HIP_TRY(c, hipMemcpyAsync(stage + kHist, in, n, hipMemcpyHostToDevice, c->stream));
  // index arrays: the match finder sees the stream through a virtual base (absolute positions, the
  // table's mod-2^16 arithmetic needs them), the entropy stage sees the new bytes only
  uint64_t h_io[8] = {0, W0 + n, 0, n, 0, 0, 0, 0};
  uint32_t *h32 = reinterpret_cast<uint32_t *>(h_io + 4);
  h32[0] = 0; h32[1] = nch;   // chunk_base
  h32[2] = 0; h32[3] = nblk;  // blk_base
  HIP_TRY(c, hipMemcpyAsync(st->io.p, h_io, sizeof h_io, hipMemcpyHostToDevice, c->stream));
  const uint64_t *d_off_abs = (const uint64_t *)st->io.p, *d_off_loc = d_off_abs + 2;
  const uint32_t *d_chunk_base = (const uint32_t *)((const uint64_t *)st->io.p + 4), *d_blk_base = d_chunk_base + 2;
  if ((rc = ensure_lz_scratch(c, nch, 1))) return rc;
  HIP_TRY(c, hipMemsetAsync(c->d_status.p, 0, 4, c->stream));
  if (nch) {
    LzParams P = lz_params(c, st->flags);
    P.in = stage + kHist - W0;  // virtual: only positions >= W0 - 32768 are ever dereferenced
    P.in_off = d_off_abs;
    P.chunk_base = d_chunk_base;
    // One launch per run of windows between two shift_offsets of the reference (one launch, except
    // for the piece in which `cur` passes buffer_reset: window 32 766 of a Writer, then every 32 767).
    const bool forgets = !(st->flags & FLATE_HIP_COMPAT_GO);
    uint32_t k0 = 0;        // first window (of this piece) of the launch being collected
    bool forget0 = false;   // ... and whether it starts on a cleared table
    auto flush = [&](uint32_t k1) {
      if (k1 == k0) return;
      LzParams Q = P;
      Q.win0 = win0 + k0;
      Q.matches = P.matches + (size_t)k0 * kMatchCapPerChunk;  // the kernel indexes both by window - win0
      Q.chunk_nmatch = P.chunk_nmatch + k0;
      Q.chunk_ntok = P.chunk_ntok + k0;
      hipLaunchKernelGGL(lz77_resume_kernel, dim3(1), dim3(64), 0, c->stream, Q, (uint16_t *)st->table.p,
                         (uint32_t *)st->clock.p, k1 - k0, k0 == 0 ? rebase : 0u, forget0 ? 1u : 0u);
    };
    for (uint32_t k = 0; k < nch; ++k) {
      if (st->ref_cur >= st->buffer_reset) {  // deflate-fast.mbt:130-132
        st->ref_cur = kMaxMatchOffset + 1;    // :372,388
        if (forgets) {
          flush(k);
          k0 = k;
          forget0 = true;
        }
      }
      st->ref_cur += k < full ? (int64_t)kMaxStoreBlockSize : (int64_t)r;  // :156
    }
    flush(nch);
  } else if (rebase) {
    st->pos += rebase;  // (nothing ran: the table still counts from the old origin)
  }
  if ((rc = ensure_entropy_scratch(c, nblk, n, 3))) return rc;  // (four slots of sizes and places)
  if ((rc = ensure(c, c->d_slot_off, 4 * 16))) return rc;
  uint8_t *d_out = (uint8_t *)st->out.p;
  HuffParams H = huff_params(c, st->flags, true);
  H.in = stage + kHist;
  H.in_off = d_off_loc;
  H.chunk_base = d_chunk_base;
  H.blk_base = d_blk_base;
  H.out = d_out;
  H.n_streams = 1;
  H.no_close = final ? 0u : 1u;
  SpliceParams S{};
  S.sum = (const uint64_t *)c->d_slot_off.p;
  S.stream_bit = (uint64_t *)c->d_out_off.p;
  S.total_bytes = (uint64_t *)c->d_out_len.p + 1;
  S.out_cap = cap_need;
  S.status = (int *)c->d_status.p;
  S.n_streams = 1;
  S.start_bit = st->carry_bits;
  S.no_close = H.no_close;
  hipLaunchKernelGGL(huff_hist_kernel, dim3(1), dim3(64), 0, c->stream, H);
  hipLaunchKernelGGL(huff_code_kernel, dim3(1), dim3(64), 0, c->stream, H);
  hipLaunchKernelGGL(splice_scan_kernel, dim3(1), dim3(1024), 0, c->stream, S);
  hipLaunchKernelGGL(splice_zero_kernel, dim3(1), dim3(256), 0, c->stream, S, d_out);
  // the bits left over from the previous piece share the first byte with this piece's first block
  if (st->carry_bits) HIP_TRY(c, hipMemcpyAsync(d_out, &st->carry, 1, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(huff_pack_kernel, dim3(1), dim3(64), 0, c->stream, H);
  HIP_TRY(c, hipGetLastError());
  uint64_t h_pos[2] = {0, 0};  // {end bit of the piece, total bytes}
  HIP_TRY(c, hipMemcpyAsync(&h_pos[0], (uint64_t *)c->d_out_off.p + 1, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&h_pos[1], (uint64_t *)c->d_out_len.p + 1, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&c->h_status_word, c->d_status.p, 4, hipMemcpyDeviceToHost, c->stream));
  if (!final && n >= kHist)  // what the next piece may still reference
    HIP_TRY(c, hipMemcpyAsync(st->hist.p, stage + n, kHist, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->h_status_word) return encoder_status(c, c->h_status_word);
  const uint64_t whole = final ? h_pos[1] : (h_pos[0] >> 3);
  if (whole > out_cap) return FLATE_HIP_E_OUT_TOO_SMALL;
  if (whole) HIP_TRY(c, hipMemcpyAsync(out, d_out, whole, hipMemcpyDeviceToHost, c->stream));
  st->carry_bits = final ? 0u : (uint32_t)(h_pos[0] & 7u);
  if (st->carry_bits) HIP_TRY(c, hipMemcpyAsync(&st->carry, d_out + whole, 1, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (st->carry_bits) st->carry &= (uint8_t)((1u << st->carry_bits) - 1u);
  st->pos += n;
  st->abs += n;
  *out_len = whole;
  return FLATE_HIP_OK;
}
}  // namespace

extern "C" {

int flate_hip_stream_open(flate_hip_ctx *c, uint32_t flags, flate_hip_stream **out) {
  if (!c || !out || (flags & ~FLATE_HIP_COMPAT_GO)) return FLATE_HIP_E_INVALID;
  flate_hip_stream *st = new flate_hip_stream();
  st->ctx = c;
  st->flags = flags;
  st->rebase_at = c->stream_rebase;
  if (c->debug_buffer_reset > 0) st->buffer_reset = c->debug_buffer_reset;
  *out = st;
  return FLATE_HIP_OK;
}

void flate_hip_stream_free(flate_hip_stream *st) {
  if (!st) return;
  (void)hipSetDevice(st->ctx->device);
  delete st;
}

size_t flate_hip_stream_bound(size_t n) { return flate_hip_deflate_bound(n) + 8; }

int flate_hip_stream_write(flate_hip_stream *st, const uint8_t *in, uint64_t n, int final, uint8_t *out,
                           uint64_t out_cap, uint64_t *out_len) {
  if (!st || !out_len || (n && !in) || !out) return FLATE_HIP_E_INVALID;
  *out_len = 0;
  if (st->err) return st->err;
  if (st->closed) return FLATE_HIP_E_INVALID;
  // a piece that is not the last one is whole windows: the 65535-byte staging window of
  // Compressor::fill_store (deflate.mbt:222-229) is what enc_speed compresses at a time
  if (!final && (n == 0 || n % kMaxStoreBlockSize != 0)) return FLATE_HIP_E_INVALID;
  st->ctx->hip_err.clear();
  const int rc = stream_write_impl(st, in, n, final != 0, out, out_cap, out_len);
  if (rc != FLATE_HIP_OK && rc != FLATE_HIP_E_OUT_TOO_SMALL) st->err = rc;  // sticky, as Compressor.err
  if (rc == FLATE_HIP_E_OUT_TOO_SMALL) st->err = rc;  // (the piece's state is gone with the call)
  if (rc == FLATE_HIP_OK && final) st->closed = true;
  return rc;
}

// ---- one long stream, written in parts at the batch encoder's speed (one_writer_rule.h, one_writer_kernels.hip) ----
}  // extern "C"

// Between two calls the stream rests in the handle: on the device the carried byte, the running checksum, the lengths
// (OneWriterState) and the buffer the pack kernels write into; on the host the rule's three words (OneWriterHost).
struct flate_hip_one_writer {
  flate_hip_ctx *ctx = nullptr;
  uint32_t wrap = 0, flags = 0;
  uint64_t piece = 0;       // P as given (0: the default)
  DevBuf state, buf, idx;   // OneWriterState; the call's bytes; the call's index (bits of the raw stream)
  OneWriterHost s = one_writer_fresh();
};

namespace {

// a fresh stream: no carry, the sum of nothing
int one_writer_fresh_state(flate_hip_one_writer *w) {
  flate_hip_ctx *c = w->ctx;
  OneWriterState *st = (OneWriterState *)w->state.p;
  const uint32_t empty = w->wrap == FLATE_HIP_WRAP_ZLIB ? 1u : 0u;
  HIP_TRY(c, hipMemsetAsync(st, 0, sizeof(OneWriterState), c->stream));
  HIP_TRY(c, hipMemcpyAsync(&st->sum, &empty, 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  w->s = one_writer_fresh();
  return FLATE_HIP_OK;
}

// One call that launches: the pieces of the plan through the whole call's kernels into the handle's buffer, the
// writer's kernels around them, ONE read-back (the result words, and the index where it is asked for), the download
// for a host caller.
int one_writer_run(flate_hip_one_writer *w, const OneWriterPlan &plan, const uint8_t *in, uint8_t *out, uint64_t out_cap,
                   uint64_t *in_used, uint64_t *out_len, uint64_t *bit_off, uint32_t *n_pieces) {
  flate_hip_ctx *c = w->ctx;
  const uint32_t n = (uint32_t)plan.n_pieces, wrap = w->wrap, flags = w->flags;
  const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0, fin = plan.close != 0;
  const uint64_t P = one_writer_piece(w->piece), bytes = plan.in_used;
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;

  // plan: the pieces as the streams of a spliced call
  std::vector<uint64_t> in_off((size_t)n + 1);
  for (uint32_t i = 0; i < n; ++i) in_off[i] = (uint64_t)i * P;
  in_off[n] = bytes;
  StagePlan pl;
  if (n && (rc = make_plan(in_off.data(), n, pl, flags))) return rc;
  const EncodeRoute route = encode_route(pl, c->enc, flags, true);
  const uint64_t whole[2] = {0, bytes};
  const bool summed = wrap != FLATE_HIP_WRAP_RAW && bytes != 0;
  CtlBytes ctl{n ? lz77_ctl_up(pl) + entropy_ctl_up(pl) : 0, encode_ctl_down(n)};
  if (summed) ctl += frame_after_ctl(whole, 1);
  if ((rc = ctl_begin(c, ctl.up, ctl.down))) return rc;

  // the input, the handle's buffers, the scratch of both stages
  const uint8_t *d_in = in;
  if ((rc = stage_input(c, in, bytes, flags, &d_in))) return rc;
  const uint64_t cap = one_writer_bound(bytes, w->piece);
  if ((rc = ensure(c, w->buf, cap + 64))) return rc;  // (16-byte reads of the copy kernel behind the last byte)
  if ((rc = ensure(c, w->idx, ((size_t)n + 2) * 8))) return rc;
  if (n) {
    if ((rc = ensure_entropy_scratch(c, pl.n_blocks, bytes, n))) return rc;
    if ((rc = ensure(c, c->d_slot_off, ((size_t)n + 1) * 16))) return rc;
    if ((rc = ensure_lz_scratch(c, pl.n_chunks))) return rc;
    if ((rc = blk_base_up(c, pl))) return rc;
  }
  void *unused = nullptr;
  if (summed && (rc = ctx_scratch(c, 0, checksum_scratch_bytes(whole, 1), &unused))) return rc;
  OneWriterState *st = (OneWriterState *)w->state.p;
  uint8_t *buf = (uint8_t *)w->buf.p;
  OneWriterParams Q{};
  Q.st = st;
  Q.buf = buf;
  Q.stream_bit = (const uint64_t *)c->d_out_off.p;
  Q.bit_idx = (uint64_t *)w->idx.p;
  Q.status = (const int *)c->d_status.p;
  Q.start_bit = plan.start_bit;
  Q.in_used = bytes;
  Q.out_cap = out_cap;
  Q.n_pieces = n;
  Q.wrap = wrap;
  Q.header = plan.header;
  Q.close = plan.close;

  HIP_TRY(c, hipMemsetAsync(c->d_status.p, 0, 8, c->stream));
  if (n) {
    // the match finder and the entropy stage of the whole call; the scan starts at the carried bit, only a final call
    // closes, and the header or the carry goes in between the zero kernel and the pack kernel's OR
    if ((rc = run_lz77(c, d_in, in_off.data(), pl, route, flags))) return rc;
    HuffParams H = huff_params(c, flags, true);
    H.in = d_in;
    H.in_off = (const uint64_t *)c->d_in_off.p;
    H.chunk_base = (const uint32_t *)c->d_chunk_base.p;
    H.blk_base = (const uint32_t *)c->d_blk_base.p;
    H.out = buf;
    H.n_streams = n;
    H.no_close = fin ? 0u : 1u;
    SpliceParams S{};
    S.sum = (const uint64_t *)c->d_slot_off.p;
    S.stream_bit = (uint64_t *)c->d_out_off.p;
    S.total_bytes = (uint64_t *)c->d_out_len.p + n;  // (d_out_len has n + 1 slots)
    S.out_cap = cap + 8;
    S.status = (int *)c->d_status.p;
    S.n_streams = n;
    S.start_bit = plan.start_bit;
    S.no_close = H.no_close;
    StageTimer t(c, FLATE_HIP_STAGE_HUFF_PACK);
    hipLaunchKernelGGL(huff_hist_kernel, dim3(n), dim3(64), 0, c->stream, H);
    hipLaunchKernelGGL(huff_code_kernel, dim3(n), dim3(64), 0, c->stream, H);
    hipLaunchKernelGGL(splice_scan_kernel, dim3(1), dim3(1024), 0, c->stream, S);
    hipLaunchKernelGGL(splice_zero_kernel, dim3(n / 256 + 1), dim3(256), 0, c->stream, S, buf);
    hipLaunchKernelGGL(one_writer_begin_kernel, dim3(1), dim3(64), 0, c->stream, Q);
    hipLaunchKernelGGL(huff_pack_kernel, dim3(n), dim3(64), 0, c->stream, H);
  }
  HIP_TRY(c, hipGetLastError());
  if (summed) {  // the checksum of the consumed bytes, on the input where it lies
    StageTimer t(c, FLATE_HIP_STAGE_CHECKSUM);
    if ((rc = checksum_device(c, d_in, whole, 1, frame_sum_kind(wrap), &st->part_sum, -1))) return rc;
  }
  hipLaunchKernelGGL(one_writer_index_kernel, dim3(n / 256 + 1), dim3(256), 0, c->stream, Q);
  HIP_TRY(c, hipGetLastError());

  std::vector<uint64_t> index((size_t)n + 1);  // (allocated in front of the commit point)
  const uint32_t n_idx = n + (fin ? 1u : 0u);

  // THE COMMIT POINT: the one kernel that moves the handle's device words.  A failure of the runtime behind it leaves
  // them ahead of the host's, so it ends the handle -- sticky until reset.  (In front of it nothing of the handle's
  // state has been touched, and a call may be repeated.)
  auto dead = [&](int e) {
    ctl_finish(c);
    w->s.status = e;
    return e;
  };
  hipLaunchKernelGGL(one_writer_commit_kernel, dim3(1), dim3(64), 0, c->stream, Q, make_x2n());
  if (dev) {
    const uint64_t blocks = cap / (256u * 16u * 8u) + 1u;
    hipLaunchKernelGGL(one_writer_copy_kernel, dim3((uint32_t)(blocks < 4096u ? blocks : 4096u)), dim3(256), 0, c->stream, st, buf, out);
  }
  OneWriterResult R{};
  if ((rc = ctl_down(c, &R, &st->res, sizeof R))) return dead(rc);
  if (bit_off && n_idx && (rc = ctl_down(c, index.data(), w->idx.p, (size_t)n_idx * 8))) return dead(rc);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
    c->hip_err = "one writer: the call's kernels failed";
    return dead(FLATE_HIP_E_HIP);
  }
  ctl_finish(c);
  if (R.status == FLATE_HIP_E_OUT_TOO_SMALL) {  // (not sticky: the commit kernel has left the state alone)
    if (R.out_len <= out_cap) {
      c->hip_err = "one writer: the handle's buffer is smaller than the call's bytes";
      return FLATE_HIP_E_INTERNAL;
    }
    *out_len = R.out_len;
    return FLATE_HIP_E_OUT_TOO_SMALL;
  }
  if (R.status < 0) return w->s.status = encoder_status(c, R.status);
  if (R.out_len > cap) {
    c->hip_err = "one writer: more bytes than the bound";
    return w->s.status = FLATE_HIP_E_INTERNAL;
  }
  if (!dev && R.out_len &&
      (hipMemcpyAsync(out, buf, R.out_len, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
       hipStreamSynchronize(c->stream) != hipSuccess)) {
    c->hip_err = "one writer: the download failed";
    return w->s.status = FLATE_HIP_E_HIP;
  }
  const bool used[FLATE_HIP_STAGE_COUNT] = {n != 0, n != 0, summed, false};
  if ((rc = collect_timing(c, used))) return w->s.status = rc;
  w->s.started = 1u;
  w->s.carry_bits = fin ? 0u : (uint32_t)(R.end_bit & 7u);
  if (fin) w->s.status = FLATE_HIP_STREAM_END;
  *in_used = bytes;
  *out_len = R.out_len;
  *n_pieces = n;
  if (bit_off)
    for (uint32_t i = 0; i < n_idx; ++i) bit_off[i] = index[i];
  return fin ? FLATE_HIP_STREAM_END : FLATE_HIP_OK;
}

}  // namespace

extern "C" {

size_t flate_hip_one_writer_bound(size_t in_len, size_t piece_bytes) { return (size_t)one_writer_bound(in_len, piece_bytes); }

int flate_hip_one_writer_open(flate_hip_ctx *c, uint32_t wrap, uint64_t piece_bytes, uint32_t flags,
                              flate_hip_one_writer **out) {
  // every check before any HIP call
  if (one_writer_open_check(c, wrap, piece_bytes, flags, out)) return FLATE_HIP_E_INVALID;
  *out = nullptr;
  c->hip_err.clear();
  HIP_TRY(c, hipSetDevice(c->device));
  flate_hip_one_writer *w = new flate_hip_one_writer();
  w->ctx = c;
  w->wrap = wrap;
  w->flags = flags;
  w->piece = piece_bytes;
  int rc = ensure(c, w->state, sizeof(OneWriterState) + 64);
  if (rc == FLATE_HIP_OK) rc = one_writer_fresh_state(w);
  if (rc != FLATE_HIP_OK) {
    delete w;
    return rc;
  }
  *out = w;
  return FLATE_HIP_OK;
}

int flate_hip_one_writer_reset(flate_hip_one_writer *w) {
  if (!w) return FLATE_HIP_E_INVALID;
  flate_hip_ctx *c = w->ctx;
  c->hip_err.clear();
  HIP_TRY(c, hipSetDevice(c->device));
  return one_writer_fresh_state(w);
}

void flate_hip_one_writer_free(flate_hip_one_writer *w) {
  if (!w) return;
  (void)hipSetDevice(w->ctx->device);
  delete w;
}

int flate_hip_one_writer_write(flate_hip_one_writer *w, const uint8_t *in, uint64_t in_len, int final_in, uint8_t *out,
                               uint64_t out_cap, uint64_t *in_used, uint64_t *out_len, uint64_t *bit_off,
                               uint32_t *n_pieces) {
  // every check, and everything the rule decides, before any HIP call
  if (one_writer_write_check(w, in, in_len, out, out_cap, in_used, out_len, n_pieces)) return FLATE_HIP_E_INVALID;
  *in_used = 0, *out_len = 0, *n_pieces = 0;
  const OneWriterPlan plan = one_writer_plan(w->s, in_len, final_in != 0, w->piece, w->wrap);
  if (plan.action == kWriterReturn) return plan.status;
  if (plan.action == kWriterNothing) return FLATE_HIP_OK;
  flate_hip_ctx *c = w->ctx;
  c->hip_err.clear();
  try {
    return one_writer_run(w, plan, in, out, out_cap, in_used, out_len, bit_off, n_pieces);
  } catch (const std::exception &e) {  // (out of host memory in an index vector: nothing has been launched)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

int flate_hip_lz77_matches(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n,
                           uint32_t flags, uint32_t *n_chunks, uint64_t *n_recs_cap,
                           uint32_t *chunk_nmatch, uint64_t *chunk_rec_off, uint32_t *recs) {
  if (!c || !in_off || !n_chunks || !n_recs_cap) return FLATE_HIP_E_INVALID;
  c->hip_err.clear();
  StagePlan pl;
  int rc = make_plan(in_off, n, pl, flags);
  if (rc) return rc;
  *n_chunks = pl.n_chunks;
  *n_recs_cap = (uint64_t)pl.n_chunks * kMatchCapPerChunk;
  if (!recs) return FLATE_HIP_OK;
  if (!in || !chunk_nmatch || !chunk_rec_off) return FLATE_HIP_E_INVALID;
  if (pl.n_chunks == 0) return FLATE_HIP_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const bool dev = (flags & FLATE_HIP_DEVICE_PTRS) != 0;
  const uint8_t *d_in = in;
  if (!dev) {
    if ((rc = ensure(c, c->d_in, in_off[n] + 16))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_in.p, in, in_off[n], hipMemcpyHostToDevice, c->stream));
    d_in = (const uint8_t *)c->d_in.p;
  }
  HIP_TRY(c, hipMemsetAsync(c->d_status.p, 0, 4, c->stream));
  if ((rc = ctl_begin(c, lz77_ctl_up(pl), 64))) return rc;
  if ((rc = ensure_lz_scratch(c, pl.n_chunks))) return rc;
  if ((rc = run_lz77(c, d_in, in_off, pl, encode_route(pl, c->enc, flags, false), flags))) return rc;
  HIP_TRY(c, hipMemcpyAsync(chunk_nmatch, c->d_nmatch.p, (size_t)pl.n_chunks * 4,
                            hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&c->h_status_word, c->d_status.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->h_status_word) return encoder_status(c, c->h_status_word);
  for (uint32_t k = 0; k <= pl.n_chunks; ++k) chunk_rec_off[k] = (uint64_t)k * kMatchCapPerChunk;
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIP_TRY(c, hipMemcpyAsync(recs, c->d_matches.p, (size_t)pl.n_chunks * kMatchCapPerChunk * 8, kind,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const bool used[FLATE_HIP_STAGE_COUNT] = {true, false, false, false};
  return collect_timing(c, used);
}

#if defined(FLATE_LZ_STAMPS) || defined(FLATE_LZ_FINISH)
// diagnostic builds only: per-chunk phase cycle sums (or start / finish times) of the last match-finder launch
int flate_hip_debug_lz_stamps(flate_hip_ctx *c, uint64_t *out, uint32_t max_chunks) {
  uint32_t k = c->debug_chunks < max_chunks ? c->debug_chunks : max_chunks;
  if (hipMemcpy(out, c->d_debug.p, (size_t)k * 64, hipMemcpyDeviceToHost) != hipSuccess) return -3;
  return (int)k;
}
#endif

}  // extern "C"

// flate_hip_deflate_fast_batch_dict; wrap != FLATE_HIP_WRAP_RAW: flate_hip_deflate_fast_batch_framed with dictionaries
// (zlib members, the streams that name a dictionary with FDICT and its DICTID)
static int deflate_batch_dict_run(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n,
                                  const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts,
                                  const uint32_t *dict_of, uint8_t *out, uint64_t out_cap, uint64_t *out_off,
                                  uint32_t flags, uint32_t wrap) {
  // every check before any HIP call
  if (!c || !deflate_batch_ptrs_ok(in, in_off, n, out, out_off)) return FLATE_HIP_E_INVALID;
  if (!dict_args_ok(dicts, dict_off, n_dicts, dict_of, n)) return FLATE_HIP_E_INVALID;
  const EncCall A{in, in_off, n, out, out_cap, out_off, nullptr, flags, false};
  const bool framed = wrap != FLATE_HIP_WRAP_RAW;
  std::vector<uint32_t> every0;  // dict_of == NULL: every stream uses dictionary 0
  if (framed && !dict_of) every0.assign(n, 0u);
  const FrameReq FRv{wrap, dict_of ? dict_of : every0.data(), dicts, dict_off, n_dicts};
  const FrameReq *FR = framed ? &FRv : nullptr;
  // DeflateFast::encode(d) over the last 32768 bytes of the dictionary; under 17 bytes that call is the
  // small-input path (deflate-fast.mbt:136-140) and leaves nothing behind
  const DictSlots S = dict_slots(dict_off, n_dicts, dict_of, n, (uint32_t)kSmallHuffMin);
  if (S.at.empty()) {  // no stream's encoder has seen a dictionary: the plain call, its kernels and its bytes
    if (!framed) return flate_hip_deflate_fast_batch(c, in, in_off, n, out, out_cap, out_off, flags);
    c->hip_err.clear();
    if (n == 0) {
      out_off[0] = 0;
      return FLATE_HIP_OK;
    }
    return deflate_common(c, A, nullptr, FR);
  }
  if (flags & FLATE_HIP_LZ_SERIAL) return FLATE_HIP_E_INVALID;  // (the single-lane kernel has no dictionary build)
  std::vector<uint8_t> has(n);
  for (uint32_t i = 0; i < n; ++i) has[i] = S.slot_of[i] != DictSlots::kNone;
  StagePlan pl;  // the whole index, before the context is touched
  int rc = make_plan(in_off, n, pl, flags, has.data());
  if (rc) return rc;
  c->hip_err.clear();
  const uint32_t n_slots = (uint32_t)S.at.size();
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = dict_upload(c, S, dicts, dict_off, flags))) return rc;
  if ((rc = ensure(c, c->d_dict_at, (size_t)n_slots * 8))) return rc;
  if ((rc = ensure(c, c->d_dict_len, (size_t)n_slots * 4))) return rc;
  if ((rc = ensure(c, c->d_lz_slot_of, (size_t)n * 4))) return rc;
  if ((rc = ensure(c, c->d_lz_tables, (size_t)n_slots * kTableSize * 2))) return rc;
  if ((rc = ensure(c, c->d_lz_clocks, (size_t)n_slots * 4))) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->d_dict_at.p, S.at.data(), (size_t)n_slots * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->d_dict_len.p, S.len.data(), (size_t)n_slots * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->d_lz_slot_of.p, S.slot_of.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  DeflDict DD{};
  DD.dev.dict_buf = (const uint8_t *)c->d_dicts.p;
  DD.dev.dict_at = (const uint64_t *)c->d_dict_at.p;
  DD.dev.dict_len = (const uint32_t *)c->d_dict_len.p;
  DD.dev.slot_of = (const uint32_t *)c->d_lz_slot_of.p;
  DD.dev.tables = (uint16_t *)c->d_lz_tables.p;
  DD.dev.clocks = (uint32_t *)c->d_lz_clocks.p;
  DD.n_slots = n_slots;
  DD.has = has.data();
  // (host pointers: one copy in, compress, one copy out -- the pipelined host path is the plain call's)
  return deflate_common(c, A, &DD, FR, &pl);
}

extern "C" {

int flate_hip_deflate_fast_batch_dict(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n,
                                      const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts,
                                      const uint32_t *dict_of, uint8_t *out, uint64_t out_cap, uint64_t *out_off,
                                      uint32_t flags) {
  return deflate_batch_dict_run(c, in, in_off, n, dicts, dict_off, n_dicts, dict_of, out, out_cap, out_off, flags,
                                FLATE_HIP_WRAP_RAW);
}

size_t flate_hip_frame_overhead(uint32_t wrap, int with_dict) {
  if (wrap != FLATE_HIP_WRAP_ZLIB && wrap != FLATE_HIP_WRAP_GZIP) return 0;
  return frame_header_len(wrap, with_dict != 0) + frame_trailer_len(wrap);
}

int flate_hip_deflate_fast_batch_framed(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n,
                                        uint32_t wrap, const uint8_t *dicts, const uint64_t *dict_off,
                                        uint32_t n_dicts, const uint32_t *dict_of, uint8_t *out, uint64_t out_cap,
                                        uint64_t *out_off, uint32_t flags) {
  // every check before any HIP call
  if (!c || wrap > FLATE_HIP_WRAP_GZIP) return FLATE_HIP_E_INVALID;
  const bool with_dicts = dicts || n_dicts || dict_of;
  if (with_dicts && wrap == FLATE_HIP_WRAP_GZIP) return FLATE_HIP_E_INVALID;  // (RFC 1952 has no preset dictionary)
  try {
    if (with_dicts)
      return deflate_batch_dict_run(c, in, in_off, n, dicts, dict_off, n_dicts, dict_of, out, out_cap, out_off, flags, wrap);
    if (wrap == FLATE_HIP_WRAP_RAW) return flate_hip_deflate_fast_batch(c, in, in_off, n, out, out_cap, out_off, flags);
    if (!deflate_batch_ptrs_ok(in, in_off, n, out, out_off)) return FLATE_HIP_E_INVALID;
    c->hip_err.clear();
    if (n == 0) {
      out_off[0] = 0;
      return FLATE_HIP_OK;
    }
    // (host pointers: one copy in -- the checksums run on it --, compress, one copy out)
    const FrameReq FR{wrap, nullptr, nullptr, nullptr, 0};
    return deflate_common(c, {in, in_off, n, out, out_cap, out_off, nullptr, flags, false}, nullptr, &FR);
  } catch (const std::exception &e) {  // (out of host memory in an index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

int flate_hip_deflate_fast_spliced_framed(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n,
                                          uint32_t wrap, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                                          uint64_t *bit_off, uint32_t flags) {
  if (!c || wrap > FLATE_HIP_WRAP_GZIP) return FLATE_HIP_E_INVALID;
  if (wrap == FLATE_HIP_WRAP_RAW) return flate_hip_deflate_fast_spliced(c, in, in_off, n, out, out_cap, out_len, bit_off, flags);
  if (!deflate_spliced_ptrs_ok(in, in_off, n, out, out_len)) return FLATE_HIP_E_INVALID;
  c->hip_err.clear();
  if (n == 0) {  // header, the closing block of Writer::close, the trailer of nothing
    static const uint8_t zmember[11] = {0x78, 0x01, 0x01, 0x00, 0x00, 0xff, 0xff, 0, 0, 0, 1};
    static const uint8_t gmember[23] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 4, 255, 0x01, 0x00, 0x00, 0xff, 0xff};
    const uint8_t *m = wrap == FLATE_HIP_WRAP_ZLIB ? zmember : gmember;
    const uint64_t len = wrap == FLATE_HIP_WRAP_ZLIB ? sizeof zmember : sizeof gmember;
    const int rc = emit_fixed(c, out, out_cap, m, len, flags);
    if (rc) return rc;
    *out_len = len;
    if (bit_off) bit_off[0] = 0;
    return FLATE_HIP_OK;
  }
  try {
    const FrameReq FR{wrap, nullptr, nullptr, nullptr, 0};
    return deflate_common(c, {in, in_off, n, out, out_cap, bit_off, out_len, flags, true}, nullptr, &FR);
  } catch (const std::exception &e) {
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

int flate_hip_deflate_fast_grouped_framed(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n_pieces,
                                          const uint32_t *group_off, uint32_t n_groups, uint32_t wrap, uint8_t *out,
                                          uint64_t out_cap, uint64_t *out_off, uint64_t *bit_off, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  const int bad = deflate_grouped_args(in, in_off, n_pieces, group_off, n_groups, wrap, out, out_off, flags);
  if (bad) return bad;
  c->hip_err.clear();
  if (n_groups == 0) {
    out_off[0] = 0;
    return FLATE_HIP_OK;
  }
  try {
    // (host pointers: one copy in -- the checksums run on it --, compress, one copy out)
    EncCall A{in, in_off, n_pieces, out, out_cap, out_off, nullptr, flags, true};
    A.group_off = group_off;
    A.n_groups = n_groups;
    A.bit_idx = bit_off;
    if (wrap == FLATE_HIP_WRAP_RAW) return deflate_common(c, A);
    const FrameReq FR{wrap, nullptr, nullptr, nullptr, 0};
    return deflate_common(c, A, nullptr, &FR);
  } catch (const std::exception &e) {  // (out of host memory in an index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

// ---- BGZF files (the writing half; reading: flate_api_inflate.hip) ----

size_t flate_hip_bgzf_bound(uint64_t in_len, uint32_t block_bytes) {
  return (size_t)bgzf_file_bound(in_len, block_bytes, flate_hip_deflate_bound);
}

int flate_hip_bgzf_write(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t block_bytes, uint8_t *out,
                         uint64_t out_cap, uint64_t *out_len, uint64_t *member_off, uint32_t flags) {
  // every check before any HIP call
  if (!c) return FLATE_HIP_E_INVALID;
  int rc = bgzf_write_args(in, in_len, block_bytes, out, out_len, flags);
  if (rc) return rc;
  c->hip_err.clear();
  const uint32_t bb = bgzf_block_bytes(block_bytes);
  const uint32_t n = (uint32_t)bgzf_n_blocks(in_len, bb);
  if (n == 0) {  // the EOF marker alone
    uint8_t eof[kBgzfEofLen];
    for (uint32_t i = 0; i < kBgzfEofLen; ++i) eof[i] = bgzf_eof_byte(i);
    if ((rc = emit_fixed(c, out, out_cap, eof, kBgzfEofLen, flags))) return rc;
    *out_len = kBgzfEofLen;
    if (member_off) member_off[0] = 0;
    return FLATE_HIP_OK;
  }
  try {
    // the blocks as the streams of a batch: the framed encode path with the internal wrap (host pointers: one copy
    // in -- the checksums run on it --, compress, one copy out)
    std::vector<uint64_t> in_off((size_t)n + 1), off;
    for (uint32_t k = 0; k < n; ++k) in_off[k] = (uint64_t)k * bb;
    in_off[n] = in_len;
    if (!member_off) off.resize((size_t)n + 1), member_off = off.data();
    const FrameReq FR{kWrapBgzf, nullptr, nullptr, nullptr, 0};
    return deflate_common(c, {in, in_off.data(), n, out, out_cap, member_off, out_len, flags, false}, nullptr, &FR);
  } catch (const std::exception &e) {  // (out of host memory in an index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}
}  // extern "C"

// ---- a BGZF file written in PARTS (bgzf_parts_rule.h) ----
// The blocks are independent, so a call is flate_hip_bgzf_write over the whole blocks of its part; only the final call
// writes the marker (kWrapBgzfOpen in front of it).  The handle is a few host words.
struct flate_hip_bgzf_writer {
  flate_hip_ctx *ctx = nullptr;
  uint32_t bb = 0, flags = 0;
  uint64_t file_off = 0;  // the bytes written so far: where the next member starts
  bool ended = false;
};

extern "C" {

size_t flate_hip_bgzf_writer_bound(uint64_t in_len, uint32_t block_bytes) { return flate_hip_bgzf_bound(in_len, block_bytes); }

int flate_hip_bgzf_writer_open(flate_hip_ctx *c, uint32_t block_bytes, uint32_t flags, flate_hip_bgzf_writer **out) {
  // every check before any HIP call (there is none)
  if (bgzf_writer_open_args(c, block_bytes, flags, out)) return FLATE_HIP_E_INVALID;
  flate_hip_bgzf_writer *w = new (std::nothrow) flate_hip_bgzf_writer();
  if (!w) return FLATE_HIP_E_INTERNAL;
  w->ctx = c, w->bb = bgzf_block_bytes(block_bytes), w->flags = flags;
  *out = w;
  return FLATE_HIP_OK;
}

int flate_hip_bgzf_writer_reset(flate_hip_bgzf_writer *w) {
  if (!w) return FLATE_HIP_E_INVALID;
  w->file_off = 0, w->ended = false;
  return FLATE_HIP_OK;
}

void flate_hip_bgzf_writer_free(flate_hip_bgzf_writer *w) { delete w; }

int flate_hip_bgzf_writer_write(flate_hip_bgzf_writer *w, const uint8_t *in, uint64_t in_len, int final_in, uint8_t *out,
                                uint64_t out_cap, uint64_t *in_used, uint64_t *out_len, uint64_t *member_off,
                                uint32_t *n_blocks) {
  // every check, and everything the rule decides, before any HIP call
  if (bgzf_writer_write_args(w, in, in_len, out, in_used, out_len, w && w->ended)) return FLATE_HIP_E_INVALID;
  *in_used = 0, *out_len = 0;
  if (n_blocks) *n_blocks = 0;
  const bool fin = final_in != 0;
  const uint64_t blocks = bgzf_writer_blocks(in_len, w->bb, fin), used = bgzf_writer_in_used(in_len, w->bb, fin);
  if (blocks > 0xfffffffeull) return FLATE_HIP_E_TOO_LARGE;
  const uint32_t n = (uint32_t)blocks;
  flate_hip_ctx *c = w->ctx;
  c->hip_err.clear();
  auto done = [&](uint64_t bytes) {
    w->file_off += bytes;
    *in_used = used, *out_len = bytes;
    if (n_blocks) *n_blocks = n;
    if (fin) w->ended = true;
    return fin ? FLATE_HIP_STREAM_END : FLATE_HIP_OK;
  };
  if (n == 0) {
    if (member_off) member_off[0] = w->file_off;
    if (!fin) return FLATE_HIP_OK;  // less than a block: nothing is written, nothing is launched
    uint8_t eof[kBgzfEofLen];       // the marker alone
    for (uint32_t i = 0; i < kBgzfEofLen; ++i) eof[i] = bgzf_eof_byte(i);
    const int rc = emit_fixed(c, out, out_cap, eof, kBgzfEofLen, w->flags);
    return rc ? rc : done(kBgzfEofLen);
  }
  try {
    std::vector<uint64_t> in_off((size_t)n + 1), off((size_t)n + 1);
    for (uint32_t k = 0; k < n; ++k) in_off[k] = (uint64_t)k * w->bb;
    in_off[n] = used;
    uint64_t bytes = 0;
    const FrameReq FR{fin ? kWrapBgzf : kWrapBgzfOpen, nullptr, nullptr, nullptr, 0};
    const int rc = deflate_common(c, {in, in_off.data(), n, out, out_cap, off.data(), &bytes, w->flags, false}, nullptr, &FR);
    if (rc) return rc;  // (too little room, a block BSIZE cannot express: repeatable, the handle is unchanged)
    if (member_off)
      for (uint32_t k = 0; k <= n; ++k) member_off[k] = w->file_off + off[k];
    return done(bytes);
  } catch (const std::exception &e) {  // (out of host memory in an index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}
}  // extern "C"

// ---- ZIP archives (the writing half; the entry point and the reading half: flate_api_zip.hip) ----
// with the option "zip_piece_bytes" and at least one long entry: the entries as the groups of a grouped call
int flate_host::zip_deflate_pieces(flate_hip_ctx *c, const uint8_t *in, const uint64_t *piece_in_off, uint32_t n_pieces,
                                   const uint32_t *group_off, uint32_t n, const uint8_t *names, const uint64_t *name_off,
                                   uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *entry_off, uint32_t flags) {
  try {
    std::vector<uint64_t> index((size_t)n + 1);
    const ZipReq ZR{names, name_off};
    EncCall A{in, piece_in_off, n_pieces, out, out_cap, entry_off ? entry_off : index.data(), out_len, flags, true};
    A.group_off = group_off;
    A.n_groups = n;
    return deflate_common(c, A, nullptr, nullptr, nullptr, &ZR);
  } catch (const std::exception &e) {  // (out of host memory in an index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}

int flate_host::zip_deflate(flate_hip_ctx *c, const uint8_t *in, const uint64_t *in_off, uint32_t n, const uint8_t *names,
                            const uint64_t *name_off, uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *entry_off,
                            uint32_t flags) {
  try {
    // (host pointers: one copy in, one copy out -- no "host_pipeline_groups")
    std::vector<uint64_t> index((size_t)n + 1);  // (the driver reads the archive's index back in any case)
    const ZipReq ZR{names, name_off};
    const int rc = deflate_common(c, {in, in_off, n, out, out_cap, entry_off ? entry_off : index.data(), out_len, flags, false},
                                  nullptr, nullptr, nullptr, &ZR);
    return rc;
  } catch (const std::exception &e) {  // (out of host memory in an index vector)
    c->hip_err = e.what();
    return FLATE_HIP_E_INTERNAL;
  }
}
