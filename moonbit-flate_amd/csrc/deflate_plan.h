// deflate_plan.h -- how an encode call is cut into windows and blocks, which match-finder list every stream joins, how
// the stages are launched and what the call's index arrays take of the control-array staging (plain C++17, no HIP and
// no ctx: tests/test_deflate_plan.py compiles it on the CPU).  The kernels behind a route: run_lz77 and
// launch_entropy, flate_api_deflate.hip.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "flate_common.h"
#include "flate_hip.h"

namespace flate {

// The launch options of the encoder (flate_hip_set_option; flate_hip_ctx::enc).  A lane of the host pipeline runs
// with a copy of its parent's.
struct EncodeOpts {
  int guest_blocks = 0;        // 0 = guest kernel off
  uint32_t guest_min = 1280;   // below this many streams (5 per CU) the guests stay idle: one block per stream
  uint32_t resident_blocks = 1024;  // persistent LDS-table blocks (4 per CU x 256 CUs)
  // window-granular scheduling of multi-window streams (lz77_kernels.hip, uq_*): on by default
  int window_units = 1;
  // entropy stage with one wavefront per BLOCK instead of per stream: -1 = when the batch's streams
  // have three or more blocks on average (multi-window streams), 0 = never, 1 = whenever possible
  int entropy_per_block = -1;
  // bounded waits of the persistent kernels (uq_pop): polls before giving up
  // (a poll is one relaxed load + s_sleep, >= 0.4 us; a wave that is not running does not count)
  uint32_t spin_limit = 8u << 20;
  // measurement aid (flate_hip_last_resident_share, option "profile_split_streams"): > 0: LDS-table blocks take
  // exactly the first K queue entries, the guest blocks the rest (two queues instead of one)
  uint32_t profile_split = 0;
};

struct StagePlan {
  uint32_t n_streams = 0;
  std::vector<uint32_t> chunk_base;  // n+1
  std::vector<uint32_t> ids16, ids32;
  std::vector<uint32_t> idsD;  // streams that start from a preset dictionary's table (flate_hip_deflate_fast_batch_dict)
  std::vector<uint32_t> blk_base;  // n+1
  uint32_t n_chunks = 0;
  uint32_t n_blocks = 0;
};

// has_dict (or null): per stream, whether DeflateFast::encode has run over a preset dictionary before the payload
inline int make_plan(const uint64_t *in_off, uint32_t n, StagePlan &pl, uint32_t flags, const uint8_t *has_dict = nullptr) {
  pl.n_streams = n;
  pl.chunk_base.resize((size_t)n + 1);
  pl.blk_base.resize((size_t)n + 1);
  uint64_t chunks = 0, blocks = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (in_off[i + 1] < in_off[i]) return FLATE_HIP_E_INVALID;
    const uint64_t len = in_off[i + 1] - in_off[i];
    // (a dictionary is window 0 of its stream: the payload's positions start at 65535, `cur` one window further on)
    const bool dict = has_dict && has_dict[i];
    if (len + (dict ? (uint64_t)kMaxStoreBlockSize : 0) >= 0x7ffe0000ull) return FLATE_HIP_E_TOO_LARGE;
    const uint64_t full = len / kMaxStoreBlockSize, r = len % kMaxStoreBlockSize;
    const uint64_t nch = full + (r >= (uint64_t)kSmallLzMin ? 1 : 0);
    // The reference's `cur` reaches buffer_reset at a Writer's window 32 766 (deflate-fast.mbt:55,130):
    // shift_offsets then CLEARS the table in MoonBit (`prev` is empty, :367-374).  Batch streams keep
    // their table from start to end, so a stream with an LZ77 window that far in is refused here
    // (flate_hip_stream_write follows the reference past that point); in Go's semantics the shift
    // changes no distance and the 32-bit positions above are the only limit.
    if (!(flags & FLATE_HIP_COMPAT_GO) && nch + (dict ? 1 : 0) > 32766) return FLATE_HIP_E_TOO_LARGE;
    pl.chunk_base[i] = (uint32_t)chunks;
    pl.blk_base[i] = (uint32_t)blocks;
    if (dict && nch > 0) {
      pl.idsD.push_back(i);  // (a payload under 128 bytes never reaches the match finder: its dictionary is unused)
    } else if (nch == 1) {
      pl.ids16.push_back(i);  // one LZ77 window (it starts at 0): positions fit a 16-bit slot
    } else if (nch > 0) {
      pl.ids32.push_back(i);
    }
    chunks += nch;
    if (chunks > 0xffffffffull) return FLATE_HIP_E_TOO_LARGE;
    blocks += full + (r > 0 ? 1 : 0);
    if (blocks > 0xffffffffull) return FLATE_HIP_E_TOO_LARGE;
  }
  pl.chunk_base[n] = (uint32_t)chunks;
  pl.blk_base[n] = (uint32_t)blocks;
  pl.n_chunks = (uint32_t)chunks;
  pl.n_blocks = (uint32_t)blocks;
  return FLATE_HIP_OK;
}

// How the two stages of a planned call are launched.
struct EncodeRoute {
  // The entropy stage runs one wavefront per block (huff_hist_block_kernel / huff_pack_block_kernel) instead of one
  // per stream.
  bool per_block;
  // > 0: the multi-window streams of the persistent launch run one window at a time (see uq_run), that many windows in
  // all: the streams' tables rest in global memory between windows (32 KiB each).  0: whole-stream scheduling.
  // (The driver keeps one case to itself: a device that cannot give that scratch falls back to 0 -- run_lz77.)
  uint32_t uq_units;
  // the single-window, the multi-window and the dictionary list: a resident (LDS-table) and a guest (L2-table) launch
  // side by side over one queue, instead of one block per stream
  bool pair16, pair32, pairD;
};

// grouped: the streams are the pieces of several spliced streams (splice_rule.h) -- as for spliced.
inline EncodeRoute encode_route(const StagePlan &pl, const EncodeOpts &o, uint32_t flags, bool spliced, bool grouped = false) {
  const uint32_t n = pl.n_streams;
  EncodeRoute r{};
  // One wavefront per block in the histogram and pack kernels when the streams have many blocks
  // (4096 streams of four windows are 4096 wavefronts per stream-kernel, a quarter of what fills
  // the chip).  Every stream needs at least one block (a stream without any has nobody to write
  // its closing block in that form).  Not for spliced output: where a block starts then depends on
  // the bit its stream starts at (a stored block pads to a byte of the SPLICED stream), which only the
  // stream's own walk knows.
  r.per_block = o.entropy_per_block != 0 && pl.n_blocks > 0 && !spliced && !grouped &&
                (o.entropy_per_block == 1 || (uint64_t)pl.n_blocks >= 3ull * n);
  for (uint32_t i = 0; i < n && r.per_block; ++i) r.per_block = pl.blk_base[i + 1] > pl.blk_base[i];
  const bool serial = (flags & FLATE_HIP_LZ_SERIAL) != 0;
  // (FLATE_HIP_LZ_SERIAL launches the single-lane kernel over the first two lists and looks at none of these)
  auto pair = [&](size_t count) { return o.guest_blocks > 0 && count >= o.guest_min; };
  r.pair16 = pair(pl.ids16.size());
  r.pair32 = pair(pl.ids32.size());
  r.pairD = pair(pl.idsD.size());
  // (the ready word limits window scheduling to 2^17 - 2 streams; more than that: whole-stream scheduling)
  const size_t n32 = pl.ids32.size();
  if (o.window_units && o.guest_blocks > 0 && n32 >= o.guest_min && n32 < (1u << 17) - 1u && !serial) {
    uint64_t units = 0;
    for (uint32_t sid : pl.ids32) units += pl.chunk_base[sid + 1] - pl.chunk_base[sid];
    if (units < 0xffffffffull) r.uq_units = (uint32_t)units;
  }
  return r;
}

// Which build of the match-finder kernels a batch launch takes.  The test hooks (options "debug_stall_batch" and
// "debug_drop_window_push": flate_hip_ctx::inject_stall / inject_drop_push) exist only in the kernels' HOOKS
// instantiations; a call with neither option set runs the product instantiations, whose batch loop carries no hook.
inline bool lz77_hooks_build(uint32_t inject_stall, uint32_t inject_drop_push) {
  return inject_stall != 0 || inject_drop_push != 0;
}

// The groups a host-pointer batch of n streams is cut into (host_groups / host_group_streams: the options
// "host_pipeline_groups" / "host_pipeline_group_streams"); 0 or 1: one pass.  Host pointers and a batch large enough
// that every group still fills the persistent launch (a group of 4096 64-KiB streams still runs at 80 %).
// total_bytes is in_off[n] as the caller has it, NOT in_off[n] - in_off[0]: unlike the decode side
// (inflate_batch_run), which counts the bytes that cross the link, this threshold has always looked at the index's
// last entry, and a refactor is not where that changes.
inline uint32_t encode_host_groups(const EncodeOpts &o, int host_groups, uint32_t host_group_streams, uint32_t flags,
                                   uint32_t n, uint64_t total_bytes) {
  if ((flags & FLATE_HIP_DEVICE_PTRS) || host_groups <= 1 || total_bytes < (64ull << 20)) return 0;
  uint32_t G = (uint32_t)host_groups;
  const uint32_t per = o.guest_min > host_group_streams ? o.guest_min : host_group_streams;
  if (n / per < G) G = n / per;
  return G;
}

// ---- what the steps of a call upload through the control-array staging (ctl_up), in bytes ----
// run_lz77: in_off (8 bytes per entry), chunk_base (n + 1 each), the three stream lists
inline size_t lz77_ctl_up(const StagePlan &pl) {
  return ((size_t)pl.n_streams + 1) * 12 + (pl.ids16.size() + pl.ids32.size() + pl.idsD.size()) * 4;
}
// the entropy stage: blk_base (n + 1) and blk_sid (a word per block; counted whether or not the per-block form runs)
inline size_t entropy_ctl_up(const StagePlan &pl) { return ((size_t)pl.n_streams + 1) * 4 + (size_t)pl.n_blocks * 4; }
// frame_before: dict_of (counted with or without dictionaries) and the DICTIDs' checksums (dictid_up:
// dictid_ctl_up_bytes, 0 for a call without dict_of)
inline size_t frame_before_ctl_up(uint32_t n, size_t dictid_up) { return (size_t)n * 4 + 256 + dictid_up; }
// read back: the output index (the status words and the spliced total fit the 64)
inline size_t encode_ctl_down(uint32_t n) { return ((size_t)n + 1) * 8 + 64; }
// a grouped call: group_off and every piece's group go up; the members' offsets and the groups' bit indexes come back
inline size_t grouped_ctl_up(uint32_t n_pieces, uint32_t n_groups) { return ((size_t)n_pieces + n_groups + 1) * 4 + 1024; }
inline size_t grouped_ctl_down(uint32_t n_pieces, uint32_t n_groups) { return ((size_t)n_pieces + 2 * (size_t)n_groups + 1) * 8 + 1024; }

}  // namespace flate
