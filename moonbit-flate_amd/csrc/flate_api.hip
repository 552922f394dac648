// flate_api.hip -- C ABI of libflate_hip.so (see include/flate_hip.h): the ctx, its options and what the encode and
// the decode calls share -- the scratch and the control-array staging, the host-pointer pipeline's copy threads, the
// staging of preset dictionaries.  (The encode calls: flate_api_deflate.hip; the decode calls: flate_api_inflate.hip, flate_api_units.hip;
// what crosses the file boundaries: flate_ctx.h.)
#include "flate_ctx.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "api_checks.h"

using namespace flate;
using namespace flate_host;

namespace flate {
hipStream_t ctx_stream(flate_hip_ctx *c) { return c->stream; }
int ctx_device(flate_hip_ctx *c) { return c->device; }
void ctx_set_error(flate_hip_ctx *c, const std::string &msg) { c->hip_err = msg; }
uint32_t ctx_num_cus(flate_hip_ctx *c) { return c->num_cus; }
void ctx_stage_begin(flate_hip_ctx *c, int stage) {
  if (c->profiling) (void)hipEventRecord(c->ev[2 * stage], c->stream);
}
void ctx_stage_end(flate_hip_ctx *c, int stage) {
  if (c->profiling) (void)hipEventRecord(c->ev[2 * stage + 1], c->stream);
}
int ctx_stage_collect(flate_hip_ctx *c, int stage) {
  for (int s = 0; s < FLATE_HIP_STAGE_COUNT; ++s) c->stage_ms[s] = 0.f;
  if (c->profiling) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev[2 * stage], c->ev[2 * stage + 1]) != hipSuccess) return FLATE_HIP_E_HIP;
    c->stage_ms[stage] = ms;
  }
  return FLATE_HIP_OK;
}
}  // namespace flate

namespace flate_host {

int ensure(flate_hip_ctx *c, DevBuf &b, size_t bytes) {
  if (bytes <= b.cap) return FLATE_HIP_OK;
  if (b.p) HIP_TRY(c, hipFree(b.p));
  b.p = nullptr;
  b.cap = 0;
  size_t want = bytes + (bytes >> 3) + 256;
  HIP_TRY(c, hipMalloc(&b.p, want));
  b.cap = want;
  return FLATE_HIP_OK;
}

int stage_input(flate_hip_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t flags, const uint8_t **d_in) {
  HIP_TRY(c, hipSetDevice(c->device));
  *d_in = in;
  if (flags & FLATE_HIP_DEVICE_PTRS) return FLATE_HIP_OK;
  const int rc = ensure(c, c->d_in, in_len + 16);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->d_in.p, in, in_len, hipMemcpyHostToDevice, c->stream));
  *d_in = (const uint8_t *)c->d_in.p;
  return FLATE_HIP_OK;
}

int tiles_for(const uint8_t *d_in, uint64_t lo, uint64_t len, uint32_t *n_tiles) {
  const uint64_t tiles = chain_tiles(reinterpret_cast<uintptr_t>(d_in) & 15u, lo, len);
  if (tiles > 0x7fffffffull) return FLATE_HIP_E_TOO_LARGE;
  *n_tiles = (uint32_t)tiles;
  return FLATE_HIP_OK;
}

int chain_size(ChainParams &C, uint32_t cap) {
  if (cap > 0x7ffffff0u) return FLATE_HIP_E_TOO_LARGE;
  C.cap = cap;
  C.path_len = 1u << bgzf_rounds(cap);
  return FLATE_HIP_OK;
}

// ---- small index arrays: host <-> device through pinned staging and a copy kernel (copy_ctl_kernel) ----
// ctl_begin: room for the call's uploads / downloads (a staging buffer only grows between calls: the
// stream is drained first).  ctl_up: stage + launch.  ctl_down: launch into the staging; the bytes reach
// the caller's array in ctl_finish, after the stream has been synchronised.
int ctl_begin(flate_hip_ctx *c, size_t up_bytes, size_t down_bytes) {
  auto grow = [&](flate_hip_ctx::CtlStage &b, size_t need) -> int {
    b.used = 0;
    if (need <= b.cap) return FLATE_HIP_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (b.p) HIP_TRY(c, hipHostFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    const size_t want = need + (need >> 2) + 4096;
    HIP_TRY(c, hipHostMalloc((void **)&b.p, want, hipHostMallocDefault));
    b.cap = want;
    return FLATE_HIP_OK;
  };
  c->ctl_pending.clear();
  int rc;
  if ((rc = grow(c->ctl_up_buf, up_bytes + 16 * 256))) return rc;
  return grow(c->ctl_down_buf, down_bytes + 16 * 256);
}

static void ctl_launch(flate_hip_ctx *c, void *dst, const void *src, size_t bytes) {
  const size_t nwords = (bytes + 3) / 4;
  uint32_t blocks = (uint32_t)((nwords + 255) / 256);
  if (blocks > 512) blocks = 512;
  if (blocks == 0) return;
  hipLaunchKernelGGL(copy_ctl_kernel, dim3(blocks), dim3(256), 0, c->stream, (uint32_t *)dst, (const uint32_t *)src, nwords);
}

// (bytes: a multiple of 4 or rounded up to one -- every device buffer here has that slack)
int ctl_up(flate_hip_ctx *c, void *dev_dst, const void *host_src, size_t bytes) {
  if (!bytes) return FLATE_HIP_OK;
  auto &b = c->ctl_up_buf;
  const size_t at = (b.used + 255) & ~(size_t)255;
  if (at + bytes + 4 > b.cap) return FLATE_HIP_E_INTERNAL;  // (ctl_begin was given too little)
  memcpy(b.p + at, host_src, bytes);
  b.used = at + bytes;
  ctl_launch(c, dev_dst, b.p + at, bytes);
  return FLATE_HIP_OK;
}

int ctl_down(flate_hip_ctx *c, void *host_dst, const void *dev_src, size_t bytes) {
  if (!bytes) return FLATE_HIP_OK;
  auto &b = c->ctl_down_buf;
  const size_t at = (b.used + 255) & ~(size_t)255;
  if (at + bytes + 4 > b.cap) return FLATE_HIP_E_INTERNAL;
  b.used = at + bytes;
  ctl_launch(c, b.p + at, dev_src, bytes);
  c->ctl_pending.push_back({host_dst, at, bytes});
  return FLATE_HIP_OK;
}

// after hipStreamSynchronize(c->stream)
void ctl_finish(flate_hip_ctx *c) {
  for (const auto &p : c->ctl_pending) memcpy(p.host_dst, c->ctl_down_buf.p + p.off, p.bytes);
  c->ctl_pending.clear();
}

}  // namespace flate_host
namespace flate {
int ctx_scratch(flate_hip_ctx *c, int slot, size_t bytes, void **p) {
  if (slot < 0 || slot > 1) return FLATE_HIP_E_INVALID;
  const int rc = ensure(c, c->d_aux[slot], bytes + 16);
  *p = c->d_aux[slot].p;
  return rc;
}
int ctx_ctl_begin(flate_hip_ctx *c, size_t up_bytes, size_t down_bytes) { return ctl_begin(c, up_bytes, down_bytes); }
int ctx_ctl_up(flate_hip_ctx *c, void *dev_dst, const void *host_src, size_t bytes) { return ctl_up(c, dev_dst, host_src, bytes); }
int ctx_ctl_down(flate_hip_ctx *c, void *host_dst, const void *dev_src, size_t bytes) { return ctl_down(c, host_dst, dev_src, bytes); }
void ctx_ctl_finish(flate_hip_ctx *c) { ctl_finish(c); }
}  // namespace flate
namespace {

// Probe offsets of the skip heuristic (deflate-fast.mbt:178-187) from skip = 32.
std::vector<uint16_t> make_scan_table() {
  std::vector<uint16_t> t;
  uint32_t skip = 32, pos = 0;
  while (pos <= 65535) {
    t.push_back((uint16_t)pos);
    uint32_t step = skip >> 5;
    pos += step;
    skip += step;
  }
  t.push_back(65535);  // sentinel: never a legal probe
  return t;
}

}  // namespace

int flate_host::collect_timing(flate_hip_ctx *c, const bool used[FLATE_HIP_STAGE_COUNT]) {
  for (int s = 0; s < FLATE_HIP_STAGE_COUNT; ++s) {
    c->stage_ms[s] = 0.f;
    if (c->profiling && used[s]) {
      float ms = 0.f;
      HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[2 * s], c->ev[2 * s + 1]));
      c->stage_ms[s] = ms;
    }
  }
  return FLATE_HIP_OK;
}

extern "C" {

const char *flate_hip_strerror(int code) {
  switch (code) {
    case FLATE_HIP_OK: return "ok";
    case FLATE_HIP_E_INVALID: return "invalid argument";
    case FLATE_HIP_E_OUT_TOO_SMALL: return "output buffer too small";
    case FLATE_HIP_E_HIP: return "HIP runtime error";
    case FLATE_HIP_E_CORRUPT: return "flate: corrupt input";
    case FLATE_HIP_E_NO_DEVICE: return "no usable HIP device (this engine has no CPU path)";
    case FLATE_HIP_E_TOO_LARGE:
      return "stream too large (a single long gzip member is read with flate_hip_inflate_one; a stream with 2^28 bytes "
             "or more between two dynamic block headers with flate_hip_inflate_stream_read)";
    case FLATE_HIP_E_UNEXPECTED_EOF: return "unexpected EOF";
    case FLATE_HIP_E_INTERNAL: return "internal error: encoder self-check failed";
    case FLATE_HIP_E_AGAIN: return "a shard outgrew the agreed plan (pad or stream count): repeat this batch with the blocking exchange";
    case FLATE_HIP_E_UNSUPPORTED: return "ZIP: entry not supported (encrypted, patched, or a method other than stored and deflate)";
    default: return "unknown error";
  }
}

#ifndef FLATE_HIP_BUILD_ID
#define FLATE_HIP_BUILD_ID "unknown"
#endif
#define FLATE_STR2(x) #x
#define FLATE_STR(x) FLATE_STR2(x)
#ifdef FLATE_EXPERIMENT_BUILD  // (a build that may contain FLATE_EXP_* switches: never a measurement's or a product's id)
#define FLATE_ID_EXP ";exp"
#else
#define FLATE_ID_EXP ""
#endif
#ifdef FLATE_EXPERIMENT_TABLE_BITS
const char *flate_hip_build_id(void) {
  return FLATE_HIP_BUILD_ID FLATE_ID_EXP ";NOT-BIT-EXACT:table_bits=" FLATE_STR(FLATE_EXPERIMENT_TABLE_BITS);
}
#else
const char *flate_hip_build_id(void) { return FLATE_HIP_BUILD_ID FLATE_ID_EXP; }
#endif

const char *flate_hip_last_hip_error(const flate_hip_ctx *ctx) {
  return ctx ? ctx->hip_err.c_str() : "";
}

const char *flate_hip_stage_name(int stage) {
  switch (stage) {
    case FLATE_HIP_STAGE_LZ77: return "lz77_match";
    case FLATE_HIP_STAGE_HUFF_PACK: return "huff_pack";
    case FLATE_HIP_STAGE_CHECKSUM: return "checksum";
    case FLATE_HIP_STAGE_INFLATE: return "inflate";
    default: return "?";
  }
}

int flate_hip_init(int device, flate_hip_ctx **out) {
  if (!out) return FLATE_HIP_E_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
    return FLATE_HIP_E_NO_DEVICE;
  flate_hip_ctx *c = new flate_hip_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->own_stream) != hipSuccess) {
    flate_hip_destroy(c);
    return FLATE_HIP_E_NO_DEVICE;
  }
  c->stream = c->own_stream;
  // The match finder is TWO kernels that must run side by side (LDS-table blocks on c->stream, guest blocks
  // on guest_stream, one queue of streams between them).  HIP spreads its streams over a few hardware
  // queues (four by default) round robin; two streams that land on the same one run their kernels one
  // after the other -- measured: the match finder of a sub-context 40 % slower (19.8 -> 27.9 ms per GiB in
  // 4096-stream launches) when the number of streams created before it shifted by one.  Streams of a
  // different PRIORITY come from a different pool of hardware queues, so the guest stream asks for one:
  // it can never share a queue with the (normal-priority) stream of the kernel it runs beside.
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  const char *gp = getenv("FLATE_HIP_GUEST_STREAM_PRIORITY");  // (developer A/B: "normal" = as before)
  const bool plain_guest = (gp && gp[0] == 'n') || prio_greatest == prio_least;
  if ((plain_guest ? hipStreamCreateWithFlags(&c->guest_stream, hipStreamNonBlocking)
                   : hipStreamCreateWithPriority(&c->guest_stream, hipStreamNonBlocking, prio_greatest)) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
    flate_hip_destroy(c);
    return FLATE_HIP_E_HIP;
  }
  {  // 4 resident (LDS-table) + 6 guest (L2-table, 4 KiB of LDS slot tags each) match-finder waves per CU:
     // what a CU's LDS granules hold, and the measured optimum (profiles/r05/README.md sections 6-7)
    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
      cus = prop.multiProcessorCount;
    c->num_cus = (uint32_t)cus;
    c->enc.guest_min = 5u * (uint32_t)cus;  // measured: 1024 streams 1.72 ms as one block per stream vs 2.15 ms
                                        // persistent; 1280: 3.41 vs 2.35; 2048: 3.61 vs 2.76; 3072: 5.55 vs 3.96
    // LDS comes in 128 granules of 1280 B per CU: an LDS-table block (32768 B) takes 26, a guest (4096 B of slot
    // tags) 4, so 4 + 6 blocks fill a CU exactly.  Launching MORE guests than fit (rounds 2-4 asked for 6.5 per CU)
    // lets guests that arrive first take the granules of an LDS-table block: most processes then ran 3.5 + 6.5
    // blocks per CU and the match finder 4 % slower (profiles/r05/README.md section 7).  Ask for what fits.
    c->enc.resident_blocks = 4u * (uint32_t)cus;
    c->enc.guest_blocks = 6 * cus;
  }
  if (const char *e = getenv("FLATE_HIP_GUEST_BLOCKS")) c->enc.guest_blocks = atoi(e) < 0 ? 0 : atoi(e);
  if (const char *e = getenv("FLATE_HIP_GUEST_MIN")) c->enc.guest_min = (uint32_t)atoi(e);
  if (const char *e = getenv("FLATE_HIP_RESIDENT_BLOCKS")) c->enc.resident_blocks = atoi(e) < 1 ? 1u : (uint32_t)atoi(e);
  for (auto &e : c->ev)
    if (hipEventCreate(&e) != hipSuccess) {
      flate_hip_destroy(c);
      return FLATE_HIP_E_HIP;
    }
  std::vector<uint16_t> tab = make_scan_table();
  c->scan_len = (int)tab.size();
  if (ensure(c, c->scan_tab, tab.size() * 2) != FLATE_HIP_OK ||
      hipMemcpy(c->scan_tab.p, tab.data(), tab.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
      ensure(c, c->d_status, 16) != FLATE_HIP_OK) {
    flate_hip_destroy(c);
    return FLATE_HIP_E_HIP;
  }
  *out = c;
  return FLATE_HIP_OK;
}

void flate_hip_destroy(flate_hip_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
  for (auto &l : c->lane) {
    flate_hip_destroy(l);
    l = nullptr;
  }
  if (c->ctl_up_buf.p) (void)hipHostFree(c->ctl_up_buf.p);
  if (c->ctl_down_buf.p) (void)hipHostFree(c->ctl_down_buf.p);
  if (c->h2d_stream) (void)hipStreamDestroy(c->h2d_stream);
  if (c->d2h_stream) (void)hipStreamDestroy(c->d2h_stream);
  for (auto &e : c->ev)
    if (e) (void)hipEventDestroy(e);
  if (c->guest_stream) (void)hipStreamDestroy(c->guest_stream);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;  // (and with it every DevBuf)
}

int flate_hip_set_stream(flate_hip_ctx *c, void *hip_stream) {
  if (!c) return FLATE_HIP_E_INVALID;
  c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
  return FLATE_HIP_OK;
}

int flate_hip_set_option(flate_hip_ctx *c, const char *name, int64_t value) {
  if (!c || !name) return FLATE_HIP_E_INVALID;
  const std::string k(name);
  if (k == "guest_blocks" && value >= 0 && value <= 65536) {
    c->enc.guest_blocks = (int)value;
  } else if (k == "guest_min_streams" && value >= 0) {
    c->enc.guest_min = (uint32_t)value;
  } else if (k == "inflate_lanes" && (value == 0 || value == 16 || value == 32 || value == 64)) {
    c->inflate.lanes = (int)value;
  } else if (k == "inflate_row_dwords" && (value == 0 || value == 8 || value == 16)) {
    c->inflate.row = (int)value;
  } else if (k == "inflate_simt_min_streams" && value >= 0) {
    c->inflate.simt_min = (uint32_t)value;
  } else if (k == "inflate_spec" && value >= 0 && value <= 2) {
    c->inflate.spec = (int)value;
  } else if (k == "inflate_spec_shape" && value >= 0 && value <= 2) {
    c->inflate.spec_shape = (int)value;
  } else if (k == "inflate_spec_max_streams" && value >= 0 && value <= 0x7fffffff) {
    c->inflate.spec_max = (uint32_t)value;
  } else if (k == "resident_blocks" && value > 0 && value <= 65536) {
    c->enc.resident_blocks = (uint32_t)value;
  } else if (k == "host_pipeline_groups" && value >= 0 && value <= 64) {
    c->host_groups = (int)value;
  } else if (k == "host_pipeline_group_streams" && value > 0 && value <= 0x7fffffff) {
    c->host_group_streams = (uint32_t)value;
  } else if (k == "host_pipeline_lanes" && value >= 1 && value <= 2) {
    c->host_lanes = (int)value;
  } else if (k == "profile_split_streams" && value >= 0 && value <= 0x7fffffff) {
    c->enc.profile_split = (uint32_t)value;
  } else if (k == "window_units" && (value == 0 || value == 1)) {
    c->enc.window_units = (int)value;
  } else if (k == "spin_limit_polls" && value > 0 && value <= 0x7fffffff) {
    c->enc.spin_limit = (uint32_t)value;
  } else if (k == "entropy_per_block" && value >= -1 && value <= 1) {
    c->enc.entropy_per_block = (int)value;
  } else if (k == "stream_rebase_bytes" && value >= 65535 && value <= (1ll << 30)) {
    c->stream_rebase = (uint64_t)value;
  } else if (k == "debug_drop_window_push" && value >= 0 && value <= 0x7fffffff) {
    c->inject_drop_push = (uint32_t)value;
  } else if (k == "debug_stall_batch" && value >= 0 && value <= 0x7fffffff) {
    c->inject_stall = (uint32_t)value;
  } else if (k == "debug_buffer_reset" && value >= 0 && value <= 0x7fffffff) {
    c->debug_buffer_reset = value;
  } else if (k == "gzip_member_max" && gzip_member_max_ok(value)) {
    c->gzip_member_max = (uint64_t)value;
  } else if (k == "one_unit_max" && one_unit_max_ok(value)) {
    c->one_unit_max = (uint64_t)value;
  } else if (k == "one_stored_units" && one_stored_units_ok(value)) {
    c->one_stored_units = (uint32_t)value;
  } else if (k == "one_round_units" && one_round_units_ok(value)) {
    c->one_round_units = (uint32_t)value;
  } else if (k == "zip_unit_min" && zip_unit_min_ok(value)) {
    c->zip_unit_min = (uint64_t)value;
  } else if (k == "zip_piece_bytes" && zip_piece_bytes_ok(value)) {
    c->zip_piece_bytes = (uint64_t)value;
  } else if (k == "gzfile_serial_max" && gzfile_serial_max_ok(value)) {
    c->gzfile_serial_max = (uint64_t)value;
  } else {
    return FLATE_HIP_E_INVALID;
  }
  return FLATE_HIP_OK;
}

// Host buffers the caller keeps across calls (a Writer's input buffer, a Reader's output buffer): once
// page-locked, the copies of the host-pointer calls are DMA transfers at the link's rate; from pageable
// memory the runtime stages every copy through bounce buffers of its own.  Nothing else changes: the
// copy paths hand the same pointers to hipMemcpyAsync, which knows the registered ranges.
int flate_hip_host_register(flate_hip_ctx *c, void *p, size_t bytes) {
  if (!c || !p || !bytes) return FLATE_HIP_E_INVALID;
  c->hip_err.clear();
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipHostRegister(p, bytes, hipHostRegisterDefault));
  return FLATE_HIP_OK;
}

int flate_hip_host_unregister(flate_hip_ctx *c, void *p) {
  if (!c || !p) return FLATE_HIP_E_INVALID;
  c->hip_err.clear();
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipHostUnregister(p));
  return FLATE_HIP_OK;
}

int flate_hip_host_alloc(flate_hip_ctx *c, size_t bytes, void **out) {
  if (!c || !out || !bytes) return FLATE_HIP_E_INVALID;
  *out = nullptr;
  c->hip_err.clear();
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipHostMalloc(out, bytes, hipHostMallocDefault));
  return FLATE_HIP_OK;
}

int flate_hip_host_free(flate_hip_ctx *c, void *p) {
  if (!c) return FLATE_HIP_E_INVALID;
  if (!p) return FLATE_HIP_OK;
  c->hip_err.clear();
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipHostFree(p));
  return FLATE_HIP_OK;
}

int flate_hip_last_resident_share(flate_hip_ctx *c, uint32_t *resident_streams, uint32_t *queued_streams) {
  if (!c || !resident_streams || !queued_streams) return FLATE_HIP_E_INVALID;
  *resident_streams = *queued_streams = 0;
  if (!c->d_queue.p) return FLATE_HIP_OK;
  uint32_t q[8] = {0};
  HIP_TRY(c, hipMemcpy(q, c->d_queue.p, 32, hipMemcpyDeviceToHost));
  *resident_streams = q[4] + q[5];
  *queued_streams = c->last_count[0] + c->last_count[1];
  return FLATE_HIP_OK;
}

int flate_hip_zip_last_route(const flate_hip_ctx *c, uint32_t *unit_entries, uint32_t *fallback_entries, uint32_t *n_units,
                             uint32_t *n_candidates) {
  if (!c || !unit_entries || !fallback_entries || !n_units || !n_candidates) return FLATE_HIP_E_INVALID;
  *unit_entries = c->zip_route[0], *fallback_entries = c->zip_route[1];
  *n_units = c->zip_route[2], *n_candidates = c->zip_route[3];
  return FLATE_HIP_OK;
}

int flate_hip_zip_write_last_route(const flate_hip_ctx *c, uint32_t *long_entries, uint32_t *n_pieces) {
  if (!c || !long_entries || !n_pieces) return FLATE_HIP_E_INVALID;
  *long_entries = c->zip_write_route[0], *n_pieces = c->zip_write_route[1];
  return FLATE_HIP_OK;
}

int flate_hip_gzfile_last_route(const flate_hip_ctx *c, uint32_t *serial_members, uint32_t *unit_members,
                                uint64_t *find_from) {
  const int rc = gzfile_last_route_args(c, serial_members, unit_members, find_from);
  if (rc) return rc;
  *serial_members = c->gzfile_route[0], *unit_members = c->gzfile_route[1];
  *find_from = c->gzfile_route_from;
  return FLATE_HIP_OK;
}

int flate_hip_set_profiling(flate_hip_ctx *c, int on) {
  if (!c) return FLATE_HIP_E_INVALID;
  c->profiling = on != 0;
  return FLATE_HIP_OK;
}

int flate_hip_last_timing(flate_hip_ctx *c, float *ms, int n) {
  if (!c || !ms) return FLATE_HIP_E_INVALID;
  for (int i = 0; i < n && i < FLATE_HIP_STAGE_COUNT; ++i) ms[i] = c->stage_ms[i];
  return FLATE_HIP_OK;
}

}  // extern "C"

// FLATE_HIP_TRACE_HOST=1: timestamps of the host-pointer pipeline's stages on stderr (developer aid)
static bool host_trace_on() {
  static const bool on = getenv("FLATE_HIP_TRACE_HOST") != nullptr;
  return on;
}
double flate_host::host_now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
void flate_host::host_trace(double t0, const char *what, unsigned g, double a, double b) {
  if (host_trace_on()) fprintf(stderr, "[host-pipe] %-8s g=%u  %.2f .. %.2f ms\n", what, g, a - t0, b - t0);
}

// ---- host-pointer batches, pipelined over groups of streams (flate_hip_ctx::host_groups; CopyPipe: flate_ctx.h) ----
namespace flate_host {
void CopyPipe::start(int device, hipStream_t s_in, hipStream_t s_out, std::vector<CopyJob> in_jobs) {
  const size_t n_out = out_jobs_.size();
  t_in_ = std::thread([this, device, s_in, in_jobs] {
    (void)hipSetDevice(device);
    for (size_t g = 0; g < in_jobs.size(); ++g) {
      {
        std::lock_guard<std::mutex> l(mu_);
        if (stop_) return;
      }
      const double a = host_now_ms();
      const bool ok = run(in_jobs[g], hipMemcpyHostToDevice, s_in, "host-to-device copy: ");
      host_trace(t0_, "h2d", (unsigned)g, a, host_now_ms());
      std::lock_guard<std::mutex> l(mu_);
      in_ready_[g] = ok ? 1 : -1;
      cv_.notify_all();
      if (!ok) return;
    }
  });
  t_out_ = std::thread([this, device, s_out, n_out] {
    (void)hipSetDevice(device);
    for (size_t g = 0; g < n_out; ++g) {
      CopyJob j;
      {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return out_state_[g] != 0; });
        if (out_state_[g] < 0) return;
        j = out_jobs_[g];
      }
      const double a = host_now_ms();
      if (!run(j, hipMemcpyDeviceToHost, s_out, "device-to-host copy: ")) return;
      host_trace(t0_, "d2h", (unsigned)g, a, host_now_ms());
    }
  });
}
bool CopyPipe::wait_in(size_t g) {
  std::unique_lock<std::mutex> l(mu_);
  cv_.wait(l, [&] { return in_ready_[g] != 0; });
  return in_ready_[g] > 0;
}
void CopyPipe::post_out(size_t g, CopyJob j) {
  std::lock_guard<std::mutex> l(mu_);
  out_jobs_[g] = j;
  out_state_[g] = 1;
  cv_.notify_all();
}
std::string CopyPipe::finish() {
  {
    std::lock_guard<std::mutex> l(mu_);
    stop_ = true;
    for (auto &st : out_state_)
      if (st == 0) st = -1;
    cv_.notify_all();
  }
  if (t_in_.joinable()) t_in_.join();
  if (t_out_.joinable()) t_out_.join();
  return err_;
}
bool CopyPipe::run(const CopyJob &j, hipMemcpyKind kind, hipStream_t s, const char *what) {
  hipError_t e = hipSuccess;
  if (j.bytes) e = hipMemcpyAsync(j.dst, j.src, j.bytes, kind, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e == hipSuccess) return true;
  std::lock_guard<std::mutex> l(mu_);
  if (err_.empty()) err_ = std::string(what) + hipGetErrorString(e);
  return false;
}

// Group boundaries of a host-pointer batch: group g ends at the first stream where the running byte
// count (a, plus b when given) reaches g / G of the total -- streams of very different sizes still
// give groups of equal work.  lo has G + 1 entries, lo[0] = 0, lo[G] = n, non-decreasing.
void cut_by_bytes(const uint64_t *a, const uint64_t *b, uint32_t n, uint32_t G, std::vector<uint32_t> &lo) {
  auto at = [&](uint32_t i) { return (a[i] - a[0]) + (b ? b[i] - b[0] : 0ull); };
  const uint64_t total = at(n);
  lo[0] = 0;
  uint32_t i = 0;
  for (uint32_t g = 1; g < G; ++g) {
    const uint64_t want = total / G * g;
    while (i < n && at(i) < want) ++i;
    lo[g] = i;
  }
  lo[G] = n;
}

// The two copy streams of the host-pointer pipelines: LOW priority, i.e. hardware queues of a pool of their
// own (see the guest stream in flate_hip_init): a copy that shared a hardware queue with a lane's kernels
// would wait behind them and the pipeline would run in lock step.
int host_pipe_streams(flate_hip_ctx *c) {
  int least = 0, greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
  const char *gp = getenv("FLATE_HIP_GUEST_STREAM_PRIORITY");
  const bool plain = (gp && gp[0] == 'n') || least == greatest;
  auto mk = [&](hipStream_t *s) {
    return plain ? hipStreamCreateWithFlags(s, hipStreamNonBlocking) : hipStreamCreateWithPriority(s, hipStreamNonBlocking, least);
  };
  if (!c->h2d_stream) HIP_TRY(c, mk(&c->h2d_stream));
  if (!c->d2h_stream) HIP_TRY(c, mk(&c->d2h_stream));
  return FLATE_HIP_OK;
}

// ---- preset dictionaries, as the encode and the decode calls stage them ----

// (host only, after dict_args_ok: the entry points make every check before any HIP call)
DictSlots dict_slots(const uint64_t *dict_off, uint32_t n_dicts, const uint32_t *dict_of, uint32_t n, uint32_t min_len) {
  DictSlots S;
  S.slot_of.assign(n, DictSlots::kNone);
  std::vector<uint32_t> slot_of_dict(n_dicts, DictSlots::kNone);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t j = dict_of ? dict_of[i] : 0u;
    if (j == FLATE_HIP_NO_DICT) continue;
    const uint64_t l = dict_off[j + 1] - dict_off[j];
    const uint32_t tail = l < (uint64_t)kMaxMatchOffset ? (uint32_t)l : (uint32_t)kMaxMatchOffset;
    if (tail < min_len) continue;
    if (slot_of_dict[j] == DictSlots::kNone) {
      slot_of_dict[j] = (uint32_t)S.at.size();
      S.dict.push_back(j);
      S.len.push_back(tail);
      S.at.push_back(S.total);
      S.total += ((uint64_t)tail + 16 + 15) & ~15ull;
    }
    S.slot_of[i] = slot_of_dict[j];
  }
  return S;
}

// the slots' tails into c->d_dicts (on c->stream; the caller synchronises)
int dict_upload(flate_hip_ctx *c, const DictSlots &S, const uint8_t *dicts, const uint64_t *dict_off, uint32_t flags) {
  const int rc = ensure(c, c->d_dicts, S.total);
  if (rc) return rc;
  const hipMemcpyKind kind = (flags & FLATE_HIP_DEVICE_PTRS) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  for (size_t k = 0; k < S.at.size(); ++k)
    HIP_TRY(c, hipMemcpyAsync((uint8_t *)c->d_dicts.p + S.at[k], dicts + dict_off[S.dict[k] + 1] - S.len[k], S.len[k],
                              kind, c->stream));
  return FLATE_HIP_OK;
}

// (the byte counts depend on the dictionaries' lengths only: the offsets as the caller has them will do)
size_t dictid_ctl_up_bytes(const uint64_t *dict_off, uint32_t n_dicts) { return checksum_ctl_up_bytes(dict_off, n_dicts); }
size_t dictid_scratch_bytes(const uint64_t *dict_off, uint32_t n_dicts) { return checksum_scratch_bytes(dict_off, n_dicts); }

int dictid_stage(flate_hip_ctx *c, const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts, uint32_t flags) {
  int rc;
  if ((rc = ensure(c, c->d_frame_ids, (size_t)n_dicts * 4 + 4))) return rc;
  if (!n_dicts) return FLATE_HIP_OK;
  std::vector<uint64_t> rel((size_t)n_dicts + 1, 0);  // counted from the first dictionary's start
  for (uint32_t j = 1; j <= n_dicts; ++j) rel[j] = dict_off[j] - dict_off[0];
  const uint8_t *d_whole = dicts ? dicts + dict_off[0] : nullptr;
  if (!(flags & FLATE_HIP_DEVICE_PTRS)) {
    const uint64_t bytes = rel[n_dicts];
    if ((rc = ensure(c, c->d_frame_dicts, bytes + 16))) return rc;
    if (bytes) HIP_TRY(c, hipMemcpyAsync(c->d_frame_dicts.p, d_whole, bytes, hipMemcpyHostToDevice, c->stream));
    d_whole = (const uint8_t *)c->d_frame_dicts.p;
  }
  return checksum_device(c, d_whole, rel.data(), n_dicts, FLATE_HIP_CHECKSUM_ADLER32, (uint32_t *)c->d_frame_ids.p, -1);
}

}  // namespace flate_host
