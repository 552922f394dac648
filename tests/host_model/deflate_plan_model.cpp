// deflate_plan_model.cpp -- moonbit-flate_amd/csrc/deflate_plan.h behind a C interface (tests/test_deflate_plan.py).
// Built with -DPLAN_MODEL_MAIN it is a program of its own that walks the test's table (for a sanitizer build).
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "deflate_plan.h"

using namespace flate;

namespace {
// opt = {guest_blocks, guest_min, resident_blocks, window_units, entropy_per_block, spin_limit, profile_split}
EncodeOpts opts_of(const int64_t opt[7]) {
  EncodeOpts o;
  o.guest_blocks = (int)opt[0], o.guest_min = (uint32_t)opt[1], o.resident_blocks = (uint32_t)opt[2];
  o.window_units = (int)opt[3], o.entropy_per_block = (int)opt[4], o.spin_limit = (uint32_t)opt[5];
  o.profile_split = (uint32_t)opt[6];
  return o;
}
}  // namespace

extern "C" void plan_defaults(int64_t opt[7]) {
  const EncodeOpts o;
  opt[0] = o.guest_blocks, opt[1] = o.guest_min, opt[2] = o.resident_blocks, opt[3] = o.window_units;
  opt[4] = o.entropy_per_block, opt[5] = o.spin_limit, opt[6] = o.profile_split;
}

// chunk_base, blk_base: n + 1 entries; list_of: per stream 0 = in no list, 1 = single-window, 2 = multi-window,
// 3 = dictionary; counts = {n_chunks, n_blocks, single-window streams, multi-window streams, dictionary streams}
// (nothing is written when the plan is refused; the lists must be ascending stream numbers)
extern "C" int plan_model(const uint64_t *in_off, uint32_t n, uint32_t flags, const uint8_t *has, uint32_t *chunk_base,
                          uint32_t *blk_base, int32_t *list_of, uint64_t counts[5]) {
  StagePlan pl;
  const int rc = make_plan(in_off, n, pl, flags, has);
  if (rc) return rc;
  for (uint32_t i = 0; i <= n; ++i) chunk_base[i] = pl.chunk_base[i], blk_base[i] = pl.blk_base[i];
  for (uint32_t i = 0; i < n; ++i) list_of[i] = 0;
  int k = 0;
  for (const auto *ids : {&pl.ids16, &pl.ids32, &pl.idsD}) {
    ++k;
    for (size_t j = 0; j < ids->size(); ++j) {
      if ((*ids)[j] >= n || list_of[(*ids)[j]] != 0 || (j && (*ids)[j] <= (*ids)[j - 1])) return -100;
      list_of[(*ids)[j]] = k;
    }
  }
  counts[0] = pl.n_chunks, counts[1] = pl.n_blocks;
  counts[2] = pl.ids16.size(), counts[3] = pl.ids32.size(), counts[4] = pl.idsD.size();
  return pl.n_streams == n ? 0 : -100;
}

// out = {per_block, uq_units, pair16, pair32, pairD}
extern "C" int route_model(const uint64_t *in_off, uint32_t n, uint32_t flags, const uint8_t *has, const int64_t opt[7],
                           int spliced, int64_t out[5]) {
  StagePlan pl;
  const int rc = make_plan(in_off, n, pl, flags, has);
  if (rc) return rc;
  const EncodeRoute r = encode_route(pl, opts_of(opt), flags, spliced != 0);
  out[0] = r.per_block, out[1] = r.uq_units, out[2] = r.pair16, out[3] = r.pair32, out[4] = r.pairD;
  return 0;
}

extern "C" uint32_t groups_model(const int64_t opt[7], int host_groups, uint32_t host_group_streams, uint32_t flags, uint32_t n,
                                 uint64_t total_bytes) {
  return encode_host_groups(opts_of(opt), host_groups, host_group_streams, flags, n, total_bytes);
}

// The control-array budget of a batch call as the driver adds it up: out = {up, down}.  framed: a *_framed call, whose
// checksums upload sum_up bytes and whose DICTIDs dictid_up (0 without dict_of).
extern "C" int ctl_model(const uint64_t *in_off, uint32_t n, uint32_t flags, const uint8_t *has, int framed, uint64_t dictid_up,
                         uint64_t sum_up, uint64_t out[2]) {
  StagePlan pl;
  const int rc = make_plan(in_off, n, pl, flags, has);
  if (rc) return rc;
  out[0] = lz77_ctl_up(pl) + entropy_ctl_up(pl);
  if (framed) out[0] += frame_before_ctl_up(n, (size_t)dictid_up) + sum_up;
  out[1] = encode_ctl_down(n);
  return 0;
}

#ifdef PLAN_MODEL_MAIN
namespace {
long g_cases = 0, g_bad = 0;
void want(int64_t got, int64_t expected, const char *what) {
  ++g_cases;
  if (got != expected) ++g_bad, printf("FAIL %s: %lld, expected %lld\n", what, (long long)got, (long long)expected);
}
std::vector<uint64_t> index_of(const std::vector<uint64_t> &lens, uint64_t start = 0) {
  std::vector<uint64_t> off(lens.size() + 1, start);
  for (size_t i = 0; i < lens.size(); ++i) off[i + 1] = off[i] + lens[i];
  return off;
}
}  // namespace

int main() {
  const int INV = FLATE_HIP_E_INVALID, BIG = FLATE_HIP_E_TOO_LARGE;
  const uint64_t W = 65535;
  int64_t d[7];
  plan_defaults(d);
  want(d[0] == 0 && d[1] == 1280 && d[2] == 1024 && d[3] == 1 && d[4] == -1 && d[5] == (8 << 20) && d[6] == 0, 1, "defaults");
  {  // make_plan: the block-policy edges, with and without a dictionary
    const std::vector<uint64_t> lens = {0, 1, 16, 17, 127, 128, 65534, 65535, 65536, W + 127, W + 128, 4 * W};
    const uint32_t n = (uint32_t)lens.size();
    const std::vector<uint64_t> off = index_of(lens, 7);
    for (int dict : {0, 1}) {
      std::vector<uint8_t> has(n, (uint8_t)dict);
      std::vector<uint32_t> cb(n + 1), bb(n + 1);
      std::vector<int32_t> lo(n);
      uint64_t cnt[5];
      want(plan_model(off.data(), n, 0, dict ? has.data() : nullptr, cb.data(), bb.data(), lo.data(), cnt), 0, "plan");
      uint64_t chunks = 0, blocks = 0;
      for (uint32_t i = 0; i < n; ++i) {
        const uint64_t nch = lens[i] / W + (lens[i] % W >= 128 ? 1 : 0), nblk = lens[i] / W + (lens[i] % W ? 1 : 0);
        want(cb[i], (int64_t)chunks, "chunk_base");
        want(bb[i], (int64_t)blocks, "blk_base");
        want(lo[i], nch == 0 ? 0 : dict ? 3 : nch == 1 ? 1 : 2, "list");
        chunks += nch, blocks += nblk;
      }
      want(cb[n] == chunks && bb[n] == blocks && cnt[0] == chunks && cnt[1] == blocks, 1, "totals");
    }
  }
  {  // refusals
    uint32_t cb[3], bb[3];
    int32_t lo[2];
    uint64_t cnt[5];
    const uint8_t has[2] = {0, 1};
    const uint64_t down[3] = {5, 9, 8};
    want(plan_model(down, 2, 0, nullptr, cb, bb, lo, cnt), INV, "descending");
    const uint64_t lim = 0x7ffe0000ull;
    for (uint32_t go : {0u, (uint32_t)FLATE_HIP_COMPAT_GO}) {
      const uint64_t a[3] = {3, 3, 3 + lim - 1}, b[3] = {3, 3, 3 + lim}, da[3] = {3, 3, 3 + lim - W - 1}, db[3] = {3, 3, 3 + lim - W};
      want(plan_model(a, 2, go, nullptr, cb, bb, lo, cnt), go ? 0 : BIG, "0x7ffe0000 - 1 bytes (32769 windows)");
      want(plan_model(b, 2, go, nullptr, cb, bb, lo, cnt), BIG, "0x7ffe0000 bytes");
      want(plan_model(da, 2, go, has, cb, bb, lo, cnt), go ? 0 : BIG, "dictionary: 65535 lower");
      want(plan_model(db, 2, go, has, cb, bb, lo, cnt), BIG, "dictionary: at the limit");
      // (the last window of 128 bytes: 32767 whole windows would pass the byte limit as well)
      const uint64_t w6[3] = {0, 0, 32765 * W + 128}, w7[3] = {0, 0, 32766 * W + 128}, w5[3] = {0, 0, 32764 * W + 128};
      want(plan_model(w6, 2, go, nullptr, cb, bb, lo, cnt), 0, "32766 windows");
      want(plan_model(w7, 2, go, nullptr, cb, bb, lo, cnt), go ? 0 : BIG, "32767 windows");
      want(plan_model(w5, 2, go, has, cb, bb, lo, cnt), 0, "dictionary: 32765 windows");
      want(plan_model(w6, 2, go, has, cb, bb, lo, cnt), go ? 0 : BIG, "dictionary: 32766 windows");
    }
  }
  {  // routes: every option against every batch shape of a small table
    const int64_t gm = 4;
    for (uint64_t len : {(uint64_t)0, (uint64_t)200, 2 * W + 200})
      for (uint32_t n : {3u, 4u, 5u})
        for (int dict : {0, 1})
          for (int hole : {0, 1})
            for (int spliced : {0, 1})
              for (uint32_t flags : {0u, (uint32_t)FLATE_HIP_LZ_SERIAL})
                for (int64_t per_block : {-1, 0, 1})
                  for (int64_t wu : {0, 1})
                    for (int64_t gb : {0, 6}) {
                      std::vector<uint64_t> lens(n, len);
                      if (hole) lens[1] = 0;
                      const std::vector<uint64_t> off = index_of(lens);
                      std::vector<uint8_t> has(n, (uint8_t)dict);
                      const int64_t opt[7] = {gb, gm, 1024, wu, per_block, 1 << 20, 0};
                      int64_t r[5];
                      want(route_model(off.data(), n, flags, has.data(), opt, spliced, r), 0, "route");
                      const uint32_t live = len ? n - (uint32_t)hole : 0u, blocks = live * (len > W ? 3u : 1u);
                      const bool all = live == n;
                      want(r[0], per_block != 0 && blocks > 0 && !spliced && all && (per_block == 1 || blocks >= 3 * n), "per_block");
                      const uint32_t c16 = (len && len <= W && !dict) ? live : 0, c32 = (len > W && !dict) ? live : 0, cD = dict ? live : 0;
                      want(r[2], gb > 0 && c16 >= gm, "pair16");
                      want(r[3], gb > 0 && c32 >= gm, "pair32");
                      want(r[4], gb > 0 && cD >= gm, "pairD");
                      want(r[1], (wu && gb > 0 && c32 >= gm && !flags) ? 3 * (int64_t)c32 : 0, "uq_units");
                    }
    // the ready word's limit: 2^17 - 2 multi-window streams run by window, 2^17 - 1 do not
    for (uint32_t n : {(1u << 17) - 2u, (1u << 17) - 1u}) {
      const std::vector<uint64_t> off = index_of(std::vector<uint64_t>(n, W + 128));
      const int64_t opt[7] = {6, 1280, 1024, 1, -1, 1 << 20, 0};
      int64_t r[5];
      want(route_model(off.data(), n, 0, nullptr, opt, 0, r), 0, "route");
      want(r[1], n == (1u << 17) - 2u ? 2 * (int64_t)n : 0, "uq_units at the ready word's limit");
      want(r[3], 1, "pair32");
    }
  }
  {  // host groups
    const uint64_t MiB64 = 64ull << 20;
    for (int64_t gm : {100, 5000})
      for (int hg : {0, 1, 8})
        for (uint32_t flags : {0u, (uint32_t)FLATE_HIP_DEVICE_PTRS})
          for (uint64_t total : {MiB64 - 1, MiB64})
            for (uint32_t hgs : {2048u, 4096u}) {
              const uint32_t per = gm > hgs ? (uint32_t)gm : hgs;
              for (uint32_t n : {per - 1, per, 2 * per - 1, 2 * per, 8 * per - 1, 8 * per, 9 * per}) {
                const int64_t opt[7] = {6, gm, 1024, 1, -1, 1 << 20, 0};
                const uint32_t g = groups_model(opt, hg, hgs, flags, n, total);
                const uint32_t most = n / per < 8 ? n / per : 8;
                want(g > 1 ? g : 0, (!flags && hg == 8 && total >= MiB64 && most > 1) ? most : 0, "groups");
              }
            }
  }
  {  // the budget: the driver's sum against the expression it replaced
    for (uint64_t len : {(uint64_t)200, 2 * W + 200})
      for (uint32_t n : {1u, 5u})
        for (int dict : {0, 1})
          for (int framed : {0, 1, 2}) {
            const std::vector<uint64_t> off = index_of(std::vector<uint64_t>(n, len));
            std::vector<uint8_t> has(n, (uint8_t)dict);
            uint64_t out[2];
            const uint64_t sum_up = framed ? 1000 + n : 0, dictid_up = framed == 2 ? 777 : 0;
            want(ctl_model(off.data(), n, 0, has.data(), framed, dictid_up, sum_up, out), 0, "ctl");
            const uint64_t blocks = n * (len > W ? 3 : 1);
            const uint64_t f_up = framed ? (uint64_t)n * 4 + 256 + sum_up + dictid_up : 0;
            want((int64_t)out[0], (int64_t)(((uint64_t)n + 1) * 16 + ((uint64_t)n + blocks) * 4 + f_up), "ctl up");
            want((int64_t)out[1], (int64_t)(((uint64_t)n + 1) * 8 + 64), "ctl down");
          }
  }
  printf("deflate_plan: %ld cases, %ld bad\n", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
#endif
