// bgzf_range_model.cpp -- the range rule of flate_hip_bgzf_read_ranges (moonbit-flate_amd/csrc/bgzf_range_rule.h) and
// its argument checks (api_checks.h: bgzf_ranges_args) as a stand-alone CPU program: the very functions the locate
// kernel and the entry point compile, driven by tests/test_bgzf_range_model.py and compared there with
// tests/bgzf_range_ref.py.
//   bgzf_range_model locate FILE   FILE = u32 count, then per case: u64 length + the file's bytes, u32 kind, u32
//                                  n_ranges, begin[n_ranges], end[n_ranges] (u64 each).  The index comes from the serial
//                                  walk (bgzf_rule.h).  One line per case: "status b e first last" per range, ';' between
//   bgzf_range_model checks        one line per argument-check call: name value
//   bgzf_range_model statuses FILE the status rule behind the decode (range_statuses).  FILE = text, per case the numbers
//                                  ns nr with_skip with_status, st[ns], r_lo[nr], r_hi[nr], the statuses the ranges start
//                                  with [nr], skip[nr].  One line per case: the return value, then the ranges' statuses
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "api_checks.h"
#include "bgzf_range_rule.h"
#include "bgzf_rule.h"

using namespace flate;

static int locate_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint64_t len = 0;
    if (fread(&len, 8, 1, f) != 1) return 2;
    uint8_t *buf = (uint8_t *)malloc(len ? len : 1);
    if (len && fread(buf, 1, len, f) != len) return 2;
    uint32_t kind = 0, nr = 0;
    if (fread(&kind, 4, 1, f) != 1 || fread(&nr, 4, 1, f) != 1) return 2;
    // (exact allocations: a read outside an array is a heap overflow the sanitizer reports)
    uint64_t *begin = (uint64_t *)malloc(nr ? nr * 8ull : 1), *end = (uint64_t *)malloc(nr ? nr * 8ull : 1);
    if (nr && (fread(begin, 8, nr, f) != nr || fread(end, 8, nr, f) != nr)) return 2;
    std::vector<uint64_t> walk(len / 26 + 2);
    uint64_t n = 0;
    int64_t err = -1;
    if (bgzf_serial_walk(buf, len, &n, &err, walk.data()) != 0) return 3;  // (well-formed files only)
    uint64_t *moff = (uint64_t *)malloc((n + 1) * 8), *ooff = (uint64_t *)malloc((n + 1) * 8);
    ooff[0] = 0;
    for (uint64_t i = 0; i <= n; ++i) moff[i] = walk[i];
    for (uint64_t i = 0; i < n; ++i) {
      const uint8_t *t = buf + moff[i + 1] - 4;
      ooff[i + 1] = ooff[i] + (t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24));
    }
    for (uint32_t r = 0; r < nr; ++r) {
      const BgzfRangeLoc L = bgzf_range_locate(kind, begin[r], end[r], moff, ooff, (uint32_t)n);
      printf("%d %llu %llu %lld %lld;", L.status, (unsigned long long)L.b, (unsigned long long)L.e,
             L.first == kBgzfNoMember ? -1ll : (long long)L.first, L.last == kBgzfNoMember ? -1ll : (long long)L.last);
    }
    printf("\n");
    free(buf), free(begin), free(end), free(moff), free(ooff);
  }
  fclose(f);
  return 0;
}

static int statuses_file(const char *path) {
  FILE *f = fopen(path, "r");
  if (!f) return 2;
  unsigned ns, nr, with_skip, with_status;
  while (fscanf(f, "%u %u %u %u", &ns, &nr, &with_skip, &with_status) == 4) {
    // (exact allocations: a read outside an array is a heap overflow the sanitizer reports)
    int32_t *st = (int32_t *)malloc(ns ? ns * 4ull : 1), *rs = (int32_t *)malloc(nr ? nr * 4ull : 1),
            *skip = (int32_t *)malloc(nr ? nr * 4ull : 1);
    uint32_t *lo = (uint32_t *)malloc(nr ? nr * 4ull : 1), *hi = (uint32_t *)malloc(nr ? nr * 4ull : 1);
    for (unsigned i = 0; i < ns; ++i)
      if (fscanf(f, "%d", &st[i]) != 1) return 2;
    for (unsigned r = 0; r < nr; ++r)
      if (fscanf(f, "%u", &lo[r]) != 1) return 2;
    for (unsigned r = 0; r < nr; ++r)
      if (fscanf(f, "%u", &hi[r]) != 1) return 2;
    for (unsigned r = 0; r < nr; ++r)
      if (fscanf(f, "%d", &rs[r]) != 1) return 2;
    for (unsigned r = 0; r < nr; ++r)
      if (fscanf(f, "%d", &skip[r]) != 1) return 2;
    printf("%u", range_statuses(st, ns, lo, hi, nr, with_status ? rs : nullptr, with_skip ? skip : nullptr));
    for (unsigned r = 0; r < nr; ++r) printf(" %d", rs[r]);
    printf("\n");
    free(st), free(rs), free(skip), free(lo), free(hi);
  }
  fclose(f);
  return 0;
}

static int checks() {
  uint8_t b[4] = {0};
  uint64_t lo[2] = {1, 5}, hi[2] = {1, 9}, back[2] = {1, 4}, off[3] = {0, 0, 0};
  const uint32_t D = FLATE_HIP_DEVICE_PTRS, B = FLATE_HIP_BGZF_POS_BYTES, V = FLATE_HIP_BGZF_POS_VIRTUAL;
  printf("ok_bytes %d\n", bgzf_ranges_args(b, 4, B, lo, hi, 2, b, 4, off, 0));
  printf("ok_virtual_device %d\n", bgzf_ranges_args(b, 4, V, lo, hi, 2, b, 4, off, D));
  printf("ok_size_query %d\n", bgzf_ranges_args(b, 4, B, lo, hi, 2, nullptr, 0, off, 0));
  printf("ok_empty_file %d\n", bgzf_ranges_args(nullptr, 0, V, lo, hi, 2, b, 4, off, 0));
  printf("ok_no_ranges %d\n", bgzf_ranges_args(b, 4, B, nullptr, nullptr, 0, b, 4, nullptr, 0));
  printf("ok_equal_ends %d\n", bgzf_ranges_args(b, 4, B, lo, lo, 2, b, 4, off, 0));
  printf("no_in %d\n", bgzf_ranges_args(nullptr, 4, B, lo, hi, 2, b, 4, off, 0));
  printf("no_begin %d\n", bgzf_ranges_args(b, 4, B, nullptr, hi, 2, b, 4, off, 0));
  printf("no_end %d\n", bgzf_ranges_args(b, 4, B, lo, nullptr, 2, b, 4, off, 0));
  printf("no_out_off %d\n", bgzf_ranges_args(b, 4, B, lo, hi, 2, b, 4, nullptr, 0));
  printf("no_out_with_cap %d\n", bgzf_ranges_args(b, 4, B, lo, hi, 2, nullptr, 4, off, 0));
  printf("kind_2 %d\n", bgzf_ranges_args(b, 4, 2, lo, hi, 2, b, 4, off, 0));
  printf("kind_max %d\n", bgzf_ranges_args(b, 4, 0xffffffffu, lo, hi, 2, b, 4, off, 0));
  printf("flag_go %d\n", bgzf_ranges_args(b, 4, B, lo, hi, 2, b, 4, off, FLATE_HIP_COMPAT_GO));
  printf("flag_size_only %d\n", bgzf_ranges_args(b, 4, B, lo, hi, 2, b, 4, off, D | FLATE_HIP_SIZE_ONLY));
  printf("backwards_bytes %d\n", bgzf_ranges_args(b, 4, B, lo, back, 2, b, 4, off, 0));
  printf("backwards_virtual %d\n", bgzf_ranges_args(b, 4, V, lo, back, 2, b, 4, off, 0));
  printf("backwards_not_reached %d\n", bgzf_ranges_args(b, 4, V, lo, back, 1, b, 4, off, 0));
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "locate")) return locate_file(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
  if (argc == 3 && !strcmp(argv[1], "statuses")) return statuses_file(argv[2]);
  fprintf(stderr, "usage: %s locate FILE | checks | statuses FILE\n", argv[0]);
  return 2;
}
