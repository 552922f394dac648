// gzfile_seek_rule_model.cpp -- the rule of a gzip file's seek index (moonbit-flate_amd/csrc/gzfile_seek_rule.h) and
// the argument checks of its two calls (api_checks.h) as a stand-alone CPU program: the very functions the kernels and
// the entry points compile, driven by tests/test_gzfile_seek_rule_model.py and compared there with
// tests/gzfile_seek_ref.py.
//   gzfile_seek_rule_model rule FILE  FILE = u32 count, then per case: u64 span, u32 n, out_off[n + 1], u32 m,
//                                     member_unit[m + 1], u32 n_ranges, begin[n_ranges], end[n_ranges] (u64 each).
//                                     One line per case: "unit:block" per point (block -1: a member start; the blocks
//                                     in front of it follow in brackets), '|', "b e first last seg" per range with ';'
//                                     between, '|', the decoded units -- from the difference array the locate kernel
//                                     fills and the select kernel scans --, '|', "rel dict_len final" per unit
//   gzfile_seek_rule_model ok FILE    FILE = u32 count, then per case: u64 in_len, u64 windows_bytes, u64 words, the
//                                     index.  One line per case: gzfile_seek_index_ok
//   gzfile_seek_rule_model checks     one line per argument-check call: name value
// Every array lies in an allocation of exactly its size: a read outside it is a heap overflow the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "api_checks.h"
#include "gzfile_seek_rule.h"

using namespace flate;

template <typename T>
static T *exact(size_t count) {
  return (T *)malloc(count ? count * sizeof(T) : 1);
}

static int rule_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t c = 0; c < count; ++c) {
    uint64_t span = 0;
    uint32_t n = 0, m = 0, nr = 0;
    if (fread(&span, 8, 1, f) != 1 || fread(&n, 4, 1, f) != 1) return 2;
    uint64_t *out_off = exact<uint64_t>((size_t)n + 1);
    if (fread(out_off, 8, (size_t)n + 1, f) != (size_t)n + 1 || fread(&m, 4, 1, f) != 1) return 2;
    uint64_t *member_unit = exact<uint64_t>((size_t)m + 1);
    if (fread(member_unit, 8, (size_t)m + 1, f) != (size_t)m + 1 || fread(&nr, 4, 1, f) != 1) return 2;
    uint64_t *begin = exact<uint64_t>(nr), *end = exact<uint64_t>(nr);
    if (nr && (fread(begin, 8, nr, f) != nr || fread(end, 8, nr, f) != nr)) return 2;
    span = seek_span(span);
    auto starts = [&](uint32_t k) { return member_unit[gzfile_seek_member_of(member_unit, m, k)] == k; };
    uint32_t np = 0;
    for (uint32_t k = 0; k < n; ++k) np += gzfile_seek_is_point(out_off, k, span, starts(k)) ? 1u : 0u;
    uint64_t *point_unit = exact<uint64_t>(np);
    for (uint32_t k = 0, p = 0; k < n; ++k)
      if (gzfile_seek_is_point(out_off, k, span, starts(k))) point_unit[p++] = k;
    for (uint32_t p = 0; p < np; ++p) {
      const uint32_t u = (uint32_t)point_unit[p];
      printf("%u:%lld[%u] ", u, starts(u) ? -1ll : (long long)gzfile_seek_block(member_unit, m, p, u),
             gzfile_seek_blocks_before(member_unit, m, p, u));
    }
    printf("|");
    int32_t *diff = exact<int32_t>((size_t)n + 1);
    memset(diff, 0, ((size_t)n + 1) * 4);
    for (uint32_t r = 0; r < nr; ++r) {
      const SeekLoc L = gzfile_seek_locate(begin[r], end[r], out_off, n, point_unit, np);
      printf("%llu %llu %lld %lld %lld;", (unsigned long long)L.b, (unsigned long long)L.e,
             L.first == kBgzfNoMember ? -1ll : (long long)L.first, L.last == kBgzfNoMember ? -1ll : (long long)L.last,
             L.seg == kBgzfNoMember ? -1ll : (long long)L.seg);
      if (L.first != kBgzfNoMember) diff[L.seg] += 1, diff[L.last + 1u] -= 1;
    }
    printf("|");
    int64_t cover = 0;
    for (uint32_t k = 0; k < n; ++k) {
      cover += diff[k];
      if (cover > 0) printf("%u ", k);
    }
    printf("|");
    for (uint32_t k = 0; k < n; ++k) {
      const uint64_t rel = gzfile_seek_rel(out_off, member_unit, m, k);
      printf("%llu %u %d;", (unsigned long long)rel, gzfile_seek_dict_len(rel),
             gzfile_seek_runs_to_final(member_unit, m, k) ? 1 : 0);
    }
    printf("\n");
    free(out_off), free(member_unit), free(begin), free(end), free(point_unit), free(diff);
  }
  fclose(f);
  return 0;
}

static int ok_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t c = 0; c < count; ++c) {
    uint64_t in_len = 0, windows_bytes = 0, words = 0;
    if (fread(&in_len, 8, 1, f) != 1 || fread(&windows_bytes, 8, 1, f) != 1 || fread(&words, 8, 1, f) != 1) return 2;
    uint64_t *index = exact<uint64_t>(words);
    if (words && fread(index, 8, words, f) != words) return 2;
    printf("%d %llu %llu\n", gzfile_seek_index_ok(index, words, windows_bytes, in_len) ? 1 : 0,
           words >= kGzSeekHeadWords
               ? (unsigned long long)gzfile_seek_index_words(index[kGzSeekUnitsAt], index[kGzSeekMembersAt], index[kGzSeekPointsAt])
               : 0ull,
           words >= kGzSeekHeadWords
               ? (unsigned long long)gzfile_seek_windows_bytes(index[kGzSeekPointsAt], index[kGzSeekMembersAt])
               : 0ull);
    free(index);
  }
  fclose(f);
  return 0;
}

static int checks() {
  uint8_t b[32] = {0};
  uint64_t idx[4] = {0}, lo[2] = {1, 5}, hi[2] = {1, 9}, off[3] = {0, 0, 0}, w64 = 0;
  uint32_t w32 = 0;
  int32_t st = 0;
  const uint32_t D = FLATE_HIP_DEVICE_PTRS;
#define BUILD(...) gzfile_seek_index_args(__VA_ARGS__)
  printf("build_ok %d\n", BUILD(b, 4, idx, 4, &w64, b, 4, &w64, &w32, &w32, &w32, &w64, &st, D));
  printf("build_query %d\n", BUILD(b, 4, nullptr, 0, &w64, nullptr, 0, &w64, &w32, &w32, &w32, &w64, &st, 0));
  printf("build_empty_input %d\n", BUILD(nullptr, 0, idx, 4, &w64, b, 4, &w64, &w32, &w32, &w32, &w64, &st, 0));
  printf("build_no_in %d\n", BUILD(nullptr, 4, idx, 4, &w64, b, 4, &w64, &w32, &w32, &w32, &w64, &st, 0));
  printf("build_no_index_with_cap %d\n", BUILD(b, 4, nullptr, 4, &w64, b, 4, &w64, &w32, &w32, &w32, &w64, &st, 0));
  printf("build_no_windows_with_cap %d\n", BUILD(b, 4, idx, 4, &w64, nullptr, 4, &w64, &w32, &w32, &w32, &w64, &st, 0));
  printf("build_no_index_words %d\n", BUILD(b, 4, idx, 4, nullptr, b, 4, &w64, &w32, &w32, &w32, &w64, &st, 0));
  printf("build_no_windows_bytes %d\n", BUILD(b, 4, idx, 4, &w64, b, 4, nullptr, &w32, &w32, &w32, &w64, &st, 0));
  printf("build_no_n_units %d\n", BUILD(b, 4, idx, 4, &w64, b, 4, &w64, nullptr, &w32, &w32, &w64, &st, 0));
  printf("build_no_n_members %d\n", BUILD(b, 4, idx, 4, &w64, b, 4, &w64, &w32, nullptr, &w32, &w64, &st, 0));
  printf("build_no_n_points %d\n", BUILD(b, 4, idx, 4, &w64, b, 4, &w64, &w32, &w32, nullptr, &w64, &st, 0));
  printf("build_no_out_bytes %d\n", BUILD(b, 4, idx, 4, &w64, b, 4, &w64, &w32, &w32, &w32, nullptr, &st, 0));
  printf("build_no_status %d\n", BUILD(b, 4, idx, 4, &w64, b, 4, &w64, &w32, &w32, &w32, &w64, nullptr, 0));
  printf("build_flag_go %d\n", BUILD(b, 4, idx, 4, &w64, b, 4, &w64, &w32, &w32, &w32, &w64, &st, FLATE_HIP_COMPAT_GO));
  // the read: an index of one member of one unit over a file of 32 bytes, T = 10
  uint64_t one[kGzSeekHeadWords + 9] = {kGzSeekMagic, kGzSeekVersion, 32, 10, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0,
                                        80, 100, 0, 10, 0, 32, 0, 1, 0};
  const uint64_t W = kGzSeekHeadWords + 9;
  uint64_t none[kGzSeekHeadWords] = {kGzSeekMagic, kGzSeekVersion, 0, 0, 1, 0, 0, 0};
#define READ(...) gzfile_ranges_args(__VA_ARGS__)
  printf("read_ok %d\n", READ(b, 32, one, W, nullptr, 0, lo, hi, 2, b, 4, off, D));
  printf("read_size_query %d\n", READ(b, 32, one, W, nullptr, 0, lo, hi, 2, nullptr, 0, off, 0));
  printf("read_no_ranges %d\n", READ(b, 32, one, W, nullptr, 0, nullptr, nullptr, 0, b, 4, nullptr, 0));
  printf("read_empty_file %d\n", READ(nullptr, 0, none, kGzSeekHeadWords, nullptr, 0, lo, hi, 2, b, 4, off, 0));
  printf("read_no_in %d\n", READ(nullptr, 32, one, W, nullptr, 0, lo, hi, 2, b, 4, off, 0));
  printf("read_no_index %d\n", READ(b, 32, nullptr, W, nullptr, 0, lo, hi, 2, b, 4, off, 0));
  printf("read_no_begin %d\n", READ(b, 32, one, W, nullptr, 0, nullptr, hi, 2, b, 4, off, 0));
  printf("read_no_end %d\n", READ(b, 32, one, W, nullptr, 0, lo, nullptr, 2, b, 4, off, 0));
  printf("read_no_out_off %d\n", READ(b, 32, one, W, nullptr, 0, lo, hi, 2, b, 4, nullptr, 0));
  printf("read_no_out_with_cap %d\n", READ(b, 32, one, W, nullptr, 0, lo, hi, 2, nullptr, 4, off, 0));
  printf("read_backwards %d\n", READ(b, 32, one, W, nullptr, 0, hi, lo, 2, b, 4, off, 0));
  printf("read_in_len_not_the_index %d\n", READ(b, 31, one, W, nullptr, 0, lo, hi, 2, b, 4, off, 0));
  printf("read_windows_without_buffer %d\n", READ(b, 32, one, W, nullptr, 32768, lo, hi, 2, b, 4, off, 0));
  printf("read_windows_the_index_has_not %d\n", READ(b, 32, one, W, b, 32768, lo, hi, 2, b, 4, off, 0));
  printf("read_flag_size_only %d\n", READ(b, 32, one, W, nullptr, 0, lo, hi, 2, b, 4, off, FLATE_HIP_SIZE_ONLY));
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "rule")) return rule_file(argv[2]);
  if (argc == 3 && !strcmp(argv[1], "ok")) return ok_file(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
  fprintf(stderr, "usage: %s rule FILE | ok FILE | checks\n", argv[0]);
  return 2;
}
