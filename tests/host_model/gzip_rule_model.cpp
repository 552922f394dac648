// gzip_rule_model.cpp -- the gzip member rule and walk (moonbit-flate_amd/csrc/gzip_rule.h) and the gzip argument
// checks (api_checks.h) as a stand-alone CPU program: the very functions the discovery kernels and the entry points
// compile, driven by tests/test_gzip_rule_model.py and compared there with tests/gzip_ref.py.
//   gzip_rule_model walk FILE    FILE = u32 count, then per case: u64 member_max, u64 length, the bytes, u64 n_cand and
//                                per candidate u64 offset, i64 status, u64 used, u64 size (the table of the size-only
//                                decodes, which this program cannot make itself).  One line per case:
//                                rc n_members err_off | member offsets ... | output offsets ... | the rule at EVERY
//                                offset as "offset:header length" for the offsets where a member can start
//   gzip_rule_model checks       one line per argument-check call: name value
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "api_checks.h"
#include "gzip_rule.h"

using namespace flate;

static int walk_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint64_t member_max = 0, len = 0, n_cand = 0;
    if (fread(&member_max, 8, 1, f) != 1 || fread(&len, 8, 1, f) != 1) return 2;
    // (an exact allocation: a read past in_len is a heap overflow the sanitizer reports)
    uint8_t *buf = (uint8_t *)malloc(len ? len : 1);
    if (len && fread(buf, 1, len, f) != len) return 2;
    if (fread(&n_cand, 8, 1, f) != 1) return 2;
    std::vector<GzipCand> cand(n_cand);
    for (auto &c : cand) {
      uint64_t w[4];
      if (fread(w, 8, 4, f) != 4) return 2;
      c.off = w[0], c.s = (int32_t)(int64_t)w[1], c.used = w[2], c.z = w[3];
    }
    std::vector<uint64_t> moff(len / 18 + 2), ooff(len / 18 + 2);
    uint64_t n = 0;
    int64_t err = -1;
    const int rc = gzip_serial_walk(buf, len, member_max, cand.data(), n_cand, &n, &err, moff.data(), ooff.data());
    printf("%d %llu %lld |", rc, (unsigned long long)n, (long long)err);
    for (uint64_t i = 0; i <= n; ++i) printf(" %llu", (unsigned long long)moff[i]);
    printf(" |");
    for (uint64_t i = 0; i <= n; ++i) printf(" %llu", (unsigned long long)ooff[i]);
    printf(" |");
    for (uint64_t p = 0; p < len; ++p) {
      const uint64_t hl = gzip_header_len(buf + p, gzip_range_end(p, len, member_max) - p);
      if (hl) printf(" %llu:%llu", (unsigned long long)p, (unsigned long long)hl);
    }
    printf("\n");
    free(buf);
  }
  fclose(f);
  return 0;
}

static int checks() {
  uint8_t b[4] = {0};
  uint64_t w = 0;
  uint32_t n = 0;
  const uint32_t D = FLATE_HIP_DEVICE_PTRS, G = FLATE_HIP_COMPAT_GO;
  printf("index_ok %d\n", gzip_index_args(b, 4, &w, &w, &n, &w, D));
  printf("index_query_ok %d\n", gzip_index_args(b, 4, nullptr, nullptr, &n, &w, 0));
  printf("index_one_array %d\n", gzip_index_args(b, 4, &w, nullptr, &n, &w, 0));
  printf("index_other_array %d\n", gzip_index_args(b, 4, nullptr, &w, &n, &w, 0));
  printf("index_no_count %d\n", gzip_index_args(b, 4, &w, &w, nullptr, &w, 0));
  printf("index_no_bytes %d\n", gzip_index_args(b, 4, &w, &w, &n, nullptr, 0));
  printf("index_no_in %d\n", gzip_index_args(nullptr, 4, &w, &w, &n, &w, 0));
  printf("index_empty_ok %d\n", gzip_index_args(nullptr, 0, &w, &w, &n, &w, 0));
  printf("index_flag_go %d\n", gzip_index_args(b, 4, &w, &w, &n, &w, G));
  printf("index_flag_size_only %d\n", gzip_index_args(b, 4, &w, &w, &n, &w, FLATE_HIP_SIZE_ONLY));
  printf("read_ok %d\n", gzip_read_args(b, 4, b, 4, &w, D));
  printf("read_no_out_no_cap_ok %d\n", gzip_read_args(b, 4, nullptr, 0, &w, 0));
  printf("read_no_out %d\n", gzip_read_args(b, 4, nullptr, 4, &w, 0));
  printf("read_no_len %d\n", gzip_read_args(b, 4, b, 4, nullptr, 0));
  printf("read_no_in %d\n", gzip_read_args(nullptr, 4, b, 4, &w, 0));
  printf("read_empty_ok %d\n", gzip_read_args(nullptr, 0, nullptr, 0, &w, 0));
  printf("read_flag_size_only %d\n", gzip_read_args(b, 4, b, 4, &w, FLATE_HIP_SIZE_ONLY));
  printf("member_max_0 %d\n", gzip_member_max_ok(0) ? 1 : 0);
  printf("member_max_1 %d\n", gzip_member_max_ok(1) ? 1 : 0);
  printf("member_max_4096 %d\n", gzip_member_max_ok(4096) ? 1 : 0);
  printf("member_max_default %d\n", gzip_member_max_ok((int64_t)kGzipMemberMax) ? 1 : 0);
  printf("member_max_2_28 %d\n", gzip_member_max_ok(1ll << 28) ? 1 : 0);
  printf("member_max_negative %d\n", gzip_member_max_ok(-1) ? 1 : 0);
  printf("dead_eof_unclipped %d\n", gzip_dead_code(kGzipEof, 10, 4000, 4096));
  printf("dead_eof_clipped %d\n", gzip_dead_code(kGzipEof, 10, 5000, 4096));
  printf("dead_eof_at_the_edge %d\n", gzip_dead_code(kGzipEof, 10, 4106, 4096));
  printf("dead_corrupt_clipped %d\n", gzip_dead_code(kGzipCorrupt, 10, 5000, 4096));
  printf("dead_four_gib %d\n", gzip_dead_code(kGzipOutTooSmall, 0, 100, 4096));
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "walk")) return walk_file(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
  fprintf(stderr, "usage: %s walk FILE | checks\n", argv[0]);
  return 2;
}
