// bgzf_index_model.cpp -- the BGZF member rule (moonbit-flate_amd/csrc/bgzf_rule.h) and the BGZF argument checks
// (api_checks.h) as a stand-alone CPU program: the very functions the discovery kernels and the entry points
// compile, driven by tests/test_bgzf_index_model.py and compared there with the serial walk of tests/bgzf_ref.py.
//   bgzf_index_model walk FILE    FILE = u32 count, then per case u64 length + bytes.  One line per case:
//                                 rc n_members err_off eof_marker out_bytes | member offsets ... | the rule at EVERY offset
//                                 as "offset:total" for the offsets where a member can be read
//   bgzf_index_model checks       one line per argument-check call: name value
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "api_checks.h"
#include "bgzf_rule.h"

using namespace flate;

static size_t bound_model(size_t n) { return 2 * n + 400; }

static int walk_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint64_t len = 0;
    if (fread(&len, 8, 1, f) != 1) return 2;
    // (an exact allocation: a read past in_len is a heap overflow the sanitizer reports)
    uint8_t *buf = (uint8_t *)malloc(len ? len : 1);
    if (len && fread(buf, 1, len, f) != len) return 2;
    std::vector<uint64_t> off(len / 26 + 2);
    uint64_t n = 0;
    int64_t err = -1;
    const int rc = bgzf_serial_walk(buf, len, &n, &err, off.data());
    uint64_t out_bytes = 0;
    int eof = 0;
    if (rc == 0) {
      for (uint64_t i = 0; i < n; ++i) {
        const uint8_t *t = buf + off[i + 1] - 4;
        out_bytes += t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
      }
      if (n) eof = bgzf_is_eof_marker(buf + off[n - 1], (uint32_t)(off[n] - off[n - 1])) ? 1 : 0;
    }
    printf("%d %llu %lld %d %llu |", rc, (unsigned long long)n, (long long)err, eof, (unsigned long long)out_bytes);
    if (rc == 0)
      for (uint64_t i = 0; i <= n; ++i) printf(" %llu", (unsigned long long)off[i]);
    printf(" |");
    for (uint64_t p = 0; p < len; ++p) {
      const uint32_t t = bgzf_member_total(buf + p, len - p);
      if (t) printf(" %llu:%u", (unsigned long long)p, t);
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
  printf("block_default %u\n", bgzf_block_bytes(0));
  printf("block_1 %u\n", bgzf_block_bytes(1));
  printf("block_65535 %u\n", bgzf_block_bytes(65535));
  printf("block_65536 %u\n", bgzf_block_bytes(65536));
  printf("blocks_0 %llu\n", (unsigned long long)bgzf_n_blocks(0, 65280));
  printf("blocks_65280 %llu\n", (unsigned long long)bgzf_n_blocks(65280, 65280));
  printf("blocks_65281 %llu\n", (unsigned long long)bgzf_n_blocks(65281, 65280));
  printf("bound_0 %llu\n", (unsigned long long)bgzf_file_bound(0, 0, bound_model));
  printf("bound_1 %llu\n", (unsigned long long)bgzf_file_bound(1, 0, bound_model));
  printf("bound_tail %llu\n", (unsigned long long)bgzf_file_bound(2 * 4096 + 5, 4096, bound_model));
  printf("bound_refused %llu\n", (unsigned long long)bgzf_file_bound(100, 65536, bound_model));
  printf("write_ok %d\n", bgzf_write_args(b, 4, 0, b, &w, D | G));
  printf("write_empty_ok %d\n", bgzf_write_args(nullptr, 0, 0, b, &w, 0));
  printf("write_no_in %d\n", bgzf_write_args(nullptr, 4, 0, b, &w, 0));
  printf("write_no_out %d\n", bgzf_write_args(b, 4, 0, nullptr, &w, 0));
  printf("write_no_len %d\n", bgzf_write_args(b, 4, 0, b, nullptr, 0));
  printf("write_block_65536 %d\n", bgzf_write_args(b, 4, 65536, b, &w, 0));
  printf("write_flag_size_only %d\n", bgzf_write_args(b, 4, 0, b, &w, FLATE_HIP_SIZE_ONLY));
  printf("write_too_many_blocks %d\n", bgzf_write_args(b, 0xffffffffull, 1, b, &w, 0));
  printf("write_most_blocks %d\n", bgzf_write_args(b, 0xfffffffeull, 1, b, &w, 0));
  printf("index_ok %d\n", bgzf_index_args(b, 4, &w, &w, &n, &w, D));
  printf("index_query_ok %d\n", bgzf_index_args(b, 4, nullptr, nullptr, &n, &w, 0));
  printf("index_one_array %d\n", bgzf_index_args(b, 4, &w, nullptr, &n, &w, 0));
  printf("index_other_array %d\n", bgzf_index_args(b, 4, nullptr, &w, &n, &w, 0));
  printf("index_no_count %d\n", bgzf_index_args(b, 4, &w, &w, nullptr, &w, 0));
  printf("index_no_bytes %d\n", bgzf_index_args(b, 4, &w, &w, &n, nullptr, 0));
  printf("index_no_in %d\n", bgzf_index_args(nullptr, 4, &w, &w, &n, &w, 0));
  printf("index_empty_ok %d\n", bgzf_index_args(nullptr, 0, &w, &w, &n, &w, 0));
  printf("index_flag_go %d\n", bgzf_index_args(b, 4, &w, &w, &n, &w, G));
  printf("read_ok %d\n", bgzf_read_args(b, 4, b, 4, &w, D));
  printf("read_no_out_no_cap_ok %d\n", bgzf_read_args(b, 4, nullptr, 0, &w, 0));
  printf("read_no_out %d\n", bgzf_read_args(b, 4, nullptr, 4, &w, 0));
  printf("read_no_len %d\n", bgzf_read_args(b, 4, b, 4, nullptr, 0));
  printf("read_no_in %d\n", bgzf_read_args(nullptr, 4, b, 4, &w, 0));
  printf("read_flag_size_only %d\n", bgzf_read_args(b, 4, b, 4, &w, FLATE_HIP_SIZE_ONLY));
  printf("first_cap_0 %u\n", bgzf_first_cap(0));
  printf("first_cap_1m %u\n", bgzf_first_cap(1u << 20));
  printf("rounds_0 %u\n", bgzf_rounds(0));
  printf("rounds_2 %u\n", bgzf_rounds(2));
  printf("rounds_3 %u\n", bgzf_rounds(3));
  printf("rounds_4094 %u\n", bgzf_rounds(4094));
  printf("rounds_4095 %u\n", bgzf_rounds(4095));
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "walk")) return walk_file(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
  fprintf(stderr, "usage: %s walk FILE | checks\n", argv[0]);
  return 2;
}
