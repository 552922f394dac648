// deflate_block_rule_model.cpp -- the dynamic-header rule (moonbit-flate_amd/csrc/deflate_block_rule.h) and the argument
// checks of flate_hip_inflate_one_index (api_checks.h) as a stand-alone CPU program: the very functions the discovery
// kernels and the entry point compile, driven by tests/test_deflate_block_rule_model.py and compared there with
// tests/one_ref.py.
//   deflate_block_rule_model rule FILE   FILE = u32 count, then per case: u64 length, the bytes, u64 n and n u64 bit
//                                        offsets (n == 0: EVERY bit offset of the stream, and eight behind its end).
//                                        One line per case: the offsets at which the rule holds; the head test
//                                        (dblk_head_ok, what the kernel runs in LDS first) must hold wherever it does
//   deflate_block_rule_model checks      one line per argument-check call: name value
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "api_checks.h"
#include "deflate_block_rule.h"

using namespace flate;

static int rule_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint64_t len = 0, n = 0;
    if (fread(&len, 8, 1, f) != 1) return 2;
    // (an exact allocation: a read past the stream's end is a heap overflow the sanitizer reports)
    uint8_t *buf = (uint8_t *)malloc(len ? len : 1);
    if (len && fread(buf, 1, len, f) != len) return 2;
    if (fread(&n, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> bits(n);
    if (n && fread(bits.data(), 8, n, f) != n) return 2;
    if (!n)
      for (uint64_t b = 0; b < 8 * len + 8; ++b) bits.push_back(b);
    for (uint64_t b : bits) {
      const bool hit = deflate_dyn_header_ok(buf, len, b);
      if (hit && !dblk_head_ok(buf + (b >> 3), 8 * (len - (b >> 3)), b & 7)) {
        fprintf(stderr, "the head test refuses bit %llu, which the rule takes\n", (unsigned long long)b);
        return 3;
      }
      if (hit) printf(" %llu", (unsigned long long)b);
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
  int32_t s = 0;
  const uint32_t D = FLATE_HIP_DEVICE_PTRS, G = FLATE_HIP_COMPAT_GO, Z = FLATE_HIP_WRAP_GZIP;
  printf("index_ok %d\n", one_index_args(b, 4, Z, &w, &w, &n, &w, &s, D));
  printf("index_raw_ok %d\n", one_index_args(b, 4, FLATE_HIP_WRAP_RAW, &w, &w, &n, &w, &s, 0));
  printf("index_zlib_ok %d\n", one_index_args(b, 4, FLATE_HIP_WRAP_ZLIB, &w, &w, &n, &w, &s, 0));
  printf("index_wrap_3 %d\n", one_index_args(b, 4, 3, &w, &w, &n, &w, &s, 0));
  printf("index_query_ok %d\n", one_index_args(b, 4, Z, nullptr, nullptr, &n, &w, &s, 0));
  printf("index_one_array %d\n", one_index_args(b, 4, Z, &w, nullptr, &n, &w, &s, 0));
  printf("index_other_array %d\n", one_index_args(b, 4, Z, nullptr, &w, &n, &w, &s, 0));
  printf("index_no_count %d\n", one_index_args(b, 4, Z, &w, &w, nullptr, &w, &s, 0));
  printf("index_no_bytes %d\n", one_index_args(b, 4, Z, &w, &w, &n, nullptr, &s, 0));
  printf("index_no_status %d\n", one_index_args(b, 4, Z, &w, &w, &n, &w, nullptr, 0));
  printf("index_no_in %d\n", one_index_args(nullptr, 4, Z, &w, &w, &n, &w, &s, 0));
  printf("index_empty_ok %d\n", one_index_args(nullptr, 0, Z, &w, &w, &n, &w, &s, 0));
  printf("index_flag_go %d\n", one_index_args(b, 4, Z, &w, &w, &n, &w, &s, G));
  printf("index_flag_size_only %d\n", one_index_args(b, 4, Z, &w, &w, &n, &w, &s, FLATE_HIP_SIZE_ONLY));
  printf("one_ok %d\n", one_args(b, 4, Z, b, 4, &w, &s, D));
  printf("one_query_ok %d\n", one_args(b, 4, Z, nullptr, 0, &w, &s, 0));
  printf("one_no_out %d\n", one_args(b, 4, Z, nullptr, 4, &w, &s, 0));
  printf("one_no_len %d\n", one_args(b, 4, Z, b, 4, nullptr, &s, 0));
  printf("one_no_status %d\n", one_args(b, 4, Z, b, 4, &w, nullptr, 0));
  printf("one_no_in %d\n", one_args(nullptr, 4, Z, b, 4, &w, &s, 0));
  printf("one_empty_ok %d\n", one_args(nullptr, 0, FLATE_HIP_WRAP_RAW, nullptr, 0, &w, &s, 0));
  printf("one_wrap_3 %d\n", one_args(b, 4, 3, b, 4, &w, &s, 0));
  printf("one_flag_go %d\n", one_args(b, 4, Z, b, 4, &w, &s, G));
  printf("one_flag_size_only %d\n", one_args(b, 4, Z, b, 4, &w, &s, FLATE_HIP_SIZE_ONLY));
  printf("round_units_0 %d\n", one_round_units_ok(0) ? 1 : 0);
  printf("round_units_7 %d\n", one_round_units_ok(7) ? 1 : 0);
  printf("round_units_65536 %d\n", one_round_units_ok(65536) ? 1 : 0);
  printf("round_units_65537 %d\n", one_round_units_ok(65537) ? 1 : 0);
  printf("unit_max_0 %d\n", one_unit_max_ok(0) ? 1 : 0);
  printf("unit_max_1 %d\n", one_unit_max_ok(1) ? 1 : 0);
  printf("unit_max_default %d\n", one_unit_max_ok((int64_t)kOneUnitMax) ? 1 : 0);
  printf("unit_max_above %d\n", one_unit_max_ok((1ll << 28) + 1) ? 1 : 0);
  printf("unit_max_negative %d\n", one_unit_max_ok(-1) ? 1 : 0);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "rule")) return rule_file(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
  fprintf(stderr, "usage: %s rule FILE | checks\n", argv[0]);
  return 2;
}
