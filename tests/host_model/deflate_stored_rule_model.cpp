// deflate_stored_rule_model.cpp -- the stored-header rule of the option "one_stored_units"
// (moonbit-flate_amd/csrc/deflate_block_rule.h: deflate_stored_header_ok), the option's check (api_checks.h) and the
// check of a seek index's rule word (seek_index_rule.h, gzfile_seek_rule.h) as a stand-alone CPU program: the very
// functions the discovery kernels and the entry points compile, driven by tests/test_stored_rule_model.py and compared
// there with tests/stored_ref.py.
//   deflate_stored_rule_model rule FILE   FILE = u32 count, then per case: u64 length, the bytes, u64 n and n u64 bit
//                                         offsets (n == 0: EVERY bit offset of the stream, and eight behind its end).
//                                         One line per case: the offsets at which the rule holds
//   deflate_stored_rule_model checks      one line per check: name value
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "api_checks.h"
#include "deflate_block_rule.h"
#include "gzfile_seek_rule.h"
#include "seek_index_rule.h"

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
    for (uint64_t b : bits)
      if (deflate_stored_header_ok(buf, len, b)) printf(" %llu", (unsigned long long)b);
    printf("\n");
    free(buf);
  }
  fclose(f);
  return 0;
}

static int checks() {
  printf("stored_units_0 %d\n", one_stored_units_ok(0) ? 1 : 0);
  printf("stored_units_1 %d\n", one_stored_units_ok(1) ? 1 : 0);
  printf("stored_units_2 %d\n", one_stored_units_ok(2) ? 1 : 0);
  printf("stored_units_negative %d\n", one_stored_units_ok(-1) ? 1 : 0);
  printf("stored_units_large %d\n", one_stored_units_ok(1ll << 32) ? 1 : 0);
  // the rule word of the two seek indexes: a head of zeros is an index from before the word existed
  uint64_t one[kSeekHeadWords] = {0}, gz[kGzSeekHeadWords] = {0};
  printf("rule_word_at %u %u\n", kSeekRuleAt, kGzSeekRuleAt);
  const uint64_t values[5] = {0, 1, 2, 1ull << 32, ~0ull};
  for (int i = 0; i < 5; ++i) {
    one[kSeekRuleAt] = gz[kGzSeekRuleAt] = values[i];
    printf("rule_word_%d %d %d\n", i, seek_index_rule_ok(one) ? 1 : 0, gzfile_seek_index_rule_ok(gz) ? 1 : 0);
  }
  // (no other word is the rule's)
  one[kSeekRuleAt] = gz[kGzSeekRuleAt] = 0;
  for (uint32_t k = 0; k < kSeekHeadWords; ++k)
    if (k != kSeekRuleAt) one[k] = 7;
  for (uint32_t k = 0; k < kGzSeekHeadWords; ++k)
    if (k != kGzSeekRuleAt) gz[k] = 7;
  printf("rule_word_alone %d %d\n", seek_index_rule_ok(one) ? 1 : 0, gzfile_seek_index_rule_ok(gz) ? 1 : 0);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "rule")) return rule_file(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
  fprintf(stderr, "usage: %s rule FILE | checks\n", argv[0]);
  return 2;
}
