// gzfile_rule_model.cpp -- THE HOP between the members of a gzip file (moonbit-flate_amd/csrc/gzfile_rule.h) and the
// argument checks of the two gzfile calls (api_checks.h) as a stand-alone CPU program: the very functions the link
// kernel and the entry points compile, driven by tests/test_gzfile_rule_model.py and tests/test_gzfile_abi.py and
// compared there with tests/gzfile_ref.py.
//   gzfile_rule_model hop FILE   FILE = u32 count, then per case: u64 length, the bytes, u64 n and n u64 bits.  One line
//                                per case: "kind:e:bit" of gzfile_hop at every bit | "offset:first bit" of
//                                gzfile_first_bit for the offsets where a member can start
//   gzfile_rule_model checks     one line per argument-check call: name value
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "api_checks.h"
#include "gzfile_rule.h"

using namespace flate;

static int hop_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint64_t len = 0, n = 0;
    if (fread(&len, 8, 1, f) != 1) return 2;
    // (an exact allocation: a read past in_len is a heap overflow the sanitizer reports)
    uint8_t *buf = (uint8_t *)malloc(len ? len : 1);
    if (len && fread(buf, 1, len, f) != len) return 2;
    if (fread(&n, 8, 1, f) != 1) return 2;
    std::vector<uint64_t> bits(n);
    if (n && fread(bits.data(), 8, n, f) != n) return 2;
    for (uint64_t b : bits) {
      const GzHop h = gzfile_hop(buf, len, b);
      printf(" %u:%llu:%llu", h.kind, (unsigned long long)h.e, (unsigned long long)h.bit);
    }
    printf(" |");
    for (uint64_t p = 0; p < len; ++p) {
      const uint64_t bit = gzfile_first_bit(buf, len, p);
      if (bit) printf(" %llu:%llu", (unsigned long long)p, (unsigned long long)bit);
    }
    printf("\n");
    free(buf);
  }
  fclose(f);
  return 0;
}

static int checks() {
  uint8_t b[4] = {0};
  uint64_t w = 0, a1[2] = {0}, a2[2] = {0};
  uint32_t u = 0, m = 0;
  int32_t st = 0;
  const uint32_t dev = FLATE_HIP_DEVICE_PTRS;
  auto ix = [&](const char *what, int rc) { printf("index %s %d\n", what, rc); };
  ix("ok", gzfile_index_args(b, 4, a1, a2, a1, a2, &u, &m, &w, &st, 0));
  ix("ok_device", gzfile_index_args(b, 4, a1, a2, a1, a2, &u, &m, &w, &st, dev));
  ix("ok_query", gzfile_index_args(b, 4, nullptr, nullptr, nullptr, nullptr, &u, &m, &w, &st, 0));
  ix("ok_units_only", gzfile_index_args(b, 4, a1, a2, nullptr, nullptr, &u, &m, &w, &st, 0));
  ix("ok_members_only", gzfile_index_args(b, 4, nullptr, nullptr, a1, a2, &u, &m, &w, &st, 0));
  ix("ok_empty", gzfile_index_args(nullptr, 0, a1, a2, a1, a2, &u, &m, &w, &st, 0));
  ix("no_in", gzfile_index_args(nullptr, 4, a1, a2, a1, a2, &u, &m, &w, &st, 0));
  ix("no_unit_bit", gzfile_index_args(b, 4, nullptr, a2, a1, a2, &u, &m, &w, &st, 0));
  ix("no_out_off", gzfile_index_args(b, 4, a1, nullptr, a1, a2, &u, &m, &w, &st, 0));
  ix("no_member_off", gzfile_index_args(b, 4, a1, a2, nullptr, a2, &u, &m, &w, &st, 0));
  ix("no_member_unit", gzfile_index_args(b, 4, a1, a2, a1, nullptr, &u, &m, &w, &st, 0));
  ix("no_n_units", gzfile_index_args(b, 4, a1, a2, a1, a2, nullptr, &m, &w, &st, 0));
  ix("no_n_members", gzfile_index_args(b, 4, a1, a2, a1, a2, &u, nullptr, &w, &st, 0));
  ix("no_out_bytes", gzfile_index_args(b, 4, a1, a2, a1, a2, &u, &m, nullptr, &st, 0));
  ix("no_status", gzfile_index_args(b, 4, a1, a2, a1, a2, &u, &m, &w, nullptr, 0));
  ix("flag_2", gzfile_index_args(b, 4, a1, a2, a1, a2, &u, &m, &w, &st, 2));
  ix("flag_size_only", gzfile_index_args(b, 4, a1, a2, a1, a2, &u, &m, &w, &st, dev | FLATE_HIP_SIZE_ONLY));
  auto rd = [&](const char *what, int rc) { printf("read %s %d\n", what, rc); };
  rd("ok", gzfile_read_args(b, 4, b, 4, &w, &st, 0));
  rd("ok_device", gzfile_read_args(b, 4, b, 4, &w, &st, dev));
  rd("ok_size_query", gzfile_read_args(b, 4, nullptr, 0, &w, &st, 0));
  rd("ok_empty", gzfile_read_args(nullptr, 0, nullptr, 0, &w, &st, 0));
  rd("no_in", gzfile_read_args(nullptr, 4, b, 4, &w, &st, 0));
  rd("no_out", gzfile_read_args(b, 4, nullptr, 4, &w, &st, 0));
  rd("no_out_len", gzfile_read_args(b, 4, b, 4, nullptr, &st, 0));
  rd("no_status", gzfile_read_args(b, 4, b, 4, &w, nullptr, 0));
  rd("flag_4", gzfile_read_args(b, 4, b, 4, &w, &st, 4));
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && argv[1][0] == 'h') return hop_file(argv[2]);
  if (argc == 2 && argv[1][0] == 'c') return checks();
  return 2;
}
