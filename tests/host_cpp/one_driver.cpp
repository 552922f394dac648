// one_driver.cpp -- drives the C++ host mirror's flate_host::index_one and decompress_one for tests/test_host_cpp_one.py.
//   one_driver CASES read    per case: d <k> <status> <n_units> <err_off> <n_candidates> <message> <hex of the bytes>
//   one_driver CASES    CASES = u32 count, then per case u32 wrap (0 raw, 1 zlib, 2 gzip), u64 length, bytes: a stream.
//   One line per case:
//     r <k> <status> <n_units> <out_bytes> <err_off> <n_candidates> <message with _ for spaces> | unit bits | out offsets
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "flate_host.hpp"

int main(int argc, char **argv) {
  if (argc != 2 && argc != 3) return 2;
  const bool read = argc == 3;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  flate_host::Engine e(0);
  if (!e.ok()) {
    fprintf(stderr, "no engine: %d\n", e.status());
    return 3;
  }
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t wrap = 0;
    uint64_t len = 0;
    if (fread(&wrap, 4, 1, f) != 1 || fread(&len, 8, 1, f) != 1) return 2;
    std::vector<uint8_t> data(len);
    if (len && fread(data.data(), 1, len, f) != len) return 2;
    const flate_host::Wrap w = wrap == 1 ? flate_host::Wrap::Zlib : wrap == 2 ? flate_host::Wrap::Gzip : flate_host::Wrap::Raw;
    if (read) {
      std::vector<uint8_t> out;
      flate_host::OneInfo info;
      flate_host::Err err = flate_host::decompress_one(e, data, w, out, &info);
      std::string msg = err ? err->msg : "-";
      for (char &ch : msg)
        if (ch == ' ') ch = '_';
      printf("d %u %d %u %lld %u %s ", k, info.status, info.n_units, (long long)info.err_off, info.n_candidates, msg.c_str());
      for (uint8_t b : out) printf("%02x", b);
      printf("\n");
      continue;
    }
    flate_host::OneIndex ix;
    flate_host::Err err = flate_host::index_one(e, data, w, ix);
    std::string msg = err ? err->msg : "-";
    for (char &ch : msg)
      if (ch == ' ') ch = '_';
    printf("r %u %d %u %llu %lld %u %s |", k, ix.status, ix.n_units, (unsigned long long)ix.out_bytes,
           (long long)ix.err_off, ix.n_candidates, msg.c_str());
    for (uint64_t b : ix.unit_bit) printf(" %llu", (unsigned long long)b);
    printf(" |");
    for (uint64_t b : ix.out_off) printf(" %llu", (unsigned long long)b);
    printf("\n");
  }
  fclose(f);
  return 0;
}
