// gzip_driver.cpp -- drives the C++ host mirror's flate_host::decompress_gzip for tests/test_host_cpp_gzip.py.
//   gzip_driver CASES    CASES = u32 count, then per case u64 length, bytes: a file to read.  One line per case:
//     r <k> <status> <n_members> <bad_member> <err_off> <n_candidates> <message with _ for spaces> <hex of the bytes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "flate_host.hpp"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
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
    uint64_t len = 0;
    if (fread(&len, 8, 1, f) != 1) return 2;
    std::vector<uint8_t> data(len), out;
    if (len && fread(data.data(), 1, len, f) != len) return 2;
    flate_host::GzipInfo info;
    flate_host::Err err = flate_host::decompress_gzip(e, data, out, &info);
    std::string msg = err ? err->msg : "-";
    for (char &ch : msg)
      if (ch == ' ') ch = '_';
    printf("r %u %d %u %u %lld %u %s ", k, info.status, info.n_members, info.bad_member, (long long)info.err_off,
           info.n_candidates, msg.c_str());
    for (uint8_t b : out) printf("%02x", b);
    printf("\n");
  }
  fclose(f);
  return 0;
}
