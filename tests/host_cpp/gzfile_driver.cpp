// gzfile_driver.cpp -- drives the C++ host mirror's flate_host::index_gzfile and decompress_gzfile for
// tests/test_host_cpp_gzfile.py.
//   gzfile_driver CASES [read]    CASES = u32 count, then per case u64 length, bytes: a file.  One line per case:
//     r <k> <status> <n_units> <n_members> <out_bytes> <bad_member> <err_off> <stream_err_off> <message with _ for spaces>
//       | unit bits | out offsets | member offsets | member units
//     d <k> <status> <n_units> <n_members> <bad_member> <err_off> <stream_err_off> <message> <hex of the bytes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "flate_host.hpp"

static std::string text_of(const flate_host::Err &err) {
  std::string msg = err ? err->msg : "-";
  for (char &ch : msg)
    if (ch == ' ') ch = '_';
  return msg;
}

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
    uint64_t len = 0;
    if (fread(&len, 8, 1, f) != 1) return 2;
    std::vector<uint8_t> data(len);
    if (len && fread(data.data(), 1, len, f) != len) return 2;
    if (read) {
      std::vector<uint8_t> out;
      flate_host::GzFileInfo info;
      const flate_host::Err err = flate_host::decompress_gzfile(e, data, out, &info);
      printf("d %u %d %u %u %u %lld %lld %s ", k, info.status, info.n_units, info.n_members, info.bad_member,
             (long long)info.err_off, (long long)info.stream_err_off, text_of(err).c_str());
      for (uint8_t b : out) printf("%02x", b);
      printf("\n");
      continue;
    }
    flate_host::GzFileIndex ix;
    const flate_host::Err err = flate_host::index_gzfile(e, data, ix);
    printf("r %u %d %u %u %llu %u %lld %lld %s", k, ix.status, ix.n_units, ix.n_members, (unsigned long long)ix.out_bytes,
           ix.bad_member, (long long)ix.err_off, (long long)ix.stream_err_off, text_of(err).c_str());
    for (const auto *v : {&ix.unit_bit, &ix.out_off, &ix.member_off, &ix.member_unit}) {
      printf(" |");
      for (uint64_t b : *v) printf(" %llu", (unsigned long long)b);
    }
    printf("\n");
  }
  fclose(f);
  return 0;
}
