// gzfile_serial_driver.cpp -- drives the C++ host mirror's Engine::set_option("gzfile_serial_max"), index_gzfile,
// decompress_gzfile and Engine::gzfile_last_route for tests/test_host_cpp_gzfile_serial.py.
//   gzfile_serial_driver CASES S    CASES = u32 count, then per case u64 length, bytes: a file.  Two lines per case:
//     r <k> <status> <n_units> <n_members> <serial_members> <unit_members> <find_from> | unit bits | member units
//     d <k> <status> <n_units> <n_members> <serial_members> <unit_members> <find_from> <hex of the bytes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flate_host.hpp"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  flate_host::Engine e(0);
  if (!e.ok()) {
    fprintf(stderr, "no engine: %d\n", e.status());
    return 3;
  }
  if (e.set_option("gzfile_serial_max", 1ll << 28) != FLATE_HIP_E_INVALID) return 4;  // (one above the limit)
  if (e.set_option("gzfile_serial_max", atoll(argv[2])) != 0) return 4;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint64_t len = 0;
    if (fread(&len, 8, 1, f) != 1) return 2;
    std::vector<uint8_t> data(len);
    if (len && fread(data.data(), 1, len, f) != len) return 2;
    flate_host::GzFileIndex ix;
    (void)flate_host::index_gzfile(e, data, ix);
    flate_host::Engine::GzFileRoute rt = e.gzfile_last_route();
    printf("r %u %d %u %u %u %u %llu", k, ix.status, ix.n_units, ix.n_members, rt.serial_members, rt.unit_members,
           (unsigned long long)rt.find_from);
    for (const auto *v : {&ix.unit_bit, &ix.member_unit}) {
      printf(" |");
      for (uint64_t b : *v) printf(" %llu", (unsigned long long)b);
    }
    printf("\n");
    std::vector<uint8_t> out;
    flate_host::GzFileInfo info;
    (void)flate_host::decompress_gzfile(e, data, out, &info);
    rt = e.gzfile_last_route();
    printf("d %u %d %u %u %u %u %llu ", k, info.status, info.n_units, info.n_members, rt.serial_members, rt.unit_members,
           (unsigned long long)rt.find_from);
    for (uint8_t b : out) printf("%02x", b);
    printf("\n");
  }
  fclose(f);
  return 0;
}
