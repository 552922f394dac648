// gzfile_seek_driver.cpp -- drives the C++ host mirror's flate_host::seek_index_gzfile and decompress_gzfile_ranges for
// tests/test_host_cpp_gzfile_seek.py.
//   gzfile_seek_driver CASES   CASES = u32 count, then per case u64 span, u64 length, bytes (a file), u32 n_ranges,
//                              begin[n_ranges], end[n_ranges] (u64 each).
//   Two lines per case:
//     s <k> <status> <n_units> <n_members> <n_points> <out_bytes> <windows bytes> <bad_member> <err_off>
//       <stream_err_off> <message with _ for spaces> | the index's words
//     r <k> <status> <n_decoded> <bad_unit> <message> | out offsets | range statuses | <hex of the bytes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "flate_host.hpp"

static std::string message(const flate_host::Err &err) {
  std::string msg = err ? err->msg : "-";
  for (char &ch : msg)
    if (ch == ' ') ch = '_';
  return msg;
}

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
    uint32_t nr = 0;
    uint64_t span = 0, len = 0;
    if (fread(&span, 8, 1, f) != 1 || fread(&len, 8, 1, f) != 1) return 2;
    std::vector<uint8_t> data(len);
    if (len && fread(data.data(), 1, len, f) != len) return 2;
    if (fread(&nr, 4, 1, f) != 1) return 2;
    std::vector<uint64_t> begin(nr), end(nr);
    if (nr && (fread(begin.data(), 8, nr, f) != nr || fread(end.data(), 8, nr, f) != nr)) return 2;
    flate_host::GzFileSeekIndex sx;
    flate_host::Err err = flate_host::seek_index_gzfile(e, data, span, sx);
    printf("s %u %d %u %u %u %llu %llu %u %lld %lld %s |", k, sx.status, sx.n_units, sx.n_members, sx.n_points,
           (unsigned long long)sx.out_bytes, (unsigned long long)sx.windows.size(), sx.bad_member, (long long)sx.err_off,
           (long long)sx.stream_err_off, message(err).c_str());
    for (uint64_t x : sx.index) printf(" %llu", (unsigned long long)x);
    printf("\n");
    std::vector<flate_host::OneRange> ranges(nr);
    for (uint32_t r = 0; r < nr; ++r) ranges[r].begin = begin[r], ranges[r].end = end[r];
    std::vector<uint8_t> out;
    flate_host::OneRangesInfo info;
    err = flate_host::decompress_gzfile_ranges(e, data, sx, ranges, out, &info);
    printf("r %u %d %u %u %s |", k, info.status, info.n_decoded, info.bad_unit, message(err).c_str());
    for (uint64_t x : info.out_off) printf(" %llu", (unsigned long long)x);
    printf(" |");
    for (int32_t x : info.range_status) printf(" %d", x);
    printf(" | ");
    for (uint8_t b : out) printf("%02x", b);
    printf("\n");
  }
  fclose(f);
  return 0;
}
