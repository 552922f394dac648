// bgzf_ranges_driver.cpp -- drives the C++ host mirror's BGZF random access (flate_host::decompress_bgzf_ranges) for
// tests/test_host_cpp_bgzf_ranges.py.
//   bgzf_ranges_driver CASES   CASES = u32 count, then per case u32 virtual (0 / 1), u64 length, the file's bytes, u32
//                              n_ranges, begin[n_ranges], end[n_ranges] (u64 each).  One line per case:
//     <k> <status> <n_members> <n_decoded> <bad_member> <err_off> <out_off, comma separated> <range_status, comma
//     separated, or -> <message with _ for spaces> <hex of the bytes>
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
    uint32_t virt = 0, nr = 0;
    uint64_t len = 0;
    if (fread(&virt, 4, 1, f) != 1 || fread(&len, 8, 1, f) != 1) return 2;
    std::vector<uint8_t> file(len);
    if (len && fread(file.data(), 1, len, f) != len) return 2;
    if (fread(&nr, 4, 1, f) != 1) return 2;
    std::vector<uint64_t> begin(nr), end(nr);
    if (nr && (fread(begin.data(), 8, nr, f) != nr || fread(end.data(), 8, nr, f) != nr)) return 2;
    std::vector<flate_host::BgzfRange> ranges(nr);
    for (uint32_t r = 0; r < nr; ++r) ranges[r].begin = begin[r], ranges[r].end = end[r];
    std::vector<uint8_t> out;
    flate_host::BgzfRangesInfo info;
    flate_host::Err err = flate_host::decompress_bgzf_ranges(e, file, ranges, out, &info, virt != 0);
    std::string msg = err ? err->msg : "-";
    for (char &ch : msg)
      if (ch == ' ') ch = '_';
    printf("%u %d %u %u %u %lld ", k, info.status, info.n_members, info.n_decoded, info.bad_member, (long long)info.err_off);
    for (size_t i = 0; i < info.out_off.size(); ++i) printf("%s%llu", i ? "," : "", (unsigned long long)info.out_off[i]);
    printf(" ");
    for (size_t i = 0; i < info.range_status.size(); ++i) printf("%s%d", i ? "," : "", info.range_status[i]);
    if (info.range_status.empty()) printf("-");
    printf(" %s ", msg.c_str());
    for (uint8_t b : out) printf("%02x", b);
    printf("\n");
  }
  fclose(f);
  return 0;
}
