// seek_pack_driver.cpp -- drives the C++ host mirror's flate_host::pack_seek_windows, unpack_seek_windows and
// decompress_one_ranges_packed for tests/test_gpu_host_seek_pack.py: one file round-trips.
//   seek_pack_driver CASES   CASES = u32 count, then per case u32 wrap (0 raw, 1 zlib, 2 gzip), u64 span, u32 sparse,
//                            u64 length, bytes (a stream), u32 n_ranges, begin[n_ranges], end[n_ranges] (u64 each).
//   Three lines per case:
//     p <k> <status> <kept_bytes> <packed bytes> <message with _ for spaces> | the pack index's words | <hex of packed>
//     u <k> <message> <windows bytes> <the unpacked windows equal the build's: 0 / 1> <FNV-1a of the unpacked windows>
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
    uint32_t wrap = 0, nr = 0, sparse = 0;
    uint64_t span = 0, len = 0;
    if (fread(&wrap, 4, 1, f) != 1 || fread(&span, 8, 1, f) != 1 || fread(&sparse, 4, 1, f) != 1 || fread(&len, 8, 1, f) != 1)
      return 2;
    std::vector<uint8_t> data(len);
    if (len && fread(data.data(), 1, len, f) != len) return 2;
    if (fread(&nr, 4, 1, f) != 1) return 2;
    std::vector<uint64_t> begin(nr), end(nr);
    if (nr && (fread(begin.data(), 8, nr, f) != nr || fread(end.data(), 8, nr, f) != nr)) return 2;
    const flate_host::Wrap w = wrap == 1 ? flate_host::Wrap::Zlib : wrap == 2 ? flate_host::Wrap::Gzip : flate_host::Wrap::Raw;
    flate_host::OneSeekIndex sx;
    if (flate_host::seek_index_one(e, data, w, span, sx)) return 4;
    flate_host::SeekPack pk;
    flate_host::Err err = flate_host::pack_seek_windows(e, data, w, sx, sparse != 0, pk);
    printf("p %u %d %llu %llu %s |", k, pk.status, (unsigned long long)pk.kept_bytes, (unsigned long long)pk.packed.size(),
           message(err).c_str());
    for (uint64_t x : pk.pack_index) printf(" %llu", (unsigned long long)x);
    printf(" | ");
    for (uint8_t b : pk.packed) printf("%02x", b);
    printf("\n");
    std::vector<uint8_t> windows;
    err = flate_host::unpack_seek_windows(e, pk, windows);
    uint64_t h = 1469598103934665603ull;
    for (uint8_t b : windows) h = (h ^ b) * 1099511628211ull;
    printf("u %u %s %llu %d %llu\n", k, message(err).c_str(), (unsigned long long)windows.size(), windows == sx.windows ? 1 : 0,
           (unsigned long long)h);
    std::vector<flate_host::OneRange> ranges(nr);
    for (uint32_t r = 0; r < nr; ++r) ranges[r].begin = begin[r], ranges[r].end = end[r];
    std::vector<uint8_t> out;
    flate_host::OneRangesInfo info;
    sx.windows.clear();  // (the packed read takes none)
    err = flate_host::decompress_one_ranges_packed(e, data, w, sx, pk, ranges, out, &info);
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
