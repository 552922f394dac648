// grouped_driver.cpp -- the C++ host mirror of the grouped splice (flate_host.hpp: compress_grouped), driven by
// tests/test_host_cpp_grouped.py.
//   grouped_driver FILE WRAP(0 raw / 1 zlib / 2 gzip) FLAGS
// FILE: n_groups : u32; per group n_pieces : u32, per piece len : u64 and its bytes.
// Output, per group: "m <g> <member hex>|<index ...>|<what decompress_spliced gives back, hex>".
#include <cstdio>
#include <cstring>
#include <vector>

#include "flate_host.hpp"

using namespace flate_host;

static void hex(const std::vector<uint8_t> &v) {
  for (uint8_t b : v) printf("%02x", b);
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  auto get = [&](void *p, size_t n) {
    if (n && fread(p, 1, n, f) != n) exit(3);
  };
  uint32_t n_groups = 0;
  get(&n_groups, 4);
  std::vector<std::vector<std::vector<uint8_t>>> groups(n_groups);
  for (auto &grp : groups) {
    uint32_t k = 0;
    get(&k, 4);
    grp.resize(k);
    for (auto &p : grp) {
      uint64_t len = 0;
      get(&len, 8);
      p.resize(len);
      get(p.data(), len);
    }
  }
  fclose(f);
  const Wrap wrap = argv[2][0] == '0' ? Wrap::Raw : argv[2][0] == '1' ? Wrap::Zlib : Wrap::Gzip;
  const uint32_t flags = (uint32_t)atoi(argv[3]);
  Engine e(0);
  if (!e.ok()) {
    fprintf(stderr, "no engine: %d\n", e.status());
    return 1;
  }
  std::vector<std::vector<uint8_t>> members;
  std::vector<std::vector<uint64_t>> index;
  if (auto err = compress_grouped(e, groups, members, wrap, &index, flags)) {
    fprintf(stderr, "compress_grouped failed\n");
    return 1;
  }
  for (uint32_t g = 0; g < n_groups; ++g) {
    printf("m %u ", g);
    hex(members[g]);
    printf("|");
    for (size_t i = 0; i < index[g].size(); ++i) printf(i ? " %llu" : "%llu", (unsigned long long)index[g][i]);
    printf("|");
    std::vector<uint64_t> sizes;
    for (const auto &p : groups[g]) sizes.push_back(p.size());
    std::vector<uint8_t> back;
    if (auto err = decompress_spliced(e, members[g], index[g], sizes, wrap, back)) {
      fprintf(stderr, "decompress_spliced failed for member %u\n", g);
      return 1;
    }
    hex(back);
    printf("\n");
  }
  return 0;
}
