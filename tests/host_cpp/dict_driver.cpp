// Batch inflate with preset dictionaries through the C++ host mirror (flate_host.hpp: decompress_batch /
// inflate_sizes with dictionaries).  argv[1]: a case file -- u32 count, then per dictionary u32 length + bytes;
// u32 count, then per stream u32 dictionary (0xffffffff = none) + u32 capacity + u32 length + bytes.
// Prints, per stream: "s <status> <err_off> <size-only size> <hex of the bytes>".
#include <cstdio>
#include <vector>

#include "flate_host.hpp"

using namespace flate_host;

static bool rd32(FILE *f, uint32_t &v) { return fread(&v, 4, 1, f) == 1; }
static bool rdv(FILE *f, std::vector<uint8_t> &v) {
  uint32_t n;
  if (!rd32(f, n)) return false;
  v.resize(n);
  return n == 0 || fread(v.data(), 1, n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t nd, ns;
  std::vector<std::vector<uint8_t>> dicts, streams;
  std::vector<uint32_t> dict_of;
  std::vector<uint64_t> caps;
  if (!rd32(f, nd)) return 2;
  dicts.resize(nd);
  for (auto &d : dicts)
    if (!rdv(f, d)) return 2;
  if (!rd32(f, ns)) return 2;
  streams.resize(ns);
  for (uint32_t i = 0; i < ns; ++i) {
    uint32_t j, cap;
    if (!rd32(f, j) || !rd32(f, cap) || !rdv(f, streams[i])) return 2;
    dict_of.push_back(j);
    caps.push_back(cap);
  }
  fclose(f);
  Engine eng(0);
  std::vector<Inflated> out;
  if (Err e = decompress_batch(eng, streams, caps, dicts, dict_of, out)) {
    printf("error %s\n", e->msg.c_str());
    return 1;
  }
  std::vector<uint64_t> sizes;
  if (Err e = inflate_sizes(eng, streams, dicts, dict_of, sizes)) {
    printf("error %s\n", e->msg.c_str());
    return 1;
  }
  for (uint32_t i = 0; i < ns; ++i) {
    long long eoff = -1;
    if (out[i].status == FLATE_HIP_E_CORRUPT) eoff = std::stoll(out[i].err->msg.substr(out[i].err->msg.rfind(' ') + 1));
    printf("s %d %lld %llu ", out[i].status, eoff, (unsigned long long)sizes[i]);
    for (uint8_t b : out[i].bytes) printf("%02x", b);
    printf("\n");
  }
  return 0;
}
