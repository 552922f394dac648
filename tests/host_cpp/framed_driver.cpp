// zlib and gzip members through the C++ host mirror (flate_host.hpp): compress_batch(..., Wrap) with and without a
// DictTable and compress_spliced(..., Wrap), each one call of the framed C ABI.  argv[1]: a case file -- u32 compat_go
// (0 / 1), u32 count, then per dictionary u32 length + bytes; u32 count, then per stream u32 dictionary
// (0xffffffff = none) + u32 length + bytes.
// Prints "z <i> <hex>" / "g <i> <hex>" (members without dictionaries), "d <i> <hex>" (zlib members with the
// dictionaries), "sz <hex>" / "sg <hex>" (the batch as one member) and "r <i> <hex>" (Wrap::Raw).
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
static void hex(const char *tag, int i, const std::vector<uint8_t> &b) {
  if (i >= 0)
    printf("%s %d ", tag, i);
  else
    printf("%s ", tag);
  for (uint8_t x : b) printf("%02x", x);
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t go, nd, ns;
  std::vector<std::vector<uint8_t>> dicts, streams;
  std::vector<uint32_t> dict_of;
  if (!rd32(f, go) || go > 1 || !rd32(f, nd)) return 2;
  const uint32_t flags = go ? FLATE_HIP_COMPAT_GO : 0u;
  dicts.resize(nd);
  for (auto &d : dicts)
    if (!rdv(f, d)) return 2;
  if (!rd32(f, ns)) return 2;
  streams.resize(ns);
  for (uint32_t i = 0; i < ns; ++i) {
    uint32_t j;
    if (!rd32(f, j) || !rdv(f, streams[i])) return 2;
    dict_of.push_back(j);
  }
  fclose(f);
  Engine eng(0);
  const DictTable table(dicts);
  std::vector<std::vector<uint8_t>> out;
  const struct {
    const char *tag;
    Wrap wrap;
  } plain[3] = {{"r", Wrap::Raw}, {"z", Wrap::Zlib}, {"g", Wrap::Gzip}};
  for (const auto &k : plain) {
    if (Err e = compress_batch(eng, streams, out, k.wrap, flags)) {
      printf("error %s %s\n", k.tag, e->msg.c_str());
      return 1;
    }
    for (uint32_t i = 0; i < ns; ++i) hex(k.tag, (int)i, out[i]);
  }
  if (Err e = compress_batch(eng, streams, &table, dict_of, out, Wrap::Zlib, flags)) {
    printf("error d %s\n", e->msg.c_str());
    return 1;
  }
  for (uint32_t i = 0; i < ns; ++i) hex("d", (int)i, out[i]);
  // gzip has no preset dictionaries: the call must refuse
  if (!compress_batch(eng, streams, &table, dict_of, out, Wrap::Gzip, flags)) {
    printf("error gzip with dictionaries was accepted\n");
    return 1;
  }
  std::vector<uint8_t> one;
  std::vector<uint64_t> bit_off;
  if (Err e = compress_spliced(eng, streams, one, Wrap::Zlib, &bit_off, flags)) {
    printf("error sz %s\n", e->msg.c_str());
    return 1;
  }
  hex("sz", -1, one);
  if (Err e = compress_spliced(eng, streams, one, Wrap::Gzip, nullptr, flags)) {
    printf("error sg %s\n", e->msg.c_str());
    return 1;
  }
  hex("sg", -1, one);
  printf("bits %zu\n", bit_off.size());
  return 0;
}
