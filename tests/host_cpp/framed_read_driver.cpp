// zlib and gzip members READ through the C++ host mirror (flate_host.hpp): decompress_batch(..., Wrap) and its
// dictionary overload, each one call of flate_hip_inflate_batch_framed.  argv[1]: a case file -- u32 wrap (1 = zlib,
// 2 = gzip), u32 count, then per dictionary u32 length + bytes; u32 count, then per member u32 capacity (gzip: 0 = its
// ISIZE) + u32 length + bytes.
// Prints per member "m <i> <status> <dictionary or -1> <error text, blanks as _, or -> <hex of the bytes delivered>".
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
  uint32_t w, nd, ns;
  std::vector<std::vector<uint8_t>> dicts, members;
  std::vector<uint64_t> sizes;
  if (!rd32(f, w) || (w != 1 && w != 2) || !rd32(f, nd)) return 2;
  dicts.resize(nd);
  for (auto &d : dicts)
    if (!rdv(f, d)) return 2;
  if (!rd32(f, ns)) return 2;
  members.resize(ns);
  for (uint32_t i = 0; i < ns; ++i) {
    uint32_t cap;
    if (!rd32(f, cap) || !rdv(f, members[i])) return 2;
    sizes.push_back(cap);
  }
  fclose(f);
  const Wrap wrap = w == 1 ? Wrap::Zlib : Wrap::Gzip;
  Engine eng(0);
  std::vector<Inflated> out;
  std::vector<uint32_t> used(ns, FLATE_HIP_NO_DICT);
  Err e = nd ? decompress_batch(eng, members, sizes, dicts, out, wrap, &used) : decompress_batch(eng, members, sizes, out, wrap);
  if (e) {
    printf("error %s\n", e->msg.c_str());
    return 1;
  }
  for (uint32_t i = 0; i < ns; ++i) {
    std::string msg = out[i].err ? out[i].err->msg : "-";
    for (char &ch : msg)
      if (ch == ' ') ch = '_';
    printf("m %u %d %d %s ", i, out[i].status, used[i] == FLATE_HIP_NO_DICT ? -1 : (int)used[i], msg.c_str());
    for (uint8_t x : out[i].bytes) printf("%02x", x);
    printf("\n");
  }
  if (wrap == Wrap::Gzip && nd == 0) {
    // gzip has no preset dictionaries: the dictionary overload must refuse
    const std::vector<std::vector<uint8_t>> some = {{1, 2, 3}};
    if (!decompress_batch(eng, members, sizes, some, out, wrap)) {
      printf("error gzip with dictionaries was accepted\n");
      return 1;
    }
    printf("refused\n");
  }
  return 0;
}
