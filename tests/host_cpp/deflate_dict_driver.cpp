// Batch deflate with preset dictionaries through the C++ host mirror (flate_host.hpp): a BatchWriter with a
// DictTable, every stream read back by Reader::new_dict with the same dictionary.  argv[1]: a case file -- u32
// compat_go (0 / 1: the only flag a host-buffer caller may choose), u32 count, then per dictionary u32 length +
// bytes; u32 count, then per stream u32 dictionary (0xffffffff = none) + u32 length + bytes.
// Prints, per stream: "s <read back ok 0/1> <hex of the compressed bytes>".
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
  uint32_t go, nd, ns;
  std::vector<std::vector<uint8_t>> dicts, streams;
  std::vector<uint32_t> dict_of;
  if (!rd32(f, go) || go > 1 || !rd32(f, nd)) return 2;
  const uint32_t flags = go ? FLATE_HIP_COMPAT_GO : 0u;  // (the buffers are host memory: never FLATE_HIP_DEVICE_PTRS)
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
  std::vector<Buffer> sinks(ns);
  BatchWriter bw(eng, table, flags);
  for (uint32_t i = 0; i < ns; ++i) {
    Writer &w = bw.add(sinks[i], dict_of[i]);
    // two writes per stream: the Writer stages them as one
    const size_t half = streams[i].size() / 2;
    if (w.write(streams[i].data(), half).second || w.write(streams[i].data() + half, streams[i].size() - half).second) {
      printf("error write\n");
      return 1;
    }
  }
  if (Err e = bw.close_all()) {
    printf("error %s\n", e->msg.c_str());
    return 1;
  }
  for (uint32_t i = 0; i < ns; ++i) {
    BytesReader src(sinks[i].bytes);
    auto rd = Reader::new_dict(src, eng, dict_of[i] == FLATE_HIP_NO_DICT ? std::vector<uint8_t>() : dicts[dict_of[i]]);
    std::vector<uint8_t> back, piece(1 << 16);
    bool ok = true;
    for (;;) {
      auto r = rd->read(piece.data(), piece.size());
      back.insert(back.end(), piece.begin(), piece.begin() + r.first);
      if (r.second) {
        ok = *r.second == ioeof();
        break;
      }
    }
    printf("s %d ", ok && back == streams[i] ? 1 : 0);
    for (uint8_t b : sinks[i].bytes) printf("%02x", b);
    printf("\n");
  }
  return 0;
}
