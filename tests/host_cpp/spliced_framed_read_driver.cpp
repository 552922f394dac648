// ONE zlib stream / gzip member around a spliced stream READ through the C++ host mirror (flate_host.hpp):
// decompress_spliced(eng, member, bit_off, sizes, Wrap, out), one call of flate_hip_inflate_spliced_framed.
// argv[1]: a case file -- u32 count, then per case u32 wrap (1 = zlib, 2 = gzip), u32 n, (n + 1) u64 bit offsets,
// n u64 capacities, u32 length + the member's bytes.
// Prints per case "c <i> <error text, blanks as _, or -> <hex of the bytes delivered>"; for a case that verified, the
// pieces then go through compress_spliced(..., Wrap) and back: "r <i> ok".
#include <cstdio>
#include <vector>

#include "flate_host.hpp"

using namespace flate_host;

static bool rd32(FILE *f, uint32_t &v) { return fread(&v, 4, 1, f) == 1; }
static bool rd64s(FILE *f, std::vector<uint64_t> &v, uint32_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), 8, n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t cases;
  if (!rd32(f, cases)) return 2;
  Engine eng(0);
  for (uint32_t c = 0; c < cases; ++c) {
    uint32_t w, n, len;
    std::vector<uint64_t> bit_off, sizes;
    if (!rd32(f, w) || (w != 1 && w != 2) || !rd32(f, n) || !rd64s(f, bit_off, n + 1) || !rd64s(f, sizes, n) || !rd32(f, len))
      return 2;
    std::vector<uint8_t> member(len), out;
    if (len && fread(member.data(), 1, len, f) != len) return 2;
    const Wrap wrap = w == 1 ? Wrap::Zlib : Wrap::Gzip;
    Err e = decompress_spliced(eng, member, bit_off, sizes, wrap, out);
    std::string msg = e ? e->msg : "-";
    for (char &ch : msg)
      if (ch == ' ') ch = '_';
    printf("c %u %s ", c, msg.c_str());
    for (uint8_t x : out) printf("%02x", x);
    printf("\n");
    if (e) continue;
    // what was read, written again as one member and read back from the writer's own index
    std::vector<std::vector<uint8_t>> pieces;
    size_t at = 0;
    for (uint32_t i = 0; i < n && at <= out.size(); ++i) {
      const size_t k = std::min<size_t>(sizes[i], out.size() - at);
      pieces.emplace_back(out.begin() + at, out.begin() + at + k);
      at += k;
    }
    std::vector<uint8_t> again, back;
    std::vector<uint64_t> index, caps;
    for (const auto &p : pieces) caps.push_back(p.size());
    if ((e = compress_spliced(eng, pieces, again, wrap, &index)) || (e = decompress_spliced(eng, again, index, caps, wrap, back))) {
      printf("error %s\n", e->msg.c_str());
      return 1;
    }
    printf("r %u %s\n", c, back == out ? "ok" : "differs");
  }
  fclose(f);
  return 0;
}
