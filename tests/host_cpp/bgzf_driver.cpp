// bgzf_driver.cpp -- drives the C++ host mirror's BGZF calls (flate_host::compress_bgzf / decompress_bgzf) for
// tests/test_host_cpp_bgzf.py.
//   bgzf_driver CASES    CASES = u32 count, then per case u32 kind (0 = data to write and read back, 1 = a file to
//                        read), u32 block_bytes, u32 flags, u64 length, bytes.  One line per case:
//     w <k> <hex of the file> <member offsets, comma separated> <round trip ok 0/1>
//     r <k> <status> <n_members> <bad_member> <err_off> <eof 0/1> <message with _ for spaces> <hex of the bytes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "flate_host.hpp"

static void hex(const std::vector<uint8_t> &v) {
  for (uint8_t b : v) printf("%02x", b);
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
    uint32_t kind = 0, bb = 0, flags = 0;
    uint64_t len = 0;
    if (fread(&kind, 4, 1, f) != 1 || fread(&bb, 4, 1, f) != 1 || fread(&flags, 4, 1, f) != 1 || fread(&len, 8, 1, f) != 1)
      return 2;
    std::vector<uint8_t> data(len);
    if (len && fread(data.data(), 1, len, f) != len) return 2;
    if (kind == 0) {
      std::vector<uint8_t> file, back;
      std::vector<uint64_t> off;
      flate_host::Err err = flate_host::compress_bgzf(e, data, file, bb, &off, flags);
      if (err) {
        printf("w %u error %s\n", k, err->msg.c_str());
        continue;
      }
      flate_host::BgzfInfo info;
      err = flate_host::decompress_bgzf(e, file, back, &info);
      printf("w %u ", k);
      hex(file);
      printf(" ");
      for (size_t i = 0; i < off.size(); ++i) printf("%s%llu", i ? "," : "", (unsigned long long)off[i]);
      printf(" %d\n", (!err && back == data && info.eof_marker && info.n_members == off.size()) ? 1 : 0);
    } else {
      std::vector<uint8_t> out;
      flate_host::BgzfInfo info;
      flate_host::Err err = flate_host::decompress_bgzf(e, data, out, &info);
      std::string msg = err ? err->msg : "-";
      for (char &ch : msg)
        if (ch == ' ') ch = '_';
      printf("r %u %d %u %u %lld %d %s ", k, info.status, info.n_members, info.bad_member, (long long)info.err_off,
             info.eof_marker ? 1 : 0, msg.c_str());
      hex(out);
      printf("\n");
    }
  }
  fclose(f);
  return 0;
}
