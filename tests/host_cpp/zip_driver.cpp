// zip_driver.cpp -- drives the C++ host mirror's ZIP calls (flate_host::compress_zip / decompress_zip) for
// tests/test_host_cpp_zip.py.
//   zip_driver CASES     CASES = u32 count, then per case u32 kind.  kind 0 (entries to write and read back): u32 flags,
//                        u32 n, per entry u32 name length + name, u64 length + bytes.  kind 1 (an archive to read): u64
//                        length + bytes.  One line per case:
//     w <k> <hex of the archive> <entry offsets, comma separated> <round trip ok 0/1>
//     r <k> <status> <n_entries> <err_off> <message with _ for spaces> <per entry, comma separated: hex name:status:hex bytes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "flate_host.hpp"

static void hex(const uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
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
    uint32_t kind = 0;
    if (fread(&kind, 4, 1, f) != 1) return 2;
    if (kind == 0) {
      uint32_t flags = 0, n = 0;
      if (fread(&flags, 4, 1, f) != 1 || fread(&n, 4, 1, f) != 1) return 2;
      std::vector<std::vector<uint8_t>> entries(n), back;
      std::vector<std::string> names(n);
      for (uint32_t i = 0; i < n; ++i) {
        uint32_t nl = 0;
        uint64_t len = 0;
        if (fread(&nl, 4, 1, f) != 1) return 2;
        names[i].resize(nl);
        if (nl && fread(&names[i][0], 1, nl, f) != nl) return 2;
        if (fread(&len, 8, 1, f) != 1) return 2;
        entries[i].resize(len);
        if (len && fread(entries[i].data(), 1, len, f) != len) return 2;
      }
      std::vector<uint8_t> file;
      std::vector<uint64_t> off;
      flate_host::Err err = flate_host::compress_zip(e, entries, names, file, &off, flags);
      if (err) {
        printf("w %u error %s\n", k, err->msg.c_str());
        continue;
      }
      flate_host::ZipInfo info;
      err = flate_host::decompress_zip(e, file, back, &info);
      printf("w %u ", k);
      hex(file.data(), file.size());
      printf(" ");
      for (size_t i = 0; i < off.size(); ++i) printf("%s%llu", i ? "," : "", (unsigned long long)off[i]);
      printf(" %d\n", (!err && back == entries && info.names == names) ? 1 : 0);
    } else {
      uint64_t len = 0;
      if (fread(&len, 8, 1, f) != 1) return 2;
      std::vector<uint8_t> data(len);
      if (len && fread(data.data(), 1, len, f) != len) return 2;
      std::vector<std::vector<uint8_t>> out;
      flate_host::ZipInfo info;
      flate_host::Err err = flate_host::decompress_zip(e, data, out, &info);
      std::string msg = err ? err->msg : "-";
      for (char &ch : msg)
        if (ch == ' ') ch = '_';
      printf("r %u %d %u %lld %s ", k, info.status, info.n_entries, (long long)info.err_off, msg.c_str());
      for (size_t i = 0; i < out.size(); ++i) {
        printf("%s", i ? "," : "");
        hex((const uint8_t *)info.names[i].data(), info.names[i].size());
        printf(":%d:", info.entry_status[i]);
        hex(out[i].data(), out[i].size());
      }
      printf("\n");
    }
  }
  fclose(f);
  return 0;
}
