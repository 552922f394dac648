// one_reader_driver.cpp -- flate_host::OneReader over a file: one long gzip member through two small buffers.
//   one_reader_driver IN OUT in_piece out_piece   reads the member IN piece by piece, writes what it inflates to into
//                                                 OUT, prints "end <error or EOF>", "calls N", "resident BYTES", "unread N"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flate_host.hpp"

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> member;
  uint8_t buf[4096];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) member.insert(member.end(), buf, buf + k);
  fclose(f);
  flate_host::Engine eng(0);
  flate_host::BytesReader src(member);
  flate_host::OneReader rd(src, eng, flate_host::Wrap::Gzip, (size_t)atol(argv[3]), (size_t)atol(argv[4]));
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  std::vector<uint8_t> piece(5000);  // (no multiple of anything the reader holds)
  flate_host::Err err;
  for (;;) {
    auto r = rd.read(piece.data(), piece.size());
    fwrite(piece.data(), 1, (size_t)r.first, o);
    if (r.second) {
      err = r.second;
      break;
    }
  }
  fclose(o);
  printf("end %s\n", *err == flate_host::ioeof() ? "EOF" : err->msg.c_str());
  printf("close %s\n", rd.close() ? "error" : "none");
  printf("calls %llu\nresident %zu\nunread %zu\n", (unsigned long long)rd.calls(), rd.resident_bytes(), rd.unread().size());
  return 0;
}
