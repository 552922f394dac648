// gzfile_reader_driver.cpp -- flate_host::GzFileReader over a file: a gzip file of several members through two small
// buffers.
//   gzfile_reader_driver IN OUT in_piece out_piece   reads the file IN piece by piece, writes what it inflates to into
//                                                    OUT, prints "end <error or EOF>", "close", "calls N", "members N",
//                                                    "resident BYTES", "bad_member N", "err_off N", "stream_err_off N"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flate_host.hpp"

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> file;
  uint8_t buf[4096];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + k);
  fclose(f);
  flate_host::Engine eng(0);
  flate_host::BytesReader src(file);
  flate_host::GzFileReader rd(src, eng, (size_t)atol(argv[3]), (size_t)atol(argv[4]));
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
  printf("calls %llu\nmembers %llu\nresident %zu\n", (unsigned long long)rd.calls(), (unsigned long long)rd.members(),
         rd.resident_bytes());
  printf("bad_member %u\nerr_off %lld\nstream_err_off %lld\n", rd.failure().bad_member, (long long)rd.failure().err_off,
         (long long)rd.failure().stream_err_off);
  return 0;
}
