// gzfile_reader_serial_driver.cpp -- flate_host::GzFileReader::set_serial_max over a file: a gzip file of many short
// members through two small buffers, the members that lie whole inside a piece decoded whole.
//   gzfile_reader_serial_driver IN OUT in_piece out_piece S
//     reads the file IN piece by piece, writes what it inflates to into OUT, prints "end <error or EOF>", "close",
//     "calls N", "members N", "serial_members N", "late_set 0|1" (set_serial_max behind the first read: refused),
//     "too_large_set 0|1" (2^28: refused), then reads the file AGAIN behind reset -- which keeps S -- and prints
//     "again_members N", "again_serial_members N", "again_same 0|1" (the same bytes)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flate_host.hpp"

static flate_host::Err drain(flate_host::GzFileReader &rd, std::vector<uint8_t> &out) {
  std::vector<uint8_t> piece(5000);  // (no multiple of anything the reader holds)
  for (;;) {
    auto r = rd.read(piece.data(), piece.size());
    out.insert(out.end(), piece.begin(), piece.begin() + r.first);
    if (r.second) return r.second;
  }
}

int main(int argc, char **argv) {
  if (argc != 6) return 2;
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
  const bool too_large = rd.set_serial_max(1ull << 28);
  if (!rd.set_serial_max((uint64_t)atoll(argv[5]))) return 3;
  std::vector<uint8_t> plain;
  flate_host::Err err = drain(rd, plain);
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(plain.data(), 1, plain.size(), o);
  fclose(o);
  printf("end %s\n", *err == flate_host::ioeof() ? "EOF" : err->msg.c_str());
  printf("close %s\n", rd.close() ? "error" : "none");
  printf("calls %llu\nmembers %llu\nserial_members %llu\n", (unsigned long long)rd.calls(), (unsigned long long)rd.members(),
         (unsigned long long)rd.serial_members());
  printf("late_set %d\ntoo_large_set %d\n", rd.set_serial_max(0) ? 1 : 0, too_large ? 1 : 0);
  flate_host::BytesReader src2(file);
  rd.reset(src2);
  std::vector<uint8_t> again;
  (void)drain(rd, again);
  printf("again_members %llu\nagain_serial_members %llu\nagain_same %d\n", (unsigned long long)rd.members(),
         (unsigned long long)rd.serial_members(), again == plain ? 1 : 0);
  return 0;
}
