// bgzf_parts_driver.cpp -- flate_host::BgzfReader and flate_host::BgzfWriter over files, through small buffers.
//   bgzf_parts_driver read IN OUT in_piece out_piece      reads the BGZF file IN piece by piece, writes what it inflates
//                                                         to into OUT, prints "end <error or EOF>", "close", "calls N",
//                                                         "members N", "marker 0|1", "resident BYTES", "bad_member N",
//                                                         "err_off N"
//   bgzf_parts_driver write IN OUT block part chunk       writes IN, `chunk` bytes per write(), as a BGZF file of `block`
//                                                         byte blocks into OUT, `part` bytes per call; prints "close",
//                                                         "calls N", "blocks N", "emitted N", "resident BYTES"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flate_host.hpp"

static bool slurp(const char *path, std::vector<uint8_t> &file) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + k);
  fclose(f);
  return true;
}

int main(int argc, char **argv) {
  if (argc < 6) return 2;
  std::vector<uint8_t> file;
  if (!slurp(argv[2], file)) return 2;
  FILE *o = fopen(argv[3], "wb");
  if (!o) return 2;
  flate_host::Engine eng(0);
  if (!strcmp(argv[1], "read") && argc == 6) {
    flate_host::BytesReader src(file);
    flate_host::BgzfReader rd(src, eng, (size_t)atol(argv[4]), (size_t)atol(argv[5]));
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
    printf("calls %llu\nmembers %llu\nmarker %d\nresident %zu\n", (unsigned long long)rd.calls(),
           (unsigned long long)rd.members(), rd.eof_marker() ? 1 : 0, rd.resident_bytes());
    printf("bad_member %u\nerr_off %lld\n", rd.failure().bad_member, (long long)rd.failure().err_off);
    return 0;
  }
  if (!strcmp(argv[1], "write") && argc == 7) {
    flate_host::Buffer sink;
    flate_host::BgzfWriter wr(sink, eng, (uint32_t)atol(argv[4]), 0, (size_t)atol(argv[5]));
    const size_t chunk = (size_t)atol(argv[6]);
    for (size_t at = 0; at < file.size(); at += chunk) {
      auto r = wr.write(file.data() + at, file.size() - at < chunk ? file.size() - at : chunk);
      if (r.second) {
        printf("write %s\n", r.second->msg.c_str());
        break;
      }
    }
    flate_host::Err e = wr.close();
    fwrite(sink.bytes.data(), 1, sink.bytes.size(), o);
    fclose(o);
    printf("close %s\n", e ? e->msg.c_str() : "none");
    printf("calls %llu\nblocks %llu\nemitted %llu\nresident %zu\n", (unsigned long long)wr.calls(),
           (unsigned long long)wr.blocks(), (unsigned long long)wr.emitted(), wr.resident_bytes());
    return 0;
  }
  return 2;
}
