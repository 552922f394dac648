// one_writer_driver.cpp -- flate_host::OneWriter over a file: one long stream written through bounded buffers, against
// the whole call over the same pieces.
//   one_writer_driver IN OUT WHOLE wrap piece part   writes IN through a OneWriter (wrap 0 raw, 1 zlib, 2 gzip; pieces of
//       `piece` bytes, parts of `part` bytes) with awkward write sizes into OUT, and what
//       flate_hip_deflate_fast_spliced_framed makes of IN cut every `piece` bytes into WHOLE; prints "close <error or
//       none>", "again <what a second close says>", "late <what a write behind close says>", "calls N", "pieces N",
//       "emitted N", "resident BYTES", "whole RC"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "flate_host.hpp"

int main(int argc, char **argv) {
  if (argc != 7) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> plain;
  uint8_t buf[4096];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) plain.insert(plain.end(), buf, buf + k);
  fclose(f);
  const uint32_t wrap = (uint32_t)atol(argv[4]);
  const uint64_t piece = (uint64_t)atoll(argv[5]);
  const flate_host::Wrap W = wrap == 2 ? flate_host::Wrap::Gzip : wrap == 1 ? flate_host::Wrap::Zlib : flate_host::Wrap::Raw;
  flate_host::Engine eng(0);
  flate_host::Buffer sink;
  flate_host::OneWriter wr(sink, eng, W, piece, 0, (size_t)atol(argv[6]));
  const size_t steps[] = {1, 7777, 65535, 3, 100000, 0, 65536, 12345};  // (no multiple of anything the writer holds)
  flate_host::Err err;
  size_t at = 0;
  for (size_t i = 0; at < plain.size() && !err; ++i) {
    const size_t n = std::min(steps[i % 8], plain.size() - at);
    auto r = wr.write(plain.data() + at, n);
    err = r.second;
    at += n;
  }
  if (!err) err = wr.close();
  printf("close %s\n", err ? err->msg.c_str() : "none");
  printf("again %s\n", wr.close() ? "error" : "none");
  auto late = wr.write(plain.data(), plain.empty() ? 0 : 1);
  printf("late %s\n", late.second ? late.second->msg.c_str() : "none");
  printf("calls %llu\npieces %llu\nemitted %llu\nresident %zu\n", (unsigned long long)wr.calls(),
         (unsigned long long)wr.pieces(), (unsigned long long)wr.emitted(), wr.resident_bytes());
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(sink.bytes.data(), 1, sink.bytes.size(), o);
  fclose(o);

  const uint64_t P = piece ? piece : 65535;
  std::vector<uint64_t> in_off;
  for (uint64_t x = 0; x < plain.size(); x += P) in_off.push_back(x);
  in_off.push_back(plain.size());
  const uint32_t n = (uint32_t)in_off.size() - 1;
  std::vector<uint8_t> whole(flate_hip_one_writer_bound(plain.size(), (size_t)piece) + 64);
  uint64_t len = 0;
  const int rc = flate_hip_deflate_fast_spliced_framed(eng.ctx(), plain.data(), in_off.data(), n, wrap, whole.data(),
                                                      whole.size(), &len, nullptr, 0);
  printf("whole %d\n", rc);
  o = fopen(argv[3], "wb");
  if (!o) return 2;
  fwrite(whole.data(), 1, rc == 0 ? (size_t)len : 0, o);
  fclose(o);
  return 0;
}
