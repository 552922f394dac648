// bgzf_parts_rule_model.cpp -- bgzf_parts_rule.h (with bgzf_rule.h and api_checks.h) as a stand-alone program for
// tests/test_bgzf_parts_rule_model.py, which compares every line with tests/bgzf_parts_ref.py.  What the device does in
// parallel -- the walk over a part, the ISIZE sums, the clip -- is done serially here with the same rule functions
// (bgzf_member_total, bgzf_part_stop, bgzf_part_delivers); the host's part is the library's own (bgzf_parts_call,
// bgzf_parts_fail).
//   run FILE: one command per line
//     S avail final                      -> the part stop
//     B in_len bb final                  -> blocks in_used
//     F hex                              a fresh reader over this file
//     V off status                       the member at this FILE offset does not decode: its status
//     R len final out_cap index_cap      one read of file[consumed, consumed + len) (out_cap / index_cap: - = none)
//                                        -> rc in_used out_len n_members bad_member err_off eof_marker index...
//   checks: the argument checks, one "name rc" per line
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "api_checks.h"
#include "bgzf_parts_rule.h"
#include "bgzf_rule.h"

using namespace flate;

namespace {

std::vector<uint8_t> unhex(const std::string &s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
  return v;
}

uint64_t num(const std::string &s, uint64_t none) { return s == "-" ? none : strtoull(s.c_str(), nullptr, 10); }

struct Reader {
  std::vector<uint8_t> file;
  std::map<uint64_t, int> verdict;
  BgzfPartsState s = bgzf_parts_fresh();

  void read(uint64_t len, bool fin, uint64_t out_cap, bool with_index, uint64_t index_cap) {
    uint64_t in_used = 0, out_len = 0;
    uint32_t n_members = 0;
    std::vector<uint64_t> im{s.consumed}, io{s.produced};
    auto print = [&](int rc) {
      const bool bad = s.status < 0;
      printf("%d %" PRIu64 " %" PRIu64 " %u %u %" PRId64 " %u", rc, in_used, out_len, n_members,
             bad ? s.bad_member : 0xffffffffu, bad ? s.err_off : (int64_t)-1, s.eof_marker);
      if (with_index) {
        for (size_t i = 0; i < im.size(); ++i) printf(" %" PRIu64 ":%" PRIu64, im[i], io[i]);
      }
      printf("\n");
    };
    // a copy of exactly the part, so that the sanitizer sees a read behind its end
    std::vector<uint8_t> part(file.begin() + s.consumed, file.begin() + s.consumed + len);
    uint8_t out_byte = 0;
    if (bgzf_reader_read_args(this, part.data(), len, &out_byte, out_cap, &in_used, &out_len, index_cap,
                              with_index ? im.data() : nullptr, with_index ? io.data() : nullptr)) {
      printf("-1 0 0 0 %u -1 0\n", 0xffffffffu);
      return;
    }
    if (s.status) return print(s.status);
    if (len == 0) {
      if (fin) s.status = kBgzfPartsEnd;
      return print(s.status);
    }
    // the device's part: the walk, the sums, the stop, the clip
    std::vector<uint64_t> moff, ooff{0};
    uint64_t p = 0;
    while (p < len) {
      const uint32_t t = bgzf_member_total(part.data() + p, len - p);
      if (!t) break;
      moff.push_back(p);
      const uint8_t *e = part.data() + p + t - 4;
      ooff.push_back(ooff.back() + (e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16) | ((uint32_t)e[3] << 24)));
      p += t;
    }
    moff.push_back(p);
    BgzfPartFound f{};
    f.n = (uint32_t)moff.size() - 1u;
    f.p = p;
    f.stop = bgzf_part_stop(len - p, fin);
    const uint32_t k_max = bgzf_part_k_max(with_index, index_cap);
    for (uint32_t i = 0; i < f.n; ++i)
      if (bgzf_part_delivers(i, ooff[i + 1], out_cap, k_max)) f.k = i + 1u;
    f.in_end = moff[f.k];
    f.out_end = ooff[f.k];
    f.isize0 = f.n ? ooff[1] : 0;
    f.eof_last = f.k ? bgzf_is_eof_marker(part.data() + moff[f.k - 1], (uint32_t)(moff[f.k] - moff[f.k - 1])) : 0;
    // the host's part
    BgzfPartCall c = bgzf_parts_call(s, f, len, fin);
    if (c.status == kBgzfPartsOutTooSmall) {
      out_len = c.out_len;
      return print(c.status);
    }
    uint32_t delivered = c.decode;
    for (uint32_t j = 0; j < c.decode; ++j) {
      auto it = verdict.find(s.consumed + moff[j]);
      if (it == verdict.end()) continue;
      const bool eof_before = j && bgzf_is_eof_marker(part.data() + moff[j - 1], (uint32_t)(moff[j] - moff[j - 1]));
      bgzf_parts_fail(s, c, j, it->second, moff[j], ooff[j], eof_before);
      delivered = j;
      break;
    }
    im.clear(), io.clear();
    for (uint32_t i = 0; i <= delivered; ++i) im.push_back(s.consumed + moff[i]), io.push_back(s.produced + ooff[i]);
    s = c.next;
    in_used = c.in_used, out_len = c.out_len, n_members = delivered;
    print(c.status);
  }
};

int run(const char *path) {
  std::ifstream in(path);
  std::string line;
  Reader r;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::vector<std::string> t;
    for (std::string w; ss >> w;) t.push_back(w);
    if (t.empty()) continue;
    if (t[0] == "S" && t.size() == 3) {
      printf("%u\n", bgzf_part_stop(num(t[1], 0), t[2] == "1"));
    } else if (t[0] == "B" && t.size() == 4) {
      const uint64_t n = num(t[1], 0);
      const uint32_t bb = (uint32_t)num(t[2], 0);
      printf("%" PRIu64 " %" PRIu64 "\n", bgzf_writer_blocks(n, bb, t[3] == "1"), bgzf_writer_in_used(n, bb, t[3] == "1"));
    } else if (t[0] == "F" && t.size() == 2) {
      r = Reader();
      r.file = unhex(t[1]);
    } else if (t[0] == "V" && t.size() == 3) {
      r.verdict[num(t[1], 0)] = atoi(t[2].c_str());
    } else if (t[0] == "R" && t.size() == 5) {
      r.read(num(t[1], 0), t[2] == "1", num(t[3], 1ull << 62), t[4] != "-", num(t[4], 0));
    } else {
      fprintf(stderr, "bad command: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}

int checks() {
  int ctx = 0, h = 0;
  void *slot = nullptr;
  uint8_t b[4] = {0, 0, 0, 0};
  uint64_t a = 0, o = 0, m[2] = {0, 0}, q[2] = {0, 0};
  printf("reader_open_ok %d\n", bgzf_reader_open_args(&ctx, 0, &slot));
  printf("reader_open_device_ok %d\n", bgzf_reader_open_args(&ctx, FLATE_HIP_DEVICE_PTRS, &slot));
  printf("reader_open_null_ctx %d\n", bgzf_reader_open_args(nullptr, 0, &slot));
  printf("reader_open_null_result %d\n", bgzf_reader_open_args(&ctx, 0, nullptr));
  printf("reader_open_bad_flag %d\n", bgzf_reader_open_args(&ctx, FLATE_HIP_COMPAT_GO, &slot));
  printf("reader_open_size_only %d\n", bgzf_reader_open_args(&ctx, FLATE_HIP_DEVICE_PTRS | FLATE_HIP_SIZE_ONLY, &slot));
  printf("read_ok %d\n", bgzf_reader_read_args(&h, b, 4, b, 4, &a, &o, 0, nullptr, nullptr));
  printf("read_index_ok %d\n", bgzf_reader_read_args(&h, b, 4, b, 4, &a, &o, 2, m, q));
  printf("read_nothing_ok %d\n", bgzf_reader_read_args(&h, nullptr, 0, nullptr, 0, &a, &o, 0, nullptr, nullptr));
  printf("read_index_cap_without_arrays_ok %d\n", bgzf_reader_read_args(&h, b, 4, b, 4, &a, &o, 7, nullptr, nullptr));
  printf("read_null_reader %d\n", bgzf_reader_read_args(nullptr, b, 4, b, 4, &a, &o, 0, nullptr, nullptr));
  printf("read_null_in %d\n", bgzf_reader_read_args(&h, nullptr, 4, b, 4, &a, &o, 0, nullptr, nullptr));
  printf("read_null_out %d\n", bgzf_reader_read_args(&h, b, 4, nullptr, 4, &a, &o, 0, nullptr, nullptr));
  printf("read_null_in_used %d\n", bgzf_reader_read_args(&h, b, 4, b, 4, nullptr, &o, 0, nullptr, nullptr));
  printf("read_null_out_len %d\n", bgzf_reader_read_args(&h, b, 4, b, 4, &a, nullptr, 0, nullptr, nullptr));
  printf("read_member_off_alone %d\n", bgzf_reader_read_args(&h, b, 4, b, 4, &a, &o, 2, m, nullptr));
  printf("read_out_off_alone %d\n", bgzf_reader_read_args(&h, b, 4, b, 4, &a, &o, 2, nullptr, q));
  printf("read_index_cap_zero %d\n", bgzf_reader_read_args(&h, b, 4, b, 4, &a, &o, 0, m, q));
  printf("writer_open_ok %d\n", bgzf_writer_open_args(&ctx, 0, 0, &slot));
  printf("writer_open_flags_ok %d\n", bgzf_writer_open_args(&ctx, 65535, FLATE_HIP_DEVICE_PTRS | FLATE_HIP_COMPAT_GO, &slot));
  printf("writer_open_one_ok %d\n", bgzf_writer_open_args(&ctx, 1, 0, &slot));
  printf("writer_open_null_ctx %d\n", bgzf_writer_open_args(nullptr, 0, 0, &slot));
  printf("writer_open_null_result %d\n", bgzf_writer_open_args(&ctx, 0, 0, nullptr));
  printf("writer_open_block_65536 %d\n", bgzf_writer_open_args(&ctx, 65536, 0, &slot));
  printf("writer_open_bad_flag %d\n", bgzf_writer_open_args(&ctx, 0, FLATE_HIP_SIZE_ONLY, &slot));
  printf("write_ok %d\n", bgzf_writer_write_args(&h, b, 4, b, &a, &o, false));
  printf("write_nothing_ok %d\n", bgzf_writer_write_args(&h, nullptr, 0, b, &a, &o, false));
  printf("write_null_writer %d\n", bgzf_writer_write_args(nullptr, b, 4, b, &a, &o, false));
  printf("write_null_in %d\n", bgzf_writer_write_args(&h, nullptr, 4, b, &a, &o, false));
  printf("write_null_out %d\n", bgzf_writer_write_args(&h, b, 4, nullptr, &a, &o, false));
  printf("write_null_in_used %d\n", bgzf_writer_write_args(&h, b, 4, b, nullptr, &o, false));
  printf("write_null_out_len %d\n", bgzf_writer_write_args(&h, b, 4, b, &a, nullptr, false));
  printf("write_after_the_end %d\n", bgzf_writer_write_args(&h, b, 4, b, &a, &o, true));
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "run")) return run(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
  fprintf(stderr, "usage: %s run FILE | checks\n", argv[0]);
  return 2;
}
