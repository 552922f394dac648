// one_parts_rule_model.cpp -- the rule of ONE stream read in parts (moonbit-flate_amd/csrc/one_parts_rule.h) and the
// argument checks of its calls (api_checks.h) as a stand-alone CPU program: the very functions the part kernels and
// flate_hip_one_reader_read compile, driven by tests/test_one_parts_rule_model.py and compared there with
// tests/one_parts_ref.py.
//   one_parts_rule_model run FILE   FILE holds one command per line, numbers in decimal, bytes in hex ("-": none):
//     H wrap bytes                  -> "state hl"                            one_parts_header (gzip: held against
//                                                                           gzip_rule.h's gzip_header_len first)
//     F wrap first final bytes      -> "hdr raw_off raw_end"                 one_parts_frame
//     N wrap unit_max               a fresh reader (nothing printed)
//     R in_len final out_cap bytes rc err_off fail_unit fail_out trailer_ok n bit[0..n] off[0..n]
//                                   one call of the reader on a part of in_len bytes whose first min(in_len, 64) are
//                                   `bytes` ("-" behind the header); rc .. off: what the discovery over the part yields (rc 99: no candidate),
//                                   trailer_ok: what the device's comparison says if the trailer is judged
//                                   -> "rc in_used out_len n_units err_off"
//   one_parts_rule_model checks     one line per argument-check call: name value
// The driver of R follows flate_hip_one_reader_read step by step; every decision in it is the rule's.  Every array lies
// in an allocation of exactly its size: a read outside it is a heap overflow the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "api_checks.h"
#include "gzip_rule.h"
#include "one_parts_rule.h"

using namespace flate;

static std::vector<uint8_t> unhex(const char *s) {
  std::vector<uint8_t> v;
  if (!strcmp(s, "-")) return v;
  for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
    unsigned b = 0;
    sscanf(s + i, "%2x", &b);
    v.push_back((uint8_t)b);
  }
  return v;
}
// the bytes in an allocation of exactly their size
static uint8_t *exact(const std::vector<uint8_t> &v) {
  uint8_t *p = (uint8_t *)malloc(v.size() ? v.size() : 1);
  if (!v.empty()) memcpy(p, v.data(), v.size());
  return p;
}

struct Reader {
  uint32_t wrap = 0;
  uint64_t unit_max = 0;
  OnePartsState s = one_parts_fresh();
};

static void call(Reader &r, std::vector<std::string> &t) {
  size_t at = 1;
  auto num = [&]() { return strtoll(t[at++].c_str(), nullptr, 10); };
  const uint64_t in_len = (uint64_t)num();
  const bool fin = num() != 0;
  const uint64_t out_cap = (uint64_t)num();
  const std::vector<uint8_t> bytes = unhex(t[at++].c_str());
  const int rc = (int)num();
  const int64_t d_err = num();
  const uint32_t fail_unit = (uint32_t)num();
  const uint64_t fail_out = (uint64_t)num();
  const bool trailer_ok = num() != 0;
  const uint32_t n = (uint32_t)num();
  uint64_t *bit = (uint64_t *)malloc(((size_t)n + 1) * 8), *off = (uint64_t *)malloc(((size_t)n + 1) * 8);
  for (uint32_t k = 0; k <= n && rc != 99; ++k) bit[k] = (uint64_t)num();
  for (uint32_t k = 0; k <= n && rc != 99; ++k) off[k] = (uint64_t)num();
  OnePartsState &s = r.s;
  const uint32_t tl = one_parts_trailer_len(r.wrap);
  auto say = [&](int st, uint64_t used, uint64_t out, uint32_t units, int64_t eo) {
    printf("%d %llu %llu %u %lld\n", st, (unsigned long long)used, (unsigned long long)out, units, (long long)eo);
    free(bit), free(off);
  };
  auto fail = [&](int st, int64_t eo, uint64_t used = 0, uint64_t out = 0, uint32_t units = 0) {
    s.status = st, s.err_off = eo;
    say(st, used, out, units, eo);
  };
  if (s.status) return say(s.status, 0, 0, 0, s.status < 0 ? s.err_off : -1);
  if (s.trailer_pending) {
    if (in_len < tl) return fin ? fail(kPartsEof, -1) : say(kPartsOk, 0, 0, 0, -1);
    s.consumed += tl, s.trailer_pending = 0;
    if (!trailer_ok) return fail(kPartsCorrupt, (int64_t)s.consumed, tl);
    s.status = kPartsStreamEnd;
    return say(kPartsStreamEnd, tl, 0, 0, -1);
  }
  if (in_len == 0) {
    if (!fin) return say(kPartsOk, 0, 0, 0, -1);
    return !s.header_done && r.wrap != kPartsRaw ? fail(kPartsCorrupt, 0) : fail(kPartsEof, -1);
  }
  uint8_t *m = exact(bytes);
  const OnePartFrame f = one_parts_frame(r.wrap, !s.header_done, fin, m, bytes.size() < in_len ? bytes.size() : in_len);
  free(m);
  // (the frame of a part longer than the bytes given: only its end differs)
  const uint64_t raw_off = f.raw_off;
  if (f.hdr == kPartsHdrBad) return fail(kPartsCorrupt, 0);
  if (f.hdr == kPartsHdrMore || rc == 99) return fin ? fail(kPartsEof, -1) : say(kPartsOk, 0, 0, 0, -1);
  const OnePartsPlan p = one_parts_plan(n, off, rc, fail_unit, fail_out, fin, out_cap, in_len, r.unit_max);
  if (p.action == kPartsNothing) return say(kPartsOk, 0, 0, 0, -1);
  if (p.action == kPartsReturn) {
    if (p.status == kPartsOutTooSmall) return say(kPartsOutTooSmall, 0, p.need, 0, -1);
    return fail(p.status, d_err >= 0 ? (int64_t)s.raw_base + d_err : -1);
  }
  if (p.terminal && rc != 0)
    return fail(rc, d_err >= 0 ? (int64_t)s.raw_base + d_err : -1, 0, p.total, p.n_del);
  const bool ended = p.terminal && rc == 0;
  OnePartsState next = s;
  uint64_t used = 0;
  bool trailer_now = false;
  one_parts_advance(next, r.wrap, raw_off, bit[p.n_del], p.total, ended, in_len, &used, &trailer_now);
  if (ended && trailer_now && tl && !trailer_ok) return fail(kPartsCorrupt, (int64_t)next.consumed, 0, p.total, p.n_del);
  s = next;
  if (ended && trailer_now) s.status = kPartsStreamEnd;
  say(ended && trailer_now ? kPartsStreamEnd : kPartsOk, used, p.total, p.n_del, -1);
}

static int run(const char *path) {
  FILE *fp = fopen(path, "r");
  if (!fp) return 2;
  Reader r;
  std::string line;
  int ch;
  auto flush_line = [&]() {
    std::vector<std::string> t;
    size_t i = 0;
    while (i < line.size()) {
      while (i < line.size() && line[i] == ' ') ++i;
      size_t j = i;
      while (j < line.size() && line[j] != ' ') ++j;
      if (j > i) t.push_back(line.substr(i, j - i));
      i = j;
    }
    line.clear();
    if (t.empty()) return;
    if (t[0] == "H" && t.size() == 3) {
      const std::vector<uint8_t> b = unhex(t[2].c_str());
      uint8_t *m = exact(b);
      uint64_t hl = 0;
      const uint32_t wrap = (uint32_t)atoi(t[1].c_str());
      const uint32_t st = one_parts_header(wrap, m, b.size(), &hl);
      // the whole call's header rule (gzip_rule.h, which frame_parse_kernel applies) says the same of the same bytes:
      // what it takes is good here with that length, and what is good here with room for the trailer it takes
      const uint64_t theirs = wrap == kPartsGzip ? gzip_header_len(m, b.size()) : 0;
      const bool agree = wrap != kPartsGzip || ((theirs == 0 || (st == kPartsHdrGood && hl == theirs)) &&
                                                (st != kPartsHdrGood || b.size() < hl + kGzipTrailerLen || theirs == hl) &&
                                                (st != kPartsHdrBad || theirs == 0));
      if (agree) printf("%u %llu\n", st, (unsigned long long)hl);
      else printf("gzip_rule.h disagrees: %u %llu, theirs %llu\n", st, (unsigned long long)hl, (unsigned long long)theirs);
      free(m);
    } else if (t[0] == "F" && t.size() == 5) {
      const std::vector<uint8_t> b = unhex(t[4].c_str());
      uint8_t *m = exact(b);
      const OnePartFrame f = one_parts_frame((uint32_t)atoi(t[1].c_str()), atoi(t[2].c_str()) != 0, atoi(t[3].c_str()) != 0, m, b.size());
      printf("%u %llu %llu\n", f.hdr, (unsigned long long)f.raw_off, (unsigned long long)f.raw_end);
      free(m);
    } else if (t[0] == "N" && t.size() == 3) {
      r = Reader();
      r.wrap = (uint32_t)atoi(t[1].c_str());
      r.unit_max = strtoull(t[2].c_str(), nullptr, 10);
    } else if (t[0] == "R" && t.size() >= 11) {
      call(r, t);
    } else {
      printf("?\n");
    }
  };
  while ((ch = fgetc(fp)) != EOF) {
    if (ch == '\n') flush_line();
    else line.push_back((char)ch);
  }
  flush_line();
  fclose(fp);
  return 0;
}

static int checks() {
  int ctx = 0, rd = 0;
  uint8_t b[4] = {0, 0, 0, 0};
  uint64_t a = 0, o = 0;
  printf("open_ok %d\n", one_reader_open_args(&ctx, FLATE_HIP_WRAP_GZIP, FLATE_HIP_DEVICE_PTRS, &rd));
  printf("open_raw_ok %d\n", one_reader_open_args(&ctx, FLATE_HIP_WRAP_RAW, 0, &rd));
  printf("open_null_ctx %d\n", one_reader_open_args(nullptr, FLATE_HIP_WRAP_GZIP, 0, &rd));
  printf("open_null_result %d\n", one_reader_open_args(&ctx, FLATE_HIP_WRAP_GZIP, 0, nullptr));
  printf("open_bad_wrap %d\n", one_reader_open_args(&ctx, 3, 0, &rd));
  printf("open_bad_flag %d\n", one_reader_open_args(&ctx, FLATE_HIP_WRAP_ZLIB, FLATE_HIP_COMPAT_GO, &rd));
  printf("read_ok %d\n", one_reader_read_args(&rd, b, 4, b, 4, &a, &o));
  printf("read_nothing_ok %d\n", one_reader_read_args(&rd, nullptr, 0, nullptr, 0, &a, &o));
  printf("read_null_reader %d\n", one_reader_read_args(nullptr, b, 4, b, 4, &a, &o));
  printf("read_null_in %d\n", one_reader_read_args(&rd, nullptr, 4, b, 4, &a, &o));
  printf("read_null_out %d\n", one_reader_read_args(&rd, b, 4, nullptr, 4, &a, &o));
  printf("read_null_in_used %d\n", one_reader_read_args(&rd, b, 4, b, 4, nullptr, &o));
  printf("read_null_out_len %d\n", one_reader_read_args(&rd, b, 4, b, 4, &a, nullptr));
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "run")) return run(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
  return 2;
}
