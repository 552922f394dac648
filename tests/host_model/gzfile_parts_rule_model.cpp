// gzfile_parts_rule_model.cpp -- the rule of a gzip FILE read in parts (moonbit-flate_amd/csrc/gzfile_parts_rule.h) and
// the argument checks of its calls (api_checks.h) as a stand-alone CPU program: the very functions the part kernels and
// flate_hip_gzfile_reader_read compile, driven by tests/test_gzfile_parts_rule_model.py and compared there with
// tests/gzfile_parts_ref.py.
//   gzfile_parts_rule_model run FILE   FILE holds one command per line, numbers in decimal, bytes in hex ("-": none):
//     P final b bytes               -> "kind e bit"     gzfile_parts_hop behind a final block at bit b of `bytes`
//     F bytes                       the file
//     W n status fail_raw stream_err_off fail_out  bit[0..n] off[0..n] start[0..n] reach[0..n) end[0..n) final[0..n)
//                                   the WALK over the whole file (gzfile_ref.Walk): n good units, their bits and output
//                                   offsets (entry n: the failing unit), header offset + 1 of a unit that starts a
//                                   member, the file byte behind what the serial reader holds when a unit ends, the bit
//                                   where it ends, whether it ends with BFINAL; status: the walk's verdict IN a unit
//                                   (0: none) with that member's raw stream's file offset, the serial offset and the
//                                   bytes the failing unit produced
//     T m ok[0..m)                  what the device's comparison says of every whole member's trailer
//     N unit_max                    a fresh reader (nothing printed)
//     R in_len final out_cap        one call on the part of in_len bytes that begins where the reader stands
//                                   -> "rc in_used out_len n_members n_units bad_member err_off stream_err_off"
//   gzfile_parts_rule_model checks  one line per argument-check call: name value
// The driver of R builds what the discovery over the part yields -- the units that are complete in the part's raw range
// [.., in_len - 8), the chain's end by THE PARTS HOP over the part's own bytes -- and follows
// flate_hip_gzfile_reader_read step by step; every decision in it is the rule's.  Every header the root or the hop
// meets is held against gzip_rule.h's gzip_header_len.  The part lies in an allocation of exactly its size: a read
// outside it is a heap overflow the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "api_checks.h"
#include "gzfile_parts_rule.h"
#include "gzip_rule.h"

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
// bytes in an allocation of exactly their size
static uint8_t *exact(const uint8_t *p, size_t n) {
  uint8_t *q = (uint8_t *)malloc(n ? n : 1);
  if (n) memcpy(q, p, n);
  return q;
}

struct World {
  std::vector<uint8_t> file;
  uint32_t n = 0;
  int status = 0;
  uint64_t fail_raw = 0, fail_out = 0;
  int64_t stream_err = -1;
  std::vector<uint64_t> bit, off, start, reach, end;
  std::vector<uint32_t> fin;
  std::vector<int> trailer_ok;
  uint64_t unit_max = 1ull << 28;
  GzPartsState s = gzfile_parts_fresh();
};

// one_parts_header against gzip_header_len on the same bytes
static bool headers_agree(const uint8_t *m, uint64_t len) {
  uint64_t hl = 0;
  const uint32_t st = one_parts_header(kPartsGzip, m, len, &hl);
  const uint64_t theirs = gzip_header_len(m, len);
  return (theirs == 0 || (st == kPartsHdrGood && hl == theirs)) &&
         (st != kPartsHdrGood || len < hl + kGzipTrailerLen || theirs == hl) && (st != kPartsHdrBad || theirs == 0);
}

static void say(const GzPartsState &s, int rc, uint64_t used, uint64_t out, uint32_t members, uint32_t units) {
  const bool bad = rc < 0 && rc != kPartsOutTooSmall && s.status == rc;
  printf("%d %llu %llu %u %u %u %lld %lld\n", rc, (unsigned long long)used, (unsigned long long)out, members, units,
         bad ? s.bad_member : 0xffffffffu, (long long)(bad ? s.err_off : -1), (long long)(bad ? s.stream_err_off : -1));
}

static void call(World &w, uint64_t in_len, bool fin, uint64_t out_cap) {
  GzPartsState &s = w.s;
  if (s.status) return say(s, s.status, 0, 0, 0, 0);
  auto fail_here = [&](int st, bool no_header) {
    s.status = st, s.bad_member = s.members_done, s.err_off = (int64_t)(no_header ? s.consumed : s.member_off);
    s.stream_err_off = -1;
    say(s, st, 0, 0, 0, 0);
  };
  if (in_len == 0) {
    if (!fin) return say(s, kPartsOk, 0, 0, 0, 0);
    if (s.inside) return fail_here(kPartsEof, false);
    s.status = kPartsStreamEnd;
    return say(s, kPartsStreamEnd, 0, 0, 0, 0);
  }
  if (s.inside && in_len <= kGzipTrailerLen) return fin ? fail_here(kPartsEof, false) : say(s, kPartsOk, 0, 0, 0, 0);
  const uint64_t a = s.consumed;
  if (a + in_len > w.file.size()) {
    printf("the part lies outside the file\n");
    return;
  }
  uint8_t *part = exact(w.file.data() + a, in_len);
  struct Free {
    uint8_t *p;
    ~Free() { free(p); }
  } guard{part};
  if (!s.inside) {
    uint64_t hl = 0;
    if (!headers_agree(part, in_len)) printf("gzip_rule.h disagrees at the root\n");
    const uint32_t root = gzfile_parts_root(part, in_len, &hl);
    if (root == kPartsHdrBad || (root && fin)) return fail_here(kPartsCorrupt, true);
    if (root) return in_len >= w.unit_max ? fail_here(kPartsTooLarge, true) : say(s, kPartsOk, 0, 0, 0, 0);
    if (gzip_header_len(part, in_len) != hl) printf("gzip_rule.h disagrees with a good root\n");
  }
  // where the reader stands in the walk
  uint32_t cur = 0;
  while (cur <= w.n && !(s.inside ? w.bit[cur] == 8 * a + s.b0 : w.start[cur] == a + 1)) ++cur;
  if (cur > w.n) {
    printf("the reader stands at no unit of the walk\n");
    return;
  }
  // the discovery over the part, part-relative
  const uint64_t stop = a + in_len - kGzipTrailerLen;
  std::vector<uint64_t> ub, oo, us;
  std::vector<uint32_t> uf;
  GzPartsIndex X{};
  X.rc = kPartsEof, X.err_off = -1, X.fail_unit = 1;  // (a unit that the part's end cuts)
  uint32_t k = cur;
  auto push = [&](uint32_t u) {
    ub.push_back(w.bit[u] - 8 * a);
    oo.push_back(w.off[u] - w.off[cur]);
    us.push_back(w.start[u] && !(u == cur && s.inside) ? w.start[u] - a : 0);
  };
  for (;;) {
    if (k < w.n && w.reach[k] <= stop) {
      push(k);
      uf.push_back(w.fin[k]);
      ++k;
      if (!w.fin[k - 1]) continue;
      const uint64_t b = w.end[k - 1] - 8 * a;
      const GzHop hop = gzfile_parts_hop(part, in_len, b, fin);
      if (hop.e < in_len && !headers_agree(part + hop.e, in_len - hop.e)) printf("gzip_rule.h disagrees behind a hop\n");
      if (hop.kind == kGzHopNext) {
        if (k > w.n || w.start[k] != a + hop.e + 1 || w.bit[k] != 8 * a + hop.bit) printf("the hop misses the walk's next member\n");
        continue;
      }
      X.fail_unit = 0;
      ub.push_back(b), oo.push_back(w.off[k] - w.off[cur]), us.push_back(0);
      if (hop.kind == kGzHopDead) X.rc = kPartsCorrupt, X.err_off = (int64_t)hop.e, X.no_header = 1;
      else X.rc = 0;
      break;
    }
    push(k);  // the unit that fails or is cut
    if (k == w.n && w.status) {
      if (w.status == kPartsCorrupt && w.fail_raw + (uint64_t)w.stream_err <= stop)
        X.rc = kPartsCorrupt, X.err_off = (int64_t)(w.fail_raw + (uint64_t)w.stream_err - a), X.fail_out = w.fail_out;
      else if (fin)
        X.rc = w.status, X.fail_out = w.fail_out;
    }
    break;
  }
  X.n = (uint32_t)uf.size();
  // every array in an allocation of exactly its size
  uint64_t *xb = (uint64_t *)exact((const uint8_t *)ub.data(), ub.size() * 8);
  uint64_t *xo = (uint64_t *)exact((const uint8_t *)oo.data(), oo.size() * 8);
  uint64_t *xs = (uint64_t *)exact((const uint8_t *)us.data(), us.size() * 8);
  uint32_t *xf = (uint32_t *)exact((const uint8_t *)uf.data(), uf.size() * 4);
  Free f1{(uint8_t *)xb}, f2{(uint8_t *)xo}, f3{(uint8_t *)xs}, f4{(uint8_t *)xf};
  X.unit_bit = xb, X.out_off = xo, X.u_start = xs, X.u_final = xf;
  const GzPartsCall c = gzfile_parts_call(s, X, in_len, fin, out_cap, w.unit_max);
  const OnePartsPlan &p = c.plan;
  if (p.action == kPartsNothing) return say(s, kPartsOk, 0, 0, 0, 0);
  if (p.action == kPartsReturn) {
    if (p.status == kPartsOutTooSmall) return say(s, kPartsOutTooSmall, 0, p.need, 0, 0);
    gzfile_parts_fail(s, X, c, GzPartsFail{p.status, 0xffffffffu, 0xffffffffu, -1});
    return say(s, p.status, 0, 0, 0, 0);
  }
  // what the trailer and carry kernels report
  for (uint32_t i = 0; i < c.n_end; ++i) {
    const GzPartSeg &g = c.segs[i];
    const GzPartsMember m = gzfile_parts_member(s, X, g.first_unit);
    if (g.trailer_at + kGzipTrailerLen > in_len) printf("a trailer lies outside the part\n");
    if (m.number < w.trailer_ok.size() && w.trailer_ok[m.number]) continue;
    gzfile_parts_fail(s, X, c, GzPartsFail{kPartsCorrupt, i, 0xffffffffu, -1});
    return say(s, kPartsCorrupt, 0, g.out_end, i, g.last_unit + 1u);
  }
  if (p.terminal && X.rc != 0) {
    gzfile_parts_fail(s, X, c, GzPartsFail{X.rc, 0xffffffffu, 0xffffffffu, -1});
    return say(s, X.rc, 0, p.total, c.n_end, p.n_del);
  }
  s = c.next;
  if (c.at_end) s.status = kPartsStreamEnd;
  say(s, c.at_end ? kPartsStreamEnd : kPartsOk, c.in_used, p.total, c.n_end, p.n_del);
}

static int run(const char *path) {
  FILE *fp = fopen(path, "r");
  if (!fp) return 2;
  World w;
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
    size_t at = 1;
    auto num = [&]() { return at < t.size() ? strtoll(t[at++].c_str(), nullptr, 10) : 0ll; };
    if (t[0] == "P" && t.size() == 4) {
      const bool fin = num() != 0;
      const uint64_t b = (uint64_t)num();
      const std::vector<uint8_t> bytes = unhex(t[3].c_str());
      uint8_t *m = exact(bytes.data(), bytes.size());
      const GzHop h = gzfile_parts_hop(m, bytes.size(), b, fin);
      if (h.e < bytes.size() && !headers_agree(m + h.e, bytes.size() - h.e)) printf("gzip_rule.h disagrees: ");
      printf("%u %llu %llu\n", h.kind, (unsigned long long)h.e, (unsigned long long)h.bit);
      free(m);
    } else if (t[0] == "F" && t.size() == 2) {
      w = World();
      w.file = unhex(t[1].c_str());
    } else if (t[0] == "W" && t.size() >= 6) {
      w.n = (uint32_t)num();
      w.status = (int)num();
      w.fail_raw = (uint64_t)num();
      w.stream_err = num();
      w.fail_out = (uint64_t)num();
      auto take = [&](std::vector<uint64_t> &v, size_t count) {
        v.clear();
        for (size_t q = 0; q < count; ++q) v.push_back((uint64_t)num());
      };
      take(w.bit, (size_t)w.n + 1), take(w.off, (size_t)w.n + 1), take(w.start, (size_t)w.n + 1);
      take(w.reach, w.n), take(w.end, w.n);
      w.fin.clear();
      for (uint32_t q = 0; q < w.n; ++q) w.fin.push_back((uint32_t)num());
    } else if (t[0] == "T" && t.size() >= 2) {
      const size_t m = (size_t)num();
      w.trailer_ok.clear();
      for (size_t q = 0; q < m; ++q) w.trailer_ok.push_back((int)num());
    } else if (t[0] == "N" && t.size() == 2) {
      w.unit_max = (uint64_t)num();
      w.s = gzfile_parts_fresh();
    } else if (t[0] == "R" && t.size() == 4) {
      const uint64_t in_len = (uint64_t)num();
      const bool fin = num() != 0;
      call(w, in_len, fin, (uint64_t)num());
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
  printf("open_ok %d\n", gzfile_reader_open_args(&ctx, 0, &rd));
  printf("open_device_ok %d\n", gzfile_reader_open_args(&ctx, FLATE_HIP_DEVICE_PTRS, &rd));
  printf("open_null_ctx %d\n", gzfile_reader_open_args(nullptr, 0, &rd));
  printf("open_null_result %d\n", gzfile_reader_open_args(&ctx, 0, nullptr));
  printf("open_bad_flag %d\n", gzfile_reader_open_args(&ctx, FLATE_HIP_COMPAT_GO, &rd));
  printf("open_size_only %d\n", gzfile_reader_open_args(&ctx, FLATE_HIP_DEVICE_PTRS | FLATE_HIP_SIZE_ONLY, &rd));
  printf("read_ok %d\n", gzfile_reader_read_args(&rd, b, 4, b, 4, &a, &o));
  printf("read_nothing_ok %d\n", gzfile_reader_read_args(&rd, nullptr, 0, nullptr, 0, &a, &o));
  printf("read_null_reader %d\n", gzfile_reader_read_args(nullptr, b, 4, b, 4, &a, &o));
  printf("read_null_in %d\n", gzfile_reader_read_args(&rd, nullptr, 4, b, 4, &a, &o));
  printf("read_null_out %d\n", gzfile_reader_read_args(&rd, b, 4, nullptr, 4, &a, &o));
  printf("read_null_in_used %d\n", gzfile_reader_read_args(&rd, b, 4, b, 4, nullptr, &o));
  printf("read_null_out_len %d\n", gzfile_reader_read_args(&rd, b, 4, b, 4, &a, nullptr));
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "run")) return run(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
  return 2;
}
