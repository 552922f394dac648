// gzfile_parts_serial_rule_model.cpp -- the rule of a gzip FILE read in parts with short members decoded WHOLE
// (moonbit-flate_amd/csrc/gzfile_parts_serial_rule.h) and the argument checks of its two calls (api_checks.h) as a
// stand-alone CPU program: the very functions the kernels and flate_hip_gzfile_reader_read compile, driven by
// tests/test_gzfile_parts_serial_rule_model.py and compared there with tests/gzfile_parts_serial_ref.py.
//   gzfile_parts_serial_rule_model run FILE   FILE holds one command per line, numbers in decimal, bytes in hex ("-"):
//     V final S out_cap p status used out bytes   -> "verdict"   THE THREE VERDICTS of the candidate at p of `bytes`
//     F bytes / W ... / T ...       the file, the WALK over it and the trailers, as gzfile_parts_rule_model.cpp takes them
//     N unit_max S                  a fresh reader with the setting S (nothing printed)
//     C n  off used z s  ...        the List B of the NEXT call's part: every offset that passes the header rule over
//                                   the part, with what the size-only decode over its serial range left
//     R in_len final out_cap        one call on the part of in_len bytes that begins where the reader stands
//         -> "rc in_used out_len n_members n_units bad_member err_off stream_err_off serial_members open_stop find_from"
//   gzfile_parts_serial_rule_model checks   one line per argument-check call: name value
//   gzfile_parts_serial_rule_model equalities   the whole file as the part that is final and starts at a BOUNDARY: one
//                                   line per equality: name cases mismatches, then how often each answer occurred
// The driver of R builds what the discovery over the part yields -- a WHOLE member as one unit with its phase-1 record,
// every other member's units that are complete in the part's raw range, the chain's end by the hop with the OPEN stop
// -- and follows flate_hip_gzfile_reader_read step by step; every decision in it is the rule's.  The part lies in an
// allocation of exactly its size: a read outside it is a heap overflow the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "api_checks.h"
#include "gzfile_parts_serial_rule.h"
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
struct Free {
  uint8_t *p;
  ~Free() { free(p); }
};

struct World {
  std::vector<uint8_t> file;
  uint32_t n = 0;
  int status = 0;
  uint64_t fail_raw = 0, fail_out = 0;
  int64_t stream_err = -1;
  std::vector<uint64_t> bit, off, start, reach, end;
  std::vector<uint32_t> fin;
  std::vector<int> trailer_ok;
  std::vector<GzSerialCand> cand;  // of the next call's part
  uint64_t unit_max = 1ull << 28, S = 0;
  GzPartsState s = gzfile_parts_fresh();
  uint32_t route_members = 0, route_open = 0;
  uint64_t route_from = 0;
};

static void say(const World &w, int rc, uint64_t used, uint64_t out, uint32_t members, uint32_t units) {
  const GzPartsState &s = w.s;
  const bool bad = rc < 0 && rc != kPartsOutTooSmall && s.status == rc;
  printf("%d %llu %llu %u %u %u %lld %lld %u %u %llu\n", rc, (unsigned long long)used, (unsigned long long)out, members, units,
         bad ? s.bad_member : 0xffffffffu, (long long)(bad ? s.err_off : -1), (long long)(bad ? s.stream_err_off : -1),
         w.route_members, w.route_open, (unsigned long long)w.route_from);
}

static void call(World &w, uint64_t in_len, bool fin, uint64_t out_cap) {
  GzPartsState &s = w.s;
  if (s.status) return say(w, s.status, 0, 0, 0, 0);
  auto fail_here = [&](int st, bool no_header) {
    s.status = st, s.bad_member = s.members_done, s.err_off = (int64_t)(no_header ? s.consumed : s.member_off);
    s.stream_err_off = -1;
    say(w, st, 0, 0, 0, 0);
  };
  if (in_len == 0) {
    if (!fin) return say(w, kPartsOk, 0, 0, 0, 0);
    if (s.inside) return fail_here(kPartsEof, false);
    s.status = kPartsStreamEnd;
    return say(w, kPartsStreamEnd, 0, 0, 0, 0);
  }
  if (s.inside && in_len <= kGzipTrailerLen) return fin ? fail_here(kPartsEof, false) : say(w, kPartsOk, 0, 0, 0, 0);
  const uint64_t a = s.consumed, S = w.S;
  if (a + in_len > w.file.size()) {
    printf("the part lies outside the file\n");
    return;
  }
  uint8_t *part = exact(w.file.data() + a, in_len);
  Free guard{part};
  if (!s.inside) {
    uint64_t hl = 0;
    const uint32_t root = gzfile_parts_root(part, in_len, &hl);
    if (root == kPartsHdrBad || (root && fin)) return fail_here(kPartsCorrupt, true);
    if (root) return in_len >= w.unit_max ? fail_here(kPartsTooLarge, true) : say(w, kPartsOk, 0, 0, 0, 0);
  }
  // phase 1: the verdicts of List B, the walk
  const std::vector<GzSerialCand> &cand = w.cand;
  std::vector<uint32_t> verdict(cand.size(), kGzPartLong);
  for (size_t j = 0; j < cand.size(); ++j) {
    const uint64_t p = cand[j].off;
    if (p >= in_len || gzip_header_len(part + p, in_len - p) == 0) printf("a candidate does not pass the header rule\n");
    verdict[j] = gzfile_parts_serial_verdict(in_len, fin, S, out_cap, p, gzip_header_len(part + p, in_len - p), cand[j].s,
                                             cand[j].used, cand[j].z);
  }
  auto cand_at = [&](uint64_t p) -> size_t {
    for (size_t j = 0; j < cand.size(); ++j)
      if (cand[j].off == p) return j;
    return cand.size();
  };
  auto verdict_at = [&](uint64_t e) { return cand_at(e) < cand.size() ? verdict[cand_at(e)] : kGzPartLong; };
  uint64_t find_from = 0, walk_whole = 0;
  uint32_t walk_open = 0;
  if (S) find_from = gzfile_parts_serial_walk(part, in_len, fin, s.inside != 0, S, out_cap, cand.data(), cand.size(), &walk_whole, &walk_open);
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
  std::vector<uint32_t> uf, uw;
  GzPartsIndex X{};
  X.rc = kPartsEof, X.err_off = -1, X.fail_unit = 1;  // (a unit that the part's end cuts)
  uint32_t k = cur, chain_open = 0;
  auto push = [&](uint32_t u) {
    ub.push_back(w.bit[u] - 8 * a);
    oo.push_back(w.off[u] - w.off[cur]);
    us.push_back(w.start[u] && !(u == cur && s.inside) ? w.start[u] - a : 0);
  };
  // behind a member's final block at part bit b, with k at the unit behind it: true = the chain goes on
  auto hop_on = [&](uint64_t b) {
    const GzHop hop = S ? gzfile_parts_serial_hop(part, in_len, b, fin, verdict_at) : gzfile_parts_hop(part, in_len, b, fin);
    if (hop.kind == kGzHopNext) {
      if (k > w.n || w.start[k] != a + hop.e + 1 || w.bit[k] != 8 * a + hop.bit) printf("the hop misses the walk's next member\n");
      return true;
    }
    X.fail_unit = 0;
    ub.push_back(b), oo.push_back(w.off[k] - w.off[cur]), us.push_back(0);
    if (hop.kind == kGzHopDead) X.rc = kPartsCorrupt, X.err_off = (int64_t)hop.e, X.no_header = 1;
    else X.rc = 0;
    chain_open = hop.kind == kGzHopStop && hop.e < in_len && gzfile_first_bit(part, in_len, hop.e) != 0ull ? 1u : 0u;
    return false;
  };
  for (;;) {
    if (S && k <= w.n && w.start[k] && !(k == cur && s.inside)) {  // a member's first unit: is the member WHOLE
      const uint64_t p = w.start[k] - 1 - a;
      const size_t j = cand_at(p);
      if (j == cand.size()) {
        printf("a member of the chain is no candidate\n");
        return;
      }
      if (verdict[j] == kGzPartOpen && p > 0) printf("the chain reached an OPEN member\n");
      if (verdict[j] == kGzPartWhole) {
        const uint64_t hl = gzip_header_len(part + p, in_len - p);
        const GzSerialRecord r = gzfile_serial_record(p, hl, cand[j].used, cand[j].z);
        uint32_t k2 = k + 1;
        while (k2 < w.n && !w.start[k2]) ++k2;
        if (k2 > w.n || w.off[k2] - w.off[k] != cand[j].z || (w.end[k2 - 1] - 8 * a + 7) / 8 != r.end_bit / 8)
          printf("a whole member is not the walk's\n");
        push(k);
        uf.push_back(1), uw.push_back(1);
        k = k2;
        if (hop_on(r.end_bit)) continue;
        break;
      }
    }
    if (k < w.n && w.reach[k] <= stop) {
      push(k);
      uf.push_back(w.fin[k]), uw.push_back(0);
      ++k;
      if (!w.fin[k - 1]) continue;
      if (hop_on(w.end[k - 1] - 8 * a)) continue;
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
  uw.push_back(0);
  X.n = (uint32_t)uf.size();
  // every array in an allocation of exactly its size
  uint64_t *xb = (uint64_t *)exact((const uint8_t *)ub.data(), ub.size() * 8);
  uint64_t *xo = (uint64_t *)exact((const uint8_t *)oo.data(), oo.size() * 8);
  uint64_t *xs = (uint64_t *)exact((const uint8_t *)us.data(), us.size() * 8);
  uint32_t *xf = (uint32_t *)exact((const uint8_t *)uf.data(), uf.size() * 4);
  uint32_t *xw = (uint32_t *)exact((const uint8_t *)uw.data(), uw.size() * 4);
  Free f1{(uint8_t *)xb}, f2{(uint8_t *)xo}, f3{(uint8_t *)xs}, f4{(uint8_t *)xf}, f5{(uint8_t *)xw};
  X.unit_bit = xb, X.out_off = xo, X.u_start = xs, X.u_final = xf;
  w.route_members = 0, w.route_open = S ? chain_open : 0u, w.route_from = find_from;
  if (S && !s.inside && walk_open && !chain_open) printf("the walk stopped in front of an OPEN member, the chain did not\n");
  const GzPartsCall c = gzfile_parts_serial_call(s, X, in_len, fin, out_cap, w.unit_max, S);
  const OnePartsPlan &p = c.plan;
  if (p.action == kPartsNothing) return say(w, kPartsOk, 0, 0, 0, 0);
  if (p.action == kPartsReturn) {
    if (p.status == kPartsOutTooSmall) return say(w, kPartsOutTooSmall, 0, p.need, 0, 0);
    gzfile_parts_fail(s, X, c, GzPartsFail{p.status, 0xffffffffu, 0xffffffffu, -1});
    return say(w, p.status, 0, 0, 0, 0);
  }
  // what the trailer and carry kernels report
  for (uint32_t i = 0; i < c.n_end; ++i) {
    const GzPartSeg &g = c.segs[i];
    const GzPartsMember m = gzfile_parts_member(s, X, g.first_unit);
    if (g.trailer_at + kGzipTrailerLen > in_len) printf("a trailer lies outside the part\n");
    if (m.number < w.trailer_ok.size() && w.trailer_ok[m.number]) continue;
    gzfile_parts_fail(s, X, c, GzPartsFail{kPartsCorrupt, i, 0xffffffffu, -1});
    w.route_members = gzfile_parts_serial_count(xw, g.last_unit + 1u);
    return say(w, kPartsCorrupt, 0, g.out_end, i, g.last_unit + 1u);
  }
  w.route_members = gzfile_parts_serial_count(xw, p.n_del);
  if (p.terminal && X.rc != 0) {
    gzfile_parts_fail(s, X, c, GzPartsFail{X.rc, 0xffffffffu, 0xffffffffu, -1});
    return say(w, X.rc, 0, p.total, c.n_end, p.n_del);
  }
  s = c.next;
  if (c.at_end) s.status = kPartsStreamEnd;
  say(w, c.at_end ? kPartsStreamEnd : kPartsOk, c.in_used, p.total, c.n_end, p.n_del);
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
    if (t[0] == "V" && t.size() == 9) {
      const bool fin = num() != 0;
      const uint64_t S = (uint64_t)num(), out_cap = (uint64_t)num(), p = (uint64_t)num();
      const int32_t st = (int32_t)num();
      const uint64_t used = (uint64_t)num(), out = (uint64_t)num();
      const std::vector<uint8_t> bytes = unhex(t[8].c_str());
      uint8_t *m = exact(bytes.data(), bytes.size());
      const uint64_t hl = p < bytes.size() ? gzip_header_len(m + p, bytes.size() - p) : 0;
      printf("%u\n", gzfile_parts_serial_verdict(bytes.size(), fin, S, out_cap, p, hl, st, used, out));
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
    } else if (t[0] == "N" && t.size() == 3) {
      w.unit_max = (uint64_t)num();
      w.S = (uint64_t)num();
      w.s = gzfile_parts_fresh();
      w.route_members = w.route_open = 0, w.route_from = 0;
    } else if (t[0] == "C" && t.size() >= 2) {
      const size_t m = (size_t)num();
      w.cand.clear();
      for (size_t q = 0; q < m; ++q) {
        GzSerialCand c{};
        c.off = (uint64_t)num(), c.used = (uint64_t)num(), c.z = (uint64_t)num(), c.s = (int32_t)num();
        w.cand.push_back(c);
      }
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
  int rd = 0;
  uint32_t a = 0, b = 0;
  uint64_t f = 0;
  printf("set_ok %d\n", gzfile_reader_set_serial_max_args(&rd, 4096, true));
  printf("set_zero_ok %d\n", gzfile_reader_set_serial_max_args(&rd, 0, true));
  printf("set_largest_ok %d\n", gzfile_reader_set_serial_max_args(&rd, (1ull << 28) - 1, true));
  printf("set_too_large %d\n", gzfile_reader_set_serial_max_args(&rd, 1ull << 28, true));
  printf("set_huge %d\n", gzfile_reader_set_serial_max_args(&rd, ~0ull, true));
  printf("set_not_fresh %d\n", gzfile_reader_set_serial_max_args(&rd, 4096, false));
  printf("set_null_reader %d\n", gzfile_reader_set_serial_max_args(nullptr, 4096, true));
  printf("route_ok %d\n", gzfile_reader_last_route_args(&rd, &a, &b, &f));
  printf("route_null_reader %d\n", gzfile_reader_last_route_args(nullptr, &a, &b, &f));
  printf("route_null_members %d\n", gzfile_reader_last_route_args(&rd, nullptr, &b, &f));
  printf("route_null_open %d\n", gzfile_reader_last_route_args(&rd, &a, nullptr, &f));
  printf("route_null_from %d\n", gzfile_reader_last_route_args(&rd, &a, &b, nullptr));
  GzPartsState s = gzfile_parts_fresh();
  printf("fresh_ok %d\n", gzfile_parts_is_fresh(s) ? 0 : -1);
  s.consumed = 1;
  printf("fresh_consumed %d\n", gzfile_parts_is_fresh(s) ? 0 : -1);
  s = gzfile_parts_fresh();
  s.status = kPartsStreamEnd;
  printf("fresh_ended %d\n", gzfile_parts_is_fresh(s) ? 0 : -1);
  return 0;
}

// THE THREE EQUALITIES the kernels rest on when they run the whole file as the part that is final and starts at a
// BOUNDARY.  One line each: name, the cases swept, the mismatches, then how often each answer occurred.
static int equalities() {
  // 1. gzfile_parts_hop(.., final) == gzfile_hop in all three fields, at every end bit of hand-built buffers: four
  // bytes of a stream, a trailer, and behind it ...
  const std::vector<uint8_t> head = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
  std::vector<std::vector<uint8_t>> tails;
  tails.push_back({});                                       // ... the end
  tails.push_back(head), tails.back().resize(head.size() + 9, 0x55);  // ... a good header (a raw byte, a trailer)
  tails.push_back({0x00, 0x1f, 0x8b, 8, 0});                 // ... a bad byte
  tails.push_back({0x1f, 0x8b, 8});                          // ... a header cut in its fixed bytes
  tails.push_back(head), tails.back().resize(head.size() + 7, 0x55);  // ... a header with no room for a trailer
  tails.push_back(head), tails.back()[3] = 8, tails.back().resize(head.size() + 12, 0x41);  // ... FNAME without its NUL
  tails.push_back(head), tails.back()[3] = 0x20;             // ... a reserved FLG bit
  unsigned long long cases = 0, bad = 0, kinds[3] = {0, 0, 0}, beyond = 0;
  for (const std::vector<uint8_t> &tail : tails) {
    std::vector<uint8_t> buf(4 + kGzipTrailerLen, 0xaa);
    buf.insert(buf.end(), tail.begin(), tail.end());
    if (buf.size() > 64) return 3;
    uint8_t *m = exact(buf.data(), buf.size());
    Free guard{m};
    const uint64_t n = buf.size();
    for (uint64_t b = 0; b <= 8 * n + 8; ++b) {  // (the last ones: e > in_len)
      const GzHop x = gzfile_hop(m, n, b), y = gzfile_parts_hop(m, n, b, true);
      ++cases;
      if (x.kind != y.kind || x.e != y.e || x.bit != y.bit || x.kind > kGzHopNext) ++bad;
      else ++kinds[x.kind];
      if (x.e > n) ++beyond;
    }
  }
  printf("hop %llu %llu end %llu dead %llu next %llu beyond %llu\n", cases, bad, kinds[kGzHopEnd], kinds[kGzHopDead],
         kinds[kGzHopNext], beyond);

  // 2. gzfile_parts_serial_verdict(in_len, final, S, ~0, ..) is WHOLE exactly where gzfile_serial_whole holds, LONG
  // elsewhere, never OPEN
  cases = bad = 0;
  unsigned long long n_whole = 0, n_long = 0;
  const int32_t statuses[] = {0, kPartsCorrupt, kPartsEof, kPartsOutTooSmall, kPartsTooLarge};
  const uint64_t Ss[] = {1, 5, 16, 30, 64, kGzSerialMax}, hls[] = {0, 10, 12, 19}, outs[] = {0, 7, 1ull << 33, ~0ull};
  for (uint64_t in_len = 0; in_len <= 48; ++in_len)
    for (uint64_t p = 0; p <= in_len; ++p)
      for (uint64_t S : Ss)
        for (uint64_t hl : hls)
          for (int32_t st : statuses)
            for (uint64_t used = 0; used <= in_len + 1; ++used)
              for (uint64_t out : outs) {
                const uint32_t v = gzfile_parts_serial_verdict(in_len, true, S, ~0ull, p, hl, st, used, out);
                const bool whole = gzfile_serial_whole(st, p, hl, used, gzfile_serial_end(in_len, p, S));
                ++cases;
                if (v != (whole ? kGzPartWhole : kGzPartLong)) ++bad;
                whole ? ++n_whole : ++n_long;
              }
  printf("verdict %llu %llu whole %llu long %llu\n", cases, bad, n_whole, n_long);

  // 3. gzfile_parts_serial_from at a BOUNDARY with a verdict that is not OPEN: in_len if the walk rested nowhere, else
  // where it rested, and no OPEN stop -- what the whole call's from kernel computed before it took the part's form
  cases = bad = 0;
  const uint64_t lens[] = {0, 1, 18, 77, 1ull << 40};
  for (uint64_t in_len : lens)
    for (uint64_t off : lens)
      for (int none = 0; none < 2; ++none)
        for (uint32_t v : {kGzPartLong, kGzPartWhole}) {
          uint32_t open_stop = 7;
          const uint64_t from = gzfile_parts_serial_from(in_len, false, none != 0, off, v, &open_stop);
          ++cases;
          if (from != (none ? in_len : off) || open_stop != 0) ++bad;
        }
  printf("from %llu %llu\n", cases, bad);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "run")) return run(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
  if (argc == 2 && !strcmp(argv[1], "equalities")) return equalities();
  return 2;
}
