// chain_walk_model.cpp -- the host-compilable parts of the discovery skeleton (moonbit-flate_amd/csrc/chain_rule.h:
// chain_find, chain_next, chain_first, chain_tiles; carve.h: Carve) as a stand-alone program, built by
// tests/test_chain_walk_model.py with g++ under AddressSanitizer and UBSan.
//   find           chain_find against a dictionary walk, every array in an allocation of exactly its size
//   walk <file>    per file of the corpus (u32 count, then u64 length + bytes each): the candidates are every offset
//                  that passes the BGZF member rule, linked by chain_next and followed serially from chain_first;
//                  the line is what bgzf_serial_walk says, and the program fails where the two differ
//   carve          a layout of mixed types and counts, over no buffer and over a buffer: "name offset offset bytes"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "bgzf_rule.h"
#include "carve.h"
#include "chain_rule.h"

using namespace flate;

static void fail(const char *what, uint64_t a, uint64_t b) {
  fprintf(stderr, "chain_walk_model: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
  exit(1);
}

static int run_find() {
  uint64_t checks = 0;
  for (uint32_t n : {0u, 1u, 2u, 1000u}) {
    uint64_t *off = new uint64_t[n];  // (exactly n entries: a read at off[n] is a finding)
    std::map<uint64_t, uint32_t> where;
    uint64_t at = 5, seed = 12345 + n;
    for (uint32_t i = 0; i < n; ++i) {
      off[i] = at, where[at] = i;
      seed = seed * 6364136223846793005ull + 1442695040888963407ull;
      at += 1 + (seed >> 60);  // strictly rising, gaps of 1 .. 16
    }
    std::vector<uint64_t> wants = {0, 4, at, at + 100, ~0ull};  // below the first, above the last
    for (uint32_t i = 0; i < n; ++i) wants.push_back(off[i]), wants.push_back(off[i] + 1), wants.push_back(off[i] - 1);
    std::vector<uint32_t> los = {0, n};
    for (uint32_t i = 0; i < n; i += (n > 16 ? 37 : 1)) los.push_back(i), los.push_back(i + 1);
    for (uint64_t want : wants)
      for (uint32_t lo : los) {
        if (lo > n) continue;
        const auto it = where.find(want);
        const uint32_t expect = (it != where.end() && it->second >= lo) ? it->second : n;
        if (chain_find(off, lo, n, want) != expect) fail("chain_find", want, lo);
        ++checks;
      }
    delete[] off;
  }
  printf("find_ok %llu\n", (unsigned long long)checks);
  // the tiles of a buffer at alignment A over [lo, lo + len): a sum of whole tiles from (lo + A) & ~15 that covers it
  for (uint64_t A = 0; A < 16; ++A)
    for (uint64_t lo : {0ull, 1ull, 15ull, 16ull, 4095ull, 70001ull})
      for (uint64_t len : {1ull, 15ull, 4080ull, 4081ull, 4096ull, 4097ull, 12288ull, 1ull << 40}) {
        const uint64_t t = chain_tiles(A, lo, len), v0 = (lo + A) & ~15ull;
        if (v0 + t * kTileBytes < lo + A + len || v0 + (t - 1) * kTileBytes >= lo + A + len) fail("chain_tiles", lo, len);
      }
  printf("tiles_ok 1\n");
  return 0;
}

static int run_walk(const char *path) {
  FILE *fp = fopen(path, "rb");
  if (!fp) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, fp) != 1) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint64_t len = 0;
    if (fread(&len, 8, 1, fp) != 1) return 2;
    uint8_t *f = new uint8_t[len];  // (exactly len bytes)
    if (len && fread(f, 1, len, fp) != len) return 2;
    std::vector<uint64_t> cand_off;
    std::vector<uint32_t> total;
    for (uint64_t p = 0; p < len; ++p)
      if (const uint32_t t = bgzf_member_total(f + p, len - p)) cand_off.push_back(p), total.push_back(t);
    const uint32_t n = (uint32_t)cand_off.size();
    // the link step, for the two sinks too, then the chain from candidate 0
    std::vector<uint32_t> jump(n + 2);
    for (uint32_t c = 0; c < n + 2; ++c) {
      const uint64_t want = c < n ? cand_off[c] + total[c] : 0;
      jump[c] = chain_next(cand_off.data(), c, n, true, want == len, want);
    }
    if (jump[n] != n || jump[n + 1] != n + 1) fail("a sink does not absorb", k, n);
    std::vector<uint64_t> got;
    uint32_t c = chain_first(cand_off.data(), n);
    int64_t got_err = -1;
    uint64_t end = 0;
    for (; c < n; c = jump[c]) {
      if (!got.empty() && cand_off[c] <= got.back()) fail("the chain does not rise", k, c);
      got.push_back(cand_off[c]);
      end = cand_off[c] + total[c];
    }
    const int got_rc = (c == n || len == 0) ? 0 : -4;
    if (got_rc) got_err = (int64_t)end;
    // the specification
    std::vector<uint64_t> want_off(len / 26 + 2);
    uint64_t want_n = 0;
    int64_t want_err = -1;
    const int want_rc = bgzf_serial_walk(f, len, &want_n, &want_err, want_off.data());
    if (got_rc != want_rc || got.size() != want_n || got_err != want_err) fail("the chain is not the serial walk", k, got.size());
    for (uint64_t i = 0; i < want_n; ++i)
      if (got[i] != want_off[i]) fail("a member offset differs", k, i);
    printf("%d %llu %lld |", got_rc, (unsigned long long)got.size(), (long long)got_err);
    if (!got_rc) {
      for (uint64_t o : got) printf(" %llu", (unsigned long long)o);
      printf(" %llu", (unsigned long long)len);
    }
    printf("\n");
    delete[] f;
  }
  fclose(fp);
  return 0;
}

namespace {
struct Rec {
  uint64_t a;
  uint32_t b, c;
  uint8_t d[7];
};
struct Layout {
  uint64_t *head;
  uint8_t *bytes;
  uint32_t *none;  // a count of 0
  uint16_t *halves;
  Rec *recs;
  int64_t *last;
  void lay(flate_host::Carve &k, std::vector<size_t> *ends) {
    auto mark = [&] { if (ends) ends->push_back(k.at); };
    k.take(head, 1), mark();
    k.take(bytes, 257), mark();
    k.take(none, 0), mark();
    k.take(halves, 128), mark();  // exactly 256 bytes
    k.take(recs, 3, 8), mark();   // with slack
    k.take(last, 1000), mark();
  }
};
}  // namespace

static int run_carve() {
  Layout size_pass{}, ptr_pass{};
  flate_host::Carve k0;
  std::vector<size_t> ends;
  size_pass.lay(k0, &ends);
  uint8_t *buf = (uint8_t *)aligned_alloc(256, k0.at ? k0.at : 256);
  flate_host::Carve k1{buf, 0};
  ptr_pass.lay(k1, nullptr);
  if (k0.at != k1.at) fail("the two passes disagree on the size", k0.at, k1.at);
  memset(buf, 0x5a, k1.at);  // (every array lies inside the buffer)
  ptr_pass.head[0] = 1, ptr_pass.bytes[256] = 2, ptr_pass.halves[127] = 3, ptr_pass.recs[2].d[6] = 4, ptr_pass.last[999] = 5;
  const void *s[] = {size_pass.head, size_pass.bytes, size_pass.none, size_pass.halves, size_pass.recs, size_pass.last};
  const void *p[] = {ptr_pass.head, ptr_pass.bytes, ptr_pass.none, ptr_pass.halves, ptr_pass.recs, ptr_pass.last};
  const size_t bytes[] = {8, 257, 0, 256, 3 * sizeof(Rec) + 8, 8000};
  const char *names[] = {"head", "bytes", "none", "halves", "recs", "last"};
  for (int i = 0; i < 6; ++i)
    printf("%s %llu %llu %llu %llu\n", names[i], (unsigned long long)(uintptr_t)s[i],
           (unsigned long long)((const uint8_t *)p[i] - buf), (unsigned long long)bytes[i], (unsigned long long)ends[i]);
  printf("total %llu\n", (unsigned long long)k1.at);
  free(buf);
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 2 && !strcmp(argv[1], "find")) return run_find();
  if (argc >= 3 && !strcmp(argv[1], "walk")) return run_walk(argv[2]);
  if (argc >= 2 && !strcmp(argv[1], "carve")) return run_carve();
  return 2;
}
