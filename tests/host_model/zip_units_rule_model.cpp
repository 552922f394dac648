// zip_units_rule_model.cpp -- the rule of ZIP's long entries (moonbit-flate_amd/csrc/zip_units_rule.h) and the check of
// its option (api_checks.h) as a stand-alone CPU program: the very functions the kernels and the entry point compile,
// driven by tests/test_zip_units_model.py and compared there with tests/zip_units_ref.py.
//   zip_units_rule_model form FILE    FILE = u32 count, then per case: u64 unit_min, u32 n, per entry u64 data_off, u64
//                                     comp_size, u64 size, i32 status, u32 method; u32 has_sel, u32 ns, ns x u32 sel.
//                                     One line per case: fallback hull_lo hull_hi | L: slot,lo,end,size,out ... | R:
//                                     lo,end,entry ...  (lo / end counted from hull_lo; out = the read's slots)
//   zip_units_rule_model chain FILE   FILE = u32 count, then per case: u32 na, u32 nb, na x u64 cand_off, nb x (u64 lo,
//                                     u64 end, u64 size, u64 out), then per node of na + nb: u32 ok, u32 final, u64
//                                     end_bit, u64 out.  One line per case: the nodes' links | the units of the path
//                                     from the first B node, each node,entry,slot,history | g
//   zip_units_rule_model served FILE  FILE = u32 count, per case u32 g_disc, u32 bad_unit, (g_disc + 1) x u64
//                                     entry_unit.  Prints g per case
//   zip_units_rule_model checks       one line per argument-check call: value verdict
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "api_checks.h"
#include "zip_units_rule.h"

using namespace flate;

template <typename T>
static bool rd(FILE *f, T *v) { return fread(v, sizeof(T), 1, f) == 1; }
typedef unsigned long long ull;

static int form(FILE *f) {
  uint32_t count = 0;
  if (!rd(f, &count)) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint64_t unit_min = 0;
    uint32_t n = 0, has_sel = 0, ns = 0;
    if (!rd(f, &unit_min) || !rd(f, &n)) return 2;
    std::vector<flate_hip_zip_entry> ent(n);  // (exact allocations: a read outside is a heap overflow)
    for (auto &e : ent) {
      e = flate_hip_zip_entry{};
      uint32_t method = 0;
      if (!rd(f, &e.data_off) || !rd(f, &e.comp_size) || !rd(f, &e.size) || !rd(f, &e.status) || !rd(f, &method)) return 2;
      e.method = (uint16_t)method;
    }
    if (!rd(f, &has_sel) || !rd(f, &ns)) return 2;
    std::vector<uint32_t> sel(ns);
    for (auto &s : sel)
      if (!rd(f, &s)) return 2;
    if (!has_sel) ns = n;
    // the read's slots
    std::vector<uint64_t> out_off((size_t)ns + 1, 0);
    for (uint32_t j = 0; j < ns; ++j) {
      const flate_hip_zip_entry &e = ent[has_sel ? sel[j] : j];
      const bool ok = e.status == 0 && !zip_units_too_large(e.size, e.method, e.comp_size);
      out_off[j + 1] = out_off[j] + (ok ? e.size : 0);
    }
    std::vector<ZuEntry> L;
    std::vector<ZuRange> R;
    uint32_t fallback = 0;
    zip_units_form(ent.data(), n, has_sel ? sel.data() : nullptr, ns, out_off.data(), unit_min, L, R, &fallback);
    uint64_t lo = 0, hi = 0;
    if (!L.empty()) zip_units_hull(L, R, &lo, &hi);
    printf("%u %llu %llu |", fallback, (ull)lo, (ull)hi);
    for (const ZuEntry &e : L) printf(" %u,%llu,%llu,%llu,%llu", e.slot, (ull)e.lo, (ull)e.end, (ull)e.size, (ull)e.out);
    printf(" |");
    for (const ZuRange &r : R) printf(" %llu,%llu,%u", (ull)r.lo, (ull)r.end, r.entry);
    printf("\n");
  }
  return 0;
}

struct Probe {
  uint32_t ok, final_block;
  uint64_t end_bit, out;
};

static int chain(FILE *f) {
  uint32_t count = 0;
  if (!rd(f, &count)) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t na = 0, nb = 0;
    if (!rd(f, &na) || !rd(f, &nb) || nb == 0) return 2;
    const uint32_t n = na + nb;
    std::vector<uint64_t> cand(n);
    for (uint32_t i = 0; i < na; ++i)
      if (!rd(f, &cand[i])) return 2;
    std::vector<ZuEntry> L(nb);
    std::vector<ZuRange> R(nb);
    for (uint32_t i = 0; i < nb; ++i) {
      L[i] = ZuEntry{};
      if (!rd(f, &L[i].lo) || !rd(f, &L[i].end) || !rd(f, &L[i].size) || !rd(f, &L[i].out)) return 2;
      R[i] = ZuRange{L[i].lo, L[i].end, i, 0};
      cand[na + i] = 8u * L[i].lo;
    }
    std::sort(R.begin(), R.end(), [](const ZuRange &a, const ZuRange &b) { return a.lo < b.lo; });
    std::vector<Probe> pr(n);
    for (auto &p : pr)
      if (!rd(f, &p.ok) || !rd(f, &p.final_block) || !rd(f, &p.end_bit) || !rd(f, &p.out)) return 2;
    // the link of every node, as zip_units_link_kernel computes it
    std::vector<uint32_t> next(n);
    for (uint32_t c = 0; c < n; ++c) {
      uint32_t x = nb;
      if (c >= na) {
        x = c - na;
      } else {
        const uint32_t at = zip_units_owner(R.data(), nb, cand[c] >> 3);
        if (at < nb) x = R[at].entry;
      }
      next[c] = zip_units_next(cand.data(), na, nb, x, x < nb ? L[x].end : 0, pr[c].ok != 0, pr[c].final_block != 0, pr[c].end_bit);
      printf(" %u", next[c]);
    }
    printf(" |");
    // the path from the first B node (at most n nodes: nothing cycles, and the model refuses to go on if it did)
    std::vector<uint32_t> path;
    for (uint32_t c = na; c < n && path.size() <= n; c = next[c]) path.push_back(c);
    if (path.size() > n) return 4;
    const bool whole = next[path.back()] == n;
    const uint32_t nu = whole ? (uint32_t)path.size() : (uint32_t)path.size() - 1u;  // the good units
    // entries, slots, histories; g
    uint32_t g = 0, entry = 0;
    bool counting = true;
    uint64_t rel = 0;
    for (uint32_t r = 0; r < nu; ++r) {
      const uint32_t c = path[r];
      if (c >= na) entry = c - na, rel = 0;
      printf(" %u,%u,%llu,%u", c, entry, (ull)zip_units_slot(L[entry].out, rel), zip_units_history(rel));
      rel += pr[c].out;
      if (pr[c].final_block) {
        if (counting && zip_units_good(r + 1u, nu, true, rel, L[entry].size)) ++g;
        else counting = false;
      }
    }
    printf(" | %u\n", g);
  }
  return 0;
}

static int served(FILE *f) {
  uint32_t count = 0;
  if (!rd(f, &count)) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t g_disc = 0, bad = 0;
    if (!rd(f, &g_disc) || !rd(f, &bad)) return 2;
    std::vector<uint64_t> eu((size_t)g_disc + 1);
    for (auto &v : eu)
      if (!rd(f, &v)) return 2;
    printf("%u\n", zip_units_served(eu.data(), g_disc, bad));
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 2 && std::string(argv[1]) == "checks") {
    const int64_t vals[] = {-1, 0, 1, 2, 65536, (int64_t)1 << 40, INT64_MAX, INT64_MIN};
    for (int64_t v : vals) printf("%lld %d\n", (long long)v, zip_unit_min_ok(v) ? 1 : 0);
    return 0;
  }
  if (argc < 3) return 2;
  FILE *f = fopen(argv[2], "rb");
  if (!f) return 2;
  const std::string mode(argv[1]);
  const int rc = mode == "form" ? form(f) : mode == "chain" ? chain(f) : mode == "served" ? served(f) : 2;
  fclose(f);
  return rc;
}
