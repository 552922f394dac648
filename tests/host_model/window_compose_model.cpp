// window_compose_model.cpp -- the COMPOSE operator of flate_hip_inflate_one (moonbit-flate_amd/csrc/window_compose.h) as
// a stand-alone CPU program for tests/test_window_compose_model.py: the very functions the kernels compile, scanned as
// the kernels scan them (Hillis-Steele over a chain of tail functions, then resolved against a seed window) and held
// against a brute-force resolution, unit by unit.
//   window_compose_model SEED    one line per case: name ok|FAIL
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "window_compose.h"

using namespace flate;
typedef std::vector<uint16_t> Fn;

static Fn identity() {
  Fn f(kWinEntries);
  for (uint32_t j = 0; j < kWinEntries; ++j) f[j] = wc_identity(j);
  return f;
}
// a unit that writes `z` bytes: literals, and copies from up to 32768 bytes back (into the window in front too)
static Fn random_unit(std::mt19937 &rng, uint32_t z, bool literals_only) {
  std::vector<uint16_t> win(kWinEntries);
  for (uint32_t j = 0; j < kWinEntries; ++j) win[j] = wc_identity(j);
  for (uint32_t p = 0; p < z;) {
    if (literals_only || rng() % 3 == 0) {
      win[p++ & (kWinEntries - 1)] = (uint16_t)(rng() & 255);
    } else {
      const uint32_t len = 3 + rng() % 256, dist = 1 + rng() % kWinEntries;
      for (uint32_t i = 0; i < len && p < z; ++i, ++p) win[p & (kWinEntries - 1)] = win[(p - dist) & (kWinEntries - 1)];
    }
  }
  Fn t(kWinEntries);
  for (uint32_t j = 0; j < kWinEntries; ++j) t[j] = win[(z + j) & (kWinEntries - 1)];
  return t;
}

static bool chain(std::mt19937 &rng, uint32_t n, int kind) {
  std::vector<Fn> T(n);
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t z = kind == 1 ? 0 : kind == 2 ? kWinEntries + rng() % 1000 : (rng() % 4 ? rng() % 3000 : rng() % 70000);
    T[k] = kind == 1 ? identity() : random_unit(rng, z, kind == 2);
  }
  std::vector<uint8_t> seed(kWinEntries);
  for (auto &b : seed) b = (uint8_t)rng();
  // brute force: window by window
  std::vector<std::vector<uint8_t>> want(n + 1, std::vector<uint8_t>(kWinEntries));
  want[0] = seed;
  for (uint32_t k = 0; k < n; ++k)
    for (uint32_t j = 0; j < kWinEntries; ++j) want[k + 1][j] = wc_resolve(T[k][j], want[k].data());
  // the kernels' way: scan, then resolve every function against the seed
  std::vector<Fn> cur = T, nxt(n, Fn(kWinEntries));
  for (uint32_t s = 1; s < n; s <<= 1) {
    for (uint32_t k = 0; k < n; ++k)
      for (uint32_t j = 0; j < kWinEntries; ++j) nxt[k][j] = k >= s ? wc_compose(cur[k][j], cur[k - s].data()) : cur[k][j];
    cur.swap(nxt);
  }
  for (uint32_t k = 0; k < n; ++k)
    for (uint32_t j = 0; j < kWinEntries; ++j)
      if (wc_resolve(cur[k][j], seed.data()) != want[k + 1][j]) return false;
  if (kind == 1 && want[n] != seed) return false;                      // identities pass the seed through
  if (kind == 2 && n) {                                                // all literals: nothing of the seed is left
    std::vector<uint8_t> other(kWinEntries, 0x5a);
    for (uint32_t j = 0; j < kWinEntries; ++j)
      if (wc_resolve(cur[n - 1][j], other.data()) != want[n][j]) return false;
  }
  return true;
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::mt19937 rng((uint32_t)atoi(argv[1]));
  const uint32_t lens[] = {1, 2, 3, 64, 65};
  const char *kinds[] = {"random", "identity", "all_literal"};
  for (int kind = 0; kind < 3; ++kind)
    for (uint32_t n : lens) printf("%s_%u %s\n", kinds[kind], n, chain(rng, n, kind) ? "ok" : "FAIL");
  // associativity on three random functions: (A o B) o C == A o (B o C)
  Fn A = random_unit(rng, 5000, false), B = random_unit(rng, 100, false), C = random_unit(rng, 40000, false);
  Fn AB(kWinEntries), BC(kWinEntries);
  bool ok = true;
  for (uint32_t j = 0; j < kWinEntries; ++j) AB[j] = wc_compose(A[j], B.data()), BC[j] = wc_compose(B[j], C.data());
  for (uint32_t j = 0; j < kWinEntries; ++j) ok = ok && wc_compose(AB[j], C.data()) == wc_compose(A[j], BC.data());
  printf("associative %s\n", ok ? "ok" : "FAIL");
  return 0;
}
