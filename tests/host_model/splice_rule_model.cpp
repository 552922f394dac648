// splice_rule_model.cpp -- moonbit-flate_amd/csrc/splice_rule.h (and the grouped call's checks of api_checks.h) as a
// stand-alone program for tests/test_splice_rule_model.py, built under AddressSanitizer and UBSan: every array lives in
// an allocation of exactly its size.
//   place FILE   cases {n_pieces, n_groups, trailer, has_hdr, hdr_all : u32; sum : u64[2n]; group_off : u32[g+1];
//                hdr : u32[g] if has_hdr} -> "total|piece_bit...|end_bit...|payload_off...|member_off..." per case
//   assoc FILE   {f.a f.b g.a g.b h.a h.b x : u64} -> "(fg)h.a (fg)h.b f(gh).a f(gh).b h(g(f(x))) ((fg)h)(x)" per triple
//   args FILE    {n_groups, n_pieces : u32; group_off : u32[g+1]} -> grouped_args_ok per case
//   plan FILE    {n : u32; P : u64; in_off : u64[n+1]} -> "count longs|piece_in_off...|group_off..." per case
//   api          the refusals of deflate_grouped_args, one return code per line
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "api_checks.h"
#include "splice_rule.h"

using namespace flate;

namespace {

struct Reader {
  std::vector<uint8_t> buf;
  size_t at = 0;
  explicit Reader(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) {
      perror(path);
      exit(2);
    }
    fseek(f, 0, SEEK_END);
    buf.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (!buf.empty() && fread(buf.data(), 1, buf.size(), f) != buf.size()) exit(2);
    fclose(f);
  }
  template <typename T>
  T get() {
    T v;
    if (at + sizeof(T) > buf.size()) exit(3);
    memcpy(&v, buf.data() + at, sizeof(T));
    at += sizeof(T);
    return v;
  }
  // an allocation of exactly count entries (never a vector with spare capacity)
  template <typename T>
  std::unique_ptr<T[]> array(size_t count) {
    std::unique_ptr<T[]> p(new T[count]);
    for (size_t i = 0; i < count; ++i) p[i] = get<T>();
    return p;
  }
  bool more() const { return at < buf.size(); }
};

void row(const char *sep, const uint64_t *v, size_t n) {
  fputs(sep, stdout);
  for (size_t i = 0; i < n; ++i) printf(i ? " %llu" : "%llu", (unsigned long long)v[i]);
}

int place(const char *path) {
  Reader r(path);
  while (r.more()) {
    const uint32_t n = r.get<uint32_t>(), g = r.get<uint32_t>(), tl = r.get<uint32_t>(), has = r.get<uint32_t>(),
                   all = r.get<uint32_t>();
    auto sum = r.array<uint64_t>(2 * (size_t)n);
    auto goff = r.array<uint32_t>((size_t)g + 1);
    auto hdr = r.array<uint32_t>(has ? g : 0);
    std::unique_ptr<uint64_t[]> bit(new uint64_t[n]), end(new uint64_t[g]), pay(new uint64_t[g]), mem(new uint64_t[(size_t)g + 1]);
    const uint64_t total = grouped_place(sum.get(), n, goff.get(), g, has ? hdr.get() : nullptr, all, tl, bit.get(), end.get(),
                                         pay.get(), mem.get());
    printf("%llu", (unsigned long long)total);
    row("|", bit.get(), n), row("|", end.get(), g), row("|", pay.get(), g), row("|", mem.get(), (size_t)g + 1);
    putchar('\n');
  }
  return 0;
}

int assoc(const char *path) {
  Reader r(path);
  while (r.more()) {
    PosMap f{r.get<uint64_t>(), r.get<uint64_t>()}, g{r.get<uint64_t>(), r.get<uint64_t>()}, h{r.get<uint64_t>(), r.get<uint64_t>()};
    const uint64_t x = r.get<uint64_t>();
    const PosMap l = then(then(f, g), h), m = then(f, then(g, h));
    printf("%llu %llu %llu %llu %llu %llu\n", (unsigned long long)l.a, (unsigned long long)l.b, (unsigned long long)m.a,
           (unsigned long long)m.b, (unsigned long long)apply(h, apply(g, apply(f, x))), (unsigned long long)apply(l, x));
  }
  return 0;
}

int args(const char *path) {
  Reader r(path);
  while (r.more()) {
    const uint32_t g = r.get<uint32_t>(), n = r.get<uint32_t>();
    auto goff = r.array<uint32_t>((size_t)g + 1);
    printf("%d\n", grouped_args_ok(goff.get(), g, n) ? 1 : 0);
  }
  return 0;
}

int plan(const char *path) {
  Reader r(path);
  while (r.more()) {
    const uint32_t n = r.get<uint32_t>();
    const uint64_t P = r.get<uint64_t>();
    auto in_off = r.array<uint64_t>((size_t)n + 1);
    uint32_t longs = 0;
    const uint64_t count = zip_pieces_count(in_off.get(), n, P, &longs);
    std::unique_ptr<uint64_t[]> pin(new uint64_t[count + 1]);
    std::unique_ptr<uint32_t[]> goff(new uint32_t[(size_t)n + 1]);
    zip_pieces_plan(in_off.get(), n, P, pin.get(), goff.get());
    printf("%llu %u", (unsigned long long)count, longs);
    row("|", pin.get(), count + 1);
    fputs("|", stdout);
    for (uint32_t i = 0; i <= n; ++i) printf(i ? " %u" : "%u", goff[i]);
    putchar('\n');
  }
  return 0;
}

int api() {
  const uint8_t in[8] = {0}, out[8] = {0};
  const uint64_t in_off[4] = {0, 2, 2, 8}, back[4] = {0, 5, 2, 8}, out_off[3] = {0};
  const uint32_t ok[3] = {0, 1, 3}, flat[3] = {0, 1, 1}, down[3] = {0, 2, 1}, first[3] = {1, 2, 3}, last[3] = {0, 1, 2},
                 none[1] = {0};
  const uint32_t Z = FLATE_HIP_WRAP_ZLIB;
  const int rcs[] = {
      deflate_grouped_args(in, in_off, 3, ok, 2, Z, out, out_off, 0),
      deflate_grouped_args(in, in_off, 3, ok, 2, FLATE_HIP_WRAP_RAW, out, out_off, FLATE_HIP_DEVICE_PTRS | FLATE_HIP_COMPAT_GO),
      deflate_grouped_args(in, in_off, 3, ok, 2, FLATE_HIP_WRAP_GZIP, out, out_off, 0),
      deflate_grouped_args(nullptr, in_off, 0, none, 0, Z, nullptr, out_off, 0),  // no groups: nothing else is needed
      deflate_grouped_args(in, in_off, 3, flat, 2, Z, out, out_off, 0),           // an empty group
      deflate_grouped_args(in, in_off, 3, down, 2, Z, out, out_off, 0),           // not increasing
      deflate_grouped_args(in, in_off, 3, first, 2, Z, out, out_off, 0),          // does not start at 0
      deflate_grouped_args(in, in_off, 3, last, 2, Z, out, out_off, 0),           // does not end at n_pieces
      deflate_grouped_args(in, in_off, 3, ok, 2, 3, out, out_off, 0),             // an unknown wrap
      deflate_grouped_args(in, in_off, 3, ok, 2, Z, out, out_off, FLATE_HIP_LZ_SERIAL),
      deflate_grouped_args(nullptr, in_off, 3, ok, 2, Z, out, out_off, 0),
      deflate_grouped_args(in, nullptr, 3, ok, 2, Z, out, out_off, 0),
      deflate_grouped_args(in, in_off, 3, nullptr, 2, Z, out, out_off, 0),
      deflate_grouped_args(in, in_off, 3, ok, 2, Z, nullptr, out_off, 0),
      deflate_grouped_args(in, in_off, 3, ok, 2, Z, out, nullptr, 0),
      deflate_grouped_args(in, back, 3, ok, 2, Z, out, out_off, 0),               // a piece that runs backwards
      deflate_grouped_args(in, in_off, 1, none, 0, Z, out, out_off, 0),           // pieces without a group
  };
  for (int rc : rcs) printf("%d\n", rc);
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "api") return api();
  if (argc < 3) return 2;
  if (mode == "place") return place(argv[2]);
  if (mode == "assoc") return assoc(argv[2]);
  if (mode == "args") return args(argv[2]);
  if (mode == "plan") return plan(argv[2]);
  return 2;
}
