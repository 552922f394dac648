// zip_rule_model.cpp -- the ZIP rule (moonbit-flate_amd/csrc/zip_rule.h) and the ZIP argument checks (api_checks.h)
// as a stand-alone CPU program: the very functions the kernels and the entry points compile, driven by
// tests/test_zip_rule_model.py and compared there with tests/zip_ref.py and Python's zipfile.
//   zip_rule_model index FILE      FILE = u32 count, then per case u64 length + bytes.  One line per case:
//                                  rc n_entries err_off | end_off rec_off n cd_off cd_size zip64 | the entries, each
//                                  name_off,header_off,data_off,comp_size,size,crc32,name_len,method,flags,status
//   zip_rule_model write FILE OUT  FILE = u32 n, then per entry u32 crc, u64 size, u64 name length + name, u64 raw
//                                  length + raw stream.  OUT receives the archive; prints the n + 1 entry offsets
//   zip_rule_model places FILE     FILE = u32 n, u64 the first header's offset (synthetic: 0 in an archive), then per entry
//                                  u64 member size, u32 name length (sizes only).  Prints k0, the closed-form place of
//                                  every central record, the directory's size and the end records' length
//   zip_rule_model checks          one line per argument-check call: name value
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "api_checks.h"
#include "zip_rule.h"

using namespace flate;

static size_t bound_model(size_t n) { return 2 * n + 400; }

template <typename T>
static bool rd(FILE *f, T *v) { return fread(v, sizeof(T), 1, f) == 1; }

static int index_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (!rd(f, &count)) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint64_t len = 0;
    if (!rd(f, &len)) return 2;
    // (an exact allocation: a read past in_len is a heap overflow the sanitizer reports)
    uint8_t *buf = (uint8_t *)malloc(len ? len : 1);
    if (len && fread(buf, 1, len, f) != len) return 2;
    ZipEnd E;
    uint64_t n = 0;
    int64_t err = -1;
    // the count first (the end record's n may promise more than the directory holds), then the entries
    int rc = zip_serial_index(buf, len, &E, nullptr, &n, &err);
    std::vector<flate_hip_zip_entry> ent(n + 1);
    if (n) {
      // (the walk over the well-formed records in front of err_off, with room for exactly those)
      ZipEnd E2 = E;
      uint64_t n2 = 0;
      int64_t err2 = -1;
      std::vector<flate_hip_zip_entry> all(E.n < len / 46 + 1 ? E.n : len / 46 + 1);
      const int rc2 = zip_serial_index(buf, len, &E2, all.data(), &n2, &err2);
      if (rc2 != rc || n2 != n || err2 != err) return 3;
      for (uint64_t i = 0; i < n; ++i) ent[i] = all[i];
    }
    printf("%d %llu %lld |", rc, (unsigned long long)n, (long long)err);
    ZipEnd E3;
    const int64_t p = zip_find_end(buf, len);
    if (p >= 0 && zip_end_read(buf, len, (uint64_t)p, &E3) == 0)
      printf(" %llu %llu %llu %llu %llu %u", (unsigned long long)E.end_off, (unsigned long long)E.rec_off, (unsigned long long)E.n,
             (unsigned long long)E.cd_off, (unsigned long long)E.cd_size, E.zip64);
    printf(" |");
    for (uint64_t i = 0; i < n; ++i) {
      const flate_hip_zip_entry &e = ent[i];
      printf(" %llu,%llu,%llu,%llu,%llu,%u,%u,%u,%u,%d", (unsigned long long)e.name_off, (unsigned long long)e.header_off,
             (unsigned long long)e.data_off, (unsigned long long)e.comp_size, (unsigned long long)e.size, e.crc32, e.name_len,
             e.method, e.flags, e.status);
    }
    printf("\n");
    free(buf);
  }
  fclose(f);
  return 0;
}

static int write_file(const char *path, const char *out_path) {
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t n = 0;
  if (!rd(f, &n)) return 2;
  std::vector<uint32_t> crc(n);
  std::vector<uint64_t> size(n), name_off(n + 1, 0), raw_off(n + 1, 0);
  std::vector<uint8_t> names, raw;
  for (uint32_t i = 0; i < n; ++i) {
    uint64_t nl = 0, rl = 0;
    if (!rd(f, &crc[i]) || !rd(f, &size[i]) || !rd(f, &nl)) return 2;
    names.resize(names.size() + nl);
    if (nl && fread(names.data() + name_off[i], 1, nl, f) != nl) return 2;
    name_off[i + 1] = name_off[i] + nl;
    if (!rd(f, &rl)) return 2;
    raw.resize(raw.size() + rl);
    if (rl && fread(raw.data() + raw_off[i], 1, rl, f) != rl) return 2;
    raw_off[i + 1] = raw_off[i] + rl;
  }
  fclose(f);
  const uint64_t total = zip_serial_size(raw_off.data(), name_off.data(), n);
  uint8_t *out = (uint8_t *)malloc(total);  // (exact: the writer may not pass its own size)
  std::vector<uint64_t> entry_off(n + 1);
  const uint64_t wrote = zip_serial_write(raw.data(), raw_off.data(), crc.data(), size.data(), names.data(), name_off.data(), n, out,
                                          entry_off.data());
  if (wrote != total) return 3;
  FILE *o = fopen(out_path, "wb");
  if (!o || fwrite(out, 1, total, o) != total) return 2;
  fclose(o);
  free(out);
  for (uint32_t i = 0; i <= n; ++i) printf("%llu\n", (unsigned long long)entry_off[i]);
  return 0;
}

static int places_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t n = 0;
  uint64_t base = 0;
  if (!rd(f, &n) || !rd(f, &base)) return 2;
  std::vector<uint64_t> member(n), names_before(n + 1, 0);
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t nl = 0;
    if (!rd(f, &member[i]) || !rd(f, &nl)) return 2;
    names_before[i + 1] = names_before[i] + nl;
  }
  fclose(f);
  uint64_t off = base, k0 = n;
  for (uint32_t i = 0; i < n; ++i) {
    if (k0 == n && zip_central_has_extra(off)) k0 = i;
    off += member[i];
  }
  printf("%llu\n", (unsigned long long)k0);
  for (uint32_t i = 0; i <= n; ++i) printf("%llu\n", (unsigned long long)zip_central_place(i, names_before[i], k0));
  printf("%u\n", zip_end_len(n, off, zip_central_place(n, names_before[n], k0)));
  return 0;
}

static int checks() {
  uint8_t b[8] = {0};
  uint64_t w = 0;
  uint32_t n = 0, s[2] = {0, 0};
  int32_t st = 0;
  int64_t eo = 0;
  const uint64_t io[3] = {0, 4, 4}, no[3] = {0, 1, 3}, no_empty[3] = {0, 1, 1}, no_back[3] = {2, 1, 3}, no_long[2] = {0, 65536},
                 no_max[2] = {0, 65535}, io_back[3] = {4, 0, 4};
  const uint32_t D = FLATE_HIP_DEVICE_PTRS, G = FLATE_HIP_COMPAT_GO;
  printf("write_ok %d\n", zip_write_args(b, io, 2, b, no, b, &w, D | G));
  printf("write_n0_ok %d\n", zip_write_args(nullptr, io, 0, nullptr, no, b, &w, 0));
  printf("write_name_max_ok %d\n", zip_write_args(b, io, 1, b, no_max, b, &w, 0));
  printf("write_name_empty %d\n", zip_write_args(b, io, 2, b, no_empty, b, &w, 0));
  printf("write_name_long %d\n", zip_write_args(b, io, 1, b, no_long, b, &w, 0));
  printf("write_name_off_back %d\n", zip_write_args(b, io, 2, b, no_back, b, &w, 0));
  printf("write_in_off_back %d\n", zip_write_args(b, io_back, 2, b, no, b, &w, 0));
  printf("write_no_in %d\n", zip_write_args(nullptr, io, 2, b, no, b, &w, 0));
  printf("write_no_in_off %d\n", zip_write_args(b, nullptr, 2, b, no, b, &w, 0));
  printf("write_no_names %d\n", zip_write_args(b, io, 2, nullptr, no, b, &w, 0));
  printf("write_no_name_off %d\n", zip_write_args(b, io, 2, b, nullptr, b, &w, 0));
  printf("write_no_out %d\n", zip_write_args(b, io, 2, b, no, nullptr, &w, 0));
  printf("write_no_len %d\n", zip_write_args(b, io, 2, b, no, b, nullptr, 0));
  printf("write_flag_size_only %d\n", zip_write_args(b, io, 2, b, no, b, &w, FLATE_HIP_SIZE_ONLY));
  printf("bound_0 %llu\n", (unsigned long long)zip_archive_bound(io, 0, no, bound_model));
  printf("bound_2 %llu\n", (unsigned long long)zip_archive_bound(io, 2, no, bound_model));
  printf("bound_refused %llu\n", (unsigned long long)zip_archive_bound(io, 2, no_empty, bound_model));
  printf("index_ok %d\n", zip_index_args(b, 4, b, &w, &n, &w, D));
  printf("index_query_ok %d\n", zip_index_args(b, 4, nullptr, nullptr, &n, &w, 0));
  printf("index_one_array %d\n", zip_index_args(b, 4, b, nullptr, &n, &w, 0));
  printf("index_other_array %d\n", zip_index_args(b, 4, nullptr, &w, &n, &w, 0));
  printf("index_no_count %d\n", zip_index_args(b, 4, b, &w, nullptr, &w, 0));
  printf("index_no_bytes %d\n", zip_index_args(b, 4, b, &w, &n, nullptr, 0));
  printf("index_no_in %d\n", zip_index_args(nullptr, 4, b, &w, &n, &w, 0));
  printf("index_flag_go %d\n", zip_index_args(b, 4, b, &w, &n, &w, G));
  printf("read_ok %d\n", zip_read_args(b, 4, s, 2, 2, b, 4, &w, &w, &st, &eo, D));
  printf("read_all_ok %d\n", zip_read_args(b, 4, nullptr, 0, 2, b, 4, &w, &w, &st, &eo, 0));
  printf("read_query_ok %d\n", zip_read_args(b, 4, nullptr, 0, 2, nullptr, 0, &w, &w, &st, &eo, 0));
  printf("read_sel_over_cap %d\n", zip_read_args(b, 4, s, 2, 1, b, 4, &w, &w, &st, &eo, 0));
  printf("read_count_without_sel %d\n", zip_read_args(b, 4, nullptr, 2, 2, b, 4, &w, &w, &st, &eo, 0));
  printf("read_no_out %d\n", zip_read_args(b, 4, s, 2, 2, nullptr, 4, &w, &w, &st, &eo, 0));
  printf("read_no_out_off %d\n", zip_read_args(b, 4, s, 2, 2, b, 4, nullptr, &w, &st, &eo, 0));
  printf("read_no_len %d\n", zip_read_args(b, 4, s, 2, 2, b, 4, &w, nullptr, &st, &eo, 0));
  printf("read_no_status %d\n", zip_read_args(b, 4, s, 2, 2, b, 4, &w, &w, nullptr, &eo, 0));
  printf("read_no_err_off %d\n", zip_read_args(b, 4, s, 2, 2, b, 4, &w, &w, &st, nullptr, 0));
  printf("read_no_in %d\n", zip_read_args(nullptr, 4, s, 2, 2, b, 4, &w, &w, &st, &eo, 0));
  printf("read_flag_size_only %d\n", zip_read_args(b, 4, s, 2, 2, b, 4, &w, &w, &st, &eo, FLATE_HIP_SIZE_ONLY));
  printf("first_cap_small %u\n", zip_first_cap(3, 200));
  printf("first_cap_many %u\n", zip_first_cap(70000, 70000ull * 52));
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "index")) return index_file(argv[2]);
  if (argc == 4 && !strcmp(argv[1], "write")) return write_file(argv[2], argv[3]);
  if (argc == 3 && !strcmp(argv[1], "places")) return places_file(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
  fprintf(stderr, "usage: %s index FILE | write FILE OUT | places FILE | checks\n", argv[0]);
  return 2;
}
