// api_checks_model.cpp -- moonbit-flate_amd/csrc/api_checks.h and the container constants of flate_kernels.h behind a
// C interface (tests/test_api_checks.py).  Built with -DAPI_CHECKS_MODEL_MAIN it is a program of its own that runs
// the test's table (for a sanitizer build).
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "api_checks.h"
#include "flate_kernels.h"

using namespace flate;

extern "C" int m_ptrs_ok(const uint8_t *in, const uint64_t *in_off, uint32_t n, const uint8_t *out,
                         const uint64_t *out_off, const uint64_t *out_len, const int32_t *status,
                         const int64_t *err_off, uint32_t flags) {
  return inflate_batch_ptrs_ok(in, in_off, n, out, out_off, out_len, status, err_off, flags) ? 1 : 0;
}
extern "C" int m_ranges(const uint64_t *in_off, uint32_t n, const uint64_t *out_off, uint32_t flags) {
  return inflate_batch_ranges(in_off, n, out_off, flags);
}
extern "C" int m_deflate_batch_ptrs_ok(const uint8_t *in, const uint64_t *in_off, uint32_t n, const uint8_t *out,
                                       const uint64_t *out_off) {
  return deflate_batch_ptrs_ok(in, in_off, n, out, out_off) ? 1 : 0;
}
extern "C" int m_deflate_spliced_ptrs_ok(const uint8_t *in, const uint64_t *in_off, uint32_t n, const uint8_t *out,
                                         const uint64_t *out_len) {
  return deflate_spliced_ptrs_ok(in, in_off, n, out, out_len) ? 1 : 0;
}
extern "C" int m_dict_table_ok(const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts) {
  return dict_table_ok(dicts, dict_off, n_dicts) ? 1 : 0;
}
extern "C" int m_dict_args_ok(const uint8_t *dicts, const uint64_t *dict_off, uint32_t n_dicts, const uint32_t *dict_of,
                              uint32_t n) {
  return dict_args_ok(dicts, dict_off, n_dicts, dict_of, n) ? 1 : 0;
}
extern "C" int m_spliced_index_check(const uint64_t *bit_off, uint32_t n, const uint64_t *out_off, uint64_t in_len,
                                     uint64_t frame_bytes) {
  return spliced_index_check(bit_off, n, out_off, in_len, frame_bytes);
}
extern "C" int m_is_stream_status(int rc) { return is_stream_status(rc) ? 1 : 0; }
// out = {header without / with a dictionary, trailer, shortest member, checksum kind}
extern "C" void m_frame_constants(uint32_t wrap, uint32_t out[5]) {
  out[0] = frame_header_len(wrap, false), out[1] = frame_header_len(wrap, true), out[2] = frame_trailer_len(wrap);
  out[3] = frame_min_len(wrap), out[4] = frame_sum_kind(wrap);
}

#ifdef API_CHECKS_MODEL_MAIN
static long g_cases = 0, g_bad = 0;
static void want(int got, int expected, const char *what) {
  ++g_cases;
  if (got != expected) ++g_bad, printf("FAIL %s: %d, expected %d\n", what, got, expected);
}
int main() {
  const int INV = FLATE_HIP_E_INVALID, BIG = FLATE_HIP_E_TOO_LARGE;
  const uint8_t byte = 0;
  const uint64_t len1 = 0;
  const int32_t st1 = 0;
  const int64_t eo1 = 0;
  {  // inflate_batch_ptrs_ok / inflate_batch_ranges
    const uint64_t up[3] = {0, 5, 9}, down[3] = {0, 5, 4};
    want(m_ptrs_ok(&byte, up, 2, &byte, up, &len1, &st1, &eo1, 0), 1, "ptrs ok");
    want(m_ptrs_ok(&byte, up, 2, nullptr, up, &len1, &st1, &eo1, 0), 0, "ptrs: no out");
    want(m_ptrs_ok(&byte, up, 2, &byte, nullptr, &len1, &st1, &eo1, 0), 0, "ptrs: no out_off");
    want(m_ptrs_ok(&byte, up, 2, nullptr, nullptr, &len1, &st1, &eo1, FLATE_HIP_SIZE_ONLY), 1, "ptrs: size-only");
    want(m_ptrs_ok(nullptr, up, 0, nullptr, up, &len1, &st1, &eo1, 0), 1, "ptrs: n = 0");
    want(m_ptrs_ok(nullptr, nullptr, 0, nullptr, up, &len1, &st1, &eo1, 0), 0, "ptrs: n = 0, no in_off");
    want(m_ranges(up, 2, up, 0), 0, "ranges ok");
    want(m_ranges(down, 2, up, 0), INV, "ranges: in_off descends");
    want(m_ranges(up, 2, down, 0), INV, "ranges: out_off descends");
    want(m_ranges(up, 2, nullptr, FLATE_HIP_SIZE_ONLY), 0, "ranges: size-only");
    want(m_ranges(up, 0, up, 0), 0, "ranges: n = 0");
    const uint64_t big[3] = {7, 7 + 0x7ffe0000ull, 7 + 0x7ffe0000ull}, fits[3] = {7, 7 + 0x7ffdffffull, 7 + 0x7ffdffffull};
    want(m_ranges(big, 2, up, 0), BIG, "ranges: 0x7ffe0000 bytes");
    want(m_ranges(fits, 2, up, 0), 0, "ranges: one byte less");
    const uint64_t big_down[3] = {0, 0x7ffe0000ull, 1};
    want(m_ranges(big_down, 2, up, 0), INV, "ranges: descending wins over too large");
  }
  for (uint32_t n : {0u, 2u}) {  // the encode calls' pointers: every one missing in turn, without and with streams
    const uint64_t up[3] = {0, 5, 9};
    want(m_deflate_batch_ptrs_ok(&byte, up, n, &byte, up), 1, "deflate batch ptrs ok");
    want(m_deflate_batch_ptrs_ok(nullptr, up, n, &byte, up), n ? 0 : 1, "deflate batch: no in");
    want(m_deflate_batch_ptrs_ok(&byte, nullptr, n, &byte, up), 0, "deflate batch: no in_off");
    want(m_deflate_batch_ptrs_ok(&byte, up, n, nullptr, up), n ? 0 : 1, "deflate batch: no out");
    want(m_deflate_batch_ptrs_ok(&byte, up, n, &byte, nullptr), 0, "deflate batch: no out_off");
    want(m_deflate_spliced_ptrs_ok(&byte, up, n, &byte, &len1), 1, "deflate spliced ptrs ok");
    want(m_deflate_spliced_ptrs_ok(nullptr, up, n, &byte, &len1), n ? 0 : 1, "deflate spliced: no in");
    want(m_deflate_spliced_ptrs_ok(&byte, nullptr, n, &byte, &len1), 0, "deflate spliced: no in_off");
    want(m_deflate_spliced_ptrs_ok(&byte, up, n, nullptr, &len1), 0, "deflate spliced: no out (the closing block needs it)");
    want(m_deflate_spliced_ptrs_ok(&byte, up, n, &byte, nullptr), 0, "deflate spliced: no out_len");
  }
  {  // dictionary tables
    const uint64_t up[3] = {4, 10, 10}, down[3] = {4, 10, 9}, empty[3] = {4, 4, 4};
    const uint32_t of_ok[3] = {0, FLATE_HIP_NO_DICT, 1}, of_bad[3] = {0, 2, 1};
    want(m_dict_table_ok(&byte, up, 2), 1, "table ok");
    want(m_dict_table_ok(&byte, down, 2), 0, "table: descends");
    want(m_dict_table_ok(&byte, nullptr, 2), 0, "table: no dict_off");
    want(m_dict_table_ok(nullptr, up, 2), 0, "table: no dicts");
    want(m_dict_table_ok(nullptr, empty, 2), 1, "table: empty dictionaries need no dicts");
    want(m_dict_table_ok(nullptr, nullptr, 0), 1, "table: none");
    want(m_dict_args_ok(&byte, up, 2, of_ok, 3), 1, "args ok");
    want(m_dict_args_ok(&byte, up, 2, nullptr, 3), 1, "args: every stream uses dictionary 0");
    want(m_dict_args_ok(&byte, down, 2, of_ok, 3), 0, "args: descends");
    want(m_dict_args_ok(&byte, nullptr, 2, of_ok, 3), 0, "args: no dict_off");
    want(m_dict_args_ok(nullptr, up, 2, of_ok, 3), 0, "args: no dicts");
    want(m_dict_args_ok(&byte, up, 2, of_bad, 3), 0, "args: dict_of out of range");
    want(m_dict_args_ok(nullptr, nullptr, 0, nullptr, 3), 0, "args: nothing at all");
    const uint32_t none[3] = {FLATE_HIP_NO_DICT, FLATE_HIP_NO_DICT, FLATE_HIP_NO_DICT};
    want(m_dict_args_ok(nullptr, nullptr, 0, none, 3), 1, "args: NO_DICT throughout");
  }
  for (uint32_t wrap : {FLATE_HIP_WRAP_RAW, FLATE_HIP_WRAP_ZLIB, FLATE_HIP_WRAP_GZIP}) {  // spliced indices
    uint32_t k[5];
    m_frame_constants(wrap, k);
    const uint64_t frame = wrap == FLATE_HIP_WRAP_RAW ? 0 : k[3], in_len = frame + 100;
    const uint64_t slots[3] = {0, 10, 20}, slots_down[3] = {0, 10, 9};
    const uint64_t ok[3] = {0, 300, 800}, down[3] = {0, 300, 299}, past[3] = {0, 300, 801};
    want(m_spliced_index_check(ok, 2, slots, in_len, frame), 0, "index ok (ends at the last bit)");
    want(m_spliced_index_check(down, 2, slots, in_len, frame), INV, "index: descends");
    want(m_spliced_index_check(ok, 2, slots_down, in_len, frame), INV, "index: out_off descends");
    want(m_spliced_index_check(past, 2, slots, in_len, frame), INV, "index: one bit past");
    if (frame) want(m_spliced_index_check(ok, 2, slots, frame - 1, frame), INV, "index: in_len below the shortest member");
    if (frame) want(m_spliced_index_check(ok, 2, slots, frame, frame), INV, "index: nothing left behind the frame");
    const uint64_t piece[3] = {5, 5 + (1ull << 30), 5 + (1ull << 30)}, less[3] = {5, 4 + (1ull << 30), 4 + (1ull << 30)};
    want(m_spliced_index_check(piece, 2, slots, frame + (1ull << 28), frame), BIG, "index: a piece of 2^30 bits");
    want(m_spliced_index_check(less, 2, slots, frame + (1ull << 28), frame), 0, "index: one bit less");
  }
  for (int rc = -9; rc <= 1; ++rc)
    want(m_is_stream_status(rc), rc == 0 || rc == FLATE_HIP_E_OUT_TOO_SMALL || rc == FLATE_HIP_E_CORRUPT ||
                                     rc == FLATE_HIP_E_UNEXPECTED_EOF, "is_stream_status");
  {
    uint32_t z[5], g[5];
    m_frame_constants(FLATE_HIP_WRAP_ZLIB, z);
    m_frame_constants(FLATE_HIP_WRAP_GZIP, g);
    want(z[0] == 2 && z[1] == 6 && z[2] == 4 && z[3] == 6 && z[4] == FLATE_HIP_CHECKSUM_ADLER32, 1, "zlib constants");
    want(g[0] == 10 && g[1] == 10 && g[2] == 8 && g[3] == 18 && g[4] == FLATE_HIP_CHECKSUM_CRC32, 1, "gzip constants");
  }
  printf("api_checks: %ld cases, %ld bad\n", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
#endif
