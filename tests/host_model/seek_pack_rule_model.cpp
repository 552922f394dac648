// seek_pack_rule_model.cpp -- the packed windows' rule (moonbit-flate_amd/csrc/seek_pack_rule.h) and the argument checks
// of its three calls (api_checks.h) as a stand-alone CPU program: the very functions the kernels and the entry points
// compile, driven by tests/test_seek_pack_rule_model.py and compared there with tests/seek_pack_ref.py.
//   seek_pack_rule_model keep FILE  FILE = u32 count, then per case: u64 q, u32 len, u32 dist, u64 P0.  One line per
//                                   case: "lo hi" of seek_pack_keep
//   seek_pack_rule_model ok FILE    FILE = u32 count, then per case: u64 packed_bytes, u64 words, the pack index, u64
//                                   index words, the seek index.  One line per case: seek_pack_ok, seek_pack_self_ok
//   seek_pack_rule_model head FILE  FILE = u32 mode, u64 packed_bytes, u64 kept, u64 index words, the seek index.  One
//                                   line: the 16 words of seek_pack_head
//   seek_pack_rule_model checks     one line per argument-check call: name value
// Every array lies in an allocation of exactly its size: a read outside it is a heap overflow the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "api_checks.h"
#include "seek_pack_rule.h"

using namespace flate;

template <typename T>
static T *exact(size_t count) {
  return (T *)malloc(count ? count * sizeof(T) : 1);
}

static int keep_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t c = 0; c < count; ++c) {
    uint64_t q = 0, P0 = 0;
    uint32_t len = 0, dist = 0;
    if (fread(&q, 8, 1, f) != 1 || fread(&len, 4, 1, f) != 1 || fread(&dist, 4, 1, f) != 1 || fread(&P0, 8, 1, f) != 1) return 2;
    const SeekKeep k = seek_pack_keep(q, len, dist, P0);
    printf("%u %u\n", k.lo, k.hi);
  }
  fclose(f);
  return 0;
}

static int ok_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t c = 0; c < count; ++c) {
    uint64_t packed_bytes = 0, words = 0, iwords = 0;
    if (fread(&packed_bytes, 8, 1, f) != 1 || fread(&words, 8, 1, f) != 1) return 2;
    uint64_t *pack = exact<uint64_t>(words);
    if (words && fread(pack, 8, words, f) != words) return 2;
    if (fread(&iwords, 8, 1, f) != 1) return 2;
    uint64_t *index = exact<uint64_t>(iwords);
    if (iwords && fread(index, 8, iwords, f) != iwords) return 2;
    printf("%d %d\n", seek_pack_ok(pack, words, packed_bytes, index) ? 1 : 0, seek_pack_self_ok(pack, words, packed_bytes) ? 1 : 0);
    free(pack), free(index);
  }
  fclose(f);
  return 0;
}

static int head_file(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  uint32_t mode = 0;
  uint64_t packed_bytes = 0, kept = 0, iwords = 0;
  if (fread(&mode, 4, 1, f) != 1 || fread(&packed_bytes, 8, 1, f) != 1 || fread(&kept, 8, 1, f) != 1 || fread(&iwords, 8, 1, f) != 1)
    return 2;
  uint64_t *index = exact<uint64_t>(iwords);
  if (fread(index, 8, iwords, f) != iwords) return 2;
  uint64_t *head = exact<uint64_t>(kSeekPackHeadWords);
  seek_pack_head(head, index, mode, packed_bytes, kept);
  for (uint32_t k = 0; k < kSeekPackHeadWords; ++k) printf("%llu ", (unsigned long long)head[k]);
  printf("\n");
  free(index), free(head);
  fclose(f);
  return 0;
}

static int checks() {
  uint8_t b[4] = {0};
  uint64_t lo[2] = {1, 5}, hi[2] = {1, 9}, off[3] = {0, 0, 0}, w64 = 0, pk[32] = {0};
  const uint32_t D = FLATE_HIP_DEVICE_PTRS, CO = FLATE_HIP_SEEK_PACK_COMPRESS, SP = CO | FLATE_HIP_SEEK_PACK_SPARSE;
  // an index of one unit over a raw stream of 4 bytes, T = 10: one point, no block
  uint64_t one[kSeekHeadWords + 5] = {kSeekMagic, kSeekVersion, 0, 4, 0, 4, 10, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 32, 0, 10, 0};
  const uint64_t W = kSeekHeadWords + 5;
  uint64_t pack[kSeekPackHeadWords + 1];
  seek_pack_head(pack, one, CO, 0, 0);
  pack[kSeekPackHeadWords] = 0;
  const uint64_t PW = kSeekPackHeadWords + 1;
  printf("pack_ok %d\n", seek_pack_args(b, 4, 0, one, W, nullptr, 0, SP, pk, 32, &w64, b, 4, &w64, &w64, D));
  printf("pack_no_in_compress %d\n", seek_pack_args(nullptr, 4, 0, one, W, nullptr, 0, CO, pk, 32, &w64, b, 4, &w64, &w64, 0));
  printf("pack_query %d\n", seek_pack_args(b, 4, 0, one, W, nullptr, 0, SP, nullptr, 0, &w64, nullptr, 0, &w64, &w64, 0));
  printf("pack_no_in_sparse %d\n", seek_pack_args(nullptr, 4, 0, one, W, nullptr, 0, SP, pk, 32, &w64, b, 4, &w64, &w64, 0));
  printf("pack_mode_0 %d\n", seek_pack_args(b, 4, 0, one, W, nullptr, 0, 0, pk, 32, &w64, b, 4, &w64, &w64, 0));
  printf("pack_mode_sparse_alone %d\n", seek_pack_args(b, 4, 0, one, W, nullptr, 0, 2, pk, 32, &w64, b, 4, &w64, &w64, 0));
  printf("pack_mode_4 %d\n", seek_pack_args(b, 4, 0, one, W, nullptr, 0, 5, pk, 32, &w64, b, 4, &w64, &w64, 0));
  printf("pack_flag_go %d\n", seek_pack_args(b, 4, 0, one, W, nullptr, 0, SP, pk, 32, &w64, b, 4, &w64, &w64, FLATE_HIP_COMPAT_GO));
  printf("pack_wrap_3 %d\n", seek_pack_args(b, 4, 3, one, W, nullptr, 0, SP, pk, 32, &w64, b, 4, &w64, &w64, 0));
  printf("pack_wrap_not_the_index %d\n", seek_pack_args(b, 4, 1, one, W, nullptr, 0, SP, pk, 32, &w64, b, 4, &w64, &w64, 0));
  printf("pack_no_pack_words %d\n", seek_pack_args(b, 4, 0, one, W, nullptr, 0, SP, pk, 32, nullptr, b, 4, &w64, &w64, 0));
  printf("pack_no_packed_bytes %d\n", seek_pack_args(b, 4, 0, one, W, nullptr, 0, SP, pk, 32, &w64, b, 4, nullptr, &w64, 0));
  printf("pack_no_kept_bytes %d\n", seek_pack_args(b, 4, 0, one, W, nullptr, 0, SP, pk, 32, &w64, b, 4, &w64, nullptr, 0));
  printf("pack_no_pack_index_with_cap %d\n", seek_pack_args(b, 4, 0, one, W, nullptr, 0, SP, nullptr, 32, &w64, b, 4, &w64, &w64, 0));
  printf("pack_no_packed_with_cap %d\n", seek_pack_args(b, 4, 0, one, W, nullptr, 0, SP, pk, 32, &w64, nullptr, 4, &w64, &w64, 0));
  printf("pack_windows_without_buffer %d\n", seek_pack_args(b, 4, 0, one, W, nullptr, 32768, SP, pk, 32, &w64, b, 4, &w64, &w64, 0));
  printf("pack_no_index %d\n", seek_pack_args(b, 4, 0, nullptr, W, nullptr, 0, SP, pk, 32, &w64, b, 4, &w64, &w64, 0));
  printf("unpack_ok %d\n", seek_unpack_args(pack, PW, nullptr, 0, nullptr, 0, &w64, D));
  printf("unpack_no_windows_bytes %d\n", seek_unpack_args(pack, PW, nullptr, 0, nullptr, 0, nullptr, 0));
  printf("unpack_no_pack_index %d\n", seek_unpack_args(nullptr, PW, nullptr, 0, nullptr, 0, &w64, 0));
  printf("unpack_short_pack_index %d\n", seek_unpack_args(pack, PW - 1, nullptr, 0, nullptr, 0, &w64, 0));
  printf("unpack_no_windows_with_cap %d\n", seek_unpack_args(pack, PW, nullptr, 0, nullptr, 4, &w64, 0));
  printf("unpack_flag_size_only %d\n", seek_unpack_args(pack, PW, nullptr, 0, nullptr, 0, &w64, FLATE_HIP_SIZE_ONLY));
  printf("read_ok %d\n", one_ranges_packed_args(b, 4, 0, one, W, pack, PW, nullptr, 0, lo, hi, 2, b, 4, off, D));
  printf("read_size_query %d\n", one_ranges_packed_args(b, 4, 0, one, W, pack, PW, nullptr, 0, lo, hi, 2, nullptr, 0, off, 0));
  printf("read_no_index %d\n", one_ranges_packed_args(b, 4, 0, nullptr, W, pack, PW, nullptr, 0, lo, hi, 2, b, 4, off, 0));
  printf("read_no_pack_index %d\n", one_ranges_packed_args(b, 4, 0, one, W, nullptr, PW, nullptr, 0, lo, hi, 2, b, 4, off, 0));
  printf("read_backwards %d\n", one_ranges_packed_args(b, 4, 0, one, W, pack, PW, nullptr, 0, hi, lo, 2, b, 4, off, 0));
  printf("read_wrap_not_the_index %d\n", one_ranges_packed_args(b, 4, 1, one, W, pack, PW, nullptr, 0, lo, hi, 2, b, 4, off, 0));
  printf("read_packed_without_buffer %d\n", one_ranges_packed_args(b, 4, 0, one, W, pack, PW, nullptr, 8, lo, hi, 2, b, 4, off, 0));
  pack[kSeekPackBindAt + 1] = 11;  // T is not the index's
  printf("read_pack_of_another_index %d\n", one_ranges_packed_args(b, 4, 0, one, W, pack, PW, nullptr, 0, lo, hi, 2, b, 4, off, 0));
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "keep")) return keep_file(argv[2]);
  if (argc == 3 && !strcmp(argv[1], "ok")) return ok_file(argv[2]);
  if (argc == 3 && !strcmp(argv[1], "head")) return head_file(argv[2]);
  if (argc == 2 && !strcmp(argv[1], "checks")) return checks();
  fprintf(stderr, "usage: %s keep FILE | ok FILE | head FILE | checks\n", argv[0]);
  return 2;
}
