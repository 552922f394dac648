// one_writer_rule_model.cpp -- the rule of ONE stream written in parts (csrc/one_writer_rule.h, and api_checks.h's
// one_writer_*_check), driven from a command file so that tests/test_one_writer_rule_model.py can hold every decision
// against tests/one_writer_ref.py.  A stand-alone program: it is built once plainly and once with AddressSanitizer and
// UBSan, and run as this program only.
//
//   run <file>: one command per line, one line of output each
//     N wrap P                      a fresh writer                          -> "ok"
//     W in_len final out_cap span   one call; span = the bits the pieces it consumes take (what the scan adds)
//                                   -> "rc in_used out_len n_pieces header close start_bit carry"
//                                      (carry: the handle's bits behind the call; a call that launches nothing, or
//                                      that does not fit, leaves the state alone)
//     E end_bit close wrap out_cap  one_writer_end                          -> "whole carry fits"
//     B in_len P                    one_writer_bound                        -> "bound"
//     O ctx wrap P flags writer     one_writer_open_check (ctx, writer: 0 = NULL)    -> "rc"
//     A w in in_len out out_cap used len np   one_writer_write_check (0 = NULL)      -> "rc"
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "api_checks.h"

using namespace flate;

int main(int argc, char **argv) {
  if (argc != 3 || strcmp(argv[1], "run") != 0) return 2;
  FILE *f = fopen(argv[2], "r");
  if (!f) return 2;
  OneWriterHost s = one_writer_fresh();
  uint32_t wrap = 0;
  uint64_t P = 0;
  char line[512];
  static uint8_t some[8];
  static uint64_t word;
  static uint32_t word32;
  while (fgets(line, sizeof line, f)) {
    unsigned long long a = 0, b = 0, c = 0, d = 0, e = 0, g = 0, h = 0, i = 0;
    if (line[0] == 'N' && sscanf(line + 1, "%llu %llu", &a, &b) == 2) {
      s = one_writer_fresh(), wrap = (uint32_t)a, P = b;
      printf("ok\n");
    } else if (line[0] == 'W' && sscanf(line + 1, "%llu %llu %llu %llu", &a, &b, &c, &d) == 4) {
      const OneWriterPlan p = one_writer_plan(s, a, b != 0, P, wrap);
      if (p.action == kWriterReturn) {
        printf("%d 0 0 0 0 0 0 %u\n", p.status, s.carry_bits);
      } else if (p.action == kWriterNothing) {
        printf("0 0 0 0 0 0 0 %u\n", s.carry_bits);
      } else {
        const OneWriterEnd end = one_writer_end(p.start_bit + d, p.close != 0u, wrap, c);
        int rc = kWriterOutTooSmall;
        if (end.fits) {
          rc = p.close ? kWriterStreamEnd : kWriterOk;
          s.started = 1u, s.carry_bits = end.carry_bits;
          if (p.close) s.status = kWriterStreamEnd;
        }
        printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %u %" PRIu64 " %u\n", rc, end.fits ? p.in_used : 0, end.whole,
               end.fits ? p.n_pieces : 0, p.header, p.close, p.start_bit, s.carry_bits);
      }
    } else if (line[0] == 'E' && sscanf(line + 1, "%llu %llu %llu %llu", &a, &b, &c, &d) == 4) {
      const OneWriterEnd end = one_writer_end(a, b != 0, (uint32_t)c, d);
      printf("%" PRIu64 " %u %u\n", end.whole, end.carry_bits, end.fits);
    } else if (line[0] == 'B' && sscanf(line + 1, "%llu %llu", &a, &b) == 2) {
      printf("%" PRIu64 "\n", one_writer_bound(a, b));
    } else if (line[0] == 'O' && sscanf(line + 1, "%llu %llu %llu %llu %llu", &a, &b, &c, &d, &e) == 5) {
      printf("%d\n", one_writer_open_check(a ? (const void *)some : nullptr, (uint32_t)b, c, (uint32_t)d,
                                           e ? (const void *)some : nullptr));
    } else if (line[0] == 'A' &&
               sscanf(line + 1, "%llu %llu %llu %llu %llu %llu %llu %llu", &a, &b, &c, &d, &e, &g, &h, &i) == 8) {
      printf("%d\n", one_writer_write_check(a ? (const void *)some : nullptr, b ? some : nullptr, c, d ? some : nullptr, e,
                                            g ? &word : nullptr, h ? &word : nullptr, i ? &word32 : nullptr));
    } else {
      printf("?\n");
    }
  }
  fclose(f);
  return 0;
}
