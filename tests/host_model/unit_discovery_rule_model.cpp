// unit_discovery_rule_model.cpp -- the arithmetic of the unit discoveries and of the readers' window carry
// (csrc/unit_discovery_rule.h), driven from a command file so that tests/test_unit_discovery_rule_model.py can hold
// every answer against its own count.  A stand-alone program: it is built once plainly and once with AddressSanitizer
// and UBSan, and run as this program only.
//
//   run <file>: one command per line, one line of output each
//     C na nb             two_list_cap      -> "fits cap" (cap: 0 when it does not fit)
//     L n_dec per_round   unit_last_count   -> "last_count"
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "unit_discovery_rule.h"

int main(int argc, char **argv) {
  if (argc != 3 || strcmp(argv[1], "run") != 0) {
    fprintf(stderr, "usage: %s run <file>\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[2], "r");
  if (!f) return 2;
  char op;
  uint64_t a, b;
  while (fscanf(f, " %c %" SCNu64 " %" SCNu64, &op, &a, &b) == 3) {
    if (op == 'C') {
      uint32_t cap = 0;
      const bool fits = flate::two_list_cap((uint32_t)a, (uint32_t)b, &cap);
      printf("%d %u\n", fits ? 1 : 0, fits ? cap : 0u);
    } else if (op == 'L') {
      printf("%u\n", flate::unit_last_count((uint32_t)a, (uint32_t)b));
    } else {
      fclose(f);
      return 2;
    }
  }
  fclose(f);
  return 0;
}
