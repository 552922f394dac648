// inflate_route_units (moonbit-flate_amd/csrc/inflate_route.h) as a stand-alone program: the route of a round of units
// of flate_hip_inflate_one.  Prints "<n> <decoder> <shape> <lanes> <row> <blocks per launch> <launches>" per case:
// argv[1] = the options' spec mode (0 / 1 / 2), argv[2] = lanes (0 = by batch size), argv[3] = CUs, then the counts.
#include <stdio.h>
#include <stdlib.h>

#include "inflate_route.h"

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  flate::InflateOpts o;
  o.spec = atoi(argv[1]);
  o.lanes = atoi(argv[2]);
  const uint32_t cus = (uint32_t)strtoul(argv[3], nullptr, 10);
  for (int i = 4; i < argc; ++i) {
    const uint32_t n = (uint32_t)strtoul(argv[i], nullptr, 10);
    const flate::InflateRoute r = flate::inflate_route_units(o, cus, n);
    printf("%u %d %d %d %d %u %u\n", n, r.decoder, r.shape, r.lanes, r.row, r.blocks_per_launch, r.launches);
  }
  return 0;
}
