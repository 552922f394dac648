// lz77_hooks_rule_model.cpp -- TEST INFRASTRUCTURE.  The rule that picks the match-finder kernels' build for a batch
// launch (lz77_hooks_build, moonbit-flate_amd/csrc/deflate_plan.h) behind a C entry point: this file includes the
// header the driver includes (run_lz77, flate_api_deflate.hip).
#include "deflate_plan.h"

extern "C" int hooks_build_model(uint32_t inject_stall, uint32_t inject_drop_push) {
  return flate::lz77_hooks_build(inject_stall, inject_drop_push) ? 1 : 0;
}
