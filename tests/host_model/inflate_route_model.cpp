// inflate_route_model.cpp -- moonbit-flate_amd/csrc/inflate_route.h behind a C interface (tests/test_inflate_route.py).
// Built with -DROUTE_MODEL_MAIN it is a program of its own that walks the test's table (for a sanitizer build).
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "inflate_route.h"

using namespace flate;

namespace {
void put(const InflateRoute &r, int64_t out[6]) {
  out[0] = r.decoder, out[1] = r.shape, out[2] = r.lanes, out[3] = r.row, out[4] = r.blocks_per_launch, out[5] = r.launches;
}
}  // namespace

// opt = {lanes, row, simt_min, spec, spec_shape, spec_max}
extern "C" void route_defaults(int64_t opt[6]) {
  const InflateOpts o;
  opt[0] = o.lanes, opt[1] = o.row, opt[2] = o.simt_min, opt[3] = o.spec, opt[4] = o.spec_shape, opt[5] = o.spec_max;
}

extern "C" void route_model(const int64_t opt[6], uint32_t num_cus, uint32_t n, uint64_t longest, int spliced,
                            int size_only, int64_t out[6]) {
  InflateOpts o;
  o.lanes = (int)opt[0], o.row = (int)opt[1], o.simt_min = (uint32_t)opt[2];
  o.spec = (int)opt[3], o.spec_shape = (int)opt[4], o.spec_max = (uint32_t)opt[5];
  put(inflate_route(o, num_cus, n, longest, spliced != 0, size_only != 0), out);
}

// the same from the call's index, as the driver does it
extern "C" void route_model_index(const int64_t opt[6], uint32_t num_cus, const uint64_t *off, uint32_t n, int spliced,
                                  int size_only, int64_t out[6]) {
  route_model(opt, num_cus, n, longest_entry(off, n), spliced, size_only, out);
}

#ifdef ROUTE_MODEL_MAIN
int main() {
  const uint32_t ns[] = {1, 1024, 1025, 2048, 2049, 20479, 20480, 36863, 36864, 45055, 45056, 196608};
  const uint64_t longs[] = {1, 65536, (1ull << 28) - 1, 1ull << 28, (1ull << 31) - 1, 1ull << 31};
  const int lanes[] = {0, 16, 32, 64}, rows[] = {0, 8, 16}, three[] = {0, 1, 2};
  const uint32_t mins[] = {0, 1, 2049};
  long cases = 0, bad = 0;
  for (uint32_t n : ns)
    for (uint64_t longest : longs)
      for (int spliced : {0, 1})
        for (int size_only : {0, 1})
          for (int spec : three)
            for (int shape : three)
              for (int l : lanes)
                for (int row : rows)
                  for (uint32_t smin : mins) {
                    const int64_t opt[6] = {l, row, smin, spec, shape, 45056};
                    int64_t r[6];
                    route_model(opt, 256, n, longest, spliced, size_only, r);
                    ++cases;
                    if (r[0] < 0 || r[0] > 2 || r[4] == 0 || r[5] == 0) ++bad;
                    if (r[0] == kDecodeSimt) {  // the launches cover every block, the last one is not empty
                      const int64_t sblocks = (n + r[2] - 1) / r[2];
                      if (r[4] * r[5] < sblocks || r[4] * (r[5] - 1) >= sblocks) ++bad;
                    } else if (r[4] != n || r[5] != 1) {
                      ++bad;
                    }
                  }
  {  // one long stream among small ones moves the batch; the documented split
    std::vector<uint64_t> off(4097, 0);
    for (uint32_t i = 1; i <= 4096; ++i) off[i] = off[i - 1] + (i == 7 ? (1ull << 28) : 100);
    int64_t d[6], r[6];
    route_defaults(d);
    route_model_index(d, 256, off.data(), 4096, 0, 0, r);
    if (r[0] != kDecodeWave) ++bad;
    d[0] = 64, d[3] = 0;
    route_model(d, 256, 196608, 65536, 0, 0, r);
    if (r[0] != kDecodeSimt || r[4] != 1536 || r[5] != 2) ++bad;
    cases += 2;
  }
  printf("inflate_route: %ld cases, %ld bad\n", cases, bad);
  return bad ? 1 : 0;
}
#endif
