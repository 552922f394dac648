// chain_kernels.hip -- the two kernels every discovery launches as they are (chain_walk.h; flate_kernels.h:
// ChainParams): the scan of the tiles' counts and the rounds of pointer doubling.  They know nothing of any format.
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "flate_hip.h"

namespace flate {

// One workgroup: tile_cnt becomes its exclusive scan (n_tiles + 1 entries); the head is initialised.
__global__ __launch_bounds__(1024) void chain_scan_kernel(ChainParams C) {
  __shared__ uint64_t wtot[16];
  tile_scan(C, wtot, FLATE_HIP_E_CORRUPT);
}

// Round j: the known path [0, 2^j) yields [2^j, 2^(j+1)) through jump[j & 1] (2^j steps), which is then squared into
// the other array.  A successor lies strictly above its candidate, so nothing cycles; the host launches
// ceil(log2(cap + 2)) rounds.
__global__ __launch_bounds__(256) void chain_round_kernel(ChainParams C, uint32_t j) {
  const uint32_t n = C.head->n_cand;
  if (n > C.cap) return;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t *cur = C.jump[j & 1u];
  uint32_t *nxt = C.jump[(j & 1u) ^ 1u];
  const uint32_t half = 1u << j;
  if (i < half && half + i < C.path_len) C.path[half + i] = cur[C.path[i]];
  if (i <= n + 1u) nxt[i] = cur[cur[i]];
}

}  // namespace flate
