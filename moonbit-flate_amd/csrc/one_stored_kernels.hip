// one_stored_kernels.hip -- FIND of the block discovery for the unit rule of the option "one_stored_units": dynamic
// AND stored block headers start units (one_find_kernel.inc says why this build has a file of its own; the rules:
// deflate_block_rule.h).  Everything behind FIND is one_kernels.hip's and one_probe_kernel.inc's.
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "deflate_block_rule.h"
#include "flate_hip.h"

namespace flate {

#include "one_find_kernel.inc"

template __global__ void one_count_kernel<true>(OneParams P);
template __global__ void one_fill_kernel<true>(OneParams P);

}  // namespace flate
