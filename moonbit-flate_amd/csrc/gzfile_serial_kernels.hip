// gzfile_serial_kernels.hip -- a gzip FILE's short members decoded WHOLE (S >= 1: the option "gzfile_serial_max" of
// flate_hip_gzfile_index / _read, flate_hip_gzfile_reader_set_serial_max of a reader in parts; flate_kernels.h:
// GzSerialParams; the rule: gzfile_serial_rule.h).
//
// A member whose header and raw stream fit in S bytes and decode cleanly is ONE node of the file's chain: FIND does
// not run over it when it lies in front of the first member that is not whole, PROBE leaves it at once, TAIL never
// sees it, and the read decodes it with the batch decoders straight into its place in the output.  Every other
// member is cut into units by the kernels of gzfile_kernels.hip, which these kernels only feed.  Here stand the ones
// that know nothing of a part; the walk's verdicts and what follows from them: gzfile_parts_serial_kernels.hip.
//   gzfile_serial_ranges_kernel  a B candidate's serial range [p + hl, min(in_len - 8, p + S))
//   (the batch decoders)         ONE size-only launch over those ranges: status, out_len, used; nothing is stored
//   gzfile_serial_round_kernel   one step of pointer doubling over the walk's links alone
//   gzfile_serial_base_kernel    FIND ran over in[find_from, in_len): its bits to the file's origin
//   gzfile_serial_bits_kernel    gzfile_bits_kernel, with a whole candidate parked at the raw stream's end for PROBE
//   gzfile_serial_keep_kernel    behind PROBE: a whole candidate's bit and its phase-1 record
//   gzfile_serial_marks_kernel   per unit of the path: is it a whole member, and where its stream ends
//   gzfile_serial_check_kernel   the batch against the discovery
// No kernel waits for another workgroup; every loop is bounded by a header's length.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "chain_rule.h"
#include "flate_hip.h"
#include "flate_kernels.h"
#include "gzfile_serial_rule.h"

namespace flate {

// One thread per B candidate.
__global__ __launch_bounds__(256) void gzfile_serial_ranges_kernel(GzSerialParams S) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= S.n_b) return;
  const uint64_t p = S.hdr_off[j];
  const uint64_t hl = gzip_header_len(S.in + p, S.in_len - p);  // (never 0: the fill pass applied the same rule)
  const uint64_t E = gzfile_serial_end(S.in_len, p, S.serial_max);
  S.pay_off[j] = gzfile_serial_begin(p, hl, E);
  S.pay_end[j] = E;
  if (j == 0) S.pay_off[S.n_b] = S.in_len;
}

// One thread per node.
__global__ __launch_bounds__(256) void gzfile_serial_round_kernel(const uint32_t *src, uint32_t *dst, uint32_t n) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint32_t t = src[j];
  dst[j] = t < n ? src[t] : j;
}

__global__ __launch_bounds__(256) void gzfile_serial_base_kernel(uint64_t *cand_off, uint32_t n, uint64_t base_bits) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) cand_off[i] += base_bits;
}

// One thread per B node.
__global__ __launch_bounds__(256) void gzfile_serial_bits_kernel(GzFileParams P, GzSerialParams S) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= P.n_b) return;
  // a whole candidate: the raw stream's end, where a probe meets the end of its input at once
  P.O.C.cand_off[P.n_a + j] =
      S.whole[j] ? 8u * P.O.one->pay_end : gzfile_first_bit(P.O.C.in, P.O.C.in_len, P.hdr_off[j]);
}

// One thread per B node, behind PROBE.
__global__ __launch_bounds__(256) void gzfile_serial_keep_kernel(GzFileParams P, GzSerialParams S) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= P.n_b || !S.whole[j]) return;
  P.O.C.cand_off[P.n_a + j] = gzfile_first_bit(P.O.C.in, P.O.C.in_len, P.hdr_off[j]);
  P.O.probe[P.n_a + j] = S.rec[j];
}

// One thread per path rank, behind gzfile_finish_kernel.
__global__ __launch_bounds__(256) void gzfile_serial_marks_kernel(GzFileParams P, GzSerialParams S) {
  const ChainParams &C = P.O.C;
  const uint32_t n = C.cap;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r > n || r >= C.path_len) return;
  const uint32_t c = C.path[r];
  const bool whole = c < n && c >= P.n_a && S.whole[c - P.n_a] != 0u;
  S.u_whole[r] = whole ? 1u : 0u;
  S.u_end[r] = whole ? P.O.probe[c].end_bit >> 3 : 0ull;
}

// One thread per stream of the batch of whole members.
__global__ __launch_bounds__(256) void gzfile_serial_check_kernel(GzSerialParams S, uint32_t n_whole,
                                                                  const int32_t *d_status, const uint64_t *d_out_len,
                                                                  OneDecHead *dh) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n_whole) return;
  if (d_status[k] != 0 || d_out_len[k] != S.w_size[k]) atomicMin(&dh->decode_bad, S.w_unit[k]);
}

}  // namespace flate
