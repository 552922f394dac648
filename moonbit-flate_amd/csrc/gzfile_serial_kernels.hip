// gzfile_serial_kernels.hip -- a gzip FILE's short members decoded WHOLE (flate_hip_gzfile_index / _read with the
// option "gzfile_serial_max" = S >= 1; flate_kernels.h: GzSerialParams; the rule: gzfile_serial_rule.h).
//
// A member whose header and raw stream fit in S bytes and decode cleanly is ONE node of the file's chain: FIND does
// not run over it when it lies in front of the first member that is not whole, PROBE leaves it at once, TAIL never
// sees it, and the read decodes it with the batch decoders straight into its place in the output.  Every other
// member is cut into units by the kernels of gzfile_kernels.hip, which these kernels only feed:
//   gzfile_serial_ranges_kernel  a B candidate's serial range [p + hl, min(in_len - 8, p + S))
//   (the batch decoders)         ONE size-only launch over those ranges: status, out_len, used; nothing is stored
//   gzfile_serial_nodes_kernel   THE WHOLE TEST; a whole candidate's record and its hop, every other node absorbs
//   gzfile_serial_round_kernel   one step of pointer doubling over those links alone
//   gzfile_serial_from_kernel    find_from: where the walk from candidate 0 came to rest
//   gzfile_serial_base_kernel    FIND ran over in[find_from, in_len): its bits to the file's origin
//   gzfile_serial_bits_kernel    gzfile_bits_kernel, with a whole candidate parked at the raw stream's end for PROBE
//   gzfile_serial_keep_kernel    behind PROBE: a whole candidate's bit and its phase-1 record
//   gzfile_serial_marks_kernel   per unit of the path: is it a whole member, and where its stream ends
//   gzfile_serial_list_kernel    the whole members of the good units as the streams of one batch
//   gzfile_serial_check_kernel   the batch against the discovery
// No kernel waits for another workgroup; every loop is bounded by a header's length, by the node count or by 32
// search steps.  A hop lands above the trailer it skips, so the walk's links rise and nothing cycles.
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

// One thread per node of the walk (n_b + 2 of them).
__global__ __launch_bounds__(256) void gzfile_serial_nodes_kernel(GzSerialParams S) {
  const uint32_t nb = S.n_b;
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j > nb + 1u) return;
  uint32_t next = j;  // (a candidate that is not whole and the two sinks absorb)
  if (j < nb) {
    const uint64_t p = S.hdr_off[j];
    const uint64_t hl = gzip_header_len(S.in + p, S.in_len - p);
    const uint64_t E = gzfile_serial_end(S.in_len, p, S.serial_max);
    const bool whole = gzfile_serial_whole(S.status[j], p, hl, S.used[j], E);
    S.whole[j] = whole ? 1u : 0u;
    if (whole) {
      const GzSerialRecord r = gzfile_serial_record(p, hl, S.used[j], S.out_len[j]);
      OneProbe pr;
      pr.end_bit = r.end_bit;
      pr.out = r.out;
      pr.err_off = r.err_off;
      pr.status = r.status;
      pr.final_block = r.final_block;
      S.rec[j] = pr;
      const GzHop hop = gzfile_hop(S.in, S.in_len, r.end_bit);
      next = nb + 1u;
      if (hop.kind == kGzHopEnd) {
        next = nb;
      } else if (hop.kind == kGzHopNext) {
        const uint32_t at = chain_find(S.hdr_off, 0u, nb, hop.e);
        if (at < nb) next = at;
      }
    }
  }
  S.jump[0][j] = next;
}

// One thread per node.
__global__ __launch_bounds__(256) void gzfile_serial_round_kernel(const uint32_t *src, uint32_t *dst, uint32_t n) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const uint32_t t = src[j];
  dst[j] = t < n ? src[t] : j;
}

// One thread: where the walk from the member at offset 0 came to rest.
__global__ void gzfile_serial_from_kernel(GzSerialParams S, const uint32_t *jump) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  uint64_t from = S.in_len;  // the file's end, a dead hop, or no member at offset 0: nothing to search
  if (S.n_b && S.hdr_off[0] == 0ull) {
    const uint32_t t = jump[0];
    if (t < S.n_b) from = S.hdr_off[t];
  }
  S.head->find_from = from;
  S.head->n_whole = 0;
  S.head->pad = 0;
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

// One workgroup, behind the out-scan.
__global__ __launch_bounds__(1024) void gzfile_serial_list_kernel(GzFileParams P, GzSerialParams S) {
  __shared__ uint32_t wtot[16];
  const ChainParams &C = P.O.C;
  const uint32_t hi = C.head->n_members;  // the good units
  const uint32_t nw = scan_range<16, uint32_t>(
      hi, wtot, [&](uint32_t u) { return S.u_whole[u]; },
      [&](uint32_t u, uint32_t k, uint32_t v) {
        if (!v || k >= S.n_b) return;  // (a whole unit is a B node of its own: at most n_b of them)
        S.w_in_off[k] = C.member_off[u] >> 3;
        S.w_in_end[k] = S.u_end[u];
        S.w_out_off[k] = C.out_off[u];
        S.w_size[k] = P.O.usize[u];
        S.w_unit[k] = u;
      });
  if (threadIdx.x == 0) {
    const uint32_t k = nw < S.n_b ? nw : S.n_b;
    S.w_out_off[k] = C.out_off[hi];  // the last slot ends where the good units' output does
    S.w_in_off[k] = S.in_len;
    S.head->n_whole = k;
  }
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
