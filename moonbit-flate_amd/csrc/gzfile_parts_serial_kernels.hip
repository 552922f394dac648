// gzfile_parts_serial_kernels.hip -- a gzip FILE's short members decoded WHOLE, the walk of phase 1 and what follows
// from its verdicts, for the whole file and for a PART alike (the option "gzfile_serial_max",
// flate_hip_gzfile_reader_set_serial_max: S >= 1; flate_kernels.h: GzSerialParams, GzPartSerialIn; the rule:
// gzfile_parts_serial_rule.h).  The whole file is the part that is final and starts at a BOUNDARY, with out_cap = ~0
// and no verdict array.  The other kernels of phase 1 and 2: gzfile_serial_kernels.hip; the chain's link, which stops
// a hop onto an OPEN member: gzfile_kernels.hip.
//   gzfile_serial_nodes_kernel      THE THREE VERDICTS; a WHOLE candidate's record and its link by THE PARTS HOP
//   gzfile_serial_from_kernel       find_from: INSIDE, the root, where the walk over the whole members came to rest
//   gzfile_part_serial_stop_kernel  a part's chain: did it end in front of an OPEN member
//   gzfile_serial_list_kernel       the whole members among the good units, or among the units a reader's call
//                                   decodes, as the streams of one batch
// No kernel waits for another workgroup; every loop is bounded by a header's length, by the node count or by 32 search
// steps.  A hop lands above the trailer it skips, so the links rise and nothing cycles.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "chain_rule.h"
#include "flate_hip.h"
#include "flate_kernels.h"
#include "gzfile_parts_serial_rule.h"

namespace flate {

// One thread per node of the walk (n_b + 2 of them): n_b = the file's end or a BOUNDARY stop, n_b + 1 = a dead hop.
__global__ __launch_bounds__(256) void gzfile_serial_nodes_kernel(GzSerialParams S, GzPartSerialIn A) {
  const uint32_t nb = S.n_b;
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j > nb + 1u) return;
  uint32_t next = j;  // (a candidate that is not whole and the two sinks absorb)
  if (j < nb) {
    const uint64_t p = S.hdr_off[j];
    const uint64_t hl = gzip_header_len(S.in + p, S.in_len - p);
    const uint32_t v = gzfile_parts_serial_verdict(S.in_len, A.final_in != 0u, S.serial_max, A.out_cap, p, hl, S.status[j],
                                                   S.used[j], S.out_len[j]);
    if (A.verdict) A.verdict[j] = v;
    S.whole[j] = v == kGzPartWhole ? 1u : 0u;
    if (v == kGzPartWhole) {
      const GzSerialRecord r = gzfile_serial_record(p, hl, S.used[j], S.out_len[j]);
      OneProbe pr;
      pr.end_bit = r.end_bit;
      pr.out = r.out;
      pr.err_off = r.err_off;
      pr.status = r.status;
      pr.final_block = r.final_block;
      S.rec[j] = pr;
      const GzHop hop = gzfile_parts_hop(S.in, S.in_len, r.end_bit, A.final_in != 0u);
      next = nb + 1u;
      if (hop.kind == kGzHopEnd || hop.kind == kGzHopStop) {
        next = nb;
      } else if (hop.kind == kGzHopNext) {
        const uint32_t at = chain_find(S.hdr_off, 0u, nb, hop.e);
        if (at < nb) next = at;  // (an OPEN or LONG member there absorbs: the walk rests on it)
      }
    }
  }
  S.jump[0][j] = next;
}

// One thread, behind the pointer doubling.  (No verdict array: never OPEN, and the walk rests on what is not WHOLE.)
__global__ void gzfile_serial_from_kernel(GzSerialParams S, GzPartSerialIn A, const uint32_t *jump) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  bool none = true;
  uint64_t rest_off = 0;
  uint32_t rest_verdict = kGzPartLong;
  if (S.n_b && S.hdr_off[0] == 0ull) {
    const uint32_t t = jump[0];
    if (t < S.n_b) none = false, rest_off = S.hdr_off[t], rest_verdict = A.verdict ? A.verdict[t] : kGzPartLong;
  }
  uint32_t open_stop = 0;
  S.head->find_from = gzfile_parts_serial_from(S.in_len, A.inside != 0u, none, rest_off, rest_verdict, &open_stop);
  S.head->n_whole = 0;
  S.head->pad = open_stop;
}

// One thread, behind the chain: a BOUNDARY stop at a byte where a header passes the rule is the OPEN stop (THE PARTS HOP
// alone would have gone on to that member).
__global__ void gzfile_part_serial_stop_kernel(GzFileParams P, GzSerialParams S) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const ChainParams &C = P.O.C;
  uint32_t open_stop = 0;
  if (C.head->rc == 0 && P.gh->pad[0] == kGzPartEndStop) {
    const uint64_t e = (uint64_t)P.gh->err_off;
    if (e < C.in_len && gzfile_first_bit(C.in, C.in_len, e) != 0ull) open_stop = 1u;
  }
  S.head->pad = open_stop;
}

// One workgroup: the whole members among the first n_dec units as the streams of one batch.  A slot ends at the next
// whole member's start; the LAST ends at `total`.  from_head (the whole call, behind the out-scan): the good units and
// where their output ends.  Else (a reader's call, behind the host's plan): the units the call decodes and its planned
// total, behind which the reader writes nothing.
__global__ __launch_bounds__(1024) void gzfile_serial_list_kernel(GzFileParams P, GzSerialParams S, uint32_t from_head,
                                                                  uint32_t n_dec, uint64_t total) {
  __shared__ uint32_t wtot[16];
  const ChainParams &C = P.O.C;
  if (from_head) n_dec = C.head->n_members, total = C.out_off[n_dec];
  const uint32_t nw = scan_range<16, uint32_t>(
      n_dec, wtot, [&](uint32_t u) { return S.u_whole[u]; },
      [&](uint32_t u, uint32_t k, uint32_t v) {
        if (!v || k >= S.n_b) return;  // (a whole unit is a B node of its own: at most n_b of them)
        S.w_in_off[k] = C.member_off[u] >> 3;
        S.w_in_end[k] = S.u_end[u];
        S.w_out_off[k] = C.out_off[u] < total ? C.out_off[u] : total;
        S.w_size[k] = P.O.usize[u];
        S.w_unit[k] = u;
      });
  if (threadIdx.x == 0) {
    const uint32_t k = nw < S.n_b ? nw : S.n_b;
    S.w_out_off[k] = total;
    S.w_in_off[k] = S.in_len;
    S.head->n_whole = k;
  }
}

}  // namespace flate
