// zip_units_kernels.hip -- the LONG entries of a ZIP archive decoded through units (flate_hip_zip_read with the option
// "zip_unit_min"): the units of all L entries as ONE chain over the hull's bits, the entries found from it, and the
// decode's entry-wise parts (zip_kernels.h: ZipUnitsParams, ZipUnitsDecParams; the rule: zip_units_rule.h).  The ZIP
// counterpart of gzfile_kernels.hip.
//
// The passes are the existing ones, run over the HULL as their raw stream (one_init_kernel over the hull's length:
// every bit is counted from the hull's first byte): one_count_kernel / one_fill_kernel (List A), one_probe_kernel over
// all nodes, chain_round_kernel, one_out_scan_kernel, and in the decode one_tail_kernel, one_seek_compose_kernel /
// one_seek_resolve_kernel, the lane-per-stream dictionary decoder and one_check_kernel.  What is this format's own:
//   zip_units_bits_kernel     a B node's bit: 8 * L[i].lo -- nodes placed from the directory, not from headers
//   zip_units_link_kernel     zip_units_next: the A node at a unit's end inside its entry; behind BFINAL the next L entry
//   zip_units_finish_kernel   path rank r -> unit_bit[r], the unit's size, whether it starts and whether it ends an entry;
//                             the thread at which the path meets a sink writes the unit count
//   zip_units_entries_kernel  the scan over the "starts an entry" marks -> u_entry, entry_unit, the complete entries
//   zip_units_rel_kernel      rel_off, and the ordered min of the entries whose units miss the directory's size
//   zip_units_pieces_kernel   a round's pieces: ZIP slot, history (never across an entry), seed, where the piece ends,
//                             and the gap pieces between two entries' slots
//   zip_units_fold_kernel     what DECODE reports per piece -> per unit, for one_check_kernel
//   zip_units_verdict_kernel  out_len = size, status = 0, err_off = -1 for the served entries, into the arrays that
//                             zip_prep_kernel, the clipped checksums and zip_verdict_kernel consume
// A unit ends strictly above its start and a hop rises in chain index, so nothing cycles.  No kernel waits for another
// workgroup; every loop is bounded by the unit count, an entry count or 32 search steps.
#include <hip/hip_runtime.h>

#include "chain_walk.h"
#include "flate_hip.h"
#include "window_compose.h"
#include "zip_kernels.h"
#include "zip_units_rule.h"

namespace flate {

// One thread per B node.
__global__ __launch_bounds__(256) void zip_units_bits_kernel(ZipUnitsParams P) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= P.n_b) return;
  P.O.C.cand_off[P.n_a + j] = 8u * P.L[j].lo;
}

// One thread per node (n_a + n_b + 2 of them).
__global__ __launch_bounds__(256) void zip_units_link_kernel(ZipUnitsParams P) {
  const ChainParams &C = P.O.C;
  const uint32_t n = C.cap, na = P.n_a, nb = P.n_b;
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c == 0) {
    C.path[0] = na;  // the chain starts at the first L entry (nb >= 1)
    OneHead h{};
    h.h.rc = FLATE_HIP_E_CORRUPT;  // until a finish thread has met the end sink
    h.h.n_cand = n;
    h.raw_len = P.O.one->pay_end;
    *P.O.head = h;
    ZipUnitsHead z;
    z.n_complete = 0u;
    z.first_unfit = 0xffffffffu;
    *P.zh = z;
    C.member_off[0] = 0ull;
    P.u_start[0] = 0u;
  }
  if (c > n + 1u) return;
  uint32_t next = c;  // (the sinks absorb)
  if (c < n) {
    const OneProbe pr = P.O.probe[c];
    uint32_t x = nb;  // the owner
    if (c >= na) {
      x = c - na;
    } else {
      const uint32_t at = zip_units_owner(P.R, nb, C.cand_off[c] >> 3);
      if (at < nb) x = P.R[at].entry;
    }
    next = zip_units_next(C.cand_off, na, nb, x, x < nb ? P.L[x].end : 0ull, pr.status == 0, pr.final_block != 0u, pr.end_bit);
  }
  C.jump[0][c] = next;
}

__global__ __launch_bounds__(256) void zip_units_finish_kernel(ZipUnitsParams P) {
  const ChainParams &C = P.O.C;
  const uint32_t n = C.cap;
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r + 1u >= C.path_len) return;  // (the last entry is a sink)
  const uint32_t c = C.path[r];
  if (c >= n) return;
  const OneProbe pr = P.O.probe[c];
  C.member_off[r] = C.cand_off[c];
  P.u_start[r] = c >= P.n_a ? c - P.n_a + 1u : 0u;
  P.O.usize[r] = pr.out;
  P.u_final[r] = pr.status == 0 ? pr.final_block : 0u;
  // (the chain holds at most n nodes and path_len >= n + 2: r + 1 is inside the path)
  const uint32_t succ = C.path[r + 1u];
  if (succ < n) return;
  // the path meets a sink behind this unit: one thread gets here.  The dead sink: this unit is no good one (its probe
  // failed, it ends outside its entry, or nothing starts where it ends) -- the batch decoders say why.
  BgzfHead *h = C.head;
  if (succ == n) {
    h->n_members = r + 1u;
    C.member_off[r + 1u] = pr.end_bit;
    P.u_start[r + 1u] = 0u;
    h->rc = 0;
    h->err_off = -1;
  } else {
    h->n_members = r;
  }
}

// One workgroup, behind the out-scan: the scan over the marks of the good units.  The chain starts at L[0] and a hop
// goes to the next L entry, so the e-th mark is L[e]'s.
__global__ __launch_bounds__(1024) void zip_units_entries_kernel(ZipUnitsParams P) {
  __shared__ uint32_t wtot[16];
  const uint32_t nu = P.O.C.head->n_members;
  const uint32_t started = scan_range<16, uint32_t>(
      nu, wtot, [&](uint32_t k) { return P.u_start[k] ? 1u : 0u; },
      [&](uint32_t k, uint32_t before, uint32_t v) {
        P.u_entry[k] = before + v - 1u;
        if (v) P.entry_unit[before] = k;
      });
  if (threadIdx.x == 0) {
    P.entry_unit[started] = nu;
    P.u_entry[nu] = started;
    // the last started entry is complete iff the last good unit ends it
    P.zh->n_complete = nu == 0u ? 0u : (P.u_final[nu - 1u] ? started : started - 1u);
  }
}

// One thread per good unit (and the one behind them), behind zip_units_entries_kernel.
__global__ __launch_bounds__(256) void zip_units_rel_kernel(ZipUnitsParams P) {
  const ChainParams &C = P.O.C;
  const uint32_t nu = C.head->n_members;
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k > nu) return;
  if (k == nu) {
    P.rel_off[k] = 0ull;
    return;
  }
  const uint32_t e = P.u_entry[k];
  const uint64_t first = C.out_off[P.entry_unit[e]];
  P.rel_off[k] = C.out_off[k] - first;
  if (P.u_final[k] && !zip_units_good(k + 1u, nu, true, C.out_off[k + 1u] - first, P.L[e].size))
    atomicMin(&P.zh->first_unfit, e);
}

// One thread per unit of the round (and one more).  Every unit decoded here belongs to a complete entry.
__global__ __launch_bounds__(256) void zip_units_pieces_kernel(ZipUnitsDecParams G) {
  const OneDecParams &D = G.D;
  const ZipUnitsParams &P = G.P;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i > D.count) return;
  const uint32_t fb = D.dh->first_bad;
  // where unit u starts and ends in `out`
  auto starts = [&](uint32_t u) { return zip_units_slot(P.L[P.u_entry[u]].out, P.rel_off[u]); };
  auto ends = [&](uint32_t u) {
    const uint32_t e = P.u_entry[u];
    return zip_units_slot(P.L[e].out, D.out_off[u + 1u] - D.out_off[P.entry_unit[e]]);
  };
  // the first unit that fails TAIL and every unit behind it get an empty slot: nothing is written there (the batch
  // decoders decode those entries)
  uint64_t limit = D.total;
  if (fb != 0xffffffffu) limit = starts(fb);
  if (limit > D.total) limit = D.total;
  auto clip = [&](uint64_t at) { return at < limit ? at : limit; };
  const uint32_t e0 = P.u_entry[D.u0];
  if (i == D.count) {
    const uint32_t last = D.u0 + D.count - 1u;
    D.p_out_off[D.count + (P.u_entry[last] - e0)] = clip(ends(last));
    return;
  }
  const uint32_t u = D.u0 + i, e = P.u_entry[u];
  const uint32_t p = i + (e - e0);
  const uint32_t f = (uint32_t)P.entry_unit[e];  // its entry's first unit
  D.p_out_off[p] = clip(starts(u));
  const uint32_t dict_len = zip_units_history(P.rel_off[u]);
  D.p_dict_len[p] = dict_len;
  D.p_dict_at[p] = (uint64_t)(i + 1u) * kWinEntries - dict_len;  // the tail of R[i]; R[i + 1] follows it
  G.seed[i] = f > D.u0 ? f - D.u0 : 0u;  // (an entry that began in a round in front continues from R[0])
  G.p_bit_off[p] = D.unit_bit[u];
  G.p_bit_end[p] = P.u_final[u] ? ~0ull : D.unit_bit[u + 1u];
  if (i != 0u && P.u_start[u]) {  // the gap in front of this entry: a piece of no bits, it writes nothing
    D.p_out_off[p - 1u] = clip(ends(u - 1u));
    D.p_dict_len[p - 1u] = 0u;
    D.p_dict_at[p - 1u] = 0ull;
    G.p_bit_off[p - 1u] = D.unit_bit[u];
    G.p_bit_end[p - 1u] = D.unit_bit[u];
  }
}

// One thread per unit of the round, behind DECODE.
__global__ __launch_bounds__(256) void zip_units_fold_kernel(ZipUnitsDecParams G) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= G.D.count) return;
  const uint32_t p = i + (G.P.u_entry[G.D.u0 + i] - G.P.u_entry[G.D.u0]);
  G.du_status[i] = G.dp_status[p];
  G.du_out_len[i] = G.dp_out_len[p];
}

// One thread per served entry, behind zip_prep_kernel.
__global__ __launch_bounds__(256) void zip_units_verdict_kernel(ZipUnitsDecParams G) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= G.g) return;
  const ZuEntry z = G.P.L[e];
  G.z_out_len[z.slot] = z.size;
  G.z_status[z.slot] = 0;
  G.z_err_off[z.slot] = -1;
}

}  // namespace flate
