// unit_discovery.h -- the discovery of units over TWO lists, written once (private, host only; flate_api_units.hip is
// the user).
//
// A long stream's units are found by FIND (List A: the bits that pass the block-header rule) and chained by PROBE, link,
// pointer doubling, finish and out-scan (flate_kernels.h: THE DISCOVERY SKELETON).  A gzip file, a gzip file read in
// parts, a gzip file with "gzfile_serial_max" and the long entries of a ZIP archive add List B -- the members' or
// entries' first units, found by the format's own rule -- to the same chain, and per unit the words that say which
// member or entry it belongs to.  What those discoveries share stands here: the count pass over List A, the size rule,
// the carve of the node arrays, the chain's launches behind the fills and the last read-back.  What they differ in --
// the kernels of List B, of the link, the finish and the scans, and what comes back beside the result words -- stays
// with them, as the hooks of unit_nodes_carve and unit_chain.
#pragma once

#include "flate_ctx.h"
#include "unit_discovery_rule.h"

namespace flate_host {

// FIND's count pass or fill pass over n_tiles tiles, in the build of P's unit rule (option "one_stored_units")
// parts: the builds whose chain starts at bit FrameOne::b0 (a stream or a file read in parts)
inline void one_find_launch(flate_hip_ctx *c, bool count, uint32_t n_tiles, const flate::OneParams &P, bool parts) {
  using namespace flate;
  if (parts) {
    if (count && P.stored_units)
      hipLaunchKernelGGL((one_count_kernel<true, true>), dim3(n_tiles), dim3(256), 0, c->stream, P);
    else if (count)
      hipLaunchKernelGGL((one_count_kernel<false, true>), dim3(n_tiles), dim3(256), 0, c->stream, P);
    else if (P.stored_units)
      hipLaunchKernelGGL((one_fill_kernel<true, true>), dim3(n_tiles), dim3(256), 0, c->stream, P);
    else
      hipLaunchKernelGGL((one_fill_kernel<false, true>), dim3(n_tiles), dim3(256), 0, c->stream, P);
    return;
  }
  if (count && P.stored_units)
    hipLaunchKernelGGL(one_count_kernel<true>, dim3(n_tiles), dim3(256), 0, c->stream, P);
  else if (count)
    hipLaunchKernelGGL(one_count_kernel<false>, dim3(n_tiles), dim3(256), 0, c->stream, P);
  else if (P.stored_units)
    hipLaunchKernelGGL(one_fill_kernel<true>, dim3(n_tiles), dim3(256), 0, c->stream, P);
  else
    hipLaunchKernelGGL(one_fill_kernel<false>, dim3(n_tiles), dim3(256), 0, c->stream, P);
}

// PROBE over n_blocks candidates (or the one tail probe), in the build of the unit rule its parameters carry (TAIL:
// one_tail_launch, unit_rounds.h)
inline void one_probe_launch(flate_hip_ctx *c, uint32_t n_blocks, const flate::OneParams &P, uint32_t tail) {
  if (P.stored_units)
    hipLaunchKernelGGL(flate::one_probe_kernel<true>, dim3(n_blocks), dim3(64), 0, c->stream, P, tail);
  else
    hipLaunchKernelGGL(flate::one_probe_kernel<false>, dim3(n_blocks), dim3(64), 0, c->stream, P, tail);
}

// List A beside the chain O it feeds: the chain's input, tiles, unit rule and FrameOne, the count pass's own result
// words head_a.  (PA.C.tile_cnt is the caller's take; PA.C.cand_off is the chain's once that is carved.)
inline void find_params(flate::OneParams &PA, const flate::OneParams &O, flate::OneHead *head_a) {
  PA.C.in = O.C.in;
  PA.C.in_len = O.C.in_len;
  PA.C.n_tiles = O.C.n_tiles;
  PA.C.head = &head_a->h;
  PA.head = head_a;
  PA.one = O.one;
  PA.unit_max = O.unit_max;
  PA.stored_units = O.stored_units;
}

// THE COUNT PASS over List A: FIND counts per tile, the scan leaves the candidate count in PA.head
inline void find_count(flate_hip_ctx *c, const flate::OneParams &PA, bool parts) {
  one_find_launch(c, true, PA.C.n_tiles, PA, parts);
  hipLaunchKernelGGL(flate::chain_scan_kernel, dim3(1), dim3(1024), 0, c->stream, PA.C);
}
// ... and the ONE read-back of the counts: List A's words and, where List B is counted on the device too, its own
inline int find_counts_back(flate_hip_ctx *c, const flate::OneHead *head_a, flate::OneHead &HA,
                            const flate::BgzfHead *head_b = nullptr, flate::BgzfHead *HB = nullptr) {
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&HA, head_a, sizeof HA, hipMemcpyDeviceToHost, c->stream));
  if (head_b) HIP_TRY(c, hipMemcpyAsync(HB, head_b, sizeof *HB, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FLATE_HIP_OK;
}

// THE SIZE RULE (unit_discovery_rule.h) and the sizes of the joint chain C, of List A's and -- CB != null: where List B
// is a chain of its own that has not been sized yet -- of List B's
inline int two_list_size(flate::ChainParams &C, flate::ChainParams &CA, flate::ChainParams *CB, uint32_t na, uint32_t nb) {
  int rc;
  uint32_t cap = 0;
  if (!flate::two_list_cap(na, nb, &cap)) return FLATE_HIP_E_TOO_LARGE;  // (the counts saturate at 2^32 - 1)
  if ((rc = chain_size(C, cap)) || (rc = chain_size(CA, na))) return rc;
  return CB ? chain_size(*CB, nb) : FLATE_HIP_OK;
}

// THE NODE ARRAYS of a chain of n candidates, in the order every discovery lays them out; mid(k) takes what a format
// keeps between the candidates and their probes
template <class Mid>
void chain_nodes_take(Carve &k, flate::OneParams &O, size_t n, Mid mid) {
  flate::ChainParams &C = O.C;
  k.take(C.cand_off, n);
  mid(k);
  k.take(O.probe, n);
  k.take(C.jump[0], n + 2);
  k.take(C.jump[1], n + 2);
  k.take(C.path, C.path_len);
  k.take(O.usize, n);
  k.take(C.member_off, n + 1);
  k.take(C.out_off, n + 1);
}
// ... and b as the arrays of a two-list chain P (GzFileParams, ZipUnitsParams): the nodes, the four per-unit arrays --
// u_owner is the format's name for a unit's member or entry --, then what end(k) takes
template <class FP, class Mid, class End>
int unit_nodes_carve(flate_hip_ctx *c, DevBuf &b, FP &P, uint32_t *&u_owner, size_t n, Mid mid, End end) {
  return carve(c, b, [&](Carve &k) {
    chain_nodes_take(k, P.O, n, mid);
    k.take(P.u_start, n + 1);
    k.take(P.u_final, n);
    k.take(u_owner, n + 1);
    k.take(P.rel_off, n + 1);
    end(k);
  });
}

// THE CHAIN behind the fills and PROBE: chain_tail_by with the format's link(grid), finish(grid) and mid(node_blocks),
// the out-scan of the units; behind(node_blocks) -- the format's member or entry scan, tail probe and rel kernel, in its
// order --; then the ONE read-back of the result words H, the format's head G and whatever back() queues beside them.
template <class Link, class Finish, class Mid, class Behind, class Head, class Back>
int unit_chain(flate_hip_ctx *c, const flate::OneParams &O, Link link, Finish finish, Mid mid, Behind behind,
               flate::OneHead &H, Head &G, const Head *d_g, Back back) {
  int rc;
  if ((rc = chain_tail_by(c, O.C, link, finish, mid, flate::one_out_scan_kernel, O))) return rc;
  behind((uint32_t)(((uint64_t)O.C.cap + 2 + 255) / 256));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&H, O.head, sizeof H, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&G, d_g, sizeof G, hipMemcpyDeviceToHost, c->stream));
  if ((rc = back())) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return H.h.n_members > O.C.cap ? FLATE_HIP_E_INTERNAL : FLATE_HIP_OK;
}

}  // namespace flate_host
