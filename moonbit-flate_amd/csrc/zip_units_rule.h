// zip_units_rule.h -- how the LONG entries of a ZIP archive are decoded through units (flate_hip_zip_read with the
// option "zip_unit_min"), written ONCE: plain C++17 without HIP, compiled into the kernels (zip_units_kernels.hip), into
// the library's host code (flate_api_zip.hip) and into tests/host_model/zip_units_rule_model.cpp, which compares it with
// tests/zip_units_ref.py.
//
// THE SET L (zip_units_form): the selection slots j, ascending (which is ascending out_off), whose entry has index
// status 0, method 8, comp_size >= zip_unit_min, passes the FLATE_HIP_E_TOO_LARGE test of the read, is the FIRST
// occurrence of its entry number in the selection, and whose data range [data_off, data_off + comp_size) overlaps no
// other such entry's range.  A slot that fails one of the last two conditions goes to the batch decoders (`fallback`):
// two chains must never share a node.  Chain order is slot order, not file order.
//
// THE HULL: from the smallest data_off of L to the largest range end.  FIND, PROBE, TAIL and DECODE are given the
// hull as their raw stream: EVERY BIT AND EVERY BYTE OFFSET OF THE UNIT PATH IS COUNTED FROM THE HULL'S FIRST BYTE
// (ZuEntry::lo / end, cand_off, unit_bit), never from the archive's.
//
// NODES.  List A: the FIND candidates of the hull (sorted by bit).  List B: one node per L entry at bit 8 * lo, in
// chain order -- a unit start whatever block type is there.  Node na + nb is the end sink, na + nb + 1 the dead sink.
// A node's OWNER is the L entry whose range holds the node's byte (zip_units_owner: a binary search over the ranges
// sorted by file position; an A node inside no range has none and is never linked).
//
// THE LINK (zip_units_next).  A unit of entry X that stops in front of a unit-starting header links to the A node at
// that bit, provided the bit lies inside X's range.  A unit that ends with BFINAL at or before X's end links to the B
// node of the next L entry in chain order; the last entry's to the end sink.  A unit that failed its probe, or ends
// behind X's end, or finds no node at its end, links to the dead sink.  Bytes between BFINAL and X's end are not
// examined, as the batch decoders do not examine them.  Nothing cycles: an A link rises in bits inside one entry (a
// unit ends at least three bits above its start), and a B hop rises in chain index.
//
// GOOD (zip_units_good, and the decode rounds).  An L entry is GOOD iff its chain reaches BFINAL inside its range
// with every probe status 0, its units' output sums to the directory's size, and every unit of it passes TAIL and
// the decode round's check.  g = the L entries in front of the first one that is not GOOD: L[0, g) are served by
// units, L[g] and everything behind it by the batch decoders, exactly as with the option off.
//
// SLOTS.  Unit k of GOOD entry j writes at out_off_zip[j] + rel (rel = unit out_off[k] - unit out_off[first unit of
// j]); its history is min(32768, rel) bytes and never crosses an entry.
#pragma once

#include <stdint.h>

#include "chain_rule.h"
#include "flate_hip.h"

#include <algorithm>
#include <vector>

namespace flate {

struct ZuEntry {        // one L entry, in chain order
  uint64_t lo, end;     // its data range, counted from the hull's first byte
  uint64_t size;        // what the directory says it inflates to
  uint64_t out;         // out_off_zip[slot]
  uint32_t slot, pad;   // its selection slot j
};
struct ZuRange {        // the same ranges sorted by file position
  uint64_t lo, end;
  uint32_t entry, pad;  // the chain index
};

constexpr uint32_t kZuWindow = 32768;

// the read's refusal of an entry with index status 0 (its limits are the batch decoders')
CHAIN_HD bool zip_units_too_large(uint64_t size, uint32_t method, uint64_t comp_size) {
  return size > 0xffffffffull || (method == 8 && comp_size >= 0x7ffe0000ull);
}

// the entry of L whose range holds `byte`, as its place in R (sorted, disjoint), or n: none.  At most 32 steps.
CHAIN_HD uint32_t zip_units_owner(const ZuRange *R, uint32_t n, uint64_t byte) {
  uint32_t lo = 0, hi = n;  // the first range with R.lo > byte
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (R[mid].lo <= byte) lo = mid + 1u;
    else hi = mid;
  }
  if (lo == 0) return n;
  return byte < R[lo - 1u].end ? lo - 1u : n;
}

// THE LINK: where the unit of a node goes.  x: the chain index of the node's owner, or nb: none; x_end: that entry's
// `end`; ok / final_block / end_bit: what the node's probe left; cand_off[0, na): List A's bits.
CHAIN_HD uint32_t zip_units_next(const uint64_t *cand_off, uint32_t na, uint32_t nb, uint32_t x, uint64_t x_end, bool ok,
                                 bool final_block, uint64_t end_bit) {
  const uint32_t end_sink = na + nb, dead = na + nb + 1u;
  if (!ok || x >= nb) return dead;
  if (end_bit > 8u * x_end) return dead;  // it ends behind X's end
  if (final_block) return x + 1u < nb ? na + x + 1u : end_sink;
  if (end_bit >= 8u * x_end) return dead;  // the header it stopped at lies behind X's range
  const uint32_t at = chain_find(cand_off, 0u, na, end_bit);
  return at < na ? at : dead;
}

// SLOTS: where a unit writes and how much history it has
CHAIN_HD uint64_t zip_units_slot(uint64_t entry_out, uint64_t rel) { return entry_out + rel; }
CHAIN_HD uint32_t zip_units_history(uint64_t rel) { return rel < (uint64_t)kZuWindow ? (uint32_t)rel : kZuWindow; }

// GOOD, the discovery's part, for the entry whose units are [u_first, u_next) of a chain with n_units good units:
// all of its units are good ones, the last ends with BFINAL, and they sum to the directory's size.
CHAIN_HD bool zip_units_good(uint32_t u_next, uint32_t n_units, bool last_final, uint64_t out_sum, uint64_t size) {
  return u_next <= n_units && last_final && out_sum == size;
}

// ---- host code ----

// THE SET L over the index `ent` (n entries) and the selection (sel == NULL: every entry, ns = n), with out_off the
// read's slots (ns + 1).  L in chain order with ARCHIVE offsets in lo / end (zip_units_hull moves them), R sorted by
// file position; *fallback = the slots that qualified by size and were refused as duplicates or for overlap.
// O(ns log ns).
inline void zip_units_form(const flate_hip_zip_entry *ent, uint32_t n, const uint32_t *sel, uint32_t ns,
                           const uint64_t *out_off, uint64_t unit_min, std::vector<ZuEntry> &L, std::vector<ZuRange> &R,
                           uint32_t *fallback) {
  L.clear(), R.clear();
  *fallback = 0;
  if (unit_min == 0) return;
  struct Cand {
    uint64_t lo, end;
    uint32_t slot, entry;
    bool keep;
  };
  std::vector<Cand> cs;
  for (uint32_t j = 0; j < ns; ++j) {
    const uint32_t i = sel ? sel[j] : j;
    if (i >= n) continue;
    const flate_hip_zip_entry &e = ent[i];
    if (e.status != 0 || e.method != 8 || e.comp_size < unit_min) continue;
    if (zip_units_too_large(e.size, e.method, e.comp_size)) continue;
    cs.push_back({e.data_off, e.data_off + e.comp_size, j, i, true});
  }
  // the first occurrence of an entry number (sel alone can repeat one)
  if (sel) {
    std::vector<uint32_t> order(cs.size());
    for (uint32_t k = 0; k < order.size(); ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
      return cs[a].entry != cs[b].entry ? cs[a].entry < cs[b].entry : cs[a].slot < cs[b].slot;
    });
    for (size_t k = 1; k < order.size(); ++k)
      if (cs[order[k]].entry == cs[order[k - 1]].entry) cs[order[k]].keep = false;
  }
  // overlap among the ones left (ranges of at least one byte), sorted by lo: a range overlaps one in front of it iff
  // it starts below the largest end in front of it, and one behind it iff it ends above the next one's start (every
  // later one starts at or above that).  Every range of an overlapping pair goes.
  {
    std::vector<uint32_t> order;
    for (uint32_t k = 0; k < cs.size(); ++k)
      if (cs[k].keep) order.push_back(k);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
      return cs[a].lo != cs[b].lo ? cs[a].lo < cs[b].lo : cs[a].slot < cs[b].slot;
    });
    uint64_t max_end = 0;
    for (size_t k = 0; k < order.size(); ++k) {
      Cand &c = cs[order[k]];
      if (c.lo < max_end) c.keep = false;
      if (k + 1 < order.size() && c.end > cs[order[k + 1]].lo) c.keep = false;
      if (c.end > max_end) max_end = c.end;
    }
  }
  for (const Cand &c : cs) {
    if (!c.keep) {
      ++*fallback;
      continue;
    }
    const uint32_t i = sel ? sel[c.slot] : c.slot;
    R.push_back({c.lo, c.end, (uint32_t)L.size(), 0});
    L.push_back({c.lo, c.end, ent[i].size, out_off[c.slot], c.slot, 0});
  }
  std::sort(R.begin(), R.end(), [](const ZuRange &a, const ZuRange &b) { return a.lo < b.lo; });
}

// THE HULL of a non-empty L: [*lo, *hi) in the archive; L and R are moved to count from *lo.
inline void zip_units_hull(std::vector<ZuEntry> &L, std::vector<ZuRange> &R, uint64_t *lo, uint64_t *hi) {
  uint64_t a = ~0ull, b = 0;
  for (const ZuEntry &e : L) a = e.lo < a ? e.lo : a, b = e.end > b ? e.end : b;
  for (ZuEntry &e : L) e.lo -= a, e.end -= a;
  for (ZuRange &r : R) r.lo -= a, r.end -= a;
  *lo = a, *hi = b;
}

// g from the decode rounds: entry_unit[e] = the first unit of L[e] (entry_unit[g_disc] = the units that were decoded),
// bad_unit = the first unit that failed TAIL or the round's check (0xffffffff: none).  L[e] is served iff every unit of
// it lies in front of bad_unit.
inline uint32_t zip_units_served(const uint64_t *entry_unit, uint32_t g_disc, uint32_t bad_unit) {
  uint32_t g = 0;
  while (g < g_disc && entry_unit[g + 1u] <= (uint64_t)bad_unit) ++g;
  return g;
}

}  // namespace flate
