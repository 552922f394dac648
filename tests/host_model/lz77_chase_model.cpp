// lz77_chase_model.cpp -- TEST INFRASTRUCTURE.  The chase over the fast events of a dense batch, one event per step
// and two (lz77_chase_rule.h, the header the kernels include), behind C entry points.  The arrays have 128 entries: the
// 64 lanes and, behind them, events that need the general path -- a chase that wrongly goes on past a stop (next start
// lanes reach 77) reads those and not foreign memory.  tests/test_lz77_chase_model.py also builds this file with
// -DCHASE_MUTANT_DROP_MIDDLE and with -DCHASE_MUTANT_IGNORE_STOP2 and expects the comparisons below to fail there.
#include <stdint.h>

#include "lz77_chase_rule.h"

using namespace flate;

namespace {

constexpr int kPad = 128;

void pair_words(const uint32_t *ev, uint32_t *ev2) {
  for (uint32_t l = 0; l < 64; ++l) ev2[l] = chase_pair(l, ev[l], ev[(ev[l] >> kEvNextShift) & 63u]);
  for (int l = 64; l < kPad; ++l) ev2[l] = kPairNone | kEvSlow;
}

void pad(const uint32_t *ev64, uint32_t *ev) {
  for (int l = 0; l < 64; ++l) ev[l] = ev64[l];
  for (int l = 64; l < kPad; ++l) ev[l] = 64u | kEvSlow;
}

bool same(const ChaseEnd &x, const ChaseEnd &y) { return x.vis == y.vis && x.mf == y.mf && x.a == y.a && x.exit == y.exit; }

// the word the dense batch builds for lane l (lz77_stream): a fast event has its match lane above l, 4 .. 15 bytes
uint32_t ev_word(uint32_t fv, uint32_t tf, bool slow, bool ends) {
  const uint32_t nxt = fv + tf - 1u;
  return (fv & 127u) | (tf << 8) | (slow ? kEvSlow : 0u) | (ends ? kEvEnds : 0u) |
         ((ends || nxt > (uint32_t)kDenseKeep) ? kEvStop : 0u) | ((nxt & 255u) << kEvNextShift);
}

uint64_t rng(uint64_t &s) {
  s ^= s << 13, s ^= s >> 7, s ^= s << 17;
  return s;
}

}  // namespace

// out[0..3] = {vis, mf, a, exit} of the one-event chase from lane a, out[4..7] = of the two-event chase.  Returns 1
// when they are equal.
extern "C" int chase_compare(const uint32_t *ev64, uint32_t a, uint64_t *out) {
  uint32_t ev[kPad], ev2[kPad];
  pad(ev64, ev);
  pair_words(ev, ev2);
  const ChaseEnd s = chase_single(ev, a), p = chase_paired(ev, ev2, a);
  out[0] = s.vis, out[1] = s.mf, out[2] = s.a, out[3] = s.exit;
  out[4] = p.vis, out[5] = p.mf, out[6] = p.a, out[7] = p.exit;
  return same(s, p) ? 1 : 0;
}

extern "C" uint32_t chase_pair_word(uint32_t lane, uint32_t ev_mine, uint32_t ev_next) {
  return chase_pair(lane, ev_mine, ev_next);
}

extern "C" uint32_t chase_ev_word(uint32_t fv, uint32_t tf, int slow, int ends) { return ev_word(fv, tf, slow != 0, ends != 0); }

// `count` random legal arrays, each chased from every start lane 0 .. kDenseKeep.  slow_pct: how many events in a
// hundred need the general path; short_pct: how many of the fast ones are 4 .. 7 bytes with the match lane right behind
// the start lane (long chains).  Returns the number of (array, start lane) pairs on which the two chases differ.
extern "C" uint64_t chase_random(uint64_t seed, uint32_t count, uint32_t slow_pct, uint32_t short_pct) {
  uint64_t st = seed * 0x9e3779b97f4a7c15ull + 1u, bad = 0;
  uint32_t ev[kPad], ev2[kPad], ev64[64];
  for (uint32_t it = 0; it < count; ++it) {
    for (uint32_t l = 0; l < 64; ++l) {
      const uint64_t r = rng(st);
      const bool slow = l == 63 || (r % 100u) < slow_pct;
      if (slow) {  // anything: no match lane at all, a long match, a shared slot in front of the match lane
        const uint32_t fv = (r >> 8) % 3u == 0 ? 64u : l + 1u + (uint32_t)((r >> 16) % (64u - l));  // l + 1 .. 64
        ev64[l] = ev_word(fv, 4u + (uint32_t)((r >> 24) % 13u), true, ((r >> 32) & 15u) == 0);
        ev64[l] |= (uint32_t)((r >> 40) & 1u) << 18;  // (stop means nothing on a slow event)
      } else {
        const bool sh = ((r >> 8) % 100u) < short_pct;
        const uint32_t fv = sh ? l + 1u : l + 1u + (uint32_t)((r >> 16) % (63u - l));
        const uint32_t tf = sh ? 4u + (uint32_t)((r >> 24) & 3u) : 4u + (uint32_t)((r >> 24) % 12u);
        ev64[l] = ev_word(fv, tf, false, ((r >> 32) & 63u) == 0);
      }
    }
    pad(ev64, ev);
    pair_words(ev, ev2);
    for (uint32_t a = 0; a <= (uint32_t)kDenseKeep; ++a) bad += same(chase_single(ev, a), chase_paired(ev, ev2, a)) ? 0 : 1;
  }
  return bad;
}
