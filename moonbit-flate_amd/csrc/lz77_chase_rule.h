// lz77_chase_rule.h -- the chase over the fast events of a dense batch (lz77_stream, lz77_kernels.hip), written
// ONCE: plain C++17 without HIP, compiled into the kernels and into tests/host_model/lz77_chase_model.cpp, which holds
// the two-event chase against the one-event chase on every field the batch reads afterwards.
//
// A dense batch gives every lane L the word ev[L] of "the event that would start with s-1 == L".  The chase starts at
// lane a and follows the fast events: visit a (VIS), note its match lane (MF), go to its next start lane -- until an
// event needs the general path or asks to stop.  One step is one v_readlane round trip, and the steps depend on each
// other.  The pair word ev2[L] = chase_pair(L, ev[L], ev[next lane of ev[L]]) states what up to TWO steps from L do, so
// the chase takes one round trip for them; it is a pure function of the 64 ev words.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define CHASE_HD __host__ __device__ inline
#else
#define CHASE_HD inline
#endif

namespace flate {

constexpr int kDenseKeep = 61;  // keep using a dense batch while the next s-1 lane <= this (58..61 measured: 61 best by 0.8 %)
// An event that starts at lane 62 or 63 has no scan lane left in its batch: the general path's probe masks would
// shift by 64 (undefined; the hardware shifts by 0) and the batch ends where it began -- the build with 62 hung its
// run (profiles/r05/README.md section 9).  The parser's progress guard (kStatusNoProgress) is the second line.
static_assert(kDenseKeep >= 0 && kDenseKeep <= 61, "an event must start at a lane that leaves it a scan lane (a + 2 <= 63)");

// ev, as the dense batch builds it:
//   [6:0]   fv   match lane of the event (64: none -- such an event is never fast)
//   [15:8]  tf   total match length (fast: 4 .. 15)
//   bit 16  the event needs the general path ("slow")
//   bit 17  the match ends the chunk
//   bit 18  stop chasing (bit 17, or the next start lane is above kDenseKeep)
//   [31:24] next start lane fv + tf - 1 (fast: at most 63 + 15 - 1 = 77)
constexpr uint32_t kEvSlow = 1u << 16, kEvEnds = 1u << 17, kEvStop = 1u << 18;
constexpr int kEvNextShift = 24;

// ev2, the pair word.  Bits 16 .. 18 and [6:0] sit where ev has them, so that the code behind the chase reads the last
// word of either chase alike:
//   [6:0]   fv2  match lane of the second event
//   [13:8]  fv1  match lane of the first event
//   bit 15  nothing to do: my own event is slow (bit 16 is set too); every other field is zero
//   bit 16  the chase ends at an event that needs the general path (at lane [31:25])
//   bit 17  the second event's match ends the chunk
//   bit 18  stop chasing after this word
//   [24:19] a1   start lane of the second event (<= kDenseKeep)
//   [31:25] the second event's next start lane (<= 77)
// A lane whose event is fast always has a word that does something.  Where it cannot state two events -- my event
// stops, or the event at my next lane is slow -- it states mine twice (a1 = my lane, fv1 = fv2): setting a bit of VIS
// or MF twice is setting it once, and the chase loop needs no second form of step.
constexpr uint32_t kPairNone = 1u << 15;
constexpr int kPairFv1Shift = 8, kPairA1Shift = 19, kPairNextShift = 25;
static_assert(kDenseKeep < 64 && 63 + 15 - 1 < 128, "a1 takes six bits and the next start lane seven");

// ev_next = ev[(ev_mine >> kEvNextShift) & 63] (looked at only where my event is fast and does not stop: its next
// start lane is then <= kDenseKeep).  Written as selects, not branches: on the device every lane computes its word
// at once.  (The form that leaves one OR and one select behind the shuffle, tools/experiments/chase_pair_or_form.patch,
// measured slower: profiles/r12/README.md section 3.)
// (CHASE_MUTANT_*: tests/test_lz77_chase_model.py builds the model with each and must see it fail.)
CHASE_HD uint32_t chase_pair(uint32_t lane, uint32_t ev_mine, uint32_t ev_next) {
  const bool stop = (ev_mine & kEvStop) != 0, next_slow = (ev_next & kEvSlow) != 0;
  const bool two = !stop && !next_slow;           // my event and the one at its next lane
  const uint32_t last = two ? ev_next : ev_mine;  // the event the word ends with: fv2, ends, stop, next lane
#ifndef CHASE_MUTANT_IGNORE_STOP2
  uint32_t bits = last & (kEvEnds | kEvStop);
#else
  uint32_t bits = last & (two ? kEvEnds : (kEvEnds | kEvStop));
#endif
  if (!stop && next_slow) bits = kEvSlow | kEvStop;  // mine, and out to the general path at its next lane
  const uint32_t w = (last & 63u) | ((ev_mine & 63u) << kPairFv1Shift) | bits |
                     ((two ? ev_mine >> kEvNextShift : lane) << kPairA1Shift) |
                     ((last >> kEvNextShift) << kPairNextShift);
  return (ev_mine & kEvSlow) ? (kPairNone | kEvSlow) : w;
}

// What the batch reads behind the chase: the start lanes visited, the match lanes, the lane the chase ended at, and of
// the last word bit 16 and -- where bit 16 is clear -- bit 17.
struct ChaseEnd {
  uint64_t vis, mf;
  uint32_t a, exit;
};
CHASE_HD uint32_t chase_exit_bits(uint32_t x) { return (x & kEvSlow) ? kEvSlow : (x & kEvEnds); }

// the one-event chase: x = ev[a]; slow => out; visit a, note fv, a = next; stop => out
CHASE_HD ChaseEnd chase_single(const uint32_t *ev, uint32_t a) {
  ChaseEnd r = {0, 0, a, 0};
  for (;;) {
    const uint32_t x = ev[r.a];
    r.exit = chase_exit_bits(x);
    if (x & kEvSlow) return r;
    r.vis |= 1ull << r.a;
    r.mf |= 1ull << (x & 63u);
    r.a = x >> kEvNextShift;
    if (x & kEvStop) return r;
  }
}

// the two-event chase over ev2[L] = chase_pair(L, ev[L], ev[(ev[L] >> 24) & 63]).  A word with kPairNone falls back to
// the single step from ev, which is the way out (the event is slow); the kernel leaves on the pair word itself.
CHASE_HD ChaseEnd chase_paired(const uint32_t *ev, const uint32_t *ev2, uint32_t a) {
  ChaseEnd r = {0, 0, a, 0};
  for (;;) {
    const uint32_t x = ev2[r.a];
    if (x & kPairNone) {
      const uint32_t y = ev[r.a];
      r.exit = chase_exit_bits(y);
      if (y & kEvSlow) return r;
      r.vis |= 1ull << r.a;
      r.mf |= 1ull << (y & 63u);
      r.a = y >> kEvNextShift;
      if (y & kEvStop) return r;
      continue;
    }
    r.exit = chase_exit_bits(x);
#ifndef CHASE_MUTANT_DROP_MIDDLE
    r.vis |= (1ull << r.a) | (1ull << ((x >> kPairA1Shift) & 63u));
#else
    r.vis |= 1ull << r.a;
#endif
    r.mf |= (1ull << ((x >> kPairFv1Shift) & 63u)) | (1ull << (x & 63u));
    r.a = x >> kPairNextShift;
    if (x & kEvStop) return r;
  }
}

}  // namespace flate
