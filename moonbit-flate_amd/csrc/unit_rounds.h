// unit_rounds.h -- the rounds every unit decoder runs (private, host only; flate_api_units.hip is the user).
//
// A call that decodes long DEFLATE data as units goes over them in rounds of "one_round_units": TAIL (every unit with a
// symbolic window), COMPOSE (a log-step scan of the tail functions between F[0] and F[1]), RESOLVE (the byte windows
// R[1 .. count] from the seed R[0]), then the call's own body -- DECODE and a check, or PACK and a gather.  The carve of
// c->d_one_dec, the shared parameter words, the loop and the body's decode parameters are written here once; what the
// calls differ in stays with them, as the hooks of unit_rounds.
#pragma once

#include "flate_ctx.h"
#include "unit_discovery_rule.h"
#include "window_compose.h"

namespace flate_host {

// the units of a round: the option, or all n of them when that is fewer (never 0: the arrays have a size)
inline uint32_t unit_per_round(const flate_hip_ctx *c, uint32_t n) {
  return n < c->one_round_units ? (n ? n : 1u) : c->one_round_units;
}

// What DECODE reports per piece of a round.
struct UnitResults {
  int32_t *status;
  uint64_t *out_len;
  int64_t *err_off;
  void take(Carve &k, size_t pieces) {
    k.take(status, pieces);
    k.take(out_len, pieces);
    k.take(err_off, pieces);
  }
};

// The pieces of a round as one_pieces_kernel and its kin write them (slots, histories), and -- dec != null -- what
// DECODE reports for them.  pieces: the most a round has.
inline void unit_pieces_take(Carve &k, flate::OneDecParams &D, UnitResults *dec, size_t pieces) {
  k.take(D.p_out_off, pieces + 1);
  k.take(D.p_dict_at, pieces);
  k.take(D.p_dict_len, pieces);
  if (dec) dec->take(k, pieces);
}

// c->d_one_dec as a call's arrays: the result words, whatever `front` takes (by default nothing), the two function
// arrays, the windows, the per-unit words of TAIL (n_units + 1 each), then whatever `tail` takes for the call's own rounds.
// R has per_round + 1 windows: R[0] is the seed and R[i + 1] the window behind unit i of the round, so R[count] is both
// the next round's seed and the 32 bytes behind the last run that a gather over R may touch (PACK).
template <class Tail, class Front = void (*)(Carve &)>
int unit_rounds_carve(flate_hip_ctx *c, flate::OneDecParams &D, uint32_t n_units, uint32_t per_round, Tail tail,
                      Front front = [](Carve &) {}) {
  const size_t fentries = (size_t)per_round * flate::kWinEntries;
  return carve(c, c->d_one_dec, [&](Carve &k) {
    k.take(D.dh, 1);
    front(k);
    k.take(D.F[0], fentries);
    k.take(D.F[1], fentries);
    k.take(D.R, ((size_t)per_round + 1) * flate::kWinEntries);
    k.take(D.status, (size_t)n_units + 1);
    k.take(D.err_off, (size_t)n_units + 1);
    k.take(D.produced, (size_t)n_units + 1);
    tail(k);
  });
}

// The seed of the first round, R[0]: in front of the data there is nothing, zeros.
inline int unit_zero_seed(flate_hip_ctx *c, const flate::OneDecParams &D) {
  HIP_TRY(c, hipMemsetAsync(D.R, 0, flate::kWinEntries, c->stream));
  return FLATE_HIP_OK;
}
// What TAIL reads in every call, the result words at "none" (first_bad, decode_bad) and -- zero_seed -- the first seed.
// stored_units: the rule the units were cut by, the context's option or a seek index's rule word.  No zero seed: the
// calls that read through a seek index (their load kernels write every seed), the build of the gzip file's index (it
// zeroes per round) and flate_hip_gzfile_read, which queues its own result words in front of unit_zero_seed.
inline int unit_dec_params(flate_hip_ctx *c, flate::OneDecParams &D, const uint8_t *in, const flate::FrameOne *one,
                           const uint64_t *unit_bit, const uint64_t *out_off, uint32_t stored_units, bool zero_seed) {
  D.in = in;
  D.one = one;
  D.unit_bit = unit_bit;
  D.out_off = out_off;
  D.unit_max = c->one_unit_max;
  D.stored_units = stored_units;
  HIP_TRY(c, hipMemsetAsync(D.dh, 0xff, sizeof(flate::OneDecHead), c->stream));
  return zero_seed ? unit_zero_seed(c, D) : FLATE_HIP_OK;
}
// ... and what one_check_kernel and the verdict kernels read in the calls that decode to output
inline void unit_verdict_params(flate::OneDecParams &D, uint64_t total, const UnitResults &per_unit, const flate::OneHead *head,
                                uint32_t wrap, uint64_t in_len) {
  D.total = total;
  D.d_status = per_unit.status;
  D.d_out_len = per_unit.out_len;
  D.head = head;
  D.wrap = wrap;
  D.in_len = in_len;
}

// TAIL over a round's units, in the build of the unit rule its parameters carry (the word PROBE ran with, so that both
// stop at the same bits)
inline void one_tail_launch(flate_hip_ctx *c, uint32_t n_blocks, const flate::OneDecParams &D) {
  if (D.stored_units)
    hipLaunchKernelGGL(flate::one_tail_kernel<true>, dim3(n_blocks), dim3(64), 0, c->stream, D);
  else
    hipLaunchKernelGGL(flate::one_tail_kernel<false>, dim3(n_blocks), dim3(64), 0, c->stream, D);
}

// a hook with nothing to do
inline int unit_no_hook(uint32_t, uint32_t) { return FLATE_HIP_OK; }

// THE ROUNDS over the units [lo, hi) of a call with n_total units, per_round at a time.  Per round, in this order:
// D.u0 / D.count; before(u0, count); TAIL; between(u0, count); COMPOSE and RESOLVE; body(u0, count); ONE
// hipGetLastError for all of the round's launches; the carry.  A hook returns a status, and anything but 0 ends the call.
//   tail_out_off  what TAIL takes for out_off -- offsets counted inside a unit's own member or entry, whose history is
//                 what that member has produced -- or null: D.out_off.
//   seed          null: the plain scan, every unit continues the one in front.  Else the SEGMENTED scan (the two
//                 kernels that take the marks): seed[i] != 0 marks a unit that starts a segment, and `between` or
//                 `before` is what writes the marks.
// THE CARRY: the window behind the round's last unit, R[count], seeds the next round as R[0].  It is copied only while
// units of the CALL follow (n_total; hi may be the end of one run of several): behind the call's last round R[count]
// has no reader, so the copy would be 32 KiB moved for nothing in front of the call's synchronisation.  A round whose
// first unit starts a member, an entry or a segment ignores slot 0: its seed mark keeps COMPOSE and RESOLVE from
// reaching in front of it, so what the carry left there is never read.
template <class Before, class Between, class Body>
int unit_rounds(flate_hip_ctx *c, flate::OneDecParams &D, const uint64_t *tail_out_off, const uint32_t *seed, uint32_t lo,
                uint32_t hi, uint32_t n_total, uint32_t per_round, Before before, Between between, Body body) {
  int rc;
  for (uint32_t u0 = lo; u0 < hi; u0 += per_round) {
    const uint32_t count = hi - u0 < per_round ? hi - u0 : per_round;
    D.u0 = u0;
    D.count = count;
    if ((rc = before(u0, count))) return rc;
    flate::OneDecParams T = D;
    if (tail_out_off) T.out_off = tail_out_off;
    one_tail_launch(c, count, T);
    if ((rc = between(u0, count))) return rc;
    const uint32_t entry_blocks = (uint32_t)(((uint64_t)count * flate::kWinEntries + 255) / 256);
    int cur = 0;
    for (uint32_t s = 1; s < count; s <<= 1, cur ^= 1) {
      if (seed)
        hipLaunchKernelGGL(flate::one_seek_compose_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.F[cur ^ 1],
                           seed, count, s);
      else
        hipLaunchKernelGGL(flate::one_compose_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.F[cur ^ 1], count, s);
    }
    if (seed)
      hipLaunchKernelGGL(flate::one_seek_resolve_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.R, seed, count);
    else
      hipLaunchKernelGGL(flate::one_resolve_kernel, dim3(entry_blocks), dim3(256), 0, c->stream, D.F[cur], D.R, count);
    if ((rc = body(u0, count))) return rc;
    HIP_TRY(c, hipGetLastError());
    if (u0 + count < n_total)
      HIP_TRY(c, hipMemcpyAsync(D.R, D.R + (size_t)count * flate::kWinEntries, flate::kWinEntries, hipMemcpyDeviceToDevice, c->stream));
  }
  return FLATE_HIP_OK;
}

// DECODE of a round: its n pieces as spliced streams of in[0, in_len) with dictionaries -- piece i starts at bit_off[i],
// ends at bit_end[i] (null: where the next starts; closed: the last one too, else it runs to BFINAL or its failure),
// has D.p_dict_len[i] bytes of history at R + D.p_dict_at[i] and the slot [out_off[i], out_off[i + 1]) of out.
inline flate::InfParams unit_decode_params(const flate::OneDecParams &D, const uint8_t *in, uint64_t in_len,
                                           const uint64_t *bit_off, const uint64_t *bit_end, bool closed, uint32_t n,
                                           uint8_t *out, const uint64_t *out_off, const UnitResults &res) {
  flate::InfParams I{};
  I.in = in;
  I.in_len = in_len;
  I.bit_off = bit_off;
  I.bit_end = bit_end;
  I.closed = closed ? 1u : 0u;
  I.n_streams = n;
  I.out = out;
  I.out_off = out_off;
  I.out_len = res.out_len;
  I.status = res.status;
  I.err_off = res.err_off;
  I.dict_buf = D.R;
  I.dict_at = D.p_dict_at;
  I.dict_len = D.p_dict_len;
  return I;
}
// ... through the decoder the unit route names (of several rounds the inflate stage's time is the last one's)
inline int unit_decode(flate_hip_ctx *c, const flate::InfParams &I) {
  return launch_decoders(c, flate::inflate_route_units(c->inflate, c->num_cus, I.n_streams), I, true);
}

// THE TWO DECODE BODIES of the calls that deliver output, as unit_rounds' `body`.  The CHAIN form (one stream, whole or
// in parts): one_pieces_kernel writes the round's pieces, every piece ends where the next unit starts, and the round's
// last one too when `closed` -- else it runs to BFINAL or to its failure; raw[0, raw_len) is the raw stream.
inline int unit_decode_chain(flate_hip_ctx *c, const flate::OneDecParams &D, const uint8_t *raw, uint64_t raw_len, uint32_t u0,
                             uint32_t count, bool closed, uint8_t *d_out, const UnitResults &dec) {
  const uint32_t unit_blocks = (count + 1u + 255u) / 256u;
  hipLaunchKernelGGL(flate::one_pieces_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, D);
  const int r = unit_decode(c, unit_decode_params(D, raw, raw_len, D.unit_bit + u0, nullptr, closed, count, d_out, D.p_out_off, dec));
  if (r) return r;
  hipLaunchKernelGGL(flate::one_check_kernel, dim3(unit_blocks), dim3(256), 0, c->stream, D);
  return FLATE_HIP_OK;
}
// ... and the MEMBER form (a gzip file, whole or in parts): the call's `between` hook has written the pieces, each with
// its own start and end (p_bit_off / p_bit_end)
inline int unit_decode_members(flate_hip_ctx *c, const flate::OneDecParams &D, const uint8_t *in, uint64_t in_len,
                               const uint64_t *p_bit_off, const uint64_t *p_bit_end, uint32_t count, uint8_t *d_out,
                               const UnitResults &dec) {
  const int r = unit_decode(c, unit_decode_params(D, in, in_len, p_bit_off, p_bit_end, false, count, d_out, D.p_out_off, dec));
  if (r) return r;
  hipLaunchKernelGGL(flate::one_check_kernel, dim3((count + 1u + 255u) / 256u), dim3(256), 0, c->stream, D);
  return FLATE_HIP_OK;
}

// WHERE A CALL DECODES TO: the caller's device buffer, or the ctx's staged output grown to total + 16 bytes
inline int unit_out_buffer(flate_hip_ctx *c, uint8_t *out, bool dev, uint64_t total, uint8_t *&d_out) {
  d_out = out;
  if (dev) return FLATE_HIP_OK;
  const int rc = ensure(c, c->d_out, total + 16);
  if (rc == FLATE_HIP_OK) d_out = (uint8_t *)c->d_out.p;
  return rc;
}
// ... and the result brought down ONCE, behind the read-back of the call's result words: got bytes into a host
// caller's out, synchronised
inline hipError_t unit_bring_down(flate_hip_ctx *c, uint8_t *out, const uint8_t *d_out, bool dev, uint64_t got) {
  if (dev || !got) return hipSuccess;
  const hipError_t e = hipMemcpyAsync(out, d_out, got, hipMemcpyDeviceToHost, c->stream);
  return e != hipSuccess ? e : hipStreamSynchronize(c->stream);
}
// ... by a whole call: got, which a sound call never reports above total (FLATE_HIP_E_INTERNAL), is *out_len
inline int unit_deliver(flate_hip_ctx *c, uint8_t *out, const uint8_t *d_out, bool dev, uint64_t got, uint64_t total,
                        uint64_t *out_len) {
  if (got > total) return FLATE_HIP_E_INTERNAL;
  *out_len = got;
  HIP_TRY(c, unit_bring_down(c, out, d_out, dev, got));
  return FLATE_HIP_OK;
}

// ---- what the two readers in parts share (flate_hip_one_reader_*, flate_hip_gzfile_reader_*) ----

// What every handle holds: the ctx, the caller's flags, the unit rule and "one_unit_max" of the ctx AT OPEN, whatever it
// says later, and the device words that rest between two calls.
struct UnitReader {
  flate_hip_ctx *ctx = nullptr;
  uint32_t flags = 0;
  uint64_t unit_max = 0;
  uint32_t stored_units = 0;
  DevBuf state;
};
// open: a handle R with state_bytes of device words, made fresh by fresh(r) (which sets what R adds to the base)
template <class R, class Fresh>
int unit_reader_open(flate_hip_ctx *c, uint32_t flags, size_t state_bytes, Fresh fresh, R **out) {
  *out = nullptr;
  c->hip_err.clear();
  HIP_TRY(c, hipSetDevice(c->device));
  R *r = new R();
  r->ctx = c;
  r->flags = flags;
  r->unit_max = c->one_unit_max;
  r->stored_units = c->one_stored_units;
  int rc = ensure(c, r->state, state_bytes + 64);
  if (rc == FLATE_HIP_OK) rc = fresh(r);
  if (rc != FLATE_HIP_OK) {
    delete r;
    return rc;
  }
  *out = r;
  return FLATE_HIP_OK;
}
template <class R, class Fresh>
int unit_reader_reset(R *r, Fresh fresh) {
  if (!r) return FLATE_HIP_E_INVALID;
  flate_hip_ctx *c = r->ctx;
  c->hip_err.clear();
  HIP_TRY(c, hipSetDevice(c->device));
  return fresh(r);
}
template <class R>
void unit_reader_free(R *r) {
  if (!r) return;
  (void)hipSetDevice(r->ctx->device);
  delete r;
}

// THE SEED of a reader's first round, R[0]: the handle's window
inline int unit_window_seed(flate_hip_ctx *c, const flate::OneDecParams &D, const uint8_t *window) {
  HIP_TRY(c, hipMemcpyAsync(D.R, window, flate::kWinEntries, hipMemcpyDeviceToDevice, c->stream));
  return FLATE_HIP_OK;
}
// A reader's result, behind the read-back of its result words: got > total is FLATE_HIP_E_INTERNAL; THE CARRY back into
// the handle once the words are good (`sound`) -- the window behind the last of the n_dec units, which the round driver
// leaves in R[count] of the last round (nothing has been queued behind the rounds that writes D.R) --; then the result
// comes down.  All of it moves the handle's device words or follows work that did: whatever fails here is the caller's
// to end the handle with, so nothing is reported through HIP_TRY, and a copy that fails delivers nothing.
inline int unit_reader_deliver(flate_hip_ctx *c, const flate::OneDecParams &D, uint8_t *window, uint32_t n_dec, uint32_t per_round,
                               bool sound, uint8_t *out, const uint8_t *d_out, bool dev, uint64_t got, uint64_t total,
                               uint64_t *out_len) {
  if (got > total) return FLATE_HIP_E_INTERNAL;
  if (n_dec && sound) {
    const uint8_t *last = D.R + (size_t)flate::unit_last_count(n_dec, per_round) * flate::kWinEntries;
    if (hipMemcpyAsync(window, last, flate::kWinEntries, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) return FLATE_HIP_E_HIP;
  }
  *out_len = got;
  if (unit_bring_down(c, out, d_out, dev, got) == hipSuccess) return FLATE_HIP_OK;
  *out_len = 0;
  return FLATE_HIP_E_HIP;
}

// What TAIL found, read back behind the rounds: R.first_bad = the first unit that fails (0xffffffff: none) and, of that
// unit, R.status / R.err_off = the serial decoder's status at the serial offset.  word_of != null: a word per unit of
// the caller's, the failing unit's fetched into *word in the same read-back.
inline int unit_first_bad(flate_hip_ctx *c, const flate::OneDecParams &D, uint32_t n_units, flate::OneDecHead &R,
                          const uint32_t *word_of = nullptr, uint32_t *word = nullptr) {
  HIP_TRY(c, hipMemcpyAsync(&R, D.dh, sizeof R, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  R.status = 0, R.err_off = -1;
  if (R.first_bad == 0xffffffffu) return FLATE_HIP_OK;
  if (R.first_bad >= n_units) return FLATE_HIP_E_INTERNAL;
  HIP_TRY(c, hipMemcpyAsync(&R.status, D.status + R.first_bad, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&R.err_off, D.err_off + R.first_bad, 8, hipMemcpyDeviceToHost, c->stream));
  if (word_of) HIP_TRY(c, hipMemcpyAsync(word, word_of + R.first_bad, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return FLATE_HIP_OK;
}

}  // namespace flate_host
