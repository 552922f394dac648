// one_probe_kernel.inc -- part of inflate_kernels.hip (it uses the shared reader: read_block_header, read_stored_len,
// read_tables, read_copy, huff_sym).  ONE walk over a unit, one wavefront per unit, in two builds: the PROBE of
// flate_hip_inflate_one_index decodes the raw stream from a candidate's BIT to the next dynamic block header (or
// through the final block; with the option "one_stored_units" to the next dynamic OR STORED header) and reports where
// it stopped and how many bytes it produced; the TAIL of flate_hip_inflate_one is the same walk with a symbolic window
// (below).
//
// The bits a DEFLATE stream consumes never depend on its history, so the probe keeps none: no window, no distance
// check, no stores -- a decoy can write nothing -- and 6.5 KiB of LDS.  The reader starts in the state the serial
// decoder has at a block boundary at that bit (roff = the bytes that hold the bits in front, avail = what is left of
// the last of them), so every accept / reject decision and every error offset is the serial decoder's.  Every loop
// consumes input bits or ends: a probe is bounded by the raw stream's length.
template <bool SYM>
struct WalkShared {
  Dec lit, dist;
  uint8_t lens[kMaxLit + kMaxDist + 2 + 288];
  uint32_t stage[kStage / 4];
  uint16_t win[SYM ? kWin : 1];  // SYM: window_compose.h entries
};

struct OneWalk {      // what a walk left (uniform over the wavefront)
  uint64_t base;      // the byte the unit starts in, counted from the raw stream's first byte
  uint64_t end_bit;   // where it stopped: in front of a unit-starting header, or behind the final block
  uint64_t out;       // bytes it inflates to
  int64_t err_off;    // counted from the raw stream's first byte, or -1
  int32_t status;     // 0, FLATE_HIP_E_CORRUPT / _UNEXPECTED_EOF / _TOO_LARGE
  bool final_block;   // it ended with BFINAL
};

// The walk from bit `start` of the raw stream raw[0, raw_len).  SYM (TAIL): sh.win holds 16-bit entries -- a literal
// byte, or "byte j of the 32 KiB in front of this unit" --, starts as the identity, copies move entries as they move
// bytes, and the serial decoder's distance rule is applied with the history the unit really has, min(32768, ooff +
// bytes produced): the one verdict that depends on history comes out where the reference says so.  On return entry
// (out + j) & (kWin - 1) of sh.win is the byte kWin - j places in front of the unit's end.
// STORED (the option "one_stored_units", or the rule a seek index was built with): a stored header ends the unit as a
// dynamic one does; the walk only becomes shorter.  A template flag, not a run-time test: the builds for dynamic headers
// alone are instruction for instruction what they were before the option existed (a wave-uniform test of a parameter
// word cost the default path 0.7 % of a whole call, DESIGN.md 4.5).  The host picks PROBE's and TAIL's build from the
// same word (OneParams / OneDecParams::stored_units), so they stop at the same bits.
template <bool SYM, bool STORED>
FLATE_D OneWalk one_walk(WalkShared<SYM> &sh, const uint8_t *raw, uint64_t raw_len, uint64_t unit_max, uint64_t start,
                         uint64_t ooff, int lane) {
  uint64_t base = start >> 3;  // the reader counts bytes from here: 32 bits are enough for one unit
  uint32_t k = (uint32_t)start & 7u;
  if (base >= raw_len) base = raw_len, k = 0;  // (only bit 0 of an empty stream; a start is below the stream's end)
  const uint64_t left = raw_len - base;
  const bool clipped = left > unit_max;
  const uint8_t *in = raw + base;

  Bits b;
  b.in_len = (uint32_t)(clipped ? unit_max : left);
  b.roff = k ? 1u : 0u;
  b.ipos = 0;
  b.sbase = 0;
  b.buf = 0;
  b.cnt = 0;
  b.avail = k ? 8 - (int)k : 0;
  uint64_t opos = 0;
  int err = 0;
  bool final_block = false;
  if constexpr (SYM)
    for (uint32_t j = lane; j < (uint32_t)kWin; j += 64) sh.win[j] = wc_identity(j);
  auto step = [&]() {
    bits_pin(b);
    err = (int)uni((uint32_t)err);
    if (stage_low(b)) restage(b, sh.stage, in, lane);
  };
  restage(b, sh.stage, in, lane);  // (its barrier also publishes the window)
  b.buf >>= k;  // the bits in front of the unit
  b.cnt -= (int)k;
  for (;;) {
    step();
    uint32_t typ;
    if ((err = read_block_header(b, sh.stage, final_block, typ))) break;
    if (typ == 0) {
      const int n = read_stored_len(b, in);
      if (n < 0) {
        err = n;
        break;
      }
      const uint32_t ip = b.roff, avail = b.in_len - ip;
      const uint32_t cnt = avail < (uint32_t)n ? avail : (uint32_t)n;
      if constexpr (SYM) {
        __syncthreads();
        for (uint32_t q = lane; q < cnt; q += 64) sh.win[(opos + q) & (kWin - 1)] = in[ip + q];
      }
      opos += cnt;
      b.roff += cnt;
      if (cnt < (uint32_t)n) {
        err = E_EOF;
        break;
      }
      b.ipos = b.roff;
      b.buf = 0;
      b.cnt = 0;
      b.avail = 0;
      restage(b, sh.stage, in, lane);
    } else {
      int lit_min, lit_max, dist_min, dist_max, nlit;
      if ((err = read_tables(b, sh, typ, lane, step, lit_min, lit_max, dist_min, dist_max, nlit))) break;
      for (;;) {
        step();
        const int v = huff_sym(b, sh.lit, lit_min, lit_max, sh.stage, &err);
        if (v < 0 || v == 256) break;
        if (v < 256) {
          if constexpr (SYM)
            if (lane == 0) sh.win[opos & (kWin - 1)] = (uint8_t)v;
          ++opos;
          continue;
        }
        int length, dist;
        if ((err = read_copy(b, sh.dist, dist_min, dist_max, sh.stage, v, length, dist))) break;
        if constexpr (SYM) {
          const uint64_t have = opos + ooff;  // hist_size = min(kWin, this)
          if ((uint64_t)dist > (have < (uint64_t)kWin ? have : (uint64_t)kWin)) {
            err = E_CORRUPT;
            break;
          }
          __syncthreads();
          for (int q = lane; q < length; q += 64) {
            const int o = dist >= length ? q : q % dist;
            sh.win[(opos + (uint64_t)q) & (kWin - 1)] = sh.win[(opos - (uint64_t)dist + (uint64_t)o) & (kWin - 1)];
          }
          __syncthreads();
        }
        opos += (uint32_t)length;
      }
      if (err) break;
    }
    if (final_block) break;
    // the next header: a dynamic one -- STORED: a stored one as well -- starts the next unit (the serial decoder asks
    // for the same three bits next)
    step();
    if (!bits_need(b, 3)) {
      err = E_EOF;
      break;
    }
    const uint32_t next_typ = bits_peek(b, 3) >> 1;
    if (next_typ == 2u || (STORED && next_typ == 0u)) break;
  }
  if constexpr (SYM) __syncthreads();
  OneWalk w;
  w.base = base;
  w.end_bit = 8ull * (base + b.roff) - (uint64_t)b.avail;
  w.out = opos;
  w.err_off = err == E_CORRUPT ? (int64_t)(base + b.roff) : -1;
  // In a clipped range (in_len == unit_max < the bytes left) E_EOF means exactly: the
  // reader asked for a byte at or beyond unit_max from the unit's first byte -- the three bits of the next header
  // included, which the serial decoder asks for as well.  The real end of the stream lies in no clipped range.
  w.status = err == E_EOF && clipped ? FLATE_HIP_E_TOO_LARGE : err;
  w.final_block = final_block && !err;
  return w;
}

// tail == 0: block c probes candidate c.  tail != 0 (one block): the chain stopped at head->tail_bit, a header of a
// unit-starting type that is no candidate -- the serial decoder fails there, and this probe's status and offset are its
// verdict.
template <bool STORED>
__global__ __launch_bounds__(64) void one_probe_kernel(OneParams P, uint32_t tail) {
  __shared__ WalkShared<false> sh;
  const int lane = threadIdx.x;
  const uint32_t c = blockIdx.x;
  uint64_t start;
  if (tail) {
    if (c != 0 || !P.head->tail) return;
    start = P.head->tail_bit;
  } else {
    if (c >= P.C.cap) return;
    start = P.C.cand_off[c];
  }
  const uint64_t raw_off = P.one->pay_off[0], raw_len = P.one->pay_end - raw_off;
  const OneWalk w = one_walk<false, STORED>(sh, P.C.in + raw_off, raw_len, P.unit_max, start, 0, lane);
  if (lane != 0) return;
  if (tail) {
    // (status 0 here = the rule refused a header the reader takes: the two disagree.  The CPU model holds the rule
    // against the reader's restatement at every bit offset; this word is the device's own detector.)
    P.head->h.rc = w.status ? w.status : FLATE_HIP_E_INTERNAL;
    P.head->h.err_off = w.err_off;
    P.head->h.out_bytes = 0;
    return;
  }
  OneProbe r;
  r.end_bit = w.end_bit;
  r.out = w.out;
  r.err_off = w.err_off;
  r.status = w.status;
  r.final_block = w.final_block ? 1u : 0u;
  P.probe[c] = r;
}

// ---- the decode of the units (flate_hip_inflate_one; flate_kernels.h: OneDecParams) ----

// TAIL: block i walks unit u0 + i with the symbolic window and stores its tail function: its final window as a function
// of the one in front.
template <bool STORED>
__global__ __launch_bounds__(64) void one_tail_kernel(OneDecParams D) {
  __shared__ WalkShared<true> sh;
  const int lane = threadIdx.x;
  const uint32_t i = blockIdx.x;
  if (i >= D.count) return;
  const uint32_t u = D.u0 + i;  // the unit, or (unit_list) its place in the list
  const uint32_t su = D.unit_list ? D.unit_list[u] : u;
  // Units behind a failure are not walked: their tail functions, and every window resolved from them, stay GARBAGE on
  // purpose -- one_pieces_kernel gives those units an empty slot, so nothing is decoded from such a window, and a
  // stale entry is a 15-bit index or a byte: composing it stays in bounds.  The word is read once: other workgroups of
  // this launch lower it meanwhile, but only to units of this round, which lie in front of every unit that a stale
  // value lets through.
  // A unit list is walked whole: a unit that fails there says that the index does not fit the stream, and the
  // segments behind it start from their own stored windows.
  if (!D.unit_list && u > uni(D.dh->first_bad)) return;
  const uint64_t raw_off = D.one->pay_off[0], raw_len = D.one->pay_end - raw_off;
  const OneWalk w = one_walk<true, STORED>(sh, D.in + raw_off, raw_len, D.unit_max, D.unit_bit[su], D.out_off[su], lane);
  uint16_t *t = D.F[0] + (uint64_t)i * kWin;  // entry j: the byte kWin - j places in front of the unit's end
  for (uint32_t j = lane; j < (uint32_t)kWin; j += 64) t[j] = sh.win[(w.out + j) & (kWin - 1)];
  if (lane == 0) {
    D.status[u] = w.status;
    D.err_off[u] = w.err_off;
    D.produced[u] = w.out;
    if (w.status) atomicMin(&D.dh->first_bad, u);
  }
}

// the two unit rules: dynamic headers alone (the default), dynamic and stored headers
template __global__ void one_probe_kernel<false>(OneParams P, uint32_t tail);
template __global__ void one_probe_kernel<true>(OneParams P, uint32_t tail);
template __global__ void one_tail_kernel<false>(OneDecParams D);
template __global__ void one_tail_kernel<true>(OneDecParams D);
