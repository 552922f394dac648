// inflate_stream_kernel.inc -- ONE long DEFLATE stream decoded in pieces (included by
// inflate_kernels.hip: it uses that file's decoder tables, bit reader, huff_sym and the reader steps
// next to it -- read_block_header, read_stored_len, read_tables, read_copy, restage).
//
// The reference's Decompressor is resumable: read() runs the step functions until the 32 KiB
// window has something to hand out and remembers where it stopped -- step / step_state, the bit
// buffer b / nb, copy_len / copy_dist, the Huffman tables h1 / h2 of the block in progress, the
// window and final_flag (inflate.mbt:252-290,382-407; dict-decoder.mbt:29-60).  This kernel is the
// one-symbol reader of inflate_kernel with exactly that state resting in global memory between
// launches: every call presents the next bytes of the compressed stream and room for output, the
// wavefront decodes until one of them runs out and writes its state back.
//
//   input:  the bytes start with the byte that holds the first unconsumed bit (bit_in_byte of
//           its bits are already consumed).  Unless the caller has said that nothing follows
//           (final_in), a token is only started while 8 more bytes are there and a block header
//           while 600 are (the longest dynamic header is 286 bytes), so nothing is ever decoded from
//           a half-presented token; the call then ends with the bytes it did not use reported back.
//           A token boundary is also where the reference's byte-at-a-time reader holds fewer than
//           8 bits, so roffset = the bytes consumed, rounded up: error offsets stay the reference's.
//   output: a copy that does not fit rests as {copy_left, copy_dist} (the reference's copy_len /
//           copy_dist); with the output full the decoder still reads on through tokens that
//           produce nothing (end of block, the next header), so that the end of the stream is
//           reported together with the last bytes, as Decompressor::read does (:394-397).
//
// State header (the first 64 bytes; the host reads them back after every call).
struct InfStreamHead {
  uint64_t total_in;     // bytes of the stream consumed by all calls so far
  uint64_t total_out;
  int64_t err_off;       // corrupt_input_error's offset (inflate.mbt:38), absolute in the stream
  int32_t status;        // 0 = call again, 1 = the final block is done, < 0 sticky error
  uint32_t in_used;      // of the last call: bytes of `in` consumed ...
  uint32_t out_len;      // ... and bytes written to `out`
  uint32_t bit_in_byte;  // bits of in[in_used] already consumed (0..7); that byte is NOT in in_used
  uint32_t phase;        // 0 a block header is next, 1 inside a Huffman block, 2 inside a stored block
  uint32_t final_block;
  uint32_t stored_left;
  uint32_t copy_left, copy_dist;
  int32_t lit_min, lit_max, dist_min, dist_max;
  uint32_t dict_len;     // bytes of a preset dictionary that sit in the window in front of the output (<= kWin)
};

struct InfStreamState {
  InfStreamHead h;
  Dec lit, dist;
  uint8_t win[kWin];
};

size_t inflate_stream_state_bytes() { return sizeof(InfStreamState); }

// A fresh decoder (Decompressor::new / reset, inflate.mbt:320-343,862-884).  A preset dictionary
// (&Reader::new_dict :315-317) is history that "has already been read": DictDecoder::new
// (dict-decoder.mbt:40-60) copies its last 32768 bytes into the window and starts writing behind
// them -- here output byte k of the stream lives at window index dict_len + k.
__global__ void inflate_stream_init_kernel(void *state, const uint8_t *dict, uint32_t dict_len) {
  InfStreamState *st = reinterpret_cast<InfStreamState *>(state);
  uint32_t *p = reinterpret_cast<uint32_t *>(state);
  for (uint32_t i = threadIdx.x; i < sizeof(InfStreamHead) / 4; i += blockDim.x) p[i] = 0;
  for (uint32_t i = threadIdx.x; i < dict_len; i += blockDim.x) st->win[i] = dict[i];
  __syncthreads();
  if (threadIdx.x == 0) st->h.dict_len = dict_len;
}

__global__ __launch_bounds__(64) void inflate_stream_kernel(void *state, const uint8_t *in, uint32_t in_len,
                                                            uint32_t final_in, uint8_t *out, uint32_t out_cap) {
  __shared__ InfShared sh;
  InfStreamState *st = reinterpret_cast<InfStreamState *>(state);
  const int lane = threadIdx.x;
  InfStreamHead h = st->h;
  if (h.status != 0) {  // sticky (the host does not launch then; kept for safety)
    if (lane == 0) st->h.in_used = st->h.out_len = 0;
    return;
  }
  // state -> LDS
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(st->win);
    uint4 *dst = reinterpret_cast<uint4 *>(sh.win);
    for (int i = lane; i < kWin / 16; i += 64) dst[i] = src[i];
    if (h.phase == 1) {
      const uint32_t *a = reinterpret_cast<const uint32_t *>(&st->lit);
      uint32_t *b0 = reinterpret_cast<uint32_t *>(&sh.lit);
      for (int i = lane; i < (int)(sizeof(Dec) / 4); i += 64) b0[i] = a[i];
      const uint32_t *c = reinterpret_cast<const uint32_t *>(&st->dist);
      uint32_t *d0 = reinterpret_cast<uint32_t *>(&sh.dist);
      for (int i = lane; i < (int)(sizeof(Dec) / 4); i += 64) d0[i] = c[i];
    }
  }
  __syncthreads();

  const uint32_t bib = h.bit_in_byte;
  Bits b;
  b.in_len = in_len;
  b.roff = bib ? 1u : 0u;  // the reference's reader has pulled the byte it is half-way through
  b.ipos = 0;
  b.sbase = 0;
  b.buf = 0;
  b.cnt = 0;
  b.avail = bib ? (int)(8u - bib) : 0;
  // (the host presents at least that half-consumed byte whenever bit_in_byte != 0)
  uint32_t opos = 0, fpos = 0;  // bytes produced / flushed in THIS call
  const uint32_t wbase = (uint32_t)h.total_out + h.dict_len;  // window index of this call's first byte
  const uint32_t hist0 = h.total_out + h.dict_len >= (uint64_t)kWin ? (uint32_t)kWin : (uint32_t)h.total_out + h.dict_len;
  int err = 0;
  bool suspend = false;
  uint32_t phase = h.phase, stored_left = h.stored_left;
  bool final_block = h.final_block != 0;
  uint32_t copy_left = h.copy_left, copy_dist = h.copy_dist;
  int lit_min = h.lit_min, lit_max = h.lit_max, dist_min = h.dist_min, dist_max = h.dist_max;
  bool done = false;

  auto flush = [&]() {
    __syncthreads();
    for (uint32_t i = fpos + lane; i < opos; i += 64) out[i] = sh.win[(wbase + i) & (kWin - 1)];
    fpos = opos;
  };
  // in front of every symbol: the state pinned to the scalar unit (bits_pin), the stage refilled
  auto step = [&]() {
    bits_pin(b);
    opos = uni(opos);
    fpos = uni(fpos);
    err = (int)uni((uint32_t)err);
    phase = uni(phase);
    copy_left = uni(copy_left);
    stored_left = uni(stored_left);
    if (stage_low(b)) restage(b, sh.stage, in, lane);
  };
  // bits of the presented input that are not consumed yet
  auto bits_left = [&]() -> int64_t { return 8ll * (int64_t)in_len - (8ll * (int64_t)b.roff - (int64_t)b.avail); };

  restage(b, sh.stage, in, lane);
  if (bib) {  // the consumed bits of the first byte
    b.buf >>= bib;
    b.cnt -= (int)bib;
    if (b.cnt <= 32) bits_refill(b, sh.stage);
  }

  while (!err && !suspend && !done) {
    step();
    if (opos - fpos >= (uint32_t)kFlushAt) flush();

    if (copy_left) {  // copy_history (inflate.mbt:689-704): as much as the output takes
      const uint32_t room = out_cap - opos;
      const uint32_t n = copy_left < room ? copy_left : room;
      if (n == 0) {
        suspend = true;
        break;
      }
      __syncthreads();
      const uint32_t op = wbase + opos;
      for (uint32_t i = lane; i < n; i += 64) {
        const uint32_t o = copy_dist >= n ? i : i % copy_dist;
        sh.win[(op + i) & (kWin - 1)] = sh.win[(op - copy_dist + o) & (kWin - 1)];
      }
      __syncthreads();
      opos += n;
      copy_left -= n;
      continue;
    }

    if (phase == 2) {  // copy_data (inflate.mbt:745-766): raw bytes, as many as are there and fit
      const uint32_t ip = b.roff;
      uint32_t n = stored_left;
      if (n > in_len - ip) n = in_len - ip;
      if (n > out_cap - opos) n = out_cap - opos;
      if (n > (uint32_t)kFlushAt) n = (uint32_t)kFlushAt;  // the window hands bytes on: never more than it holds unflushed
      __syncthreads();
      for (uint32_t i = lane; i < n; i += 64) sh.win[(wbase + opos + i) & (kWin - 1)] = in[ip + i];
      __syncthreads();
      opos += n;
      b.roff += n;
      stored_left -= n;
      if (opos - fpos >= (uint32_t)kFlushAt) flush();
      if (stored_left == 0) {
        phase = 0;
        b.ipos = b.roff;  // the bit reader restarts at the byte after the block
        b.buf = 0;
        b.cnt = 0;
        b.avail = 0;
        restage(b, sh.stage, in, lane);
        if (final_block) done = true;  // finish_block (:769-777)
      } else if (b.roff == in_len || opos == out_cap) {
        if (b.roff == in_len && final_in && opos < out_cap) {
          err = E_EOF;  // the input ends inside the block
        } else {
          suspend = true;
        }
      }
      continue;
    }

    if (phase == 0) {  // next_block (inflate.mbt:345-379)
      if (!final_in && bits_left() < 600 * 8) {
        suspend = true;
        break;
      }
      uint32_t typ;
      if ((err = read_block_header(b, sh.stage, final_block, typ))) break;
      if (typ == 0) {  // data_block (:708-742)
        const int n = read_stored_len(b, in);
        if (n < 0) {
          err = n;
          break;
        }
        b.avail = 0;  // "discard current half-byte"
        if (n == 0) {
          b.ipos = b.roff;
          b.buf = 0;
          b.cnt = 0;
          restage(b, sh.stage, in, lane);
          if (final_block) done = true;
        } else {
          stored_left = n;
          phase = 2;
        }
        continue;
      }
      int nlit;
      if ((err = read_tables(b, sh, typ, lane, step, lit_min, lit_max, dist_min, dist_max, nlit))) break;
      phase = 1;
      continue;
    }

    // phase 1: one token of read_literal (:565-684)
    if (!final_in && bits_left() < 64) {
      suspend = true;
      break;
    }
    const Bits saved = b;  // (no restage happens inside a token: `saved` stays valid)
    const int v = huff_sym(b, sh.lit, lit_min, lit_max, sh.stage, &err);
    if (v < 0) break;
    if (v < 256) {
      if (opos >= out_cap) {  // no room: the literal is read again by the next call
        b = saved;
        suspend = true;
        break;
      }
      if (lane == 0) sh.win[(wbase + opos) & (kWin - 1)] = (uint8_t)v;  // DictDecoder::write_byte
      ++opos;
      continue;
    }
    if (v == 256) {  // finish_block
      phase = 0;
      if (final_block) done = true;
      continue;
    }
    if (opos >= out_cap) {  // a copy produces at least three bytes
      b = saved;
      suspend = true;
      break;
    }
    int length, dist;
    if ((err = read_copy(b, sh.dist, dist_min, dist_max, sh.stage, v, length, dist))) break;
    uint32_t hist = hist0 + opos;  // hist_size (dict-decoder.mbt:63-69)
    if (hist > (uint32_t)kWin || hist < opos) hist = (uint32_t)kWin;
    if ((uint32_t)dist > hist) {
      err = E_CORRUPT;
      break;
    }
    copy_left = (uint32_t)length;
    copy_dist = (uint32_t)dist;
  }
  flush();
  // LDS -> state
  __syncthreads();
  {
    uint4 *dst = reinterpret_cast<uint4 *>(st->win);
    const uint4 *src = reinterpret_cast<const uint4 *>(sh.win);
    for (int i = lane; i < kWin / 16; i += 64) dst[i] = src[i];
    if (phase == 1) {
      uint32_t *a = reinterpret_cast<uint32_t *>(&st->lit);
      const uint32_t *b0 = reinterpret_cast<const uint32_t *>(&sh.lit);
      for (int i = lane; i < (int)(sizeof(Dec) / 4); i += 64) a[i] = b0[i];
      uint32_t *c = reinterpret_cast<uint32_t *>(&st->dist);
      const uint32_t *d0 = reinterpret_cast<const uint32_t *>(&sh.dist);
      for (int i = lane; i < (int)(sizeof(Dec) / 4); i += 64) c[i] = d0[i];
    }
  }
  if (lane == 0) {
    // consumed bits of this call's input; the byte that holds the next bit is presented again
    const uint64_t consumed = 8ull * b.roff - (uint64_t)b.avail;
    uint32_t used = (uint32_t)(consumed >> 3), nbib = (uint32_t)(consumed & 7u);
    if (err || done) {  // the reader's roffset (:260): every byte it has pulled
      used = b.roff;
      nbib = 0;
    }
    h.in_used = used;
    h.out_len = opos;
    h.total_in += used;
    h.total_out += opos;
    h.bit_in_byte = nbib;
    h.phase = phase;
    h.final_block = final_block;
    h.stored_left = stored_left;
    h.copy_left = copy_left;
    h.copy_dist = copy_dist;
    h.lit_min = lit_min;
    h.lit_max = lit_max;
    h.dist_min = dist_min;
    h.dist_max = dist_max;
    h.status = err ? err : (done ? 1 : 0);
    h.err_off = err == E_CORRUPT ? (int64_t)(h.total_in) : -1;
    st->h = h;
  }
}
