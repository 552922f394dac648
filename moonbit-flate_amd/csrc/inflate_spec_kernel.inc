// inflate_spec_kernel.inc -- included by inflate_kernels.hip (inside namespace flate, after the
// wave-per-stream kernel whose helpers it shares: Dec, dec_init, Bits, huff_sym and the reader steps
// next to it, uni, ld32g).
//
// Third inflater: one WAVEFRONT per stream, 64 sub-blocks of the bit stream decoded at once.
//
// The lane-per-stream kernel needs tens of thousands of streams to fill the chip (a lane decodes
// ~2 MB/s whatever the load), the wave-per-stream kernel above walks the bit stream on one lane
// (~1000 cycles per symbol).  This kernel splits the next 64 * kSub bits of the stream into 64
// sub-blocks, one per lane:
//  1. every lane decodes the tokens (literal, or length + distance with their extra bits) of its
//     sub-block one after the other, from a GUESSED first token start (the sub-block's first bit;
//     lane 0 knows its start), into its own token list in LDS, and notes where its last token ends;
//  2. Huffman streams resynchronise: a decoder started at a wrong bit falls in step with the real
//     token chain after ~60 bits (median; p99 ~460 on the headline text, tools/experiments/
//     sync_model.py), so most lanes END at the right bit even when they started at a wrong one.  Lane
//     L + 1 now compares its start with lane L's end and decodes again if they differ; this repeats
//     until no start changes (3-5 rounds) or kRounds is reached -- the lanes in front of the first
//     inconsistent one are exact either way, and the batch simply ends there;
//  3. the tokens of the consistent lanes are numbered (prefix sum of the lists' lengths), fetched 64
//     at a time in stream order, a second prefix sum gives their output offsets, and the bytes are
//     produced 64 per step, literals and copies alike: every output byte finds the token it belongs
//     to by a marker + prefix maximum, copies read the history.
//
// What stays exactly the reference's (inflate.mbt:345-854, dict-decoder.mbt:114-185):
//  * block headers, table construction, stored blocks, and every irregular token -- end of block,
//    an invalid code, a distance beyond the history, the end of the input or of the output slot --
//    go through the SAME one-symbol-at-a-time reader as the kernel above (huff_sym and the reader
//    steps next to it in inflate_kernels.hip, on Bits), so accept / reject decisions and error
//    offsets cannot differ: a lane whose list would contain such a token ends the batch in front of
//    itself;
//  * the fast path only runs where none of that can happen (every token it takes lies >= 64 bits in
//    front of the end of the input); it keeps the byte-at-a-time reader's `roffset`
//    (inflate.mbt:260,789,818-831) up to date as the bytes the bit requests of the last token taken
//    would have pulled (the requests grow monotonically along the chain), so an error raised later
//    reports the reference's offset.
// History: the last kSpecRing bytes of output live in an LDS ring (a copy reads them there); older
// history is read back from the output buffer itself, the loads left pending while the next chunk is
// prepared.  A copy whose source reaches into the 64-byte chunk being produced ends that chunk in
// front of itself (it starts the next one), so every byte a chunk reads is already there.

namespace {

// Template parameters of the kernel:
//  SUB   bits per sub-block: a multiple of 32 with an ODD number of dwords, so that the 64 lanes' reads
//        of the staged input (lane L reads around dword L * sub / 32) fall into different LDS banks.
//        SUB is the largest and the first size; a stream whose tokens are shorter than ~10 bits on
//        average goes down in steps of 64 bits (to 32), so that a list holds ~CAP / 2 tokens whatever
//        the data.
//  CAP   tokens a lane's list holds (odd: the lists are CAP dwords apart).  A list that is full ends
//        where it is (the next list goes on from there).
//  RING  bytes of recent output kept in LDS (a power of two).
// Two instances: batches that leave most SIMDs with one wavefront get long lists and a ring that holds
// most copies' sources (nothing hides a load's latency there); large batches get the small footprint
// (9 wavefronts per CU).
#ifndef FLATE_SPEC_ROUNDS
#define FLATE_SPEC_ROUNDS 8
#endif
#ifndef FLATE_SPEC_FULLS
#define FLATE_SPEC_FULLS 4  // lists that filled up in one batch before the sub-blocks get smaller
#endif
constexpr int kRounds = FLATE_SPEC_ROUNDS;  // decode rounds per batch (the first only measures: lists 0..kRounds-2 are exact at least)
static_assert(kRounds >= 2, "one measuring round + one decoding round");

template <int SUB, int CAP, int RING>
struct SpecShared {
  static_assert(SUB % 64 == 32, "sub-block = odd number of dwords, steps of two dwords");
  static_assert(CAP % 2 == 1, "odd list stride");
  static_assert((RING & (RING - 1)) == 0, "ring size");
  // bytes of compressed input staged: what a batch reads (64 sub-blocks + the 5-dword view of the
  // last lane), at least the exact reader's kStage
  static constexpr int kStageBytes = (64 * SUB / 8 + 64 + 255) / 256 * 256 > kStage ? (64 * SUB / 8 + 64 + 255) / 256 * 256 : kStage;
  static constexpr int kStageWords = kStageBytes / 4 + 6;
  Dec lit, dist;
  uint32_t stage[kStageWords];  // compressed input from byte `sbase` on (+ margin for 5-dword views)
  uint8_t ring[RING];
  union {
    uint8_t lens[kMaxLit + kMaxDist + 2 + 288];  // code lengths while a block's tables are built
    uint32_t tok[64 * CAP];  // lane L's tokens: ol | copy << 9 | bits << 10 | (literal or distance) << 16
  };
  // the literal/length table once more, with everything the sub-block decode needs in one word
  // (spec_lit_entry): what would be a dozen instructions per token on the (symbol, length) pair
  uint32_t lit32[kPrimSize];
  uint32_t mark[16];   // one byte per output byte of a chunk: 1 + lane of the token that starts there
  uint32_t lmark[16];  // one byte per token of a group: 1 + lane whose list starts there
};

// A code longer than the 9-bit table: canonical search, length by length (the exact reader's loop,
// huff_sym above).  -> (symbol << 4) | length, 0 = no such code.  v: >= 15 bits of the stream.
FLATE_D uint32_t spec_long(const Dec &d, uint32_t v, int dmax) {
  uint32_t code = __brev(v & (uint32_t)(kPrimSize - 1)) >> (32 - kPrimBits);
  for (int L = kPrimBits + 1; L <= dmax; ++L) {
    code = (code << 1) | ((v >> (L - 1)) & 1u);
    const uint32_t idx = code - d.first[L];
    if (idx < d.count[L]) return ((uint32_t)d.sorted[d.offs[L] + idx] << 4) | (uint32_t)L;
  }
  return 0u;
}

// A literal/length table entry, (symbol << 4) | code length as HuffmanDecoder keeps it (0 = no such
// code, kLongCode = longer than the table's 9 bits), as the sub-block decoder wants it: bits 0-3 code
// length, 4-5 kind (0 = end of block or invalid: not for the fast path, 1 = literal, 2 = length,
// 3 = a longer code), 8-10 number of extra bits, 16-24 the literal / the base length
// (inflate.mbt:600-640).
// table = true: `ent` is a table entry; false: the result of spec_long, where the value of kLongCode
// is symbol 0 with a 15-bit code.
FLATE_D uint32_t spec_lit_entry(uint32_t ent, bool table) {
  const uint32_t clen = ent & 15u, sym = ent >> 4;
  if (table && ent == (uint32_t)kLongCode) return 3u << 4;
  if (ent == 0u || sym == 256u || sym > 285u) return 0u;
  if (sym < 256u) return clen | (1u << 4) | (sym << 16);
  const uint32_t ls = sym - 257u;  // length code 0..28
  const uint32_t nx = ls < 8u || ls == 28u ? 0u : (ls >> 2) - 1u;
  const uint32_t lbase = ls == 28u ? 258u : (ls < 8u ? 3u + ls : 3u + ((4u + (ls & 3u)) << nx));
  return clen | (2u << 4) | (nx << 8) | (lbase << 16);
}

// inclusive wave prefix sum: six DPP adds (hand-written: the compiler's version of the update_dpp
// form spent four instructions per step in this kernel)
FLATE_D uint32_t spec_scan(uint32_t v) {
  asm volatile(
      "s_nop 1\n\t"
      "v_add_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\t"
      "v_add_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\t"
      "v_add_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\t"
      "v_add_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
      "s_nop 1\n\t"
      "v_add_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      : "+v"(v));
  return v;
}
template <int CTRL, int ROW_MASK>
FLATE_D uint32_t spec_dpp_max(uint32_t v) {
  const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
  return o > v ? o : v;
}
FLATE_D uint32_t spec_scan_max(uint32_t v) {  // inclusive wave prefix maximum
  v = spec_dpp_max<0x111, 0xf>(v);
  v = spec_dpp_max<0x112, 0xf>(v);
  v = spec_dpp_max<0x114, 0xf>(v);
  v = spec_dpp_max<0x118, 0xf>(v);
  v = spec_dpp_max<0x142, 0xa>(v);
  v = spec_dpp_max<0x143, 0xc>(v);
  return v;
}
FLATE_D uint32_t spec_max(uint32_t v) {
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
    v = o > v ? o : v;
  }
  return v;
}

}  // namespace

// DICT: with the preset dictionaries of InfParams -- the ring starts out holding the dictionary's tail (it
// holds [opos - kSpecRing, opos) in history positions, the dictionary at -dict_len .. -1), and a far
// source in front of the output reads the tail in memory.
template <int SUB, int CAP, int RING, bool DICT>
FLATE_D void inflate_spec(const InfParams &P, SpecShared<SUB, CAP, RING> &sh) {
  using Shared = SpecShared<SUB, CAP, RING>;
  constexpr uint32_t kSub = SUB;
  constexpr int kCap = CAP;
  constexpr int kSpecRing = RING;
  constexpr int kStageWords = Shared::kStageWords;
  const int lane = threadIdx.x;
  const uint32_t sid = blockIdx.x;
  if (sid >= P.n_streams) return;
  // size_only: the same decoding, no byte produced (token lengths are all a size needs: neither the
  // history nor the output exist) and no capacity limit: out_len becomes the size the stream inflates to
  const bool size_only = P.size_only != 0;
  uint8_t *out = size_only ? nullptr : P.out + P.out_off[sid];
  const uint64_t cap64 = size_only ? ~0ull : P.out_off[sid + 1] - P.out_off[sid];
  const uint32_t out_cap = cap64 > 0xfffffff0ull ? 0xfffffff0u : (uint32_t)cap64;
  // Spliced input (P.bit_off): the n_streams pieces of ONE DEFLATE stream; mine starts at bit g0 of it
  // and ends where the next one starts (always a block boundary), the last one at BFINAL.  Bit
  // positions are kept relative to the dword the piece starts in (32-bit arithmetic; byte alignment
  // relative to the whole stream is preserved, as stored blocks need it).
  const uint8_t *in;
  uint32_t in_len, start_bit = 0, stop_bit = ~0u;
  uint64_t in_base = 0;  // byte offset of `in` inside P.in (for the reported error offset)
  if (P.bit_off == nullptr) {
    in = P.in + P.in_off[sid];
    in_len = (uint32_t)((P.in_end ? P.in_end[sid] : P.in_off[sid + 1]) - P.in_off[sid]);  // < 2^28: checked by the host
  } else {
    const uint64_t g0 = P.bit_off[sid], g1 = P.bit_off[sid + 1];
    in_base = (g0 >> 5) * 4;
    in = P.in + in_base;
    start_bit = (uint32_t)(g0 - 8 * in_base);
    const uint64_t rest = P.in_len - in_base;
    in_len = rest < (1ull << 28) ? (uint32_t)rest : (1u << 28);
    if (sid + 1 != P.n_streams) stop_bit = (uint32_t)(g1 - 8 * in_base);  // piece < 2^28 B: host
  }

  Bits b;
  b.in_len = in_len;
  b.roff = (start_bit + 7u) >> 3;  // the reference's reader has pulled the byte the piece starts in
  b.ipos = 0;
  b.sbase = 0;
  b.buf = 0;
  b.cnt = 0;
  b.avail = (int)(8u * b.roff - start_bit);
  uint32_t opos = 0;      // bytes produced (all of them stored: there is no pending window)
  uint32_t done_pos = 0;  // output below this is known to have reached memory (see put_group)
  int err = 0;
  bool final_block = false;
  uint32_t dict_len = 0;  // DICT: the stream's dictionary tail, history positions -dict_len .. -1
  const uint8_t *dict_tail = nullptr;
  if constexpr (DICT) {
    dict_len = P.dict_len[sid];
    dict_tail = P.dict_buf + P.dict_at[sid];
  }
#ifdef FLATE_SPEC_STATS
  uint32_t st_batches = 0, st_rounds = 0, st_steps = 0, st_lanes = 0, st_tokens = 0, st_groups = 0, st_chunks = 0, st_exact = 0,
           st_far = 0, st_waits = 0, st_fill = 0, st_stop = 0, st_full = 0, st_check = 0, st_hazard = 0;
  uint32_t st_wsteps = 0, st_wlong = 0;
  uint64_t st_c1 = 0, st_c3 = 0, st_call = 0, st_cfill = 0, st_chdr = 0, st_cinit = 0;
  uint64_t st_lr_front = 0, st_lr_rounds = 0, st_lr_out = 0, st_lr_all = 0;
  uint32_t st_lr_steps = 0, st_lr_codes = 0;
  const uint64_t st_t0 = __builtin_readcyclecounter();
#define SPEC_STAT(x) (x)
#else
#define SPEC_STAT(x) ((void)0)
#endif

  // Stage the input from byte `base` (a multiple of 4) on; zeros behind the end of the input.
  auto stage_fill = [&](uint32_t base) {
    SPEC_STAT(++st_fill);
    __syncthreads();
    if (in_len >= 4u) {
#pragma unroll 4
      for (int k = lane; k < kStageWords; k += 64) {
        const uint32_t p = base + 4u * k;
        // (the last dword of the input is loaded from in_len - 4 and shifted into place)
        const uint32_t pp = p + 4u <= in_len ? p : in_len - 4u;
        const uint32_t w = p < in_len ? ld32g(in + pp) >> (8u * (p - pp)) : 0u;
        sh.stage[k] = w;
      }
    } else {
      for (int k = lane; k < kStageWords; k += 64) {
        const uint32_t p = base + 4u * k;
        uint32_t w = 0;
        for (uint32_t q = p; q < in_len; ++q) w |= (uint32_t)in[q] << (8 * (q - p));
        sh.stage[k] = w;
      }
    }
    __syncthreads();
    b.sbase = base;
  };
  // Point the bit reader at bit bp (inside the stage).  roff / avail, the reference reader's
  // bookkeeping, are not touched.
  auto bits_at = [&](uint32_t bp) {
    const uint32_t k = ((bp >> 3) - b.sbase) & ~3u;
    b.ipos = b.sbase + k;
    b.buf = 0;
    b.cnt = 0;
    bits_refill(b, sh.stage);
    const uint32_t d = bp - 8u * (b.sbase + k);  // < 32
    b.buf >>= d;
    b.cnt -= (int)d;
    if (b.cnt <= 32) bits_refill(b, sh.stage);
  };
  auto restage_at = [&](uint32_t bp) {
    stage_fill((bp >> 3) & ~3u);
    bits_at(bp);
  };
  auto bit_pos = [&]() { return 8u * b.ipos - (uint32_t)b.cnt; };
  auto pin = [&]() {
    bits_pin(b);
    opos = uni(opos);
    done_pos = uni(done_pos);
    err = (int)uni((uint32_t)err);
  };
  // in front of every code-length symbol (read_tables)
  auto step = [&]() {
    pin();
    if (stage_low(b)) restage_at(bit_pos());
  };

  // Bytes of history older than the LDS ring come back from the output buffer itself (written by
  // lanes of this wavefront: the CU's vector L1 is coherent for its own stores, and done_pos keeps a
  // load from overtaking a store still in flight).  That load takes a microsecond; nothing that follows needs
  // its result except the store of the bytes themselves, so both are left PENDING: the next chunk
  // (of this group, of the next one, or the exact reader's next byte) finds its tokens meanwhile and
  // completes them (ring + output) before it reads any history.
  bool pend = false;          // wave-uniform: a pending chunk exists
  bool pend_lane = false;     // my lane holds a pending byte ...
  uint32_t pend_val = 0;      // ... this one (the load's destination) ...
  uint32_t pend_at = 0;       // ... for this output index
  uint32_t pend_issue = 0;    // opos when the loads were issued: every store before them is older
  auto complete_pending = [&]() {
    if (!pend) return;
    if (pend_lane) {
      sh.ring[pend_at & (kSpecRing - 1)] = (uint8_t)pend_val;
      out[pend_at] = (uint8_t)pend_val;
    }
    // the loads have returned, so every store this wavefront issued before them has completed
    done_pos = pend_issue;
    pend = false;
    pend_lane = false;
  };
  // Store cnt <= 64 bytes (lane j holds byte j; lanes in `skip` are pending) at output position opos.
  auto put = [&](uint32_t v, uint32_t cnt, bool skip) {
    if ((uint32_t)lane < cnt && !skip && !size_only) {
      sh.ring[(opos + (uint32_t)lane) & (kSpecRing - 1)] = (uint8_t)v;
      out[opos + (uint32_t)lane] = (uint8_t)v;
    }
    opos += cnt;
  };
  // A group of tokens in stream order, one per lane (live; oo = output offset inside the group, ol =
  // bytes, tw = oo | copy << 15 | (literal or distance) << 16), produces T bytes at opos, in chunks
  // of up to 64.  A chunk ends in front of a copy whose source reaches into it, so every byte a
  // chunk reads lies below its first byte.
  auto put_group = [&](bool live, uint32_t oo, uint32_t ol, uint32_t tw, uint32_t T) {
    if (size_only) {
      opos += T;
      return;
    }
    SPEC_STAT(++st_groups);
    const uint32_t base0 = opos;
    const bool copy = live && (tw & 0x8000u);
    const uint32_t dist = tw >> 16;
    const uint32_t span = dist < ol ? dist : ol;
    uint32_t c_lo = 0;
    while (c_lo < T) {
      SPEC_STAT(++st_chunks);
      uint32_t c_hi = T - c_lo < 64u ? T : c_lo + 64u;
      // (source of a copy at oo: [oo - dist, oo - dist + span); it must end at or below c_lo unless
      // the copy is the chunk's first token -- then it ends at or below oo = c_lo anyway)
      const uint64_t O = __ballot(copy && oo > c_lo && oo < c_hi && oo + span > c_lo + dist);
      if (O) c_hi = (uint32_t)__builtin_amdgcn_readlane((int)oo, __builtin_ctzll(O));
      const uint32_t cnt = c_hi - c_lo;
      // the token every byte of this chunk belongs to: tokens mark the byte they start at with their
      // lane, the token that covers byte c_lo is the carry, a prefix maximum spreads the marks
      if (lane < 16) sh.mark[lane] = 0;
      if (live && oo - c_lo < cnt) reinterpret_cast<uint8_t *>(sh.mark)[oo - c_lo] = (uint8_t)(lane + 1);
      const uint64_t Bc = __ballot(live && oo <= c_lo);
      const uint32_t carry = 64u - (uint32_t)__builtin_clzll(Bc);  // (Bc != 0: the first token starts at 0)
      uint32_t m = reinterpret_cast<const uint8_t *>(sh.mark)[lane];
      if (lane == 0) m = m > carry ? m : carry;
      const uint32_t ow = spec_scan_max(m) - 1u;
      const uint32_t t = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(ow << 2), (int)tw);
      const uint32_t j = c_lo + (uint32_t)lane;
      const bool livej = (uint32_t)lane < cnt;
      const uint32_t val = t >> 16;
      const bool cpy = livej && (t & 0x8000u);
      uint32_t v = val;  // a literal
      uint32_t s = 0;
      if (cpy) {  // a copy of distance val: write_copy, dict-decoder.mbt:114-154
        uint32_t k = j - (t & 0x7fffu);
        if (k >= val) k %= val;  // overlapping copy = periodic extension of the val bytes in front
        s = base0 + (t & 0x7fffu) - val + k;
      }
      // the ring holds [opos - kSpecRing, opos) at this point (opos = base0 + c_lo)
      bool far = cpy && s + (uint32_t)kSpecRing < opos;
      bool in_dict = false;  // DICT: a far source in front of the output (opos - s: its distance from opos)
      if constexpr (DICT) {
        far = cpy && opos - s > (uint32_t)kSpecRing;
        in_dict = far && opos - s > opos;
      }
      // the far bytes of the chunk in front of this one (their loads had all of the above to arrive):
      // into the ring and the output before anything is read from the ring
      complete_pending();
      if (cpy && !far) v = sh.ring[s & (kSpecRing - 1)];
      if (__ballot(far)) {
        SPEC_STAT(++st_far);
        // a byte that left this wavefront only recently may still be on its way to memory
        if (__ballot(far && !in_dict && s >= done_pos)) {
          SPEC_STAT(++st_waits);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          done_pos = opos;
        }
        pend = true;
        pend_lane = far;
        pend_at = opos + (uint32_t)lane;
        pend_issue = opos;
      }
      put(v, cnt, far);
      if constexpr (DICT) {
        if (in_dict) pend_val = dict_tail[dict_len + s];  // (s < 0: wraps to the tail's index)
        else if (far) pend_val = out[s];
      } else {
        if (far) pend_val = out[s];  // (after the store of the chunk's other bytes: nothing is issued behind it)
      }
      c_lo = c_hi;
    }
  };

  if constexpr (DICT) {
    if (!size_only) {
      const uint32_t m = dict_len < (uint32_t)kSpecRing ? dict_len : (uint32_t)kSpecRing;
      for (uint32_t i = lane; i < m; i += 64) sh.ring[(i - m) & (kSpecRing - 1)] = dict_tail[dict_len - m + i];
    }
  }
  restage_at(start_bit);  // (its barrier also publishes the ring)
  while (!final_block && !err) {  // next_block (inflate.mbt:345-379)
    SPEC_STAT(st_chdr -= __builtin_readcyclecounter());
    pin();
    if (stop_bit != ~0u && bit_pos() >= stop_bit) {  // spliced input: the next piece starts here
      if (bit_pos() != stop_bit) err = E_CORRUPT;    // the index does not point at a block boundary
      break;
    }
    if (stage_low(b)) restage_at(bit_pos());
    uint32_t typ;
    if ((err = read_block_header(b, sh.stage, final_block, typ))) break;
    if (typ == 0) {  // data_block (:708-766): discard the partial byte, LEN, ~LEN, raw bytes
      const int n = read_stored_len(b, in);
      if (n < 0) {
        err = n;
        break;
      }
      const uint32_t ip = b.roff, avail = in_len - ip;
      const uint32_t cnt = avail < n ? avail : n;
      if (cnt > out_cap - opos) {
        err = E_OUT_SMALL;
        break;
      }
      complete_pending();
      if (size_only) {
        opos += cnt;
      } else {
        // whole KiB in front of the block's last kSpecRing bytes: 16 bytes per lane straight from the
        // input to the output (the ring only ever needs the end of the block) ...
        const uint32_t bulk = cnt > (uint32_t)kSpecRing ? (cnt - (uint32_t)kSpecRing) & ~1023u : 0u;
        for (uint32_t c0 = 0; c0 < bulk; c0 += 1024) {
          const uint8_t *src = in + ip + c0 + 16u * (uint32_t)lane;
          uint8_t *dst = out + opos + c0 + 16u * (uint32_t)lane;
          uint32_t w[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) w[k] = ld32g(src + 4 * k);
#pragma unroll
          for (int k = 0; k < 4; ++k) __builtin_memcpy(dst + 4 * k, &w[k], 4);
        }
        opos += bulk;
        // ... the rest through the ring, four chunks' loads in flight
        for (uint32_t c0 = bulk; c0 < cnt; c0 += 256) {
          uint32_t v[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const uint32_t i = c0 + 64u * k + (uint32_t)lane;
            v[k] = i < cnt ? in[ip + i] : 0u;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const uint32_t at = c0 + 64u * k;
            if (at < cnt) put(v[k], cnt - at < 64u ? cnt - at : 64u, false);
          }
        }
      }
      b.roff += cnt;
      if (cnt < n) {
        err = E_EOF;
        break;
      }
      b.avail = 0;
      restage_at(8u * b.roff);  // the bit reader restarts at the byte after the block
      SPEC_STAT(st_chdr += __builtin_readcyclecounter());
      continue;
    }
    int lit_min, lit_max, dist_min, dist_max, nlit;
    SPEC_STAT(st_cinit -= __builtin_readcyclecounter());  // (stats build: the whole tables read, either block type)
    if ((err = read_tables(b, sh, typ, lane, step, lit_min, lit_max, dist_min, dist_max, nlit))) break;
    // a dynamic block whose literal/length code stops at the end-of-block symbol
    // (write_block_huff, huffman-bit-writer.mbt:738-824: num_literals = 257)
    const bool lit_only = typ == 2 && nlit == 257;

    for (int i = lane; i < kPrimSize; i += 64) sh.lit32[i] = spec_lit_entry(sh.lit.prim[i], true);
    __syncthreads();
    SPEC_STAT(st_chdr += __builtin_readcyclecounter());
    SPEC_STAT(st_cinit += __builtin_readcyclecounter());
    for (;;) {  // read_literal (:565-684)
      pin();
      // ------------------------------ literal runs --------------------------------------
      // A block without length codes (the encoder's Huffman-only blocks: incompressible input) is a
      // string of literals whose 7/8/9-bit codes never fall in step with a decoder started at a
      // wrong bit: 64 sub-blocks buy nothing there (8 rounds settle ~18 lists).  Such a block is
      // decoded by POINTER JUMPING instead, ~60 literals per step:
      //  1. every bit offset i of a window of W = 63 * (shortest code) bits gets the code that WOULD
      //     start there: J1[i] = i + its length (a table in LDS, a few offsets per lane).  Offsets that
      //     cannot be jumped from -- behind the window, or a code that is not a literal (end of block,
      //     no such code) -- are absorbing: J1[i] = i;
      //  2. six rounds k = 0 .. 5 on the table J_(2^k) = J1 applied 2^k times: lane t jumps from its offset
      //     (0 at first) if bit k of t is set, so that it ends at the start of the t-th code, and the
      //     table is squared for the next round (one gather + one store per offset; a lane's offsets stay
      //     in its registers).  Eleven dependent LDS round trips, whatever the number of codes;
      //  3. a window holds at most 63 codes, so lane 63 always ends in the absorbing offset the chain
      //     leaves through: the next window's first code, or the token the exact reader has to look at;
      //  4. the lanes whose offset is a literal's start store its byte: lane t the t-th byte, one
      //     coalesced store.
      // (The first version of this path walked the code lengths of 64 offsets with a scalar chase,
      // v_readlane -> s_add -> lane select: ~85 cycles per code whatever the instruction count; it
      // took random bytes from 15.1 to 3.7 ms per 1024 streams.)
#ifndef FLATE_SPEC_NO_FAST
      if (lit_only) {
        uint32_t bp = bit_pos();
        uint32_t racc = 0;
        bool moved = false;
        const uint32_t safe_end = 8u * in_len > 64u ? 8u * in_len - 64u : 0u;
        constexpr uint32_t kTab = 1024u;        // offsets a window's tables hold (63 * 15 + 16 <= 1024)
        static_assert(3u * kTab * 2u + kTab * 2u <= sizeof(sh.tok), "the jump tables live in the token lists");
        uint32_t *const T0 = sh.tok;            // [kTab]: J1 | byte << 16 | absorbing << 24
        uint16_t *const Ja = reinterpret_cast<uint16_t *>(sh.tok + kTab);  // [kTab] J2
        uint16_t *const Jb = Ja + kTab;                                     // [kTab] J4
        const uint32_t cmin = (uint32_t)uni((uint32_t)sh.lit.min);          // shortest code of the block (>= 1)
        for (;;) {
          bp = uni(bp);
          if (bp >= safe_end || (!size_only && out_cap - opos < 64u)) break;
          // every code looked at starts below safe_end (the last codes of the input: the exact reader)
          uint32_t W = 63u * cmin;
          if (W > safe_end - bp) W = safe_end - bp;
          if (W < 32u) break;  // (1-bit codes: the window is 63 bits)
          const uint32_t m = (W + 16u + 63u) >> 6;  // table entries per lane (<= 16)
          if (((bp + 64u * (m > 8u ? 16u : 8u) + 31u - 8u * b.sbase) >> 5) + 2u > (uint32_t)kStageWords) stage_fill((bp >> 3) & ~3u);
          // My entries (offsets lane, 64 + lane, ...) stay in registers from round to round, eight at a time
          // with their LDS operations in flight together; the second eight only when the window has them
          // (entries behind the last one are absorbing and cost nothing but their slot).
          uint32_t jr[16];
          const bool two = m > 8u;
          SPEC_STAT(st_lr_all -= __builtin_readcyclecounter());
          SPEC_STAT(st_lr_front -= __builtin_readcyclecounter());
          // ---- 1. J1 and the bytes
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            if (g == 0 || two) {
              uint32_t v0[8], e32[8];
#pragma unroll
              for (int u = 0; u < 8; ++u) {
                const uint32_t q = bp + 64u * (8 * g + u) + (uint32_t)lane;
                const uint32_t idx = (q - 8u * b.sbase) >> 5;
                v0[u] = __builtin_amdgcn_alignbit(sh.stage[idx + 1], sh.stage[idx], q & 31u);
              }
#pragma unroll
              for (int u = 0; u < 8; ++u) e32[u] = sh.lit32[v0[u] & (kPrimSize - 1)];
              bool any_long = false;
#pragma unroll
              for (int u = 0; u < 8; ++u) {
                const uint32_t i = 64u * (8 * g + u) + (uint32_t)lane;
                const uint32_t kind = (e32[u] >> 4) & 3u;
                const bool lit = i < W && kind == 1u;
                any_long |= i < W && kind == 3u;
                jr[8 * g + u] = lit ? i + (e32[u] & 15u) : i;
                T0[i] = lit ? jr[8 * g + u] | (e32[u] & 0x00ff0000u) : i | (1u << 24);
              }
              // codes longer than the 9-bit table (rare symbols; mostly lanes that look at arbitrary bits):
              // resolved behind the straight-line part, which keeps its LDS operations in flight together
              if (__ballot(any_long)) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                  const uint32_t i = 64u * (8 * g + u) + (uint32_t)lane;
                  if (i < W && ((e32[u] >> 4) & 3u) == 3u) {
                    const uint32_t ee = spec_lit_entry(spec_long(sh.lit, v0[u], lit_max), false);
                    if (((ee >> 4) & 3u) == 1u) {
                      jr[8 * g + u] = i + (ee & 15u);
                      T0[i] = jr[8 * g + u] | (ee & 0x00ff0000u);
                    }
                  }
                }
              }
            }
          }
          __syncthreads();
          SPEC_STAT(st_lr_front += __builtin_readcyclecounter());
          SPEC_STAT(st_lr_rounds -= __builtin_readcyclecounter());
          // ---- 2 + 3. rounds k = 0 .. 5 on J_(2^k): lane t jumps if bit k of t is set, then the table is
          // squared (J_(2^(k+1)) [i] = J_(2^k) [J_(2^k) [i]]; my entries' gathers and the jump's in flight together)
          uint32_t pos = 0;
#pragma unroll
          for (int k = 0; k < 6; ++k) {
            const uint16_t *const tab = k == 0 ? nullptr : (((k - 1) & 1) ? Jb : Ja);
            auto at = [&](uint32_t x) -> uint32_t { return k == 0 ? (T0[x] & 0xffffu) : (uint32_t)tab[x]; };
            const uint32_t hop = at(pos);
            if (k < 5) {
#pragma unroll
              for (int u = 0; u < 8; ++u) jr[u] = at(jr[u]);
              if (two) {
#pragma unroll
                for (int u = 8; u < 16; ++u) jr[u] = at(jr[u]);
              }
              uint16_t *const nxt = (k & 1) ? Jb : Ja;
#pragma unroll
              for (int u = 0; u < 8; ++u) nxt[64u * u + (uint32_t)lane] = (uint16_t)jr[u];
              if (two) {
#pragma unroll
                for (int u = 8; u < 16; ++u) nxt[64u * u + (uint32_t)lane] = (uint16_t)jr[u];
              }
            }
            if (((uint32_t)lane >> k) & 1u) pos = hop;
            if (k < 5) __syncthreads();
          }
          pos &= kTab - 1u;
          const uint32_t mine = T0[pos];
          SPEC_STAT(st_lr_rounds += __builtin_readcyclecounter() + (mine & 0u));
          SPEC_STAT(st_lr_out -= __builtin_readcyclecounter());
          // (a literal's start: the offsets grow along the chain until it is absorbed, so these lanes
          // are lanes 0 .. cnt - 1)
          const uint64_t vm = __ballot(!((mine >> 24) & 1u));
          if (!(vm & 1ull)) break;  // the token at bp itself is for the exact reader
          const uint32_t cnt = (uint32_t)__builtin_popcountll(vm);
          const uint32_t exit_off = (uint32_t)__builtin_amdgcn_readlane((int)pos, 63);
          const uint32_t last_s = (uint32_t)__builtin_amdgcn_readlane((int)pos, (int)cnt - 1);
          const uint32_t last_l = exit_off - last_s;
          SPEC_STAT(++st_batches);
          if (!size_only) {
            complete_pending();
            if ((uint32_t)lane < cnt) {
              sh.ring[(opos + (uint32_t)lane) & (kSpecRing - 1)] = (uint8_t)(mine >> 16);
              out[opos + (uint32_t)lane] = (uint8_t)(mine >> 16);
            }
          }
          opos += cnt;
          // roffset after the last literal taken: huff_sym asks for max(lit_min, code length) bits (:803-854)
          racc = (bp + last_s + (last_l > (uint32_t)lit_min ? last_l : (uint32_t)lit_min) + 7u) >> 3;
          bp += exit_off;
          moved = true;
          SPEC_STAT(st_lr_out += __builtin_readcyclecounter());
          SPEC_STAT(st_lr_all += __builtin_readcyclecounter());
          SPEC_STAT(++st_lr_steps);
          SPEC_STAT(st_lr_codes += cnt);
          if (exit_off < W) break;  // absorbed inside the window: in front of a token that is not a literal
        }
        if (moved) {
          const uint32_t roff = racc > b.roff ? racc : b.roff;
          if ((bp >> 3) + (uint32_t)kStageMargin > b.sbase + (uint32_t)kStage) stage_fill((bp >> 3) & ~3u);
          bits_at(bp);
          b.roff = roff;
          b.avail = (int)(8u * roff - bp);
          pin();
        }
      } else
#endif
      // ------------------------------ fast batches --------------------------------------
      // While there is plenty of input: 64 sub-blocks per batch.  Left with `break` as soon as the
      // token at the front needs the exact reader below (which then handles exactly it).
      {
        uint32_t bp = bit_pos();
        uint32_t racc = 0;  // roffset after the last token taken
        bool moved = false;
        // a token that starts below this bit lies inside the input with all the bits the reference's
        // reader would ask for on its behalf (<= 48 bits of token, requests of <= 15 bits at a time)
        const uint32_t safe_end = 8u * in_len > 64u ? 8u * in_len - 64u : 0u;
        uint32_t sub = kSub;
        for (;;) {
          bp = uni(bp);
#ifdef FLATE_SPEC_NO_FAST  // (diagnostic build: every token through the exact reader)
          break;
#endif
          if (bp >= safe_end) break;
          uint32_t nl = (safe_end - bp + sub - 1u) / sub;  // sub-blocks that start below safe_end
          nl = nl < 64u ? nl : 64u;
          // (a lane keeps three dwords of the stage from the one that holds its bit on, and reads two ahead)
          if (((bp + 64u * sub + 63u - 8u * b.sbase) >> 5) + 5u > (uint32_t)kStageWords) stage_fill((bp >> 3) & ~3u);
          SPEC_STAT(++st_batches);
          SPEC_STAT(st_call -= __builtin_readcyclecounter());
          SPEC_STAT(st_c1 -= __builtin_readcyclecounter());

          // ---- 1. token lists, rounds until the starts agree with the ends in front of them
          const uint32_t sub_end = bp + ((uint32_t)lane + 1u) * sub;
          const uint32_t lim = sub_end < safe_end ? sub_end : safe_end;
          uint32_t st = bp + (uint32_t)lane * sub;  // where my list starts
          uint32_t e = st;    // where it ends: the start of the first token at or behind lim
          uint32_t n = 0;     // tokens in my list
          uint32_t osum = 0;  // bytes they produce
          uint32_t rl = 0;    // roffset after my last token
          uint32_t fl = 0;    // 1 = my list ends the batch: in front of a token that is not for this path; 2 = it is full
          bool redo = (uint32_t)lane < nl;
          bool have = false;  // my list's tokens are stored (round 0 only measures)
          bool ok = false;
          uint32_t* const mytok = sh.tok + lane * kCap;
          // One token from the 64 bits v1:v0 that start at its first bit.  FULL = false: only what the
          // chain needs (its length in bits, whether it is a token for this path at all).
          struct Tok {
            uint32_t clen, t1, dlen, tl;  // bits: literal/length code, + length extra, distance code, whole token
            uint32_t ol, val;             // FULL: bytes it produces, literal byte or distance
            bool is_lit, stop;            // stop: end of block or an invalid code -- not for this path
          };
          auto tok_decode = [&](uint32_t v0, uint32_t v1, auto full) {
            constexpr bool FULL = decltype(full)::value;
            Tok t;
            uint32_t e32 = sh.lit32[v0 & (kPrimSize - 1)];
            SPEC_STAT(st_wlong += (((e32 >> 4) & 3u) == 3u && (uint32_t)lane == (uint32_t)__builtin_ctzll(__ballot(((e32 >> 4) & 3u) == 3u))) ? 1u : 0u);
            if (((e32 >> 4) & 3u) == 3u) e32 = spec_lit_entry(spec_long(sh.lit, v0, lit_max), false);
            // (a lane decoding from a wrong start sees arbitrary bits; every field of an entry is in
            // range whatever the bits were, and kind 0 entries carry zeros)
            const uint32_t clen = e32 & 15u, kind = (e32 >> 4) & 3u, nx = (e32 >> 8) & 7u;
            const bool is_lit = kind == 1u, is_len = kind == 2u;
            const uint32_t t1 = clen + nx;  // <= 20
            const uint32_t w = __builtin_amdgcn_alignbit(v1, v0, t1);
            uint32_t ent2 = sh.dist.prim[w & (kPrimSize - 1)];
            if (is_len && ent2 == (uint32_t)kLongCode) ent2 = spec_long(sh.dist, w, dist_max);
            const uint32_t dlen = ent2 & 15u, dsym_raw = ent2 >> 4;
            const bool bad2 = ent2 == 0u || dsym_raw >= (uint32_t)kMaxDist;
            const uint32_t dsym = bad2 ? 0u : dsym_raw;
            const uint32_t nb = dsym < 4u ? 0u : (dsym - 2u) >> 1;  // <= 13
            t.clen = clen;
            t.t1 = t1;
            t.dlen = dlen;
            t.tl = is_lit ? clen : t1 + dlen + nb;  // (<= 48)
            t.is_lit = is_lit;
            t.stop = !is_lit && (!is_len || bad2);  // end of block, an invalid code
            t.ol = 0;
            t.val = 0;
            if (FULL) {
              const uint32_t length = (e32 >> 16) + ((v0 >> clen) & ((1u << nx) - 1u));
              const uint32_t dbase = dsym < 4u ? dsym + 1u : (1u << (nb + 1u)) + 1u + ((dsym & 1u) << nb);
              const uint32_t dist = dbase + ((w >> dlen) & ((1u << nb) - 1u));  // (dlen + nb <= 28)
              t.ol = is_lit ? 1u : length;
              t.val = is_lit ? (e32 >> 16) : dist;
            }
            return t;
          };
          // My list from st on.  The 96 bits from the dword that holds the current bit on stay in
          // registers; the two dwords behind them are requested at the top of every step (their address
          // does not depend on the token being decoded).
          auto decode_list = [&](auto full) {
            constexpr bool FULL = decltype(full)::value;
            uint32_t q = st, lq = st;
            n = 0;
            osum = 0;
            fl = 0;
            uint32_t idx = (q - 8u * b.sbase) >> 5;
            uint32_t w0 = sh.stage[idx], w1 = sh.stage[idx + 1], w2 = sh.stage[idx + 2];
            while (q < lim) {
              SPEC_STAT(++st_steps);
              SPEC_STAT(st_wsteps += (uint32_t)lane == uni((uint32_t)lane) ? 1u : 0u);
              const uint32_t w3 = sh.stage[idx + 3], w4 = sh.stage[idx + 4];
              const uint32_t shb = q & 31u;  // (sbase is a multiple of four bytes)
              const Tok t = tok_decode(__builtin_amdgcn_alignbit(w1, w0, shb), __builtin_amdgcn_alignbit(w2, w1, shb), full);
              if (t.stop) {
                fl = 1u;
                break;
              }
              if (n == (uint32_t)kCap) {
                fl = 2u;
                SPEC_STAT(++st_full);
                break;
              }
              if (FULL) {
                mytok[n] = t.ol | (t.is_lit ? 0u : 0x200u) | (t.tl << 10) | (t.val << 16);
                osum += t.ol;
              }
              ++n;
              lq = q;
              q += t.tl;
              const uint32_t nidx = (q - 8u * b.sbase) >> 5;  // (at most two dwords on: shb + tl <= 79)
              const uint32_t adv = nidx - idx;
              idx = nidx;
              w0 = adv == 0u ? w0 : (adv == 1u ? w1 : w2);
              w1 = adv == 0u ? w1 : (adv == 1u ? w2 : w3);
              w2 = adv == 0u ? w2 : (adv == 1u ? w3 : w4);
            }
            e = q;
            have = FULL;
            if (FULL && n) {
              // roffset after the list's last token (decoded once more: cheaper than carrying it through
              // every step): the largest of ceil((bit where a request starts + bits asked) / 8) over
              // huff_sym's and more_bits' requests (inflate.mbt:789-854)
              const uint32_t li = (lq - 8u * b.sbase) >> 5, shb = lq & 31u;
              const uint32_t d0 = sh.stage[li], d1 = sh.stage[li + 1], d2 = sh.stage[li + 2];
              const Tok t = tok_decode(__builtin_amdgcn_alignbit(d1, d0, shb), __builtin_amdgcn_alignbit(d2, d1, shb), std::false_type{});
              uint32_t rq = lq + (t.clen > (uint32_t)lit_min ? t.clen : (uint32_t)lit_min);
              if (!t.is_lit) {
                const uint32_t r2 = lq + t.t1 + (t.dlen > (uint32_t)dist_min ? t.dlen : (uint32_t)dist_min);
                const uint32_t r3 = lq + t.tl;
                rq = rq > r2 ? rq : r2;
                rq = rq > r3 ? rq : r3;
              }
              rl = (rq + 7u) >> 3;
            }
          };
          // Round 0 only measures (it exists to find where the lists end: nine starts in ten are wrong
          // and their tokens with them); round 1 decodes every list for real, from the ends round 0
          // found; later rounds repeat the lists whose start has moved.
          for (int round = 0;; ++round) {
            SPEC_STAT(++st_rounds);
            if (redo) {
              if (round == 0)
                decode_list(std::false_type{});
              else
                decode_list(std::true_type{});
            }
            // the list in front of mine: where it ends, whether it ends the batch
            const uint32_t pe = (uint32_t)__shfl_up((int)e, 1);
            const bool ps = (__shfl_up((int)fl, 1) & 1) != 0;
            const uint32_t want = lane == 0 ? bp : pe;
            const bool dead = (uint32_t)lane >= nl || (lane != 0 && ps);
            ok = !dead && want == st && have;
            redo = !dead && (want != st || !have);
            if (!__ballot(redo) || round + 1 >= kRounds) break;
            if (redo) st = want;
          }
          SPEC_STAT(st_c1 += __builtin_readcyclecounter());
          const uint64_t okm = __ballot(ok);
          uint32_t V = ~okm ? (uint32_t)__builtin_ctzll(~okm) : 64u;  // lists 0..V-1 are the stream's tokens (V >= 1)

          bool refused = false;
          // ---- 2. tokens that cannot be taken here (a distance beyond the history, dict-decoder
          // hist_size; output beyond the slot) end the batch in front of their LIST: the exact reader
          // walks up to them and raises the reference's error.  Only possible in the first 32 KiB of
          // output or at the end of the slot.
          {
            const uint32_t oincl = spec_scan((uint32_t)lane < V ? osum : 0u);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)oincl, 63);
            if (opos < 32768u - dict_len || total > out_cap - opos) {
              SPEC_STAT(++st_check);
              uint32_t off = opos + oincl - osum;
              bool refuse = false;
              if ((uint32_t)lane < V) {
                for (uint32_t i = 0; i < n; ++i) {
                  const uint32_t t = mytok[i];
                  const uint32_t hist = off < 32768u - dict_len ? off + dict_len : 32768u;
                  refuse |= ((t & 0x200u) && (t >> 16) > hist) || (t & 0x1ffu) > out_cap - off;
                  off += t & 0x1ffu;
                }
              }
              const uint64_t R = __ballot(refuse);
              if (R) {  // the batch ends where that list starts (= where the one in front of it ends)
                V = (uint32_t)__builtin_ctzll(R);
                refused = true;
              }
            }
          }
          // where the batch ends, and whether the token there is one for the exact reader
          uint32_t bp_next = bp;
          bool ends_exact = true;
          if (V) {
            bp_next = (uint32_t)__builtin_amdgcn_readlane((int)e, (int)V - 1);
            ends_exact = refused || ((uint32_t)__builtin_amdgcn_readlane((int)fl, (int)V - 1) & 1u);
          }
          const bool mine = (uint32_t)lane < V;
          uint32_t osum_taken = 0;  // (size_only: the bytes the lists taken stand for)
          if (size_only) osum_taken = (uint32_t)__builtin_amdgcn_readlane((int)spec_scan(mine ? osum : 0u), 63);
          const uint32_t nn = mine ? n : 0u;
          const uint32_t nincl = spec_scan(nn);
          const uint32_t nbase = nincl - nn;
          const uint32_t NT = (uint32_t)__builtin_amdgcn_readlane((int)nincl, 63);
          if (mine && n) racc = rl;  // (requests grow along the chain: the last list with tokens decides)
          SPEC_STAT(st_lanes += V);
          SPEC_STAT(st_tokens += NT);

          // ---- 3. the tokens, 64 at a time in stream order
          SPEC_STAT(st_c3 -= __builtin_readcyclecounter());
          if (size_only) opos += osum_taken;
          for (uint32_t t0 = 0; t0 < NT && !size_only; t0 += 64) {
            // the list every token of this group comes from: lists mark the token they start at
            if (lane < 16) sh.lmark[lane] = 0;
            if (nn && nbase - t0 < 64u) reinterpret_cast<uint8_t *>(sh.lmark)[nbase - t0] = (uint8_t)(lane + 1);
            const uint64_t Bc = __ballot(nn && nbase <= t0);
            const uint32_t carry = 64u - (uint32_t)__builtin_clzll(Bc);  // (Bc != 0: t0 < NT)
            uint32_t m = reinterpret_cast<const uint8_t *>(sh.lmark)[lane];
            if (lane == 0) m = m > carry ? m : carry;
            const uint32_t lo = spec_scan_max(m) - 1u;
            const uint32_t nb_o = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(lo << 2), (int)nbase);
            const bool live = t0 + (uint32_t)lane < NT;
            const uint32_t tk = live ? sh.tok[lo * kCap + (t0 + (uint32_t)lane - nb_o)] : 0u;
            const uint32_t ol = tk & 0x1ffu;
            const uint32_t incl = spec_scan(ol);
            const uint32_t oo = incl - ol;
            const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            put_group(live, oo, ol, oo | ((tk & 0x200u) << 6) | (tk & 0xffff0000u), T);
          }
          SPEC_STAT(st_c3 += __builtin_readcyclecounter());
          SPEC_STAT(st_call += __builtin_readcyclecounter());
          if (bp_next != bp) moved = true;
          {  // next batch: ~kCap / 2 tokens per list
            const uint32_t per = V ? NT / V : 0u;
            // (down when a list filled up or the average is close to it; up again when the average the
            // larger size would have had is well below the capacity)
            if ((per > (uint32_t)(kCap * 3 / 4) || __builtin_popcountll(__ballot(mine && fl == 2u)) >= FLATE_SPEC_FULLS) && sub > 32u) sub -= 64u;
            else if (per * (sub + 64u) < (uint32_t)(kCap * 5 / 8) * sub && sub < kSub) sub += 64u;
          }
          bp = bp_next;
          if (ends_exact || NT == 0) break;
        }
        if (moved) {  // hand the position (and the reference reader's byte count) back to the bit reader
          const uint32_t r = spec_max(racc);
          const uint32_t roff = r > b.roff ? r : b.roff;
          if ((bp >> 3) + (uint32_t)kStageMargin > b.sbase + (uint32_t)kStage) stage_fill((bp >> 3) & ~3u);
          bits_at(bp);
          b.roff = roff;
          b.avail = (int)(8u * roff - bp);
          pin();
        }
      }
      // ------------------------------ one token, exactly --------------------------------
      if (stage_low(b)) restage_at(bit_pos());
      const int v = huff_sym(b, sh.lit, lit_min, lit_max, sh.stage, &err);
      SPEC_STAT(++st_exact);
      if (v < 0) break;
      if (v < 256) {
        if (opos >= out_cap) {
          err = E_OUT_SMALL;
          break;
        }
        complete_pending();
        put((uint32_t)v, 1u, false);  // DictDecoder::write_byte
        continue;
      }
      if (v == 256) break;  // finish_block
      int length, dist;
      if ((err = read_copy(b, sh.dist, dist_min, dist_max, sh.stage, v, length, dist))) break;
      const uint32_t hist = opos < (uint32_t)kWin - dict_len ? opos + dict_len : (uint32_t)kWin;  // hist_size
      if ((uint32_t)dist > hist) {
        err = E_CORRUPT;
        break;
      }
      if ((uint32_t)length > out_cap - opos) {
        err = E_OUT_SMALL;
        break;
      }
      // copy_history (:689) / write_copy (dict-decoder.mbt:114-154)
      put_group(lane == 0, 0u, lane == 0 ? (uint32_t)length : 0u, 0x8000u | ((uint32_t)dist << 16), (uint32_t)length);
    }
  }
  if (final_block && !err && stop_bit != ~0u) err = E_CORRUPT;  // BFINAL inside a spliced stream
  complete_pending();
#ifdef FLATE_SPEC_STATS
  st_wsteps = (uint32_t)__builtin_amdgcn_readlane((int)spec_scan(st_wsteps), 63);
  st_wlong = (uint32_t)__builtin_amdgcn_readlane((int)spec_scan(st_wlong), 63);
  st_full = (uint32_t)__builtin_amdgcn_readlane((int)spec_scan(st_full), 63);
  if (lane == 0 && sid == 0) printf("spec wave steps %u, with a long literal code %u\n", st_wsteps, st_wlong);
  if (lane == 0 && (sid < 8 || __builtin_readcyclecounter() - st_t0 > 8000000ull))
    printf("spec stats: sid %u out %u batches %u rounds %u steps %u lanes %u tokens %u groups %u chunks %u exact %u far %u waits %u hazard %u fills %u stop %u full %u check %u\n",
           sid, opos, st_batches, st_rounds, st_steps, st_lanes, st_tokens, st_groups, st_chunks, st_exact, st_far, st_waits, st_hazard,
           st_fill, st_stop, st_full, st_check);
  if (lane == 0 && (sid < 8 || __builtin_readcyclecounter() - st_t0 > 8000000ull))
    printf("spec cycles: total %llu batches %llu decode %llu emit %llu header %llu (tables %llu)\n", (unsigned long long)(__builtin_readcyclecounter() - st_t0),
           (unsigned long long)st_call, (unsigned long long)st_c1, (unsigned long long)st_c3, (unsigned long long)st_chdr, (unsigned long long)st_cinit);
  if (lane == 0 && sid < 4 && st_lr_steps)
    printf("literal runs: sid %u steps %u codes %u cycles %llu (front %llu rounds %llu out %llu) of total %llu\n", sid, st_lr_steps, st_lr_codes,
           (unsigned long long)st_lr_all, (unsigned long long)st_lr_front, (unsigned long long)st_lr_rounds, (unsigned long long)st_lr_out,
           (unsigned long long)(__builtin_readcyclecounter() - st_t0));
  if (lane == 0 && sid == 0)
    printf("spec stats: out %u batches %u rounds %u steps %u lanes %u tokens %u groups %u chunks %u exact %u far %u waits %u hazard %u fills %u stop %u full %u check %u\n",
           opos, st_batches, st_rounds, st_steps, st_lanes, st_tokens, st_groups, st_chunks, st_exact, st_far, st_waits, st_hazard,
           st_fill, st_stop, st_full, st_check);
#endif
  if (lane == 0) {
    P.out_len[sid] = opos;
    P.status[sid] = err;
    P.err_off[sid] = err == E_CORRUPT ? (long long)(in_base + b.roff) : -1;
    // (8 * roff - avail bits are consumed: the last of them closes the final block)
    if (P.used) P.used[sid] = in_base + ((8ull * b.roff - (uint64_t)b.avail + 7u) >> 3);
  }
}

template <int SUB, int CAP, int RING>
__global__ __launch_bounds__(64) void inflate_spec_kernel(InfParams P) {
  __shared__ SpecShared<SUB, CAP, RING> sh;
  inflate_spec<SUB, CAP, RING, false>(P, sh);
}
template <int SUB, int CAP, int RING>
__global__ __launch_bounds__(64) void inflate_spec_dict_kernel(InfParams P) {
  __shared__ SpecShared<SUB, CAP, RING> sh;
  inflate_spec<SUB, CAP, RING, true>(P, sh);
}
