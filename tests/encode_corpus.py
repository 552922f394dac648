"""Input BYTES that drive the encoder's entropy stage into its rarely taken branches, a reader of what the oracle
wrote for them, and the rules that say which branch a case reached.

The decoders have tests/deflate_corpus.py, a corpus of hand-written streams.  An encoder cannot be handed a stream:
its corpus is input data, chosen so that the reference's block policy (deflate.mbt:236-277), its length-limited
Huffman construction (huffman-code.mbt:295-343), its code-length run coding (huffman-bit-writer.mbt:241-330) and the
stored-block padding take a particular path.  A case never states expected bytes; the oracle (oracle/pyoracle.py)
is the only judge of those.  What a case is FOR is stated as a rule, and every rule is detected from the oracle's
own output: its bytes, read back by the RFC 1951 header reader below, its block trace (kind, in_len, ntokens,
bit_start) and its DeflateFast tokens.  tests/test_encode_corpus.py fails when a rule of REQUIRED_RULES is reached
by no case.

Three parts: (a) read_block / walk_block / token_stats / unlimited_depth, (b) the cases, (c) facts() and
REQUIRED_RULES.

"Limit active" means: the depth of a plain (heap) Huffman tree of the block's histogram is greater than the limit
(15, or 7 for the code-length code) -- ties in the heap go to the shallower subtree, so this is the least depth any
optimal code has -- while the oracle's longest code is exactly the limit.

How the cases reach the matcher (deflate-fast.mbt:123-270): a position is entered in the hash table only when the
scan visits it or a match ends one byte before or on it, and the scan's step grows after 32 misses in a row.  So
random lead-ins make no matches.  The generators therefore keep the scan dense (runs of one byte, or back-to-back
copies) in front of every planted match, and the offset-code case keeps a model of the 16384-entry table so that it
only copies from positions whose entry is still alive; the rules check the outcome, not the model.

Branches that input bytes cannot reach (so no rule asks for them):
 * num_offsets == 0 in a dynamic block (huffman-bit-writer.mbt:575-581): without a match ntok == n, and
   n > n - (n >> 4) sends the window to the Huffman-only writer, which has its own one-code offset table;
 * the default-mode stored decision ssize < (size + size) >> 4 (huffman-bit-writer.mbt:527,780): 8 (n + 5) is less
   than an eighth of the coded size only above 64 bits per byte, and no code is longer than 15 bits;
 * two or more "18 with 127" items in a row (a zero run of 276 or more): the longest zero run a literal alphabet
   can make is 254 (bytes 0 and 255 only), and between the end-of-block code and length code 285 lie 28 symbols.
"""
import heapq

import numpy as np

from deflate_corpus import CL_ORDER, DBASE, DEXT, LBASE, LEXT, canonical

W = 65535          # max_store_block_size: one window, one block
MOONBIT, GO = 0, 1
BOTH = (MOONBIT, GO)
STORED, HUFF, DYN = 0, 1, 2   # the oracle's block kinds; HUFF and DYN are both BTYPE 2 in the stream
KIND_LETTER = "SHD"


def _oracle():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


def lz_chunks(n):
    """(start, length) of the windows that go through DeflateFast::encode (engine.lz_chunks restated, so that this
    module needs no built library)."""
    full, r = divmod(int(n), W)
    return [(i * W, W) for i in range(full)] + ([(full * W, r)] if r >= 128 else [])


# ---------------------------------------------------------------------------------------------------------------
# (a) a reader of what the oracle wrote

class BitReader:
    """LSB-first bits of `data` from bit position `pos`."""

    def __init__(self, data, pos):
        self.data, self.pos = data, pos

    def get(self, n):
        v = 0
        for k in range(n):
            p = self.pos + k
            v |= ((self.data[p >> 3] >> (p & 7)) & 1) << k
        self.pos += n
        return v

    def sym(self, table):
        """One Huffman symbol; table = {(length, code): symbol}, codes MSB first."""
        code = 0
        for n in range(1, 16):
            code = (code << 1) | self.get(1)
            if (n, code) in table:
                return table[(n, code)]
        raise ValueError("no code at bit %d" % self.pos)


def _by_code(lengths):
    return {(n, c): s for s, (c, n) in canonical(lengths).items()}


def read_block(data, bit_start):
    """The header of the block at bit_start -> dict: final, btype, and for BTYPE 2 nlit (HLIT + 257), ndist
    (HDIST + 1), ncl (HCLEN + 4), cl_lens (19, by symbol), lit_lens, dist_lens, items [(symbol, extra or None)] and
    body (the bit where the block's symbols start); for BTYPE 0 len and body (the first data byte's bit)."""
    r = BitReader(data, bit_start)
    h = {"final": r.get(1), "btype": r.get(2)}
    if h["btype"] == 0:
        r.pos = (r.pos + 7) & ~7
        h["len"] = r.get(16)
        if r.get(16) != (~h["len"] & 0xFFFF):
            raise ValueError("LEN / NLEN")
        h["body"] = r.pos
        return h
    if h["btype"] != 2:
        raise ValueError("BTYPE %d: the encoder writes no such block" % h["btype"])
    nlit, ndist, ncl = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
    cl = [0] * 19
    for i in range(ncl):
        cl[CL_ORDER[i]] = r.get(3)
    table = _by_code(cl)
    lens, items = [], []
    while len(lens) < nlit + ndist:
        s = r.sym(table)
        if s < 16:
            items.append((s, None))
            lens.append(s)
            continue
        nbits, base = {16: (2, 3), 17: (3, 3), 18: (7, 11)}[s]
        extra = r.get(nbits)
        items.append((s, extra))
        lens.extend([lens[-1] if s == 16 else 0] * (base + extra))
    if len(lens) != nlit + ndist:
        raise ValueError("code lengths overrun")
    h.update(nlit=nlit, ndist=ndist, ncl=ncl, cl_lens=cl, lit_lens=lens[:nlit], dist_lens=lens[nlit:], items=items,
             body=r.pos)
    return h


def _decode_table(lengths):
    """Peek table: index = the next maxlen bits as they lie in the stream, value = symbol << 4 | code length."""
    codes = canonical(lengths)
    mx = max(lengths)
    tab = np.zeros(1 << mx, dtype=np.int64)
    for s, (c, n) in codes.items():
        rev = int(format(c, "0%db" % n)[::-1], 2)
        tab[rev::1 << n] = (s << 4) | n
    return tab.tolist(), mx


def walk_block(data, h):
    """Decode the block whose header read_block returned, with codes RE-MADE from the parsed lengths by
    deflate_corpus.canonical -> (bytes it produces, symbols before end-of-block, the bit after it)."""
    if h["btype"] == 0:
        return h["len"], 0, h["body"] + 8 * h["len"]
    lit, lmax = _decode_table(h["lit_lens"])
    dist, dmax = _decode_table(h["dist_lens"])
    lmask, dmask = (1 << lmax) - 1, (1 << dmax) - 1
    bit = h["body"]
    byte = bit >> 3
    acc = int.from_bytes(data[byte:byte + 8], "little") >> (bit & 7)
    n = 64 - (bit & 7)
    byte += 8
    out = ntok = 0
    while True:
        if n < 48:
            k = (64 - n) >> 3
            acc |= int.from_bytes(data[byte:byte + k], "little") << n
            byte += k
            n += 8 * k
        e = lit[acc & lmask]
        ln = e & 15
        if not ln:
            raise ValueError("no literal/length code at bit %d" % (byte * 8 - n))
        acc >>= ln
        n -= ln
        s = e >> 4
        if s < 256:
            out += 1
        elif s == 256:
            break
        else:
            eb = LEXT[s - 257]
            out += LBASE[s - 257] + (acc & ((1 << eb) - 1))
            acc >>= eb
            n -= eb
            e = dist[acc & dmask]
            ln = e & 15
            if not ln:
                raise ValueError("no distance code at bit %d" % (byte * 8 - n))
            eb = ln + DEXT[e >> 4]
            acc >>= eb
            n -= eb
        ntok += 1
    return out, ntok, byte * 8 - n


_LEN_CODE = np.searchsorted(np.array(LBASE[:28]), np.arange(3, 259), side="right") - 1
_LEN_CODE[255] = 28   # 258 has a code of its own


def token_stats(tokens):
    """DeflateFast tokens of one window (match tokens have bit 30 set, token.mbt:13-24) -> literal/length histogram
    (286, without end-of-block), offset histogram (30), and start position and length of every match."""
    t = np.asarray(tokens, dtype=np.int64)
    m = t >= (1 << 30)
    length = np.where(m, ((t >> 22) & 0xFF) + 3, 1)
    start = np.cumsum(length) - length
    lit = np.bincount(t[~m], minlength=286)
    lit += np.bincount(257 + _LEN_CODE[length[m] - 3], minlength=286)
    off = (t[m] & 0x3FFFFF) + 1
    dist = np.bincount(np.searchsorted(np.array(DBASE), off, side="right") - 1, minlength=30)
    return lit, dist, start[m], length[m]


def unlimited_depth(hist):
    """Depth of a Huffman tree built with a plain heap and no length limit (ties: the shallower subtree first)."""
    h = [(int(w), 0) for w in hist if w > 0]
    if len(h) < 2:
        return len(h)
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1))
    return h[0][1]


def runs_of(lens):
    """Maximal runs of equal values -> [(value, count)]."""
    out = []
    for v in lens:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return [(v, c) for v, c in out]


class Analysis:
    """One case in one compat mode, as the oracle encodes it."""

    def __init__(self, name, data, compat, oracle=None):
        o = oracle or _oracle()
        self.name, self.compat, self.n = name, compat, len(data)
        self.out, trace = o.deflate(data, compat=compat, with_blocks=True)
        df = o.DeflateFast(compat)
        self.tokens = [df.encode(data[s:s + k]) for s, k in lz_chunks(len(data))]
        self.blocks, pos = [], 0
        for kind, in_len, ntokens, bit_start in trace:
            b = {"kind": kind, "in_len": in_len, "ntokens": ntokens, "bit_start": bit_start, "pos": pos,
                 "hdr": read_block(self.out, bit_start)}
            if kind == DYN:
                lit, dist, _, _ = token_stats(self.tokens[pos // W])
                lit[256] += 1
                b["lit_hist"], b["dist_hist"] = lit, dist
            elif kind == HUFF:
                lit = np.bincount(np.frombuffer(data[pos:pos + in_len], np.uint8), minlength=286)
                lit[256] += 1
                b["lit_hist"], b["dist_hist"] = lit, None
            self.blocks.append(b)
            pos += in_len
        assert pos == self.n


# ---------------------------------------------------------------------------------------------------------------
# (c) rules, detected from an Analysis alone

ZERO_GAPS = (1, 2, 3, 10, 11, 137, 138, 139, 140, 141, 148, 149, 254)
NZ_RUNS = (1, 2, 3, 4, 7, 8, 9, 10)
TAILS = (0, 1, 16, 17, 127, 128)


def _zero_class(c):
    """How generate_codegen (huffman-bit-writer.mbt:299-318) writes a zero run of c: 18s of 138 while c >= 138
    (c / 138 of them), then the remainder as nothing / plain zeros / one 17 / one 18."""
    if c < 138:
        return "zrun_short_%s" % ("1_2" if c < 3 else "3_10" if c < 11 else "11_137")
    r = c % 138
    return "zrun_138k_plus_%s" % ("0" if r == 0 else "1_2" if r < 3 else "3_10" if r < 11 else "ge11")


def _nz_class(c):
    """A run of c equal non-zero lengths: the length, then 16s of 6 ((c - 1) / 6), then the remainder as nothing /
    plain lengths / one 16 (huffman-bit-writer.mbt:284-298)."""
    if c < 4:
        return "nzrun_short_1_3"
    r = (c - 1) % 6
    return "nzrun_6k_plus_%s" % ("0" if r == 0 else "1_2" if r < 3 else "ge3")


def facts(an):
    """The set of rule names the oracle's output of this analysis satisfies."""
    f = set()
    mode = "go" if an.compat == GO else "default"
    data_blocks = an.blocks[:-1]   # the last block is the closing empty stored block (deflate.mbt:171-176)
    for i, b in enumerate(an.blocks):
        h, kind = b["hdr"], b["kind"]
        prev = an.blocks[i - 1] if i else None
        if kind == STORED:
            if prev is not None and prev["kind"] != STORED:
                if i == len(an.blocks) - 1:
                    f.add("close_phase_%d" % (b["bit_start"] % 8))
                elif b["in_len"] > 16 and an.compat == GO:
                    f.add("stored_phase_%d" % (b["bit_start"] % 8))
        else:
            lit, dist, cl = h["lit_lens"], h["dist_lens"], h["cl_lens"]
            if max(lit) == 15 and unlimited_depth(b["lit_hist"]) > 15:
                f.add("lit_len15_limited")
            if kind == DYN and max(dist) == 15 and unlimited_depth(b["dist_hist"]) > 15:
                f.add("dist_len15_limited")
            cl_hist = np.bincount([s for s, _ in h["items"]], minlength=19)
            if max(cl) == 7 and unlimited_depth(cl_hist) > 7:
                f.add("cl_len7_limited")
            used = sum(1 for v in lit if v)
            if used in (2, 3, 4):
                f.add("lit_used_%d" % used)
            if kind == DYN:
                dused = sum(1 for v in dist if v)
                if dused in (1, 2):
                    f.add("dist_used_%d" % dused)
                if h["ndist"] in (1, 30):
                    f.add("hdist_%d" % h["ndist"])
                if lit[-1] == dist[0]:
                    f.add("run_crosses_hlit")
            if h["nlit"] == 286:
                f.add("hlit_286")
            if h["ncl"] == 19:
                f.add("hclen_19")
            runs = runs_of(lit + dist)
            for v, c in runs:
                if v == 0:
                    f.add(_zero_class(c))
                    if c in ZERO_GAPS:
                        f.add("zrun_%d" % c)
                else:
                    f.add(_nz_class(c))
                    if c in NZ_RUNS:
                        f.add("nzrun_%d" % c)
                    if c >= 70:
                        f.add("nzrun_ge70")
            if len(runs) > 64:
                f.add("runs_gt_64")
            if len(runs) > 128:
                f.add("runs_gt_128")
            if len(h["items"]) > 128:
                f.add("items_gt_128")
        n = b["in_len"]
        if i < len(an.blocks) - 1 and (n == W or n >= 128):   # this window went through enc_speed's switch
            d = b["ntokens"] - (n - (n >> 4))
            size = "n65535" if n == W else "small" if n <= 400 else None
            if size and d in (0, 1):
                f.add("switch_at_%s_%s" % ("0" if d == 0 else "plus1", size))
        if prev is not None and i < len(an.blocks) - 1:
            if all(x["kind"] != STORED or x["in_len"] > 16 for x in (prev, b)):
                f.add("pair_%s_%s%s" % (mode, KIND_LETTER[prev["kind"]], KIND_LETTER[kind]))
    full = [b["kind"] for b in data_blocks if b["in_len"] == W]
    if len(full) >= 2 and len(set(full)) >= 2:
        tail = an.n % W
        if tail in TAILS:
            f.add("tail_%d_after_mixed_%s" % (tail, mode))
    for (start, k), toks in zip(lz_chunks(an.n), an.tokens):
        _, _, pos, length = token_stats(toks)
        if pos.size == 0:
            continue
        if pos.size >= 14000:
            f.add("matches_per_chunk_ge_14000")
        if np.bincount(pos >> 8).max() >= 60:
            f.add("tile_with_ge_60_starts")
        if (pos & 255 == 255).any():
            f.add("match_start_at_255")
        if ((pos & 255 == 255) & (length == 258)).any():
            f.add("match_258_across_two_tile_edges")
        if k == W and (pos + length == W).any():
            f.add("match_ends_window")
        if np.unique(pos & 3).size == 4:
            f.add("match_starts_every_mod4")
    return f


def switch_distance(b):
    """ntokens - (n - (n >> 4)) of a block that went through the enc_speed switch (deflate.mbt:266)."""
    return b["ntokens"] - (b["in_len"] - (b["in_len"] >> 4))


def family_facts(analyses):
    """Rules that need two cases: `stored_flip_both_sides` -- two cases of the stored_flip family whose m differ by
    one and whose (single) data block is stored in one and Huffman-coded in the other (Go mode)."""
    by = {}
    for an in analyses:
        if an.name.startswith("stored_flip_") and an.compat == GO:
            fam, m = an.name.rsplit("_m", 1)
            by.setdefault(fam, {})[int(m)] = an.blocks[0]["kind"] == STORED
    out = {}
    for fam, d in by.items():
        for m in d:
            if m + 1 in d and d[m] != d[m + 1]:
                out.setdefault("stored_flip_both_sides", []).append("%s_m%d/m%d" % (fam, m, m + 1))
    return out


REQUIRED_RULES = sorted(
    ["lit_len15_limited", "dist_len15_limited", "cl_len7_limited", "lit_used_2", "lit_used_3", "lit_used_4",
     "dist_used_1", "dist_used_2", "hlit_286", "hdist_30", "hdist_1", "hclen_19",
     "zrun_short_1_2", "zrun_short_3_10", "zrun_short_11_137",
     "zrun_138k_plus_0", "zrun_138k_plus_1_2", "zrun_138k_plus_3_10", "zrun_138k_plus_ge11",
     "nzrun_short_1_3", "nzrun_6k_plus_0", "nzrun_6k_plus_1_2", "nzrun_6k_plus_ge3", "nzrun_ge70",
     "runs_gt_64", "runs_gt_128", "items_gt_128", "run_crosses_hlit",
     "switch_at_0_n65535", "switch_at_plus1_n65535", "switch_at_0_small", "switch_at_plus1_small",
     "stored_flip_both_sides",
     "matches_per_chunk_ge_14000", "tile_with_ge_60_starts", "match_start_at_255", "match_ends_window",
     "match_258_across_two_tile_edges", "match_starts_every_mod4"]
    + ["zrun_%d" % g for g in ZERO_GAPS] + ["nzrun_%d" % c for c in NZ_RUNS]
    + ["pair_go_%s%s" % (a, b) for a in "SHD" for b in "SHD"]
    + ["pair_default_%s%s" % (a, b) for a in "HD" for b in "HD"]
    + ["stored_phase_%d" % p for p in range(8)] + ["close_phase_%d" % p for p in range(8)]
    + ["tail_%d_after_mixed_%s" % (t, m) for t in TAILS for m in ("go", "default")])


# The case that each rule was built with ("name/compat mode"), as the oracle showed when the corpus was made;
# tests/test_encode_corpus.py checks every entry.  Most rules are reached by more cases than the one named here.
COVERED_BY = {
    "cl_len7_limited": "fib_code_lengths/default", "close_phase_0": "close_after_31/default",
    "close_phase_1": "close_after_24/default", "close_phase_2": "close_after_17/default",
    "close_phase_3": "close_after_20/default", "close_phase_4": "close_after_22/default",
    "close_phase_5": "close_after_18/default", "close_phase_6": "close_after_19/default",
    "close_phase_7": "close_after_39/default", "dist_len15_limited": "fib_offsets/default",
    "dist_used_1": "fib_literals_dynamic/default", "dist_used_2": "run_then_pairs/default",
    "hclen_19": "fib_literals/default", "hdist_1": "run_x600/default", "hdist_30": "far_copy_24664/default",
    "hlit_286": "run_x600/default", "items_gt_128": "alternating_256/default",
    "lit_len15_limited": "fib_literals_dynamic/default", "lit_used_2": "one_byte_x17/default",
    "lit_used_3": "two_bytes_x100/default", "lit_used_4": "three_bytes_x100/default",
    "match_258_across_two_tile_edges": "planted_matches/default", "match_ends_window": "planted_matches/default",
    "match_start_at_255": "planted_matches/default", "match_starts_every_mod4": "planted_matches/default",
    "matches_per_chunk_ge_14000": "dense_words/default", "nzrun_1": "equal_counts_x1/default",
    "nzrun_10": "uniform_2pow4/default", "nzrun_2": "equal_counts_x5/default", "nzrun_3": "equal_counts_x3/default",
    "nzrun_4": "equal_counts_x11/default", "nzrun_6k_plus_0": "equal_counts_x7/default",
    "nzrun_6k_plus_1_2": "equal_counts_x12/default", "nzrun_6k_plus_ge3": "equal_counts_x6/default",
    "nzrun_7": "equal_counts_x7/default", "nzrun_8": "uniform_2pow7/default", "nzrun_9": "equal_counts_x12/default",
    "nzrun_ge70": "equal_counts_x100/default", "nzrun_short_1_3": "equal_counts_x1/default",
    "pair_default_DD": "sequence_SSHHDDSDHS/default", "pair_default_DH": "sequence_SSHHDDSDHS/default",
    "pair_default_HD": "sequence_SSHHDDSDHS/default", "pair_default_HH": "sequence_SSHHDDSDHS/default",
    "pair_go_DD": "sequence_SSHHDDSDHS/go", "pair_go_DH": "sequence_SSHHDDSDHS/go",
    "pair_go_DS": "sequence_SSHHDDSDHS/go", "pair_go_HD": "sequence_SSHHDDSDHS/go",
    "pair_go_HH": "sequence_SSHHDDSDHS/go", "pair_go_HS": "sequence_SSHHDDSDHS/go",
    "pair_go_SD": "sequence_SSHHDDSDHS/go", "pair_go_SH": "sequence_SSHHDDSDHS/go",
    "pair_go_SS": "sequence_SSHHDDSDHS/go", "run_crosses_hlit": "run_x600/default",
    "runs_gt_128": "alternating_256/default", "runs_gt_64": "alternating_256/default",
    "stored_flip_both_sides": "stored_flip_n65535_m7369/m7370", "stored_phase_0": "phase_sweep_9/go",
    "stored_phase_1": "phase_sweep_1/go", "stored_phase_2": "phase_sweep_2/go",
    "stored_phase_3": "phase_sweep_0/go", "stored_phase_4": "phase_sweep_14/go",
    "stored_phase_5": "phase_sweep_6/go", "stored_phase_6": "phase_sweep_20/go",
    "stored_phase_7": "phase_sweep_4/go", "switch_at_0_n65535": "switch_n65535_p0/default",
    "switch_at_0_small": "switch_n272_p0/default", "switch_at_plus1_n65535": "switch_n65535_p1/default",
    "switch_at_plus1_small": "switch_n272_p1/default", "tail_0_after_mixed_default": "mixed_SDH_tail0/default",
    "tail_0_after_mixed_go": "mixed_SDH_tail0/go", "tail_127_after_mixed_default": "mixed_SDH_tail127/default",
    "tail_127_after_mixed_go": "mixed_SDH_tail127/go", "tail_128_after_mixed_default": "mixed_SDH_tail128/default",
    "tail_128_after_mixed_go": "mixed_SDH_tail128/go", "tail_16_after_mixed_default": "mixed_SDH_tail16/default",
    "tail_16_after_mixed_go": "mixed_SDH_tail16/go", "tail_17_after_mixed_default": "mixed_SDH_tail17/default",
    "tail_17_after_mixed_go": "mixed_SDH_tail17/go", "tail_1_after_mixed_default": "mixed_SDH_tail1/default",
    "tail_1_after_mixed_go": "mixed_SDH_tail1/go", "tile_with_ge_60_starts": "dense_words/default",
    "zrun_1": "gap1_from0/default", "zrun_10": "gap10_from0/default", "zrun_11": "gap11_from0/default",
    "zrun_137": "gap137_from0/default", "zrun_138": "gap138_from0/default",
    "zrun_138k_plus_0": "gap138_from0/default", "zrun_138k_plus_1_2": "gap139_from0/default",
    "zrun_138k_plus_3_10": "gap141_from0/default", "zrun_138k_plus_ge11": "gap1_from0/default",
    "zrun_139": "gap139_from0/default", "zrun_140": "gap140_from0/default", "zrun_141": "gap141_from0/default",
    "zrun_148": "gap148_from0/default", "zrun_149": "gap149_from0/default", "zrun_2": "gap2_from0/default",
    "zrun_254": "gap254_from0/default", "zrun_3": "gap3_from0/default", "zrun_short_11_137": "gap11_from0/default",
    "zrun_short_1_2": "gap1_from0/default", "zrun_short_3_10": "gap3_from0/default",
}


def coverage(analyses):
    """{rule: [case name / compat, ...]} over a list of Analysis objects."""
    cov = {}
    for an in analyses:
        for r in facts(an):
            cov.setdefault(r, []).append("%s/%s" % (an.name, "go" if an.compat == GO else "default"))
    for r, names in family_facts(analyses).items():
        cov.setdefault(r, []).extend(names)
    return cov


# ---------------------------------------------------------------------------------------------------------------
# (b) the cases

def _rng(*key):
    return np.random.default_rng([20240917] + [int(k) for k in key])


def _counts(rng, counts):
    """A shuffled array in which byte value v occurs counts[v] times."""
    a = np.repeat(np.array(list(counts.keys()), dtype=np.uint8), list(counts.values()))
    rng.shuffle(a)
    return a


_VOCAB = None


def text(rng, n):
    """Compressible text: words of a fixed 300-word vocabulary in random order (many matches of 4..12 bytes)."""
    global _VOCAB
    if _VOCAB is None:
        r = _rng(1)
        letters = np.frombuffer(b"etaoinshrdlucmfwypvbgk", np.uint8)
        _VOCAB = [bytes(r.choice(letters, int(r.integers(2, 10)))) + b" " for _ in range(300)]
    out, size = [], 0
    while size < n:
        w = _VOCAB[int(rng.integers(0, len(_VOCAB)))]
        out.append(w)
        size += len(w)
    return np.frombuffer(b"".join(out)[:n], np.uint8).copy()


def rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8)


def rand7(rng, n):
    """Seven bits of entropy per byte and no matches: Huffman-only in both compat modes."""
    return rng.integers(64, 192, n, dtype=np.uint8)


def _hash(v):
    return ((v * 0x1E35A7BD) & 0xFFFFFFFF) >> 18   # deflate-fast.mbt:78


def fib_literals(rng, n=W, others=100, dynamic=False):
    """Byte values that occur 1, 2, 3, 5, ... 377 times among bytes drawn evenly from `others` more values.  With
    the end-of-block code, which occurs once, the rare symbols are a Fibonacci chain 13 deep at the bottom of a
    Huffman tree whose top is about log2(n / 986) deep.  (One more symbol that occurs once -- the histogram 1, 1, 1,
    2, 3, ... -- halves the chain's depth: the chain has to be exact.)

    dynamic: the window starts with a run of 1 + 21 * 258 equal bytes, that is 21 matches of length 258, enough to
    take the window past the enc_speed switch; length code 285 then stands in the chain for the byte value that
    would occur 21 times."""
    weights = fib(14)[1:]
    run = 0
    if dynamic:
        weights.remove(21)
        run = 1 + 21 * 258
    chain = {3 + 2 * i: c for i, c in enumerate(weights)}
    body = n - run - sum(chain.values())
    a = np.concatenate([_counts(rng, chain), rng.integers(64, 64 + others, body).astype(np.uint8)])
    rng.shuffle(a)
    if a[0] == 64:
        a[0] = 65
    return np.concatenate([np.full(run, 64, np.uint8), a])


# code lengths {length: how many symbols have it} with 2 ** -length summing to one.  With the two 18s for the 172
# unused byte values in front and the one-bit offset code of a Huffman-only block, the code length symbols occur
# 1, 1, 2, 3, 5, 8, 13, 21, 34 times: a plain Huffman tree of those is 8 deep
_CL_PROFILE = {15: 8, 14: 34, 13: 13, 8: 1, 7: 3, 5: 21, 4: 5}


def fib_code_lengths(rng):
    """32767 bytes in which a byte value whose code is to be l bits long occurs 2 ** (15 - l) times (the end-of-block
    code is the last of the 15-bit ones), the values 172..255 taking their lengths in an order that leaves no run
    of equal ones."""
    left = dict(_CL_PROFILE)
    left[15] -= 1
    order, last = [], None
    while sum(left.values()):
        l = max((k for k in left if left[k] and k != last), key=lambda k: left[k], default=None)
        if l is None:
            l = next(k for k in left if left[k])
        order.append(l)
        left[l] -= 1
        last = l
    assert len(order) == 84
    return _counts(rng, {172 + i: 1 << (15 - l) for i, l in enumerate(order)})


# offset codes a unit of eight bytes can reach: its source lies 1..4 bytes before an earlier unit's end, so the
# distance is 1..4 mod 8 -- codes 4 (5..6), 5 (7..8) and 7 (13..16) have no such distance.  Codes 0 and 1 are left
# out: a copy from 1 or 2 back makes the four bytes in FRONT of the unit a repeat too (xxxx, abab), which the scan
# looks up first and finds somewhere far behind
_UNIT_CODES = [c for c in range(2, 30)
               if any((d & 7) in (1, 2, 3, 4) for d in range(DBASE[c], DBASE[c] + (1 << DEXT[c])))]


def offset_schedule(rng, weights, lead_units=750):
    """One window of units "5 bytes copied from an earlier position + 3 fresh bytes" in which offset code c is used
    weights[c] times; the first lead_units units copy from 9 back (code 6) and count for that code.

    A model of the matcher's table (which position owns each of the 16384 slots) says which earlier positions a
    copy may start from: only a position the scan entered -- the last four of a unit -- whose slot no later entry
    has taken, and which no unit has copied from yet (a second copy would find the first one instead)."""
    plan = []
    for c, w in sorted(weights.items()):
        plan += [c] * (w - (lead_units if c == 6 else 0))
    queue = [6] * lead_units + [plan[i] for i in rng.permutation(len(plan))]
    data = bytearray(rng.integers(0, 256, 16, dtype=np.uint8).tobytes())
    owner, used = {}, set()
    for p in range(13):                        # the scan visits every position of the 16 random bytes
        owner[_hash(int.from_bytes(data[p:p + 4], "little"))] = p
    pending = [13, 14, 15]                     # entries whose four bytes reach into the next unit
    i = misses = 0
    while i < len(queue) and misses < 1000:
        u = len(data)
        assert u + 8 <= W - 16
        c = queue[i]
        ds = [d for d in range(DBASE[c], min(DBASE[c] + (1 << DEXT[c]) - 1, u) + 1) if (d & 7) in (1, 2, 3, 4)]
        found = None
        for d in (ds[int(j)] for j in rng.permutation(len(ds))):
            p = u - d
            if p in used:
                continue
            ext = bytearray(data[u - 16:])      # the last 16 bytes and, appended, the five copied ones
            base = u - 16
            for k in range(5):
                ext.append(data[p + k] if p + k < u else ext[p + k - base])

            def val(q):
                return int.from_bytes(ext[q - base:q - base + 4], "little") if q >= base else \
                    int.from_bytes(data[q:q + 4], "little")
            slot = _hash(val(p))
            later = [_hash(val(q)) for q in pending if q > p]   # entries made after p's and before the lookup
            if slot in later or (p not in pending and owner.get(slot) != p):
                continue
            found = (p, bytes(ext[16:]), [(q, _hash(val(q))) for q in pending])
            break
        if found is None:                      # no live source for this code here: try it a few units later
            j = min(len(queue) - 1, i + 1 + int(rng.integers(0, 20)))
            queue[i], queue[j] = queue[j], queue[i]
            misses += 1
            continue
        p, copied, entries = found
        data += copied
        fresh = rng.integers(0, 256, 3, dtype=np.uint8).tolist()
        while fresh[0] == data[p + 5]:         # the match must end after five bytes
            fresh[0] = (fresh[0] + 1) & 255
        data += bytes(fresh)
        used.add(p)
        for q, h in entries:
            owner[h] = q
        owner[_hash(int.from_bytes(data[u:u + 4], "little"))] = u          # the scan finds the match here
        owner[_hash(int.from_bytes(data[u + 4:u + 8], "little"))] = u + 4  # one byte before the match's end
        pending = [u + 5, u + 6, u + 7]
        i += 1
    data += rng.integers(0, 256, W - len(data), dtype=np.uint8).tobytes()
    return np.frombuffer(bytes(data), np.uint8).copy()


def fib(n):
    a = [1, 1]
    while len(a) < n:
        a.append(a[-1] + a[-2])
    return a[:n]


def fib_offsets(seed=0):
    """Eighteen offset codes used 1, 1, 2, 3, ... 2584 times: a plain Huffman tree of them is 17 deep.  The near
    codes get the large weights; code 6 gets 987, which holds the lead-in.

    The chain has to be exact: one stray match (a nineteenth code used once) or one missing gives 1, 1, 1, 2, ...
    and a tree of depth 10 to 12.  The table model leaves about one such accident per window (a match found at
    another distance than planned, or not found).  Of the seeds 0..15 the oracle's tokens were exact for 9 (depth
    17, longest offset code 15 bits) and deeper than 15 also for 6, 8 and 15 (depth 16); the others gave depth
    10..12 with a longest code of 10..15 bits.  The corpus uses seed 9."""
    ws = sorted(fib(18), reverse=True)
    ws.remove(987)
    weights = {6: 987}
    for c in _UNIT_CODES[:18]:
        if c != 6:
            weights[c] = ws.pop(0)
    assert not ws
    return offset_schedule(_rng(2, seed), weights)


def gaps_alphabet(first, gaps):
    vals = [first]
    for g in gaps:
        vals.append(vals[-1] + g + 1)
    assert vals[-1] <= 255, vals
    return vals


def dense_words(rng, windows=2, lead=1000):
    """Lead-in of `lead` units "4-byte word + 4 bytes copied from 9 back", then the words in random order back to
    back: a match of four bytes every four bytes."""
    d = bytearray(rng.integers(0, 256, 9, dtype=np.uint8).tobytes())
    words = []
    for k in range(lead):
        w = bytes([k & 255, k >> 8]) + rng.integers(0, 256, 2, dtype=np.uint8).tobytes()
        words.append(w)
        d += w
        d += d[-9:-5]
    n = windows * W
    idx = rng.integers(0, lead, (n - len(d)) // 4 + 1)
    d += b"".join(words[int(i)] for i in idx)
    return np.frombuffer(bytes(d[:n]), np.uint8).copy()


def planted_matches(rng):
    """One window: 300 random bytes P; a run of one byte up to a position 255 mod 256; P[:258] again (a 258-byte
    match that starts at 255 mod 256 and crosses two tile edges); runs and short copies of P at every position mod
    4; and P[:100] as the window's last bytes (a match that ends on the window's last byte)."""
    P = rand(rng, 300)
    parts = [P, np.full(256 * 3 + 255 - 300, 122, np.uint8), P[:258], np.full(1, 33, np.uint8)]
    for k in range(8):
        run = np.full(40 + k, 97 + k, np.uint8)
        parts += [run, P[8 * k:8 * k + 9 + k], np.full(1, 35 + k, np.uint8)]
    size = sum(p.size for p in parts)
    # (the copy that ends the window needs a source within 32768 bytes: a second one 20101 bytes in front of it)
    parts += [np.full(W - 100 - size - 20101, 119, np.uint8), P[:100], np.full(1, 36, np.uint8),
              np.full(20000, 120, np.uint8), P[:100]]
    return np.concatenate(parts)


def _first_block_kind(o, data, compat):
    return o.deflate(data, compat=compat, with_blocks=True)[1][0][0]


def _build_cases():
    o = _oracle()
    C = []

    def add(name, data, modes=BOTH):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        C.append((name, data.tobytes(), tuple(modes)))

    # ---- code length limits ----
    add("fib_literals", fib_literals(_rng(3)))
    add("fib_literals_dynamic", fib_literals(_rng(3, 1), dynamic=True))
    add("fib_offsets", fib_offsets(9))
    add("fib_code_lengths", fib_code_lengths(_rng(3, 2)))

    # ---- few symbols ----
    add("one_byte_x17", np.full(17, 65, np.uint8))
    add("one_byte_x127", np.full(127, 65, np.uint8))
    add("two_bytes_x100", _counts(_rng(4), {65: 60, 200: 40}))
    add("three_bytes_x100", _counts(_rng(5), {65: 50, 66: 30, 200: 20}))
    add("run_x600", np.full(600, 65, np.uint8))                      # 258-byte matches at distance 1
    add("run_then_pairs", np.concatenate([np.full(150, 65, np.uint8), np.tile(np.array([66, 67], np.uint8), 100)]))
    for k in (129, 200, 263, 264, 265, 300, 520):
        add("run_x%d" % k, np.full(k, 65, np.uint8))
    r = _rng(6)
    head = rand(r, 64)
    add("far_copy_24664", np.concatenate([head, np.full(24600, 48, np.uint8), head, rand(r, 40)]))

    # ---- zero runs of the literal lengths, by alphabet ----
    for g in ZERO_GAPS:
        for first in (0, 1):
            if first + g + 1 <= 255:
                vals = gaps_alphabet(first, [g])
                add("gap%d_from%d" % (g, first), _rng(7, g, first).choice(np.array(vals, np.uint8), 60))
    vals = gaps_alphabet(2, [1, 2, 3, 10, 11, 137])
    add("gaps_1_2_3_10_11_137", _rng(8).choice(np.array(vals, np.uint8), 120))
    add("gaps_138_then_to_eob", _rng(9).choice(np.array([9, 148, 149, 152], np.uint8), 90))
    r = _rng(10)                                                     # a dynamic block with the same gaps
    add("gaps_dynamic", np.tile(r.choice(np.array(gaps_alphabet(3, [139, 3, 10, 11, 2]), np.uint8), 300), 3))

    # ---- runs of equal non-zero lengths ----
    for m in list(range(1, 17)) + [70, 100]:
        counts = {40 + k: 4 for k in range(m)}
        counts.update({10: 1, 20: 1, 200: 40})
        add("equal_counts_x%d" % m, _counts(_rng(11, m), counts))
    for k in (3, 4, 5, 6, 7):
        add("uniform_2pow%d" % k, _rng(12, k).integers(32, 32 + (1 << k), 3000, dtype=np.uint8))
    add("alternating_256", _counts(_rng(13), {v: (8 if v % 2 == 0 else 1) for v in range(256)}))
    add("alternating_140", _counts(_rng(14), {v: (8 if v % 2 == 0 else 1) for v in range(100, 240)}))

    # ---- the enc_speed switch ntok > n - (n >> 4) ----
    for n, period, label in ((W, 40, "n65535"), (272, 8, "n272")):
        r = _rng(15, n)
        base, body = rand7(r, period), rand7(r, n)
        want, t = set(range(-4, 5)), (n >> 4) - 8
        while want and t < (n >> 4) + 40:
            d = np.concatenate([base, np.resize(base, t), body])[:n]
            toks = o.DeflateFast(MOONBIT).encode(d)
            dist = toks.size - (n - (n >> 4))
            if dist in want:
                want.discard(dist)
                add("switch_%s_%s%d" % (label, "m" if dist < 0 else "p", abs(dist)), d)
            t += 1

    # ---- the Go-mode stored decision ssize < size + (size >> 4) ----
    for n in (2000, W):
        r = _rng(16, n)
        body, txt = rand(r, n), text(r, n)

        def mix(m):
            return np.concatenate([txt[:m], body[m:]])
        lo, hi = 0, n                          # stored at lo, not stored at hi
        assert _first_block_kind(o, mix(lo), GO) == STORED and _first_block_kind(o, mix(hi), GO) != STORED
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if _first_block_kind(o, mix(mid), GO) == STORED:
                lo = mid
            else:
                hi = mid
        for m in range(lo - 2, hi + 3):
            add("stored_flip_n%d_m%d" % (n, m), mix(m), (GO,))

    # ---- block sequences ----
    r = _rng(17)
    kinds = {"S": rand, "H": rand7, "D": text}
    add("sequence_SSHHDDSDHS", np.concatenate([kinds[k](r, W) for k in "SSHHDDSDHS"]))
    for t in TAILS:
        r = _rng(18, t)
        add("mixed_SDH_tail%d" % t, np.concatenate([rand(r, W), text(r, W), rand7(r, W), text(r, t)]))
    # a stored window behind a block that ends at every bit phase, and the closing block likewise: the first
    # window's tokens change with j, and with them the bit where its block ends
    seen_s, seen_c, j = set(), set(), 0
    while (len(seen_s) < 8 or len(seen_c) < 8) and j < 64:
        r = _rng(19, j)
        d = np.concatenate([np.resize(text(r, 700 + j), W), rand(r, W), text(r, 40 + j)])
        blocks = o.deflate(d, compat=GO, with_blocks=True)[1]
        ps, pc = blocks[1][3] % 8, blocks[-1][3] % 8
        if blocks[1][0] == STORED and blocks[2][0] != STORED and (ps not in seen_s or pc not in seen_c):
            seen_s.add(ps)
            seen_c.add(pc)
            add("phase_sweep_%d" % j, d)
        j += 1
    for k in range(17, 40):                    # small streams: the closing block at every phase, both modes
        add("close_after_%d" % k, text(_rng(20, k), k))

    # ---- match density and placement ----
    add("dense_words", dense_words(_rng(21)))
    add("planted_matches", planted_matches(_rng(22)))
    return C


_CASES = None


def cases():
    """[(name, bytes, compat modes)] -- built once per process."""
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
    return _CASES


def analyses(oracle=None):
    return [Analysis(name, data, compat, oracle) for name, data, modes in cases() for compat in modes]
