"""A raw DEFLATE bit writer (RFC 1951) and a hand-built corpus of edge cases for the inflaters.

The writer writes any block -- stored, fixed or dynamic -- and checks nothing: a dynamic header's HLIT, HDIST and
HCLEN fields, its code-length-code lengths and its sequence of code-length symbols (16, 17 and 18 with their extra
bits) are the caller's, so invalid headers can be written.  It records the bit position of what it writes and the
furthest bit the reference decoder has to have read at each point (`hw`), and it keeps the output a correct decoder
produces (`out`), so that a case states its expected result itself.

The roffset rule (inflate.mbt more_bits :789-799, huff_sym :803-854; oracle/inflate.c more_bits / huff_sym) that the
pinned error offsets follow: the reader takes whole bytes, and only when it needs more bits than it holds.  A Huffman
lookup needs max(tree.min, code length) bits from its start -- for the literal/length tree min is raised to the
length of the end-of-block code (inflate.mbt:545-547) -- a dynamic header's first read needs its 14 bits at once, and
extra bits are read as they are needed.  So the byte count read at a failure is ceil(hw / 8), hw being the furthest
bit needed so far; a corrupt_input_error reports that count (inflate.mbt:38).  An unexpected end reports no offset (-1).

Each base case pins the oracle's status, out_len, output bytes and err_off.  Derived variants (other output slots,
every byte-boundary truncation, a prefix block in front) are compared with the oracle at run time by the GPU tests.
"""
import heapq

E_OK, E_OUT_TOO_SMALL, E_CORRUPT, E_EOF = 0, -1, -2, -3  # oracle/pyoracle.py: OK, E_OUT_TOO_SMALL, ...
HIST = 32768

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
         258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
         4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# a complete code-length code in which every symbol has a code: 0..12 at 4 bits, 13..18 at 5 bits
CL_DEFAULT = [4] * 13 + [5] * 6
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def canonical(lengths):
    """RFC 1951 3.2.2 codes {symbol: (code, length)} -- also for incomplete or over-subscribed lengths (the
    codes of an over-subscribed set are not prefix-free; nothing decodes them)."""
    mx = max(lengths, default=0)
    count = [0] * (mx + 2)
    for n in lengths:
        if n:
            count[n] += 1
    code, nxt = 0, [0] * (mx + 2)
    for b in range(1, mx + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = {}
    for s, n in enumerate(lengths):
        if n:
            codes[s] = (nxt[n], n)
            nxt[n] += 1
    return codes


def huff_lens(weights, limit=15):
    """Huffman code lengths for {symbol: weight} (a complete code; one symbol gets length 1)."""
    items = [(w, i, [s]) for i, (s, w) in enumerate(sorted(weights.items()))]
    lens = {s: 0 for s in weights}
    if len(items) == 1:
        return {items[0][2][0]: 1}
    heapq.heapify(items)
    k = len(items)
    while len(items) > 1:
        w1, _, a = heapq.heappop(items)
        w2, _, b = heapq.heappop(items)
        for s in a + b:
            lens[s] += 1
        heapq.heappush(items, (w1 + w2, k, a + b))
        k += 1
    assert max(lens.values()) <= limit
    return lens


def lens_list(d, n):
    out = [0] * n
    for s, v in d.items():
        out[s] = v
    return out


def rle(lens):
    """Code-length symbols for a list of lengths: 16 / 17 / 18 where they fit, as [(sym, extra)]."""
    seq, i = [], 0
    while i < len(lens):
        v, r = lens[i], 1
        while i + r < len(lens) and lens[i + r] == v:
            r += 1
        if v == 0 and r >= 11:
            k = min(r, 138)
            seq.append((18, k - 11))
        elif v == 0 and r >= 3:
            k = min(r, 10)
            seq.append((17, k - 3))
        elif v != 0 and r >= 4:
            seq.append((v, None))
            k = 1 + min(r - 1, 6)
            seq.append((16, k - 4))
        else:
            seq.append((v, None))
            k = 1
        i += k
    return seq


class Writer:
    """LSB-first DEFLATE bits, the furthest bit the reference must have read (hw), marks, and the output."""

    def __init__(self, zdict=b""):
        self.bits = []
        self.hw = 0
        self.marks = {}
        self.zdict = bytes(zdict)[-HIST:]
        self.out = bytearray()
        self.events = []  # (kind, out_start, out_end): "lit", "copy", "stored"

    @property
    def pos(self):
        return len(self.bits)

    def need(self, n):
        """The reader needs n bits from here."""
        self.hw = max(self.hw, self.pos + n)

    def mark(self, name):
        self.marks[name] = self.pos
        return self.pos

    def put(self, v, n):  # LSB first
        self.bits.extend((v >> k) & 1 for k in range(n))
        self.need(0)

    def put_read(self, v, n):  # a field the reader needs as a whole
        self.need(n)
        self.put(v, n)

    def code(self, c, n):  # Huffman codes MSB first
        self.bits.extend((c >> (n - 1 - k)) & 1 for k in range(n))

    def align(self):
        self.bits.extend([0] * (-self.pos % 8))

    def data(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))

    def roff(self, extra=0):
        """Bytes the reference has read when it needs `extra` more bits from the current position."""
        return (max(self.hw, self.pos + extra) + 7) // 8

    # ---- output model ----
    def hist(self):
        return min(len(self.out) + len(self.zdict), HIST)

    def emit_lit(self, b):
        self.out.append(b)
        self.events.append(("lit", len(self.out) - 1, len(self.out)))

    def emit_copy(self, length, dist):
        if dist > self.hist():
            return False
        start = len(self.out)
        for _ in range(length):
            p = len(self.out) - dist
            self.out.append(self.out[p] if p >= 0 else self.zdict[len(self.zdict) + p])
        self.events.append(("copy", start, len(self.out)))
        return True

    # ---- blocks ----
    def header(self, final, btype):
        self.mark("block")
        self.put_read(int(final), 1)
        self.put_read(btype, 2)

    def stored(self, payload, final=True, length=None, nlength=None, cut=None):
        """A stored block (inflate.mbt:708-766): LEN / NLEN may be given wrong; cut = bytes of payload written."""
        self.header(final, 0)
        self.align()
        self.hw = max(self.hw, self.pos)  # data_block drops the bit buffer: it reads from the next whole byte
        ln = len(payload) if length is None else length
        nl = (~ln & 0xFFFF) if nlength is None else nlength
        self.mark("stored_len")
        self.put_read(ln, 16)
        self.put_read(nl, 16)
        self.mark("stored_data")
        body = payload if cut is None else payload[:cut]
        for b in body:
            self.put(b, 8)
        start = len(self.out)
        self.out += body
        if body:
            self.events.append(("stored", start, len(self.out)))

    def fixed(self, final=True):
        self.header(final, 1)
        return Block(self, canonical(FIXED_LIT), None, 7, 0)

    def dynamic(self, lit_lens, dist_lens, final=True, hlit=None, hdist=None, hclen=None, cl_lens=None, cl_seq=None):
        """A dynamic block header.  lit_lens / dist_lens are the lengths the block's codes use; hlit / hdist /
        hclen (the raw 5 / 5 / 4-bit fields), cl_lens (19 lengths by symbol) and cl_seq ([(sym, extra)]) default
        to a valid header for them.  Nothing is checked."""
        self.header(final, 2)
        hlit = len(lit_lens) - 257 if hlit is None else hlit
        hdist = len(dist_lens) - 1 if hdist is None else hdist
        hclen = 15 if hclen is None else hclen
        cl_lens = CL_DEFAULT if cl_lens is None else cl_lens
        cl_seq = rle(list(lit_lens) + list(dist_lens)) if cl_seq is None else cl_seq
        self.mark("hlit")
        self.need(14)  # read_huffman: while nb < 5 + 5 + 4
        self.put(hlit, 5)
        self.mark("hdist")
        self.put(hdist, 5)
        self.mark("hclen")
        self.put(hclen, 4)
        self.mark("cl_lens")
        for i in range(hclen + 4):
            self.put_read(cl_lens[CL_ORDER[i]], 3)
        self.mark("cl_syms")
        used = [cl_lens[CL_ORDER[i]] if i < hclen + 4 else 0 for i in range(19)]
        cl_by_sym = [0] * 19
        for i in range(19):
            cl_by_sym[CL_ORDER[i]] = used[i]
        cl_codes = canonical(cl_by_sym)
        cl_min = min((n for n in cl_by_sym if n), default=0)
        for s, extra in cl_seq:
            c, n = cl_codes[s]
            self.need(max(cl_min, n))
            self.code(c, n)
            if s >= 16:
                self.put_read(extra, {16: 2, 17: 3, 18: 7}[s])
        self.mark("body")
        lit_min = min((n for n in lit_lens if n), default=0)
        lit_min = max(lit_min, lit_lens[256] if len(lit_lens) > 256 else 0)
        dist_min = min((n for n in dist_lens if n), default=0)
        return Block(self, canonical(lit_lens), canonical(dist_lens), lit_min, dist_min)


class Block:
    """Symbols of one Huffman block: literals and matches update the output model, raw symbols do not."""

    def __init__(self, w, lit, dist, lit_min, dist_min):
        self.w, self.lit, self.dist, self.lit_min, self.dist_min = w, lit, dist, lit_min, dist_min

    def sym(self, s):
        c, n = self.lit[s]
        self.w.need(max(self.lit_min, n))
        self.w.code(c, n)

    def dsym(self, d):
        if self.dist is None:  # fixed distance codes: 5 bits, read at once
            self.w.need(5)
            self.w.code(d, 5)
        else:
            c, n = self.dist[d]
            self.w.need(max(self.dist_min, n))
            self.w.code(c, n)

    def bit(self, v):
        """One raw bit where a code is due (to reach a tree's invalid half)."""
        self.w.put(v, 1)

    def lits(self, data):
        for b in data:
            self.sym(b)
            self.w.emit_lit(b)

    def match(self, length, dist, lcode=None, lextra=None):
        li = max(k for k in range(29) if LBASE[k] <= length) if lcode is None else lcode - 257
        ext = length - LBASE[li] if lextra is None else lextra
        self.sym(257 + li)
        self.w.put_read(ext, LEXT[li])
        di = max(k for k in range(30) if DBASE[k] <= dist)
        self.dsym(di)
        self.w.put_read(dist - DBASE[di], DEXT[di])
        return self.w.emit_copy(length, dist)

    def end(self):
        self.sym(256)


class Case:
    def __init__(self, name, rule, ref, build, zdict=b"", cap=None, zlib_rejects_at=None, note=""):
        self.name, self.rule, self.ref, self.zdict, self.note = name, rule, ref, bytes(zdict), note
        self.build = build
        w = Writer(zdict)
        res = build(w)
        self.data = w.data()
        self.status, self.err_off = res[0], res[1]
        self.out = bytes(w.out)
        self.zlib_more = bytes(getattr(w, "zlib_more", b""))  # bytes zlib delivers beyond `out`
        self.events = list(w.events)
        self.cap = len(self.out) + 16 if cap is None else cap
        # a byte count at which the reference still wants more input while zlib has already rejected the stream
        self.zlib_rejects_at = zlib_rejects_at(w) if callable(zlib_rejects_at) else zlib_rejects_at

    def __repr__(self):
        return "Case(%s)" % self.name


def ok(w):
    return E_OK, -1


def eof(w):
    return E_EOF, -1


def corrupt(w, off):
    return E_CORRUPT, off


# ---------------------------------------------------------------------------------------------------------------
# building blocks

TEXT = b"the edge of the block is the edge of the table; "


def full_tree_lens(nlit=286, ndist=30):
    """A complete literal/length code over all nlit symbols and a complete distance code over ndist."""
    lit = huff_lens({s: (40 if (s < 256 and s in TEXT) or s == 256 else 1) for s in range(nlit)})
    dist = huff_lens({d: 1 for d in range(ndist)})
    return lens_list(lit, nlit), lens_list(dist, ndist)


def small_lens():
    """A small complete code for TEXT's bytes, EOB and a few length codes; four distance codes."""
    wts = {b: TEXT.count(b) for b in set(TEXT)}
    wts.update({256: 1, 257: 3, 258: 2, 260: 1, 265: 1})
    return lens_list(huff_lens(wts), 266), lens_list(huff_lens({0: 2, 1: 1, 4: 1, 9: 1}), 10)


def dyn_body(blk):
    blk.lits(TEXT[:20])
    blk.match(3, 1)
    blk.match(4, 2)
    blk.lits(TEXT[20:30])
    blk.match(6, 5)
    blk.match(11, 25)


def prefix_block(w, phase, final=False):
    """A fixed block of literals that ends at bit phase `phase` and leaves history behind it."""
    blk = w.fixed(final)
    blk.lits(b"prefix:")
    while (w.pos + 7) % 8 != phase:  # the end-of-block code is 7 bits; a 9-bit literal moves the phase by one
        blk.lits(b"\xf0")
    blk.end()


# ---------------------------------------------------------------------------------------------------------------
# the cases

def _hlit(field):
    def build(w):
        lit, dist = full_tree_lens(286, 30)
        blk = w.dynamic(lit, dist, hlit=field)
        if field > 29:
            return corrupt(w, (w.marks["hlit"] + 14 + 7) // 8)
        blk.lits(TEXT)
        blk.match(258, len(TEXT))
        blk.end()
        return ok(w)
    return build


def _hdist(field):
    def build(w):
        lit, dist = full_tree_lens(286, 30)
        blk = w.dynamic(lit, dist, hdist=field)
        if field > 29:
            return corrupt(w, (w.marks["hlit"] + 14 + 7) // 8)
        blk.lits(TEXT)
        blk.match(10, 30)
        blk.end()
        return ok(w)
    return build


def _hclen4(w):
    # only 16, 17, 18, 0 have lengths: every length is zero -> two empty trees; the first lookup is corrupt
    cl = [0] * 19
    cl[0], cl[16], cl[17], cl[18] = 1, 2, 3, 3
    w.dynamic([0] * 257, [0], hclen=0, cl_lens=cl, cl_seq=[(18, 138 - 11), (18, 119 - 11), (0, None)])
    return corrupt(w, w.roff())


def _hclen19(w):
    lit, dist = small_lens()
    blk = w.dynamic(lit, dist, hclen=15)
    dyn_body(blk)
    blk.end()
    return ok(w)


def _cut_header(field):
    """A dynamic header cut after the byte in which `field` starts (the block header starts at bit phase 6, so
    that cut falls inside its three bits)."""
    def build(w):
        prefix_block(w, 6)
        n0 = len(w.out)
        lit, dist = small_lens()
        blk = w.dynamic(lit, dist)
        dyn_body(blk)
        blk.end()
        w.bits = w.bits[:8 * (w.marks[field] // 8 + 1)]
        del w.out[n0:]  # only the prefix block's output
        return eof(w)
    return build


def _cl_oversub(w):
    cl = list(CL_DEFAULT)
    cl[0] = cl[1] = cl[2] = 1
    w.dynamic(*small_lens(), cl_lens=cl)
    return corrupt(w, (w.marks["cl_syms"] + 7) // 8)


def _cl_incomplete(w):
    cl = [0] * 19
    for s in (0, 4, 5, 6, 7, 8, 9, 10, 18):  # nine codes of 4 bits: 9/16 of the code space
        cl[s] = 4
    lit = lens_list({s: 8 for s in range(256)} | {256: 8}, 257)  # (never decoded)
    w.dynamic(lit, [0], cl_lens=cl, cl_seq=[])
    return corrupt(w, (w.marks["cl_syms"] + 7) // 8)


def _cl_single(bad):
    def build(w):
        cl = [0] * 19
        cl[0] = 1  # one code of length 1: accepted (inflate.mbt:161); zlib rejects it
        seq = [(0, None)] * 258
        if bad:
            seq = seq[:100]
        w.dynamic([0] * 257, [0], cl_lens=cl, cl_seq=seq)
        if bad:
            w.need(1)
            w.put(1, 1)  # the unused half of the code-length code
        # (all lengths zero: two empty trees, and the first literal lookup finds no code)
        return corrupt(w, w.roff())
    return build


def _cl_rep16_first(w):
    lit, dist = small_lens()
    w.dynamic(lit, dist, cl_seq=[(16, 1)] + rle(lit + dist))
    # the reference rejects 16 at position 0 before its extra bits (inflate.mbt:472-476): its code is 5 bits
    return corrupt(w, (w.marks["cl_syms"] + 5 + 7) // 8)


def _cl_overrun(sym):
    def build(w):
        lit, dist = small_lens()
        # two lengths short of nlit + ndist, a repeat of 3 (16: after one more length), 3 or 11
        seq = rle(lit + dist[:-2]) + ([(5, None), (16, 0)] if sym == 16 else [(sym, 0)])
        w.dynamic(lit, dist, cl_seq=seq)
        return corrupt(w, w.roff())
    return build


def _cl_cross_build(w):
    wts = {b: TEXT.count(b) for b in set(TEXT)}
    wts.update({256: 1, 257: 2})
    lit = lens_list(huff_lens(wts), 286)
    dist = [0] * 4 + [1, 1]  # distance codes 4 (5..6) and 5 (7..8)
    # one 18 for the last 28 literal/length lengths and the first four distance lengths
    seq = rle(lit[:258]) + [(18, (286 - 258) + 4 - 11), (1, None), (1, None)]
    blk = w.dynamic(lit, dist, cl_seq=seq)
    blk.lits(TEXT)
    blk.match(3, 5)
    blk.match(3, 8)
    blk.end()
    return ok(w)


def _tree(kind, which):
    """Over-subscribed or incomplete literal/length or distance code."""
    def build(w):
        lit, dist = small_lens()
        if which == "lit":
            lit = list(lit)
            if kind == "oversub":
                lit[ord("z")] = 1
            else:
                i = max(range(len(lit)), key=lambda s: lit[s])
                lit[i] = 0  # drop one of the longest codes
        else:
            dist = list(dist)
            if kind == "oversub":
                dist[7] = 1
            else:
                dist[9] = 0
        w.dynamic(lit, dist)
        return corrupt(w, w.roff())
    return build


def _lit_single(bit):
    def build(w):
        prefix_block(w, 5)
        blk = w.dynamic(lens_list({256: 1}, 257), [0])  # only the end-of-block code, 1 bit
        if bit == 0:
            blk.end()
            return ok(w)
        w.need(1)
        blk.bit(1)
        return corrupt(w, w.roff())
    return build


def _dist_single(bit):
    def build(w):
        lit = lens_list({b: 2 for b in b"ab"} | {256: 2, 262: 2}, 263)
        blk = w.dynamic(lit, [1])  # one distance code of 1 bit: distance 1
        blk.lits(b"ab")
        if bit == 0:
            blk.match(8, 1)
            blk.lits(b"ba")
            blk.end()
            return ok(w)
        blk.sym(262)  # length 8
        w.need(1)
        blk.bit(1)
        return corrupt(w, w.roff())
    return build


def _dist_empty(used):
    def build(w):
        lit = lens_list({b: 2 for b in b"ab"} | {256: 2, 257: 2}, 258)
        blk = w.dynamic(lit, [0])
        blk.lits(b"abba")
        if not used:
            blk.end()
            return ok(w)
        blk.sym(257)
        return corrupt(w, w.roff())  # the empty tree has no code: corrupt without reading
    return build


def _lit_empty(w):
    prefix_block(w, 6)
    w.dynamic([0] * 257, [1, 1])
    return corrupt(w, w.roff())


def _no_eob(w):
    # literal codes only, none for end-of-block: the reference decodes literals until the input ends
    blk = w.dynamic(lens_list({ord("x"): 1, ord("y"): 1}, 257), [0])
    blk.lits(b"xyyxxxyxyyyxyxxy" * 3)
    while w.pos % 8:  # (padding bits would decode as literals too)
        blk.lits(b"x")
    return eof(w)


def _long_codes(w):
    # lengths 1..14 for 'a'..'n', then 15 for length code 285 and end-of-block: the longest code is EOB
    lit = {ord("a") + k: k + 1 for k in range(14)}
    lit.update({285: 15, 256: 15})
    dist = {k: k + 1 for k in range(14)}
    dist.update({14: 15, 15: 15})
    blk = w.dynamic(lens_list(lit, 286), lens_list(dist, 16))
    blk.lits(b"abcdefghijklmnnmlkjihgfedcba")
    blk.match(258, 28)
    blk.match(258, 200)   # distance code 15 (193..256), 15 bits
    blk.match(258, 150)   # distance code 14, 15 bits
    blk.match(258, 1)     # code 0, 1 bit
    blk.match(258, 100)   # code 13 (97..128), 14 bits
    blk.end()
    return ok(w)


def _lit_min_eof(w):
    # 'a' and 'b' have 2-bit codes, EOB 3 bits: lit_min = 3.  The stream ends 2 bits after the last 'a' starts:
    # the code is there, the 3 bits the reference wants first are not -- one literal short
    lit = lens_list({ord("a"): 2, ord("b"): 2, ord("c"): 3, 256: 3, 257: 3, 258: 3}, 259)
    blk = w.dynamic(lit, [0])
    blk.lits(b"abab" * 5)
    if w.pos % 2:
        blk.lits(b"c")
    while w.pos % 8 != 6:
        blk.lits(b"a")
    blk.lits(b"a")
    assert w.pos % 8 == 0
    w.zlib_more = w.out[-1:]  # the last literal's code is complete but fewer than lit_min bits are left:
    del w.out[-1:]            # zlib delivers it, the reference does not
    return eof(w)


def _len258(code):
    def build(w):
        blk = w.fixed()
        blk.lits(b"Q")
        if code == 285:
            blk.match(258, 1)
        else:
            blk.match(258, 1, lcode=284, lextra=31)  # 227 + 31: the reference accepts it (inflate.mbt:606-612)
        blk.lits(b"!")
        blk.end()
        return ok(w)
    return build


def _fixed_sym(s):
    def build(w):
        blk = w.fixed()
        blk.lits(b"abc")
        blk.sym(s)
        return corrupt(w, w.roff())
    return build


def _fixed_dist(d):
    def build(w):
        blk = w.fixed()
        blk.lits(b"abcdef")
        blk.sym(257)
        blk.dsym(d)
        return corrupt(w, w.roff())
    return build


def _history(h, over, dlen=0):
    """h bytes of output (stored), then a fixed-block copy at distance hist (over: hist + 1)."""
    def build(w):
        data = bytes((i * 131 + (i >> 8)) & 255 for i in range(h))
        for k in range(0, h, 65535):
            w.stored(data[k:k + 65535], final=False)
        blk = w.fixed()
        hist = min(h + dlen, HIST)
        dist = hist + 1 if over else hist
        blk.lits(b"")
        blk.match(5, dist)
        if over:
            return corrupt(w, w.roff())
        blk.lits(b"@")
        blk.end()
        return ok(w)
    return build


def _stored(kind):
    def build(w):
        blk = w.fixed(final=False)
        blk.lits(b"pre")
        blk.end()
        if kind == "nlen":
            w.stored(b"0123456789", length=10, nlength=0xFFF5 ^ 1)
            w.out = w.out[:3]
            return corrupt(w, w.marks["stored_data"] // 8)
        if kind == "len0":
            w.stored(b"", final=False)
            blk = w.fixed()
            blk.lits(b"post")
            blk.end()
            return ok(w)
        if kind == "len65535":
            w.stored(bytes(range(256)) * 255 + bytes(range(255)))
            return ok(w)
        if kind == "cut":
            w.stored(bytes(range(100)), cut=40)  # the oracle copies the 40 bytes that are there
            return eof(w)
        raise ValueError(kind)
    return build


def _stored_slot(w):
    blk = w.fixed(final=False)
    blk.lits(b"before")
    blk.end()
    w.stored(bytes(range(200)))
    w.out = w.out[:6]  # nothing of a stored block that does not fit is copied (inflate.mbt:745-750)
    return E_OUT_TOO_SMALL, -1


def _stored_phase(p):
    def build(w):
        blk = w.fixed(final=False)
        blk.lits(b"ph")
        while w.pos % 8 != (p - 7) % 8:
            blk.lits(b"\xf1")
        blk.end()
        assert w.pos % 8 == p
        w.stored(b"stored after phase %d" % p)
        return ok(w)
    return build


def _nonfinal_end(w):
    blk = w.fixed(final=False)
    blk.lits(b"not final")
    blk.end()
    w.align()
    return eof(w)


def _trailing(w):
    blk = w.fixed()
    blk.lits(b"final")
    blk.end()
    w.align()
    w.put(0xA5, 8)
    w.put(0x07, 8)
    return ok(w)


def _slot_mid(kind):
    """A valid stream decoded into a slot that fills up inside a copy, a literal run or a stored block."""
    def build(w):
        blk = w.fixed(final=False)
        blk.lits(b"0123456789")
        blk.match(50, 10)
        blk.lits(b"abcdefghij")
        blk.end()
        w.stored(b"S" * 40 + b"T" * 40)
        # slots of 35, 65 and 120 bytes: a copy that does not fit is not started, literals fill the slot, and a
        # stored block that does not fit is not started
        del w.out[{"copy": 10, "lits": 65, "stored": 70}[kind]:]
        return E_OUT_TOO_SMALL, -1
    return build


def _build_cases():
    C = []
    add = lambda *a, **k: C.append(Case(*a, **k))
    for f in (29, 30, 31):
        add("hlit_%d" % f, "hlit_%d" % f, "inflate.mbt:429-437 / inflate.c:193", _hlit(f),
            cap=len(TEXT) + 258 + 16)
    for f in (29, 30, 31):
        add("hdist_%d" % f, "hdist_%d" % f, "inflate.mbt:438-441 / inflate.c:196", _hdist(f))
    add("hclen_4", "hclen_4", "inflate.mbt:442-455 / inflate.c:199-207", _hclen4)
    add("hclen_19", "hclen_19", "inflate.mbt:442-455 / inflate.c:199-207", _hclen19)
    for f in ("block", "hlit", "hdist", "hclen", "cl_lens", "cl_syms"):
        add("header_cut_" + f, "header_cut", "inflate.mbt:431-458 / inflate.c:190-212", _cut_header(f))
    add("clc_oversubscribed", "clc_oversubscribed", "inflate.mbt:161 / inflate.c:68,210", _cl_oversub)
    add("clc_incomplete", "clc_incomplete", "inflate.mbt:161 / inflate.c:68,210", _cl_incomplete)
    add("clc_single_len1", "clc_single_len1", "inflate.mbt:161 / inflate.c:68", _cl_single(False),
        zlib_rejects_at=lambda w: (w.marks["cl_syms"] + 7) // 8)
    add("clc_single_len1_bad_bit", "clc_single_len1", "inflate.mbt:837-845 / inflate.c:171", _cl_single(True),
        zlib_rejects_at=lambda w: (w.marks["cl_syms"] + 7) // 8)
    add("clc_rep16_first", "clc_rep16_first", "inflate.mbt:472-476 / inflate.c:229", _cl_rep16_first)
    for s in (16, 17, 18):
        add("clc_rep%d_overrun" % s, "clc_rep_overrun", "inflate.mbt:518-520 / inflate.c:250", _cl_overrun(s))
    add("clc_rep18_crosses_into_dist", "clc_rep_cross", "inflate.mbt:518-525 / inflate.c:250-254", _cl_cross_build)
    for which in ("lit", "dist"):
        for kind in ("oversub", "incomplete"):
            add("%s_%s" % (which, kind), "%s_%s" % (which, kind), "inflate.mbt:161,530-533 / inflate.c:68,257",
                _tree(kind, which))
    add("lit_single_len1", "lit_single_len1", "inflate.mbt:161 / inflate.c:68", _lit_single(0))
    add("lit_single_len1_bad_bit", "lit_single_len1", "inflate.mbt:837-845 / inflate.c:171", _lit_single(1))
    add("dist_single_len1", "dist_single_len1", "inflate.mbt:161 / inflate.c:68", _dist_single(0))
    add("dist_single_len1_bad_bit", "dist_single_len1", "inflate.mbt:837-845 / inflate.c:171", _dist_single(1))
    add("dist_empty_unused", "dist_empty_unused", "inflate.mbt:143-145 / inflate.c:58", _dist_empty(False))
    add("dist_empty_used", "dist_empty_used", "inflate.mbt:837-845 / inflate.c:171", _dist_empty(True))
    add("lit_empty", "lit_empty", "inflate.mbt:143-145,837-845 / inflate.c:58,171", _lit_empty)
    add("no_eob_code", "no_eob", "inflate.mbt:545-547 / inflate.c:260", _no_eob,
        zlib_rejects_at=lambda w: (w.marks["body"] + 7) // 8)
    add("long_codes_eob_longest", "long_codes", "inflate.mbt:167-188,826-836 / inflate.c:70-83,164-168",
        _long_codes)
    add("lit_min_eof", "lit_min", "inflate.mbt:545-547,810-825 / inflate.c:152-162,260", _lit_min_eof)
    add("len258_code285", "len258_code285", "inflate.mbt:613-615 / inflate.c:306", _len258(285))
    add("len258_code284_extra31", "len258_code284", "inflate.mbt:609-612 / inflate.c:303", _len258(284))
    for s in (286, 287):
        add("fixed_sym_%d" % s, "fixed_sym_%d" % s, "inflate.mbt:616-618 / inflate.c:309", _fixed_sym(s))
    for d in (30, 31):
        add("fixed_dist_%d" % d, "fixed_dist_%d" % d, "inflate.mbt:672-674 / inflate.c:344", _fixed_dist(d))
    for h in (0, 1, 32767, 32768, 32769):
        if h:
            add("dist_eq_hist_at_%d" % h, "dist_eq_hist", "inflate.mbt:677-680 / inflate.c:349-350",
                _history(h, False))
        if h < HIST:
            add("dist_over_hist_at_%d" % h, "dist_over_hist", "inflate.mbt:677-680 / inflate.c:349-350",
                _history(h, True))
    for dl in (1, 100, 32768):
        zd = bytes((i * 37 + 11) & 255 for i in range(dl))
        for h in (0, 1, 32767, 32768, 32769):
            add("dict%d_dist_eq_hist_at_%d" % (dl, h), "dict_dist_eq_hist", "dict-decoder.mbt:63-68 / inflate.c:348",
                _history(h, False, dl), zdict=zd)
            if h + dl < HIST:
                add("dict%d_dist_over_hist_at_%d" % (dl, h), "dict_dist_over_hist",
                    "dict-decoder.mbt:63-68 / inflate.c:348", _history(h, True, dl), zdict=zd)
    add("stored_nlen_mismatch", "stored_nlen", "inflate.mbt:727-731 / inflate.c:376", _stored("nlen"))
    add("stored_len0", "stored_len0", "inflate.mbt:732-735 / inflate.c:377", _stored("len0"))
    add("stored_len65535", "stored_len65535", "inflate.mbt:736-766 / inflate.c:378-385", _stored("len65535"))
    add("stored_cut", "stored_cut", "inflate.mbt:751-766 / inflate.c:379-384", _stored("cut"))
    add("stored_slot_too_small", "stored_slot", "inflate.mbt:745-750 / inflate.c:380", _stored_slot, cap=100)
    for p in range(8):
        add("stored_after_phase_%d" % p, "stored_phase", "inflate.mbt:708-716 / inflate.c:366-373", _stored_phase(p))
    add("nonfinal_then_end", "nonfinal_end", "inflate.mbt:345-349 / inflate.c:436-444", _nonfinal_end)
    add("bytes_after_final", "trailing_bytes", "inflate.mbt:769-776 / inflate.c:434", _trailing)
    for k in ("copy", "lits", "stored"):
        add("slot_full_mid_" + k, "slot_mid_" + k, "dict-decoder.mbt:114-185 / inflate.c:269,352,380",
            _slot_mid(k), cap={"copy": 35, "lits": 65, "stored": 120}[k])
    return C


REQUIRED_RULES = sorted([
    "hlit_29", "hlit_30", "hlit_31", "hdist_29", "hdist_30", "hdist_31", "hclen_4", "hclen_19", "header_cut",
    "clc_oversubscribed", "clc_incomplete", "clc_single_len1", "clc_rep16_first", "clc_rep_overrun", "clc_rep_cross",
    "lit_oversub", "lit_incomplete", "dist_oversub", "dist_incomplete", "lit_single_len1", "dist_single_len1",
    "dist_empty_unused", "dist_empty_used", "lit_empty", "no_eob", "long_codes", "lit_min",
    "len258_code285", "len258_code284", "fixed_sym_286", "fixed_sym_287", "fixed_dist_30", "fixed_dist_31",
    "dist_eq_hist", "dist_over_hist", "dict_dist_eq_hist", "dict_dist_over_hist",
    "stored_nlen", "stored_len0", "stored_len65535", "stored_cut", "stored_slot", "stored_phase",
    "nonfinal_end", "trailing_bytes", "slot_mid_copy", "slot_mid_lits", "slot_mid_stored",
])

CASES = _build_cases()


# ---------------------------------------------------------------------------------------------------------------
# derived variants (compared with the oracle at run time)

def with_prefix(case, phase):
    """The case's stream behind a non-final fixed block that ends at bit phase `phase` (history behind it)."""
    w = Writer(case.zdict)
    prefix_block(w, phase)
    case.build(w)
    return w.data()


def slot_caps(case):
    """Output capacities for a valid case: exact, one short, zero, and inside each kind of output event."""
    n = len(case.out)
    caps = {n, max(n - 1, 0), 0}
    for kind in ("copy", "lit", "stored"):
        ev = [e for e in case.events if e[0] == kind and e[2] - e[1] >= 1]
        if ev:
            a, b = ev[len(ev) // 2][1:]
            caps.add(a + (b - a) // 2 if kind != "lit" else a)
    return sorted(caps)


def variants(max_trunc=200):
    """(name, stream, cap, zdict) for every derived variant: output slots, truncations, prefix blocks."""
    out = []
    for i, c in enumerate(CASES):
        if c.status == E_OK:
            for cap in slot_caps(c):
                out.append(("%s/cap%d" % (c.name, cap), c.data, cap, c.zdict))
        room = max(len(c.out), c.cap) + 64
        if len(c.data) < max_trunc:
            for k in range(len(c.data)):
                out.append(("%s/cut%d" % (c.name, k), c.data[:k], room, c.zdict))
        pre = with_prefix(c, i % 8)
        out.append(("%s/prefix%d" % (c.name, i % 8), pre, room + 64, c.zdict))
    return out
