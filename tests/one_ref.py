"""One long DEFLATE stream on the CPU: the reference of flate_hip_inflate_one_index.

`Walk` is a bit-level block walker in pure Python: it reads a raw stream block by block as the serial decoder does --
the same accept / reject decisions, and the reader's byte count (roffset) by the rule of deflate_corpus.py: the reader
takes whole bytes when it needs more bits than it holds, so the count at a failure is ceil(hw / 8), hw the furthest
bit needed so far -- and reports every block's start bit, type, BFINAL and output size, and from that the UNITS: bit 0
and every dynamic block header the decode reaches.  It keeps no history: a distance that reaches in front of the
stream is only noted (`far`), as in the index call, whose verdict is history-free.  Truth about a stream's CONTENT
comes from zlib.  `rule` restates the dynamic-header rule (csrc/deflate_block_rule.h) at one bit offset.  The file also
builds the corpus the tests of the call share; bits are read from bytes, and a test module computes each file once."""
import struct
import zlib

import gzip_ref

OK, CORRUPT, TOO_LARGE, UNEXPECTED_EOF = 0, -4, -6, -7
RAW, ZLIB, GZIP = 0, 1, 2
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


class Stop(Exception):
    def __init__(self, status):
        self.status = status


class Code:
    """HuffmanDecoder::initialize on a list of code lengths: `ok` (the empty code, a complete code, or the one code
    of one bit) and the table {(length, the code's bits LSB first): symbol}, the codes of up to 9 bits spread over
    `fast`."""

    def __init__(self, lens):
        count = [0] * 16
        for n in lens:
            count[n] += 1
        count[0] = 0
        used = [n for n in range(16) if count[n]]
        self.min, self.max = (used[0], used[-1]) if used else (0, 0)
        code, nxt = 0, [0] * 16
        for n in range(1, 16):
            code = (code + count[n - 1]) << 1
            nxt[n] = code
        self.ok = not used or code + count[15] == 1 << 15 or (self.max == 1 and count[1] == 1)
        self.fast, self.long = [None] * 512, {}
        if not self.ok:
            return
        for s, n in enumerate(lens):
            if n:
                r = int(format(nxt[n], "0%db" % n)[::-1], 2)
                nxt[n] += 1
                if n <= 9:
                    for k in range(r, 512, 1 << n):
                        self.fast[k] = (s, n)
                else:
                    self.long[(n, r)] = s


class Bits:
    def __init__(self, buf, pos=0):
        self.buf, self.pos, self.hw, self.end = buf, pos, pos, 8 * len(buf)

    def need(self, n):
        self.hw = max(self.hw, self.pos + n)
        if self.hw > self.end:
            self.hw = self.end
            raise Stop(UNEXPECTED_EOF)

    def peek(self, n):  # n <= 25; zeros behind the end
        q = self.pos >> 3
        return (int.from_bytes(self.buf[q:q + 4], "little") >> (self.pos & 7)) & ((1 << n) - 1)

    def get(self, n):
        self.need(n)
        v = self.peek(n)
        self.pos += n
        return v

    def sym(self, c, cmin):  # huff_sym
        self.need(cmin)
        w = self.peek(15)
        e = c.fast[w & 511]
        if e is None:
            for n in range(10, c.max + 1):
                s = c.long.get((n, w & ((1 << n) - 1)))
                if s is not None:
                    e = (s, n)
                    break
            if e is None:
                raise Stop(CORRUPT)
        self.need(e[1])
        self.pos += e[1]
        return e[0]


def read_dynamic(r):
    """read_huffman behind the 3-bit header -> (lit, dist, the code lengths of the literal/length code)."""
    v = r.get(14)
    nlit, ndist, nclen = (v & 31) + 257, ((v >> 5) & 31) + 1, (v >> 10) + 4
    if nlit > 286 or ndist > 30:
        raise Stop(CORRUPT)
    cl = [0] * 19
    for i in range(nclen):
        cl[CL_ORDER[i]] = r.get(3)
    cc = Code(cl)
    if not cc.ok:
        raise Stop(CORRUPT)
    lens = []
    while len(lens) < nlit + ndist:
        s = r.sym(cc, cc.min)
        if s < 16:
            lens.append(s)
            continue
        if s == 16 and not lens:
            raise Stop(CORRUPT)
        rep = r.get({16: 2, 17: 3, 18: 7}[s]) + (11 if s == 18 else 3)
        if len(lens) + rep > nlit + ndist:
            raise Stop(CORRUPT)
        lens += [lens[-1] if s == 16 else 0] * rep
    lit, dist = Code(lens[:nlit]), Code(lens[nlit:])
    if not lit.ok or not dist.ok:
        raise Stop(CORRUPT)
    return lit, dist, lens[:nlit]


def rule(raw, bit):
    """THE RULE at one bit offset: a dynamic block header the decoder takes starts at `bit` of raw."""
    r = Bits(raw, bit)
    if r.end - bit < 17 or (r.peek(3) >> 1) != 2 or ((r.peek(8) >> 3) & 31) > 29 or ((r.peek(13) >> 8) & 31) > 29:
        return False
    try:
        r.get(3)
        read_dynamic(r)
    except Stop:
        return False
    return True


FIXED = (Code(FIXED_LIT), Code([5] * 32))


class Walk:
    """The serial decode of raw from bit 0, without history: status, err_off (-1 unless CORRUPT), blocks [(start bit,
    type, BFINAL, output bytes)] of the blocks that were read whole, unit_bit / out_off (n_units + 1 entries; of a
    stream that fails the good units and where the failing one starts), out_bytes (0 unless status == 0), out_len (the
    bytes in front of the failure), far (some distance reached in front of the stream), reach (per good unit: the
    bytes of the stream the reader has taken when the unit ends, the three bits of the next header included)."""

    def __init__(self, raw):
        raw = bytes(raw)
        r = Bits(raw)
        self.blocks, self.far, self.status, self.err_off = [], False, OK, -1
        starts, total, self.reach = [0], 0, []
        try:
            while True:
                at = r.pos
                h = r.get(3)
                final, typ = h & 1, h >> 1
                if typ == 3:
                    raise Stop(CORRUPT)
                if typ == 2 and at:
                    starts.append(at)
                    self.reach.append((r.hw + 7) // 8)  # (the unit in front ends with the reader holding these bytes)
                n = 0
                if typ == 0:
                    p = (r.hw + 7) // 8
                    if len(raw) - p < 4:
                        r.hw = r.end
                        raise Stop(UNEXPECTED_EOF)
                    ln, nl = struct.unpack_from("<HH", raw, p)
                    r.hw = 8 * (p + 4)
                    if ln != (~nl & 0xffff):
                        raise Stop(CORRUPT)
                    n = min(ln, len(raw) - p - 4)
                    total += n
                    r.pos = r.hw = 8 * (p + 4 + n)
                    if n < ln:
                        raise Stop(UNEXPECTED_EOF)
                else:
                    if typ == 1:
                        lit, dist = FIXED
                        lmin = 7
                    else:
                        lit, dist, ll = read_dynamic(r)
                        lmin = max(lit.min, ll[256])
                    while True:
                        s = r.sym(lit, lmin)
                        if s < 256:
                            n += 1
                            total += 1
                            continue
                        if s == 256:
                            break
                        if s >= 286:
                            raise Stop(CORRUPT)
                        ln = LBASE[s - 257] + (r.get(LEXT[s - 257]) if LEXT[s - 257] else 0)
                        d = r.sym(dist, dist.min)
                        if d >= 30:
                            raise Stop(CORRUPT)
                        nb = (d - 2) >> 1 if d >= 4 else 0
                        d = DBASE[d] + (r.get(nb) if nb else 0)
                        self.far = self.far or d > total
                        n += ln
                        total += ln
                self.blocks.append((at, typ, final, n))
                if final:
                    self.reach.append((r.hw + 7) // 8)
                    break
        except Stop as e:
            self.status = e.status
            self.err_off = (r.hw + 7) // 8 if e.status == CORRUPT else -1
        self.out_len, self.end_bit = total, r.pos
        good = starts if self.status == OK else starts[:-1]
        self.n_units = len(good)
        self.unit_bit = starts + [r.pos] if self.status == OK else starts
        self.out_off = [sum(b[3] for b in self.blocks if b[0] < u) for u in self.unit_bit[:self.n_units]]
        self.out_off.append(sum(b[3] for b in self.blocks if b[0] < self.unit_bit[self.n_units]) if self.status
                            else total)
        self.out_bytes = total if self.status == OK else 0


def candidates(raw):
    """Every bit offset the discovery probes: bit 0 and the offsets that pass the rule (small streams only: the 13
    bits every header is first judged by come from one big integer, the rest from `rule`)."""
    v, out = int.from_bytes(raw, "little"), {0}
    for b in range(max(8 * len(raw) - 16, 0)):
        h = (v >> b) & 0x1fff
        if (h >> 1) & 3 == 2 and (h >> 3) & 31 <= 29 and h >> 8 <= 29 and rule(raw, b):
            out.add(b)
    return sorted(out)


# ---- containers ----

def wrap(raw, plain, kind):
    if kind == ZLIB:
        return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(plain))
    if kind == GZIP:
        return gzip_ref.header() + raw + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff)
    return raw


def header_len(kind):
    return {RAW: 0, ZLIB: 2, GZIP: 10}[kind]


# ---- the corpus: [(what, raw stream, plain)] ----

def deflate(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    parts = [c.compress(data[i:i + flush_every]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(data), flush_every)]
    return b"".join(parts) + c.flush()


TEXT_BYTES = 300000
MANY_UNITS = 3  # the index of the memLevel = 1 file in good_streams()


def good_streams(oracle=None):
    t = gzip_ref.text(TEXT_BYTES, seed=21)
    mixed = t[:100000] + gzip_ref.rand(70000, seed=8) + t[100000:200000]
    out = [
        ("level 1", deflate(t, 1), t),
        ("level 6", deflate(t, 6), t),
        ("level 9", deflate(t, 9), t),
        ("level 6, memLevel 1: hundreds of short units", deflate(t, 6, mem=1), t),
        ("level 6, memLevel 2", deflate(t, 6, mem=2), t),
        ("Z_FULL_FLUSH every 10 000 bytes: empty stored blocks inside units", deflate(t, 6, flush_every=10000), t),
        ("text, 70 000 random bytes, text: stored blocks mid-stream", deflate(mixed, 6), mixed),
        ("Z_FIXED only: one unit", deflate(t[:60000], 6, strategy=zlib.Z_FIXED), t[:60000]),
        ("level 0 only: one unit", deflate(t[:150000], 0), t[:150000]),
        ("a final dynamic block", deflate(t[:5000], 9), t[:5000]),
        ("17 bytes of input", deflate(t[:17], 6), t[:17]),
        ("the empty stream", deflate(b"", 6), b""),
    ]
    if oracle is not None:
        import numpy as np
        p = t[:200000]
        out.append(("the oracle's own stream for 200 000 bytes", bytes(oracle.deflate(np.frombuffer(p, np.uint8))), p))
    return out


def decoy_streams():
    """A complete raw stream inside a stored block of an outer stream, behind 0 .. 7 leading pad bits (a fixed block of
    literals in front moves the stored block's header through every bit phase; the stored bytes are byte aligned in the
    outer stream, so the inner stream's dynamic headers pass the rule at their own bit offsets)."""
    import deflate_corpus as dc
    t = gzip_ref.text(9000, seed=23)
    inner = deflate(t, 6)
    out = []
    for phase in range(8):
        w = dc.Writer()
        dc.prefix_block(w, phase)
        w.stored(inner, final=False)
        blk = w.fixed(True)
        blk.lits(b"tail")
        blk.end()
        out.append(("a stream inside a stored block, phase %d" % phase, w.data(), bytes(w.out)))
    return out


def history_pair():
    """Two dynamic blocks; the SECOND holds a distance that reaches exactly the stream's first byte (legal) or one byte
    in front of it -> (legal stream, its plain bytes, illegal stream)."""
    import deflate_corpus as dc
    out = []
    for over in (0, 1):
        w = dc.Writer()
        lit, dist = dc.small_lens()
        dist = dc.lens_list(dc.huff_lens({d: 1 for d in range(12)}), 12)
        blk = w.dynamic(lit, dist, final=False)
        blk.lits(dc.TEXT[:30])
        blk.end()
        blk = w.dynamic(lit, dist, final=True)
        blk.lits(dc.TEXT[:5])
        blk.match(4, 35 + over)  # (the writer writes the token either way and models no output for the bad one)
        blk.end()
        out.append((w.data(), bytes(w.out)))
    return out[0][0], out[0][1], out[1][0]
