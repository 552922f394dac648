"""Hand-built streams for flate_hip_inflate_one: the edges of the 32 KiB window across UNIT boundaries, and unit shapes
that zlib never writes (it emits no distance above 32768 - 262, no empty dynamic block, no stored block inside a unit
that a later unit reads through).  Pure Python, no GPU: every stream comes from deflate_corpus.Writer with a code in
which every literal, length and distance has a code word (full_tree_lens), over RANDOM ground bytes, so that a source
that is off by one byte gives other bytes.  What a stream inflates to is the Writer's output model -- held against zlib
by test_one_window_corpus.py, the test of this file -- and never the code under test.

good_streams()    [(what, raw stream, plain, marks)]; marks = [(output position, length, distance)] of the copies the
                  case exists for.  intent(what) = (units the case intends, [the unit each mark's source STARTS in]):
                  what the builder was told, not what a walk of the stream finds.
failing_twins()   [(what, raw stream, front, kind)]: kind "far" -- the stream of a good case in which the one marked
                  copy with distance == total (< 32768: it reaches the stream's first byte) has distance + 1, and the
                  copy at total == 32767 with distance 32768; front = the Writer's bytes in front of that copy.  kind
                  "cut" -- a good stream cut in the middle of the unit that holds its marked copy; front = the whole
                  plain text, of which the decoder delivers a prefix.

A unit is what tests/one_ref.py's Walk calls one: bit 0 and every dynamic block header start one, and the stored and
fixed blocks behind a dynamic block belong to its unit."""
import numpy as np

import deflate_corpus as dc
import gzip_ref

W = 32768
ZLIB_MAX_DIST = W - 262  # zlib's deflate never reaches further back (MAX_DIST = w_size - MIN_LOOKAHEAD)
LIT, DIST = dc.full_tree_lens()
FAR_DISTANCES = (W, W - 1, ZLIB_MAX_DIST + 1, ZLIB_MAX_DIST)
UNITS_BACK = (1, 2, 9)
UNIT_SIZES = (W - 1, W, W + 1, 2 * W + 5)
OVERLAP_DISTANCES = (1, 2, 3, 63, 64, 65)


class Stream:
    """One stream under construction: the Writer, the units begun so far (their start bits), the marks and, per mark,
    the unit the case says the source starts in."""

    def __init__(self, what, over=0):
        self.what, self.over = what, over  # over: added to the distance of the copy marked `twin`
        self.w, self.blk = dc.Writer(), None
        self.unit_bits, self.marks, self.src, self.mark_unit = [], [], [], []  # mark_unit: the unit that holds the copy
        self.front = None  # the output in front of the first copy the Writer refused

    def _close(self):
        if self.blk is not None:
            self.blk.end()
            self.blk = None

    def unit(self, final=False):
        """A dynamic block: it starts a unit."""
        self._close()
        self.unit_bits.append(self.w.pos)
        self.blk = self.w.dynamic(LIT, DIST, final=final)
        return self

    def fixed(self, final=False):
        self._close()
        if not self.w.pos:
            self.unit_bits.append(0)
        self.blk = self.w.fixed(final)

    def stored(self, payload, final=False):
        """Writer.stored for a long payload: the same bits and marks, the bytes through numpy."""
        self._close()
        w = self.w
        if not w.pos:
            self.unit_bits.append(0)
        w.header(final, 0)
        w.align()
        w.hw = max(w.hw, w.pos)
        w.put_read(len(payload), 16)
        w.put_read(~len(payload) & 0xffff, 16)
        w.bits.extend(np.unpackbits(np.frombuffer(bytes(payload), np.uint8), bitorder="little").tolist())
        w.need(0)
        w.out += payload

    def lits(self, data):
        self.blk.lits(data)

    def match(self, length, dist, src=None, twin=False):
        """A copy; src = the unit its source starts in marks it.  twin: the copy that the failing twin moves."""
        pos = len(self.w.out)
        if twin:
            dist += self.over
        if not self.blk.match(length, dist) and self.front is None:
            self.front = bytes(self.w.out)
        if src is not None:
            self.marks.append((pos, length, dist))
            self.src.append(src)
            self.mark_unit.append(len(self.unit_bits) - 1)

    def raw(self):
        self._close()
        return np.packbits(np.array(self.w.bits, np.uint8), bitorder="little").tobytes()


def ground(n, seed):
    return gzip_ref.rand(n, seed=seed)


def ground_unit(s, n, seed):
    """A unit of exactly n bytes (n >= 1): one literal, the rest stored (and, beyond 65535 of those, literals of a
    fixed block)."""
    g = ground(n, seed)
    s.unit()
    s.lits(g[:1])
    s.stored(g[1:65536])
    if n > 65536:
        s.fixed()
        s.lits(g[65536:])


# ---- the good streams (each builder takes `over`: 0, or 1 for the failing twin) ----

def far_reach(over=0):
    s = Stream("far reach: five empty units, then match(258, 32768) as a unit's first token", over)
    ground_unit(s, W, 31)
    for _ in range(5):
        s.unit()
    s.unit()
    s.match(258, W, src=0)
    s.unit()
    s.match(3, 1, src=6)
    s.lits(ground(9, 32))
    s.match(258, 1, src=7)
    s.unit(final=True)
    s.match(10, W, src=0)
    s.lits(b"end")
    return s


def far_distance(d, k):
    def build(over=0):
        s = Stream("distance %d, the source %d units back" % (d, k), over)
        ground_unit(s, W + 300, 40 + k)
        for i in range(k - 1):
            s.unit()
            s.lits(ground(1 + i % 3, 50 + i))
        s.unit(final=True)
        s.match(258, d, src=0)
        s.lits(b"!")
        return s
    return build


def unit_size(n):
    def build(over=0):
        s = Stream("a unit of exactly %d bytes, read at distance 32768 and 1" % n, over)
        s.unit()
        s.lits(ground(2, 60))
        ground_unit(s, n, 61)
        s.unit()
        s.match(258, W, src=0 if n < W else 1)  # (n = 32767: THROUGH unit 1 into unit 0, one pass-through entry)
        s.match(258, 1, src=2)
        s.lits(ground(3, 62))
        s.unit(final=True)
        s.match(3, 1, src=2)
        return s
    return build


def early_fourth_unit(over=0):
    s = Stream("total < 32768: the 4th unit copies at distance == total", over)
    s.unit()
    s.lits(ground(20, 70))
    s.unit()
    s.lits(ground(2, 71))
    s.unit()
    s.lits(ground(3, 72))
    s.unit(final=True)
    s.match(20, 25, src=0, twin=True)
    s.lits(b"?")
    return s


def early_at(total):
    def build(over=0):
        s = Stream("a unit starts at total == %d and copies at distance == total" % total, over)
        ground_unit(s, total, 73)
        s.unit(final=True)
        s.match(258, total, src=0, twin=True)
        s.lits(b"?")
        return s
    return build


def overlap(ground_bytes):
    def build(over=0):
        where = "total > 32768" if ground_bytes > W else "total < 32768"
        s = Stream("overlapping copies across the unit boundary, %s" % where, over)
        ground_unit(s, ground_bytes, 80)
        for i, d in enumerate(OVERLAP_DISTANCES):
            s.unit()
            s.match(258, d, src=i)  # (the whole source lies in the unit in front)
            s.lits(ground(70, 81 + i))
        s.unit(final=True)
        s.lits(ground(2, 90))
        s.match(258, 5, src=len(OVERLAP_DISTANCES))  # (three bytes of the unit in front, two of this one)
        return s
    return build


PASS_UNITS = 70


def long_pass_through(over=0):
    s = Stream("long pass-through: a byte read through %d units" % PASS_UNITS, over)
    ground_unit(s, W, 91)
    for i in range(PASS_UNITS):
        s.unit()
        s.lits(bytes([0x30 + i]))
    s.unit(final=True)
    s.match(258, W, src=0)
    s.match(PASS_UNITS, PASS_UNITS + 258, src=1)
    return s


def stored_inside(over=0):
    s = Stream("stored blocks of 65535 and 0 bytes inside a unit that the next unit reads at distance 32768", over)
    s.unit()
    s.stored(ground(65535, 92))
    s.stored(b"")
    s.fixed()
    s.match(5, W, src=0)
    s.unit(final=True)
    s.match(258, W, src=0)
    s.match(258, 1, src=1)
    return s


def empty_three(over=0):
    s = Stream("three empty units and nothing else", over)
    s.unit().unit().unit(final=True)
    return s


def empty_first(over=0):
    s = Stream("the first unit is empty", over)
    s.unit()
    s.unit()
    s.lits(ground(9, 93))
    s.unit(final=True)
    s.match(4, 9, src=1, twin=True)  # (distance == total: the stream's first byte)
    return s


def empty_last(over=0):
    s = Stream("the last unit is empty", over)
    s.unit()
    s.lits(ground(9, 94))
    s.unit()
    s.match(4, 5, src=0)
    s.lits(ground(2, 95))
    s.unit(final=True)
    return s


BUILDERS = ([far_reach] + [far_distance(d, k) for d in FAR_DISTANCES for k in UNITS_BACK]
            + [unit_size(n) for n in UNIT_SIZES]
            + [early_fourth_unit, early_at(W - 1), early_at(W), overlap(300), overlap(W + 300), long_pass_through,
               stored_inside, empty_three, empty_first, empty_last])
# what the corpus has to hold, by (part of) the name
REQUIRED = (["far reach", "long pass-through", "stored blocks of 65535 and 0 bytes", "three empty units",
             "the first unit is empty", "the last unit is empty", "the 4th unit copies at distance == total",
             "total == 32767 and copies", "total == 32768 and copies",
             "overlapping copies across the unit boundary, total < 32768",
             "overlapping copies across the unit boundary, total > 32768"]
            + ["distance %d, the source %d units back" % (d, k) for d in FAR_DISTANCES for k in UNITS_BACK]
            + ["a unit of exactly %d bytes" % n for n in UNIT_SIZES])
CUT = ("far reach", "long pass-through")  # the good streams that are also cut inside the marked copy's unit

_built = {}


def _all():
    if not _built:
        good, intents, twins = [], {}, []
        for b in BUILDERS:
            s = b()
            raw, plain = s.raw(), bytes(s.w.out)
            assert s.front is None, s.what  # (the Writer took every copy)
            good.append((s.what, raw, plain, list(s.marks)))
            intents[s.what] = (len(s.unit_bits), list(s.src))
            if any(pos == d < W for pos, _, d in s.marks):  # distance == total < W: the twin reaches one byte too far
                t = b(over=1)
                traw = t.raw()
                assert t.front is not None, s.what
                twins.append((s.what + "; distance + 1", traw, t.front, "far"))
            if s.what.startswith(CUT):
                u = s.mark_unit[0]
                end = s.unit_bits[u + 1] if u + 1 < len(s.unit_bits) else 8 * len(raw)
                twins.append((s.what + "; cut inside unit %d" % u, raw[:(s.unit_bits[u] + end) // 16], plain, "cut"))
                if u + 1 == len(s.unit_bits):  # behind its copies too: the failing unit delivers what it read through
                    twins.append((s.what + "; cut in front of the last byte", raw[:-1], plain, "cut"))
        _built.update(good=good, intents=intents, twins=twins)
    return _built


def good_streams():
    return list(_all()["good"])


def intent(what):
    return _all()["intents"][what]


def failing_twins():
    return list(_all()["twins"])
