"""The slot corpus: batches for the decoders' WRITE FOOTPRINT, and the exact memory image a call must leave.

The batch decoders store wide (16-byte copies, 8-byte literal words, 32- and 64-byte rows, LDS window flushes), in a
shape that depends on how far a stream is from the end of its output slot.  Packed slots hide a store that crosses
into a neighbour's slot: the neighbour overwrites it later, or it lands in the neighbour's unspecified tail.  Here
every real stream lies between two GUARD streams -- streams that produce no bytes, and so, in a call with device
pointers (include/flate_hip.h), write nothing -- in an output buffer prefilled with 0xA5.  Every byte outside the real
streams' unspecified tails [out_off[i] + out_len[i], out_off[i+1]) is compared, so a store that leaves its slot shows
whatever the order of the lanes.  No GPU is needed here: tests/test_slot_corpus.py checks the checker against mutants of a plain Python decoder,
tests/test_gpu_inflate_slots.py runs the batches through every decoder configuration.

Real streams: every length of LENGTHS x every fill of FILLS x four encoders.  Guards: one between every two real
streams and one at each end, their slot sizes from GUARD_SLOTS, so real slots begin at every residue mod 16.
Capacity of real stream k: its size + slack_of(k) (pass "A"); in pass "B" every third one gets size - d, and the
expectation is what the oracle delivers with E_OUT_TOO_SMALL."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from framed_read_ref import NO_DICT, expected as framed_expected, oracle_member
from util import STATUS_OF_ORACLE, flate, make_streams

FILL = 0xA5          # what the output buffer holds before the call
OUTER = 256          # compared bytes in front of and behind the slots' range
LENGTHS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 259, 260, 300, 1000,
           4097, 65535, 65536, 70000]
FILLS = ["text", "zero", "period", "runs", "rand"]
ENCODERS = ["oracle", "zlib9", "fixed", "stored"]
DICT_ENCODERS = ["zlib9", "fixed", "stored", "zlib1"]  # (the oracle's encoder takes no dictionary)
GUARD_SLOTS = [1, 2, 3, 5, 7, 8, 13, 16, 31, 33, 64]
# The slack values lie on both sides of the 8-, 16-, 32- and 64-byte thresholds of the stores.  A zero stands between
# every two of them, so that more than half of the streams end right in front of a guard, nothing of their slot left
# uncompared (a cycle with some of the values side by side -- ... 8, 9, 0, 15, 16, 0 ... -- has 10 zeros in 25, too few
# for that); the cycle's length (31) shares no factor with the 20 (fill, encoder) pairs of one length.
SLACKS = [0, 0, 1, 0, 3, 0, 4, 0, 7, 0, 8, 0, 9, 0, 15, 0, 16, 0, 17, 0, 31, 0, 32, 0, 33, 0, 63, 0, 64, 0, 65]
SHORT_BY = [1, 2, 7, 8, 9, 16, 17, 33, 64, 259]  # pass B: capacity = size - d
GUARD_INPUTS = [b"", b"\x07"]  # unexpected EOF / BTYPE 3: corrupt at offset 1 -- both without a byte of output

Meta = namedtuple("Meta", "fill encoder length slack")
Violation = namedtuple("Violation", "kind stream distance message")
# kind: "outer_guard"  a byte outside [out_off[0], out_off[n]) was written
#       "guard_slot"   a byte in the slot of a stream that produces nothing was written; stream = the nearest real
#                      stream, distance = bytes from that stream's slot border (1 = the byte next to it; negative:
#                      in front of the stream's slot, positive: behind it)
#       "bytes"        bytes a stream produced differ; distance = offset of the first one inside the slot
#       "result"       status, out_len or err_off differ


def slack_of(k):
    return SLACKS[k % len(SLACKS)]


@functools.lru_cache(maxsize=None)
def payloads():
    """[(fill, bytes)]: one payload per (length, fill), lengths outermost (computed once, shared, never changed)."""
    specs = [(fill, n) for n in LENGTHS for fill in FILLS]
    data, off = make_streams(specs, seed=4242)
    return [(specs[i][0], data[int(off[i]):int(off[i + 1])].tobytes()) for i in range(len(specs))]


@functools.lru_cache(maxsize=None)
def shared_dict():
    """One 32 KiB dictionary of the text the text payloads are made of, with the head of the long text payloads in
    it, so that their first matches reach in front of the output."""
    heads = b"".join(p[:600] for fill, p in payloads() if fill == "text" and len(p) >= 1000)
    return (flate.synth("text", 1, 32768, seed=0x5EED0001, first_stream=977).tobytes() + heads)[-32768:]


def _zlib_raw(p, level, strategy=zlib.Z_DEFAULT_STRATEGY, zdict=None):
    kw = {"zdict": zdict} if zdict else {}
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy, **kw)
    return co.compress(p) + co.flush()


def encode(oracle, name, p, zdict=None):
    if name == "oracle":  # stored tails of 1..16 bytes, Huffman-only blocks under 128 bytes
        assert zdict is None
        return oracle.deflate(np.frombuffer(p, np.uint8))
    if name == "zlib9":   # matches up to the very last byte
        return _zlib_raw(p, 9, zdict=zdict)
    if name == "zlib1":
        return _zlib_raw(p, 1, zdict=zdict)
    if name == "fixed":
        return _zlib_raw(p, 6, zlib.Z_FIXED, zdict=zdict)
    if name == "stored":
        return _zlib_raw(p, 0, zdict=zdict)
    raise ValueError(name)


class Batch:
    """One call's arguments and the memory image it must leave.

    streams[i]   input of stream i (framed: the member); meta[i] = Meta of a real stream, None of a guard
    caps         slot sizes; out_off = their running sum, counted from the first slot
    want_*       expected status, err_off, out_len per stream; want_bytes[i] = the bytes stream i delivers
    image        uint8[OUTER + out_off[n] + OUTER]: 0xA5 with every stream's bytes in place
    mask         True where `image` is compared: everywhere but the real streams' tails beyond out_len
    """

    def __init__(self, streams, meta, caps, results):
        self.streams, self.meta = list(streams), list(meta)
        self.n = len(streams)
        self.caps = np.array(caps, dtype=np.uint64)
        self.out_off = np.zeros(self.n + 1, np.uint64)
        np.cumsum(self.caps, out=self.out_off[1:])
        self.total = int(self.out_off[-1])
        self.want_status = np.array([r[0] for r in results], np.int32)
        self.want_err_off = np.array([r[1] for r in results], np.int64)
        self.want_bytes = [r[2] for r in results]
        self.want_len = np.array([len(b) for b in self.want_bytes], np.uint64)
        self.real = [i for i, m in enumerate(self.meta) if m is not None]
        self.image = np.full(OUTER + self.total + OUTER, FILL, np.uint8)
        self.mask = np.ones(self.image.size, bool)
        for i in range(self.n):
            a, e, k = OUTER + int(self.out_off[i]), OUTER + int(self.out_off[i + 1]), len(self.want_bytes[i])
            assert k <= e - a
            self.image[a:a + k] = np.frombuffer(self.want_bytes[i], np.uint8)
            if k:  # (a stream that produces nothing writes nothing: its whole slot is compared, real or guard)
                self.mask[a + k:e] = False
        for i, m in enumerate(self.meta):  # guards produce nothing, and every real stream has a guard on each side
            assert (m is None) == (i % 2 == 0) and (m is not None or self.want_len[i] == 0), i
        assert self.meta[0] is None and self.meta[-1] is None
        self.image.setflags(write=False)
        self.mask.setflags(write=False)
        # optional arguments of the variants
        self.zdict = None       # dictionary batch: the shared dictionary; dict_of = per stream, NO_DICT for guards
        self.dict_of = None
        self.spliced = None     # spliced batch: the one stream, and bit_off[n+1] with empty pieces for the guards
        self.bit_off = None

    def in_blob(self):
        """(data uint8[] with 16 spare bytes behind it, in_off uint64[n+1])"""
        off = np.zeros(self.n + 1, np.uint64)
        np.cumsum(np.array([len(s) for s in self.streams], dtype=np.uint64), out=off[1:])
        return np.frombuffer(b"".join(self.streams) + b"\0" * 16, np.uint8).copy(), off

    def describe(self, i):
        m = self.meta[i]
        if m is None:
            return "stream %d (guard, slot of %d)" % (i, int(self.caps[i]))
        return "stream %d (fill %s, encoder %s, length %d, slack %d, slot start mod 64 = %d)" % (
            i, m.fill, m.encoder, m.length, m.slack, int(self.out_off[i]) % 64)

    def slot_starts(self):
        return [int(self.out_off[i]) for i in self.real]

    # ---- the checker ----

    def check(self, image_after, out_len, status, err_off):
        """The violations of the footprint property in what a call left: a list of Violation (empty = none).
        image_after: the whole buffer, OUTER bytes in front of out + out_off[0] and OUTER behind out + out_off[n]."""
        image_after = np.asarray(image_after, dtype=np.uint8)
        assert image_after.shape == self.image.shape
        out = []
        got = np.stack([np.asarray(status, np.int64), np.asarray(out_len).astype(np.int64),
                        np.asarray(err_off, np.int64)])
        want = np.stack([self.want_status.astype(np.int64), self.want_len.astype(np.int64), self.want_err_off])
        assert got.shape == want.shape, (got.shape, want.shape)
        for i in np.nonzero((got != want).any(axis=0))[0]:
            out.append(Violation("result", int(i), 0, "%s: (status, out_len, err_off) = %s, expected %s" % (
                self.describe(i), tuple(got[:, i].tolist()), tuple(want[:, i].tolist()))))
        bad = np.nonzero((image_after != self.image) & self.mask)[0]
        if bad.size == 0:
            return out
        lo, hi = OUTER, OUTER + self.total
        for side, idx in (("in front of", bad[bad < lo]), ("behind", bad[bad >= hi])):
            if idx.size:
                near = self.real[0] if side == "in front of" else self.real[-1]
                d = int(idx[-1]) - lo if side == "in front of" else int(idx[0]) - hi + 1
                out.append(Violation("outer_guard", near, d, "%d bytes %s the slots' range written (the nearest %d from "
                                     "it); nearest real stream: %s" % (idx.size, side, abs(d), self.describe(near))))
        inside = bad[(bad >= lo) & (bad < hi)] - lo
        owner = np.searchsorted(self.out_off.astype(np.int64), inside, side="right") - 1
        for i in np.unique(owner):
            at = inside[owner == i]
            a, e = int(self.out_off[i]), int(self.out_off[i + 1])
            if self.want_len[i]:
                first = int(at[0]) - a
                out.append(Violation("bytes", int(i), first, "%s: %d produced bytes differ, the first at %d of %d" % (
                    self.describe(i), at.size, first, int(self.want_len[i]))))
                continue
            # a slot nobody may write: blame the nearer real neighbour (a real stream that delivers nothing: itself)
            if self.meta[i] is not None:
                near, d, how = int(i), 0, "its own slot"
            else:
                behind, front = int(at[0]) - a + 1, e - int(at[-1])  # distance from the slot in front / behind
                if i == self.n - 1 or (i > 0 and behind <= front):
                    near, d, how = int(i) - 1, behind, "%d behind its slot" % behind
                else:
                    near, d, how = int(i) + 1, -front, "%d in front of its slot" % front
            out.append(Violation("guard_slot", near, d, "%d bytes written in the slot of stream %d, which produces "
                                 "nothing (slot [%d, %d), bytes %d..%d): %s of %s" % (
                                     at.size, i, a, e, int(at[0]), int(at[-1]), how, self.describe(near))))
        return out


def report(violations, limit=6):
    return "%d violations of the slot property, the first:\n  %s" % (
        len(violations), "\n  ".join(v.message for v in violations[:limit]))


def _guard_slot(g):
    return GUARD_SLOTS[g % len(GUARD_SLOTS)]


def _interleave(reals, guard):
    """G R G R ... R G: reals = [(stream, meta, cap, result)], guard(g) = the same for guard g."""
    rows = []
    for k, r in enumerate(reals):
        rows += [guard(k), r]
    rows.append(guard(len(reals)))
    return Batch(*zip(*rows))


def _assert_conditions(batch):
    """What makes the corpus worth running: real slots start at every residue mod 16 and at 32 or more mod 64, and at
    least half of the real streams end right in front of a guard."""
    starts = batch.slot_starts()
    assert {s % 16 for s in starts} == set(range(16))
    assert len({s % 64 for s in starts}) >= 32
    tight = sum(1 for i in batch.real if batch.meta[i].slack == 0)
    assert 2 * tight >= len(batch.real), (tight, len(batch.real))


def _raw_batch(oracle, encoders, pass_, zdict):
    assert pass_ in ("A", "B")
    guards = []
    for g_in in GUARD_INPUTS:  # (checked here, on the CPU: the guards' verdicts, and that they deliver nothing)
        rc, got, _, eoff = oracle.inflate(g_in, 64, full=True)
        guards.append((STATUS_OF_ORACLE[rc], eoff, got))
    assert guards == [(-7, -1, b""), (-4, 1, b"")], guards
    reals = []
    for fill, p in payloads():
        for enc in encoders:
            k = len(reals)
            s = encode(oracle, enc, p, zdict)
            slack = slack_of(k)
            cap = len(p) + slack
            if pass_ == "B" and k % 3 == 0:
                d = SHORT_BY[k // 3 % len(SHORT_BY)]
                if len(p) > d:
                    cap, slack = len(p) - d, -d
            rc, got, _, eoff = oracle.inflate(s, cap, full=True, zdict=zdict)
            if cap >= len(p):
                assert rc == 0 and got == p, (fill, enc, len(p), rc)
            else:  # the oracle refuses whole tokens: up to 257 bytes below the capacity, and a stored block as a whole
                assert rc == oracle.E_OUT_TOO_SMALL and len(got) <= cap and got == p[:len(got)]
            reals.append((s, Meta(fill, enc, len(p), slack), cap, (STATUS_OF_ORACLE[rc], eoff, got)))
    b = _interleave(reals, lambda g: (GUARD_INPUTS[g % 2], None, _guard_slot(g), guards[g % 2]))
    if pass_ == "A":
        _assert_conditions(b)
    else:
        short = [-b.meta[i].slack for i in b.real if b.meta[i].slack < 0]  # every d on several streams
        assert all(short.count(d) >= 5 for d in SHORT_BY), short
    return b


@functools.lru_cache(maxsize=None)
def plain(oracle, pass_="A"):
    """flate_hip_inflate_batch: the payloads by four encoders."""
    return _raw_batch(oracle, ENCODERS, pass_, None)


@functools.lru_cache(maxsize=None)
def dictionary(oracle):
    """flate_hip_inflate_batch_dict: the payloads compressed against one shared dictionary; guards without one."""
    d = shared_dict()
    b = _raw_batch(oracle, DICT_ENCODERS, "A", d)
    b.zdict = d
    b.dict_of = np.array([NO_DICT if m is None else 0 for m in b.meta], np.uint32)
    # the dictionary is needed: without it some of the streams reach in front of their output
    needs = sum(1 for i in b.real if oracle.inflate(b.streams[i], int(b.caps[i]), full=True)[0] == oracle.E_CORRUPT)
    assert needs >= 20, needs
    return b


@functools.lru_cache(maxsize=None)
def spliced(oracle):
    """flate_hip_inflate_spliced: the payloads as the pieces of ONE stream of the oracle's spliced compressor; the
    guards are empty pieces (bit_off[i] == bit_off[i+1]: status 0, nothing produced) with slots of their own."""
    pl = payloads()
    data = np.frombuffer(b"".join(p for _, p in pl) + b"\0", np.uint8)
    off = np.zeros(len(pl) + 1, np.uint64)
    np.cumsum(np.array([len(p) for _, p in pl], dtype=np.uint64), out=off[1:])
    stream, bit_off = oracle.deflate_spliced(data, off)
    assert oracle.inflate(stream, int(off[-1])) == data[:int(off[-1])].tobytes()
    reals = [(b"", Meta(fill, "spliced", len(p), slack_of(k)), len(p) + slack_of(k), (0, -1, p))
             for k, (fill, p) in enumerate(pl)]
    b = _interleave(reals, lambda g: (b"", None, _guard_slot(g), (0, -1, b"")))
    _assert_conditions(b)
    b.spliced = stream
    b.bit_off = np.repeat(bit_off, 2)  # guard g starts and ends where real piece g starts; the last: at the closing block
    assert b.bit_off.size == b.n + 1
    return b


@functools.lru_cache(maxsize=None)
def framed(oracle):
    """flate_hip_inflate_batch_framed, zlib wrap: the payloads as zlib members; the guards are members whose first
    header byte is bad -- a whole valid member behind it, or nothing -- so they are corrupt and deliver nothing."""
    probe = oracle_member(oracle, "zlib", b"a guard's payload, never to be seen " * 3)
    guard_members = [b"\x77" + probe[1:], b"\x00"]
    guards = []
    for m in guard_members:
        st, eo, got, j = framed_expected(oracle, m, "zlib", 64, None)
        guards.append((st, eo, got))
    assert guards == [(-4, 0, b""), (-4, 0, b"")], guards
    reals = []
    for fill, p in payloads():
        for enc in ENCODERS:
            k = len(reals)
            m = oracle_member(oracle, "zlib", p) if enc == "oracle" else \
                b"\x78\x01" + encode(oracle, enc, p) + zlib.adler32(p).to_bytes(4, "big")
            cap = len(p) + slack_of(k)
            st, eo, got, j = framed_expected(oracle, m, "zlib", cap, None)
            assert st == 0 and got == p and j == NO_DICT, (fill, enc, len(p), st)
            reals.append((m, Meta(fill, enc, len(p), slack_of(k)), cap, (st, eo, got)))
    b = _interleave(reals, lambda g: (guard_members[g % 2], None, _guard_slot(g), guards[g % 2]))
    _assert_conditions(b)
    return b


# ---- a plain decoder: writes exactly the expected bytes -- the checker's clean case, and what its mutants change ----

def plain_decode(batch, scribble_tails=False):
    """(image, out_len, status, err_off) of a decoder that stores every stream's bytes and nothing else; with
    scribble_tails it also fills the real streams' slots beyond out_len, which the contract leaves unspecified."""
    img = np.full(batch.image.size, FILL, np.uint8)
    for i in range(batch.n):
        a, e, k = OUTER + int(batch.out_off[i]), OUTER + int(batch.out_off[i + 1]), len(batch.want_bytes[i])
        img[a:a + k] = np.frombuffer(batch.want_bytes[i], np.uint8)
        if scribble_tails and k:
            img[a + k:e] = 0x3C
    return img, batch.want_len.copy(), batch.want_status.copy(), batch.want_err_off.copy()


def store(img, batch, i, at, width):
    """A decoder's wide store of stream i at offset `at` of its slot, not clipped to the slot: the stream's own bytes
    where it has them, other bytes beyond (each different from what is there)."""
    a = OUTER + int(batch.out_off[i]) + at
    own = np.frombuffer(batch.want_bytes[i], np.uint8)
    for j in range(width):
        img[a + j] = own[at + j] if 0 <= at + j < own.size else img[a + j] ^ 0x5A
