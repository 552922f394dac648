"""Damaged multi-unit DEFLATE streams on the CPU: the corpus of the unit decoders' damage sweep.

Three small streams of many units each (one_ref.deflate with a lowered memLevel) and, of each, some hundred damaged
versions: one flipped bit in a unit's header, in front of the next header (the end-of-block code), in the token body,
in a stored block's LEN / NLEN / padding; one byte overwritten, deleted, inserted; cuts; two streams crossed inside a
unit.  Every damage is a named record, and every expectation comes from three references that are not the library:
the oracle (status, err_off, out_len, the bytes), one_ref.Walk (the units, `far`, end_bit, reach) and zlib (accept or
reject, the bytes).  The file imports nothing of the library; the oracle module is handed in (the `oracle` fixture).
Everything is seeded: two builds are byte-identical.  `corpus(oracle)` builds once per process and is shared."""
import collections
import hashlib
import random
import struct
import zlib

import gzip_ref
import one_ref as ref

OK, CORRUPT, UNEXPECTED_EOF = ref.OK, ref.CORRUPT, ref.UNEXPECTED_EOF
STATUS_OF_ORACLE = {0: 0, -2: -4, -3: -7, -1: -2}  # (util.STATUS_OF_ORACLE; the GPU sweep holds the two equal)
FLAGS = ("corrupt", "eof", "valid_same_bytes", "valid_other_bytes", "history_only", "past_header", "other_chain",
         "good_units_behind_damage", "later_unit", "stored_header")
KINDS = ("header", "eob", "body", "stored", "overwrite", "delete", "insert", "cut", "crossed")
HEADER_UNITS, EOB_UNITS, BYTE_UNITS, BODY_FLIPS = 12, 6, 6, 12

Base = collections.namedtuple("Base", "name raw plain walk")
# base: the base's name ("a" / "b" / "c"; of a crossed stream the head's); kind: one of KINDS; unit: the unit of the
# base that holds the damage; at: its bit (flips) or byte (byte damage) in the base; raw: the damaged stream;
# true_end: the bit of the DAMAGED stream at which the first true header behind the damage stands -- where the damaged
# unit of the base ends; of a crossed stream where the tail's unit ends (None: a cut in front of that header)
Damage = collections.namedtuple("Damage", "name base kind unit at raw true_end")
# status, err_off, out: the oracle's (status in the library's numbers); walk: one_ref.Walk of raw; zlib_ok, zlib_out:
# zlib's verdict and bytes; flags: the set of class names
Case = collections.namedtuple("Case", "damage status err_off out walk zlib_ok zlib_out flags")


# ---- base streams ----

def bases():
    t = gzip_ref.text(24000, seed=61)
    mixed = t[:8000] + gzip_ref.rand(3000, seed=62) + t[8000:16000]
    made = [("a", ref.deflate(t, 6, mem=1), t), ("b", ref.deflate(mixed, 6, mem=1), mixed), ("c", ref.deflate(t, 1, mem=2), t)]
    out = []
    for name, raw, plain in made:
        w = ref.Walk(raw)
        assert w.status == OK and not w.far and zlib.decompress(raw, -15) == plain and len(plain) < 32768, name
        out.append(Base(name, raw, plain, w))
    return out


def composition(w):
    """(units, dynamic blocks, fixed blocks, stored blocks) of a walk."""
    return (w.n_units,) + tuple(sum(1 for b in w.blocks if b[1] == t) for t in (2, 1, 0))


def header_layout(raw, bit):
    """The dynamic header at `bit` -> (HCLEN's count of code-length lengths, the first bit of the token body)."""
    r = ref.Bits(raw, bit)
    assert r.get(3) >> 1 == 2
    nclen = (r.peek(14) >> 10) + 4
    ref.read_dynamic(r)
    return nclen, r.pos


def unit_of(w, bit):
    return max(k for k in range(w.n_units) if w.unit_bit[k] <= bit)


def spread(n_units, count):
    """`count` units spread evenly over 1 .. n_units - 2: never the first and never the last."""
    inner = list(range(1, n_units - 1))
    if len(inner) <= count:
        return inner
    return sorted({inner[(2 * i + 1) * len(inner) // (2 * count)] for i in range(count)})


# ---- damage ----

def flip(raw, bit):
    b = bytearray(raw)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


def damages(bs=None):
    """[Damage] in a fixed order, names unique.  No reference runs here."""
    bs = bs or bases()
    out, seen = [], set()

    def add(base, kind, unit, at, raw, true_end, what):
        name = "%s/%s/u%d/%s" % (base.name, kind, unit, what)
        assert name not in seen, name
        seen.add(name)
        out.append(Damage(name, base.name, kind, unit, at, bytes(raw), true_end))

    for bi, base in enumerate(bs):
        raw, w = base.raw, base.walk
        rnd = random.Random(1000 + bi)
        units = spread(w.n_units, HEADER_UNITS)
        for k in units:
            u, end = w.unit_bit[k], w.unit_bit[k + 1]
            nclen, body = header_layout(raw, u)
            rl = 17 + 3 * nclen  # the first bit of the run-length coded lengths, counted from the header
            spots = [("bfinal", 0), ("btype0", 1), ("btype1", 2), ("hlit", 4), ("hdist", 9), ("hclen", 14),
                     ("cl1", 17 + 3 * 1 + 1), ("cl_last", 17 + 3 * (nclen - 1)),
                     ("rl_a", rl + (body - u - rl) // 3), ("rl_b", rl + 2 * (body - u - rl) // 3)]
            for what, o in spots:
                assert o < body - u
                add(base, "header", k, u + o, flip(raw, u + o), end, "%s+%d" % (what, o))
            assert end - 15 > body + BODY_FLIPS
            for bit in sorted(rnd.sample(range(body, end - 15), BODY_FLIPS)):
                add(base, "body", k, bit, flip(raw, bit), end, "bit%d" % (bit - u))
        for k in spread(w.n_units, EOB_UNITS):
            end = w.unit_bit[k + 1]
            for back in range(15, 0, -1):
                add(base, "eob", k, end - back, flip(raw, end - back), end, "end-%d" % back)
        if any(b[1] == 0 for b in w.blocks):
            for j, (at, typ, final, n) in enumerate(w.blocks):
                if typ != 0:
                    continue
                p = (at + 3 + 7) // 8  # LEN's byte
                k = unit_of(w, at)
                end = w.unit_bit[k + 1]
                spots = [("len0", 8 * p), ("len9", 8 * p + 9), ("nlen3", 8 * p + 16 + 3), ("nlen15", 8 * p + 31)]
                if 8 * p > at + 3:
                    spots.append(("pad", at + 3))
                for what, bit in spots[j % 2::2] if j % 4 else spots:  # every fourth block all of them, else half
                    add(base, "stored", k, bit, flip(raw, bit), end, "s%d_%s" % (j, what))
        for k in spread(w.n_units, BYTE_UNITS):
            u, end = w.unit_bit[k], w.unit_bit[k + 1]
            mid = (u + end) // 16
            other = (raw[mid] + 1 + rnd.randrange(255)) & 255
            assert other != raw[mid]
            add(base, "overwrite", k, mid, raw[:mid] + bytes([other]) + raw[mid + 1:], end, "byte%d" % mid)
            add(base, "delete", k, mid, raw[:mid] + raw[mid + 1:], end - 8, "byte%d" % mid)
            add(base, "insert", k, mid, raw[:mid] + bytes([rnd.randrange(256)]) + raw[mid:], end + 8, "byte%d" % mid)
            add(base, "cut", k, mid, raw[:mid], None, "byte%d" % mid)
            for d in (-1, 0, 1):  # (reach[k]: the three bits of the next header included)
                n = w.reach[k] + d
                add(base, "cut", k, n, raw[:n], end if 8 * n >= end + 3 else None, "reach%+d" % d)
    for hi, head in enumerate(bs):
        for ti, tail in enumerate(bs):
            if hi == ti:
                continue
            for k, j in zip(spread(head.walk.n_units, 3), spread(tail.walk.n_units, 3)[::-1]):
                a = (head.walk.unit_bit[k] + head.walk.unit_bit[k + 1]) // 16
                b = (tail.walk.unit_bit[j] + tail.walk.unit_bit[j + 1]) // 16
                add(head, "crossed", k, a, head.raw[:a] + tail.raw[b:], tail.walk.unit_bit[j + 1] + 8 * (a - b),
                    "%s_u%d" % (tail.name, j))
    return out


def digest(ds):
    h = hashlib.sha256()
    for d in ds:
        h.update(repr(d[:5] + (d.true_end,)).encode() + d.raw)
    return h.hexdigest()


# ---- expectations ----

def zlib_verdict(raw):
    """(accepted, the bytes as far as zlib comes): accepted iff the stream ends, with or without bytes behind it."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw)
    except zlib.error:
        return False, b""
    return d.eof, out


def judge(d, base, oracle):
    """One damaged stream against the three references -> Case."""
    w = ref.Walk(d.raw)
    rc, out, _, err_off = oracle.inflate(d.raw, w.out_len + 600, full=True)
    status = STATUS_OF_ORACLE[rc]
    zok, zout = zlib_verdict(d.raw)
    flags = set()
    if status == CORRUPT:
        flags.add("corrupt")
    if status == UNEXPECTED_EOF:
        flags.add("eof")
    if status == OK:
        flags.add("valid_same_bytes" if out == base.plain else "valid_other_bytes")
    if w.status == OK and status == CORRUPT:
        flags.add("history_only")
    if d.true_end is not None:
        if status != OK and w.status != OK and w.end_bit > d.true_end:
            flags.add("past_header")
        if status == CORRUPT and 8 * (err_off - 1) >= d.true_end:
            flags.add("later_unit")  # the whole of the last byte taken lies behind the damaged unit's true end
    if w.status == OK and w.unit_bit != base.walk.unit_bit:
        flags.add("other_chain")
    if w.n_units > d.unit + 1:
        flags.add("good_units_behind_damage")  # the walk completes units behind the damaged one
    if d.kind == "stored":
        flags.add("stored_header")
    return Case(d, status, err_off, out, w, zok, zout, frozenset(flags))


Corpus = collections.namedtuple("Corpus", "bases cases")
_CACHE = {}


def corpus(oracle):
    """The judged corpus, built once per process: Corpus(bases {name: Base}, cases [Case])."""
    if "corpus" not in _CACHE:
        bs = bases()
        by = {b.name: b for b in bs}
        _CACHE["corpus"] = Corpus(by, [judge(d, by[d.base], oracle) for d in damages(bs)])
    return _CACHE["corpus"]


def counts(cases):
    c = collections.Counter()
    for x in cases:
        c.update(x.flags)
    return {f: c[f] for f in FLAGS}


# ---- what the framed and the file calls must say of a damaged stream (references only) ----

def framed_expect(c, f):
    """The member f = header + c's stream + a trailer -> (status, err_off, the bytes), the framed serial verdict
    (framed_read_ref.expected): the decoder's own status first, then the trailer at err_off = len(f)."""
    if c.status != OK:
        return c.status, c.err_off, c.out
    gz = f[:2] == b"\x1f\x8b"
    want = struct.pack("<II", zlib.crc32(c.out), len(c.out) & 0xffffffff) if gz else struct.pack(">I", zlib.adler32(c.out))
    return (OK, -1, c.out) if f[-len(want):] == want else (CORRUPT, len(f), c.out)


def gzfile_expect(oracle, f, w, front, behind):
    """The three-member file f whose MIDDLE member holds a damaged stream -> ((status, bad_member, err_off,
    stream_err_off), the bytes delivered, history): the verdict order of the read.  w: gzfile_ref.Walk(f); front, behind:
    (member, plain) of the members around it.  The middle member's stream is read over [r, len(f) - 8), as the walk
    reads it, by the oracle; history: the oracle's verdict is one the history-free walk cannot give."""
    none = 0xffffffff
    p, r = len(front[0]), len(front[0]) + len(gzip_ref.header())
    assert w.member_off[:2] == [0, p]
    span = f[r:len(f) - 8]
    rc, out, _, eo = oracle.inflate(span, ref.Walk(span).out_len + 600, full=True)
    st = STATUS_OF_ORACLE[rc]
    if st != OK:  # the chain breaks in the middle member, at the serial offset
        history = not (w.status == st and w.bad_member == 1 and w.stream_err_off == eo)
        assert not history or (w.far and st == CORRUPT)
        return (st, 1, p, eo), front[1] + out, history
    assert w.n_members >= 2 or w.bad_member >= 2
    if w.status != OK:  # ... behind it: the hop lands where no member starts
        assert w.bad_member == 2 and w.status == CORRUPT and w.stream_err_off == -1
        return (w.status, 2, w.err_off, -1), front[1] + out, False
    assert w.n_members == 3 and f[w.member_off[2]:] == behind[0]
    if f[w.member_off[2] - 8:w.member_off[2]] != struct.pack("<II", zlib.crc32(out), len(out) & 0xffffffff):
        return (CORRUPT, 1, p, w.member_off[2] - p), front[1] + out + behind[1], False
    return (OK, none, -1, -1), front[1] + out + behind[1], False
