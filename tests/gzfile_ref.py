"""A gzip file of any members on the CPU: the reference of flate_hip_gzfile_index / flate_hip_gzfile_read.

`Walk` is the walk of include/flate_hip.h restated here from gzip_ref's header rule and one_ref.Walk per member: bits
are counted from the FILE's first byte, a member's raw stream is read over [r, len - 8), its units are one_ref's, and
the hop behind a final block is e = ceil(b / 8) + 8.  It keeps no history and reads no trailer, as the index call.
Truth about a file's CONTENT comes from zlib: `members_of` walks zlib.decompressobj(31) over unused_data.  The file also
builds the corpus the tests of the two calls share; a test module computes each walk once."""
import struct
import zlib

import gzip_ref as gz
import one_ref

OK, OUT_TOO_SMALL, CORRUPT, TOO_LARGE, UNEXPECTED_EOF = 0, -2, -4, -6, -7
NONE = 0xffffffff


def hop(buf, b):
    """THE HOP behind a final block that ends at bit b -> ("end" | "dead" | "next", e, the next member's first bit)."""
    e = (b + 7) // 8 + 8
    if e >= len(buf):
        return ("end" if e == len(buf) else "dead"), e, 0
    hl = gz.header_len(buf, e, len(buf))
    return ("next", e, 8 * (e + hl)) if hl else ("dead", e, 0)


class Walk:
    """status, bad_member (NONE), err_off, stream_err_off (-1), n_units, n_members, out_bytes (0 unless status == 0),
    unit_bit / out_off (n_units + 1 entries), member_off / member_unit (n_members + 1 entries) -- of a broken chain the
    good prefix, entry n_units where the failing unit starts, entry n_members the failing member (or where no member
    could start, with member_unit = n_units) --, out_len (the bytes a read delivers: in front of the failure), sizes
    (what every whole member inflates to), end_bits (the bit behind every whole member's final block), far (some distance reached in front of its member)."""

    def __init__(self, buf):
        buf = bytes(buf)
        n = len(buf)
        self.status, self.bad_member, self.err_off, self.stream_err_off = OK, NONE, -1, -1
        self.unit_bit, self.out_off, self.member_off, self.member_unit = [], [], [], []
        self.sizes, self.end_bits, self.far = [], [], False
        p, total, end_bit, end_out = 0, 0, 0, 0
        while p < n:
            hl = gz.header_len(buf, p, n)
            if not hl:  # no member can start here
                self.status, self.err_off = CORRUPT, p
                self.member_off.append(p)
                self.member_unit.append(len(self.unit_bit))
                break
            r = p + hl
            w = one_ref.Walk(buf[r:max(r, n - 8)])
            self.far = self.far or w.far
            self.member_off.append(p)
            self.member_unit.append(len(self.unit_bit))
            self.unit_bit += [8 * r + b for b in w.unit_bit[:w.n_units]]
            self.out_off += [total + o for o in w.out_off[:w.n_units]]
            if w.status:  # the walk ends in this member: where the failing unit starts, what is delivered
                self.status, self.err_off, self.stream_err_off = w.status, p, w.err_off
                end_bit, end_out = 8 * r + w.unit_bit[w.n_units], total + w.out_off[w.n_units]
                total += w.out_len
                break
            self.sizes.append(w.out_len)
            total += w.out_len
            end_bit, end_out = 8 * r + w.end_bit, total
            self.end_bits.append(end_bit)
            p = (end_bit + 7) // 8 + 8
            assert p <= n  # (the stream ends in front of the file's last 8 bytes)
        self.unit_bit.append(end_bit)
        self.out_off.append(end_out)
        self.n_units = len(self.unit_bit) - 1
        self.out_len = total
        if self.status == OK:
            self.member_off.append(n)
            self.member_unit.append(self.n_units)
        self.n_members = len(self.member_off) - 1
        if self.status:
            self.bad_member = self.n_members
        self.out_bytes = total if self.status == OK else 0

    def index_words(self):
        return (self.status, self.n_units, self.n_members, self.out_bytes, self.bad_member, self.err_off,
                self.stream_err_off)


def members_of(f):
    """What zlib's own gzip reader makes of the file, member by member (raises zlib.error)."""
    out, rest = [], bytes(f)
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        if not d.eof:
            raise zlib.error("the last member is cut short")
        rest = d.unused_data
    return out


def wrap(raw, plain, **hdr):
    """A member around a raw stream."""
    return gz.header(**hdr) + bytes(raw) + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff)


# ---- the corpus ----

def phase_members():
    """24 members of 4 to 9 units each whose final blocks end at all eight bit phases -> [(member, plain)]."""
    t = gz.text(40000, seed=21)
    out = []
    for i in range(24):
        p = t[7 * i:7 * i + 1500 + 131 * i]
        out.append((wrap(one_ref.deflate(p, 6, mem=1), p), p))
    return out


def tiny_file():
    """Members whose first block is stored, fixed and dynamic, an empty member, a 17-byte member, every optional header
    field, 3000 random bytes: few units, many members -> (file, plain)."""
    t = gz.text(6000, seed=5)
    parts = [
        (gz.stored(t[:900]), t[:900]),
        (gz.fixed(t[900:1500]), t[900:1500]),
        (gz.member(t[1500:4000], 6), t[1500:4000]),
        (gz.member(b""), b""),
        (gz.member(t[:17], 6), t[:17]),
        (gz.member(t[4000:4300], 6, flg=gz.FNAME, name=b"a name"), t[4000:4300]),
        (gz.member(t[4300:4600], 6, flg=gz.FEXTRA, extra=b"ab\x03\x00xyz"), t[4300:4600]),
        (gz.member(t[4600:4900], 9, flg=gz.FCOMMENT, comment=b"a comment"), t[4600:4900]),
        (gz.member(t[4900:5200], 1, flg=gz.FHCRC), t[4900:5200]),
        (gz.stored(b""), b""),
        (gz.member(gz.rand(3000, seed=2), 6), gz.rand(3000, seed=2)),
        (gz.fixed(b""), b""),
    ]
    return b"".join(m for m, _ in parts), b"".join(p for _, p in parts)


def interleaved_file():
    """One 300 000-byte level-6 member between runs of tiny ones -> (file, plain)."""
    a, pa = gz.tiny_members(9, seed=4)
    b, pb = gz.tiny_members(7, seed=6)
    big = gz.text(300000, seed=21)
    return a + gz.member(big, 6) + b, pa + big + pb


def padded_front(total, seed):
    """A member of exactly `total` bytes that ends with a stored block: a dynamic part and random stored bytes."""
    t = gz.text(1200, seed=seed)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    head = c.compress(t) + c.flush(zlib.Z_FULL_FLUSH)  # (ends byte aligned, with an empty stored block)
    pad = total - 10 - len(head) - 5 - 8
    assert 0 <= pad < 65536
    fill = gz.rand(pad, seed=seed + 1)
    raw = head + b"\x01" + struct.pack("<HH", pad, pad ^ 0xffff) + fill
    m = wrap(raw, t + fill)
    assert len(m) == total
    return m, t + fill


def tile_edge_files():
    """[(what, file, plain)]: a member boundary, a trailer and a header across a 4096-byte tile edge and across the
    16-byte halo (file offsets; the test moves the buffer's address by 0, 1 and 15)."""
    long_hdr = dict(flg=gz.FEXTRA | gz.FNAME, extra=b"ab\x14\x00" + b"\x1f" * 20, name=b"n" * 30)
    second = gz.text(2500, seed=77)
    out = []
    for start in (4096, 4100, 4092, 4112, 4104, 4090, 8192 - 30):
        m, p = padded_front(start, seed=start)
        for hdr in ({}, long_hdr):
            out.append(("the second member at %d%s" % (start, ", a 66-byte header" if hdr else ""),
                        m + gz.member(second, 6, **hdr) + gz.fixed(b"end"), p + second + b"end"))
    return out


def history_files():
    """The legal and the illegal stream of one_ref.history_pair() as the SECOND member behind a 40 000-byte member ->
    (legal file, its plain, illegal file, member 0, its plain, the illegal raw stream)."""
    legal, plain, illegal = one_ref.history_pair()
    p0 = gz.text(40000, seed=12)
    m0 = gz.member(p0, 6)
    return m0 + wrap(legal, plain), p0 + plain, m0 + wrap(illegal, plain), m0, p0, illegal


def decoy_files():
    """[(what, file, plain)]: candidates that are off the path."""
    t = gz.text(6000, seed=11)
    inner = gz.member(t[:3000], 6) + gz.member(t[3000:], 9, flg=gz.FNAME, name=b"inner")
    pay = b"junk" + inner + b"more junk"
    name = b"x" + gz.MAGIC + b"\x01aaaa\x02\x03" + b"y" * 20
    out = [("a two-member file inside a stored block", gz.member(t[:500], 1) + gz.stored(pay) + gz.member(t[:700], 6),
            t[:500] + pay + t[:700]),
           ("a gzip header inside an FNAME", gz.member(t[:800], 6, flg=gz.FNAME, name=name) + gz.member(t[:500], 1),
            t[:800] + t[:500])]
    streams = one_ref.decoy_streams()
    out.append(("streams inside stored blocks as members", b"".join(wrap(r, p) for _, r, p in streams),
                b"".join(p for _, _, p in streams)))
    return out


def three_members():
    """Three members, the middle one of several units -> [(member, plain)]."""
    t = gz.text(30000, seed=31)
    mid = t[3000:21000]
    return [(gz.member(t[:3000], 6, flg=gz.FNAME, name=b"first"), t[:3000]), (wrap(one_ref.deflate(mid, 6, mem=1), mid), mid),
            (gz.member(t[21000:], 9), t[21000:])]
