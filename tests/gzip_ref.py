"""Plain multi-member gzip files on the CPU: the reference of flate_hip_gzip_index / flate_hip_gzip_read.

Truth about a file's CONTENT comes from zlib: `plain_of` walks zlib.decompressobj(31) over unused_data, as gzip -d does.
The INDEX is the walk of include/flate_hip.h restated here (`Walk`): the header rule at p over in[p, min(n, p + M)), a
size-only decode of the raw stream in front of the range's last 8 bytes (zlib.decompressobj(-15): it reports the end of
the final block through unused_data, to the byte, and does not look at the trailer -- a wrong CRC is a member's failure,
not the chain's), the link to p + header + used + 8.  The file also builds the corpus every gzip test shares."""
import gzip
import struct
import zlib

import numpy as np

OUT_TOO_SMALL, CORRUPT, TOO_LARGE, UNEXPECTED_EOF = -2, -4, -6, -7
MEMBER_MAX = (1 << 28) - 1
MAGIC = b"\x1f\x8b\x08"
FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


# ---- the rule and the walk ----

def header_len(buf, p, end):
    """gzip_header_len over buf[p:end]: the header's length, or 0 -- no member can start at p."""
    n = end - p
    if n < 10 or buf[p:p + 3] != MAGIC or buf[p + 3] & 0xe0:
        return 0
    flg, q = buf[p + 3], 10
    if flg & FEXTRA:
        if n < q + 2:
            return 0
        q += 2 + (buf[p + q] | (buf[p + q + 1] << 8))
    for bit in (FNAME, FCOMMENT):
        if flg & bit:
            z = buf.find(b"\0", p + q, end) if q < n else -1
            if z < 0:
                return 0
            q = z - p + 1
    if flg & FHCRC:
        q += 2
    return q if n >= q + 8 else 0


def range_end(p, n, member_max=MEMBER_MAX):
    return min(n, p + member_max)


def size_only(buf, a, b):
    """The raw stream buf[a:b] decoded for its size -> (status, used, size)."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(buf[a:b])
    except zlib.error:
        return CORRUPT, 0, 0
    if not d.eof:
        return UNEXPECTED_EOF, 0, 0
    return 0, (b - a) - len(d.unused_data), len(out)


def candidates(buf, member_max=MEMBER_MAX):
    """[(offset, status, used, size)] of every offset that passes the rule, in file order."""
    buf, out, p = bytes(buf), [], -1
    while True:
        p = buf.find(MAGIC, p + 1)
        if p < 0:
            return out
        e = range_end(p, len(buf), member_max)
        hl = header_len(buf, p, e)
        if hl:
            out.append((p,) + size_only(buf, p + hl, e - 8))


def dead_code(s, p, n, member_max):
    if s == OUT_TOO_SMALL or (s == UNEXPECTED_EOF and p + member_max < n):
        return TOO_LARGE
    return s


class Walk:
    """The serial walk from offset 0: rc, n_members, err_off (-1: none), member_off / out_off (n_members + 1 entries,
    of a broken chain its good prefix), out_bytes (0 unless rc == 0), n_candidates, table (candidates)."""

    def __init__(self, buf, member_max=MEMBER_MAX):
        buf = bytes(buf)
        n = len(buf)
        self.table = candidates(buf, member_max)
        self.n_candidates = len(self.table)
        at = {c[0]: c for c in self.table}
        self.rc, self.err_off, self.member_off, self.out_off = 0, -1, [], []
        p, total = 0, 0
        while p < n:
            c = at.get(p)
            if c is None:
                self.rc = CORRUPT
                break
            if c[1]:
                self.rc = dead_code(c[1], p, n, member_max)
                break
            self.member_off.append(p)
            self.out_off.append(total)
            total += c[3]
            p += header_len(buf, p, range_end(p, n, member_max)) + c[2] + 8
        if self.rc:
            self.err_off = p
        self.n_members = len(self.member_off)
        self.member_off.append(p)
        self.out_off.append(total)
        self.out_bytes = 0 if self.rc else total

    def members(self, buf):
        return [bytes(buf[self.member_off[i]:self.member_off[i + 1]]) for i in range(self.n_members)]


def plain_of(f):
    """What gzip -d makes of the file: zlib's own gzip reader walked over unused_data (raises zlib.error)."""
    out, rest = [], bytes(f)
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        if not d.eof:
            raise zlib.error("the last member is cut short")
        rest = d.unused_data
    return b"".join(out)


# ---- members ----

def text(n, seed=9):
    """n bytes of word soup: compresses like prose, with matches and a skewed alphabet."""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(2, 10, 300)]
    out, size = [], 0
    for i in rng.zipf(1.3, n // 3 + 8):
        w = words[int(i) % len(words)] + b" "
        out.append(w)
        size += len(w)
        if size >= n:
            break
    return b"".join(out)[:n].ljust(n, b".")


def rand(n, seed=5):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def header(flg=0, extra=b"", name=b"", comment=b"", mtime=0, xfl=0, os_=255):
    h = MAGIC + bytes([flg]) + struct.pack("<I", mtime) + bytes([xfl, os_])
    if flg & FEXTRA:
        h += struct.pack("<H", len(extra)) + extra
    if flg & FNAME:
        h += name + b"\0"
    if flg & FCOMMENT:
        h += comment + b"\0"
    if flg & FHCRC:
        h += struct.pack("<H", zlib.crc32(h) & 0xffff)
    return h


def member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **hdr):
    return header(**hdr) + raw(data, level, strategy) + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def stored(data, **hdr):
    return member(data, 0, **hdr)


def fixed(data, **hdr):
    return member(data, 9, zlib.Z_FIXED, **hdr)


def own_member(raw_stream, data):
    """A member as flate_hip_deflate_fast_batch_framed(FLATE_HIP_WRAP_GZIP) writes it, around a raw stream."""
    return header(xfl=4) + bytes(raw_stream) + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


# ---- the corpus: [(what, file, plain)] ----

MEMBER_COUNTS = [1, 2, 3, 257, 1025]


def tiny_members(n, seed=3):
    """n members of 0 .. 40 bytes each: empty ones (stored and fixed), stored and fixed ones, at every offset mod 16."""
    rng = np.random.default_rng(seed)
    parts, plain = [], []
    for k in range(n):
        p = b"" if k % 4 == 1 else bytes(rng.integers(32, 127, (k * 7) % 41, dtype=np.uint8))
        parts.append(stored(p) if k % 3 == 0 else fixed(p))
        plain.append(p)
    return b"".join(parts), b"".join(plain)


def straddle_file(start, long_header=False):
    """Two members, the second one at offset `start` -- with a header of 10 bytes, or one longer than a tile's halo."""
    a = rand(start - 23, seed=start)
    f = stored(a)
    assert len(f) == start
    b = text(700, seed=start)
    hdr = dict(flg=FEXTRA | FNAME | FHCRC, extra=b"ab\x3c\x00" + b"\x1f" * 60, name=b"n" * 40) if long_header else {}
    return f + member(b, 6, **hdr), a + b


def good_files():
    t = text(120000)
    out = []
    for n in MEMBER_COUNTS:
        out.append(("%d tiny members" % n,) + tiny_members(n))
    out.append(("empty members", stored(b"") + fixed(b"") + member(b"") + stored(b""), b""))
    out.append(("stored only", stored(t[:20000]) + stored(rand(70000)), t[:20000] + rand(70000)))
    out.append(("fixed blocks", fixed(t[:9000]) + fixed(t[9000:9100]), t[:9100]))
    out.append(("dynamic blocks", member(t, 9) + member(t[:50000], 1), t + t[:50000]))
    out.append(("python gzip levels 1 6 9", b"".join(gzip.compress(t[k * 30000:(k + 1) * 30000], lv, mtime=1234567 + k)
                                                     for k, lv in enumerate((1, 6, 9))), t[:90000]))
    combos, plain = [], []
    for k in range(16):  # every FEXTRA / FNAME / FCOMMENT / FHCRC combination, FTEXT on every other one
        flg = (k << 1) | (k & 1)
        p = t[k * 100:k * 100 + 37 * k]
        combos.append(member(p, 6, flg=flg, extra=b"ab\x03\x00xyz" * (k % 3), name=b"file-%d.txt" % k,
                             comment=b"c" * k, mtime=k))
        plain.append(p)
    out.append(("every header combination", b"".join(combos), b"".join(plain)))
    for start in (4093, 4094, 4095, 4096, 4097):
        out.append(("magic at %d" % start,) + straddle_file(start))
    for start in (4000, 4090):  # the 120-byte header itself lies across the tile's edge
        out.append(("a long header from %d on" % start,) + straddle_file(start, True))
    return out


def decoy_files():
    """[(what, file, plain, more_candidates)]: bytes that pass the rule without being on the path from offset 0."""
    t = text(6000, seed=11)
    inner_a, inner_b = member(t[:3000], 6), member(t[3000:], 9, flg=FNAME, name=b"inner")
    tail = member(t[:500], 1)
    out = []
    # a complete member, gzipped again at level 0: it lies verbatim in a stored block, decodes cleanly and its successor
    # (the second inner member) is a candidate too
    pay = b"junk" + inner_a + inner_b + b"more junk"
    assert len(pay) < 60000
    out.append(("members inside a stored block", stored(pay) + tail, pay + t[:500], True))
    # a decoy whose own chain reaches in_len: the outer member's trailer serves as the inner one's
    pay = b"front" + inner_a[:-8]
    out.append(("a decoy chain that reaches the end", tail + stored(pay), t[:500] + pay, True))
    # decoy headers inside a true header's FNAME (no NUL: FLG = FTEXT, a non-zero MTIME) and FEXTRA (a plain header)
    name = b"x" + MAGIC + b"\x01aaaa\x02\x03" + b"y" * 20
    extra = b"zz\x20\x00" + header() + raw(b"decoy", 6) + b"\0" * 8
    extra = extra[:4] + extra[4:].ljust(0x20, b"\0")
    out.append(("decoys in FNAME and FEXTRA", member(t[:800], 6, flg=FNAME | FEXTRA, name=name, extra=extra) + tail,
                t[:800] + t[:500], True))
    # in the last 18 bytes: a header with an empty stream in front of the file's last 8 bytes (a candidate that meets
    # the end of its stream at once); in the last 17: one byte short of being a candidate at all
    pay = t[:300]
    out.append(("a decoy in the last 18 bytes", tail + stored(pay + header()), t[:500] + pay + header(), True))
    out.append(("a decoy in the last 17 bytes", tail + stored(pay + header()[:9]), t[:500] + pay + header()[:9], False))
    return out


def malformed_files():
    """[(what, file, member_max, rc, err_off, n_members)]: the verdict every index and read must give."""
    t = text(9000, seed=21)
    m = [member(t[:3000], 6, flg=FNAME, name=b"first"), member(t[3000:6000], 9), stored(t[6000:])]
    a, ab, abc = len(m[0]), len(m[0]) + len(m[1]), len(b"".join(m))
    bad_mid = bytearray(b"".join(m))
    bad_mid[a + 10] = 0x07  # the middle stream starts with a block of the reserved type
    big = stored(rand(5000 - 23, seed=4))
    assert len(big) == 5000
    return [
        ("garbage after the last member", b"".join(m) + b"garbage!!", MEMBER_MAX, CORRUPT, abc, 3),
        ("three bytes of garbage", b"".join(m) + b"\x1f\x8b\x08", MEMBER_MAX, CORRUPT, abc, 3),
        ("zero padding", b"".join(m) + b"\0" * 512, MEMBER_MAX, CORRUPT, abc, 3),
        ("one zero byte", b"".join(m) + b"\0", MEMBER_MAX, CORRUPT, abc, 3),
        ("cut inside a header", m[0] + m[1][:7], MEMBER_MAX, CORRUPT, a, 1),
        ("cut inside a file name", m[1] + m[0][:13] + b"nameless" * 3, MEMBER_MAX, CORRUPT, len(m[1]), 1),
        ("cut inside a stream", m[0] + m[1] + m[2][:2000], MEMBER_MAX, UNEXPECTED_EOF, ab, 2),
        ("cut inside a trailer", m[0] + m[1][:-3], MEMBER_MAX, UNEXPECTED_EOF, a, 1),
        ("a corrupt middle stream", bytes(bad_mid), MEMBER_MAX, CORRUPT, a, 1),
        ("17 bytes", header() + b"\x03\x00" + b"\0" * 5, MEMBER_MAX, CORRUPT, 0, 0),
        ("no gzip file", b"PK\x03\x04" + t[:100], MEMBER_MAX, CORRUPT, 0, 0),
        ("a 5000-byte member under gzip_member_max 4096", m[1] + big + m[0], 4096, TOO_LARGE, len(m[1]), 1),
        ("a 5000-byte member at the end under gzip_member_max 4096", m[1] + big, 4096, TOO_LARGE, len(m[1]), 1),
    ]


def failing_files():
    """[(what, file, rc, bad_member)]: a sound chain with a member that fails at read time."""
    t = text(9000, seed=31)
    m = [member(t[:3000], 6), member(t[3000:6000], 9), fixed(t[6000:6500])]
    crc = bytearray(m[1])
    crc[-8] ^= 0x40
    isize = bytearray(m[1])
    isize[-4] ^= 0x01
    return [("a wrong CRC in the middle member", m[0] + bytes(crc) + m[2], CORRUPT, 1),
            ("a wrong ISIZE in the middle member", m[0] + bytes(isize) + m[2], CORRUPT, 1)]
