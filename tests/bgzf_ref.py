"""CPU reference for BGZF files (flate_hip_bgzf_write / _index / _read), shared by tests/test_bgzf_abi.py,
tests/test_bgzf_index_model.py, tests/test_gpu_bgzf.py and tests/test_host_cpp_bgzf.py: a member builder around the
oracle's raw streams, the serial walk in Python -- THE SPECIFICATION of member discovery -- and the file corpus
(hand-built headers, decoys inside stored blocks, malformed chains, members that fail).  Nothing here needs a GPU."""
import struct
import zlib

import numpy as np

from util import make_streams

HEAD16 = bytes.fromhex("1f8b08040000000000ff060042430200")  # htslib's; BSIZE follows
EOF = HEAD16 + bytes.fromhex("1b00") + b"\x03\x00" + b"\0" * 8
BLOCK_DEFAULT = 65280
MEMBER_MAX = 65536
OK, OUT_TOO_SMALL, CORRUPT, TOO_LARGE, UNEXPECTED_EOF = 0, -2, -4, -6, -7


# ---- building members ----

def wrap_raw(raw, block, before=b"", after=b"", isize=None, crc=None, flg=4):
    """One member around the raw stream `raw` of `block`: the fixed gzip header, an extra field of `before` | the 'BC'
    subfield | `after` (whole subfields each), the stream, CRC-32 and ISIZE."""
    xlen = len(before) + 6 + len(after)
    total = 12 + xlen + len(raw) + 8
    assert total <= MEMBER_MAX, total
    extra = before + b"BC\x02\x00" + struct.pack("<H", total - 1) + after
    head = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", xlen) + extra
    return head + raw + struct.pack("<II", zlib.crc32(block) if crc is None else crc,
                                    len(block) if isize is None else isize)


def member(oracle, block, compat=0):
    """The member flate_hip_bgzf_write writes for `block`: the 18-byte header, oracle.deflate(block), the trailer."""
    m = wrap_raw(oracle.deflate(np.frombuffer(bytes(block), np.uint8), compat=compat), bytes(block))
    assert m[:16] == HEAD16
    return m


def stored_raw(payload):
    """A raw stream of one final stored block: its bytes can be chosen."""
    assert len(payload) <= 65535
    return b"\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xffff) + payload


def stored_member(payload, **kw):
    return wrap_raw(stored_raw(payload), payload, **kw)


def zlib_member(block, level=6, **kw):
    """A foreign writer: zlib's fixed and dynamic blocks inside the same member."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return wrap_raw(co.compress(block) + co.flush(), block, **kw)


def blocks_of(data, block_bytes=0):
    bb = block_bytes or BLOCK_DEFAULT
    return [data[i:i + bb] for i in range(0, len(data), bb)]


def build_file(oracle, data, block_bytes=0, compat=0):
    """(file, member_off) as flate_hip_bgzf_write defines them."""
    members = [member(oracle, b, compat) for b in blocks_of(bytes(data), block_bytes)]
    off = np.zeros(len(members) + 1, np.uint64)
    np.cumsum(np.array([len(m) for m in members], np.uint64), out=off[1:])
    return b"".join(members) + EOF, off


# ---- the serial walk: the specification ----

def member_total(buf, p):
    """The size of the member at offset p of buf, or 0: no member can be read there (flate_hip.h, "BGZF files")."""
    avail = len(buf) - p
    if avail < 26 or buf[p:p + 3] != b"\x1f\x8b\x08" or not buf[p + 3] & 4 or buf[p + 3] & 0xe0:
        return 0
    xlen = buf[p + 10] | buf[p + 11] << 8
    if xlen < 6 or avail < 12 + xlen + 8:
        return 0
    x, q, total = buf[p + 12:p + 12 + xlen], 0, 0
    while q < xlen:
        if q + 4 > xlen:
            return 0
        slen = x[q + 2] | x[q + 3] << 8
        if q + 4 + slen > xlen:
            return 0
        if not total and x[q:q + 2] == b"BC" and slen == 2:
            total = (x[q + 4] | x[q + 5] << 8) + 1
        q += 4 + slen
    return total if total and 12 + xlen + 8 <= total <= avail else 0


class Walk:
    """rc, n_members, err_off, member_off[n + 1], out_off[n + 1], out_bytes, eof_marker of the walk from offset 0."""

    def __init__(self, buf):
        buf = bytes(buf)
        p, self.member_off, self.out_off = 0, [], [0]
        self.rc, self.err_off, self.eof_marker = OK, -1, 0
        while p < len(buf):
            t = member_total(buf, p)
            if not t:
                self.rc, self.err_off = CORRUPT, p
                break
            self.member_off.append(p)
            self.out_off.append(self.out_off[-1] + struct.unpack_from("<I", buf, p + t - 4)[0])
            self.eof_marker = int(buf[p:p + t] == EOF)
            p += t
        self.n_members = len(self.member_off)
        self.member_off.append(len(buf))
        self.out_bytes = self.out_off[-1]
        if self.rc:
            self.out_bytes, self.eof_marker, self.member_off, self.out_off = 0, 0, None, None

    def members(self, buf):
        return [bytes(buf[self.member_off[i]:self.member_off[i + 1]]) for i in range(self.n_members)]


# ---- the corpus ----

WRITE_LENGTHS = [0, 1, 16, 17, 127, 128, 65279, 65280, 65281, 2 * 65280, 3 * 65280 + 5]
FILLS = ["text", "rand", "zero", "ramp", "low", "period", "runs"]  # (framed_read_ref.FILLS)


def write_inputs():
    """{in_len: bytes}: one input per length of WRITE_LENGTHS, every 65280-byte block of it with another fill."""
    out, k = {}, 0
    for n in WRITE_LENGTHS:
        specs = []
        for b in range(0, n, BLOCK_DEFAULT):
            specs.append((FILLS[k % len(FILLS)], min(BLOCK_DEFAULT, n - b)))
            k += 1
        data, _ = make_streams(specs, seed=500 + n % 977) if specs else (np.zeros(0, np.uint8), None)
        out[n] = data[:n].tobytes()
    return out


def text(n, seed=9):
    return make_streams([("text", n)], seed=seed)[0][:n].tobytes()


FULL_PAYLOAD = MEMBER_MAX - 18 - 5 - 8  # a stored member of exactly 65536 bytes


def many_members(n, seed=3):
    """A file of n members: runs of adjacent 28-byte empty members (several share one cache line), stored members of
    31 + j bytes that move the following starts to every offset mod 64, and -- every 97th -- a full 65536-byte member;
    the last one is the EOF marker.  Returns (file, the payloads' concatenation)."""
    rng = np.random.default_rng(seed)
    parts, plain = [], []
    for k in range(n - 1):
        if k % 97 == 5:
            p = rng.integers(0, 256, FULL_PAYLOAD, dtype=np.uint8).tobytes()
        elif k % 5 == 4 or n <= 3:
            p = rng.integers(0, 256, (k * 7) % 41, dtype=np.uint8).tobytes()
        else:
            parts.append(EOF)
            continue
        m = stored_member(p)
        assert len(m) == 31 + len(p)
        parts.append(m)
        plain.append(p)
    parts.append(EOF)
    return b"".join(parts), b"".join(plain)


MEMBER_COUNTS = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025]


def decoy_header(total, xlen_pad=0):
    """The bytes of a complete, valid member header that claims `total` bytes: planted inside a stored block."""
    pad = b"" if not xlen_pad else b"zz" + struct.pack("<H", xlen_pad - 4) + b"\0" * (xlen_pad - 4)
    return bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", 6 + len(pad)) + b"BC\x02\x00" + \
        struct.pack("<H", total - 1) + pad


def decoy_files():
    """[(what, file)]: chosen bytes inside stored blocks that pass the member rule.  The walk from 0 never starts at
    them; every case must come out as the walk says."""
    t = text(3000)
    b_mem, c_mem = zlib_member(t[:1200]), zlib_member(t[1200:])
    cases = []

    def file_with(payload_of, what, check):
        # A = a stored member whose payload holds the decoy; payload_of(a_off, a_len, rest_len) -> payload
        a_len = 31 + 600
        rest = b_mem + c_mem + EOF
        payload = payload_of(a_len, len(rest))
        assert len(payload) == 600
        f = stored_member(payload) + rest
        assert len(f) == a_len + len(rest)
        check(f, a_len)
        cases.append((what, f))

    at = 18 + 5 + 100  # where the decoy starts in the file

    def fill(decoy, where=at):
        p = bytearray(np.random.default_rng(8).integers(0, 31, 600, dtype=np.uint8).tobytes())  # (no 0x1f 0x8b by chance)
        p[where - 23:where - 23 + len(decoy)] = decoy
        return bytes(p)

    def merges(f, a_len):
        assert member_total(f, at) == a_len + len(b_mem) - at  # the decoy's successor is C: a true member start
    file_with(lambda a_len, rest: fill(decoy_header(a_len + len(b_mem) - at)), "a side chain that merges into the true one", merges)

    def to_end(f, a_len):
        assert at + member_total(f, at) == len(f)
    file_with(lambda a_len, rest: fill(decoy_header(a_len + rest - at)), "a decoy chain that reaches in_len on its own", to_end)

    def past(f, a_len):
        assert member_total(f, at) == 0 and f[at:at + 3] == b"\x1f\x8b\x08"
    file_with(lambda a_len, rest: fill(decoy_header(a_len + rest - at + 1)), "a decoy pointing past in_len", past)

    last = 18 + 5 + 600 - 18  # the decoy's 18 bytes end the payload: A's trailer, then the true header
    def in_front(f, a_len):
        assert member_total(f, last) == 26 and last + 26 == a_len
    file_with(lambda a_len, rest: fill(decoy_header(26), last), "a decoy immediately in front of a true header", in_front)

    # the decoy's extra field runs over A's trailer and B's first bytes: 22 bytes end the payload, then a padding
    # subfield of 8 + 20 bytes
    over = 18 + 5 + 600 - 22
    def overlaps(f, a_len):
        assert member_total(f, over) == 200 and over + 12 + 6 + 4 > a_len - 8 - 1 and over + 12 + 38 > a_len + 18
    def overlap_payload(a_len, rest):
        d = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", 6 + 4 + 28) + b"BC\x02\x00" + \
            struct.pack("<H", 199) + b"zz" + struct.pack("<H", 28)
        return fill(d, over)
    file_with(overlap_payload, "a decoy overlapping a true header", overlaps)
    for what, f in cases:
        assert Walk(f).rc == OK and Walk(f).n_members == 4, what
    return cases


def header_files():
    """[(what, file)]: well-formed chains with other headers than ours."""
    t = text(5000, seed=4)
    other = b"XY\x03\x00abc"                      # another subfield in front of 'BC'
    pad = b"pd\x05\x00\0\0\0\0\0" + b"q\0\0\0"    # ... and two behind it, the second empty
    return [
        ("another subfield in front of BC", zlib_member(t[:2000], before=other) + EOF),
        ("XLEN > 6 and padding subfields behind BC", zlib_member(t[:2000], after=pad) + zlib_member(t[2000:], after=pad) + EOF),
        ("both, and FNAME-less flags MTIME/XFL ignored", zlib_member(t[:100], before=other, after=pad) + stored_member(b"") + EOF),
        ("a BC subfield of another length first", zlib_member(t[:300], before=b"BC\x01\x00\x07") + EOF),
        ("no EOF marker", zlib_member(t[:2000]) + zlib_member(t[2000:])),
        ("the EOF marker alone", EOF),
        ("a foreign writer: fixed and dynamic blocks", b"".join(zlib_member(t[i:i + n]) for i, n in ((0, 40), (40, 3000), (3040, 9), (3049, 1951))) + EOF),
    ]


def malformed_files():
    """[(what, file, err_off, n_members)]: chains the walk cannot finish."""
    t = text(4000, seed=5)
    a, b = zlib_member(t[:1500]), zlib_member(t[1500:])
    good = a + b + EOF
    la, lab = len(a), len(a) + len(b)

    def retotal(m, total):
        return m[:16] + struct.pack("<H", total - 1) + m[18:]
    return [
        ("cut inside a header", good[:la + 7], la, 1),
        ("cut inside a payload", good[:la + 200], la, 1),
        ("cut inside a trailer", good[:lab - 3], la, 1),
        ("cut inside the marker", good[:lab + 27], lab, 2),
        ("BSIZE too small for header plus trailer", a + retotal(b, 25) + EOF, la, 1),
        ("FEXTRA without a BC subfield", a + b[:12] + b"BD" + b[14:] + EOF, la, 1),
        ("a subfield running past XLEN", a + b[:14] + b"\x03\x00" + b[16:] + EOF, la, 1),
        ("a subfield header cut by XLEN", zlib_member(t[:50], after=b"q\0\0") + EOF, 0, 0),
        ("FEXTRA flag clear", a + b[:3] + b"\0" + b[4:] + EOF, la, 1),
        ("a reserved flag bit", a + b[:3] + b"\x24" + b[4:] + EOF, la, 1),
        ("5 bytes of garbage after the last member", good + b"\x1f\x8b\x08\x04\x00", len(good), 3),
        ("garbage in front of the first", b"\x00" + good, 0, 0),
        ("XLEN below 6", a + b[:10] + b"\x05\x00" + b[12:] + EOF, la, 1),
    ]


def failing_files():
    """[(what, file, rc, bad_member)]: chains that are fine, members that are not; all other members are delivered."""
    t = text(6000, seed=6)
    blocks = [t[:2000], t[2000:4500], t[4500:]]
    m = [zlib_member(b) for b in blocks]

    def flip(x, at):
        y = bytearray(x)
        y[at] ^= 0x10
        return bytes(y)
    raw1 = m[1][18:-8]
    cut = wrap_raw(raw1[:-9], blocks[1])  # the raw stream cut short, BSIZE lowered with it
    return [
        ("a flipped CRC", m[0] + flip(m[1], len(m[1]) - 6) + m[2] + EOF, CORRUPT, 1),
        ("ISIZE one too large", m[0] + m[1] + zlib_member(blocks[2], isize=len(blocks[2]) + 1) + EOF, CORRUPT, 2),
        ("ISIZE one too small", zlib_member(blocks[0], isize=len(blocks[0]) - 1) + m[1] + m[2] + EOF, OUT_TOO_SMALL, 0),
        ("a raw stream cut short", m[0] + cut + m[2] + EOF, UNEXPECTED_EOF, 1),
        ("two failures: the first is reported", m[0] + cut + flip(m[2], len(m[2]) - 6) + EOF, UNEXPECTED_EOF, 1),
    ]


def index_corpus():
    """[(what, file)]: every file above whose header bytes the member rule has to judge (without the large ones)."""
    out = header_files() + decoy_files() + [(w, f) for w, f, _, _ in malformed_files()] + \
        [(w, f) for w, f, _, _ in failing_files()]
    out += [("%d members" % n, many_members(n)[0]) for n in (1, 2, 3, 65)]
    out.append(("an empty file", b""))
    return out
