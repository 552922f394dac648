"""CPU reference for BGZF files read and written in PARTS (flate_hip_bgzf_reader_* / flate_hip_bgzf_writer_*), shared by
tests/test_bgzf_parts_ref.py, tests/test_bgzf_parts_rule_model.py, tests/test_gpu_bgzf_parts.py and
tests/test_gpu_host_bgzf_parts.py.  ReaderModel is built on bgzf_ref's serial walk and member rule and on zlib for the
members' bytes and verdicts; WriterModel on bgzf_ref.build_file.  Nothing here needs a GPU."""
import collections
import struct
import zlib

import numpy as np

import bgzf_ref as ref

OK, STREAM_END, INVALID, OUT_TOO_SMALL, CORRUPT, TOO_LARGE, UNEXPECTED_EOF = 0, 1, -1, -2, -4, -6, -7
NONE = 0xffffffff
UNBOUNDED = 1 << 62
BOUNDARY, STOP, DEAD = 0, 1, 2

# one call's words, the index of the delivered members in FILE coordinates (None without arrays) and the bytes
Read = collections.namedtuple("Read", "rc in_used out_len n_members bad_member err_off eof_marker member_off out_off data")
Write = collections.namedtuple("Write", "rc in_used out_len n_blocks member_off data")


def part_stop(avail, final):
    """THE PART STOP at the offset where the walk over a part finds no member; avail: the bytes behind it."""
    if avail == 0:
        return BOUNDARY
    return DEAD if final or avail >= ref.MEMBER_MAX else STOP


def member_verdict(m):
    """(status, bytes) of the member m as flate_hip_inflate_batch_framed judges it in a slot of ISIZE bytes: 0 with the
    bytes, or UNEXPECTED_EOF (the raw stream ends early), CORRUPT (a bad stream, CRC-32 or ISIZE), OUT_TOO_SMALL (it
    produces more than ISIZE)."""
    xlen = m[10] | m[11] << 8
    raw, (crc, isize) = m[12 + xlen:len(m) - 8], struct.unpack_from("<II", m, len(m) - 8)
    d = zlib.decompressobj(-15)
    try:
        plain = d.decompress(raw)
    except zlib.error:
        return CORRUPT, b""
    if not d.eof:
        return UNEXPECTED_EOF, b""
    if len(plain) > isize:
        return OUT_TOO_SMALL, b""
    if d.unused_data or len(plain) != isize or zlib.crc32(plain) != crc:
        return CORRUPT, b""
    return OK, plain


class ReaderModel:
    """The reader over `file`: read(part, final, out_cap, index_cap) -> Read.  `part` is file[consumed:][:len(part)],
    as the convention "begins with the unused bytes" makes it; index_cap None: no index arrays."""

    def __init__(self, file):
        self.file = bytes(file)
        self.consumed = self.produced = self.members = self.eof_marker = 0
        self.sticky = None
        self._verdicts = {}

    def _verdict(self, off, m):
        if off not in self._verdicts:
            self._verdicts[off] = member_verdict(m)
        return self._verdicts[off]

    def _nothing(self, rc, with_index, bad=NONE, err_off=-1, out_len=0):
        idx = ([self.consumed], [self.produced]) if with_index else (None, None)
        return Read(rc, 0, out_len, 0, bad, err_off, self.eof_marker, idx[0], idx[1], b"")

    def read(self, part, final, out_cap=UNBOUNDED, index_cap=None):
        part = bytes(part)
        assert part == self.file[self.consumed:self.consumed + len(part)], "the part does not begin with the unused bytes"
        with_index = index_cap is not None
        if with_index and index_cap == 0:
            return Read(INVALID, 0, 0, 0, NONE, -1, 0, None, None, b"")
        if self.sticky is not None:
            rc, bad, eo = self.sticky
            return self._nothing(rc, with_index, bad, eo)
        if not part:
            if not final:
                return self._nothing(OK, with_index)
            self.sticky = (STREAM_END, NONE, -1)
            return self._nothing(STREAM_END, with_index)
        # the serial walk over the part
        p, moff, ooff = 0, [], [0]
        while p < len(part):
            t = ref.member_total(part, p)
            if not t:
                break
            moff.append(p)
            ooff.append(ooff[-1] + struct.unpack_from("<I", part, p + t - 4)[0])
            p += t
        moff.append(p)
        n, stop = len(moff) - 1, part_stop(len(part) - p, final)
        # delivery: the longest prefix that fits both rooms
        k = 0
        while k < n and ooff[k + 1] <= out_cap and (not with_index or k + 2 <= index_cap):
            k += 1
        if k == 0 and n >= 1:
            return self._nothing(OUT_TOO_SMALL, with_index, out_len=ooff[1])
        data, fail = [], None
        for j in range(k):
            st, plain = self._verdict(self.consumed + moff[j], part[moff[j]:moff[j + 1]])
            if st:
                fail = (st, self.members + j, self.consumed + moff[j])
                k = j
                break
            data.append(plain)
        if fail is None and k == n and stop == DEAD:
            fail = (CORRUPT, self.members + n, self.consumed + p)
        idx = ([self.consumed + x for x in moff[:k + 1]], [self.produced + x for x in ooff[:k + 1]]) if with_index else (None, None)
        if k:
            self.eof_marker = int(part[moff[k - 1]:moff[k]] == ref.EOF)
        self.members += k
        self.produced += ooff[k]
        if fail is not None:
            self.sticky = fail
            return Read(fail[0], 0, ooff[k], k, fail[1], fail[2], self.eof_marker, idx[0], idx[1], b"".join(data))
        self.consumed += moff[k]
        rc = OK
        if final and k == n and moff[k] == len(part):
            rc, self.sticky = STREAM_END, (STREAM_END, NONE, -1)
        return Read(rc, moff[k], ooff[k], k, NONE, -1, self.eof_marker, idx[0], idx[1], b"".join(data))


def writer_blocks(in_len, bb, final):
    """The blocks a write compresses, and the bytes it uses."""
    return (-(-in_len // bb), in_len) if final else (in_len // bb, in_len // bb * bb)


class WriterModel:
    """The writer over `data`: write(part, final) -> Write.  `part` is data[used so far:][:len(part)]."""

    def __init__(self, oracle, data, block_bytes=0, compat=0):
        self.data, self.bb = bytes(data), block_bytes or ref.BLOCK_DEFAULT
        self.file, off = ref.build_file(oracle, self.data, block_bytes, compat)
        self.off = [int(x) for x in off]
        self.used = self.block = 0
        self.ended = False

    def write(self, part, final):
        part = bytes(part)
        if self.ended:
            return Write(INVALID, 0, 0, 0, None, b"")
        assert part == self.data[self.used:self.used + len(part)], "the part does not begin with the unused bytes"
        k, used = writer_blocks(len(part), self.bb, final)
        assert not final or self.used + used == len(self.data), "a final part that is not the input's end"
        a, b = self.off[self.block], self.off[self.block + k]
        data = self.file[a:b] + (ref.EOF if final else b"")
        moff = self.off[self.block:self.block + k + 1]
        self.used, self.block, self.ended = self.used + used, self.block + k, bool(final)
        return Write(STREAM_END if final else OK, used, len(data), k, moff, data)


def feed(read, f, sizes, max_calls, grow=1):
    """The feeding loop every test uses, with its hard cap on calls.  read(part bytes, final) -> a Read or a Write;
    sizes: an iterator of how many NEW bytes each call appends (exhausted: everything left); a call that used nothing is
    followed by `grow` more bytes.  -> ([calls], the bytes, the unused rest)."""
    sizes = iter(sizes)
    f = bytes(f)
    pos, buf, calls, out = 0, b"", [], []
    add = next(sizes, len(f))
    while True:
        assert len(calls) < max_calls, "no progress: %d calls" % len(calls)
        pos, buf = pos + len(f[pos:pos + add]), buf + f[pos:pos + add]
        final = pos >= len(f)
        c = read(buf, final)
        calls.append(c)
        out.append(bytes(c.data))
        buf = buf[c.in_used:]
        if c.rc != OK:
            return calls, b"".join(out), buf
        if final and not c.in_used and not getattr(c, "n_members", 1):
            raise AssertionError("a final part, nothing used, nothing delivered, FLATE_HIP_OK")
        add = next(sizes, len(f)) if c.in_used else grow


def fixed(step):
    """The `sizes` of feed() for parts of `step` new bytes each."""
    while True:
        yield step


def cut_sizes(cuts):
    """The `sizes` of feed() for parts that end at the file offsets `cuts` (rising)."""
    last = 0
    for c in cuts:
        yield c - last
        last = c


def random_sizes(seed, top):
    rng = np.random.default_rng(seed)
    while True:
        yield int(rng.integers(1, top))


def summary(calls, data):
    """What must be the same for every cut: the bytes, the final status with its words, the input used."""
    last = calls[-1]
    return data, last.rc, last.bad_member, last.err_off, sum(c.in_used for c in calls)


SMALL_STEPS, LARGE_STEPS = (1, 27, 28, 29, 100), (4096, 65536, 70000)


def schedules(f, window_at=None):
    """[(name, sizes factory, grow)] for the file f: one final part; fixed parts (the small steps for files of at most
    8 KiB: a call per byte of a larger one shows nothing new); two parts [cut, rest] at every 37th cut, and at every
    cut of the 60 bytes around window_at; a seeded random schedule."""
    out = [("one part", lambda: iter(()), 1)]
    for s in (SMALL_STEPS if len(f) <= 8192 else ()) + LARGE_STEPS:
        out.append(("parts of %d" % s, (lambda s=s: fixed(s)), s))
    cuts = set(range(1, len(f), 37))
    if window_at is not None:
        cuts |= set(range(max(1, window_at - 30), min(len(f), window_at + 30)))
    if len(f) > 8192:
        cuts = set(sorted(cuts)[::max(1, len(cuts) // 24)])
    for c in sorted(cuts):
        out.append(("cut at %d" % c, (lambda c=c: cut_sizes([c])), 64))
    out.append(("random", lambda: random_sizes(len(f) + 11, max(2, min(len(f), 200000) // 3 + 2)), 4096))
    return out
