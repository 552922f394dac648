"""One long stream read in PARTS on the CPU: the reference of flate_hip_one_reader_read.

Built on one_ref.Walk -- the units of the WHOLE raw stream, their bits, their sizes and `reach`, the bytes of the stream
the serial reader has taken when a unit ends (the three bits of the next header included) -- and on zlib for the
contents.  A unit is COMPLETE in a part iff its reach lies inside the part's raw range; everything a call must return
follows from that, from the capacities and from the container's bytes.  `Model` plays a whole reader: read(in_len,
final, out_cap) -> Call, for the part that begins where the sum of in_used stands and has in_len bytes.  `discovery`
exposes what the device's discovery over that part yields (part-relative bits and offsets), which is what
csrc/one_parts_rule.h is given: tests/test_one_parts_rule_model.py drives the rule with it."""
import collections
import struct
import zlib

import one_ref as ref

OK, STREAM_END, INVALID, OUT_TOO_SMALL, CORRUPT, TOO_LARGE, EOF = 0, 1, -1, -2, -4, -6, -7
RAW, ZLIB, GZIP = ref.RAW, ref.ZLIB, ref.GZIP
GOOD, BAD, MORE = 0, 1, 2
TRAILER = {RAW: 0, ZLIB: 4, GZIP: 8}

Call = collections.namedtuple("Call", "rc in_used out_len n_units err_off")
# what the discovery over one part yields: the complete units (bits counted from the part's first raw byte, n + 1
# entries each), the verdict behind them and what the failing unit produced in front of its failure
Discovery = collections.namedtuple("Discovery", "hdr raw_off rc err_off fail_unit fail_out unit_bit out_off")


def header_state(kind, m):
    """The container's header at the front of the bytes m -> (GOOD, its length) / (BAD, 0) / (MORE, 0): refused only
    because m ends here.  zlib: RFC 1950 2.2 without FDICT; gzip: RFC 1952 2.3, read field by field."""
    m = bytes(m)
    if kind == RAW:
        return GOOD, 0
    if kind == ZLIB:
        if m[:1] and (m[0] & 15 != 8 or m[0] >> 4 > 7):
            return BAD, 0
        if len(m) < 2:
            return MORE, 0
        return (BAD, 0) if (m[0] * 256 + m[1]) % 31 or m[1] & 0x20 else (GOOD, 2)
    if any(a != b for a, b in zip(m[:3], b"\x1f\x8b\x08")) or (m[3:4] and m[3] & 0xe0):
        return BAD, 0
    if len(m) < 10:  # the fixed bytes; then what FLG announces, in the RFC's order
        return MORE, 0
    p, flg = 10, m[3]
    if flg & 4:
        if len(m) < p + 2:
            return MORE, 0
        p += 2 + struct.unpack_from("<H", m, p)[0]
    for bit in (8, 16):
        if flg & bit:
            z = m.find(b"\0", p)
            if z < 0:
                return MORE, 0
            p = z + 1
    if flg & 2:
        p += 2
    return (MORE, 0) if p > len(m) else (GOOD, p)


def plain_of(raw):
    """What zlib makes of the raw stream, as far as it comes."""
    d = zlib.decompressobj(-15)
    try:
        return d.decompress(bytes(raw))
    except zlib.error:
        out, d = [], zlib.decompressobj(-15)
        try:
            for i in range(0, len(raw), 1):
                out.append(d.decompress(raw[i:i + 1]))
        except zlib.error:
            pass
        return b"".join(out)


class Model:
    """A reader over the member f (kind: RAW / ZLIB / GZIP), dynamic headers starting units (the default rule)."""

    def __init__(self, f, kind, unit_max=1 << 28, walk=None, plain=None):
        """walk, plain: one_ref.Walk of the raw stream and its bytes, where the caller has them already."""
        self.f, self.kind, self.unit_max, self.tl = bytes(f), kind, unit_max, TRAILER[kind]
        self.w, self.plain, self.hl, self._cut = walk, plain, None, {}
        self.reset()

    def reset(self):
        self.consumed = self.produced = self.cur = 0
        self.header_done = self.pending = False
        self.status, self.err_off = 0, -1

    def _walk(self):
        self.raw = self.f[self.hl:]
        if self.w is None:
            self.w = ref.Walk(self.raw)
        if self.plain is None:
            self.plain = plain_of(self.raw)
        return self.w

    def _cut_out(self, end):
        """Bytes the serial decoder has produced when the raw stream ends at byte `end`."""
        if end not in self._cut:
            self._cut[end] = ref.Walk(self.raw[:end]).out_len
        return self._cut[end]

    def discovery(self, in_len, final):
        """The discovery over the part f[consumed, consumed + in_len)."""
        a = self.consumed
        part = self.f[a:a + in_len]
        raw_off = 0
        if not self.header_done:
            hdr, hl = header_state(self.kind, part)
            if final and (hdr == MORE or (hdr == GOOD and in_len < hl + self.tl)):
                hdr = BAD
            if hdr != GOOD:
                return Discovery(hdr, 0, CORRUPT if hdr == BAD else 0, 0 if hdr == BAD else -1, 0, 0, [], [])
            raw_off, self.hl = hl, hl
        w = self._walk()
        hl = self.hl
        lo = a + raw_off - hl                     # the part's first raw byte, counted in the raw stream
        end = a + in_len - hl                     # ... and the end of its raw range
        if final:
            end = max(end - self.tl, lo)
        if end <= lo and not final:
            return Discovery(GOOD, raw_off, None, -1, 0, 0, [], [])  # no raw byte: no candidate
        k = self.cur
        while k < w.n_units and w.reach[k] <= end:
            k += 1
        rel = lambda bit: bit - 8 * lo
        base = w.out_off[self.cur]
        bits = [rel(b) for b in w.unit_bit[self.cur:k + 1]]
        offs = [o - base for o in w.out_off[self.cur:k + 1]]
        if k == w.n_units and w.status == 0:
            return Discovery(GOOD, raw_off, 0, -1, 0, 0, bits, offs)
        if k == w.n_units and w.status == CORRUPT and w.err_off <= end:
            fail_out = w.out_len - w.out_off[k]
            return Discovery(GOOD, raw_off, CORRUPT, w.err_off - lo, 1, fail_out, bits, offs)
        fail_out = max(self._cut_out(end) - w.out_off[k], 0) if final else 0
        return Discovery(GOOD, raw_off, EOF, -1, 1, fail_out, bits, offs)

    def read(self, in_len, final, out_cap):
        """One call on the part of in_len bytes -> Call; the bytes are plain[produced_before : + out_len]."""
        if self.status:
            return Call(self.status, 0, 0, 0, self.err_off if self.status < 0 else -1)
        fail = lambda st, eo, **kw: self._fail(st, eo, **kw)
        if self.pending:
            if in_len < self.tl:
                return fail(EOF, -1) if final else Call(OK, 0, 0, 0, -1)
            self.pending = False
            ok = self._trailer_ok(self.consumed)
            self.consumed += self.tl
            if not ok:
                return fail(CORRUPT, self.consumed, in_used=self.tl)
            self.status = STREAM_END
            return Call(STREAM_END, self.tl, 0, 0, -1)
        if in_len == 0:
            if not final:
                return Call(OK, 0, 0, 0, -1)
            return fail(CORRUPT, 0) if not self.header_done and self.kind != RAW else fail(EOF, -1)
        d = self.discovery(in_len, final)
        if d.hdr == BAD:
            return fail(CORRUPT, 0)
        if d.hdr == MORE or d.rc is None:
            return fail(EOF, -1) if final else Call(OK, 0, 0, 0, -1)
        n, verdict = len(d.unit_bit) - 1, d.rc in (0, CORRUPT) or (d.rc == EOF and final)
        whole = d.out_off[n] + (d.fail_out if verdict and d.fail_unit else 0)
        lo = self.consumed + d.raw_off - self.hl
        if verdict and whole <= out_cap:
            n_del, total, terminal = n, whole, True
        else:
            n_del = max(k for k in range(n + 1) if d.out_off[k] <= out_cap)
            total, terminal = d.out_off[n_del], False
            if n_del == 0:
                if n or verdict:
                    return Call(OUT_TOO_SMALL, 0, d.out_off[1] if n else whole, 0, -1)
                if in_len >= self.unit_max:
                    return fail(TOO_LARGE, -1)
                return Call(OK, 0, 0, 0, -1)
        if terminal and d.rc != 0:
            self.produced += total
            return fail(d.rc, lo + d.err_off if d.err_off >= 0 else -1, out_len=total, n_units=n_del)
        ended = terminal
        bit = d.unit_bit[n_del]
        used = d.raw_off + ((bit + 7) // 8 if ended else bit // 8)
        self.header_done, self.cur, self.produced = True, self.cur + n_del, self.produced + total
        if not ended:
            self.consumed += used
            return Call(OK, used, total, n_del, -1)
        if in_len - used < self.tl:
            self.consumed += used
            self.pending = True
            return Call(OK, used, total, n_del, -1)
        ok = self._trailer_ok(self.consumed + used)
        used += self.tl
        self.consumed += used
        if not ok:
            return fail(CORRUPT, self.consumed, in_used=0, out_len=total, n_units=n_del)
        self.status = STREAM_END
        return Call(STREAM_END, used, total, n_del, -1)

    def _fail(self, st, eo, in_used=0, out_len=0, n_units=0):
        self.status, self.err_off = st, eo
        return Call(st, in_used, out_len, n_units, eo)

    def _trailer_ok(self, at):
        t = self.f[at:at + self.tl]
        if self.kind == ZLIB:
            return t == struct.pack(">I", zlib.adler32(self.plain))
        if self.kind == GZIP:
            return t == struct.pack("<II", zlib.crc32(self.plain), len(self.plain) & 0xffffffff)
        return True


def feed(read, f, sizes, out_cap, max_calls, grow=1):
    """The feeding loop every test uses, with its hard cap on calls.  read(part bytes, final, out_cap) -> (Call, the
    bytes delivered); sizes: an iterator of how many NEW bytes each call appends (exhausted: everything left); a call
    that used nothing and delivered nothing is followed by `grow` more bytes.  -> ([Call], the bytes, the unused
    rest)."""
    sizes = iter(sizes)
    pos, buf, calls, out = 0, b"", [], []
    add = next(sizes, len(f))
    while True:
        assert len(calls) < max_calls, "the reader makes no progress: %d calls" % len(calls)
        pos, buf = pos + len(f[pos:pos + add]), buf + f[pos:pos + add]
        final = pos >= len(f)
        c, got = read(buf, final, out_cap)
        calls.append(c)
        out.append(bytes(got))
        buf = buf[c.in_used:]
        if c.rc != OK:
            return calls, b"".join(out), buf
        if c.rc == OK and final and not c.in_used and not c.out_len:
            raise AssertionError("a final part, nothing used, nothing delivered, FLATE_HIP_OK")
        add = next(sizes, len(f)) if (c.in_used or c.out_len) else grow


def model_reader(m):
    """`read` of feed() for a Model: the part is wherever the model stands."""
    def read(buf, final, out_cap):
        before = m.produced
        c = m.read(len(buf), final, out_cap if out_cap is not None else 1 << 62)
        return c, (m.plain[before:before + c.out_len] if c.out_len and c.rc != OUT_TOO_SMALL else b"")
    return read
