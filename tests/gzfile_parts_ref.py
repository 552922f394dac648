"""A gzip file of any members read in PARTS on the CPU: the reference of flate_hip_gzfile_reader_read.

Built on gzfile_ref.Walk over the WHOLE file -- the members, the units, their bits and sizes and the verdict --, on
gzfile_ref.hop, on one_ref.Walk's `reach` per member (one_parts_ref's notion: a unit is COMPLETE in a part iff the
bytes the serial reader has taken when it ends lie inside the part's raw range, which on every part is
[.., part end - 8)), on one_parts_ref.header_state for a header that a part cuts, and on zlib for the contents and the
CRC-32.  `Model` plays a whole reader: read(in_len, final, out_cap) -> Call for the part that begins where the sum of
in_used stands and has in_len bytes; final is taken to mean that the part ends where the file does.  The model knows
the default unit rule only (dynamic headers start units) and keeps no history, as the walks it is built on."""
import collections
import struct
import zlib

import gzfile_ref as gf
import gzip_ref as gz
import one_parts_ref as opr
import one_ref

OK, STREAM_END, INVALID, OUT_TOO_SMALL, CORRUPT, TOO_LARGE, EOF = 0, 1, -1, -2, -4, -6, -7
NONE = 0xffffffff

Call = collections.namedtuple("Call", "rc in_used out_len n_members n_units bad_member err_off stream_err_off")


def _inflate_some(raw):
    """What zlib makes of the raw stream, as far as it comes."""
    d = zlib.decompressobj(-15)
    try:
        return d.decompress(bytes(raw))
    except zlib.error:
        return opr.plain_of(raw)


class Model:
    def __init__(self, f, unit_max=1 << 28, plain=None):
        """plain: the bytes of the file this one was made from by damage behind which nothing is delivered -- what it
        delivers is a prefix of them (zlib gives no bytes of the call that fails); None: zlib says."""
        self.f, self.unit_max = bytes(f), unit_max
        f, n = self.f, len(self.f)
        self.w = w = gf.Walk(f)
        # per good unit: the file byte behind what the serial reader holds when it ends; per unit (the failing one
        # too): its member; per member: its bytes
        self.reach, self.member_of, plains = [], [], []
        members = w.n_members + (1 if w.status and self._has_header(w.member_off[w.n_members]) else 0)
        for j in range(members):
            p = w.member_off[j]
            r = p + gz.header_len(f, p, n)
            raw = f[r:max(r, n - 8)]
            m = one_ref.Walk(raw)
            self.reach += [r + x for x in m.reach[:m.n_units]]
            self.member_of += [j] * (m.n_units + (1 if m.status else 0))
            at = sum(len(x) for x in plains)
            plains.append(plain[at:at + m.out_len] if plain is not None else _inflate_some(raw)[:m.out_len])
            assert len(plains[-1]) == m.out_len
        assert len(self.reach) == w.n_units
        self.plains = plains
        self.plain = b"".join(plains)
        assert len(self.plain) == w.out_len
        self.reset()

    def _has_header(self, p):
        return p < len(self.f) and gz.header_len(self.f, p, len(self.f)) != 0

    def reset(self):
        self.consumed = self.produced = self.cur = 0
        self.boundary = True
        self.sticky = None

    def _member_end(self, j):
        """The byte behind member j's trailer (j whole)."""
        return (self.w.end_bits[j] + 7) // 8 + 8

    def _trailer_ok(self, j):
        e = self._member_end(j)
        p = self.plains[j]
        return self.f[e - 8:e] == struct.pack("<II", zlib.crc32(p), len(p) & 0xffffffff)

    def _fail(self, rc, bad_member, err_off, stream_err_off, out_len=0, n_members=0, n_units=0):
        self.produced += out_len
        self.sticky = Call(rc, 0, 0, 0, 0, bad_member, err_off, stream_err_off)
        return Call(rc, 0, out_len, n_members, n_units, bad_member, err_off, stream_err_off)

    def read(self, in_len, final, out_cap):
        """One call on the part of in_len bytes -> Call; the bytes are plain[produced before : + out_len]."""
        if self.sticky:
            return self.sticky
        w, f, a = self.w, self.f, self.consumed
        if in_len == 0:
            if not final:
                return Call(OK, 0, 0, 0, 0, NONE, -1, -1)
            if not self.boundary:
                j = self.member_of[self.cur]
                return self._fail(EOF, j, w.member_off[j], -1)
            self.sticky = Call(STREAM_END, 0, 0, 0, 0, NONE, -1, -1)
            return self.sticky
        end, stop = a + in_len, a + in_len - 8  # the part's end in the file, and its raw range's
        if self.boundary:
            j = self._members_before(self.cur)
            hdr, hl = opr.header_state(opr.GZIP, f[a:end])
            if hdr == opr.GOOD and in_len < hl + 8:
                hdr = opr.MORE
            if hdr == opr.BAD or (hdr == opr.MORE and final):
                return self._fail(CORRUPT, j, a, -1)
            if hdr == opr.MORE:
                return self._fail(TOO_LARGE, j, a, -1) if in_len >= self.unit_max else Call(OK, 0, 0, 0, 0, NONE, -1, -1)
        elif in_len <= 8:
            j = self.member_of[self.cur]
            return self._fail(EOF, j, w.member_off[j], -1) if final else Call(OK, 0, 0, 0, 0, NONE, -1, -1)
        # the chain over the part: the complete units from cur on, then what ends it
        k, verdict, stop_at = self.cur, None, None  # verdict: (rc, fail_unit bytes, bad_member, err_off, stream_err_off)
        while True:
            if k < w.n_units and self.reach[k] <= stop:
                j = self.member_of[k]
                k += 1
                if k < len(self.member_of) and self.member_of[k] == j:
                    continue
                # the member's final block lies behind: the parts hop
                kind, e, _ = gf.hop(f[:end], w.end_bits[j])
                assert e == self._member_end(j) <= end
                if kind == "end":
                    verdict, stop_at = (0, 0, NONE, -1, -1), e
                elif kind == "next":
                    continue
                elif final or opr.header_state(opr.GZIP, f[e:end])[0] == opr.BAD:
                    verdict = (CORRUPT, 0, j + 1, e, -1)
                else:
                    verdict, stop_at = (0, 0, NONE, -1, -1), e
                break
            if k == w.n_units and w.status:  # the unit the file's walk fails in
                j = w.bad_member
                raw = w.unit_bit[w.member_unit[j]] // 8
                if w.status == CORRUPT and raw + w.stream_err_off <= stop:
                    verdict = (CORRUPT, w.out_len - w.out_off[k], j, w.err_off, w.stream_err_off)
                elif final:
                    verdict = (w.status, w.out_len - w.out_off[k], j, w.err_off, w.stream_err_off)
            break
        sizes = [w.out_off[i + 1] - w.out_off[i] for i in range(self.cur, k)]
        n = len(sizes)
        whole = sum(sizes) + (verdict[1] if verdict else 0)
        if verdict and whole <= out_cap:
            n_del, total, terminal = n, whole, True
        else:
            n_del, total, terminal = 0, 0, False
            while n_del < n and total + sizes[n_del] <= out_cap:
                total += sizes[n_del]
                n_del += 1
            if n_del == 0:
                if n or verdict:
                    return Call(OUT_TOO_SMALL, 0, sizes[0] if n else whole, 0, 0, NONE, -1, -1)
                if in_len >= self.unit_max:
                    j = self.member_of[self.cur]
                    return self._fail(TOO_LARGE, j, w.member_off[j], -1)
                return Call(OK, 0, 0, 0, 0, NONE, -1, -1)
        # the members that end among the delivered units, in file order: their trailers
        nxt, n_end, before = self.cur + n_del, 0, self.produced
        for i in range(self.cur, nxt):
            j = self.member_of[i]
            if i + 1 < len(self.member_of) and self.member_of[i + 1] == j:
                continue
            if i + 1 == len(self.member_of) and j >= w.n_members:
                continue  # (the failing member's last good unit)
            if not self._trailer_ok(j):
                e = self._member_end(j)
                return self._fail(CORRUPT, j, w.member_off[j], e - w.member_off[j], out_len=w.out_off[i + 1] - before,
                                  n_members=n_end, n_units=i + 1 - self.cur)
            n_end += 1
        if terminal and verdict[0] != 0:
            return self._fail(verdict[0], verdict[2], verdict[3], verdict[4], out_len=total, n_members=n_end, n_units=n_del)
        self.produced += total
        self.cur = nxt
        if terminal:
            used = stop_at - a
            self.consumed, self.boundary = stop_at, True
            if final:
                self.sticky = Call(STREAM_END, 0, 0, 0, 0, NONE, -1, -1)
                return Call(STREAM_END, used, total, n_end, n_del, NONE, -1, -1)
            return Call(OK, used, total, n_end, n_del, NONE, -1, -1)
        used = w.unit_bit[nxt] // 8 - a
        self.consumed, self.boundary = a + used, False
        return Call(OK, used, total, n_end, n_del, NONE, -1, -1)

    def _members_before(self, unit):
        return len([m for m in self.w.member_unit[:self.w.n_members] if m < unit]) if unit else 0


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
        if final and not c.in_used and not c.out_len:
            raise AssertionError("a final part, nothing used, nothing delivered, FLATE_HIP_OK")
        add = next(sizes, len(f)) if (c.in_used or c.out_len) else grow


def model_reader(m):
    """`read` of feed() for a Model: the part is wherever the model stands."""
    def read(buf, final, out_cap):
        before = m.produced
        c = m.read(len(buf), final, out_cap if out_cap is not None else 1 << 62)
        return c, (m.plain[before:before + c.out_len] if c.out_len and c.rc != OUT_TOO_SMALL else b"")
    return read


def cut_sizes(cuts):
    """The `sizes` of feed() for parts that end at the file offsets `cuts` (rising)."""
    last = 0
    for c in cuts:
        yield c - last
        last = c
