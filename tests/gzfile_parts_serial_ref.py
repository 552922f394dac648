"""A gzip file read in PARTS with short members decoded WHOLE inside a part, on the CPU: the reference of
flate_hip_gzfile_reader_read on a handle with flate_hip_gzfile_reader_set_serial_max(S).

`Model` has gzfile_parts_ref.Model's interface plus S: read(in_len, final, out_cap) -> (Call, route), Call being the
eight words and route = (serial_members, open_stop, find_from) as flate_hip_gzfile_reader_last_route reports them after
that call.  It is built on gzfile_ref.Walk over the whole file (through gzfile_parts_ref.Model, whose units, reach and
trailers it keeps), on gzfile_serial_ref.candidate / is_whole over the PART's bytes -- zlib's raw decoder as the
size-only decode over the serial range [p + hl, min(len(part) - 8, p + S)) -- and on gzfile_ref.hop.

The rule, restated from include/flate_hip.h.  A member whose header starts at part offset p is WHOLE when the whole
test holds over the part and it inflates to at most out_cap bytes: one unit.  It is OPEN when the part is not final,
len(part) - 8 < p + S and the decode ran out of input: a hop onto it ends the chain with a BOUNDARY stop at p; at the
root it is LONG.  Every other member is LONG: the units of S = 0.  With S >= 1 a call whose first undelivered unit
starts a member stops in front of that member's header.  find_from: 0 INSIDE a member; else the offset of the first
member on the chain from the root that is not whole (an OPEN one behind the root, the file's end, a dead hop or a
stop: len(part)); 0 with S = 0."""
import gzfile_parts_ref as base
import gzfile_ref as gf
import gzfile_serial_ref as gs
import one_parts_ref as opr
from gzfile_parts_ref import (CORRUPT, EOF, NONE, OK, OUT_TOO_SMALL, STREAM_END, TOO_LARGE, Call,  # noqa: F401
                              cut_sizes, feed)

LONG, WHOLE, OPEN = 0, 1, 2
NO_ROUTE = (0, 0, 0)


def verdict(part, p, S, final, out_cap):
    """THE THREE VERDICTS of the offset p that passes the header rule over part[p:] -> (LONG | WHOLE | OPEN, size)."""
    n = len(part)
    hl, E, st, used, size = gs.candidate(part, p, S)
    if gs.is_whole(p, hl, E, st, used):
        return (WHOLE if size <= out_cap else LONG), size
    if final:
        return LONG, 0
    by_part = max(n - 8, 0) < p + S
    ran_out = hl == 0 or p + hl > E or st == EOF
    return (OPEN if by_part and ran_out else LONG), 0


class Model(base.Model):
    def __init__(self, f, S=0, unit_max=1 << 28, plain=None):
        self.S = S
        self._verdicts = {}  # (the header's file offset, the part's end, final, out_cap) -> verdict(): a cut decides it
        base.Model.__init__(self, f, unit_max=unit_max, plain=plain)

    def reset(self):
        base.Model.reset(self)
        self.route = NO_ROUTE

    def _first_of(self, k):
        """Unit k (a good one, or the failing one of a member with a header) starts its member."""
        return k < len(self.member_of) and k == self.w.member_unit[self.member_of[k]]

    def read(self, in_len, final, out_cap):
        c = self._read(in_len, final, out_cap)
        return c, self.route

    def _read(self, in_len, final, out_cap):
        if self.sticky:
            return self.sticky
        w, f, a, S = self.w, self.f, self.consumed, self.S
        if in_len == 0:
            if not final:
                return Call(OK, 0, 0, 0, 0, NONE, -1, -1)
            if not self.boundary:
                j = self.member_of[self.cur]
                return self._fail(EOF, j, w.member_off[j], -1)
            self.sticky = Call(STREAM_END, 0, 0, 0, 0, NONE, -1, -1)
            return self.sticky
        end, stop = a + in_len, a + in_len - 8  # the part's end in the file, and its raw range's
        inside = not self.boundary
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
        # the chain over the part: items (first unit, the unit behind, bytes, is a whole member), then what ends it
        part = f[a:end]
        items, k, verd, stop_at, open_stop = [], self.cur, None, None, 0
        find_from = 0 if (S == 0 or inside) else None
        while True:
            ended = None  # the member whose final block lies behind the item just taken
            if S and self._first_of(k) and not (k == self.cur and inside):
                j = self.member_of[k]
                p = w.member_off[j] - a
                key = (a + p, end, final, out_cap)
                if key not in self._verdicts:
                    self._verdicts[key] = verdict(part, p, S, final, out_cap)
                v, size = self._verdicts[key]
                if v == OPEN and p > 0:
                    verd, stop_at, open_stop = (0, 0, NONE, -1, -1), a + p, 1
                    break
                if v == WHOLE:
                    assert j < w.n_members and size == w.sizes[j]
                    items.append((k, w.member_unit[j + 1], size, True))
                    k, ended = w.member_unit[j + 1], j
                elif find_from is None:
                    find_from = p  # LONG, or OPEN at the root
            if ended is None and k < w.n_units and self.reach[k] <= stop:
                j = self.member_of[k]
                items.append((k, k + 1, w.out_off[k + 1] - w.out_off[k], False))
                k += 1
                if k < len(self.member_of) and self.member_of[k] == j:
                    continue
                ended = j
            if ended is not None:  # the parts hop
                j = ended
                kind, e, _ = gf.hop(f[:end], w.end_bits[j])
                assert e == self._member_end(j) <= end
                if kind == "end":
                    verd, stop_at = (0, 0, NONE, -1, -1), e
                elif kind == "next":
                    continue
                elif final or opr.header_state(opr.GZIP, f[e:end])[0] == opr.BAD:
                    verd = (CORRUPT, 0, j + 1, e, -1)
                else:
                    verd, stop_at = (0, 0, NONE, -1, -1), e
                break
            if k == w.n_units and w.status:  # the unit the file's walk fails in
                j = w.bad_member
                raw = w.unit_bit[w.member_unit[j]] // 8
                if w.status == CORRUPT and raw + w.stream_err_off <= stop:
                    verd = (CORRUPT, w.out_len - w.out_off[k], j, w.err_off, w.stream_err_off)
                elif final:
                    verd = (w.status, w.out_len - w.out_off[k], j, w.err_off, w.stream_err_off)
            break
        if find_from is None:
            find_from = in_len
        self.route = (0, open_stop, find_from)
        sizes = [it[2] for it in items]
        n = len(sizes)
        whole = sum(sizes) + (verd[1] if verd else 0)
        if verd and whole <= out_cap:
            n_del, total, terminal = n, whole, True
        else:
            n_del, total, terminal = 0, 0, False
            while n_del < n and total + sizes[n_del] <= out_cap:
                total += sizes[n_del]
                n_del += 1
            if n_del == 0:
                if n or verd:
                    return Call(OUT_TOO_SMALL, 0, sizes[0] if n else whole, 0, 0, NONE, -1, -1)
                if in_len >= self.unit_max:
                    j = self.member_of[self.cur]
                    return self._fail(TOO_LARGE, j, w.member_off[j], -1)
                return Call(OK, 0, 0, 0, 0, NONE, -1, -1)

        def serial(count):
            self.route = (sum(1 for it in items[:count] if it[3]), open_stop, find_from)

        # the members that end among the delivered units, in file order: their trailers
        nxt = items[n_del][0] if n_del < n else k
        n_end, before = 0, self.produced
        for x, (k0, k1, _, _) in enumerate(items[:n_del]):
            i = k1 - 1
            j = self.member_of[i]
            if i + 1 < len(self.member_of) and self.member_of[i + 1] == j:
                continue
            if i + 1 == len(self.member_of) and j >= w.n_members:
                continue  # (the failing member's last good unit)
            if not self._trailer_ok(j):
                e = self._member_end(j)
                serial(x + 1)
                return self._fail(CORRUPT, j, w.member_off[j], e - w.member_off[j], out_len=w.out_off[k1] - before,
                                  n_members=n_end, n_units=x + 1)
            n_end += 1
        serial(n_del)
        if terminal and verd[0] != 0:
            return self._fail(verd[0], verd[2], verd[3], verd[4], out_len=total, n_members=n_end, n_units=n_del)
        self.produced += total
        self.cur = nxt
        if terminal:
            used = stop_at - a
            self.consumed, self.boundary = stop_at, True
            if final:
                self.sticky = Call(STREAM_END, 0, 0, 0, 0, NONE, -1, -1)
                return Call(STREAM_END, used, total, n_end, n_del, NONE, -1, -1)
            return Call(OK, used, total, n_end, n_del, NONE, -1, -1)
        if S and self._first_of(nxt):  # stop at the BOUNDARY in front of that member's header
            used = w.member_off[self.member_of[nxt]] - a
            self.consumed, self.boundary = a + used, True
            return Call(OK, used, total, n_end, n_del, NONE, -1, -1)
        used = w.unit_bit[nxt] // 8 - a
        self.consumed, self.boundary = a + used, False
        return Call(OK, used, total, n_end, n_del, NONE, -1, -1)


def model_reader(m, routes=None):
    """`read` of gzfile_parts_ref.feed() for a Model: the part is wherever the model stands; routes: a list that takes
    every call's route."""
    def read(buf, final, out_cap):
        before = m.produced
        c, route = m.read(len(buf), final, out_cap if out_cap is not None else 1 << 62)
        if routes is not None:
            routes.append(route)
        return c, (m.plain[before:before + c.out_len] if c.out_len and c.rc != OUT_TOO_SMALL else b"")
    return read
