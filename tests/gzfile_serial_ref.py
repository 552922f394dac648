"""Short members of a gzip file decoded WHOLE (the option "gzfile_serial_max" = S) on the CPU: the model of what
flate_hip_gzfile_index / flate_hip_gzfile_read report with the option on, over gzfile_ref.Walk (the option-0 walk) and
gzip_ref (the header rule; zlib's raw decoder as the size-only serial decode).

The rule, restated from include/flate_hip.h: the member whose header starts at p and is hl bytes long has the serial
range [p + hl, E), E = min(n - 8, p + S); it is WHOLE iff the size-only decode over that range ends its final block with
status 0 and p + hl + used <= E.  A whole member is one unit; every other member keeps option 0's units."""
import numpy as np

import gzfile_ref as ref
import gzip_ref as gz

S_MAX = (1 << 28) - 1


def serial_end(n, p, S):
    raw_end = max(n - 8, 0)
    if p >= raw_end:
        return raw_end
    return p + S if raw_end - p > S else raw_end


def candidate(buf, p, S):
    """(hl, E, status, used, size) of the offset p that passes the header rule over buf[p:]."""
    n = len(buf)
    hl = gz.header_len(buf, p, n)
    E = serial_end(n, p, S)
    lo = p + hl if hl and p + hl <= E else E
    return (hl, E) + gz.size_only(buf, lo, E)


def is_whole(p, hl, E, status, used):
    return status == 0 and hl != 0 and p + hl <= E and used <= E - (p + hl)


def table(buf):
    """The offsets of List B: every offset that passes the header rule with no clip."""
    buf, out, p = bytes(buf), [], -1
    while True:
        p = buf.find(gz.MAGIC, p + 1)
        if p < 0:
            return out
        if gz.header_len(buf, p, len(buf)):
            out.append(p)


class Model:
    """With the option at S: whole (per good member of the walk), unit_bit / out_off / member_unit (collapsed),
    n_units, find_from, serial_members, unit_members; `ends`: per good member hl + used of an unclipped decode (None for
    a member zlib does not decode alone).  Everything else is the walk's, unchanged."""

    def __init__(self, buf, S, walk=None):
        buf = bytes(buf)
        n = len(buf)
        w = walk if walk is not None else ref.Walk(buf)
        self.walk, self.S = w, S
        self.whole, self.ends = [], []
        self.unit_bit, self.out_off, self.member_unit = [], [], []
        last_end = None  # the rounded end of the last good unit when that is a whole member
        for k in range(w.n_members):
            p = w.member_off[k]
            hl, E, st, used, _ = candidate(buf, p, S)
            wh = is_whole(p, hl, E, st, used)
            self.whole.append(wh)
            st1, used1, _ = gz.size_only(buf, p + hl, max(n - 8, p + hl))
            self.ends.append(hl + used1 if st1 == 0 else None)
            a, b = w.member_unit[k], w.member_unit[k + 1]
            self.member_unit.append(len(self.unit_bit))
            keep = range(a, a + 1) if wh else range(a, b)
            self.unit_bit += [w.unit_bit[u] for u in keep]
            self.out_off += [w.out_off[u] for u in keep]
            last_end = 8 * (p + hl + used) if wh else None
        # the member the chain breaks in (never whole: its decode fails) keeps its good units
        self.member_unit.append(len(self.unit_bit))
        tail = range(w.member_unit[w.n_members], w.n_units)
        self.unit_bit += [w.unit_bit[u] for u in tail]
        self.out_off += [w.out_off[u] for u in tail]
        self.n_units = len(self.unit_bit)
        failing_starts = w.status != 0 and gz.header_len(buf, w.err_off, n) != 0  # (else: no member could start there)
        # entry n_units: where a failing unit starts is the walk's; the end of a whole member is byte-rounded
        end_bit = w.unit_bit[w.n_units]
        if last_end is not None and not failing_starts:
            end_bit = last_end
        self.unit_bit.append(end_bit)
        self.out_off.append(w.out_off[w.n_units])
        self.serial_members = sum(self.whole)
        self.unit_members = w.n_members - self.serial_members
        # find_from: the first member on the walk that is not whole
        self.find_from = n
        if n and gz.header_len(buf, 0, n):
            for k in range(w.n_members):
                if not self.whole[k]:
                    self.find_from = w.member_off[k]
                    break
            else:
                if failing_starts:
                    self.find_from = w.err_off

    def index_words(self):
        w = self.walk
        return (w.status, self.n_units, w.n_members, w.out_bytes, w.bad_member, w.err_off, w.stream_err_off)


def flat_text(n, seed):
    """n bytes of words drawn evenly from 4000: it compresses about twofold, so that zlib's blocks are many."""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(2, 10, 4000)]
    return b" ".join(words[int(i)] for i in rng.integers(0, 4000, n // 4 + 8))[:n].ljust(n, b".")


def long_member(nbytes, seed):
    """A level-6 member of nbytes of seeded text (the tests assert: at least 3 units) -> (member, plain)."""
    plain = flat_text(nbytes, seed)
    return gz.member(plain, 6), plain


def mixed_file():
    """Three tiny members, a LONG one, two tiny ones, a second long one, one tiny one -> (file, plain, the long
    members' indices)."""
    t, pt = [], []
    for k, seed in enumerate((41, 42, 43, 44, 45, 46)):
        p = gz.text(300 + 170 * k, seed=seed)
        t.append(gz.member(p, 6) if k % 2 else gz.fixed(p))
        pt.append(p)
    a, pa = long_member(260000, 51)
    b, pb = long_member(250000, 52)
    parts = [t[0], t[1], t[2], a, t[3], t[4], b, t[5]]
    plain = [pt[0], pt[1], pt[2], pa, pt[3], pt[4], pb, pt[5]]
    f = b"".join(parts)
    assert len(f) < 1000000
    return f, b"".join(plain), (3, 6)
