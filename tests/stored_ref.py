"""The unit rule of the option "one_stored_units" on the CPU, on top of tests/one_ref.py: units start at bit 0 and at
every dynamic AND every stored block header the serial decode reaches.

`Walk` is one_ref.Walk's serial decode restated with that rule.  one_ref.Walk keeps the blocks it read whole but not
where the block it failed in started, nor of what type it was -- and that block's header starts the failing unit when
its type is 0 or 2 --, so the loop stands here once more, built from one_ref's own reader (Bits, read_dynamic, the
codes).  With stored=False it is one_ref.Walk, which tests/test_stored_rule_model.py holds it against on the whole
corpus.  `rule` restates deflate_stored_header_ok (csrc/deflate_block_rule.h) at one bit offset; `hits` finds the same
offsets from the other side, from every aligned LEN / NLEN pair; `candidates` is what the discovery probes."""
import struct

import one_ref

OK, CORRUPT, TOO_LARGE, UNEXPECTED_EOF = one_ref.OK, one_ref.CORRUPT, one_ref.TOO_LARGE, one_ref.UNEXPECTED_EOF


def rule(raw, bit):
    """THE STORED RULE at one bit offset: BTYPE = 0 behind either BFINAL, the padding up to the next byte boundary
    unread, four bytes from there on inside the stream, LEN the complement of NLEN."""
    q = (bit + 3 + 7) // 8
    if q + 4 > len(raw):
        return False
    btype = ((raw[(bit + 1) >> 3] >> ((bit + 1) & 7)) & 1) | (((raw[(bit + 2) >> 3] >> ((bit + 2) & 7)) & 1) << 1)
    if btype != 0:
        return False
    ln, nl = struct.unpack_from("<HH", raw, q)
    return ln == (~nl & 0xffff)


def hits(raw):
    """Every bit offset that passes the rule: the (up to 8) offsets in front of each aligned LEN / NLEN pair whose
    BTYPE bits are 0."""
    v, out = int.from_bytes(raw, "little"), []
    for q in range(1, len(raw) - 3):
        ln, nl = struct.unpack_from("<HH", raw, q)
        if ln != (~nl & 0xffff):
            continue
        for bit in range(max(8 * q - 10, 0), 8 * q - 2):  # (bit + 10) // 8 == q
            if (v >> (bit + 1)) & 3 == 0:
                out.append(bit)
    return sorted(out)


def candidates(raw):
    """Every bit offset the discovery probes with the option on: one_ref.candidates and the stored hits."""
    return sorted(set(one_ref.candidates(raw)) | set(hits(raw)))


class Walk:
    """The serial decode of raw from bit 0, without history, cut into units at every header of a type in `starts_unit`
    (stored=True: dynamic and stored; False: dynamic alone, which is one_ref.Walk).  The fields are one_ref.Walk's:
    status, err_off, blocks, n_units, unit_bit / out_off (n_units + 1 entries; of a stream that fails the good units
    and where the failing one starts), out_bytes, out_len, far, end_bit, reach."""

    def __init__(self, raw, stored=True):
        raw = bytes(raw)
        starts_unit = (0, 2) if stored else (2,)
        r = one_ref.Bits(raw)
        self.blocks, self.far, self.status, self.err_off = [], False, OK, -1
        starts, total, self.reach = [0], 0, []
        before = [0]  # per entry of starts: the output in front of it
        try:
            while True:
                at = r.pos
                h = r.get(3)
                final, typ = h & 1, h >> 1
                if typ == 3:
                    raise one_ref.Stop(CORRUPT)
                if typ in starts_unit and at:  # the failing block's start and type are known HERE, before it can fail
                    starts.append(at)
                    before.append(total)
                    self.reach.append((r.hw + 7) // 8)
                n = 0
                if typ == 0:
                    p = (r.hw + 7) // 8
                    if len(raw) - p < 4:
                        r.hw = r.end
                        raise one_ref.Stop(UNEXPECTED_EOF)
                    ln, nl = struct.unpack_from("<HH", raw, p)
                    r.hw = 8 * (p + 4)
                    if ln != (~nl & 0xffff):
                        raise one_ref.Stop(CORRUPT)
                    n = min(ln, len(raw) - p - 4)
                    total += n
                    r.pos = r.hw = 8 * (p + 4 + n)
                    if n < ln:
                        raise one_ref.Stop(UNEXPECTED_EOF)
                else:
                    if typ == 1:
                        lit, dist = one_ref.FIXED
                        lmin = 7
                    else:
                        lit, dist, ll = one_ref.read_dynamic(r)
                        lmin = max(lit.min, ll[256])
                    while True:
                        s = r.sym(lit, lmin)
                        if s < 256:
                            n += 1
                            total += 1
                            continue
                        if s == 256:
                            break
                        if s >= 286:
                            raise one_ref.Stop(CORRUPT)
                        ln = one_ref.LBASE[s - 257] + (r.get(one_ref.LEXT[s - 257]) if one_ref.LEXT[s - 257] else 0)
                        d = r.sym(dist, dist.min)
                        if d >= 30:
                            raise one_ref.Stop(CORRUPT)
                        nb = (d - 2) >> 1 if d >= 4 else 0
                        d = one_ref.DBASE[d] + (r.get(nb) if nb else 0)
                        self.far = self.far or d > total
                        n += ln
                        total += ln
                self.blocks.append((at, typ, final, n))
                if final:
                    self.reach.append((r.hw + 7) // 8)
                    break
        except one_ref.Stop as e:
            self.status = e.status
            self.err_off = (r.hw + 7) // 8 if e.status == CORRUPT else -1
        self.out_len, self.end_bit = total, r.pos
        if self.status == OK:
            self.n_units = len(starts)
            self.unit_bit = starts + [r.pos]
            self.out_off = before + [total]
        else:  # the last start is the failing unit's; its out_off is what the whole BLOCKS in front inflate to
            self.n_units = len(starts) - 1
            self.unit_bit = starts
            self.out_off = before
        self.out_bytes = total if self.status == OK else 0


def gzfile_walk(buf):
    """gzfile_ref.Walk with every member's units cut by the stored rule: that walk asks one_ref for each member's
    units by name, so the name is lent to the Walk above for the length of the call."""
    import gzfile_ref
    keep = one_ref.Walk
    one_ref.Walk = Walk
    try:
        return gzfile_ref.Walk(buf)
    finally:
        one_ref.Walk = keep


# ---- the hand-built corpus (deflate_corpus.Writer) ----

def stored_block(w, payload, final=False, pad=0xff, length=None, nlength=None, cut=None):
    """Writer.stored with the padding bits between the header and LEN written from `pad` (LSB first) where align()
    gives zeros: the decoder drops them unread, and so must the rule."""
    w.header(final, 0)
    k = 0
    while w.pos % 8:
        w.put((pad >> k) & 1, 1)
        k += 1
    w.hw = max(w.hw, w.pos)
    ln = len(payload) if length is None else length
    nl = (~ln & 0xffff) if nlength is None else nlength
    w.put_read(ln, 16)
    w.put_read(nl, 16)
    body = payload if cut is None else payload[:cut]
    for b in body:
        w.put(b, 8)
    w.out += body


def _fixed(w, data, final=False):
    blk = w.fixed(final)
    blk.lits(data)
    blk.end()


def _dynamic(w, final, build):
    import deflate_corpus as dc
    lit, dist = dc.full_tree_lens()
    blk = w.dynamic(lit, dist, final=final)
    build(blk)
    blk.end()


def hand_streams():
    """[(what, raw stream, plain, units with the option on)] -- streams the serial decoder takes."""
    import deflate_corpus as dc
    import gzip_ref
    text = (dc.TEXT * 4)[:150]
    out = []
    for phase in range(8):  # the header's three bits start at bit `phase` of a byte
        w = dc.Writer()
        dc.prefix_block(w, phase)
        assert w.pos % 8 == phase
        stored_block(w, text[:60 + phase])
        _fixed(w, b"tail", True)
        out.append(("a stored header at bit phase %d, ones as padding" % phase, w.data(), bytes(w.out), 2))
    w = dc.Writer()
    _fixed(w, b"fixed one;")
    stored_block(w, text[:40])
    _fixed(w, b"fixed two;")
    stored_block(w, text[40:90], final=True)
    out.append(("fixed, stored, fixed, stored: cut at the stored headers only", w.data(), bytes(w.out), 3))
    w = dc.Writer()
    for _ in range(3):
        stored_block(w, b"")
    stored_block(w, text[:33])
    for _ in range(3):
        stored_block(w, b"", pad=0x55)
    _dynamic(w, False, lambda blk: (blk.lits(text[:20]), blk.match(10, 30)))
    for k in range(3):
        stored_block(w, b"", final=k == 2)
    out.append(("empty stored blocks: zero-byte units first, in the middle and last", w.data(), bytes(w.out), 11))
    w = dc.Writer()
    _dynamic(w, False, lambda blk: blk.lits(text[:50]))
    stored_block(w, text[50:120], final=True)
    out.append(("a final stored block behind a dynamic one", w.data(), bytes(w.out), 2))
    # a stored block whose data is a whole stream with dynamic and (empty) stored headers of its own: off the path
    inner = one_ref.deflate(gzip_ref.text(9000, seed=29), 6, flush_every=3000)
    w = dc.Writer()
    dc.prefix_block(w, 3)
    stored_block(w, inner)
    _fixed(w, b"tail", True)
    out.append(("a stream with stored and dynamic headers inside a stored block", w.data(), bytes(w.out), 2))
    w = dc.Writer()
    _dynamic(w, False, lambda blk: blk.lits(text[:30]))
    stored_block(w, gzip_ref.rand(100, seed=3))
    _dynamic(w, True, lambda blk: (blk.lits(b"xy"), blk.match(20, 125), blk.match(5, 152)))
    out.append(("a distance across a 100-byte stored unit into the unit in front", w.data(), bytes(w.out), 3))
    w = dc.Writer()
    _fixed(w, b"front:")
    stored_block(w, gzip_ref.rand(40000, seed=4))
    _dynamic(w, True, lambda blk: (blk.lits(b"z"), blk.match(258, 32768), blk.match(100, 25000)))
    out.append(("distances into a stored unit longer than 32 KiB", w.data(), bytes(w.out), 3))
    return out


def failing_streams():
    """[(what, raw stream, status the serial decoder ends with)] -- err_off, units and the bytes in front come from Walk
    and from the batch decoder."""
    import deflate_corpus as dc
    import gzip_ref
    text = (dc.TEXT * 4)[:150]
    out = []
    w = dc.Writer()
    stored_block(w, text[:50])
    _dynamic(w, True, lambda blk: (blk.lits(b"abcde"), blk.match(4, 56), blk.lits(b"never")))
    out.append(("a distance one byte in front of the stream, behind a stored unit", w.data(), CORRUPT))
    w = dc.Writer()
    _dynamic(w, False, lambda blk: blk.lits(text[:40]))
    stored_block(w, text[40:80])
    stored_block(w, text[80:100], nlength=(~20 & 0xffff) ^ 0x0100)
    _fixed(w, b"tail", True)
    out.append(("a wrong NLEN at a header the chain reaches", w.data(), CORRUPT))
    w = dc.Writer()
    _dynamic(w, False, lambda blk: blk.lits(text[:40]))
    stored_block(w, text[40:140], final=True, cut=30)
    out.append(("a stored block cut short", w.data(), UNEXPECTED_EOF))
    w = dc.Writer()
    _dynamic(w, False, lambda blk: blk.lits(text[:40]))
    w.header(False, 0)
    w.align()
    w.put(0x1234, 16)
    w.put(0xed, 8)  # three bytes behind the header: LEN / NLEN do not fit
    out.append(("three bytes behind a stored header", w.data(), UNEXPECTED_EOF))
    return out


def gz_members():
    """The gzip file of the tests: text at level 6, a level-0 member (its first block is stored), 70 000 random bytes at
    level 6 -> [(member, plain)]."""
    import gzip_ref
    t = gzip_ref.text(120000, seed=33)
    r = gzip_ref.rand(70000, seed=9)
    return [(gzip_ref.member(t[:60000], 6), t[:60000]), (gzip_ref.member(t[60000:], 0), t[60000:]),
            (gzip_ref.member(r, 6), r)]
