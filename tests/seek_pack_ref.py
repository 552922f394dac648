"""The packed windows of the seek index on the CPU: the reference of flate_hip_seek_windows_pack / _unpack and
flate_hip_inflate_one_ranges_packed.

The keep rule, the sparse windows, the empty-block rule, the pack index's words and the packed read's verdicts, restated
in Python -- csrc/seek_pack_rule.h says the same in C++, and tests/host_model/seek_pack_rule_model.cpp holds the two
against each other.  `copies` is a token walk on one_ref.Bits / Code / read_dynamic; bytes come from zlib (`plain`), the
blocks' streams from the oracle encoder, units and points from seek_ref."""
import bisect

import one_ref as ref
import seek_ref as sk

WINDOW = sk.WINDOW
HEAD_WORDS = 16
MAGIC = int.from_bytes(b"FONESWPK", "little")
VERSION = 1
COMPRESS, SPARSE = 1, 2
BIND = (3, 6, 7, 8, 12)  # the seek index's words the head binds to: in_len, T, span, n, the unit rule
OK, INVALID, OUT_TOO_SMALL, CORRUPT = 0, -1, -2, -4
FF = bytes([0, 255]) + bytes(254)


def copies(raw):
    """Every copy token of the raw stream in stream order -> [(q, length, dist)], q the output position it writes at."""
    r = ref.Bits(bytes(raw))
    out, total = [], 0
    while True:
        h = r.get(3)
        final, typ = h & 1, h >> 1
        assert typ != 3
        if typ == 0:
            p = (r.hw + 7) // 8
            ln = int.from_bytes(raw[p:p + 2], "little")
            total += ln
            r.pos = r.hw = 8 * (p + 4 + ln)
        else:
            if typ == 1:
                lit, dist = ref.FIXED
                lmin = 7
            else:
                lit, dist, ll = ref.read_dynamic(r)
                lmin = max(lit.min, ll[256])
            while True:
                s = r.sym(lit, lmin)
                if s < 256:
                    total += 1
                    continue
                if s == 256:
                    break
                ln = ref.LBASE[s - 257] + (r.get(ref.LEXT[s - 257]) if ref.LEXT[s - 257] else 0)
                d = r.sym(dist, dist.min)
                nb = (d - 2) >> 1 if d >= 4 else 0
                d = ref.DBASE[d] + (r.get(nb) if nb else 0)
                out.append((total, ln, d))
                total += ln
        if final:
            return out


def segment_fits(raw, start, end, seg_out, last):
    """MARK's verdict for a segment it walks whole: the blocks from bit `start` end exactly at bit `end` (last: with the
    final block) after exactly seg_out bytes, and no header, table or code on the way is bad."""
    raw = bytes(raw)
    r = ref.Bits(raw, start)
    total = 0
    try:
        while r.pos < end:
            h = r.get(3)
            final, typ = h & 1, h >> 1
            if typ == 3:
                return False
            if typ == 0:
                p = (r.hw + 7) // 8
                if len(raw) - p < 4:
                    return False
                ln, nl = int.from_bytes(raw[p:p + 2], "little"), int.from_bytes(raw[p + 2:p + 4], "little")
                if ln != (~nl & 0xffff) or len(raw) - p - 4 < ln:
                    return False
                total += ln
                r.pos = r.hw = 8 * (p + 4 + ln)
            else:
                if typ == 1:
                    lit, dist = ref.FIXED
                    lmin = 7
                else:
                    lit, dist, ll = ref.read_dynamic(r)
                    lmin = max(lit.min, ll[256])
                while True:
                    s = r.sym(lit, lmin)
                    if s < 256:
                        total += 1
                        continue
                    if s == 256:
                        break
                    if s >= 286:
                        return False
                    total += ref.LBASE[s - 257] + (r.get(ref.LEXT[s - 257]) if ref.LEXT[s - 257] else 0)
                    d = r.sym(dist, dist.min)
                    if d >= 30:
                        return False
                    if d >= 4:
                        r.get((d - 2) >> 1)
            if final:
                return last and r.pos == end and total == seg_out
    except ref.Stop:
        return False
    return not last and r.pos == end and total == seg_out


def keep(q, ln, dist, P0):
    """THE KEEP RULE for one copy: the window offsets [lo, hi) it keeps of the block in front of P0; (0, 0): none."""
    if not (P0 <= q < P0 + WINDOW) or not (1 <= dist <= WINDOW) or ln == 0:
        return 0, 0
    a_lo, a_hi = max(q - dist, 0, P0 - WINDOW), min(q - dist + ln, P0)
    if a_lo >= a_hi:
        return 0, 0
    return a_lo - (P0 - WINDOW), a_hi - (P0 - WINDOW)


def keep_masks(cps, out_off, pts):
    """Per block (point p >= 1): a bytearray of WINDOW flags, 1 = some copy of the segment's first 32 KiB reads it."""
    masks = []
    T = out_off[-1]
    qs = [c[0] for c in cps]
    for i, u in enumerate(pts[1:], 1):
        P0 = out_off[u]
        P1 = out_off[pts[i + 1]] if i + 1 < len(pts) else T
        m = bytearray(WINDOW)
        for q, ln, d in cps[bisect.bisect_left(qs, P0):bisect.bisect_left(qs, min(P1, P0 + WINDOW))]:
            lo, hi = keep(q, ln, d, P0)
            if hi > lo:
                m[lo:hi] = b"\1" * (hi - lo)
        masks.append(m)
    return masks


def sparse_windows(plain, out_off, pts, masks):
    """The blocks with every byte that is not kept set to zero -> [bytes]."""
    out = []
    for u, m in zip(pts[1:], masks):
        w = sk.window(plain, out_off[u])
        keep_ff = int.from_bytes(bytes(m).translate(FF), "little")
        out.append((int.from_bytes(w, "little") & keep_ff).to_bytes(WINDOW, "little"))
    return out


def blocks(plain, out_off, pts, mode, cps=None):
    """([the blocks as the mode stores them], kept_bytes)."""
    if mode & SPARSE:
        masks = keep_masks(cps, out_off, pts)
        return sparse_windows(plain, out_off, pts, masks), sum(sum(m) for m in masks)
    raw = [sk.window(plain, out_off[u]) for u in pts[1:]]
    return raw, len(raw) * WINDOW


def pack(blks, deflate):
    """(off, packed): THE EMPTY-BLOCK RULE -- a block of zeros has no bytes, every other is deflate(block)."""
    off, parts = [0], []
    for b in blks:
        s = b"" if not any(b) else bytes(deflate(b))
        parts.append(s)
        off.append(off[-1] + len(s))
    return off, b"".join(parts)


def pack_words(index, mode, off, kept):
    """The pack index of the seek index `index` (its words) as a list of 64-bit words."""
    head = [MAGIC, VERSION, mode, len(off) - 1, off[-1], kept] + [index[k] for k in BIND] + [0] * 5
    return head + list(off)


def pack_ok(words, packed_bytes, index):
    """seek_pack_ok."""
    if len(words) < HEAD_WORDS + 1 or words[0] != MAGIC or words[1] != VERSION or words[2] not in (COMPRESS, COMPRESS | SPARSE):
        return False
    nb = words[3]
    if len(words) != HEAD_WORDS + nb + 1 or words[4] != packed_bytes:
        return False
    if (words[5] > nb * WINDOW) if words[2] & SPARSE else (words[5] != nb * WINDOW):
        return False
    if any(words[11:16]):
        return False
    off = words[HEAD_WORDS:]
    if off[0] != 0 or off[-1] != packed_bytes or any(b < a for a, b in zip(off, off[1:])):
        return False
    return nb + 1 == index[9] and [words[6 + k] for k in range(5)] == [index[k] for k in BIND]


def violations(words, packed_bytes):
    """One hand-made violation of every clause of seek_pack_ok -> [(what, words, packed_bytes)], for a pack index of at
    least three blocks of which the second is not empty."""
    nb = words[3]
    assert nb >= 3 and words[HEAD_WORDS + 2] > words[HEAD_WORDS + 1]

    def put(at, v):
        w = list(words)
        w[at] = v
        return w

    return [
        ("magic", put(0, MAGIC ^ 1), packed_bytes),
        ("version", put(1, VERSION + 1), packed_bytes),
        ("mode 0", put(2, 0), packed_bytes),
        ("mode SPARSE alone", put(2, SPARSE), packed_bytes),
        ("mode 4", put(2, 4), packed_bytes),
        ("one block more than points", put(3, nb + 1), packed_bytes),
        ("one word short", words[:-1], packed_bytes),
        ("one word more", list(words) + [packed_bytes], packed_bytes),
        ("packed_bytes is not the call's", words, packed_bytes + 1),
        ("kept above the whole", put(5, nb * WINDOW + 1), packed_bytes),
        ("in_len is not the index's", put(6, words[6] + 1), packed_bytes),
        ("T is not the index's", put(7, words[7] + 1), packed_bytes),
        ("span is not the index's", put(8, words[8] + 1), packed_bytes),
        ("n is not the index's", put(9, words[9] + 1), packed_bytes),
        ("the unit rule is not the index's", put(10, words[10] ^ 1), packed_bytes),
        ("a reserved word", put(13, 1), packed_bytes),
        ("off does not start at 0", put(HEAD_WORDS, 1), packed_bytes),
        ("off decreases", put(HEAD_WORDS + 2, words[HEAD_WORDS + 1] - 1), packed_bytes),
        ("off does not end at packed_bytes", put(HEAD_WORDS + nb, packed_bytes - 1), packed_bytes),
    ]


def segment_stream(raw, unit_bit, pts, i, window):
    """Segment i (point pts[i] up to the next point) as a raw stream of its own -> (stream, zdict, skip): zlib, given
    zdict, inflates stream to skip bytes to throw away and then the segment's output.  The segment's bits are moved
    to the front but keep their position modulo 8 (a stored block pads to the stream's byte grid): in front of them
    stand empty fixed blocks of 10 bits and, for an odd position, one fixed block of 35 bits that copies 3 bytes at
    distance 32768 -- the dictionary is the window rotated by those 3 bytes, so that the 32 KiB in front of the
    segment are the window again.  Unless the segment holds the final block, an empty final fixed block ends it."""
    start = unit_bit[pts[i]]
    last = i + 1 == len(pts)
    end = unit_bit[pts[i + 1]] if not last else unit_bit[-1]
    acc = [0, 0]

    def put(v, nbits):
        acc[0] |= v << acc[1]
        acc[1] += nbits

    zdict, skip = window, 0
    if start & 1:
        put(2, 3)        # BFINAL 0, fixed
        put(64, 7)       # length symbol 257 (3 bytes): the code 0000001, first bit first
        put(23, 5)       # distance symbol 29: 11101
        put(8191, 13)    # its extra bits: 24577 + 8191 = 32768
        put(0, 7)        # end of block
        zdict, skip = window[-3:] + window[:-3], 3
    while (acc[1] - start) & 7:
        put(2, 3)
        put(0, 7)
    put((int.from_bytes(raw, "little") >> start) & ((1 << (end - start)) - 1), end - start)
    if not last:
        put(3, 3)        # BFINAL 1, fixed, end of block
        put(0, 7)
    return acc[0].to_bytes((acc[1] + 7) // 8, "little"), zdict, skip


def read(plain, out_off, pts, begin, end, bad_blocks=(), **kw):
    """The packed read's verdict behind verdict 1 -> seek_ref.read's tuple.  bad_blocks: the blocks whose stream does
    not inflate to 32768 bytes: block b makes unit pts[b + 1] a bad unit of status CORRUPT, if it is decoded."""
    return sk.read(plain, out_off, pts, begin, end, unit_status={pts[b + 1]: CORRUPT for b in bad_blocks}, **kw)
