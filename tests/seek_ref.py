"""The seek index of one long stream on the CPU: the reference of flate_hip_inflate_one_seek_index / _ranges.

The point rule, pstart, the touched and decoded sets, the output layout and the verdict order of the read, restated in
Python over one_ref.Walk (unit_bit / out_off) -- csrc/seek_index_rule.h says the same in C++, and
tests/host_model/seek_index_rule_model.cpp holds the two against each other.  Bytes come from zlib (`plain`)."""
import bisect
import struct
import zlib

import one_ref as ref

SPAN_DEFAULT, SPAN_NONE = 1 << 20, (1 << 64) - 1
WINDOW = 32768
HEAD_WORDS = 16
MAGIC = int.from_bytes(b"FONESIDX", "little")
VERSION = 1
UNIT_BITS_MAX = 8 << 28
OK, INVALID, OUT_TOO_SMALL, CORRUPT = 0, -1, -2, -4
NO_UNIT = 0xffffffff
U64 = (1 << 64) - 1


def points(out_off, span):
    """THE POINT RULE: unit 0, and every unit that starts in another span of the output than the unit in front."""
    span = span or SPAN_DEFAULT
    return [k for k in range(len(out_off) - 1) if k == 0 or out_off[k] // span > out_off[k - 1] // span]


def pstart(pts, k):
    return pts[bisect.bisect_right(pts, k) - 1]


def locate(out_off, begin, end):
    """(b, e, first, last): U[b, e) and the first / last unit with bytes inside it (None: the range is empty)."""
    T = out_off[-1]
    b, e = min(begin, T), min(end, T)
    if b >= e:
        return b, e, None, None
    return b, e, bisect.bisect_right(out_off, b) - 1, bisect.bisect_left(out_off, e) - 1


def touched(out_off, ranges):
    hit = set()
    for begin, end in ranges:
        b, e, first, last = locate(out_off, begin, end)
        if first is not None:
            hit.update(k for k in range(first, last + 1) if out_off[k + 1] > out_off[k])
    return hit


def decoded(out_off, pts, ranges):
    """The union over the touched units k of [pstart(k), k]."""
    dec = set()
    for k in touched(out_off, ranges):
        dec.update(range(pstart(pts, k), k + 1))
    return dec


def window(plain, at):
    """The 32 KiB in front of output position `at`, bytes in front of the stream 0."""
    return (b"\0" * WINDOW + plain)[at:at + WINDOW]


def windows(plain, out_off, pts):
    return b"".join(window(plain, out_off[u]) for u in pts[1:])


def trailer(plain, kind):
    """(want, isize) as frame_parse_kernel reads them."""
    if kind == ref.ZLIB:
        return zlib.adler32(plain), 0
    if kind == ref.GZIP:
        return zlib.crc32(plain), len(plain) & 0xffffffff
    return 0, 0


def index_words(w, plain, raw_len, kind, span):
    """The index of the stream whose Walk is w, inside container `kind`, as a list of 64-bit words."""
    span = span or SPAN_DEFAULT
    pts = points(w.out_off, span)
    want, isize = trailer(plain, kind)
    raw_off = ref.header_len(kind)
    in_len = len(ref.wrap(b"\0" * raw_len, plain, kind))
    head = [MAGIC, VERSION, kind, in_len, raw_off, raw_off + raw_len, w.out_off[-1], span, w.n_units, len(pts), want, isize,
            0, 0, 0, 0]
    return head + list(w.unit_bit) + list(w.out_off) + pts


def index_ok(words, windows_bytes, kind, in_len):
    """seek_index_ok."""
    if len(words) < HEAD_WORDS or words[0] != MAGIC or words[1] != VERSION or words[2] != kind or words[3] != in_len:
        return False
    raw_off, raw_end, T, span, n, np_ = words[4:10]
    if not (1 <= n < NO_UNIT and 1 <= np_ <= n and span >= 1):
        return False
    if len(words) != HEAD_WORDS + 2 * (n + 1) + np_ or windows_bytes != (np_ - 1) * WINDOW:
        return False
    if raw_off > raw_end or raw_end > in_len:
        return False
    ub = words[HEAD_WORDS:HEAD_WORDS + n + 1]
    oo = words[HEAD_WORDS + n + 1:HEAD_WORDS + 2 * (n + 1)]
    pu = words[HEAD_WORDS + 2 * (n + 1):]
    if ub[0] != 0 or oo[0] != 0 or oo[n] != T or ub[n] > 8 * (raw_end - raw_off):
        return False
    if any(b <= a or b - a > UNIT_BITS_MAX for a, b in zip(ub, ub[1:])) or any(b < a for a, b in zip(oo, oo[1:])):
        return False
    return pu == points(oo, span)


def violations(words, windows_bytes, kind, in_len):
    """One hand-made violation of every clause of verdict 1 -> [(what, words, windows_bytes, kind, in_len)], for an
    index of at least four units and two points."""
    n, np_ = words[8], words[9]
    assert n >= 4 and np_ >= 2
    ub, oo, pu = HEAD_WORDS, HEAD_WORDS + n + 1, HEAD_WORDS + 2 * (n + 1)

    def put(at, v):
        w = list(words)
        w[at] = v
        return w

    moved = list(words)  # a point moved to its neighbour unit: no longer the rule's set
    moved[pu + 1] = words[pu + 1] + 1 if words[pu + 1] + 1 < n and (np_ == 2 or words[pu + 2] > words[pu + 1] + 1) else words[pu + 1] - 1
    return [
        ("magic", put(0, MAGIC ^ 1), windows_bytes, kind, in_len),
        ("version", put(1, VERSION + 1), windows_bytes, kind, in_len),
        ("wrap is not the call's", words, windows_bytes, (kind + 1) % 3, in_len),
        ("in_len is not the call's", words, windows_bytes, kind, in_len + 1),
        ("one word short", words[:-1], windows_bytes, kind, in_len),
        ("one word more", list(words) + [0], windows_bytes, kind, in_len),
        ("windows one byte short", words, windows_bytes - 1, kind, in_len),
        ("windows one block more", words, windows_bytes + WINDOW, kind, in_len),
        ("the point count", put(9, np_ + 1), windows_bytes, kind, in_len),
        ("unit_bit repeats", put(ub + 2, words[ub + 1]), windows_bytes, kind, in_len),
        ("unit_bit does not start at 0", put(ub, 1), windows_bytes, kind, in_len),
        ("unit_bit ends behind the raw stream", put(ub + n, 8 * (words[5] - words[4]) + 1), windows_bytes, kind, in_len),
        ("the raw stream ends behind the input", put(5, in_len + 1), windows_bytes, kind, in_len),
        ("out_off decreases", put(oo + 2, words[oo + 1] - 1), windows_bytes, kind, in_len),
        ("out_off does not end at T", put(6, words[6] + 1), windows_bytes, kind, in_len),
        ("span 0", put(7, 0), windows_bytes, kind, in_len),
        ("a point that the rule does not make", moved, windows_bytes, kind, in_len),
    ]


def read(plain, out_off, pts, begin, end, out_cap=None, unit_status=None, same_stream=True):
    """The read's verdict behind verdict 1, in order -> (rc, out_off, range_status, n_decoded, bad_unit, bytes).
    unit_status: {unit: status} of decoded units that are not good; the bytes of a range whose status is not 0 are
    None (unspecified)."""
    nr = len(begin)
    if nr == 0:
        return OK, [0], [], 0, NO_UNIT, []
    if not same_stream:
        return CORRUPT, [0] * (nr + 1), [CORRUPT] * nr, 0, NO_UNIT, [None] * nr
    locs = [locate(out_off, b, e) for b, e in zip(begin, end)]
    off = [0]
    for b, e, _, _ in locs:
        off.append(off[-1] + e - b)
    dec = sorted(decoded(out_off, pts, list(zip(begin, end))))
    if out_cap is not None and off[-1] > out_cap:
        return OUT_TOO_SMALL, off, [0] * nr, len(dec), NO_UNIT, [None] * nr
    unit_status = unit_status or {}
    bad = [k for k in dec if unit_status.get(k, 0)]
    status, data = [], []
    for b, e, first, last in locs:
        st = 0
        if first is not None:
            st = next((unit_status[k] for k in range(pstart(pts, first), last + 1) if unit_status.get(k, 0)), 0)
        status.append(st)
        data.append(None if st else plain[b:e])
    return (unit_status[bad[0]] if bad else OK), off, status, len(dec), (bad[0] if bad else NO_UNIT), data


def edge_ranges(out_off, pts):
    """The range list of the read tests: everything, behind the end, empty ranges, every unit and point boundary +- 1,
    one byte in the last unit of the longest segment, duplicates, overlaps -- then the whole list again in reverse."""
    T = out_off[-1]
    r = [(0, T), (T + 1, U64), (0, 0), (T, T), (T // 2, T // 2)]
    for at in sorted(set(out_off)) + [out_off[u] for u in pts]:
        lo, hi = max(at - 1, 0), min(at + 1, T)
        r += [(lo, at), (at, hi), (lo, hi)]
    k = longest_segment_last(out_off, pts)
    if out_off[k + 1] > out_off[k]:
        r.append((out_off[k + 1] - 1, out_off[k + 1]))
    if T > 10:
        r += [(T // 3, T // 3 + 5), (T // 3, T // 3 + 5), (T // 3 + 2, min(T, T // 3 + 40000)), (T // 4, T // 2)]
    return r + r[::-1]


def longest_segment_last(out_off, pts):
    """The last unit of the longest segment."""
    n = len(out_off) - 1
    ends = pts[1:] + [n]
    length, p, e = max((e - p, p, e) for p, e in zip(pts, ends))
    return e - 1
