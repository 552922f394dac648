"""The seek index of a gzip file of any members on the CPU: the reference of flate_hip_gzfile_seek_index / _ranges.

The point rule with the member starts, the block numbers, the windows (zeros in front of a member), the index words,
the index check and the verdict order of the read, restated in Python over gzfile_ref.Walk and seek_ref --
csrc/gzfile_seek_rule.h says the same in C++, and tests/host_model/gzfile_seek_rule_model.cpp holds the two against
each other.  Bytes come from zlib (`plain`), never from the code under test."""
import bisect

import gzfile_ref as gzf
import gzip_ref as gz
import one_ref
import seek_ref as sk

SPAN_DEFAULT, SPAN_NONE, WINDOW, HEAD_WORDS = sk.SPAN_DEFAULT, sk.SPAN_NONE, sk.WINDOW, sk.HEAD_WORDS
MAGIC = int.from_bytes(b"FGZFSIDX", "little")
VERSION = 1
UNIT_BITS_MAX = sk.UNIT_BITS_MAX
OK, INVALID, OUT_TOO_SMALL, CORRUPT = 0, -1, -2, -4
NO_UNIT = sk.NO_UNIT
SPANS = (1, 4096, 40000, 100000, 0, SPAN_NONE)


def starts(w):
    """The units that start a member."""
    return list(w.member_unit[:w.n_members])


def points(w, span):
    """THE POINT RULE: unit 0, every member's first unit, and every unit that starts in another span of the output than
    the unit in front."""
    return sorted(set(sk.points(w.out_off, span)) | set(starts(w)))


def first_unit(w, k):
    """f(k)."""
    mu = starts(w)
    return mu[bisect.bisect_right(mu, k) - 1]


def block(w, pts, p):
    """The block of point p, or None: it starts a member."""
    u, mu = pts[p], starts(w)
    return None if u in mu else p - bisect.bisect_right(mu, u)


def rel(w, k):
    return w.out_off[k] - w.out_off[first_unit(w, k)]


def window(w, plain, u):
    """The 32 KiB of u's MEMBER in front of unit u; in front of the member: zeros."""
    lo, at = w.out_off[first_unit(w, u)], w.out_off[u]
    return (b"\0" * WINDOW + plain[lo:at])[-WINDOW:]


def windows(w, plain, pts):
    mu = set(starts(w))
    return b"".join(window(w, plain, u) for u in pts if u not in mu)


def partial(w, pts):
    """The window-bearing points with fewer than 32 KiB of their member in front."""
    mu = set(starts(w))
    return [u for u in pts if u not in mu and rel(w, u) < WINDOW]


def index_words(w, in_len, span):
    """The index of the file whose (good) Walk is w, as a list of 64-bit words."""
    span = span or SPAN_DEFAULT
    if w.n_units == 0:
        return [MAGIC, VERSION, in_len, 0, span, 0, 0, 0] + [0] * 8
    pts = points(w, span)
    head = [MAGIC, VERSION, in_len, w.out_off[-1], span, w.n_units, w.n_members, len(pts)] + [0] * 8
    return head + list(w.unit_bit) + list(w.out_off) + list(w.member_off) + list(w.member_unit) + pts


def windows_bytes(w, span):
    return (len(points(w, span)) - w.n_members) * WINDOW if w.n_units else 0


def split(words):
    """(unit_bit, out_off, member_off, member_unit, point_unit) of words that pass the count checks."""
    n, m = words[5], words[6]
    a = HEAD_WORDS
    cuts = [a, a + n + 1, a + 2 * (n + 1), a + 2 * (n + 1) + m + 1, a + 2 * (n + 1) + 2 * (m + 1), len(words)]
    return [words[x:y] for x, y in zip(cuts, cuts[1:])]


def index_ok(words, win_bytes, in_len):
    """gzfile_seek_index_ok."""
    if len(words) < HEAD_WORDS or words[0] != MAGIC or words[1] != VERSION or words[2] != in_len:
        return False
    T, span, n, m, np_ = words[3:8]
    if n == 0:
        return m == 0 and np_ == 0 and in_len == 0 and T == 0 and len(words) == HEAD_WORDS and win_bytes == 0
    if not (n < NO_UNIT and 1 <= m <= n and m <= np_ <= n and span >= 1):
        return False
    if len(words) != HEAD_WORDS + 2 * (n + 1) + 2 * (m + 1) + np_ or win_bytes != (np_ - m) * WINDOW:
        return False
    ub, oo, mo, mu, pu = split(words)
    if oo[0] != 0 or oo[n] != T or mo[0] != 0 or mo[m] != in_len or mu[0] != 0 or mu[m] != n:
        return False
    if any(b <= a for a, b in zip(ub, ub[1:])) or any(b < a for a, b in zip(oo, oo[1:])):
        return False
    if any(b <= a or b - a < 18 for a, b in zip(mo, mo[1:])) or any(b <= a or b > n for a, b in zip(mu, mu[1:])):
        return False
    for j in range(m):
        lo, hi, end_bit = mu[j], mu[j + 1], 8 * (mo[j + 1] - 8)
        if ub[lo] < 8 * (mo[j] + 10) or ub[hi - 1] >= end_bit:
            return False
        if any((ub[k + 1] if k + 1 < hi else end_bit) - ub[k] > UNIT_BITS_MAX for k in range(lo, hi)):
            return False
    rule = sorted(set(sk.points(oo, span)) | set(mu[:m]))
    return pu == rule


def violations(words, win_bytes, in_len):
    """One hand-made violation of every clause of verdict 1 -> [(what, words, windows_bytes, in_len)], for an index of
    at least three members, a middle member of at least three units, and a window."""
    T, span, n, m, np_ = words[3:8]
    ub, oo, mo, mu, pu = (HEAD_WORDS, HEAD_WORDS + n + 1, HEAD_WORDS + 2 * (n + 1), HEAD_WORDS + 2 * (n + 1) + m + 1,
                          HEAD_WORDS + 2 * (n + 1) + 2 * (m + 1))
    assert m >= 3 and np_ > m
    j = next(j for j in range(1, m) if words[mu + j + 1] - words[mu + j] >= 3)  # a member of several units
    f = words[mu + j]

    def put(at, v, base=None):
        w = list(words if base is None else base)
        w[at] = v
        return w

    # a window-bearing point moved to a neighbour that is none, or dropped for one
    p = next(p for p in range(np_) if words[pu + p] not in words[mu:mu + m])
    u = words[pu + p]
    other = next(k for k in (u + 1, u - 1) if 0 < k < n and k not in words[pu:pu + np_])
    moved = put(pu + p, other)
    moved[pu:pu + np_] = sorted(moved[pu:pu + np_])
    huge = list(words)  # a unit longer than kSeekUnitBitsMax: everything behind it moved up, in_len with it
    shift = UNIT_BITS_MAX
    for k in range(f + 2, n + 1):
        huge[ub + k] += shift
    for k in range(j + 1, m + 1):
        huge[mo + k] += shift // 8
    huge[2] = in_len + shift // 8
    return [
        ("magic", put(0, MAGIC ^ 1), win_bytes, in_len),
        ("version", put(1, VERSION + 1), win_bytes, in_len),
        ("in_len is not the call's", words, win_bytes, in_len + 1),
        ("one word short", words[:-1], win_bytes, in_len),
        ("one word more", list(words) + [0], win_bytes, in_len),
        ("windows one byte short", words, win_bytes - 1, in_len),
        ("windows one block more", words, win_bytes + WINDOW, in_len),
        ("the point count", put(7, np_ + 1), win_bytes, in_len),
        ("no unit, but members", put(5, 0), win_bytes, in_len),
        ("no member", put(6, 0), win_bytes, in_len),
        ("more members than units", put(6, n + 1), win_bytes, in_len),
        ("fewer points than members", put(7, m - 1), win_bytes, in_len),
        ("span 0", put(4, 0), win_bytes, in_len),
        ("unit_bit repeats", put(ub + f + 2, words[ub + f + 1]), win_bytes, in_len),
        ("out_off decreases", put(oo + f + 2, words[oo + f + 1] - 1), win_bytes, in_len),
        ("out_off does not start at 0", put(oo, 1), win_bytes, in_len),
        ("out_off does not end at T", put(3, T + 1), win_bytes, in_len),
        ("member_off repeats", put(mo + 2, words[mo + 1]), win_bytes, in_len),
        ("member_off does not start at 0", put(mo, 1), win_bytes, in_len),
        ("member_off does not end at in_len", put(mo + m, in_len - 1), win_bytes, in_len),
        ("member_unit repeats", put(mu + 2, words[mu + 1]), win_bytes, in_len),
        ("member_unit does not start at 0", put(mu, 1), win_bytes, in_len),
        ("member_unit does not end at n", put(mu + m, n - 1), win_bytes, in_len),
        ("a first unit inside its member's header", put(ub + f, 8 * (words[mo + j] + 10) - 1), win_bytes, in_len),
        ("a last unit inside its member's trailer", put(mo + j + 1, (words[ub + words[mu + j + 1] - 1] >> 3) + 8),
         win_bytes, in_len),
        ("a unit of more than 2^28 bytes", huge, win_bytes, in_len + shift // 8),
        ("a point that the rule does not make", moved, win_bytes, in_len),
        ("a member start that is no point", put(mu + j, f + 1), win_bytes, in_len),
    ]


def decoded(w, pts, ranges):
    """The union over the non-empty ranges of [pstart(first), last]: the union over the touched units k of
    [pstart(k), k] and, between two touched units of one range, the units that produce no output -- an empty member is
    a segment of its own, which no touched unit names."""
    dec = set()
    for begin, end in ranges:
        b, e, first, last = sk.locate(w.out_off, begin, end)
        if first is not None:
            dec.update(range(sk.pstart(pts, first), last + 1))
    strict = sk.decoded(w.out_off, pts, ranges)
    assert strict <= dec and all(w.out_off[k + 1] == w.out_off[k] for k in dec - strict)
    return dec


def read(w, plain, pts, begin, end, out_cap=None, unit_status=None, same_file=True):
    """The read's verdict behind verdict 1, in order: seek_ref.read's, with verdict 3 the members check and the
    decoded set above."""
    rc, off, status, nd, bad, data = sk.read(plain, w.out_off, pts, begin, end, out_cap, unit_status, same_stream=same_file)
    if len(begin) and same_file:
        nd = len(decoded(w, pts, list(zip(begin, end))))
    return rc, off, status, nd, bad, data


def edge_ranges(w, pts):
    """seek_ref's range list, extended by every member boundary +- 1 (ranges that cross members) -- before the list is
    reversed and repeated."""
    T = w.out_off[-1]
    base = sk.edge_ranges(w.out_off, pts)
    r = base[:len(base) // 2]
    for u in w.member_unit:
        at = w.out_off[u]
        lo, hi = max(at - 1, 0), min(at + 1, T)
        r += [(lo, at), (at, hi), (lo, hi), (max(at - 40000, 0), min(at + 40000, T))]
    return r + r[::-1]


def segments(n, pts):
    """[(first unit, units)] of every segment."""
    return [(p, e - p) for p, e in zip(pts, pts[1:] + [n])]


# ---- the corpus ----

def seek_file():
    """Small members, a 300 000-byte member of hundreds of units, an empty member and a stored one -> (file, plain)."""
    three = gzf.three_members()
    big = gz.text(300000, seed=21)
    s = gz.text(900, seed=3)
    parts = [three[0], (gzf.wrap(one_ref.deflate(big, 6, mem=1), big), big), (gz.member(b""), b""), three[1],
             (gz.stored(s), s), three[2]]
    return b"".join(m for m, _ in parts), b"".join(p for _, p in parts)
