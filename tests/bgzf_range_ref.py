"""CPU model of flate_hip_bgzf_read_ranges (include/flate_hip.h, "BGZF random access"), shared by
tests/test_bgzf_range_model.py, tests/test_bgzf_ranges_abi.py, tests/test_gpu_bgzf_ranges.py and
tests/test_host_cpp_bgzf_ranges.py: positions, the validity of virtual offsets, the touched set, out_off, the statuses
and the order of the verdict, on top of the serial walk of tests/bgzf_ref.py and gzip's own reader.  Written from the
contract, with per-byte coverage where the library uses searches and scans.  Nothing here needs a GPU."""
import gzip

import numpy as np

import bgzf_ref as ref

POS_BYTES, POS_VIRTUAL = 0, 1
OK, INVALID, OUT_TOO_SMALL, CORRUPT = 0, -1, -2, -4
NONE32 = 0xffffffff
U64_MAX = (1 << 64) - 1


def virtual_pos(v, w):
    """p(v) of the virtual offset v over the walk w, or None: v is not valid."""
    c, u = v >> 16, v & 0xffff
    if c not in w.member_off:  # (n + 1 entries: the last is the end of the file)
        return None
    k = w.member_off.index(c)
    isize = w.out_off[k + 1] - w.out_off[k] if k < w.n_members else 0
    return w.out_off[k] + u if u <= isize else None


def locate(kind, b, e, w):
    """(b, e) in U of one range, or None: an invalid end point."""
    if kind == POS_VIRTUAL:
        pb, pe = virtual_pos(b, w), virtual_pos(e, w)
        return None if pb is None or pe is None or pb > pe else (pb, pe)
    return min(b, w.out_bytes), min(e, w.out_bytes)


def members_of(w, b, e):
    """The members with ISIZE > 0 whose output intersects [b, e), in file order."""
    return [k for k in range(w.n_members) if w.out_off[k] < w.out_off[k + 1] and w.out_off[k] < e and b < w.out_off[k + 1]] \
        if b < e else []


class Result:
    """What one call must come out as.  data: the delivered bytes; exact[r]: every byte of range r is specified (it is
    valid and touches no member with a status)."""
    pass


def read_ranges(f, kind, begin, end, out_cap=None, status=None):
    """The model.  status: {member index: its non-zero status} for files whose members fail (tests/bgzf_ref.py:
    failing_files); out_cap None: exactly what is needed."""
    f = bytes(f)
    status = status or {}
    R = Result()
    n_ranges = len(begin)
    R.n_members = R.n_decoded = 0
    R.bad_member, R.err_off = NONE32, -1
    R.out_off, R.range_status, R.data, R.exact = [0] * (n_ranges + 1), [0] * n_ranges, b"", [True] * n_ranges
    if kind not in (POS_BYTES, POS_VIRTUAL) or any(b > e for b, e in zip(begin, end)):
        R.rc = INVALID
        return R
    if n_ranges == 0:
        R.rc = OK
        return R
    w = ref.Walk(f)
    R.n_members = w.n_members
    if w.rc:
        R.rc, R.err_off, R.bad_member = w.rc, w.err_off, w.n_members
        R.range_status, R.exact = [CORRUPT] * n_ranges, [False] * n_ranges
        return R
    T = w.out_bytes
    where = [locate(kind, b, e, w) for b, e in zip(begin, end)]
    R.out_off = [0] + list(np.cumsum([0 if x is None else x[1] - x[0] for x in where], dtype=object))
    R.out_off = [int(x) for x in R.out_off]
    # the touched members, by coverage of the bytes themselves
    d = np.zeros(T + 2, np.int64)
    for x in where:
        if x is not None and x[0] < x[1]:
            d[x[0]] += 1
            d[x[1]] -= 1
    covered = np.cumsum(d)[:T] > 0
    touched = [k for k in range(w.n_members) if covered[w.out_off[k]:w.out_off[k + 1]].any()]
    R.touched = touched
    R.n_decoded = len(touched)
    any_invalid = any(x is None for x in where)
    R.range_status = [INVALID if x is None else OK for x in where]
    R.exact = [x is not None for x in where]
    if out_cap is not None and R.out_off[-1] > out_cap:
        R.rc = OUT_TOO_SMALL
        return R
    # U: gzip's own reader, member by member where some member fails (its slot of ISIZE bytes is unspecified)
    if status:
        parts = []
        for k, m in enumerate(w.members(f)):
            parts.append(gzip.decompress(m) if k not in status else b"\0" * (w.out_off[k + 1] - w.out_off[k]))
            assert len(parts[-1]) == w.out_off[k + 1] - w.out_off[k]
        U = b"".join(parts)
    else:
        U = gzip.decompress(f) if f else b""
    assert len(U) == T
    R.data = b"".join(U[x[0]:x[1]] for x in where if x is not None)
    for r, x in enumerate(where):
        if x is None or not status:
            continue
        for k in sorted(status):  # the first member with a status that the range touches, in file order
            if w.out_off[k] < w.out_off[k + 1] and w.out_off[k] < x[1] and x[0] < w.out_off[k + 1] and x[0] < x[1]:
                R.range_status[r], R.exact[r] = status[k], False
                break
    bad = [k for k in touched if k in status]
    if bad:
        R.rc, R.bad_member, R.err_off = status[bad[0]], bad[0], w.member_off[bad[0]]
    else:
        R.rc = INVALID if any_invalid else OK
    return R


# ---- range lists that sit on every edge ----

def byte_edge_ranges(w):
    """Ranges around every member boundary +-1, T, T + 1 and 2^64 - 1."""
    T = w.out_bytes
    pts = sorted({max(p + d, 0) for p in w.out_off for d in (-1, 0, 1)} | {T, T + 1, U64_MAX})
    rs = []
    for i, p in enumerate(pts):
        rs += [(p, p), (p, p + 1 if p < U64_MAX else p), (0, p), (p, U64_MAX)]
        if i + 1 < len(pts):
            rs.append((p, pts[i + 1]))
        if i + 3 < len(pts):
            rs.append((p, pts[i + 3]))
    return rs


def decoy_offsets(f, w):
    """Offsets that pass the member rule without being members of the chain."""
    return [p for p in range(len(f)) if p not in w.member_off and ref.member_total(f, p)]


def virtual_edge_points(f, w, max_members=None):
    """Virtual offsets: every (member_off[k], u) with u in {0, 1, ISIZE - 1, ISIZE, ISIZE + 1}, c inside a member, c at
    a decoy, c == in_len with u in {0, 1}.  Sorted numerically."""
    pts = set()
    ks = range(w.n_members) if max_members is None else range(min(w.n_members, max_members))
    for k in ks:
        isize = w.out_off[k + 1] - w.out_off[k]
        for u in (0, 1, isize - 1, isize, isize + 1):
            if 0 <= u <= 0xffff:
                pts.add(w.member_off[k] << 16 | u)
    for k in list(ks)[:7]:
        pts.add((w.member_off[k] + 1) << 16)
        pts.add((w.member_off[k] + 9) << 16 | 3)
    for p in decoy_offsets(f, w) if len(f) < 200000 else []:
        pts.add(p << 16)
        pts.add(p << 16 | 1)
    pts.add(len(f) << 16)
    pts.add(len(f) << 16 | 1)
    pts.add((len(f) + 1) << 16)
    return sorted(pts)


def virtual_edge_ranges(f, w, max_members=None):
    pts = virtual_edge_points(f, w, max_members)
    rs = []
    for i, p in enumerate(pts):
        rs += [(p, p), (0, p), (p, len(f) << 16)] if p <= len(f) << 16 else [(p, p), (0, p)]
        if i + 1 < len(pts):
            rs.append((p, pts[i + 1]))
        if i + 4 < len(pts):
            rs.append((p, pts[i + 4]))
    return rs


def valid_virtual_offsets(w, f):
    """Every valid virtual offset of a (small) file, ordered."""
    out = []
    for k in range(w.n_members):
        out += [w.member_off[k] << 16 | u for u in range(w.out_off[k + 1] - w.out_off[k] + 1)]
    out.append(len(f) << 16)
    return sorted(out)
