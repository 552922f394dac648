"""The seek index of a gzip file of any members on the GPU: flate_hip_gzfile_seek_index (build) and
flate_hip_gzfile_ranges (read).  Bytes come from zlib (plain[b:e]); units and members from gzfile_ref.Walk; points,
blocks, windows, decoded sets and the verdict order from tests/gzfile_seek_ref.py; the status of the illegal stream from
the batch decoder on the same bytes -- never from the code under test."""
import ctypes as C

import numpy as np
import pytest

import gzfile_ref as gzf
import gzfile_seek_ref as R
import gzip_ref as gz
import one_ref
import seek_ref as sk
from test_gpu_inflate_one import on_device
from util import flate

pytestmark = pytest.mark.gpu

DEVICE_PTRS = 1
GUARD = 0xA5
GUARD_WORD = 0xA5A5A5A5A5A5A5A5
NONE = 0xffffffff
SPANS = R.SPANS
SHIFTS = (0, 1, 15)


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


class File:
    """A corpus file with its walk; points, words and windows of a span are computed once."""

    def __init__(self, what, f, plain):
        self.what, self.f, self.plain, self.w = what, bytes(f), bytes(plain), gzf.Walk(f)
        assert self.w.status == 0 and b"".join(gzf.members_of(f)) == plain, what
        self._at = {}

    def at(self, span):
        if span not in self._at:
            pts = R.points(self.w, span)
            self._at[span] = (pts, R.index_words(self.w, len(self.f), span), R.windows(self.w, self.plain, pts))
        return self._at[span]


@pytest.fixture(scope="module")
def corpus():
    """{name: File}: computed once, shared, never changed."""
    out = {"seek": File("seek_file", *R.seek_file()), "tiny": File("tiny_file", *gzf.tiny_file())}
    pm = gzf.phase_members()
    out["phases"] = File("phase_members", b"".join(m for m, _ in pm), b"".join(p for _, p in pm))
    legal_f, legal_plain = gzf.history_files()[:2]
    out["history"] = File("history_files, the legal one", legal_f, legal_plain)
    tm = gzf.three_members()
    out["three"] = File("three_members", b"".join(m for m, _ in tm), b"".join(p for _, p in tm))
    for i, (what, f, plain) in enumerate(gzf.tile_edge_files()):
        out["tile%d" % i] = File(what, f, plain)
    return out


def place(f, device, shift):
    if device:
        return on_device(f, shift)
    keep = np.frombuffer(b"\xee" * shift + bytes(f) + b"\xee", np.uint8).copy()
    return keep, keep.ctypes.data + shift


def build(eng, f, span, device=False, shift=0, wshift=0, words=0, room=0, query=False):
    """One build call into guarded buffers -> dict of everything it reports."""
    n = len(f)
    keep, ptr = place(f, device, shift)
    words = 0 if query else words
    room = 0 if query else room
    idx = np.full(words + 4, GUARD_WORD, np.uint64)
    wbuf = np.full(wshift + room + 64, GUARD, np.uint8)
    if device:
        import torch
        d_w = torch.from_numpy(wbuf).cuda()
        w_ptr = d_w.data_ptr() + wshift
    else:
        w_ptr = wbuf.ctypes.data + wshift
    iw, wb, nu, nm, npt = C.c_uint64(99), C.c_uint64(99), C.c_uint32(99), C.c_uint32(99), C.c_uint32(99)
    ob, nc, st, bm, eo, seo = C.c_uint64(99), C.c_uint32(99), C.c_int32(99), C.c_uint32(99), C.c_int64(99), C.c_int64(99)
    rc = eng._L.flate_hip_gzfile_seek_index(
        eng._ctx, ptr if n else None, n, span, None if query else idx.ctypes.data + 16, words, C.byref(iw),
        None if query else w_ptr, room, C.byref(wb), C.byref(nu), C.byref(nm), C.byref(npt), C.byref(ob), C.byref(nc),
        C.byref(st), C.byref(bm), C.byref(eo), C.byref(seo), DEVICE_PTRS if device else 0)
    assert rc != -3, "HIP_FAILURE in the build"
    if device:
        import torch
        torch.cuda.synchronize()
        wbuf = d_w.cpu().numpy()
    assert (idx[:2] == GUARD_WORD).all() and (idx[2 + words:] == GUARD_WORD).all(), "index guard words touched"
    assert (wbuf[:wshift] == GUARD).all() and (wbuf[wshift + room:] == GUARD).all(), "windows guard bytes touched"
    return dict(rc=rc, index=idx[2:2 + words], windows=wbuf[wshift:wshift + room], index_words=iw.value,
                windows_bytes=wb.value, n_units=nu.value, n_members=nm.value, n_points=npt.value, out_bytes=ob.value,
                n_candidates=nc.value, status=st.value, bad_member=bm.value, err_off=eo.value, stream_err_off=seo.value)


def check_build(eng, F, span, **kw):
    """The build equals the model: words, windows byte for byte, counts."""
    pts, want, wins = F.at(span)
    g = build(eng, F.f, span, words=len(want), room=len(wins), **kw)
    tag = (F.what, span, kw)
    assert (g["rc"], g["status"], g["bad_member"], g["err_off"], g["stream_err_off"]) == (0, 0, NONE, -1, -1), (tag, g["rc"], g["status"])
    assert (g["index_words"], g["windows_bytes"], g["n_units"], g["n_members"], g["n_points"], g["out_bytes"]) == \
        (len(want), len(wins), F.w.n_units, F.w.n_members, len(pts), len(F.plain)), tag
    assert [int(x) for x in g["index"]] == want, tag
    assert g["windows"].tobytes() == wins, tag


def read(eng, f, words, wins, begin, end, cap, device=False, shift=0, wshift=0, out_shift=0, query=False,
         windows_bytes=None):
    """One read call into a 0xA5-prefilled buffer -> (rc, out_off, range_status, n_decoded, bad_unit, out bytes)."""
    keep, ptr = place(f, device, shift)
    words = np.ascontiguousarray(words, np.uint64)
    wk, w_ptr = place(wins, device, wshift)
    begin, end = np.array(begin, np.uint64), np.array(end, np.uint64)
    nr = len(begin)
    obuf = np.full(out_shift + cap + 64, GUARD, np.uint8)
    if device:
        import torch
        d_out = torch.from_numpy(obuf).cuda()
        out_ptr = d_out.data_ptr() + out_shift
    else:
        out_ptr = obuf.ctypes.data + out_shift
    off, status = np.full(nr + 1, 7, np.uint64), np.full(max(nr, 1), 7, np.int32)
    nd, bad = C.c_uint32(99), C.c_uint32(99)
    rc = eng._L.flate_hip_gzfile_ranges(
        eng._ctx, ptr if len(f) else None, len(f), words.ctypes.data, len(words), w_ptr if len(wins) else None,
        len(wins) if windows_bytes is None else windows_bytes, begin.ctypes.data, end.ctypes.data, nr,
        None if query else out_ptr, 0 if query else cap, off.ctypes.data, status.ctypes.data, C.byref(nd), C.byref(bad),
        DEVICE_PTRS if device else 0)
    assert rc != -3, "HIP_FAILURE in the read"
    if device:
        import torch
        torch.cuda.synchronize()
        obuf = d_out.cpu().numpy()
    assert (obuf[:out_shift] == GUARD).all() and (obuf[out_shift + cap:] == GUARD).all(), "guard bytes touched"
    return rc, [int(x) for x in off], [int(x) for x in status[:nr]], nd.value, bad.value, obuf[out_shift:out_shift + cap]


def check_read(eng, F, span, ranges, **kw):
    """The read equals the model: plain[b:e] back to back, the model's layout and n_decoded, nothing behind the total."""
    pts, words, wins = F.at(span)
    begin, end = [r[0] for r in ranges], [r[1] for r in ranges]
    rc_m, off_m, st_m, nd_m, bad_m, data_m = R.read(F.w, F.plain, pts, begin, end)
    cap = off_m[-1] + 32
    rc, off, st, nd, bad, body = read(eng, F.f, words, wins, begin, end, cap, **kw)
    assert (rc, off, st, nd, bad) == (rc_m, off_m, st_m, nd_m, bad_m), (F.what, span, kw, rc, nd, nd_m, bad)
    assert body[:off[-1]].tobytes() == b"".join(data_m), (F.what, span, kw)
    assert (body[off[-1]:] == GUARD).all(), "bytes behind the total touched"
    return nd


# ---- build ----

def test_build_equals_the_model_on_the_main_files(eng, corpus):
    for name in ("seek", "tiny", "phases", "history", "three"):
        for span in SPANS:
            for device in (False, True):
                for shift in SHIFTS:
                    check_build(eng, corpus[name], span, device=device, shift=shift, wshift=SHIFTS[(shift + 1) % 3])


def test_build_equals_the_model_at_tile_edges(eng, corpus):
    for i in range(14):
        for j, span in enumerate(SPANS):
            for shift in SHIFTS:
                check_build(eng, corpus["tile%d" % i], span, device=(i + j + shift) % 2 == 1, shift=shift, wshift=shift)


def test_build_in_rounds(eng, corpus):
    F = corpus["seek"]
    assert F.w.member_unit[2] - F.w.member_unit[1] >= 200
    try:
        for units in (7, 1, 64):
            eng.set_option("one_round_units", units)
            for span in (4096, 100000, 1) if units != 1 else (4096,):
                check_build(eng, F, span, device=True, shift=1, wshift=15)
            check_build(eng, corpus["tiny"], 1, shift=1)
    finally:
        eng.set_option("one_round_units", 4096)


def test_build_size_query_and_short_capacities(eng, corpus):
    F = corpus["seek"]
    pts, want, wins = F.at(4096)
    counts = (len(want), len(wins), F.w.n_units, F.w.n_members, len(pts), len(F.plain))
    for device in (False, True):
        for kw in (dict(query=True), dict(words=len(want) - 1, room=len(wins)), dict(words=len(want), room=len(wins) - 1)):
            g = build(eng, F.f, 4096, device=device, **kw)
            assert (g["rc"], g["status"]) == (-2, 0), kw
            assert (g["index_words"], g["windows_bytes"], g["n_units"], g["n_members"], g["n_points"], g["out_bytes"]) == counts, kw
            assert (g["index"] == GUARD_WORD).all() and (g["windows"] == GUARD).all(), kw  # nothing written
    # refused before any HIP call
    src = np.frombuffer(F.f, np.uint8).copy()
    z64, z32, zi = C.c_uint64(0), C.c_uint32(0), C.c_int32(0)
    ok = [eng._ctx, src.ctypes.data, len(F.f), 0, None, 0, C.byref(z64), None, 0, C.byref(z64), C.byref(z32), C.byref(z32),
          C.byref(z32), C.byref(z64), None, C.byref(zi), None, None, None, 0]
    for at, v in ((5, 5), (8, 5), (19, 8), (19, 2), (6, None), (9, None), (10, None), (11, None), (12, None), (13, None),
                  (15, None), (1, None)):
        a = list(ok)
        a[at] = v
        assert eng._L.flate_hip_gzfile_seek_index(*a) == -1, at


def test_the_empty_file(eng):
    g = build(eng, b"", 4096, words=16, room=0)
    assert (g["rc"], g["status"], g["index_words"], g["windows_bytes"], g["n_units"], g["n_members"], g["n_points"]) == \
        (0, 0, 16, 0, 0, 0, 0)
    want = R.index_words(gzf.Walk(b""), 0, 4096)
    assert [int(x) for x in g["index"]] == want and R.index_ok(want, 0, 0)
    assert build(eng, b"", 4096, query=True)["rc"] == -2
    rc, off, st, nd, bad, body = read(eng, b"", want, b"", [0, 5], [9, 5], 16)
    assert (rc, off, st, nd, bad) == (0, [0, 0, 0], [0, 0], 0, NONE) and (body == GUARD).all()


def check_no_index(eng, what, f, want):
    """A file that fails: (status, bad_member, err_off, stream_err_off) and no index."""
    for device in (False, True):
        g = build(eng, f, 4096, device=device, shift=int(device), words=4096, room=16 * R.WINDOW)
        got = (g["status"], g["bad_member"], g["err_off"], g["stream_err_off"])
        assert g["rc"] == want[0] != 0 and got == want, (what, device, g["rc"], got, want)
        assert (g["index_words"], g["windows_bytes"], g["n_points"], g["out_bytes"]) == (0, 0, 0, 0), what
        assert (g["index"] == GUARD_WORD).all(), what


def test_failing_files_get_the_walks_verdict_and_no_index(eng, corpus):
    F = corpus["three"]
    f, w = F.f, F.w
    a, ab = w.member_off[1], w.member_off[2]
    flag = bytearray(f)
    flag[a + 3] |= 0x20
    cases = [("cut inside the last member's stream", f[:ab + (len(f) - ab) // 2]),
             ("cut inside the last member's trailer", f[:-3]),
             ("cut inside the middle member's header", f[:a + 7]),
             ("a reserved FLG bit in the middle member", bytes(flag)),
             ("one garbage byte behind the last member", f + b"g"),
             ("eight zero bytes behind the last member", f + b"\0" * 8)]
    seen = set()
    for what, bad in cases:
        wb = gzf.Walk(bad)
        assert wb.status != 0, what
        check_no_index(eng, what, bad, (wb.status, wb.bad_member, wb.err_off, wb.stream_err_off))
        seen.add(wb.status)
    assert seen == {gzf.CORRUPT, gzf.UNEXPECTED_EOF}
    # a distance in front of its member: the walk keeps no history, TAIL finds it at the serial offset
    legal_f, legal_plain, bad_f, m0, p0, illegal = gzf.history_files()
    data = np.frombuffer(illegal + b"\0" * 8, np.uint8).copy()
    out, ooff, olen, status, err = eng.inflate_batch(data, np.array([0, len(illegal)], np.uint64), [600], check=False)
    assert int(status[0]) == gzf.CORRUPT and int(err[0]) > 0
    wb = gzf.Walk(bad_f)
    assert wb.status == 0 and wb.far
    check_no_index(eng, "history_files' illegal stream as the second member", bad_f, (gzf.CORRUPT, 1, len(m0), int(err[0])))
    # a trailer that does not match is not judged
    wrong = bytearray(f)
    wrong[ab - 8] ^= 1
    assert build(eng, bytes(wrong), 4096, words=4096, room=16 * R.WINDOW)["rc"] == 0


# ---- read ----

def test_read_every_edge_range_of_the_seek_file(eng, corpus):
    F = corpus["seek"]
    for j, span in enumerate(SPANS):
        ranges = R.edge_ranges(F.w, F.at(span)[0])
        check_read(eng, F, span, ranges, device=j % 2 == 1, shift=SHIFTS[j % 3], wshift=SHIFTS[(j + 1) % 3], out_shift=j % 3)
    ranges = R.edge_ranges(F.w, F.at(4096)[0])
    perm = np.random.default_rng(5).permutation(len(ranges))
    check_read(eng, F, 4096, [ranges[i] for i in perm], device=True, shift=1, wshift=1)
    check_read(eng, F, 4096, [ranges[i] for i in perm], shift=15, wshift=15, out_shift=1)


def test_read_every_edge_range_of_the_other_files(eng, corpus):
    for i, name in enumerate(n for n in corpus if n != "seek"):
        F = corpus[name]
        for j, span in enumerate(SPANS):
            if name.startswith("tile") and (i + j) % 3:  # a tile-edge file: two spans each, all six over the files
                continue
            ranges = R.edge_ranges(F.w, F.at(span)[0])
            check_read(eng, F, span, ranges, device=(i + j) % 2 == 1, shift=SHIFTS[(i + j) % 3], wshift=SHIFTS[i % 3])
            if span == 4096:
                perm = np.random.default_rng(i).permutation(len(ranges))
                check_read(eng, F, span, [ranges[k] for k in perm], device=(i + j) % 2 == 0, shift=1)


def test_one_byte_decodes_one_segment_prefix(eng, corpus):
    F = corpus["seek"]
    w = F.w
    for span in (4096, 40000, 100000, R.SPAN_NONE):
        pts = F.at(span)[0]
        k = sk.longest_segment_last(w.out_off, pts)
        at = w.out_off[k + 1] - 1
        nd = check_read(eng, F, span, [(at, at + 1)], device=True)
        assert nd == k - sk.pstart(pts, k) + 1 and nd < w.n_units


def test_partial_windows(eng, corpus):
    """A unit behind a point with fewer than 32 KiB of its member in front: the read is exact, and the stored block has
    zeros where U has the bytes of the member in front."""
    F = corpus["seek"]
    w = F.w
    pts, words, wins = F.at(4096)
    part = R.partial(w, pts)
    assert len(part) >= 10
    hit = 0
    for u in part:
        if R.first_unit(w, u) == 0:  # (nothing lies in front of the first member)
            continue
        p = pts.index(u)
        blk = wins[R.block(w, pts, p) * R.WINDOW:][:R.WINDOW]
        zeros = R.WINDOW - R.rel(w, u)
        in_front = sk.window(F.plain, w.out_off[u])  # what U has there
        assert blk[:zeros] == b"\0" * zeros and blk[zeros:] == in_front[zeros:] and in_front[:zeros].strip(b"\0")
        nxt = pts[p + 1] if p + 1 < len(pts) else w.n_units
        k = nxt - 1  # the last unit of the segment behind the partial point
        if w.out_off[k + 1] > w.out_off[k]:
            at = w.out_off[k + 1] - 1
            nd = check_read(eng, F, 4096, [(at, at + 1)], device=hit % 2 == 1, wshift=1)
            assert nd == k - u + 1
            hit += 1
    assert hit >= 5
    g = build(eng, F.f, 4096, device=True, words=len(words), room=len(wins))  # the device's own blocks say the same
    assert g["windows"].tobytes() == wins


def test_ranges_across_the_empty_and_the_stored_member(eng, corpus):
    F = corpus["seek"]
    w = F.w
    sizes = [w.out_off[w.member_unit[j + 1]] - w.out_off[w.member_unit[j]] for j in range(w.n_members)]
    assert sizes[2] == 0 and sizes[4] == 900
    e, s = w.out_off[w.member_unit[2]], w.out_off[w.member_unit[4]]
    ranges = [(e - 5, e + 5), (e, e + 1), (e - 1, e), (s - 3, s + 903), (s, s + 900), (s + 899, s + 901), (e - 70000, s + 950)]
    for span in SPANS:
        check_read(eng, F, span, ranges, device=span % 2 == 1, shift=1)


def test_rounds_cut_segments_and_carry_the_seed(eng, corpus):
    F = corpus["seek"]
    segs = lambda span: max(c for _, c in R.segments(F.w.n_units, F.at(span)[0]))
    assert segs(100000) == 81 and segs(R.SPAN_NONE) == 230
    try:
        for units in (7, 1, 64):
            eng.set_option("one_round_units", units)
            for span in (100000,) if units == 1 else (100000, R.SPAN_NONE, 4096):
                ranges = R.edge_ranges(F.w, F.at(span)[0])
                check_read(eng, F, span, ranges, device=True, shift=1, wshift=1)
    finally:
        eng.set_option("one_round_units", 4096)


def test_span_none_delivers_what_gzfile_read_delivers(eng, corpus):
    for name in ("seek", "tiny", "phases"):
        F = corpus[name]
        pts, words, wins = F.at(R.SPAN_NONE)
        assert wins == b"" and pts == R.starts(F.w)
        out, r = eng.gzfile_read(np.frombuffer(F.f, np.uint8))
        T = len(F.plain)
        rc, off, st, nd, bad, body = read(eng, F.f, words, wins, [0], [T], T)
        assert (rc, off, st, bad) == (0, [0, T], [0], NONE)
        assert r.rc == 0 and body.tobytes() == out[:r.out_len].tobytes() == F.plain


def test_a_one_member_file_has_the_index_of_inflate_one_seek_index(eng):
    for k in (one_ref.MANY_UNITS, 6, 10):
        what, raw, plain = one_ref.good_streams()[k]
        hdr = dict(flg=gz.FNAME, name=b"one member") if k % 2 else {}
        f = np.frombuffer(gzf.wrap(raw, plain, **hdr), np.uint8)
        hl = len(gz.header(**hdr))
        for span in (4096, R.SPAN_NONE):
            one = eng.inflate_one_seek_index(np.frombuffer(gzf.wrap(raw, plain), np.uint8), "gzip", span)
            s = eng.gzfile_seek_index(f, span)
            assert one.rc == 0 and s.rc == 0 and (s.n_units, s.n_members, s.n_points) == (one.n_units, 1, one.n_points), what
            n = s.n_units
            ub, oo, mo, mu, pu = R.split([int(x) for x in s.index])
            o = [int(x) for x in one.index[sk.HEAD_WORDS:]]
            assert [b - 8 * hl for b in ub] == o[:n + 1] and oo == o[n + 1:2 * (n + 1)] and pu == o[2 * (n + 1):], what
            assert (mo, mu) == ([0, len(f)], [0, n]) and s.windows.tobytes() == one.windows.tobytes(), what


# ---- verdicts ----

def test_every_clause_of_verdict_one_is_refused_on_a_ctx_that_works(eng, corpus):
    F = corpus["seek"]
    pts, words, wins = F.at(4096)
    for what, w2, wb, in_len in R.violations(words, len(wins), len(F.f)):
        assert not R.index_ok(w2, wb, in_len), what
        ff = F.f + b"\0" * min(max(in_len - len(F.f), 0), 64)  # (refused before a byte is read)
        keep, ptr = place(ff, False, 0)
        w2 = np.array(w2, np.uint64)
        wk = np.frombuffer(wins + b"\0" * R.WINDOW, np.uint8)
        b, e, off = np.array([0], np.uint64), np.array([10], np.uint64), np.zeros(2, np.uint64)
        obuf = np.zeros(64, np.uint8)
        rc = eng._L.flate_hip_gzfile_ranges(eng._ctx, ptr, in_len, w2.ctypes.data, len(w2), wk.ctypes.data, wb, b.ctypes.data,
                                            e.ctypes.data, 1, obuf.ctypes.data, 64, off.ctypes.data, None, None, None, 0)
        assert rc == -1, what
    assert read(eng, F.f, words, wins, [5], [4], 64)[0] == -1  # begin > end
    assert read(eng, F.f, words, wins, [0], [10], 64, windows_bytes=len(wins) - 1)[0] == -1
    rc, off, st, nd, bad, body = read(eng, F.f, words, wins, [0], [10], 64)  # the ctx still works
    assert (rc, off) == (0, [0, 10]) and body[:10].tobytes() == F.plain[:10]
    assert read(eng, F.f, words, wins, [], [], 64)[:2] == (0, [0])


def test_a_members_header_that_is_not_where_the_index_has_it(eng, corpus):
    F = corpus["seek"]
    pts, words, wins = F.at(4096)
    other = bytearray(F.f)
    other[F.w.member_off[3]] ^= 1  # the middle member's magic byte
    for device in (False, True):
        rc, off, st, nd, bad, body = read(eng, bytes(other), words, wins, [0, 7], [100, 9], 256, device=device)
        assert (rc, off, st, nd, bad) == (gzf.CORRUPT, [0, 0, 0], [gzf.CORRUPT] * 2, 0, NONE)
        assert (body == GUARD).all()


def test_the_same_headers_around_other_data(eng, corpus):
    """The long member's stream replaced, from its 31st unit on, by other bytes of the same length: every header is
    where the index has it, the units there no longer fit, every segment that did not fail is exact."""
    F = corpus["seek"]
    w = F.w
    span = 40000
    pts, words, wins = F.at(span)
    lo, hi = w.member_unit[1], w.member_unit[2]
    inside = [p for p in pts if lo < p < hi]
    k = inside[1] + 3  # inside a segment of the long member
    assert k not in pts and k + 2 < inside[2]
    other = bytearray(F.f)
    a, b = (w.unit_bit[k] >> 3) + 1, w.unit_bit[k + 1] >> 3
    other[a:b] = gz.rand(b - a, seed=9)
    oo = w.out_off
    ranges = [(0, oo[inside[1]]), (oo[inside[1]], oo[k]), (oo[k], oo[k] + 1), (oo[k + 2], oo[k + 2] + 9),
              (oo[inside[2]], oo[inside[2]] + 70000), (oo[hi] - 10, len(F.plain)), (oo[lo] - 5, oo[lo] + 5)]
    begin, end = [r[0] for r in ranges], [r[1] for r in ranges]
    for device in (False, True):
        rc, off, st, nd, bad, body = read(eng, bytes(other), words, wins, begin, end, sum(e - b for b, e in ranges), device=device)
        assert rc != 0 and bad == k and st[2] == rc, (rc, bad, st)
        model = R.read(w, F.plain, pts, begin, end, unit_status={k: rc})
        assert (off, nd) == (model[1], model[3])
        assert [s != 0 for s in st] == [s != 0 for s in model[2]], (st, model[2])
        assert [s != 0 for s in st][3:] == [True, False, False, False] and not st[0]
        for r, want in enumerate(model[5]):
            if want is not None:
                assert body[off[r]:off[r + 1]].tobytes() == want, r


def test_out_one_byte_short_and_the_size_query(eng, corpus):
    F = corpus["seek"]
    pts, words, wins = F.at(4096)
    begin, end = [10, 50000, 7], [20, 50100, 7]
    for device in (False, True):
        for kw in (dict(cap=109), dict(cap=0, query=True)):
            rc, off, st, nd, bad, body = read(eng, F.f, words, wins, begin, end, device=device, **kw)
            assert (rc, off) == (-2, [0, 10, 110, 110]) and (body == GUARD).all(), kw
    rc, off, st, nd, bad, body = read(eng, F.f, words, wins, [3], [3], 0, query=True)
    assert (rc, off, nd) == (0, [0, 0], 0)


def test_the_engine_wrappers(eng, corpus):
    F = corpus["seek"]
    f = np.frombuffer(F.f, np.uint8)
    pts, words, wins = F.at(4096)
    s = eng.gzfile_seek_index(f, 4096)
    assert (s.rc, s.n_units, s.n_members, s.n_points, s.out_bytes, s.status, s.bad_member, s.err_off, s.stream_err_off) == \
        (0, F.w.n_units, 6, len(pts), len(F.plain), 0, NONE, -1, -1)
    assert [int(x) for x in s.index] == words and s.windows.tobytes() == wins
    out, r = eng.gzfile_ranges(f, s, [5, 100000], [25, 100100])
    assert (r.rc, list(r.out_off), list(r.range_status), r.bad_unit) == (0, [0, 20, 120], [0, 0], NONE)
    assert out[:120].tobytes() == F.plain[5:25] + F.plain[100000:100100]
    import torch
    d = torch.from_numpy(f.copy()).cuda()
    s = eng.gzfile_seek_index(d, 40000)
    assert s.rc == 0 and s.windows.is_cuda and s.windows.cpu().numpy().tobytes() == F.at(40000)[2]
    T = len(F.plain)
    out, r = eng.gzfile_ranges(d, s, [T - 10], [1 << 40])
    assert r.rc == 0 and out.is_cuda and out[:10].cpu().numpy().tobytes() == F.plain[T - 10:]
    out, r = eng.gzfile_ranges(d, (s.index, s.windows), [3], [9], out=torch.zeros(64, dtype=torch.uint8, device="cuda"), out_cap=6)
    assert r.rc == 0 and out[:6].cpu().numpy().tobytes() == F.plain[3:9]
    half = f[:len(f) // 2]
    s, ix = eng.gzfile_seek_index(half, 4096), eng.gzfile_index(half, query=True)
    assert s.rc == s.status == ix.status != 0 and s.index is None and s.windows is None
    assert (s.bad_member, s.err_off, s.stream_err_off) == (ix.bad_member, ix.err_off, ix.stream_err_off)
    with pytest.raises(flate.FlateError):
        eng.gzfile_ranges(f, (np.zeros(16, np.uint64), None), [0], [1])
