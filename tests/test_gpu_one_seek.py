"""The seek index of one long stream on the GPU: flate_hip_inflate_one_seek_index (build) and
flate_hip_inflate_one_ranges (read).  Bytes come from zlib (plain[b:e]); units, points, decoded sets and the verdict
order from tests/seek_ref.py over one_ref.Walk; the statuses of failing streams from the serial decoders on the same
bytes -- never from the code under test.  The corpus is tests/one_ref.py's."""
import ctypes as C

import numpy as np
import pytest

import one_ref as ref
import seek_ref as sk
from test_gpu_inflate_one import failing_streams, on_device
from util import STATUS_OF_ORACLE, flate

pytestmark = pytest.mark.gpu

DEVICE_PTRS = 1
GUARD = 0xA5
GUARD_WORD = 0xA5A5A5A5A5A5A5A5
KINDS = (ref.RAW, ref.ZLIB, ref.GZIP)
SPANS = (1, 4096, 40000, 100000, sk.SPAN_NONE)


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def good(oracle):
    """[(what, raw stream, plain, Walk)]: computed once, shared, never changed."""
    return [(w, r, p, ref.Walk(r)) for w, r, p in ref.good_streams(oracle)]


def stream_ptr(f, device, shift):
    if device:
        return on_device(f, shift)
    keep = np.frombuffer(b"\xee" * shift + bytes(f) + b"\xee", np.uint8).copy()
    return keep, keep.ctypes.data + shift


def build(eng, f, kind, span, device=False, shift=0, wshift=0, words=None, room=None, query=False):
    """One build call into guarded buffers -> (rc, index words or None, windows bytes or None, counts...)."""
    n = len(f)
    keep, ptr = stream_ptr(f, device, shift)
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
    iw, wb, nu, npt = C.c_uint64(99), C.c_uint64(99), C.c_uint32(99), C.c_uint32(99)
    ob, nc, st, eo = C.c_uint64(99), C.c_uint32(99), C.c_int32(99), C.c_int64(99)
    rc = eng._L.flate_hip_inflate_one_seek_index(
        eng._ctx, ptr if n else None, n, kind, span, None if query else idx.ctypes.data + 16, words, C.byref(iw),
        None if query else w_ptr, room, C.byref(wb), C.byref(nu), C.byref(npt), C.byref(ob), C.byref(nc), C.byref(st),
        C.byref(eo), DEVICE_PTRS if device else 0)
    assert rc != -3, "HIP_FAILURE in the build"
    if device:
        import torch
        torch.cuda.synchronize()
        wbuf = d_w.cpu().numpy()
    assert (idx[:2] == GUARD_WORD).all() and (idx[2 + words:] == GUARD_WORD).all(), "index guard words touched"
    assert (wbuf[:wshift] == GUARD).all() and (wbuf[wshift + room:] == GUARD).all(), "windows guard bytes touched"
    body = wbuf[wshift:wshift + room]
    return dict(rc=rc, index=idx[2:2 + words], windows=body, index_words=iw.value, windows_bytes=wb.value,
                n_units=nu.value, n_points=npt.value, out_bytes=ob.value, n_candidates=nc.value, status=st.value,
                err_off=eo.value)


def check_build(eng, raw, plain, w, what, kind, span, **kw):
    """The build equals the model: arrays = Walk's, points = the rule's, every window = the 32 KiB in front."""
    f = ref.wrap(raw, plain, kind)
    want = sk.index_words(w, plain, len(raw), kind, span)
    pts = sk.points(w.out_off, span)
    wins = sk.windows(plain, w.out_off, pts)
    g = build(eng, f, kind, span, words=len(want), room=len(wins), **kw)
    tag = (what, kind, span, kw)
    assert (g["rc"], g["status"], g["err_off"]) == (0, 0, -1), (tag, g["rc"], g["status"])
    assert (g["index_words"], g["windows_bytes"], g["n_units"], g["n_points"], g["out_bytes"]) == \
        (len(want), len(wins), w.n_units, len(pts), len(plain)), tag
    assert [int(x) for x in g["index"]] == want, tag
    assert g["windows"].tobytes() == wins, tag
    return np.array(want, np.uint64), wins


def read(eng, f, kind, words, wins, begin, end, cap, device=False, shift=0, wshift=0, out_shift=0, query=False,
         index_words=None, windows_bytes=None):
    """One read call into a 0xA5-prefilled buffer -> (rc, out_off, range_status, n_decoded, bad_unit, out bytes)."""
    keep, ptr = stream_ptr(f, device, shift)
    words = np.ascontiguousarray(words, np.uint64)
    wk, w_ptr = stream_ptr(wins, device, wshift)
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
    rc = eng._L.flate_hip_inflate_one_ranges(
        eng._ctx, ptr, len(f), kind, words.ctypes.data, len(words) if index_words is None else index_words,
        w_ptr if len(wins) else None, len(wins) if windows_bytes is None else windows_bytes, begin.ctypes.data,
        end.ctypes.data, nr, None if query else out_ptr, 0 if query else cap, off.ctypes.data, status.ctypes.data,
        C.byref(nd), C.byref(bad), DEVICE_PTRS if device else 0)
    assert rc != -3, "HIP_FAILURE in the read"
    if device:
        import torch
        torch.cuda.synchronize()
        obuf = d_out.cpu().numpy()
    assert (obuf[:out_shift] == GUARD).all() and (obuf[out_shift + cap:] == GUARD).all(), "guard bytes touched"
    return rc, [int(x) for x in off], [int(x) for x in status[:nr]], nd.value, bad.value, obuf[out_shift:out_shift + cap]


def check_read(eng, f, kind, plain, w, span, words, wins, ranges, **kw):
    """The read equals the model: plain[b:e] back to back, the model's layout and n_decoded, nothing behind the total."""
    pts = sk.points(w.out_off, span)
    begin, end = [r[0] for r in ranges], [r[1] for r in ranges]
    rc_m, off_m, st_m, nd_m, bad_m, data_m = sk.read(plain, w.out_off, pts, begin, end)
    cap = off_m[-1] + 32
    rc, off, st, nd, bad, body = read(eng, f, kind, words, wins, begin, end, cap, **kw)
    assert (rc, off, st, nd, bad) == (rc_m, off_m, st_m, nd_m, bad_m), (span, kw, rc, nd, nd_m, bad)
    assert body[:off[-1]].tobytes() == b"".join(data_m), (span, kw)
    assert (body[off[-1]:] == GUARD).all(), "bytes behind the total touched"
    return nd


# ---- the conditions that keep the corpus from going vacuous ----

def test_the_corpus_reaches_every_edge(good):
    w = good[ref.MANY_UNITS][3]
    sizes = [b - a for a, b in zip(w.out_off, w.out_off[1:])]
    assert w.n_units >= 200 and max(sizes) < 32768 // 20
    assert len(sk.points(w.out_off, 1)) == w.n_units
    assert len(sk.points(w.out_off, 4096)) >= 50
    pts = sk.points(w.out_off, 100000)
    assert max(b - a for a, b in zip(pts, pts[1:] + [w.n_units])) >= 64  # a seven-step segmented scan
    for k in (0, 1):  # units of more than 32 KiB: a window lies inside one unit
        wk = good[k][3]
        assert max(b - a for a, b in zip(wk.out_off, wk.out_off[1:])) > 32768
    assert good[7][3].n_units == 1 and good[8][3].n_units == 1 and len(good[10][2]) == 17 and good[11][2] == b""


# ---- build ----

def test_build_every_stream_in_every_container(eng, good):
    for k, (what, raw, plain, w) in enumerate(good):
        for j, span in enumerate(SPANS):
            kind = KINDS[(k + j) % 3]
            check_build(eng, raw, plain, w, what, kind, span)
    what, raw, plain, w = good[ref.MANY_UNITS]
    for kind in KINDS:
        check_build(eng, raw, plain, w, what, kind, 4096)
    check_build(eng, raw, plain, w, what, ref.GZIP, 0)  # the default span: 1 MiB, one point


def test_build_with_device_pointers_at_shifted_addresses(eng, good):
    for k in (0, 1, ref.MANY_UNITS, 6, 7, 10, 11):
        what, raw, plain, w = good[k]
        for shift in (0, 1, 3):
            check_build(eng, raw, plain, w, what, KINDS[shift % 3], (4096, 40000, 1)[shift % 3], device=True, shift=shift,
                        wshift=shift)
    what, raw, plain, w = good[ref.MANY_UNITS]
    check_build(eng, raw, plain, w, what, ref.ZLIB, 4096, shift=3, wshift=1)


def test_build_in_rounds(eng, good):
    what, raw, plain, w = good[ref.MANY_UNITS]
    try:
        for units in (7, 1, 64):
            eng.set_option("one_round_units", units)
            check_build(eng, raw, plain, w, what, ref.GZIP, 4096, device=True, shift=1, wshift=3)
    finally:
        eng.set_option("one_round_units", 4096)


def test_build_size_query_and_short_capacities(eng, good):
    what, raw, plain, w = good[ref.MANY_UNITS]
    f = ref.wrap(raw, plain, ref.GZIP)
    want = sk.index_words(w, plain, len(raw), ref.GZIP, 4096)
    pts = sk.points(w.out_off, 4096)
    counts = (len(want), (len(pts) - 1) * sk.WINDOW, w.n_units, len(pts), len(plain))
    for device in (False, True):
        for kw in (dict(query=True), dict(words=len(want) - 1, room=counts[1]), dict(words=len(want), room=counts[1] - 1)):
            g = build(eng, f, ref.GZIP, 4096, device=device, **kw)
            assert (g["rc"], g["status"]) == (-2, 0), kw
            assert (g["index_words"], g["windows_bytes"], g["n_units"], g["n_points"], g["out_bytes"]) == counts, kw
            assert (g["index"] == GUARD_WORD).all() and (g["windows"] == GUARD).all(), kw  # nothing written
    # refused before any HIP call
    src = np.frombuffer(f, np.uint8).copy()
    z64, z32, zi = C.c_uint64(0), C.c_uint32(0), C.c_int32(0)
    ok = [eng._ctx, src.ctypes.data, len(f), 2, 0, None, 0, C.byref(z64), None, 0, C.byref(z64), C.byref(z32), C.byref(z32),
          C.byref(z64), None, C.byref(zi), None, 0]
    for at, v in ((3, 3), (6, 5), (9, 5), (17, 8), (17, 2), (7, None), (10, None), (11, None), (15, None), (1, None)):
        a = list(ok)
        a[at] = v
        assert eng._L.flate_hip_inflate_one_seek_index(*a) == -1, at


def test_failing_streams_get_the_serial_verdict_and_no_index(eng, good, oracle):
    cases = failing_streams(good)
    off = np.zeros(len(cases) + 1, np.uint64)
    np.cumsum(np.array([len(r) for _, r in cases], dtype=np.uint64), out=off[1:])
    data = np.frombuffer(b"".join(r for _, r in cases) + b"\0" * 8, np.uint8).copy()
    caps = [ref.Walk(raw).out_len + 600 for _, raw in cases]
    out, ooff, olen, status, err = eng.inflate_batch(data, off, caps, check=False)
    seen = set()
    for k, (what, raw) in enumerate(cases):
        rc, want, _, eoff = oracle.inflate(raw, caps[k], full=True)  # the yardstick itself against the oracle
        assert (int(status[k]), int(err[k]), int(olen[k])) == (STATUS_OF_ORACLE[rc], eoff, len(want)), (what, rc, eoff)
        g = build(eng, raw, ref.RAW, 4096, device=k % 2 == 1, words=4096, room=128 * sk.WINDOW)
        want = (int(status[k]), int(status[k]), int(err[k]) if status[k] else -1)
        assert (g["rc"], g["status"], g["err_off"]) == want, (what, g)
        if status[k]:
            assert (g["index_words"], g["windows_bytes"], g["n_points"]) == (0, 0, 0), what
            assert (g["index"] == GUARD_WORD).all(), what
        seen.add(g["status"])
    assert seen >= {0, ref.CORRUPT, ref.UNEXPECTED_EOF}
    legal, plain, illegal = ref.history_pair()
    k = [r for _, r in cases].index(illegal)
    assert int(status[k]) == ref.CORRUPT and int(err[k]) > 0  # the history-dependent verdict is in the list
    # a trailer that does not match is not judged here
    what, raw, plain, w = good[ref.MANY_UNITS]
    f = bytearray(ref.wrap(raw, plain, ref.GZIP))
    f[-8] ^= 1
    g = build(eng, bytes(f), ref.GZIP, 4096, words=8192, room=128 * sk.WINDOW)
    assert (g["rc"], g["status"]) == (0, 0)
    for kind, st, eo in ((ref.RAW, ref.UNEXPECTED_EOF, -1), (ref.ZLIB, ref.CORRUPT, 0), (ref.GZIP, ref.CORRUPT, 0)):
        g = build(eng, b"", kind, 4096, words=64, room=0)
        assert (g["rc"], g["status"], g["err_off"], g["index_words"]) == (st, st, eo, 0), kind


# ---- read ----

@pytest.fixture(scope="module")
def built(eng, good):
    """{(k, span): (f, words, windows)} of the gzip members the read tests share, from the MODEL (the build tests hold
    the device's index against it)."""
    out = {}
    for k in (0, 1, ref.MANY_UNITS, 5, 6, 7, 8, 10, 11):
        what, raw, plain, w = good[k]
        for span in SPANS:
            words = sk.index_words(w, plain, len(raw), ref.GZIP, span)
            out[k, span] = (ref.wrap(raw, plain, ref.GZIP), np.array(words, np.uint64),
                            sk.windows(plain, w.out_off, sk.points(w.out_off, span)))
    return out


def test_read_every_edge_range(eng, good, built):
    for (k, span), (f, words, wins) in built.items():
        what, raw, plain, w = good[k]
        ranges = sk.edge_ranges(w.out_off, sk.points(w.out_off, span))
        check_read(eng, f, ref.GZIP, plain, w, span, words, wins, ranges, device=(k + span) % 2 == 1, shift=k % 4,
                   wshift=(k + 1) % 4, out_shift=k % 3)


def test_read_in_the_other_containers(eng, good):
    what, raw, plain, w = good[ref.MANY_UNITS]
    for kind in (ref.RAW, ref.ZLIB):
        words, wins = check_build(eng, raw, plain, w, what, kind, 40000, device=True)
        ranges = sk.edge_ranges(w.out_off, sk.points(w.out_off, 40000))
        check_read(eng, ref.wrap(raw, plain, kind), kind, plain, w, 40000, words, wins, ranges, device=True, shift=1, wshift=3)


def test_one_byte_decodes_one_segment_prefix(eng, good, built):
    what, raw, plain, w = good[ref.MANY_UNITS]
    for span in (4096, 40000, 100000):
        f, words, wins = built[ref.MANY_UNITS, span]
        pts = sk.points(w.out_off, span)
        k = sk.longest_segment_last(w.out_off, pts)
        at = w.out_off[k + 1] - 1
        nd = check_read(eng, f, ref.GZIP, plain, w, span, words, wins, [(at, at + 1)], device=True)
        assert nd == k - sk.pstart(pts, k) + 1 and nd < w.n_units


def test_rounds_cut_segments_and_carry_the_seed(eng, good, built):
    what, raw, plain, w = good[ref.MANY_UNITS]
    try:
        for units in (7, 1, 4096):
            eng.set_option("one_round_units", units)
            for span in (4096, 100000) if units == 1 else SPANS:
                f, words, wins = built[ref.MANY_UNITS, span]
                ranges = sk.edge_ranges(w.out_off, sk.points(w.out_off, span))
                check_read(eng, f, ref.GZIP, plain, w, span, words, wins, ranges, device=True, shift=1, wshift=1)
            f, words, wins = built[5, 40000]
            check_read(eng, f, ref.GZIP, good[5][2], good[5][3], 40000, words, wins, [(20000, 250000), (5, 6)], device=True)
    finally:
        eng.set_option("one_round_units", 4096)


def test_span_none_delivers_what_inflate_one_delivers(eng, good, built):
    for k in (1, ref.MANY_UNITS, 6):
        what, raw, plain, w = good[k]
        f, words, wins = built[k, sk.SPAN_NONE]
        assert wins == b""
        out, r = eng.inflate_one(np.frombuffer(f, np.uint8), "gzip")
        rc, off, st, nd, bad, body = read(eng, f, ref.GZIP, words, wins, [0], [len(plain)], len(plain))
        assert (rc, off, st, bad) == (0, [0, len(plain)], [0], sk.NO_UNIT)
        assert body.tobytes() == out[:r.out_len].tobytes() == plain
        assert nd == max(u for u in range(w.n_units) if w.out_off[u + 1] > w.out_off[u]) + 1


# ---- verdicts ----

def test_every_clause_of_verdict_one_is_refused_on_a_ctx_that_works(eng, good, built):
    what, raw, plain, w = good[ref.MANY_UNITS]
    f, words, wins = built[ref.MANY_UNITS, 4096]
    for what, w2, wb, kind, in_len in sk.violations([int(x) for x in words], len(wins), ref.GZIP, len(f)):
        assert not sk.index_ok(w2, wb, kind, in_len), what
        ff = f + b"\0" * (in_len - len(f))
        rc = read(eng, ff, kind, w2, wins + b"\0" * sk.WINDOW, [0], [10], 64, windows_bytes=wb)[0]
        assert rc == -1, what
    assert read(eng, f, ref.GZIP, words, wins, [5], [4], 64)[0] == -1  # begin > end
    assert read(eng, f, ref.GZIP, words, wins, [0], [10], 64)[0] == 0   # the ctx still works
    assert read(eng, f, ref.GZIP, words, wins, [], [], 64)[:2] == (0, [0])


def test_another_stream_of_the_same_length(eng, good, built):
    what, raw, plain, w = good[ref.MANY_UNITS]
    f, words, wins = built[ref.MANY_UNITS, 4096]
    other = bytearray(f)
    other[-8] ^= 1  # the same length, another trailer
    for device in (False, True):
        rc, off, st, nd, bad, body = read(eng, bytes(other), ref.GZIP, words, wins, [0, 7], [100, 9], 256, device=device)
        assert (rc, off, st, nd, bad) == (ref.CORRUPT, [0, 0, 0], [ref.CORRUPT] * 2, 0, sk.NO_UNIT)
        assert (body == GUARD).all()


def test_an_index_that_does_not_fit_the_stream(eng, good, built):
    """One interior unit_bit entry moved by one bit: the index stays sound by verdict 1, the unit in front no longer
    ends at a block boundary and the unit itself starts inside a header."""
    what, raw, plain, w = good[ref.MANY_UNITS]
    span = 40000
    f, words, wins = built[ref.MANY_UNITS, span]
    pts = sk.points(w.out_off, span)
    k = pts[3] + 5  # inside a segment: neither the unit nor the one in front is a point
    assert k - 1 not in pts and k not in pts and k + 3 < pts[4]
    bent = words.copy()
    bent[sk.HEAD_WORDS + k] += 1
    assert sk.index_ok([int(x) for x in bent], len(wins), ref.GZIP, len(f))
    oo = w.out_off
    ranges = [(0, oo[pts[3]]), (oo[pts[3]], oo[k - 1]), (oo[k - 1], oo[k]), (oo[k] + 1, oo[k] + 2), (oo[k + 3], oo[k + 3] + 9),
              (oo[pts[4]], oo[pts[4]] + 70000), (oo[pts[2]] + 1, oo[pts[5]] + 1), (oo[pts[5] + 2], len(plain))]
    begin, end = [r[0] for r in ranges], [r[1] for r in ranges]
    for device in (False, True):
        rc, off, st, nd, bad, body = read(eng, f, ref.GZIP, bent, wins, begin, end, sum(e - b for b, e in ranges), device=device)
        model = sk.read(plain, oo, pts, begin, end, unit_status={k - 1: st[2], k: -4})
        assert (off, nd, bad) == (model[1], model[3], k - 1), (off, nd, bad)
        assert rc == st[2] != 0
        assert [s != 0 for s in st] == [s != 0 for s in model[2]], (st, model[2])
        assert [s != 0 for s in st] == [False, False, True, True, True, False, True, False]
        for r, want in enumerate(model[5]):
            if want is not None:
                assert body[off[r]:off[r + 1]].tobytes() == want, r


def test_out_one_byte_short_and_the_size_query(eng, good, built):
    what, raw, plain, w = good[ref.MANY_UNITS]
    f, words, wins = built[ref.MANY_UNITS, 4096]
    begin, end = [10, 50000, 7], [20, 50100, 7]
    for device in (False, True):
        for kw in (dict(cap=109), dict(cap=0, query=True)):
            rc, off, st, nd, bad, body = read(eng, f, ref.GZIP, words, wins, begin, end, device=device, **kw)
            assert (rc, off) == (-2, [0, 10, 110, 110]) and (body == GUARD).all(), kw
    rc, off, st, nd, bad, body = read(eng, f, ref.GZIP, words, wins, [3], [3], 0, query=True)
    assert (rc, off, nd) == (0, [0, 0], 0)


def test_the_engine_wrappers(eng, good):
    what, raw, plain, w = good[ref.MANY_UNITS]
    f = np.frombuffer(ref.wrap(raw, plain, ref.GZIP), np.uint8)
    s = eng.inflate_one_seek_index(f, "gzip", 4096)
    pts = sk.points(w.out_off, 4096)
    assert (s.rc, s.n_units, s.n_points, s.out_bytes, s.status, s.err_off) == (0, w.n_units, len(pts), len(plain), 0, -1)
    assert [int(x) for x in s.index] == sk.index_words(w, plain, len(raw), ref.GZIP, 4096)
    assert s.windows.tobytes() == sk.windows(plain, w.out_off, pts)
    out, r = eng.inflate_one_ranges(f, s, [5, 100000], [25, 100100])
    assert (r.rc, list(r.out_off), list(r.range_status), r.bad_unit) == (0, [0, 20, 120], [0, 0], sk.NO_UNIT)
    assert out[:120].tobytes() == plain[5:25] + plain[100000:100100]
    import torch
    d = torch.from_numpy(f.copy()).cuda()
    s = eng.inflate_one_seek_index(d, "gzip", 40000)
    assert s.rc == 0 and s.windows.is_cuda and s.windows.cpu().numpy().tobytes() == \
        sk.windows(plain, w.out_off, sk.points(w.out_off, 40000))
    out, r = eng.inflate_one_ranges(d, s, [299990], [1 << 40])
    assert r.rc == 0 and out.is_cuda and out[:10].cpu().numpy().tobytes() == plain[299990:]
    half = f[:len(f) // 2]
    s, (_, one) = eng.inflate_one_seek_index(half, "gzip", 4096), eng.inflate_one(half, "gzip", out_cap=len(plain))
    assert s.rc == s.status == one.status != 0 and s.err_off == one.err_off and s.index is None and s.windows is None
