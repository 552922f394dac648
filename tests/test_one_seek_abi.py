"""The seek index's two calls on the CPU side: exported and listed, refused without a ctx before any device is touched,
and the Python model of the read (tests/seek_ref.py) -- the yardstick of the GPU tests -- delivers plain[b:e] for every
edge range of the corpus."""
import ctypes as C
from importlib import import_module

import pytest

import one_ref as ref
import seek_ref as sk
from util import flate

NAMES = ("flate_hip_inflate_one_seek_index", "flate_hip_inflate_one_ranges")


@pytest.fixture(scope="module")
def lib():
    flate.build()
    return import_module("moonbit-flate_amd._lib").load()


def test_both_symbols_are_exported_and_listed(lib):
    mod = import_module("moonbit-flate_amd._lib")
    for name in NAMES:
        assert hasattr(lib, name) and name in mod.EXPORTS and name in mod.SIGNATURES, name
    assert len(mod.SIGNATURES[NAMES[0]][1]) == 18 and len(mod.SIGNATURES[NAMES[1]][1]) == 18
    assert flate.SEEK_SPAN_DEFAULT == sk.SPAN_DEFAULT and flate.SEEK_SPAN_NONE == sk.SPAN_NONE
    assert hasattr(flate.FlateEngine, "inflate_one_seek_index") and hasattr(flate.FlateEngine, "inflate_one_ranges")


def test_each_refuses_a_null_ctx_before_it_touches_a_device(lib):
    buf = (C.c_uint8 * 4)(3, 0, 0, 0)
    idx = (C.c_uint64 * 32)()
    w64, w32, st = C.c_uint64(7), C.c_uint32(7), C.c_int32(7)
    rc = lib.flate_hip_inflate_one_seek_index(None, buf, 4, 0, 0, idx, 32, C.byref(w64), None, 0, C.byref(w64),
                                              C.byref(w32), C.byref(w32), C.byref(w64), None, C.byref(st), None, 0)
    assert rc == -1 and (w64.value, w32.value, st.value) == (7, 7, 7)  # nothing was written either
    lo, hi, off = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(1), (C.c_uint64 * 2)(9, 9)
    rc = lib.flate_hip_inflate_one_ranges(None, buf, 4, 0, idx, 32, None, 0, lo, hi, 1, buf, 4, off, None, None, None, 0)
    assert rc == -1 and list(off) == [9, 9]


def test_the_model_delivers_the_bytes_of_every_edge_range():
    for what, raw, plain in ref.good_streams():
        w = ref.Walk(raw)
        for span in (1, 4096, 40000, 100000, 0, sk.SPAN_NONE):
            pts = sk.points(w.out_off, span)
            assert pts[0] == 0 and pts == sorted(set(pts)) and all(sk.pstart(pts, k) <= k for k in range(w.n_units))
            ranges = sk.edge_ranges(w.out_off, pts)
            begin, end = [r[0] for r in ranges], [r[1] for r in ranges]
            rc, off, status, nd, bad, data = sk.read(plain, w.out_off, pts, begin, end)
            assert (rc, bad) == (0, sk.NO_UNIT) and status == [0] * len(ranges), (what, span)
            T = len(plain)
            assert data == [plain[min(b, T):min(e, T)] for b, e in ranges], (what, span)
            assert off == [sum(len(d) for d in data[:r]) for r in range(len(ranges) + 1)][:len(off)], (what, span)
            # the windows and the decoded set restart every segment from bytes zlib produced
            wins = sk.windows(plain, w.out_off, pts)
            assert len(wins) == (len(pts) - 1) * sk.WINDOW
            for p, u in enumerate(pts[1:]):
                at = w.out_off[u]
                assert wins[p * sk.WINDOW:(p + 1) * sk.WINDOW][-min(at, sk.WINDOW):] == plain[max(at - sk.WINDOW, 0):at]
            words = sk.index_words(w, plain, len(raw), ref.GZIP, span)
            assert sk.index_ok(words, len(wins), ref.GZIP, len(ref.wrap(raw, plain, ref.GZIP))), (what, span)
    # the verdict order: a foreign stream in front of the capacity, the capacity in front of the decode
    w = ref.Walk(ref.good_streams()[ref.MANY_UNITS][1])
    plain = ref.good_streams()[ref.MANY_UNITS][2]
    pts = sk.points(w.out_off, 4096)
    assert sk.read(plain, w.out_off, pts, [0], [10], out_cap=5, same_stream=False)[:3] == (sk.CORRUPT, [0, 0], [sk.CORRUPT])
    assert sk.read(plain, w.out_off, pts, [0], [10], out_cap=9)[:2] == (sk.OUT_TOO_SMALL, [0, 10])
    k = pts[2] + 1
    got = sk.read(plain, w.out_off, pts, [w.out_off[pts[2]], w.out_off[k + 1], 0], [w.out_off[k], len(plain), 5],
                  unit_status={k: -4})
    assert (got[0], got[2], got[4]) == (-4, [0, -4, 0], k) and got[5][0] == plain[w.out_off[pts[2]]:w.out_off[k]]
