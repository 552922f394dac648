"""Short members of a gzip file decoded WHOLE on the GPU: flate_hip_gzfile_index / flate_hip_gzfile_read with the
option "gzfile_serial_max" against the same calls with the option off (every result that must not change, word for
word and byte for byte) and against the model of tests/gzfile_serial_ref.py (the index arrays that do change, and
flate_hip_gzfile_last_route), on the gzfile corpus, its failing files and the mixed file; with host and device pointers,
shifted addresses inside guarded buffers, the size query, a capacity one byte short, the round sizes, the stored-unit
rule, the three decoders the whole-member batch can route to, and the seek-index calls, which ignore the option."""
import contextlib

import numpy as np
import pytest

import gzfile_ref as ref
import gzfile_serial_ref as sref
import test_gpu_gzfile as base
from test_gzfile_rule_model import corpus
from util import flate

pytestmark = pytest.mark.gpu

GUARD, NONE = base.GUARD, ref.NONE
SIZES = (20, 1000, 70000, sref.S_MAX)


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@contextlib.contextmanager
def options(eng, **kw):
    defaults = {"gzfile_serial_max": 0, "one_round_units": 4096, "one_stored_units": 0, "inflate_spec": 1,
                "inflate_simt_min_streams": 2049}
    try:
        for k, v in kw.items():
            eng.set_option(k, v)
        yield
    finally:
        for k in kw:
            eng.set_option(k, defaults[k])


def failing_files():
    """[(what, file)] beyond the corpus: wrong trailers in members that are whole, BTYPE = 3 in a unit."""
    m = ref.three_members()
    f = b"".join(x for x, _ in m)
    w = ref.Walk(f)
    out = []
    for k in range(3):
        for what, at, bit in (("CRC-32", -8, 0x40), ("ISIZE", -4, 0x01)):
            bad = bytearray(f)
            bad[w.member_off[k + 1] + at] ^= bit
            out.append(("a wrong %s in member %d" % (what, k), bytes(bad)))
    bad = bytearray(f)
    bit = w.unit_bit[w.member_unit[1] + 2] + 1  # BTYPE = 2 -> 3
    bad[bit >> 3] |= 1 << (bit & 7)
    out.append(("BTYPE = 3", bytes(bad)))
    return out


@pytest.fixture(scope="module")
def files(eng):
    """[(what, file, its walk, the option-0 read on device pointers, the option-0 candidate count)]: computed once,
    shared, never changed."""
    out = []
    for what, f in corpus() + failing_files() + [("the mixed file", sref.mixed_file()[0])]:
        w = ref.Walk(f)
        r0 = base.read(eng, f, w.out_len + 64, device=True)
        nc0 = base.index(eng, f, query=True)[6]
        out.append((what, f, w, r0, nc0))
    return out


def route(eng):
    return eng.gzfile_last_route()


def test_the_option_is_off_by_default_and_refuses_what_the_header_says(eng):
    f = sref.mixed_file()[0]
    base.index(eng, f, query=True)
    assert route(eng) == (0, 8, 0)
    for bad in (-1, 1 << 28, 1 << 40):
        with pytest.raises(flate.FlateError):
            eng.set_option("gzfile_serial_max", bad)
    for ok in (1, (1 << 28) - 1, 0):
        eng.set_option("gzfile_serial_max", ok)
    L, C = eng._L, base.C
    a, b, w = C.c_uint32(7), C.c_uint32(7), C.c_uint64(7)
    for args in ((None, C.byref(b), C.byref(w)), (C.byref(a), None, C.byref(w)), (C.byref(a), C.byref(b), None)):
        assert L.flate_hip_gzfile_last_route(eng._ctx, *args) == -1
    assert (a.value, b.value, w.value) == (7, 7, 7)


@pytest.mark.parametrize("S", SIZES)
def test_the_read_is_the_option_0_read_and_the_index_is_the_models(eng, files, S):
    seen = set()
    for k, (what, f, w, r0, nc0) in enumerate(files):
        m = sref.Model(f, S, w)
        with options(eng, gzfile_serial_max=S):
            # the index call against the model, host pointers
            rc, words, ub, oo, mo, mu, nc = base.index(eng, f)
            got_route = route(eng)
            assert rc == w.status and words == m.index_words(), (what, S, rc, words, m.index_words())
            assert ub == m.unit_bit and oo == m.out_off, (what, S, ub[-3:], m.unit_bit[-3:])
            assert mo == w.member_off and mu == m.member_unit, (what, S)
            assert got_route == (m.serial_members, m.unit_members, m.find_from if f else 0), (what, S, got_route)
            assert nc <= nc0, (what, S, nc, nc0)
            if f and m.find_from == len(f):
                assert nc == len(sref.table(f)), (what, S)
            # the read against the option-0 read, device pointers at a shifted address
            r = base.read(eng, f, w.out_len + 64, device=True, shift=k % 16, out_shift=(3 * k) % 16)
            assert route(eng) == got_route, (what, S)
        assert r[:5] == r0[:5], (what, S, r[0], r[2:5], r0[0], r0[2:5])  # rc, bytes, out_len, verdict, n_members
        if w.status or r0[0] == 0:  # (a failure TAIL finds numbers the units of ITS member)
            assert r[5] == m.n_units, (what, S, r[5], m.n_units)
        if w.n_members and all(m.whole) and m.find_from == len(f):
            seen.add("all whole")
        if m.serial_members and m.unit_members:
            seen.add("mixed")
        if w.status and m.serial_members:
            seen.add("whole in front of a failure")
    want = {20: set(), 1000: {"mixed"}, 70000: {"mixed", "whole in front of a failure", "all whole"},
            sref.S_MAX: {"whole in front of a failure", "all whole"}}[S]
    assert seen >= want, (S, seen)


def test_pointers_guards_the_size_query_and_a_capacity_one_byte_short(eng):
    f, plain, longs = sref.mixed_file()
    w = ref.Walk(f)
    m = sref.Model(f, 4096, w)
    assert m.serial_members == 6 and m.unit_members == 2 and 0 < m.find_from < len(f)
    good = (0, NONE, -1, -1)
    with options(eng, gzfile_serial_max=4096):
        for device, shift, out_shift in ((False, 0, 0), (False, 1, 3), (True, 0, 0), (True, 1, 1), (True, 15, 15),
                                         (True, 0, 15), (True, 15, 0)):
            rc, got, ol, verdict, nm, nu, _ = base.read(eng, f, len(plain), device, shift, out_shift)
            assert (rc, ol, verdict, nm, nu) == (0, len(plain), good, 8, m.n_units), (device, shift, out_shift)
            assert got == plain, (device, shift, out_shift)
            assert route(eng) == (6, 2, m.find_from)
        for device in (False, True):
            rc, _, ol, _, nm, nu, _ = base.read(eng, f, 0, device, query=True)
            assert (rc, ol, nm, nu) == (ref.OUT_TOO_SMALL, len(plain), 8, m.n_units), device
            rc, _, ol, _, _, _, body = base.read(eng, f, len(plain) - 1, device, out_shift=1)
            assert (rc, ol) == (ref.OUT_TOO_SMALL, len(plain)) and (body == GUARD).all(), device
            rc, words, ub, oo, mo, mu, nc = base.index(eng, f, device=device, shift=5 * int(device))
            assert (rc, ub, oo, mu) == (0, m.unit_bit, m.out_off, m.member_unit), device
        # arrays that are too small are refused with the counts, as with the option off
        rc, words, *_ = base.index(eng, f, ucap=m.n_units, mcap=9)
        assert rc == ref.OUT_TOO_SMALL and words == m.index_words()
    # every member whole: no bit-offset search at all
    with options(eng, gzfile_serial_max=sref.S_MAX):
        rc, got, ol, verdict, nm, nu, _ = base.read(eng, f, len(plain), True, 1, 1)
        assert (rc, got, nm, nu) == (0, plain, 8, 8) and route(eng) == (8, 0, len(f))
    # an empty file
    with options(eng, gzfile_serial_max=4096):
        rc, got, ol, verdict, nm, nu, _ = base.read(eng, b"", 16, True)
        assert (rc, got, ol, verdict, nm, nu) == (0, b"", 0, good, 0, 0) and route(eng) == (0, 0, 0)


@pytest.mark.parametrize("units", [1, 4, 5])
def test_round_sizes(eng, units):
    f, plain, _ = sref.mixed_file()
    pm = ref.phase_members()
    g, gp = b"".join(x for x, _ in pm), b"".join(p for _, p in pm)
    for what, data, want, S in (("mixed", f, plain, 4096), ("24 members", g, gp, 1000), ("24 members", g, gp, 2000)):
        m = sref.Model(data, S)
        with options(eng, gzfile_serial_max=S, one_round_units=units):
            for device in (False, True):
                rc, got, ol, verdict, nm, nu, _ = base.read(eng, data, len(want), device, shift=1)
                assert (rc, ol, verdict, nu) == (0, len(want), (0, NONE, -1, -1), m.n_units), (what, S, units, device)
                assert got == want, (what, S, units, device)


def test_stored_units_together_with_the_option(eng):
    """The two options compose: with "one_stored_units" the ordinary members have more units, the whole ones still one."""
    f, plain, _ = sref.mixed_file()
    t, tp = ref.tiny_file()
    for what, data, want, S in (("mixed", f, plain, 4096), ("first blocks and tiny members", t, tp, 400)):
        with options(eng, one_stored_units=1):
            rc0, w0, ub0, oo0, mo0, mu0, nc0 = base.index(eng, data)
        with options(eng, one_stored_units=1, gzfile_serial_max=S):
            rc, w1, ub, oo, mo, mu, nc = base.index(eng, data)
            sm, um, ff = route(eng)
            r = base.read(eng, data, len(want), device=True, shift=3, out_shift=5)
        assert rc == rc0 == 0 and mo == mo0 and w1[2:] == w0[2:] and nc <= nc0, what
        assert sm and um and sm + um == len(mo) - 1, (what, sm, um)
        assert set(ub[:-1]) <= set(ub0[:-1]) and set(oo) <= set(oo0) and [ub[u] for u in mu[:-1]] == [ub0[u] for u in mu0[:-1]]
        assert (r[0], r[1], r[3], r[4]) == (0, want, (0, NONE, -1, -1), len(mo) - 1), what


@pytest.mark.parametrize("opts", [dict(inflate_spec=0), dict(inflate_spec=2),
                                  dict(inflate_spec=0, inflate_simt_min_streams=1)])
def test_every_decoder_the_whole_member_batch_can_route_to(eng, opts):
    """One wavefront per member (the scalar walk), the sub-block decoder, one lane per member."""
    f, plain, _ = sref.mixed_file()
    t, tp = ref.tiny_file()
    pm = ref.phase_members()
    g, gp = b"".join(x for x, _ in pm), b"".join(p for _, p in pm)
    for what, data, want, S in (("mixed", f, plain, 4096), ("tiny", t, tp, sref.S_MAX), ("24 members", g, gp, sref.S_MAX)):
        m = sref.Model(data, S)
        with options(eng, gzfile_serial_max=S, **opts):
            for device, shift in ((False, 0), (True, 7)):
                rc, got, ol, verdict, nm, nu, _ = base.read(eng, data, len(want), device, shift, shift)
                assert (rc, ol, verdict, nu) == (0, len(want), (0, NONE, -1, -1), m.n_units), (what, opts, device)
                assert got == want, (what, opts, device)
                assert route(eng)[0] == m.serial_members


def test_the_seek_index_calls_ignore_the_option(eng):
    f, plain, _ = sref.mixed_file()
    begin, end = np.array([0, 900, 300000], np.uint64), np.array([50, 270000, len(plain)], np.uint64)
    sx0 = eng.gzfile_seek_index(f, span=65536)
    out0, r0 = eng.gzfile_ranges(f, sx0, begin, end)
    with options(eng, gzfile_serial_max=4096):
        sx = eng.gzfile_seek_index(f, span=65536)
        out, r = eng.gzfile_ranges(f, sx, begin, end)
    assert sx0.rc == sx.rc == 0 and (sx.index == sx0.index).all() and (np.asarray(sx.windows) == np.asarray(sx0.windows)).all()
    assert (sx.n_units, sx.n_members, sx.n_points, sx.n_candidates) == (sx0.n_units, sx0.n_members, sx0.n_points, sx0.n_candidates)
    assert r.rc == r0.rc == 0 and list(r.out_off) == list(r0.out_off)
    n = int(r.out_off[-1])
    assert bytes(out[:n]) == bytes(out0[:n]) == plain[0:50] + plain[900:270000] + plain[300000:]
