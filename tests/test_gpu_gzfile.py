"""A gzip file of any members on the GPU: flate_hip_gzfile_index and flate_hip_gzfile_read against the walk of
tests/gzfile_ref.py (every array entry and every verdict word) and against zlib (the bytes), with host and device
pointers, at shifted addresses, with the size query, a capacity one byte short and guard bytes around `out`.  The
serial offsets of the history cases come from the batch decoder on the same member alone -- the yardstick, not the code
under test."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import gzfile_ref as ref
import gzip_ref as gz
import one_ref
from test_gpu_inflate_one import on_device
from util import flate

pytestmark = pytest.mark.gpu

DEVICE_PTRS = 1
GUARD = 0xA5
NONE = ref.NONE


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


def place(f, device, shift):
    if device:
        return on_device(f, shift)
    keep = np.frombuffer(b"\xee" * shift + bytes(f) + b"\xee", np.uint8).copy()
    return keep, keep.ctypes.data + shift


def index(eng, f, device=False, shift=0, ucap=None, mcap=None, query=False):
    """One call -> (rc, words, unit_bit, out_off, member_off, member_unit, n_candidates); words as Walk.index_words()."""
    n = len(f)
    keep, ptr = place(f, device, shift)
    ucap = n // 8 + 8 if ucap is None else ucap
    mcap = n // 18 + 8 if mcap is None else mcap
    t = [np.full(max(c, 1) + 1, 0xDEAD, np.uint64) for c in (ucap, ucap, mcap, mcap)]
    nu, nm, ob, nc = C.c_uint32(99), C.c_uint32(99), C.c_uint64(99), C.c_uint32(99)
    st, bad, eo, seo = C.c_int32(99), C.c_uint32(99), C.c_int64(99), C.c_int64(99)
    a = [None] * 4 if query else [x.ctypes.data for x in t]
    rc = eng._L.flate_hip_gzfile_index(eng._ctx, ptr if n else None, n, 0 if query else ucap, a[0], a[1],
                                       0 if query else mcap, a[2], a[3], C.byref(nu), C.byref(nm), C.byref(ob),
                                       C.byref(nc), C.byref(st), C.byref(bad), C.byref(eo), C.byref(seo),
                                       DEVICE_PTRS if device else 0)
    for x, c in zip(t, (ucap, ucap, mcap, mcap)):
        assert (x[c:] == 0xDEAD).all(), "an index array was written behind its capacity"
    words = (st.value, nu.value, nm.value, ob.value, bad.value, eo.value, seo.value)
    ku, km = nu.value + 1, nm.value + 1
    return (rc, words, [int(v) for v in t[0][:ku]], [int(v) for v in t[1][:ku]], [int(v) for v in t[2][:km]],
            [int(v) for v in t[3][:km]], nc.value)


def read(eng, f, cap, device=False, shift=0, out_shift=0, query=False, untouched_from=None):
    """One call into a 0xA5-prefilled buffer -> (rc, bytes, out_len, (status, bad_member, err_off, stream_err_off),
    n_members, n_units, buffer).  Nothing outside out[0, cap) may change; with device pointers nothing outside
    out[0, out_len) either -- or, untouched_from = T given (the one documented exception, "gzfile_serial_max" on and a
    failure that only TAIL finds), nothing at or behind out + T."""
    n = len(f)
    obuf = np.full(out_shift + cap + 64, GUARD, np.uint8)
    keep, ptr = place(f, device, shift)
    if device:
        import torch
        d_out = torch.from_numpy(obuf).cuda()
        out_ptr = d_out.data_ptr() + out_shift
    else:
        out_ptr = obuf.ctypes.data + out_shift
    ol, nm, nu, nc = C.c_uint64(99), C.c_uint32(99), C.c_uint32(99), C.c_uint32(99)
    st, bad, eo, seo = C.c_int32(99), C.c_uint32(99), C.c_int64(99), C.c_int64(99)
    rc = eng._L.flate_hip_gzfile_read(eng._ctx, ptr if n else None, n, None if query else out_ptr, 0 if query else cap,
                                      C.byref(ol), C.byref(nm), C.byref(nu), C.byref(nc), C.byref(st), C.byref(bad),
                                      C.byref(eo), C.byref(seo), DEVICE_PTRS if device else 0)
    if device:
        import torch
        torch.cuda.synchronize()
        obuf = d_out.cpu().numpy()
    assert (obuf[:out_shift] == GUARD).all() and (obuf[out_shift + cap:] == GUARD).all(), "guard bytes touched"
    body = obuf[out_shift:out_shift + cap]
    if ol.value <= cap and (device or rc not in (0, ref.OUT_TOO_SMALL)):
        lo = ol.value if untouched_from is None else untouched_from
        assert (body[lo:] == GUARD).all(), "bytes behind out_len touched"
    return (rc, body[:min(ol.value, cap)].tobytes(), ol.value, (st.value, bad.value, eo.value, seo.value), nm.value,
            nu.value, body)


def check_index(eng, what, f, w, **kw):
    rc, words, ub, oo, mo, mu, nc = index(eng, f, **kw)
    assert rc == w.status and words == w.index_words(), (what, kw, rc, words, w.index_words())
    assert ub == w.unit_bit and oo == w.out_off, (what, kw)
    assert mo == w.member_off and mu == w.member_unit, (what, kw, mo, w.member_off, mu, w.member_unit)
    assert nc >= w.n_units, (what, kw)
    rc, qwords, *_ = index(eng, f, query=True, **{k: v for k, v in kw.items() if k in ("device", "shift")})
    assert rc == w.status and qwords == words, (what, "the count query")
    return nc


def check_good(eng, what, f, plain, w, device=False, shift=0, out_shift=0):
    """Every check the corpus asks for on a file that reads cleanly."""
    assert w.status == 0 and w.out_bytes == len(plain), what
    nc = check_index(eng, what, f, w, device=device, shift=shift)
    good = (0, NONE, -1, -1)
    rc, got, ol, verdict, nm, nu, _ = read(eng, f, len(plain), device, shift, out_shift)
    assert (rc, ol, verdict, nm, nu) == (0, len(plain), good, w.n_members, w.n_units), (what, device, rc, ol, verdict)
    assert got == plain, (what, device)
    rc, _, ol, verdict, nm, nu, _ = read(eng, f, 0, device, shift, query=True)
    assert (rc, ol, nm, nu) == (ref.OUT_TOO_SMALL if plain else 0, len(plain), w.n_members, w.n_units), (what, "size query")
    if plain:
        rc, _, ol, _, _, _, body = read(eng, f, len(plain) - 1, device, shift, out_shift)
        assert (rc, ol) == (ref.OUT_TOO_SMALL, len(plain)) and (body == GUARD).all(), (what, "one byte short")
    return nc


@pytest.fixture(scope="module")
def phases():
    """(the 24 members, the file of all of them, its plain, its Walk): computed once, shared, never changed."""
    pm = ref.phase_members()
    f = b"".join(m for m, _ in pm)
    return pm, f, b"".join(p for _, p in pm), ref.Walk(f)


# ---- the corpus ----

def test_empty_file_is_zero_members(eng):
    for device in (False, True):
        rc, words, ub, oo, mo, mu, nc = index(eng, b"", device=device)
        assert (rc, words, ub, oo, mo, mu, nc) == (0, (0, 0, 0, 0, NONE, -1, -1), [0], [0], [0], [0], 0)
        rc, got, ol, verdict, nm, nu, _ = read(eng, b"", 16, device)
        assert (rc, got, ol, verdict, nm, nu) == (0, b"", 0, (0, NONE, -1, -1), 0, 0)


def test_final_blocks_at_all_eight_bit_phases(eng, phases):
    pm, f, plain, w = phases
    assert {b % 8 for b in w.end_bits} == set(range(8))
    units = [w.member_unit[i + 1] - w.member_unit[i] for i in range(24)]
    assert min(units) >= 2 and max(units) > min(units)
    assert b"".join(ref.members_of(f)) == plain
    for device in (False, True):
        check_good(eng, "24 members", f, plain, w, device=device, shift=3 if device else 0, out_shift=1)


def test_every_phase_in_front_of_a_member(eng, phases):
    pm = phases[0]
    for i in range(24):
        (a, pa), (b, pb) = pm[i], pm[(i + 1) % 24]
        f = a + b
        check_good(eng, "members %d and %d" % (i, (i + 1) % 24), f, pa + pb, ref.Walk(f), device=i % 2 == 0, shift=i % 5)


def test_first_blocks_and_tiny_members(eng):
    f, plain = ref.tiny_file()
    w = ref.Walk(f)
    assert w.n_members == 12 and b"".join(ref.members_of(f)) == plain
    for device in (False, True):
        check_good(eng, "first blocks and tiny members", f, plain, w, device=device, shift=int(device))


def test_a_long_member_between_runs_of_tiny_ones(eng):
    f, plain = ref.interleaved_file()
    w = ref.Walk(f)
    assert w.n_members == 17 and max(w.sizes) == 300000 and b"".join(ref.members_of(f)) == plain
    for device in (False, True):
        check_good(eng, "a long member between tiny ones", f, plain, w, device=device, shift=2 * int(device))


def test_member_boundaries_at_tile_edges(eng):
    for what, f, plain in ref.tile_edge_files():
        w = ref.Walk(f)
        assert b"".join(ref.members_of(f)) == plain, what
        for shift in (0, 1, 15):
            check_good(eng, what, f, plain, w, device=True, shift=shift, out_shift=shift)
    what, f, plain = ref.tile_edge_files()[0]
    check_good(eng, what, f, plain, ref.Walk(f))


def test_members_at_round_edges(eng, phases):
    """"one_round_units" = 4 on the bit-phase file: members start at the first, the last and a middle place of a round,
    and the window carried into a round that starts with a member is not that member's history."""
    pm, f, plain, w = phases
    places = {u % 4 for u in w.member_unit[:-1]}
    assert places == {0, 1, 2, 3}
    try:
        for units in (4, 1, 5):
            eng.set_option("one_round_units", units)
            for device in (False, True):
                rc, got, ol, verdict, nm, nu, _ = read(eng, f, len(plain), device, shift=1)
                assert (rc, ol, verdict, nm, nu) == (0, len(plain), (0, NONE, -1, -1), 24, w.n_units), (units, device)
                assert got == plain, (units, device)
    finally:
        eng.set_option("one_round_units", 4096)


def test_history_never_crosses_a_member(eng):
    legal_f, legal_plain, bad_f, m0, p0, illegal = ref.history_files()
    w = ref.Walk(legal_f)
    assert not w.far and w.n_members == 2
    for device in (False, True):
        check_good(eng, "a distance to the member's first byte", legal_f, legal_plain, w, device=device)
    # the yardstick: the batch decoder on the illegal stream alone
    data = np.frombuffer(illegal + b"\0" * 8, np.uint8).copy()
    out, ooff, olen, status, err = eng.inflate_batch(data, np.array([0, len(illegal)], np.uint64), [600], check=False)
    assert int(status[0]) == ref.CORRUPT and int(err[0]) > 0
    front = bytes(out[:int(olen[0])])
    wb = ref.Walk(bad_f)
    check_index(eng, "the index call keeps no history", bad_f, wb)
    assert wb.status == 0 and wb.far  # (the walk keeps no history: it notes the distance)
    for device in (False, True):
        rc, got, ol, verdict, nm, nu, body = read(eng, bad_f, len(legal_plain) + 64, device, shift=1)
        assert rc == ref.CORRUPT and verdict == (ref.CORRUPT, 1, len(m0), int(err[0])), (device, rc, verdict)
        assert nm == 1 and got == p0 + front and ol == len(p0) + len(front), device
        assert (body[ol:] == GUARD).all(), "a copy from the member in front"


def test_decoys_are_off_the_path(eng):
    for what, f, plain in ref.decoy_files():
        w = ref.Walk(f)
        assert b"".join(ref.members_of(f)) == plain, what
        nc = check_good(eng, what, f, plain, w, device=True, shift=1, out_shift=3)
        assert nc > w.n_units + w.n_members, what
        check_good(eng, what, f, plain, w)


def test_one_member_files_have_the_units_of_inflate_one_index(eng):
    for k in (one_ref.MANY_UNITS, 6, 7, 8, 10, 11):
        what, raw, plain = one_ref.good_streams()[k]
        hdr = dict(flg=gz.FNAME, name=b"one member") if k % 2 else {}
        f = ref.wrap(raw, plain, **hdr)
        hl = len(gz.header(**hdr))
        one = eng.inflate_one_index(ref.wrap(raw, plain), "gzip")
        rc, words, ub, oo, mo, mu, nc = index(eng, f, device=True)
        assert rc == 0 and one.rc == 0 and words[1:3] == (one.n_units, 1), what
        assert ub == [int(b) + 8 * hl for b in one.unit_bit] and oo == [int(o) for o in one.out_off], what
        assert mo == [0, len(f)] and mu == [0, one.n_units], what
        rc, got, ol, verdict, nm, nu, _ = read(eng, f, len(plain), device=True)
        assert (rc, got, nm, nu) == (0, plain, 1, one.n_units), what


def test_index_arrays_that_are_too_small(eng, phases):
    pm, f, plain, w = phases
    for ucap, mcap in ((w.n_units, w.n_members + 1), (w.n_units + 1, w.n_members), (1, 1)):
        rc, words, *_ = index(eng, f, ucap=ucap, mcap=mcap)
        assert rc == ref.OUT_TOO_SMALL and words == w.index_words(), (ucap, mcap)
    rc, words, ub, oo, mo, mu, _ = index(eng, f, ucap=w.n_units + 1, mcap=w.n_members + 1)
    assert rc == 0 and ub == w.unit_bit and mu == w.member_unit


def test_python_wrapper(eng, phases):
    pm, f, plain, w = phases
    ix = eng.gzfile_index(f)
    assert ix.rc == 0 and list(ix.unit_bit) == w.unit_bit and list(ix.member_off) == w.member_off
    assert list(ix.member_unit) == w.member_unit and list(ix.out_off) == w.out_off
    q = eng.gzfile_index(f, query=True)
    assert (q.n_units, q.n_members, q.out_bytes, q.unit_bit) == (w.n_units, 24, len(plain), None)
    out, r = eng.gzfile_read(f)
    assert r.rc == 0 and r.out_len == len(plain) and bytes(out[:r.out_len]) == plain and r.bad_member == NONE
    import torch
    d = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()
    out, r = eng.gzfile_read(d)
    assert r.rc == 0 and out.is_cuda and bytes(out[:r.out_len].cpu().numpy()) == plain
    ix = eng.gzfile_index(d, index_cap=3)
    assert ix.rc == ref.OUT_TOO_SMALL and ix.unit_bit is None and list(ix.member_unit) == w.member_unit


def test_bad_arguments_are_refused_before_any_hip_call(eng):
    L, ctx = eng._L, eng._ctx
    buf = np.zeros(64, np.uint8)
    a = [np.zeros(8, np.uint64) for _ in range(4)]
    p = [x.ctypes.data for x in a]
    w, u, m, st = C.c_uint64(7), C.c_uint32(7), C.c_uint32(7), C.c_int32(7)

    def ix(in_ptr=buf.ctypes.data, ub=p[0], oo=p[1], mo=p[2], mu=p[3], nu=C.byref(u), nm=C.byref(m), ob=C.byref(w),
           status=C.byref(st), flags=0):
        return L.flate_hip_gzfile_index(ctx, in_ptr, 64, 8, ub, oo, 8, mo, mu, nu, nm, ob, None, status, None, None, None, flags)

    for kw in (dict(in_ptr=None), dict(ub=None), dict(oo=None), dict(mo=None), dict(mu=None), dict(nu=None), dict(nm=None),
               dict(ob=None), dict(status=None), dict(flags=2), dict(flags=DEVICE_PTRS | 4)):
        assert ix(**kw) == -1, kw
    # (a host pointer under FLATE_HIP_DEVICE_PTRS would be read by a kernel: the refusals above never get that far)
    assert (u.value, m.value, w.value, st.value) == (7, 7, 7, 7)

    def rd(in_ptr=buf.ctypes.data, out=buf.ctypes.data, cap=64, ol=C.byref(w), status=C.byref(st), flags=0):
        return L.flate_hip_gzfile_read(ctx, in_ptr, 64, out, cap, ol, None, None, None, status, None, None, None, flags)

    for kw in (dict(in_ptr=None), dict(out=None), dict(ol=None), dict(status=None), dict(flags=2), dict(flags=8)):
        assert rd(**kw) == -1, kw
    assert (w.value, st.value) == (7, 7)
    assert ix() == ref.CORRUPT and rd() == ref.CORRUPT  # 64 zero bytes: no member can start at offset 0


# ---- failures ----

@pytest.fixture(scope="module")
def three():
    m = ref.three_members()
    f = b"".join(x for x, _ in m)
    w = ref.Walk(f)
    assert w.status == 0 and w.member_unit[2] - w.member_unit[1] >= 4
    return m, f, b"".join(p for _, p in m), w


def check_bad(eng, what, f, w, delivered, trailer=None):
    """A file that fails: the index call against the walk, the read's verdict, the delivered prefix byte for byte and
    nothing behind it.  trailer: (member, its offset, its length) of a chain that is good."""
    check_index(eng, what, f, w)
    check_index(eng, what, f, w, device=True, shift=1)
    for device in (False, True):
        rc, got, ol, verdict, nm, nu, body = read(eng, f, len(delivered) + 100, device, shift=int(device), out_shift=2)
        if trailer is None:
            want = (w.status, w.bad_member, w.err_off, w.stream_err_off)
            assert (rc, verdict, nm, nu) == (w.status, want, w.n_members, w.n_units), (what, device, rc, verdict, nm, nu)
        else:
            assert (rc, verdict) == (ref.CORRUPT, (ref.CORRUPT,) + trailer), (what, device, rc, verdict)
            assert (nm, nu) == (w.n_members, w.n_units), (what, device)
        assert ol == len(delivered) and got == delivered, (what, device, ol, len(delivered))
        assert (body[ol:] == GUARD).all(), (what, "bytes behind the failure changed")


def test_wrong_trailers(eng, three):
    m, f, plain, w = three
    for k in range(3):
        for what, at, bit in (("CRC-32", -8, 0x40), ("ISIZE", -4, 0x01)):
            end = w.member_off[k + 1]
            bad = bytearray(f)
            bad[end + at] ^= bit
            wb = ref.Walk(bytes(bad))
            assert wb.index_words() == w.index_words()  # the chain is good: the index call reads no trailer
            check_bad(eng, "a wrong %s in member %d" % (what, k), bytes(bad), wb, plain,
                      trailer=(k, w.member_off[k], w.member_off[k + 1] - w.member_off[k]))
    bad = bytearray(f)  # two wrong trailers: the first in file order is the verdict
    bad[w.member_off[3] - 8] ^= 1
    bad[w.member_off[2] - 1] ^= 1
    check_bad(eng, "two wrong trailers", bytes(bad), ref.Walk(bytes(bad)), plain,
              trailer=(1, w.member_off[1], w.member_off[2] - w.member_off[1]))


def test_bytes_behind_the_last_member(eng, three):
    m, f, plain, w = three
    for what, tail in (("one garbage byte", b"g"), ("eight zero bytes", b"\0" * 8)):
        wb = ref.Walk(f + tail)
        assert wb.index_words() == (ref.CORRUPT, w.n_units, 3, 0, 3, len(f), -1), what
        # the decoders read nothing of a file's last 8 bytes: the last member's stream may end inside them
        check_bad(eng, what, f + tail, wb, plain[:wb.out_len])


def test_cut_files(eng, three):
    m, f, plain, w = three
    a, ab = w.member_off[1], w.member_off[2]
    cases = [("cut inside the last member's stream", f[:ab + (len(f) - ab) // 2], ref.UNEXPECTED_EOF, 2),
             ("cut inside the last member's trailer", f[:-3], ref.UNEXPECTED_EOF, 2),
             ("cut inside the middle member's header", f[:a + 7], ref.CORRUPT, 1)]
    for what, cut, status, bad_member in cases:
        wb = ref.Walk(cut)
        assert (wb.status, wb.bad_member) == (status, bad_member), what
        assert wb.err_off == w.member_off[bad_member], what
        check_bad(eng, what, cut, wb, plain[:wb.out_len])


def test_a_reserved_flag_bit_in_the_middle_member(eng, three):
    m, f, plain, w = three
    bad = bytearray(f)
    bad[w.member_off[1] + 3] |= 0x20
    wb = ref.Walk(bytes(bad))
    assert wb.index_words() == (ref.CORRUPT, w.member_unit[1], 1, 0, 1, w.member_off[1], -1)
    check_bad(eng, "a reserved FLG bit", bytes(bad), wb, m[0][1])


def test_a_reserved_block_type_in_the_middle_members_third_unit(eng, three):
    m, f, plain, w = three
    u = w.member_unit[1] + 2
    bad = bytearray(f)
    bit = w.unit_bit[u] + 1  # BTYPE = 2 -> 3
    bad[bit >> 3] |= 1 << (bit & 7)
    wb = ref.Walk(bytes(bad))
    assert (wb.status, wb.bad_member, wb.err_off, wb.n_units) == (ref.CORRUPT, 1, w.member_off[1], u - 1)
    assert wb.stream_err_off > 0 and wb.out_len == w.out_off[u]
    check_bad(eng, "BTYPE = 3", bytes(bad), wb, plain[:wb.out_len])
