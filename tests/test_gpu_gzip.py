"""Plain multi-member gzip files on the GPU: flate_hip_gzip_index and flate_hip_gzip_read.  Every expectation comes from
the CPU: tests/gzip_ref.py (the corpus, the walk restated over zlib's raw inflater, zlib's own gzip reader for the
bytes)."""
import ctypes as C

import numpy as np
import pytest

import gzip_ref as ref
from util import flate

pytestmark = pytest.mark.gpu

DEVICE_PTRS = 1
GUARD = 0xA5
NONE32 = 0xffffffff


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def good():
    """[(what, file, plain, Walk)]: computed once, shared, never changed."""
    return [(w, f, p, ref.Walk(f)) for w, f, p in ref.good_files()]


@pytest.fixture(scope="module")
def decoys():
    return [(w, f, p, more, ref.Walk(f)) for w, f, p, more in ref.decoy_files()]


def on_device(b, shift=0, pad=64):
    """bytes -> (keep-alive tensor, device pointer of the first byte): the file at byte `shift` of a larger tensor."""
    import torch
    t = torch.from_numpy(np.frombuffer(b"\xee" * shift + bytes(b) + b"\xee" * pad, np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + shift


def index(eng, f, n_members, device=False, shift=0, cap=None, query=False):
    """One flate_hip_gzip_index call -> (rc, n_members, out_bytes, n_candidates, err_off, member_off, out_off)."""
    n = len(f)
    keep, ptr = on_device(f, shift) if device else (np.frombuffer(b"\xee" * shift + bytes(f) + b"\xee", np.uint8).copy(), None)
    if not device:
        ptr = keep.ctypes.data + shift
    if cap is None:
        cap = n_members + 1
    moff, ooff = np.full(cap + 2, 7, np.uint64), np.full(cap + 2, 7, np.uint64)
    nm, ob, nc, eo = C.c_uint32(99), C.c_uint64(99), C.c_uint32(99), C.c_int64(99)
    rc = eng._L.flate_hip_gzip_index(eng._ctx, ptr if n else None, n, 0 if query else cap,
                                     None if query else moff.ctypes.data, None if query else ooff.ctypes.data,
                                     C.byref(nm), C.byref(ob), C.byref(nc), C.byref(eo), DEVICE_PTRS if device else 0)
    assert (moff[cap:] == 7).all() and (ooff[cap:] == 7).all(), "the arrays were written past index_cap"
    return rc, nm.value, ob.value, nc.value, eo.value, moff, ooff


def check_index(eng, f, w, what, **kw):
    """The call equals the walk w: verdict, counts and -- of a broken chain too -- the index of the good members."""
    rc, nm, ob, nc, eo, moff, ooff = index(eng, f, w.n_members, **kw)
    assert (rc, nm, ob, eo) == (w.rc, w.n_members, w.out_bytes, w.err_off), (what, kw)
    assert nc == w.n_candidates and nc >= nm, (what, kw, nc)
    assert list(moff[:nm + 1]) == w.member_off and list(ooff[:nm + 1]) == w.out_off, (what, kw)
    return nc


def read(eng, f, cap, device=False, shift=0, out_shift=0):
    """One flate_hip_gzip_read call into a prefilled buffer -> (rc, out bytes, out_len, n_members, bad_member, err_off,
    the whole buffer behind out_shift)."""
    n = len(f)
    obuf = np.full(out_shift + cap + 64, GUARD, np.uint8)
    if device:
        import torch
        keep, ptr = on_device(f, shift)
        d_out = torch.from_numpy(obuf).cuda()
        out_ptr = d_out.data_ptr() + out_shift
    else:
        keep = np.frombuffer(b"\xee" * shift + bytes(f) + b"\xee", np.uint8).copy()
        ptr, out_ptr = keep.ctypes.data + shift, obuf.ctypes.data + out_shift
    ol, nm, bad, eo = C.c_uint64(99), C.c_uint32(99), C.c_uint32(99), C.c_int64(99)
    rc = eng._L.flate_hip_gzip_read(eng._ctx, ptr if n else None, n, out_ptr, cap, C.byref(ol), C.byref(nm),
                                    C.byref(bad), C.byref(eo), DEVICE_PTRS if device else 0)
    if device:
        import torch
        torch.cuda.synchronize()
        obuf = d_out.cpu().numpy()
    assert (obuf[:out_shift] == GUARD).all() and (obuf[out_shift + cap:] == GUARD).all(), "guard bytes touched"
    body = obuf[out_shift:out_shift + cap]
    return rc, body[:min(ol.value, cap)].tobytes(), ol.value, nm.value, bad.value, eo.value, body


def check_read_good(eng, f, plain, w, what, **kw):
    rc, got, ol, nm, bad, eo, _ = read(eng, f, len(plain), **kw)
    assert (rc, ol, nm, bad, eo) == (0, len(plain), w.n_members, NONE32, -1), (what, kw)
    assert got == plain, (what, kw)


# ---- the corpus ----

def test_every_file_with_host_pointers(eng, good):
    for what, f, plain, w in good:
        assert w.rc == 0 and ref.plain_of(f) == plain, what
        check_index(eng, f, w, what)
        check_read_good(eng, f, plain, w, what)
    check_index(eng, good[2][1], good[2][3], "host buffer at an odd address", shift=3)
    check_read_good(eng, good[2][1], good[2][2], good[2][3], "host buffer at an odd address", shift=5, out_shift=1)


@pytest.mark.parametrize("part", range(4))
def test_every_file_at_every_device_alignment(eng, good, part):
    """The file at each of the 16 alignments inside a larger tensor (the tiles lie on the grid of the ADDRESS: every
    shift moves every member against them), the output between guard bytes at every alignment too."""
    for k, (what, f, plain, w) in enumerate(good):
        if k % 4 != part:
            continue
        for shift in range(16):
            check_index(eng, f, w, what, device=True, shift=shift)
            if len(f) < 20000 or shift % 5 == k % 5:
                check_read_good(eng, f, plain, w, what, device=True, shift=shift, out_shift=(3 * shift + k) % 16)


def test_decoys(eng, decoys):
    for k, (what, f, plain, more, w) in enumerate(decoys):
        assert w.rc == 0 and (w.n_candidates > w.n_members) == more, what
        for device in (False, True):
            for shift in ((0, 1, 9, 15) if device else (0,)):
                nc = check_index(eng, f, w, what, device=device, shift=shift)
                assert nc > w.n_members if more else nc == w.n_members, what
                check_read_good(eng, f, plain, w, what, device=device, shift=shift, out_shift=k)


def test_malformed_files(eng):
    try:
        for k, (what, f, m, rc, err_off, n_good) in enumerate(ref.malformed_files()):
            eng.set_option("gzip_member_max", m)
            w = ref.Walk(f, m)
            assert (w.rc, w.err_off, w.n_members) == (rc, err_off, n_good), what
            for device in (False, True):
                shift = (k + 1) % 16 if device else 0
                check_index(eng, f, w, what, device=device, shift=shift)
                got = index(eng, f, n_good, device=device, shift=shift, query=True)
                assert got[:3] + got[4:5] == (rc, n_good, 0, err_off), (what, device)
                # an array too small for the good prefix: the walk's verdict all the same, nothing written
                if n_good:
                    got = index(eng, f, n_good, device=device, shift=shift, cap=n_good)
                    assert got[:3] + got[4:5] == (rc, n_good, 0, err_off), (what, device)
                    assert (got[5] == 7).all() and (got[6] == 7).all(), what
                got = read(eng, f, 16384, device=device, shift=shift)
                assert got[0:1] + got[2:6] == (rc, 0, n_good, n_good, err_off), (what, device, got[:6])
                assert (got[6] == GUARD).all(), (what, "nothing may be written")
    finally:
        eng.set_option("gzip_member_max", ref.MEMBER_MAX)
    for bad in (0, 1 << 28, -1):
        with pytest.raises(flate.FlateError):
            eng.set_option("gzip_member_max", bad)


def test_the_good_prefix_of_a_broken_chain_can_be_salvaged(eng):
    what, f, m, rc, err_off, n_good = ref.malformed_files()[6]  # cut inside the third stream
    ix = eng.gzip_index(np.frombuffer(f, np.uint8))
    assert (ix.rc, ix.n_members, ix.err_off, ix.out_bytes) == (rc, n_good, err_off, 0) and n_good == 2
    out, ooff, olen, status = eng.inflate_batch_framed(np.frombuffer(f, np.uint8), ix.member_off, "gzip")
    assert not status.any() and (ooff == ix.out_off).all()
    assert out[:int(ooff[-1])].tobytes() == ref.text(9000, seed=21)[:6000]


def test_failing_members_on_a_sound_chain(eng):
    whole = ref.text(9000, seed=31)[:6500]
    for what, f, want_rc, want_bad in ref.failing_files():
        w = ref.Walk(f)
        for device in (False, True):
            check_index(eng, f, w, what, device=device, shift=2)  # the index is clean
            rc, got, ol, nm, bad, eo, _ = read(eng, f, w.out_bytes, device=device, shift=3)
            assert (rc, bad, eo) == (want_rc, want_bad, w.member_off[want_bad]), (what, device, rc, bad, eo)
            assert (ol, nm) == (w.out_bytes, w.n_members) and ol == len(whole), what
            lo, hi = w.out_off[want_bad], w.out_off[want_bad + 1]
            assert got[:lo] == whole[:lo] and got[hi:] == whole[hi:], what  # the other members are delivered


def test_capacity_and_queries(eng, good):
    what, f, plain, w = good[9]  # python gzip levels 1 6 9
    for device in (False, True):
        rc, _, ol, nm, bad, eo, body = read(eng, f, len(plain) - 1, device=device)
        assert (rc, ol, nm) == (-2, len(plain), w.n_members) and (body == GUARD).all(), device
        rc, _, ol, nm, bad, eo, body = read(eng, f, 0, device=device)  # the size query
        assert (rc, ol, nm) == (-2, len(plain), w.n_members), device
        got = index(eng, f, w.n_members, device=device, query=True)
        assert got[:5] == (0, w.n_members, len(plain), w.n_candidates, -1)
        # index_cap one entry short: the counts are set, the arrays untouched
        got = index(eng, f, w.n_members, device=device, cap=w.n_members)
        assert got[:3] == (-2, w.n_members, len(plain)) and (got[5] == 7).all() and (got[6] == 7).all()
    # an empty file: no members
    assert index(eng, b"", 0)[:5] == (0, 0, 0, 0, -1)
    assert index(eng, b"", 0, cap=0)[0] == -2
    assert read(eng, b"", 16)[:6] == (0, b"", 0, 0, NONE32, -1)
    # the optional out-parameters may be NULL; other flags are refused
    src = np.frombuffer(f, np.uint8)
    out, ol = np.zeros(len(plain), np.uint8), C.c_uint64()
    L = eng._L
    assert L.flate_hip_gzip_read(eng._ctx, src.ctypes.data, len(f), out.ctypes.data, len(plain), C.byref(ol), None, None,
                                 None, 0) == 0 and out.tobytes() == plain
    nm, ob = C.c_uint32(), C.c_uint64()
    assert L.flate_hip_gzip_index(eng._ctx, src.ctypes.data, len(f), 0, None, None, C.byref(nm), C.byref(ob), None, None,
                                  0) == 0 and (nm.value, ob.value) == (w.n_members, len(plain))
    one = np.zeros(4, np.uint64)
    assert L.flate_hip_gzip_index(eng._ctx, src.ctypes.data, len(f), 4, one.ctypes.data, None, C.byref(nm), C.byref(ob),
                                  None, None, 0) == -1  # one array without the other
    for flags in (2, 8, 9):
        assert L.flate_hip_gzip_index(eng._ctx, src.ctypes.data, len(f), 0, None, None, C.byref(nm), C.byref(ob), None,
                                      None, flags) == -1
        assert L.flate_hip_gzip_read(eng._ctx, src.ctypes.data, len(f), out.ctypes.data, len(plain), C.byref(ol), None,
                                     None, None, flags) == -1


# ---- the decoders behind the size-only pass ----

@pytest.mark.parametrize("option, value", [("inflate_spec", 0), ("inflate_spec_shape", 1), ("inflate_spec_shape", 2)])
def test_every_decoder_a_size_only_pass_can_route_to(eng, good, decoys, option, value):
    """`used` from inflate_kernel (the sub-block decoder switched off) and from both builds of inflate_spec_kernel."""
    default = {"inflate_spec": 1, "inflate_spec_shape": 0}[option]
    eng.set_option(option, value)
    try:
        for what, f, plain, w in good[2:] + [d[:3] + d[4:] for d in decoys]:
            check_index(eng, f, w, (what, option, value), device=True, shift=7)
        what, f, plain, w = good[8]
        check_read_good(eng, f, plain, w, (what, option, value), device=True)
        for what, f, m, rc, err_off, n_good in ref.malformed_files():
            if m == ref.MEMBER_MAX:
                check_index(eng, f, ref.Walk(f), (what, option, value), device=True, shift=1)
    finally:
        eng.set_option(option, default)


# ---- our own members, and the callers of frame_parse_kernel ----

EDGE_LENS = [0, 1, 16, 17, 127, 128, 129, 5552, 65534, 65535, 65536, 65537, 131070, 200000]


def test_round_trip_of_our_own_members(eng):
    """deflate_batch_framed("gzip") -> the members concatenated are a plain gzip file: gzip_read gives the input back
    without the side array, and gzip_index gives the side array."""
    lens = [EDGE_LENS[k % len(EDGE_LENS)] if k < 28 else (k * 37) % 301 for k in range(64)]
    fills = [ref.text, ref.rand]
    parts = [fills[k % 2](n, seed=100 + k) for k, n in enumerate(lens)]
    data = np.frombuffer(b"".join(parts), np.uint8)
    in_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    f, moff = eng.deflate_batch_framed(data, in_off, "gzip")
    f = bytes(f)
    assert ref.plain_of(f) == data.tobytes()
    for device in (False, True):
        rc, nm, ob, nc, eo, got_m, got_o = index(eng, f, 64, device=device, shift=11 if device else 0)
        assert (rc, nm, ob, eo) == (0, 64, len(data), -1) and nc >= 64
        assert (got_m[:65] == moff).all() and (got_o[:65] == in_off).all()
        rc, got, ol, nm, bad, eo, _ = read(eng, f, len(data), device=device, shift=4, out_shift=3)
        assert (rc, ol, nm, bad, eo) == (0, len(data), 64, NONE32, -1) and got == data.tobytes()


def test_framed_batch_read_is_unchanged_on_the_same_members(eng, good, decoys):
    """frame_parse_kernel now calls the shared rule: the framed gzip read over the members the index returns gives every
    member the status and the bytes the reference expects -- good members, and members whose trailer is wrong."""
    for what, f, plain, w in good[2:] + [d[:3] + d[4:] for d in decoys]:
        src = np.frombuffer(f, np.uint8)
        ix = eng.gzip_index(src)
        assert ix.rc == 0 and list(ix.member_off) == w.member_off and list(ix.out_off) == w.out_off, what
        out, ooff, olen, status = eng.inflate_batch_framed(src, ix.member_off, "gzip")
        assert not status.any() and (ooff == ix.out_off).all() and (np.diff(ix.out_off) == olen).all(), what
        assert out[:int(ooff[-1])].tobytes() == plain, what
    for what, f, want_rc, want_bad in ref.failing_files():
        src = np.frombuffer(f, np.uint8)
        ix = eng.gzip_index(src)
        _, _, _, status = eng.inflate_batch_framed(src, ix.member_off, "gzip", out_sizes=np.diff(ix.out_off))
        assert list(status) == [want_rc if i == want_bad else 0 for i in range(3)], what
    # members that are no members: a bad magic, reserved FLG bits, a file name without its NUL, too short for a trailer
    t = ref.text(300)
    m = ref.member(t, 6, flg=ref.FNAME, name=b"n")
    bad = [b"\x1f\x8b\x09" + m[3:], m[:3] + b"\x28" + m[4:], m[:10] + b"x" * (len(m) - 10), m[:19]]
    f = m + b"".join(bad) + m
    off = np.cumsum([0, len(m)] + [len(b) for b in bad] + [len(m)]).astype(np.uint64)
    _, _, olen, status = eng.inflate_batch_framed(np.frombuffer(f, np.uint8), off, "gzip", out_sizes=[300] * 6)
    assert list(status) == [0, -4, -4, -4, -4, 0] and list(olen) == [300, 0, 0, 0, 0, 300]


# ---- the Python interface ----

def test_engine_methods_on_numpy_and_cuda_tensors(eng, good, decoys):
    import torch
    what, f, plain, w = good[10]  # every header combination
    src = np.frombuffer(f, np.uint8)
    ix = eng.gzip_index(src)
    assert (ix.rc, ix.n_members, ix.out_bytes, ix.err_off) == (0, 16, len(plain), -1) and ix.n_candidates >= 16
    assert list(ix.member_off) == w.member_off and list(ix.out_off) == w.out_off
    q = eng.gzip_index(src, query=True)
    assert q[:5] == ix[:5] and q.member_off is None
    out, r = eng.gzip_read(src)
    assert r == (0, len(plain), 16, NONE32, -1) and out[:r.out_len].tobytes() == plain
    d = torch.from_numpy(src.copy()).cuda()
    d_out, r = eng.gzip_read(d)
    assert d_out.is_cuda and r.rc == 0 and d_out[:r.out_len].cpu().numpy().tobytes() == plain
    assert eng.gzip_index(d)[:5] == ix[:5]
    out, r = eng.gzip_read(src, out=np.zeros(len(plain) - 1, np.uint8))
    assert (r.rc, r.out_len) == (-2, len(plain))
    what, f, m, rc, err_off, n_good = ref.malformed_files()[8]  # a corrupt middle stream
    ix = eng.gzip_index(f)
    assert (ix.rc, ix.n_members, ix.err_off) == (rc, n_good, err_off) and list(ix.member_off) == [0, err_off]
    out, r = eng.gzip_read(f)
    assert (r.rc, r.out_len, r.n_members, r.bad_member, r.err_off) == (rc, 0, n_good, n_good, err_off)
