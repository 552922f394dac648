"""One long DEFLATE stream decoded in parallel on the GPU: flate_hip_inflate_one.  The bytes come from zlib; status,
err_off and out_len of the failing streams come from the serial decoders on the same bytes as one stream
(flate_hip_inflate_batch for raw streams, flate_hip_inflate_batch_framed for zlib and gzip members) -- the yardstick,
not the code under test.  The corpus is tests/one_ref.py's."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import one_ref as ref
from test_gpu_inflate_one import failing_streams, on_device
from util import STATUS_OF_ORACLE, flate

pytestmark = pytest.mark.gpu

DEVICE_PTRS = 1
GUARD = 0xA5
INVALID, OUT_TOO_SMALL = -1, -2
KINDS = (ref.RAW, ref.ZLIB, ref.GZIP)
NAMES = {ref.ZLIB: "zlib", ref.GZIP: "gzip"}


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def good(oracle):
    """[(what, raw stream, plain, Walk)]: computed once, shared, never changed."""
    return [(w, r, p, ref.Walk(r)) for w, r, p in ref.good_streams(oracle)]


def read(eng, f, kind, cap, device=False, shift=0, out_shift=0, query=False):
    """One call into a 0xA5-prefilled buffer -> (rc, bytes, out_len, status, err_off, n_units, n_candidates, buffer)."""
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
    ol, st, eo, nu, nc = C.c_uint64(99), C.c_int32(99), C.c_int64(99), C.c_uint32(99), C.c_uint32(99)
    rc = eng._L.flate_hip_inflate_one(eng._ctx, ptr if n else None, n, kind, None if query else out_ptr, 0 if query else cap,
                                      C.byref(ol), C.byref(st), C.byref(eo), C.byref(nu), C.byref(nc),
                                      DEVICE_PTRS if device else 0)
    if device:
        import torch
        torch.cuda.synchronize()
        obuf = d_out.cpu().numpy()
    assert (obuf[:out_shift] == GUARD).all() and (obuf[out_shift + cap:] == GUARD).all(), "guard bytes touched"
    body = obuf[out_shift:out_shift + cap]
    if device and ol.value <= cap:  # with device pointers nothing outside out[0, out_len) is written
        assert (body[ol.value:] == GUARD).all(), "bytes behind out_len touched"
    return rc, body[:min(ol.value, cap)].tobytes(), ol.value, st.value, eo.value, nu.value, nc.value, body


def check_good(eng, raw, plain, w, what, kind, **kw):
    rc, got, ol, st, eo, nu, nc, _ = read(eng, ref.wrap(raw, plain, kind), kind, len(plain), **kw)
    assert (rc, st, eo, ol, nu) == (0, 0, -1, len(plain), w.n_units), (what, kind, kw, rc, st, eo, ol)
    assert got == plain, (what, kind, kw)
    return nc


# ---- the corpus ----

def test_every_stream_in_every_container_with_host_pointers(eng, good):
    for what, raw, plain, w in good:
        assert zlib.decompress(raw, -15) == plain, what
        for kind in KINDS:
            check_good(eng, raw, plain, w, what, kind)
    what, raw, plain, w = good[ref.MANY_UNITS]
    check_good(eng, raw, plain, w, what, ref.GZIP, shift=3, out_shift=1)


def test_device_pointers_at_shifted_addresses(eng, good):
    for k in (0, ref.MANY_UNITS, 5, 6, 7, 8, 12):
        what, raw, plain, w = good[k]
        for shift in (0, 1, 3):
            check_good(eng, raw, plain, w, what, KINDS[shift % 3], device=True, shift=shift, out_shift=shift)


def test_rounds_carry_the_window(eng, good):
    """"one_round_units" = 7 forces 33 rounds on the 230-unit file, whose units are all shorter than 32 KiB: every
    window is mostly pass-through and the seed crosses every round."""
    w = good[ref.MANY_UNITS][3]
    assert w.n_units >= 100 and max(b - a for a, b in zip(w.out_off, w.out_off[1:])) < 32768
    try:
        for units in (7, 1, 64):
            eng.set_option("one_round_units", units)
            for k in (ref.MANY_UNITS, 4, 5):
                what, raw, plain, wk = good[k]
                check_good(eng, raw, plain, wk, what, ref.GZIP, device=True, shift=1)
    finally:
        eng.set_option("one_round_units", 4096)
    for bad in (0, 65537):
        with pytest.raises(flate.FlateError):
            eng.set_option("one_round_units", bad)


def test_decoys_write_nothing(eng):
    for what, raw, plain in ref.decoy_streams():
        w = ref.Walk(raw)
        nc = check_good(eng, raw, plain, w, what, ref.RAW, device=True, shift=1, out_shift=5)
        assert nc > w.n_units, what


def test_size_query_capacity_and_wrappers(eng, good):
    what, raw, plain, w = good[ref.MANY_UNITS]
    f = ref.wrap(raw, plain, ref.GZIP)
    rc, _, ol, st, eo, nu, nc, _ = read(eng, f, ref.GZIP, 0, query=True)
    assert (rc, ol, st, nu) == (OUT_TOO_SMALL, len(plain), 0, w.n_units)
    for device in (False, True):
        rc, _, ol, st, eo, nu, nc, body = read(eng, f, ref.GZIP, len(plain) - 1, device=device)  # one byte short
        assert (rc, ol) == (OUT_TOO_SMALL, len(plain)) and (body == GUARD).all(), device
    out, r = eng.inflate_one(np.frombuffer(f, np.uint8), "gzip")
    assert (r.rc, r.out_len, r.status, r.err_off, r.n_units) == (0, len(plain), 0, -1, w.n_units)
    assert out[:r.out_len].tobytes() == plain
    import torch
    d = torch.from_numpy(np.frombuffer(ref.wrap(raw, plain, ref.ZLIB), np.uint8).copy()).cuda()
    out, r = eng.inflate_one(d, "zlib")
    assert r[:4] == (0, len(plain), 0, -1) and out.is_cuda and out[:r.out_len].cpu().numpy().tobytes() == plain
    out, r = eng.inflate_one(ref.wrap(b"\x03\x00", b"", ref.GZIP), "gzip")
    assert r[:4] == (0, 0, 0, -1)
    # refused before any HIP call
    src = np.frombuffer(f, np.uint8).copy()
    ol64, st32 = C.c_uint64(0), C.c_int32(0)
    for wrap, out_ptr, cap, flags in ((3, None, 0, 0), (2, None, 5, 0), (2, None, 0, 8), (2, None, 0, 2)):
        assert eng._L.flate_hip_inflate_one(eng._ctx, src.ctypes.data, len(f), wrap, out_ptr, cap, C.byref(ol64),
                                            C.byref(st32), None, None, None, flags) == INVALID


# ---- failing streams ----

def test_failing_raw_streams_equal_the_serial_decoder(eng, good, oracle):
    """Every case and variant of the edge corpus, cuts and flipped bits in the 230-unit file, and the distance that
    reaches one byte in front of the stream: status, err_off, out_len and the bytes in front of the error."""
    cases = failing_streams(good)
    off = np.zeros(len(cases) + 1, np.uint64)
    np.cumsum(np.array([len(r) for _, r in cases], dtype=np.uint64), out=off[1:])
    data = np.frombuffer(b"".join(r for _, r in cases) + b"\0" * 8, np.uint8).copy()
    caps = [ref.Walk(raw).out_len + 600 for _, raw in cases]
    out, ooff, olen, status, err = eng.inflate_batch(data, off, caps, check=False)
    seen = set()
    for k, (what, raw) in enumerate(cases):
        want = bytes(out[int(ooff[k]):int(ooff[k]) + int(olen[k])])
        orc, obytes, _, oerr = oracle.inflate(raw, caps[k], full=True)  # the yardstick itself against the oracle
        assert (int(status[k]), int(err[k]), want) == (STATUS_OF_ORACLE[orc], oerr, obytes), (what, orc, oerr, len(obytes))
        rc, got, ol, st, eo, nu, nc, _ = read(eng, raw, ref.RAW, caps[k], device=k % 2 == 1)
        assert (rc, st, eo, ol) == (int(status[k]), int(status[k]), int(err[k]), int(olen[k])), (what, rc, st, eo, ol)
        assert got == want, what
        seen.add(st)
    assert seen >= {0, ref.CORRUPT, ref.UNEXPECTED_EOF}
    legal, plain, illegal = ref.history_pair()
    k = [r for _, r in cases].index(illegal)
    assert int(status[k]) == ref.CORRUPT and int(err[k]) > 0  # the history-dependent verdict is in the list
    assert read(eng, legal, ref.RAW, len(plain))[:5] == (0, plain, len(plain), 0, -1)


def test_failing_members_equal_the_framed_decoder(eng, good):
    _, raw, plain, w = good[ref.MANY_UNITS]
    cut = raw[:(w.unit_bit[5] + w.unit_bit[6]) // 16]
    flipped = bytearray(raw)
    flipped[(w.unit_bit[7] + 20) >> 3] ^= 1 << ((w.unit_bit[7] + 20) & 7)
    body = bytearray(raw)
    bit = (w.unit_bit[100] + w.unit_bit[101]) // 2
    body[bit >> 3] ^= 1 << (bit & 7)
    members = []
    for kind in (ref.ZLIB, ref.GZIP):
        good_f = ref.wrap(raw, plain, kind)
        members += [(kind, "cut", ref.wrap(cut, plain, kind)), (kind, "flipped header bit", ref.wrap(bytes(flipped), plain, kind)),
                    (kind, "flipped body bit", ref.wrap(bytes(body), plain, kind)),
                    (kind, "wrong checksum", good_f[:-8 if kind == ref.GZIP else -4] + b"\x00" + good_f[-7 if kind == ref.GZIP else -3:])]
    g = ref.wrap(raw, plain, ref.GZIP)
    members.append((ref.GZIP, "wrong ISIZE", g[:-4] + struct.pack("<I", len(plain) + 1)))
    z = ref.wrap(raw, plain, ref.ZLIB)
    members.append((ref.ZLIB, "FDICT set", bytes([0x78, 0xbb]) + z[2:]))
    members.append((ref.GZIP, "too short for header and trailer", ref.wrap(b"", b"", ref.GZIP)[:17]))
    for kind, what, f in members:
        arr = np.frombuffer(f, np.uint8)
        fout, foff, folen, fstatus = eng.inflate_batch_framed(arr, np.array([0, arr.size], np.uint64), NAMES[kind],
                                                              out_sizes=[len(plain)])
        rc, got, ol, st, eo, nu, nc, _ = read(eng, f, kind, len(plain), device=True, shift=1)
        assert st != 0 and (rc, st, ol) == (int(fstatus[0]), int(fstatus[0]), int(folen[0])), (what, kind, rc, st, ol)
        assert got == bytes(fout[:int(folen[0])]), (what, kind)
        if what in ("wrong checksum", "wrong ISIZE"):
            assert (st, eo, ol) == (ref.CORRUPT, len(f), len(plain)), (what, kind, eo)  # the trailer: err_off = in_len
        if what in ("FDICT set", "too short for header and trailer"):
            assert (st, eo, ol, nc) == (ref.CORRUPT, 0, 0, 0), (what, kind)
    for kind, want in ((ref.RAW, (ref.UNEXPECTED_EOF, -1)), (ref.ZLIB, (ref.CORRUPT, 0)), (ref.GZIP, (ref.CORRUPT, 0))):
        rc, got, ol, st, eo, nu, nc, _ = read(eng, b"", kind, 16)
        assert (rc, st, eo, ol) == (want[0], want[0], want[1], 0), kind
