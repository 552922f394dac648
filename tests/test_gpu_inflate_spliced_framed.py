"""flate_hip_inflate_spliced_framed on the GPU: ONE zlib stream or gzip member around a spliced stream, its header
measured, its pieces decoded from the index and its trailer checked against the checksum of their concatenation by one
call.  Every expectation comes from the CPU (tests/spliced_framed_ref.py: the oracle's spliced stream, index, frame,
inflate and checksums; Python's zlib / gzip accept every fixture); the per-piece results must also be those of
flate_hip_inflate_spliced on the raw range alone."""
import ctypes as C
import gzip
import zlib

import numpy as np
import pytest

from framed_read_ref import gzmember
from spliced_framed_ref import Member, fixture_members, many_pieces_specs
from test_splice import _inflaters
from util import flate

pytestmark = pytest.mark.gpu

WRAP = {"raw": 0, "zlib": 1, "gzip": 2}
DEVICE_PTRS, SIZE_ONLY = 1, 8
GUARD = 0xA5


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def members(oracle):
    """{(compat, wrap): Member}: computed once, shared, never changed."""
    return fixture_members(oracle)


def call(eng, member, wrap, bit_off, slots, device=False, in_shift=0, out_shift=0, flags=0, words=True, raw=False):
    """One flate_hip_inflate_spliced_framed call through ctypes (raw=True: flate_hip_inflate_spliced on the same
    arguments).  Returns (rc, out bytes of the slots' range, out_off, out_len, status, err_off, member_status,
    member_err_off); the guard bytes around the output must have stayed what they were."""
    bit_off = np.ascontiguousarray(bit_off, dtype=np.uint64)
    n = bit_off.size - 1
    out_off = np.zeros(n + 1, np.uint64)
    np.cumsum(np.array(slots, dtype=np.uint64), out=out_off[1:])
    blob = np.frombuffer(b"\0" * in_shift + member + b"\0" * 16, np.uint8).copy()
    total = int(out_off[-1])
    obuf = np.full(out_shift + total + 64, GUARD, np.uint8)
    out_len = np.full(max(n, 1), 4242, np.uint64)
    status = np.full(max(n, 1), 99, np.int32)
    err_off = np.full(max(n, 1), 77, np.int64)
    ms, me = C.c_int32(555), C.c_int64(555)
    if device:
        import torch
        d_in, d_out = torch.from_numpy(blob).cuda(), torch.from_numpy(obuf).cuda()
        in_ptr, out_ptr = d_in.data_ptr() + in_shift, d_out.data_ptr() + out_shift
        assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    else:
        in_ptr, out_ptr = blob.ctypes.data + in_shift, obuf.ctypes.data + out_shift
    fl = flags | (DEVICE_PTRS if device else 0)
    if raw:
        rc = eng._L.flate_hip_inflate_spliced(eng._ctx, in_ptr, len(member), bit_off.ctypes.data, n, out_ptr,
                                              out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data,
                                              err_off.ctypes.data, fl)
    else:
        rc = eng._L.flate_hip_inflate_spliced_framed(
            eng._ctx, in_ptr, len(member), WRAP[wrap], bit_off.ctypes.data, n, out_ptr, out_off.ctypes.data,
            out_len.ctypes.data, status.ctypes.data, err_off.ctypes.data, C.byref(ms) if words else None,
            C.byref(me) if words else None, fl)
    if device:
        import torch
        torch.cuda.synchronize()
        obuf = d_out.cpu().numpy()
    assert (obuf[:out_shift] == GUARD).all() and (obuf[out_shift + total:] == GUARD).all(), "guard bytes touched"
    return rc, obuf[out_shift:out_shift + total], out_off, out_len[:n], status[:n], err_off[:n], ms.value, me.value


def same_as_the_raw_call(eng, framed, raw_stream, bit_off, slots, device):
    """out_len / status / err_off and the delivered bytes of a framed call == flate_hip_inflate_spliced on the raw
    range alone."""
    rc, out, ooff, olen, status, err, ms, me = framed
    rc2, out2, _, olen2, status2, err2, _, _ = call(eng, raw_stream, "raw", bit_off, slots, device=device, raw=True)
    assert (olen.tolist(), status.tolist(), err.tolist()) == (olen2.tolist(), status2.tolist(), err2.tolist())
    for i in range(len(slots)):
        a, k = int(ooff[i]), min(int(olen[i]), slots[i])
        assert out[a:a + k].tobytes() == out2[a:a + k].tobytes(), i
    first = next((int(s) for s in status if s), 0)
    assert rc2 == first
    return first


def good(eng, m, member, bit_off, slots, device, **kw):
    """A member that verifies: the pieces are the oracle's, the raw call's, and the member's words say so."""
    res = call(eng, member, m.wrap, bit_off, slots, device=device, **kw)
    rc, out, ooff, olen, status, err, ms, me = res
    assert rc == 0 and (ms, me) == (0, -1) and (status == 0).all() and (err == -1).all()
    assert olen.tolist() == m.sizes
    for i, p in enumerate(m.pieces):
        assert out[int(ooff[i]):int(ooff[i]) + len(p)].tobytes() == p, i
    return res


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
@pytest.mark.parametrize("compat", ["moonbit", "go"])
def test_round_trip(eng, members, compat, wrap, device):
    m = members[(compat, wrap)]
    for kernel in _inflaters(eng):
        for extra in (0, 1, 70000):  # the last: whole clipped-away checksum pieces behind the data
            slots = [s + extra for s in m.sizes]
            res = good(eng, m, m.member, m.bit_off, slots, device)
            assert same_as_the_raw_call(eng, res, m.raw, m.bit_off, slots, device) == 0, (kernel, extra)


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_device_pointers_at_every_alignment(eng, oracle, wrap):
    m = Member(oracle, [("text", 65537), ("text", 0), ("rand", 1), ("text", 17), ("ramp", 1025)], wrap, seed=3)
    slots = [s + (i % 3) for i, s in enumerate(m.sizes)]
    for kernel in _inflaters(eng):
        for a in range(16):
            good(eng, m, m.member, m.bit_off, slots, True, in_shift=a, out_shift=(5 * a + 3) % 16)


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_the_writers_own_blob_stays_on_the_device(eng, wrap):
    import torch
    n, blen = 256, 4096
    host = flate.synth("text", n, blen, seed=0x5EED0002)
    d_in = torch.from_numpy(host).cuda()
    blob, nbytes, bit_off = eng.deflate_spliced_framed(d_in, flate.uniform_offsets(n, blen), wrap)
    assert blob.is_cuda
    dst = torch.full((n * blen + 100,), GUARD, dtype=torch.uint8, device="cuda")
    out, ooff, olen, status, err, ms = eng.inflate_spliced_framed(blob, nbytes, wrap, bit_off, [blen] * n, out=dst)
    assert out is dst and ms == 0 and (status == 0).all() and (olen == blen).all() and (err == -1).all()
    assert torch.equal(dst[:n * blen], d_in) and bool((dst[n * blen:] == GUARD).all())
    # a flipped bit of the trailer raises with check=True and is reported with check=False
    blob[nbytes - 1] ^= 1
    with pytest.raises(flate.FlateError) as ei:
        eng.inflate_spliced_framed(blob, nbytes, wrap, bit_off, [blen] * n)
    assert ei.value.code == -4
    _, _, _, status, _, ms = eng.inflate_spliced_framed(blob, nbytes, wrap, bit_off, [blen] * n, check=False)
    assert ms == -4 and (status == 0).all() and eng.last_member_err_off == nbytes


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_a_blob_of_no_input(eng, wrap):
    blob, nbytes, bit_off = eng.deflate_spliced_framed(np.zeros(8, np.uint8), np.zeros(1, np.uint64), wrap, index=True)
    assert bit_off.tolist() == [0]
    assert (zlib.decompress if wrap == "zlib" else gzip.decompress)(bytes(blob[:nbytes])) == b""
    for device in (False, True):
        data = blob
        if device:
            import torch
            data = torch.from_numpy(np.ascontiguousarray(blob)).cuda()
        out, ooff, olen, status, err, ms = eng.inflate_spliced_framed(data, nbytes, wrap, bit_off, [])
        assert ms == 0 and status.tolist() == [0] and olen.tolist() == [0] and ooff.tolist() == [0, 0]
    # ... and the trailer of nothing is still checked
    bad = np.array(blob[:nbytes + 8], np.uint8)
    bad[nbytes - 1] ^= 1
    _, _, _, status, _, ms = eng.inflate_spliced_framed(bad, nbytes, wrap, bit_off, [], check=False)
    assert ms == -4 and status.tolist() == [0]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_foreign_gzip_headers_around_the_same_raw_stream(eng, members, device):
    """FNAME, FEXTRA, and both plus FHCRC: the index is unchanged -- the header's length is found on the device."""
    m = members[("moonbit", "gzip")]
    for flg, extra in ((8, b""), (4, b"\x01\x02" * 21), (4 | 8 | 2, b"\x07" * 300), (4 | 8 | 16 | 2, b"")):
        member = gzmember(m.whole, flg=flg, extra=extra, raw=m.raw)
        assert gzip.decompress(member) == m.whole and len(member) > len(m.member)
        res = good(eng, m, member, m.bit_off, [s + 1 for s in m.sizes], device)
        same_as_the_raw_call(eng, res, m.raw, m.bit_off, [s + 1 for s in m.sizes], device)


def case3(eng, m, member, device, slots=None):
    """Every piece 0 and delivered, the member corrupt at its end."""
    slots = m.sizes if slots is None else slots
    rc, out, ooff, olen, status, err, ms, me = call(eng, member, m.wrap, m.bit_off, slots, device=device)
    assert rc == -4 and (ms, me) == (-4, len(member)), (rc, ms, me)
    assert (status == 0).all() and (err == -1).all() and olen.tolist() == m.sizes
    return out, ooff


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_a_trailer_that_does_not_match(eng, oracle, members, wrap, device):
    m = members[("moonbit", wrap)]
    for kernel in _inflaters(eng):
        for k in range(4):  # every byte of the checksum
            bad = bytearray(m.member)
            bad[len(bad) - m.tl + k] ^= 0x10
            out, ooff = case3(eng, m, bytes(bad), device)
            assert out.tobytes() == m.whole
    if wrap == "gzip":  # a wrong ISIZE alone
        for k in range(4):
            bad = bytearray(m.member)
            bad[len(bad) - 4 + k] ^= 1
            case3(eng, m, bytes(bad), device)
    # one flipped payload byte inside the stored block of piece 11 (16 bytes of text): every piece still decodes
    at = m.hl + (int(m.bit_off[12]) >> 3) - 5
    bad = bytearray(m.member)
    bad[at] ^= 0x20
    assert m.member[at:at + 1] == m.pieces[11][11:12]
    rc, got, _, _ = oracle.inflate(bytes(bad[m.hl:len(bad) - m.tl]), len(m.whole), full=True)
    assert rc == 0 and got != m.whole and len(got) == len(m.whole)
    out, ooff = case3(eng, m, bytes(bad), device)
    assert out.tobytes() == got
    # the NULL member words are optional
    rc, _, _, _, status, _, ms, me = call(eng, bytes(bad), wrap, m.bit_off, m.sizes, device=device, words=False)
    assert rc == -4 and (status == 0).all() and (ms, me) == (555, 555)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_a_bad_header(eng, members, device):
    for wrap, member in (("gzip", b"\x1f\x8c" + members[("moonbit", "gzip")].member[2:]),
                         ("zlib", b"\x78\x20\0\0\0\1" + members[("moonbit", "zlib")].member[2:]),   # FDICT
                         ("zlib", b"\x78\x02" + members[("moonbit", "zlib")].member[2:])):          # FCHECK
        m = members[("moonbit", wrap)]
        for kernel in _inflaters(eng):
            rc, out, ooff, olen, status, err, ms, me = call(eng, member, wrap, m.bit_off, m.sizes, device=device)
            assert rc == -4 and (ms, me) == (-4, 0)
            assert (status == -4).all() and (err == 0).all() and (olen == 0).all()
            if device:  # (host pointers: the slots' range is copied back as one piece, as in the raw call)
                assert (out == GUARD).all(), "a bad header wrote to the output"


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_a_raw_stream_cut_short_in_front_of_the_trailer(eng, oracle, members, wrap, device):
    """The last piece meets the raw stream's end, -7, and nothing of the trailer is decoded: the results are the raw
    call's on the cut stream alone.  Cut by 9 bytes the index no longer fits behind the SHORTEST header (the stream
    ends in front of bit_off[n]), which the host refuses; behind a longer foreign header it passes the host's check
    and the device clamps the entry."""
    m = members[("moonbit", wrap)]
    n = len(m.sizes)
    cuts = [(1, m.member[:m.hl])]
    if wrap == "gzip":
        hdr = gzmember(b"", flg=4 | 8, extra=b"\x05" * 40, raw=b"")[:-8]
        cuts += [(1, hdr), (9, hdr)]
    for kernel in _inflaters(eng):
        for k, hdr in cuts:
            raw = m.raw[:-k]
            member = hdr + raw + m.trailer
            assert oracle.inflate(raw, len(m.whole), full=True)[0] == oracle.E_UNEXPECTED_EOF
            res = call(eng, member, wrap, m.bit_off, m.sizes, device=device)
            rc, out, ooff, olen, status, err, ms, me = res
            assert rc == -7 and (ms, me) == (-7, -1), (kernel, k, rc, ms, me)
            assert status[n - 1] == -7 and (status[:n - 1] == 0).all()
            if int(m.bit_off[-1]) <= 8 * len(raw):  # (else the raw call refuses the index: the oracle alone judges)
                assert same_as_the_raw_call(eng, res, raw, m.bit_off, m.sizes, device) == -7
            for i in range(n - 1):
                assert out[int(ooff[i]):int(ooff[i + 1])].tobytes() == m.pieces[i]
            a = int(ooff[n - 1])  # ... and the last piece delivers what a reader of the cut stream has in hand
            assert b"".join(m.pieces[:n - 1]) + out[a:a + int(olen[n - 1])].tobytes() == \
                oracle.inflate(raw, len(m.whole), full=True)[1]
    member = m.member[:m.hl] + m.raw[:-9] + m.trailer
    assert call(eng, member, wrap, m.bit_off, m.sizes, device=device)[0] == -1


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_index_entries_behind_the_raw_streams_end(eng, oracle, device):
    """Behind a long foreign header the host cannot see that most of the raw stream is missing: every piece that would
    start behind its end is clamped there, sees no input and reports -7; nothing behind the end is read."""
    m = Member(oracle, [("text", 300), ("text", 0), ("rand", 40), ("text", 17), ("text", 200)], "gzip", seed=8)
    hdr = gzmember(b"", flg=4, extra=b"\x05" * 400, raw=b"")[:-8]
    keep = (int(m.bit_off[1]) >> 3) - 20  # the raw stream ends inside piece 0
    member = hdr + m.raw[:keep] + m.trailer
    assert int(m.bit_off[-1]) <= 8 * (len(member) - 18)
    for kernel in _inflaters(eng):
        rc, out, ooff, olen, status, err, ms, me = call(eng, member, "gzip", m.bit_off, m.sizes, device=device)
        assert rc == -7 and (ms, me) == (-7, -1), kernel
        assert (status == -7).all() and (err == -1).all() and (olen[1:] == 0).all(), (kernel, status, err, olen)
        assert out[:int(olen[0])].tobytes() == oracle.inflate(m.raw[:keep], 300, full=True)[1]


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_an_index_entry_off_its_block_boundary(eng, members, wrap):
    m = members[("go", wrap)]
    bad = m.bit_off.copy()
    bad[7] += 1  # piece 6 now runs into piece 7's first block, piece 7 starts mid-block
    for kernel in _inflaters(eng):
        res = call(eng, m.member, wrap, bad, m.sizes, device=True)
        rc, out, ooff, olen, status, err, ms, me = res
        assert status[6] in (-2, -4) and status[7] != 0, kernel
        assert (np.delete(status, [6, 7]) == 0).all(), kernel
        assert rc == status[6] == ms and me == -1
        assert same_as_the_raw_call(eng, res, m.raw, bad, m.sizes, True) == status[6]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_a_piece_that_produces_less_than_its_slot_in_the_middle(eng, members, wrap, device):
    m = members[("moonbit", wrap)]
    slots = list(m.sizes)
    slots[2] += 5000
    slots[6] += 65536 + 3
    slots[1] += 9  # (an empty piece with room)
    good(eng, m, m.member, m.bit_off, slots, device)


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_3000_pieces(eng, oracle, wrap):
    """More pieces than one chunk of the join kernel's walk, a random third of them empty."""
    m = Member(oracle, many_pieces_specs(), wrap, seed=5)
    assert m.sizes.count(0) > 800 and len(m.sizes) == 3000
    for kernel in _inflaters(eng):
        good(eng, m, m.member, m.bit_off, [s + (i % 2) for i, s in enumerate(m.sizes)], True)
    bad = bytearray(m.member)
    bad[-m.tl] ^= 1
    case3(eng, m, bytes(bad), True)


def test_wrap_raw_is_the_raw_call(eng, members):
    m = members[("moonbit", "zlib")]
    bad = m.bit_off.copy()
    bad[7] += 1
    for bits in (m.bit_off, bad):
        rc, out, ooff, olen, status, err, ms, me = call(eng, m.raw, "raw", bits, m.sizes, device=True)
        rc2, out2, _, olen2, status2, err2, _, _ = call(eng, m.raw, "raw", bits, m.sizes, device=True, raw=True)
        assert (rc, olen.tolist(), status.tolist(), err.tolist()) == (rc2, olen2.tolist(), status2.tolist(), err2.tolist())
        assert (ms, me) == (next((int(s) for s in status if s), 0), -1)
        assert out.tobytes() == out2.tobytes()


def test_no_pieces_and_refused_arguments(eng, members):
    """Every refusal is made before any HIP call; they need a ctx to be told from a missing one."""
    m = members[("moonbit", "gzip")]
    n = len(m.sizes)
    z = members[("moonbit", "zlib")]

    def f(member=m.member, wrap="gzip", bits=m.bit_off, flags=0, n_=None, null=None, in_len=None):
        bits = np.ascontiguousarray(bits, np.uint64)
        k = bits.size - 1 if n_ is None else n_
        buf = np.frombuffer(member + b"\0" * 16, np.uint8).copy()
        ooff = np.zeros(n + 1, np.uint64)
        np.cumsum(np.array(m.sizes, np.uint64), out=ooff[1:])
        if null == "out_off not monotone":
            ooff[3] = ooff[4] + 1
        out = np.zeros(int(ooff[-1]) + 16, np.uint8)
        olen, st, eo = np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.int64)
        ms, me = C.c_int32(555), C.c_int64(555)
        args = {"in": buf.ctypes.data, "bit_off": bits.ctypes.data, "out": out.ctypes.data, "out_off": ooff.ctypes.data,
                "out_len": olen.ctypes.data, "status": st.ctypes.data, "err_off": eo.ctypes.data}
        if null in args:
            args[null] = None
        rc = eng._L.flate_hip_inflate_spliced_framed(
            eng._ctx, args["in"], len(member) if in_len is None else in_len, WRAP.get(wrap, wrap), args["bit_off"], k,
            args["out"], args["out_off"], args["out_len"], args["status"], args["err_off"], C.byref(ms), C.byref(me),
            flags)
        if rc in (-1, -6):
            assert (ms.value, me.value) == (555, 555)  # a refused call writes nothing
        return rc
    assert f() == 0
    for wrap in ("raw", "zlib", "gzip"):
        assert f(wrap=wrap, n_=0) == 0                                      # nothing is read
    assert f(wrap=3) == -1 and f(wrap=0xFFFFFFFF) == -1                     # an unknown wrap
    for wrap, mem in (("raw", m.raw), ("zlib", z.member), ("gzip", m.member)):
        assert f(member=mem, wrap=wrap, flags=SIZE_ONLY) == -1              # no size-only pass
        for null in ("in", "bit_off", "out", "out_off", "out_len", "status", "err_off"):
            assert f(member=mem, wrap=wrap, null=null) == -1, (wrap, null)
        assert f(member=mem, wrap=wrap, in_len=0) == -1
        assert f(member=mem, wrap=wrap, null="out_off not monotone") == -1
    notmono = m.bit_off.copy()
    notmono[5] = notmono[6] + 1
    assert f(bits=notmono) == -1                                            # the index is not monotone
    beyond = m.bit_off.copy()
    beyond[-1] = 8 * (len(m.member) - 18) + 1
    assert f(bits=beyond) == -1                                             # ... or runs beyond the member
    beyond[-1] -= 1
    assert f(bits=beyond) in (0, -2, -4, -7)
    zb = z.bit_off.copy()
    zb[-1] = 8 * (len(z.member) - 6) + 1
    assert f(member=z.member, wrap="zlib", bits=zb) == -1
    for wrap, frame in (("zlib", 6), ("gzip", 18)):                         # shorter than header plus trailer
        assert f(member=bytes(frame - 1), wrap=wrap, bits=[0, 0]) == -1
        assert f(member=bytes(frame), wrap=wrap, bits=[0, 0]) == -4         # (long enough: the device reads it)
    big = np.array([0, 1 << 30], np.uint64)
    assert f(member=m.member, bits=big, in_len=1 << 40) == -6               # a piece of 2^30 bits


def test_stages_are_reported_with_profiling_on(eng, members):
    m = members[("moonbit", "gzip")]
    eng.set_profiling(True)
    try:
        good(eng, m, m.member, m.bit_off, m.sizes, True)
        t = eng.last_timing()
    finally:
        eng.set_profiling(False)
    assert t["inflate"] > 0 and t["checksum"] > 0 and t["lz77_match"] == 0 and t["huff_pack"] == 0, t
