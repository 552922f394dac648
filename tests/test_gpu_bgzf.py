"""BGZF files on the GPU: flate_hip_bgzf_write, flate_hip_bgzf_index and flate_hip_bgzf_read.  Every expectation comes
from the CPU: tests/bgzf_ref.py (the member builder around the oracle's streams, the serial walk, the corpus), gzip's
own reader, and framed_read_ref.expected for what one member must come out as."""
import ctypes as C
import gzip

import numpy as np
import pytest

import bgzf_ref as ref
from framed_read_ref import expected
from util import flate

pytestmark = pytest.mark.gpu

DEVICE_PTRS, COMPAT_GO = 1, 2
GUARD = 0xA5
NONE32 = 0xffffffff


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def inputs():
    """One input per length of ref.WRITE_LENGTHS, mixed fills (computed once, shared, never changed)."""
    return ref.write_inputs()


@pytest.fixture(scope="module")
def ref_files(oracle, inputs):
    """{(in_len, block_bytes, compat): (file, member_off)} by the reference, built once."""
    out = {}
    for n, data in inputs.items():
        for bb in (0, 4096, 65280) + ((1,) if n <= 300 else ()):
            for compat in (0, 1):
                out[n, bb, compat] = ref.build_file(oracle, data, bb, compat)
    return out


def on_device(b, shift=0, pad=64):
    """bytes -> (keep-alive tensor, device pointer of the first byte) at the given byte alignment."""
    import torch
    t = torch.from_numpy(np.frombuffer(b"\0" * shift + bytes(b) + b"\0" * pad, np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + shift


# ---- write ----

def write(eng, data, bb, compat, device=False, out_shift=0, cap=None, want_off=True):
    """One flate_hip_bgzf_write call through ctypes -> (rc, file bytes, member_off); the guard bytes around the
    capacity must have stayed what they were."""
    n = len(data)
    nb = -(-n // (bb or ref.BLOCK_DEFAULT))
    if cap is None:
        cap = eng._L.flate_hip_bgzf_bound(n, bb)
    obuf = np.full(out_shift + cap + 64, GUARD, np.uint8)
    src = np.frombuffer(data, np.uint8) if n else np.zeros(1, np.uint8)
    moff = np.full(nb + 1, 7, np.uint64)
    out_len = C.c_uint64(0)
    flags = (COMPAT_GO if compat else 0) | (DEVICE_PTRS if device else 0)
    if device:
        import torch
        d_in, d_out = torch.from_numpy(src.copy()).cuda(), torch.from_numpy(obuf).cuda()
        in_ptr, out_ptr = d_in.data_ptr(), d_out.data_ptr() + out_shift
    else:
        in_ptr, out_ptr = src.ctypes.data, obuf.ctypes.data + out_shift
    rc = eng._L.flate_hip_bgzf_write(eng._ctx, in_ptr if n else None, n, bb, out_ptr, cap, C.byref(out_len),
                                     moff.ctypes.data if want_off else None, flags)
    if device:
        import torch
        torch.cuda.synchronize()
        obuf = d_out.cpu().numpy()
    assert (obuf[:out_shift] == GUARD).all() and (obuf[out_shift + cap:] == GUARD).all(), "guard bytes touched"
    return rc, obuf[out_shift:out_shift + int(out_len.value)].tobytes(), moff


@pytest.mark.parametrize("compat", [0, 1])
def test_write_host_pointers_equal_the_reference(eng, inputs, ref_files, compat):
    for (n, bb, cg), (want, want_off) in ref_files.items():
        if cg != compat:
            continue
        rc, got, moff = write(eng, inputs[n], bb, compat)
        assert rc == 0 and got == want, (n, bb, len(got), len(want))
        assert (moff == want_off).all(), (n, bb)
        assert gzip.decompress(got) == inputs[n], (n, bb)


@pytest.mark.parametrize("compat", [0, 1])
def test_write_device_pointers_at_every_alignment_of_out(eng, inputs, ref_files, compat):
    k = 0
    for (n, bb, cg), (want, want_off) in ref_files.items():
        if cg != compat or (bb == 1 and n > 17):
            continue
        for shift in ((k % 8, (k + 3) % 8) if n < 65279 else (k % 8,)):
            rc, got, moff = write(eng, inputs[n], bb, compat, device=True, out_shift=shift)
            assert rc == 0 and got == want and (moff == want_off).all(), (n, bb, shift)
        k += 1
    data = inputs[65281]
    want = ref_files[65281, 4096, compat][0]
    for shift in range(8):  # every alignment, members of several blocks
        rc, got, _ = write(eng, data, 4096, compat, device=True, out_shift=shift, want_off=False)
        assert rc == 0 and got == want, shift


def test_write_tight_capacity(eng, inputs, ref_files):
    for n, bb in ((0, 0), (1, 0), (128, 1), (65281, 4096), (3 * 65280 + 5, 0)):
        want = ref_files[n, bb, 0][0]
        for device in (False, True):
            rc, got, _ = write(eng, inputs[n], bb, 0, device=device, cap=len(want))
            assert rc == 0 and got == want, (n, bb, device)
            rc, _, _ = write(eng, inputs[n], bb, 0, device=device, cap=len(want) - 1)
            assert rc == -2, (n, bb, device)


def test_write_refuses_bad_arguments(eng, inputs):
    for bb in (65536, 70000, 0xffffffff):
        assert write(eng, inputs[128], bb, 0, cap=4096)[0] == -1
    out, n64 = (C.c_uint8 * 64)(), C.c_uint64()
    src = (C.c_uint8 * 16)()
    L = eng._L
    assert L.flate_hip_bgzf_write(eng._ctx, src, 16, 0, None, 64, C.byref(n64), None, 0) == -1
    assert L.flate_hip_bgzf_write(eng._ctx, None, 16, 0, out, 64, C.byref(n64), None, 0) == -1
    assert L.flate_hip_bgzf_write(eng._ctx, src, 16, 0, out, 64, None, None, 0) == -1
    assert L.flate_hip_bgzf_write(eng._ctx, src, 16, 0, out, 64, C.byref(n64), None, 8) == -1  # FLATE_HIP_SIZE_ONLY


def test_write_the_65536_edge(eng, oracle):
    """A member larger than 65536 bytes cannot carry its size.  The expectations are the oracle's sizes now; seen with
    default_rng(1) random bytes: Go mode 65500 -> 65536 (BSIZE ff ff), 65501 -> 65537; MoonBit mode 65280 -> 65365,
    65499 -> 65584."""
    rnd = np.random.default_rng(1).integers(0, 256, 65535, dtype=np.uint8).tobytes()
    text = ref.text(3000)
    seen = set()
    for compat, n in ((1, 65500), (1, 65501), (0, 65280), (0, 65499)):
        block = rnd[:n]
        size = 18 + len(oracle.deflate(np.frombuffer(block, np.uint8), compat=compat)) + 8
        fits = size <= ref.MEMBER_MAX
        seen.add((fits, size == ref.MEMBER_MAX))
        data = block
        rc, got, moff = write(eng, data, n, compat, device=True)
        if fits:
            assert rc == 0 and got == ref.build_file(oracle, data, n, compat)[0], (compat, n, size)
            assert got[16:18] == (size - 1).to_bytes(2, "little") and gzip.decompress(got) == data
        else:
            assert rc == ref.TOO_LARGE, (compat, n, size, rc)
            assert "block 0" in eng._L.flate_hip_last_hip_error(eng._ctx).decode()
    assert (True, True) in seen and (False, False) in seen  # a member of exactly 65536 bytes, and one too large
    # the first oversized block is named: three blocks, the last two too large (block_bytes 65535, random bytes)
    rc, _, _ = write(eng, text[:65535].ljust(65535, b"a") + rnd + rnd[::-1], 65535, 0)
    assert rc == ref.TOO_LARGE and "block 1 " in eng._L.flate_hip_last_hip_error(eng._ctx).decode()


def test_engine_bgzf_write_and_read_round_trip(eng, inputs, ref_files):
    import torch
    data = inputs[3 * 65280 + 5]
    f, moff = eng.bgzf_write(data, index=True)
    assert f == ref_files[len(data), 0, 0][0] and (moff == ref_files[len(data), 0, 0][1]).all()
    out, r = eng.bgzf_read(np.frombuffer(f, np.uint8))
    assert r == (0, len(data), 5, NONE32, -1, 1) and out[:r.out_len].tobytes() == data
    d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    d_f, d_len = eng.bgzf_write(d, block_bytes=4096, compat_go=True)
    assert d_f.is_cuda and d_f[:d_len].cpu().numpy().tobytes() == ref_files[len(data), 4096, 1][0]
    d_out, r = eng.bgzf_read(d_f[:d_len].clone())
    assert d_out.is_cuda and r.rc == 0 and r.eof_marker == 1 and d_out[:r.out_len].cpu().numpy().tobytes() == data
    ix = eng.bgzf_index(d_f[:d_len].clone())
    assert ix.rc == 0 and ix.n_members == -(-len(data) // 4096) + 1 and ix.out_bytes == len(data)
    with pytest.raises(flate.FlateError):
        eng.bgzf_write(data, block_bytes=65536)


# ---- index ----

def index(eng, f, device=False, shift=0, cap=None, query=False):
    """One flate_hip_bgzf_index call -> (rc, n_members, out_bytes, eof_marker, err_off, member_off, out_off)."""
    n = len(f)
    keep, ptr = on_device(f, shift) if device else (np.frombuffer(bytes(f) + b"\0", np.uint8).copy(), None)
    if not device:
        ptr = keep.ctypes.data
    w = ref.Walk(f)
    if cap is None:
        cap = w.n_members + 1
    moff, ooff = np.full(cap + 2, 7, np.uint64), np.full(cap + 2, 7, np.uint64)
    nm, ob, eof, eo = C.c_uint32(99), C.c_uint64(99), C.c_int(99), C.c_int64(99)
    rc = eng._L.flate_hip_bgzf_index(eng._ctx, ptr if n else None, n, 0 if query else cap,
                                     None if query else moff.ctypes.data, None if query else ooff.ctypes.data,
                                     C.byref(nm), C.byref(ob), C.byref(eof), C.byref(eo), DEVICE_PTRS if device else 0)
    assert (moff[cap:] == 7).all() and (ooff[cap:] == 7).all(), "the arrays were written past index_cap"
    return rc, nm.value, ob.value, eof.value, eo.value, moff, ooff


def check_index(eng, f, what, **kw):
    w = ref.Walk(f)
    rc, nm, ob, eof, eo, moff, ooff = index(eng, f, **kw)
    assert (rc, nm, ob, eof, eo) == (w.rc, w.n_members, w.out_bytes, w.eof_marker, w.err_off), (what, kw)
    if rc == 0:
        assert list(moff[:nm + 1]) == w.member_off and list(ooff[:nm + 1]) == w.out_off, (what, kw)
    else:
        assert (moff == 7).all() and (ooff == 7).all(), what


# ---- read ----

def read(eng, f, device=False, shift=0, out_shift=0, cap=None):
    """One flate_hip_bgzf_read call into a prefilled buffer -> (rc, out bytes, out_len, n_members, bad_member,
    err_off, eof_marker, the whole buffer behind out_shift)."""
    n = len(f)
    w = ref.Walk(f)
    if cap is None:
        cap = w.out_bytes
    obuf = np.full(out_shift + cap + 64, GUARD, np.uint8)
    if device:
        import torch
        keep, ptr = on_device(f, shift)
        d_out = torch.from_numpy(obuf).cuda()
        out_ptr = d_out.data_ptr() + out_shift
    else:
        keep = np.frombuffer(b"\0" * shift + bytes(f) + b"\0", np.uint8).copy()
        ptr, out_ptr = keep.ctypes.data + shift, obuf.ctypes.data + out_shift
    ol, nm, bad, eo, eof = C.c_uint64(99), C.c_uint32(99), C.c_uint32(99), C.c_int64(99), C.c_int(99)
    rc = eng._L.flate_hip_bgzf_read(eng._ctx, ptr if n else None, n, out_ptr, cap, C.byref(ol), C.byref(nm),
                                    C.byref(bad), C.byref(eo), C.byref(eof), DEVICE_PTRS if device else 0)
    if device:
        import torch
        torch.cuda.synchronize()
        obuf = d_out.cpu().numpy()
    assert (obuf[:out_shift] == GUARD).all() and (obuf[out_shift + cap:] == GUARD).all(), "guard bytes touched"
    body = obuf[out_shift:out_shift + cap]
    return rc, body[:min(ol.value, cap)].tobytes(), ol.value, nm.value, bad.value, eo.value, eof.value, body


def check_read_good(eng, f, plain, what, **kw):
    w = ref.Walk(f)
    rc, got, ol, nm, bad, eo, eof, _ = read(eng, f, **kw)
    assert (rc, ol, nm, bad, eo, eof) == (0, len(plain), w.n_members, NONE32, -1, w.eof_marker), (what, kw)
    assert got == plain, (what, kw)


def test_many_member_files(eng):
    """1 ... 1025 members: runs of 28-byte empty members inside one cache line, full 65536-byte members, starts at
    every offset mod 64 -- index against the walk, read against gzip and against the framed gzip read fed with the
    index."""
    for k, n in enumerate(ref.MEMBER_COUNTS):
        f, plain = ref.many_members(n)
        assert gzip.decompress(f) == plain
        check_index(eng, f, n, device=True, shift=k % 16)
        check_read_good(eng, f, plain, n, device=True, shift=(5 * k + 1) % 16, out_shift=k % 8)
        if n in (3, 65, 1025):
            check_index(eng, f, n)
            check_read_good(eng, f, plain, n)
    f, plain = ref.many_members(1025)
    ix = eng.bgzf_index(np.frombuffer(f, np.uint8))
    out, ooff, olen, status = eng.inflate_batch_framed(np.frombuffer(f, np.uint8), ix.member_off, "gzip")
    assert not status.any() and (np.diff(ix.out_off) == olen).all() and (ooff == ix.out_off).all()
    assert out[:int(ooff[-1])].tobytes() == plain


def test_more_candidates_than_the_first_guess(eng):
    """Nothing but empty members: one candidate per 28 bytes, more than the discovery arrays hold at first -- the pass is
    repeated with arrays sized from the count."""
    f = ref.EOF * 6000
    assert 6000 > 4096 + len(f) // 1024
    check_index(eng, f, "6000 markers", device=True, shift=3)
    check_read_good(eng, f, b"", "6000 markers", device=True)


def test_foreign_headers_and_writers(eng):
    for k, (what, f) in enumerate(ref.header_files()):
        plain = gzip.decompress(f)
        for device in (False, True):
            check_index(eng, f, what, device=device, shift=(2 * k + 1) % 16 if device else 0)
            check_read_good(eng, f, plain, what, device=device, shift=(3 * k + 5) % 16)
    assert index(eng, ref.header_files()[4][1])[3] == 0  # without the EOF marker: still fine


def test_input_at_every_device_alignment(eng, oracle, inputs):
    f, _ = ref.build_file(oracle, inputs[65281], 4096)
    for shift in range(16):
        check_index(eng, f, "alignment", device=True, shift=shift)
    for shift in (1, 7, 15):
        check_read_good(eng, f, inputs[65281], "alignment", device=True, shift=shift)


def test_decoys(eng):
    for k, (what, f) in enumerate(ref.decoy_files()):
        plain = gzip.decompress(f)
        for device in (False, True):
            check_index(eng, f, what, device=device, shift=k + 1 if device else 0)
            check_read_good(eng, f, plain, what, device=device, shift=2 * k)


def test_malformed_chains(eng):
    for k, (what, f, err_off, n_good) in enumerate(ref.malformed_files()):
        for device in (False, True):
            shift = (k + 1) % 16 if device else 0
            rc, nm, ob, eof, eo, _, _ = index(eng, f, device=device, shift=shift)
            assert (rc, nm, ob, eo) == (ref.CORRUPT, n_good, 0, err_off), (what, device)
            check_index(eng, f, what, device=device, shift=shift)
            rc, _, ol, nm, bad, eo, _, body = read(eng, f, device=device, shift=shift, cap=8192)
            assert (rc, ol, nm, bad, eo) == (ref.CORRUPT, 0, n_good, n_good, err_off), (what, device)
            assert (body == GUARD).all(), (what, "nothing may be written")


def test_member_failures(eng, oracle):
    for what, f, want_rc, want_bad in ref.failing_files():
        w = ref.Walk(f)
        members = w.members(f)
        for device in (False, True):
            rc, _, ol, nm, bad, eo, eof, body = read(eng, f, device=device, shift=3)
            assert (rc, bad, eo) == (want_rc, want_bad, w.member_off[want_bad]), (what, device, rc, bad, eo)
            assert (ol, nm, eof) == (w.out_bytes, w.n_members, 1), what
            first = None
            for i, m in enumerate(members):  # every member is what the framed gzip read makes of it
                slot = w.out_off[i + 1] - w.out_off[i]
                st, _, want, _ = expected(oracle, m, "gzip", slot, None)
                if st and first is None:
                    first = (st, i)
                if st == 0 or i != want_bad:
                    assert body[w.out_off[i]:w.out_off[i] + len(want)].tobytes() == want, (what, i)
            assert first == (want_rc, want_bad), (what, first)


def test_capacity_and_query(eng, oracle, inputs):
    data = inputs[2 * 65280]
    f, _ = ref.build_file(oracle, data, 4096)
    w = ref.Walk(f)
    for device in (False, True):
        rc, _, ol, nm, bad, eo, eof, body = read(eng, f, device=device, cap=len(data) - 1)
        assert (rc, ol, nm) == (-2, len(data), w.n_members) and (body == GUARD).all(), device
        # the query form: the counts, no arrays
        rc, nm, ob, eof, eo, _, _ = index(eng, f, device=device, query=True)
        assert (rc, nm, ob, eof, eo) == (0, w.n_members, len(data), 1, -1)
        # index_cap one entry short: the counts are set, the arrays untouched
        rc, nm, ob, eof, eo, moff, ooff = index(eng, f, device=device, cap=w.n_members)
        assert (rc, nm, ob) == (-2, w.n_members, len(data)) and (moff == 7).all() and (ooff == 7).all()
    # an empty file: no members
    assert index(eng, b"")[:5] == (0, 0, 0, 0, -1)
    assert read(eng, b"", cap=16)[:7] == (0, b"", 0, 0, NONE32, -1, 0)
    # the optional out-parameters may be NULL
    src = np.frombuffer(f, np.uint8)
    out, ol = np.zeros(len(data), np.uint8), C.c_uint64()
    assert eng._L.flate_hip_bgzf_read(eng._ctx, src.ctypes.data, len(f), out.ctypes.data, len(data), C.byref(ol), None,
                                      None, None, None, 0) == 0 and out.tobytes() == data
    nm, ob = C.c_uint32(), C.c_uint64()
    assert eng._L.flate_hip_bgzf_index(eng._ctx, src.ctypes.data, len(f), 0, None, None, C.byref(nm), C.byref(ob), None,
                                       None, 0) == 0 and (nm.value, ob.value) == (w.n_members, len(data))
    one = np.zeros(4, np.uint64)
    assert eng._L.flate_hip_bgzf_index(eng._ctx, src.ctypes.data, len(f), 4, one.ctypes.data, None, C.byref(nm),
                                       C.byref(ob), None, None, 0) == -1  # one array without the other


def test_existing_framed_calls_still_refuse_the_internal_wrap(eng):
    src, off = np.zeros(64, np.uint8), np.array([0, 64], np.uint64)
    out, ooff = np.zeros(4096, np.uint8), np.zeros(2, np.uint64)
    assert eng._L.flate_hip_deflate_fast_batch_framed(eng._ctx, src.ctypes.data, off.ctypes.data, 1, 3, None, None, 0,
                                                      None, out.ctypes.data, 4096, ooff.ctypes.data, 0) == -1
