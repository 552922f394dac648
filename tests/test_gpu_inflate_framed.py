"""flate_hip_inflate_batch_framed on the GPU: zlib and gzip members parsed, decoded and checked against their trailers
by one call.  Every expectation comes from the CPU: the host mirrors' header helpers (parse_container_header,
zlib_member_header, zlib_dict_ids), the oracle's inflate on the exact payload range (with the member's dictionary)
and the oracle's Adler-32 / CRC-32.  Checked per member: the bytes delivered, out_len, status, err_off, dict_used --
and the call's return value, the first non-zero status."""
import ctypes as C
import gzip
import itertools
import struct
import zlib

import numpy as np
import pytest

from framed_read_ref import (FILLS, LENGTHS, NO_DICT, bad_members, dict_batch, engine, expected, gzmember,
                             make_payloads, oracle_member, zmember)
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
def payloads():
    """One payload per length of LENGTHS, mixed fills (computed once, shared, never changed)."""
    return make_payloads()


def call(eng, members, wrap, slots, dicts=None, device=False, in_shift=0, out_shift=0, flags=0, want_used=True):
    """One flate_hip_inflate_batch_framed call through ctypes.  Returns (rc, out bytes of the slots' range, out_off,
    out_len, status, err_off, dict_used); the guard bytes around the output must have stayed what they were."""
    n = len(members)
    in_off = np.zeros(n + 1, np.uint64)
    np.cumsum(np.array([len(m) for m in members], dtype=np.uint64), out=in_off[1:])
    out_off = np.zeros(n + 1, np.uint64)
    np.cumsum(np.array(slots, dtype=np.uint64), out=out_off[1:])
    blob = np.frombuffer(b"\0" * in_shift + b"".join(members) + b"\0" * 16, np.uint8).copy()
    total = int(out_off[-1])
    obuf = np.full(out_shift + total + 64, GUARD, np.uint8)
    out_len = np.zeros(max(n, 1), np.uint64)
    status = np.full(max(n, 1), 99, np.int32)
    err_off = np.full(max(n, 1), 77, np.int64)
    used = np.full(max(n, 1), 12345, np.uint32)
    dk = engine._DictArgs(dicts, None, n, device) if dicts else None
    if device:
        import torch
        d_in, d_out = torch.from_numpy(blob).cuda(), torch.from_numpy(obuf).cuda()
        in_ptr, out_ptr = d_in.data_ptr() + in_shift, d_out.data_ptr() + out_shift
        assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    else:
        in_ptr, out_ptr = blob.ctypes.data + in_shift, obuf.ctypes.data + out_shift
    size_only = bool(flags & SIZE_ONLY)
    rc = eng._L.flate_hip_inflate_batch_framed(
        eng._ctx, in_ptr, in_off.ctypes.data, n, WRAP[wrap], dk.ptr if dk else None, dk.off_ptr if dk else None,
        dk.n_dicts if dk else 0, None if size_only else out_ptr, None if size_only else out_off.ctypes.data,
        out_len.ctypes.data, status.ctypes.data, err_off.ctypes.data, used.ctypes.data if want_used else None,
        flags | (DEVICE_PTRS if device else 0))
    if device:
        import torch
        torch.cuda.synchronize()
        obuf = d_out.cpu().numpy()
    assert (obuf[:out_shift] == GUARD).all() and (obuf[out_shift + total:] == GUARD).all(), "guard bytes touched"
    return rc, obuf[out_shift:out_shift + total], out_off, out_len[:n], status[:n], err_off[:n], used[:n]


def check(oracle, eng, members, wrap, slots, dicts=None, **kw):
    rc, out, ooff, olen, status, err, used = call(eng, members, wrap, slots, dicts, **kw)
    first = 0
    for i, m in enumerate(members):
        st, eo, want, j = expected(oracle, m, wrap, slots[i], dicts)
        got = (int(status[i]), int(err[i]), int(olen[i]), int(used[i]))
        assert got == (st, eo, len(want), j), (wrap, i, got, (st, eo, len(want), j), len(m), slots[i])
        assert out[int(ooff[i]):int(ooff[i]) + int(olen[i])].tobytes() == want, (wrap, i)
        if first == 0:
            first = st
    assert rc == first, (rc, first)
    return status


@pytest.fixture(scope="module")
def round_trip(eng, oracle, payloads):
    """{wrap: (members, slots)}: every payload as the GPU's own member and as the oracle's, each with three slots."""
    out = {}
    for wrap in ("zlib", "gzip"):
        data = np.frombuffer(b"".join(payloads) + b"\0", np.uint8)
        off = np.zeros(len(payloads) + 1, np.uint64)
        np.cumsum(np.array([len(p) for p in payloads], dtype=np.uint64), out=off[1:])
        framed, foff = eng.deflate_batch_framed(data, off, wrap)
        members, slots = [], []
        for i, p in enumerate(payloads):
            own = framed[int(foff[i]):int(foff[i + 1])].tobytes()
            assert own == oracle_member(oracle, wrap, p)  # (the write side's own test; here only a precondition)
            foreign = zmember(p, level=1 + i % 9) if wrap == "zlib" else gzmember(p, flg=8 if i % 2 else 0)
            for m in (own, foreign):
                for extra in (0, 1, 70000):  # the last: two whole clipped-away pieces behind the data
                    members.append(m)
                    slots.append(len(p) + extra)
        out[wrap] = (members, slots)
    return out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_round_trip(eng, oracle, round_trip, wrap, device):
    members, slots = round_trip[wrap]
    status = check(oracle, eng, members, wrap, slots, device=device)
    assert (status == 0).all()


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_device_pointers_at_every_alignment(eng, oracle, payloads, wrap):
    pick = [p for p in payloads if len(p) in (0, 1, 17, 1025, 65537)]
    members = [oracle_member(oracle, wrap, p) for p in pick]
    slots = [len(p) + (i % 3) for i, p in enumerate(pick)]
    for a in range(16):
        status = check(oracle, eng, members, wrap, slots, device=True, in_shift=a, out_shift=(5 * a + 3) % 16)
        assert (status == 0).all()


DECODERS = {
    "wave_per_stream": {"inflate_spec": 0},
    "speculative": {"inflate_spec": 2},
    "lanes16_row0": {"inflate_spec": 0, "inflate_simt_min_streams": 1, "inflate_lanes": 16, "inflate_row_dwords": 0},
    "lanes16_row8": {"inflate_spec": 0, "inflate_simt_min_streams": 1, "inflate_lanes": 16, "inflate_row_dwords": 8},
    "lanes64_row0": {"inflate_spec": 0, "inflate_simt_min_streams": 1, "inflate_lanes": 64, "inflate_row_dwords": 0},
    "lanes64_row8": {"inflate_spec": 0, "inflate_simt_min_streams": 1, "inflate_lanes": 64, "inflate_row_dwords": 8},
}


@pytest.fixture(scope="module", params=list(DECODERS))
def decoder_eng(request):
    e = flate.FlateEngine(0)
    for k, v in DECODERS[request.param].items():
        e.set_option(k, v)
    yield e
    e.close()


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_every_batch_decoder_plain(decoder_eng, oracle, round_trip, wrap):
    members, slots = round_trip[wrap]
    # (with a member cut short among them: the raw stream's end is where every decoder must stop)
    tl = 4 if wrap == "zlib" else 8
    cut = members[40][:-tl - 5] + members[40][-tl:]
    status = check(oracle, decoder_eng, members[:60] + [cut] + members[60:], wrap, slots[:60] + [slots[40]] + slots[60:],
                   device=True)
    assert status[60] == -7 and (np.delete(status, 60) == 0).all()


def test_every_batch_decoder_with_dictionaries(decoder_eng, oracle):
    members, slots, dicts = dict_batch(oracle)
    status = check(oracle, decoder_eng, members, "zlib", slots, dicts, device=True)
    assert status[5] == -4 and (np.delete(status, 5) == 0).all()


def test_2304_members_of_4_kib_at_the_default_options(eng, oracle):
    n, blen = 2304, 4096
    data = flate.synth("text", n, blen)
    framed, foff = eng.deflate_batch_framed(data, flate.uniform_offsets(n, blen), "gzip")
    members = [framed[int(foff[i]):int(foff[i + 1])].tobytes() for i in range(n)]
    rc, out, ooff, olen, status, err, used = call(eng, members, "gzip", [blen + (i % 2) for i in range(n)], device=True)
    assert rc == 0 and (status == 0).all() and (olen == blen).all() and (used == NO_DICT).all()
    for i in range(n):
        assert out[int(ooff[i]):int(ooff[i]) + blen].tobytes() == data[i * blen:(i + 1) * blen].tobytes(), i


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_long_outputs(eng, oracle, wrap):
    """Fold runs longer than one piece (65 pieces) and the fold's table path (257 pieces)."""
    a = bytes(64 * 65536 + 1)
    b = flate.synth("text", 1, 257 * 65536).tobytes()
    if wrap == "zlib":
        members = [zlib.compress(a, 1), zlib.compress(b, 1)]
    else:
        members = [gzip.compress(a, 1), gzip.compress(b, 1)]
    for slots in ([len(a), len(b)], [len(a) + 70000, len(b) + 1]):
        rc, out, ooff, olen, status, err, used = call(eng, members, wrap, slots, device=True)
        assert rc == 0 and status.tolist() == [0, 0] and olen.tolist() == [len(a), len(b)]
        assert zlib.crc32(out[:len(a)].tobytes()) == zlib.crc32(a)
        assert out[int(ooff[1]):int(ooff[1]) + len(b)].tobytes() == b
    # and a flipped bit of the long member's checksum is seen
    bad = bytearray(members[1])
    assert expected(oracle, bytes(bad), wrap, len(b), None)[0] == 0
    t = -1 if wrap == "zlib" else -5
    bad[t] ^= 1
    rc, out, ooff, olen, status, err, used = call(eng, [members[0], bytes(bad)], wrap, [len(a), len(b)], device=True)
    assert rc == -4 and status.tolist() == [0, -4] and int(err[1]) == len(bad) and int(olen[1]) == len(b)


def test_foreign_members(eng, oracle, payloads):
    p = payloads[LENGTHS.index(65537)]
    q = payloads[LENGTHS.index(1025)]
    zl = [zlib.compress(p, lvl) for lvl in (1, 6, 9)] + [zlib.compress(q, 9), zlib.compress(b"")]
    status = check(oracle, eng, zl, "zlib", [len(p)] * 3 + [len(q), 0])
    assert (status == 0).all()
    gz = [gzip.compress(p), gzip.compress(q, 1), gzip.compress(b"")]
    slots = [len(p), len(q), 0]
    for bits in itertools.product((0, 2), (0, 4), (0, 8), (0, 16)):  # every combination of the optional fields
        gz.append(gzmember(q, flg=sum(bits), extra=b"\x01\x02" * 21))
        slots.append(len(q) + 1)
    gz.append(gzmember(q, flg=4, extra=b""))  # FEXTRA of length 0
    gz.append(gzmember(q, flg=4 | 8 | 16 | 2, extra=b"", name=b"\0", comment=b"\0"))
    slots += [len(q), len(q)]
    for device in (False, True):
        status = check(oracle, eng, gz, "gzip", slots, device=device)
        assert (status == 0).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_zlib_dictionaries(eng, oracle, device):
    members, slots, dicts = dict_batch(oracle)
    rc, out, ooff, olen, status, err, used = call(eng, members, "zlib", slots, dicts, device=device)
    assert used[1:5].tolist() == [1, NO_DICT, 2, 0]  # (the duplicate of dictionary 0 is never chosen: the first wins)
    assert 3 not in used.tolist() and int(used[5]) == NO_DICT and int(status[5]) == -4
    status = check(oracle, eng, members, "zlib", slots, dicts, device=device)
    assert (np.delete(status, 5) == 0).all()
    # FDICT with n_dicts == 0: every member that names a dictionary is a bad header, the others are untouched
    status = check(oracle, eng, members, "zlib", slots, None, device=device)
    fdict = np.array([bool(m[1] & 0x20) for m in members])
    assert (status[fdict] == -4).all() and (status[~fdict] == 0).all()
    # members the GPU wrote with dictionaries come back with them (dict_used may be NULL)
    pay = [flate.synth("text", 1, n, seed=90 + i).tobytes() for i, n in enumerate((3000, 200, 70000, 4096))]
    data = np.frombuffer(b"".join(pay) + b"\0", np.uint8)
    off = np.zeros(len(pay) + 1, np.uint64)
    np.cumsum(np.array([len(p) for p in pay], dtype=np.uint64), out=off[1:])
    of = [1, NO_DICT, 0, 4]
    framed, foff = eng.deflate_batch_framed(data, off, "zlib", compat_go=True, zdicts=dicts, dict_of=of)
    own = [framed[int(foff[i]):int(foff[i + 1])].tobytes() for i in range(len(pay))]
    rc, out, ooff, olen, status, err, used = call(eng, own, "zlib", [len(p) for p in pay], dicts, device=device)
    assert rc == 0 and used.tolist() == of and out.tobytes() == b"".join(pay)
    rc, out, ooff, olen, status, err, used = call(eng, own, "zlib", [len(p) for p in pay], dicts, device=device,
                                                  want_used=False)
    assert rc == 0 and out.tobytes() == b"".join(pay) and (used == 12345).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_bad_members_beside_good_ones(eng, oracle, payloads, wrap, device):
    cases = bad_members(oracle, wrap, payloads)
    members, slots = [m for _, m, _ in cases], [s for _, _, s in cases]
    status = check(oracle, eng, members, wrap, slots, device=device)
    by = {what: int(status[i]) for i, (what, _, _) in enumerate(cases)}
    for i, (what, _, _) in enumerate(cases):
        assert (int(status[i]) == 0) == what.startswith("good"), (what, int(status[i]))
    assert by["a payload cut short"] == -7 and by["a payload cut to nothing"] == -7
    assert by["a slot too small"] == -2 and by["a corrupt payload"] == -4
    assert by["a flipped payload byte that still decodes"] == -4 and by["a flipped checksum bit"] == -4


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_size_only(eng, oracle, payloads, wrap):
    cases = bad_members(oracle, wrap, payloads)
    members = [m for _, m, _ in cases]
    for device in (False, True):
        rc, _, _, olen, status, err, used = call(eng, members, wrap, [0] * len(members), device=device, flags=SIZE_ONLY)
        first = 0
        for i, (what, m, _) in enumerate(cases):
            st, eo, want, j = expected(oracle, m, wrap, 1 << 20, None, size_only=True)
            assert (int(status[i]), int(err[i]), int(olen[i])) == (st, eo, len(want)), (what, i)
            first = first or st
        assert rc == first


def test_no_members_and_refused_arguments(eng, oracle, payloads):
    L, ctx = eng._L, eng._ctx
    m = oracle_member(oracle, "zlib", payloads[3])
    buf = np.frombuffer(m + b"\0" * 16, np.uint8).copy()
    off = np.array([0, len(m)], np.uint64)
    ooff = np.array([0, 64], np.uint64)
    out = np.zeros(80, np.uint8)
    olen, st, eo, used = np.zeros(1, np.uint64), np.zeros(1, np.int32), np.zeros(1, np.int64), np.zeros(1, np.uint32)
    d = np.frombuffer(b"0123456789" * 4, np.uint8).copy()
    doff = np.array([0, 40], np.uint64)

    def f(n=1, wrap=1, dicts=None, dict_off=None, n_dicts=0, out_len=olen, flags=0, in_=buf):
        return L.flate_hip_inflate_batch_framed(
            ctx, in_.ctypes.data if in_ is not None else None, off.ctypes.data, n, wrap,
            dicts.ctypes.data if dicts is not None else None, dict_off.ctypes.data if dict_off is not None else None,
            n_dicts, out.ctypes.data, ooff.ctypes.data, out_len.ctypes.data if out_len is not None else None,
            st.ctypes.data, eo.ctypes.data, used.ctypes.data, flags)
    for wrap in (0, 1, 2):
        assert f(n=0, wrap=wrap) == 0
    assert f() == 0 and int(olen[0]) == len(payloads[3]) and out[:int(olen[0])].tobytes() == payloads[3]
    assert f(wrap=3) == -1 and f(wrap=0xFFFFFFFF) == -1
    assert f(out_len=None) == -1 and f(in_=None) == -1                      # the raw call's checks
    assert f(wrap=2, dicts=d, dict_off=doff, n_dicts=1) == -1               # gzip has no preset dictionary
    assert f(wrap=2, dicts=d) == -1 and f(wrap=2, dict_off=doff) == -1 and f(wrap=2, n_dicts=1) == -1
    assert f(wrap=0, dicts=d, dict_off=doff, n_dicts=1) == -1 and f(wrap=0, n_dicts=1) == -1
    assert f(dicts=d, dict_off=np.array([0, 40, 30], np.uint64), n_dicts=2) == -1   # not monotone
    assert f(dicts=None, dict_off=doff, n_dicts=1) == -1                    # non-empty dictionaries without bytes
    assert f(dicts=d, dict_off=None, n_dicts=1) == -1
    assert f(dicts=None, dict_off=np.array([7, 7], np.uint64), n_dicts=1) == 0      # (an empty one needs none)
    assert f(dicts=d, dict_off=doff, n_dicts=1) == 0


def test_wrap_raw_is_the_raw_call(eng, oracle, payloads):
    raws = [oracle.deflate(np.frombuffer(p, np.uint8)) for p in payloads[:12]]
    raws.insert(4, raws[9][:-5])
    raws.insert(7, b"\x07\x00")
    slots = [LENGTHS[11]] * len(raws)
    rc, out, ooff, olen, status, err, used = call(eng, raws, "raw", slots, device=True)
    data = np.frombuffer(b"".join(raws) + b"\0" * 16, np.uint8)
    off = np.zeros(len(raws) + 1, np.uint64)
    np.cumsum(np.array([len(r) for r in raws], dtype=np.uint64), out=off[1:])
    out2, ooff2, olen2, status2, err2 = eng.inflate_batch(data, off, slots, check=False)
    assert status.tolist() == status2.tolist() and err.tolist() == err2.tolist() and olen.tolist() == olen2.tolist()
    assert rc == next((int(s) for s in status if s), 0) and (used == NO_DICT).all()
    for i in range(len(raws)):
        a = int(ooff[i])
        assert out[a:a + int(olen[i])].tobytes() == out2[a:a + int(olen[i])].tobytes()


@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_engine_method_keeps_data_on_the_device(eng, payloads, wrap):
    """FlateEngine.inflate_batch_framed on a CUDA tensor -- what deflate_batch_framed left there -- without out_sizes
    (zlib: the size-only pass of the same call; gzip: the ISIZEs, gathered on the device) and into out=."""
    import torch
    data = np.frombuffer(b"".join(payloads) + b"\0", np.uint8).copy()
    off = np.zeros(len(payloads) + 1, np.uint64)
    np.cumsum(np.array([len(p) for p in payloads], dtype=np.uint64), out=off[1:])
    d_framed, foff = eng.deflate_batch_framed(torch.from_numpy(data).cuda(), off, wrap)
    assert d_framed.is_cuda
    dst = torch.full((int(off[-1]) + 100,), GUARD, dtype=torch.uint8, device="cuda")
    out, ooff, olen, status = eng.inflate_batch_framed(d_framed, foff, wrap, out=dst)
    assert out is dst and (status == 0).all() and ooff.tolist() == off.tolist()
    assert olen.tolist() == [len(p) for p in payloads]
    back = dst.cpu().numpy()
    assert back[:int(off[-1])].tobytes() == b"".join(payloads) and (back[int(off[-1]):] == GUARD).all()
    err_off, used = eng.last_framed_read
    assert (used == NO_DICT).all()
    # the same from host memory
    out, ooff, olen, status = eng.inflate_batch_framed(d_framed.cpu().numpy(), foff, wrap)
    assert (status == 0).all() and out[:int(ooff[-1])].tobytes() == b"".join(payloads)
