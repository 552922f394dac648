"""BGZF files in parts on the GPU: flate_hip_bgzf_reader_* and flate_hip_bgzf_writer_*.  Every call's words and bytes
equal the CPU reference tests/bgzf_parts_ref.py (bgzf_ref's serial walk, zlib's verdicts, bgzf_ref.build_file), for every
file of the corpus and every schedule of parts; the index of the calls is flate_hip_bgzf_index of the whole file; guard
bytes around `out` stay what they were."""
import ctypes as C
import gzip

import numpy as np
import pytest

import bgzf_parts_ref as R
import bgzf_ref as ref
from util import flate

pytestmark = pytest.mark.gpu

DEVICE_PTRS, COMPAT_GO = 1, 2
GUARD = 0xA5


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def big():
    """The 1025-member file (about 0.7 MB), built once."""
    return ref.many_members(1025)


def room(f):
    """"Unbounded": more than any prefix of the file inflates to (the ISIZE sums of the walk as far as it gets)."""
    p, total = 0, 0
    while p < len(f):
        t = ref.member_total(f, p)
        if not t:
            break
        total += int.from_bytes(f[p + t - 4:p + t], "little")
        p += t
    return total + 1


class Reader:
    """flate_hip_bgzf_reader_* through ctypes: read(part, final, out_cap, index_cap) -> R.Read, host or device pointers,
    `in` and `out` at any byte alignment, guard bytes around out[0, out_cap) checked on every call."""

    def __init__(self, eng, device=False, in_shift=0, out_shift=0):
        self.eng, self.L, self.device = eng, eng._L, device
        self.in_shift, self.out_shift = in_shift, out_shift
        self.h = C.c_void_p()
        assert self.L.flate_hip_bgzf_reader_open(eng._ctx, DEVICE_PTRS if device else 0, C.byref(self.h)) == 0

    def read(self, part, final, out_cap=0, index_cap=None):
        part = bytes(part)
        n, s, t = len(part), self.in_shift, self.out_shift
        src = np.frombuffer(b"\0" * s + part + b"\0" * 16, np.uint8).copy()
        obuf = np.full(t + out_cap + 64, GUARD, np.uint8)
        if self.device:
            import torch
            d_in, d_out = torch.from_numpy(src).cuda(), torch.from_numpy(obuf).cuda()
            assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
            in_ptr, out_ptr = d_in.data_ptr() + s, d_out.data_ptr() + t
        else:
            in_ptr, out_ptr = src.ctypes.data + s, obuf.ctypes.data + t
        k_room = max(index_cap or 0, 1)
        moff, ooff = np.full(k_room, 7, np.uint64), np.full(k_room, 7, np.uint64)
        used, ol = C.c_uint64(99), C.c_uint64(99)
        nm, bm, eo, em = C.c_uint32(99), C.c_uint32(99), C.c_int64(99), C.c_int(99)
        rc = self.L.flate_hip_bgzf_reader_read(
            self.h, in_ptr if n else None, n, int(final), out_ptr if out_cap else None, out_cap, C.byref(used), C.byref(ol),
            index_cap or 0, moff.ctypes.data if index_cap is not None else None,
            ooff.ctypes.data if index_cap is not None else None, C.byref(nm), C.byref(bm), C.byref(eo), C.byref(em))
        if self.device:
            import torch
            torch.cuda.synchronize()
            obuf = d_out.cpu().numpy()
        assert (obuf[:t] == GUARD).all() and (obuf[t + out_cap:] == GUARD).all(), "guard bytes touched"
        if rc == R.INVALID:
            return R.Read(rc, 0, 0, 0, R.NONE, -1, 0, None, None, b"")
        k = int(nm.value)
        repeatable = rc == R.OUT_TOO_SMALL and bm.value == R.NONE
        data = b"" if repeatable else obuf[t:t + int(ol.value)].tobytes()
        idx = index_cap is not None
        return R.Read(rc, int(used.value), int(ol.value), k, int(bm.value), int(eo.value), int(em.value),
                      [int(x) for x in moff[:k + 1]] if idx else None, [int(x) for x in ooff[:k + 1]] if idx else None, data)

    def reset(self):
        assert self.L.flate_hip_bgzf_reader_reset(self.h) == 0

    def close(self):
        self.L.flate_hip_bgzf_reader_free(self.h)


def both(eng, f, sizes, grow, out_cap=None, index_cap=None, device=False, in_shift=0, out_shift=0, name=""):
    """One schedule through the GPU reader and the reference: every call's words and bytes are equal.  -> the calls."""
    cap = room(f) if out_cap is None else out_cap
    m, g = R.ReaderModel(f), Reader(eng, device, in_shift, out_shift)
    n_call = [0]

    def read(part, final):
        want = m.read(part, final, cap, index_cap)
        got = g.read(part, final, cap, index_cap)
        assert got == want, (name, n_call[0], len(part), final)
        n_call[0] += 1
        return got
    try:
        return R.feed(read, f, sizes, 4 * len(f) + 64, grow)
    finally:
        g.close()


SMALL_CORPUS = ref.header_files() + ref.decoy_files() + [(w, f) for w, f, _, _ in ref.malformed_files()] + \
    [(w, f) for w, f, _, _ in ref.failing_files()] + [("%d members" % n, ref.many_members(n)[0]) for n in (1, 2, 3)] + \
    [("an empty file", b"")]
IDS = [w for w, _ in SMALL_CORPUS]


@pytest.mark.parametrize("device", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("what,f", SMALL_CORPUS, ids=IDS)
def test_reader_small_corpus(eng, what, f, device):
    """One final part, fixed parts of 1 .. 70000 bytes, two parts at every 37th cut and at every cut of the 60 bytes
    around the first member boundary of the "XLEN > 6" file, a seeded random schedule."""
    window_at = ref.Walk(f).member_off[1] if what.startswith("XLEN > 6") else None
    for name, sizes, grow in R.schedules(f, window_at):
        if device and name == "parts of 1":
            continue  # (a call per byte: with host pointers)
        calls, data, rest = both(eng, f, sizes(), grow, device=device, index_cap=None if device else 2048, name=name)
    w = ref.Walk(f)
    if w.rc == R.OK and not any(R.member_verdict(m)[0] for m in w.members(f)):
        assert calls[-1].rc == R.STREAM_END and data == (gzip.decompress(f) if f else b"") and rest == b""


@pytest.mark.parametrize("n", [65, 1025])
@pytest.mark.parametrize("device", [False, True], ids=["host", "dev"])
def test_reader_many_members(eng, big, n, device):
    """Runs of 28-byte members in one cache line, starts at every offset mod 64, full 65536-byte members: where the
    candidate tiles and the clip can go wrong."""
    f, plain = big if n == 1025 else ref.many_members(n)
    for name, sizes, grow in (("one part", iter(()), 1), ("4096", R.fixed(4096), 4096), ("65536", R.fixed(65536), 65536),
                              ("70000", R.fixed(70000), 70000), ("random", R.random_sizes(n, 200000), 4096)):
        calls, data, rest = both(eng, f, sizes, grow, device=device, index_cap=2048, name=name)
        assert calls[-1].rc == R.STREAM_END and data == plain and calls[-1].eof_marker == 1
    w = ref.Walk(f)
    k = n // 2
    for cap in (0, w.out_off[k] - 1, w.out_off[k]):
        _rooms(eng, f, cap, None, device, plain)
    for icap in (1, 3):
        _rooms(eng, f, room(f), icap, device, plain)


def _rooms(eng, f, cap, index_cap, device, plain):
    """A reader with little room: every call equals the reference; a repeatable -2 really changes nothing -- the same
    call with room for the member delivers what the reference says."""
    m, g = R.ReaderModel(f), Reader(eng, device)
    out, buf, cur, moff = [], f, cap, [0]
    try:
        for _ in range(4 * len(f)):
            want, got = m.read(buf, True, cur, index_cap), g.read(buf, True, cur, index_cap)
            assert got == want
            if got.rc == R.OUT_TOO_SMALL and got.bad_member == R.NONE:
                if index_cap == 1:
                    return  # (an index of one entry holds no member)
                assert got.in_used == 0 and got.out_len > cur
                cur = got.out_len
                continue
            out.append(got.data)
            if index_cap is not None:
                assert got.member_off[0] == moff[-1]
                moff += got.member_off[1:]
            buf, cur = buf[got.in_used:], cap
            if got.rc != R.OK:
                break
        assert got.rc == R.STREAM_END and b"".join(out) == plain
        if index_cap is not None:
            assert moff == list(ref.Walk(f).member_off)
    finally:
        g.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "dev"])
def test_reader_small_rooms(eng, device):
    f = dict(SMALL_CORPUS)["a foreign writer: fixed and dynamic blocks"]
    w = ref.Walk(f)
    plain = gzip.decompress(f)
    for cap in (0, w.out_off[1] - 1, w.out_off[2] - 1, w.out_off[2]):
        _rooms(eng, f, cap, None, device, plain)
    for icap in (1, 3):
        _rooms(eng, f, room(f), icap, device, plain)


@pytest.mark.parametrize("device", [False, True], ids=["host", "dev"])
def test_reader_alignments(eng, device):
    """`in` and `out` at every address alignment 0..15, two parts cut inside the second member."""
    f = dict(SMALL_CORPUS)["XLEN > 6 and padding subfields behind BC"]
    cut = ref.Walk(f).member_off[1] + 9
    for a in range(16):
        both(eng, f, R.cut_sizes([cut]), 64, device=device, in_shift=a, out_shift=(5 * a + 3) % 16, name="shift %d" % a)


def test_reader_decoy_pointing_past_the_part(eng):
    """A decoy whose claimed end lies behind the part but inside the file: a candidate of the whole file and of later
    parts, none of this part.  The result is the walk's."""
    f = dict(SMALL_CORPUS)["a decoy chain that reaches in_len on its own"]
    at = 18 + 5 + 100
    assert at + ref.member_total(f, at) == len(f)
    for cut in (at + 40, 31 + 600, 31 + 600 + 50, len(f) - 28, len(f) - 1):
        assert ref.member_total(f[:cut], at) == 0
        for device in (False, True):
            calls, data, _ = both(eng, f, R.cut_sizes([cut]), 64, device=device, index_cap=16)
            assert calls[-1].rc == R.STREAM_END and data == gzip.decompress(f)


def test_reader_index_is_the_whole_files(eng, big):
    f, _ = big
    n = C.c_uint32(0)
    ob, em, eo = C.c_uint64(0), C.c_int(0), C.c_int64(0)
    moff, ooff = np.zeros(1026, np.uint64), np.zeros(1026, np.uint64)
    src = np.frombuffer(f, np.uint8)
    assert eng._L.flate_hip_bgzf_index(eng._ctx, src.ctypes.data, len(f), 1026, moff.ctypes.data, ooff.ctypes.data,
                                       C.byref(n), C.byref(ob), C.byref(em), C.byref(eo), 0) == 0
    calls, _, _ = both(eng, f, R.fixed(100000), 4096, index_cap=2048)
    gm, go = [0], [0]
    for c in calls:
        assert c.member_off[0] == gm[-1] and c.out_off[0] == go[-1]
        gm += c.member_off[1:]
        go += c.out_off[1:]
    assert gm == [int(x) for x in moff] and go == [int(x) for x in ooff] and n.value == 1025


def test_reader_other_calls_between_two_reads_change_nothing(eng):
    f = dict(SMALL_CORPUS)["a foreign writer: fixed and dynamic blocks"]
    other = ref.many_members(65)[0]
    m, g = R.ReaderModel(f), Reader(eng)
    try:
        a = 1500
        assert g.read(f[:a], False, room(f)) == m.read(f[:a], False, room(f))
        used = m.consumed
        got = eng.bgzf_read(np.frombuffer(other, np.uint8))
        assert bytes(got[0]) == ref.many_members(65)[1]
        want = m.read(f[used:], True, room(f))
        assert g.read(f[used:], True, room(f)) == want and want.rc == R.STREAM_END
    finally:
        g.close()


def test_reader_reset_and_sticky_words(eng):
    bad = dict(SMALL_CORPUS)["a flipped CRC"]
    good = dict(SMALL_CORPUS)["no EOF marker"]
    g = Reader(eng)
    try:
        m = R.ReaderModel(bad)
        first = g.read(bad, True, room(bad), 8)
        assert first == m.read(bad, True, room(bad), 8) and first.rc == R.CORRUPT and first.bad_member == 1
        for _ in range(2):  # sticky: word for word, nothing used, nothing delivered
            again = g.read(bad, True, room(bad), 8)
            assert again == m.read(bad, True, room(bad), 8)
            assert (again.rc, again.bad_member, again.err_off, again.in_used, again.out_len) == \
                (first.rc, first.bad_member, first.err_off, 0, 0)
        g.reset()
        m = R.ReaderModel(good)
        got = g.read(good, True, room(good), 8)
        assert got == m.read(good, True, room(good), 8) and got.rc == R.STREAM_END and got.data == gzip.decompress(good)
        assert g.read(b"", True, 0) == m.read(b"", True, 0)  # the end is sticky too
        g.reset()
        assert g.read(b"", True, 0).rc == R.STREAM_END  # an empty file
        g.reset()
        assert g.read(good, True, room(good), 0).rc == R.INVALID  # index arrays without room
        assert g.read(good, True, room(good), 8).rc == R.STREAM_END  # ... and nothing had changed
    finally:
        g.close()


def test_engine_reader(eng):
    """FlateEngine.open_bgzf_reader: numpy and CUDA tensors, the named-tuple result, the index."""
    import torch
    f, plain = ref.many_members(65)
    w = ref.Walk(f)
    for device in (False, True):
        rd = eng.open_bgzf_reader(device=device)
        buf, pos, out, moff = b"", 0, [], [0]
        while True:
            buf, pos = buf + f[pos:pos + 30000], min(len(f), pos + 30000)
            a = np.frombuffer(buf, np.uint8)
            used, got, res = rd.read(torch.from_numpy(a.copy()).cuda() if device else a, final=pos == len(f), index=True)
            out.append(bytes(got.cpu().numpy()) if device else bytes(got))
            moff += [int(x) for x in res.member_off[1:]]
            buf = buf[used:]
            if res.rc != 0:
                break
        assert res.rc == 1 and res.eof_marker == 1 and b"".join(out) == plain and moff == list(w.member_off)
        rd.reset()
        rd.close()


# ---- the writer ----

@pytest.fixture(scope="module")
def inputs():
    return ref.write_inputs()


class Writer:
    def __init__(self, eng, bb, compat, device=False, out_shift=0):
        self.eng, self.L, self.device, self.bb, self.out_shift = eng, eng._L, device, bb, out_shift
        self.h = C.c_void_p()
        flags = (COMPAT_GO if compat else 0) | (DEVICE_PTRS if device else 0)
        assert self.L.flate_hip_bgzf_writer_open(eng._ctx, bb, flags, C.byref(self.h)) == 0

    def write(self, part, final, cap=None):
        part = bytes(part)
        n, t = len(part), self.out_shift
        if cap is None:
            cap = self.L.flate_hip_bgzf_writer_bound(n, self.bb)
        src = np.frombuffer(part + b"\0" * 16, np.uint8).copy()
        obuf = np.full(t + cap + 64, GUARD, np.uint8)
        if self.device:
            import torch
            d_in, d_out = torch.from_numpy(src).cuda(), torch.from_numpy(obuf).cuda()
            in_ptr, out_ptr = d_in.data_ptr(), d_out.data_ptr() + t
        else:
            in_ptr, out_ptr = src.ctypes.data, obuf.ctypes.data + t
        moff = np.full(n // (self.bb or ref.BLOCK_DEFAULT) + 2, 7, np.uint64)
        used, ol, nb = C.c_uint64(99), C.c_uint64(99), C.c_uint32(99)
        rc = self.L.flate_hip_bgzf_writer_write(self.h, in_ptr if n else None, n, int(final), out_ptr, cap, C.byref(used),
                                                C.byref(ol), moff.ctypes.data, C.byref(nb))
        if self.device:
            import torch
            torch.cuda.synchronize()
            obuf = d_out.cpu().numpy()
        assert (obuf[:t] == GUARD).all() and (obuf[t + cap:] == GUARD).all(), "guard bytes touched"
        if rc < 0:
            return R.Write(rc, int(used.value), int(ol.value), int(nb.value), None, b"")
        k = int(nb.value)
        return R.Write(rc, int(used.value), int(ol.value), k, [int(x) for x in moff[:k + 1]],
                       obuf[t:t + int(ol.value)].tobytes())

    def close(self):
        self.L.flate_hip_bgzf_writer_free(self.h)


def writer_schedules(n, step):
    return [("one part", lambda: iter(()), 1), ("one block", lambda: R.fixed(step), step),
            ("two blocks + 5", lambda: R.fixed(2 * step + 5), step), ("a block - 1", lambda: R.fixed(max(step - 1, 1)), max(step - 1, 1)),
            ("random", lambda: R.random_sizes(n + step, 3 * step + 2), step)]


@pytest.mark.parametrize("compat", [0, 1])
@pytest.mark.parametrize("bb", [0, 4096, 1])
def test_writer_any_cut_writes_the_same_file(eng, oracle, inputs, bb, compat):
    shift = 0
    for n, data in inputs.items():
        if bb == 1 and n > 300:
            continue
        step = bb or ref.BLOCK_DEFAULT
        want, off = ref.build_file(oracle, data, bb, compat)
        for device in (False, True):
            for name, sizes, grow in writer_schedules(n, step):
                if bb == 4096 and n > 70000 and name != "two blocks + 5" and device:
                    continue  # (the long inputs in 4 KiB blocks: one schedule with device pointers)
                m, g = R.WriterModel(oracle, data, bb, compat), Writer(eng, bb, compat, device, shift % 8)
                shift += 1

                def write(part, final):
                    w, got = m.write(part, final), g.write(part, final)
                    assert got == w, (n, name, device, len(part), final)
                    return got
                try:
                    calls, got, rest = R.feed(write, data, sizes(), 4 * n + 64, grow)
                    assert got == want and rest == b"" and calls[-1].rc == R.STREAM_END
                    assert g.write(b"x", False).rc == R.INVALID and g.write(b"", True).rc == R.INVALID  # after the end
                finally:
                    g.close()
        assert gzip.decompress(want) == data


@pytest.mark.parametrize("device", [False, True], ids=["host", "dev"])
def test_writer_too_little_room_is_repeatable(eng, oracle, inputs, device):
    data = inputs[2 * 65280]
    want, off = ref.build_file(oracle, data, 0, 0)
    g = Writer(eng, 0, 0, device)
    try:
        a = g.write(data[:65280 + 7], False)
        assert a.rc == R.OK and a.in_used == 65280 and a.data == want[:int(off[1])] and a.member_off == [0, int(off[1])]
        rest = data[65280:]
        need = int(off[2] - off[1]) + 28
        for cap in (0, 27, need - 28, need - 1):
            assert g.write(rest, True, cap).rc == R.OUT_TOO_SMALL
        b = g.write(rest, True, need)
        assert b.rc == R.STREAM_END and a.data + b.data == want and b.member_off == [int(off[1]), int(off[2])]
    finally:
        g.close()


def test_writer_marker_alone_and_reset(eng):
    g = Writer(eng, 0, 0)
    try:
        assert g.write(b"abc", False) == R.Write(R.OK, 0, 0, 0, [0], b"")  # less than a block: nothing
        w = g.write(b"", True, 27)
        assert w.rc == R.OUT_TOO_SMALL
        w = g.write(b"", True)
        assert w == R.Write(R.STREAM_END, 0, 28, 0, [0], ref.EOF)
        assert g.write(b"", True).rc == R.INVALID
        assert eng._L.flate_hip_bgzf_writer_reset(g.h) == 0
        assert g.write(b"", True).data == ref.EOF
    finally:
        g.close()


def test_round_trip_writer_parts_into_reader_parts(eng, inputs):
    """The writer's parts fed straight into the reader's parts, cut differently, through the engine's classes."""
    data = inputs[3 * 65280 + 5]
    wr, rd = eng.open_bgzf_writer(block_bytes=4096), eng.open_bgzf_reader()
    file_parts, pos, pending = [], 0, b""
    for step in (10000, 1, 4095, 4097, 70000, len(data)):
        pending += data[pos:pos + step]
        pos = min(len(data), pos + step)
        used, out, res = wr.write(np.frombuffer(pending, np.uint8), final=pos == len(data), index=True)
        pending = pending[used:]
        file_parts.append(bytes(out))
        if res.rc == 1:
            break
    f = b"".join(file_parts)
    assert f == bytes(eng.bgzf_write(np.frombuffer(data, np.uint8), block_bytes=4096))
    out, buf, pos = [], b"", 0
    rng = np.random.default_rng(5)
    while True:
        step = int(rng.integers(1, 50000))
        buf, pos = buf + f[pos:pos + step], min(len(f), pos + step)
        used, got, res = rd.read(np.frombuffer(buf, np.uint8), final=pos == len(f))
        out.append(bytes(got))
        buf = buf[used:]
        if res.rc != 0:
            break
    assert res.rc == 1 and res.eof_marker == 1 and b"".join(out) == data and gzip.decompress(f) == data
    wr.close()
    rd.close()
