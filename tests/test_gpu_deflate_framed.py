"""GPU tests of zlib / gzip members written through the C ABI (flate_hip_deflate_fast_batch_framed,
flate_hip_deflate_fast_spliced_framed): every output is compared BYTE FOR BYTE with what the CPU makes --
    plain members       pyoracle.frame(kind, pyoracle.deflate(p, compat), p)
    dictionary members  zlib_dict_header(d) + deflate_dict(p, d, compat) + adler32(p)   (tests/deflate_dict_ref.py)
    the spliced form    pyoracle.frame(kind, pyoracle.deflate_spliced(...)[0], all the bytes)
-- and read back by zlib / gzip on the CPU.  The expectations are computed once per module."""
import gzip
import importlib
import zlib

import numpy as np
import pytest

from deflate_dict_ref import deflate_dict
from util import flate, make_streams

pytestmark = pytest.mark.gpu

engine = importlib.import_module("moonbit-flate_amd.engine")
NO_DICT = flate.NO_DICT
E_INVALID, E_OUT_TOO_SMALL = -1, -2
WRAPS = ["zlib", "gzip"]
MODES = [False, True]  # compat_go
HLEN = {"zlib": 2, "gzip": 10}
TLEN = {"zlib": 4, "gzip": 8}
# the block-policy edges of enc_speed (17, 128, 65535), the Adler block size (5552), the checksum's 64 KiB piece
EDGE_LENS = [0, 1, 16, 17, 127, 128, 129, 5552, 65534, 65535, 65536, 65537, 131070, 200000]
SPLICE_LENS = [0, 1, 17, 40000, 65535, 65536, 131071, 0, 200]
GUARD = 64


@pytest.fixture(scope="module")
def eng():
    flate.build()
    e = flate.FlateEngine(0)
    yield e
    e.close()


def fill(k, n):
    """Fills cycle through synthetic text, zeros, random bytes and 0xff."""
    if n == 0:
        return b""
    kind = ["text", "zero", "rand", "ff"][k % 4]
    if kind == "ff":
        return b"\xff" * n
    data, _ = make_streams([(kind, n)], seed=50 + k)
    return data[:n].tobytes()


def words(seed, n):
    return flate.synth("text", 1, n, seed=seed).tobytes() if n else b""


def pack(blobs):
    off = np.zeros(len(blobs) + 1, np.uint64)
    np.cumsum(np.array([len(b) for b in blobs], dtype=np.uint64), out=off[1:])
    return np.frombuffer(b"".join(blobs) + b"\0" * 16, dtype=np.uint8).copy(), off


def kind_of(oracle, wrap):
    return oracle.FRAME_ZLIB if wrap == "zlib" else oracle.FRAME_GZIP


def cpu_read(wrap, member):
    return zlib.decompress(member) if wrap == "zlib" else gzip.decompress(member)


class Batch:
    """A batch, its raw streams and its members as the CPU makes them, per compat mode and wrap."""

    def __init__(self, oracle, payloads, modes=MODES):
        self.payloads = payloads
        self.data, self.off = pack(payloads)
        self.raw = {go: [oracle.deflate(p, compat=1 if go else 0) for p in payloads] for go in modes}
        self.members = {(w, go): [oracle.frame(kind_of(oracle, w), r, p) for r, p in zip(self.raw[go], payloads)]
                        for w in WRAPS for go in modes}

    def want(self, wrap, go):
        m = self.members[(wrap, go)]
        off = np.zeros(len(m) + 1, np.uint64)
        np.cumsum(np.array([len(x) for x in m], dtype=np.uint64), out=off[1:])
        return b"".join(m), off


@pytest.fixture(scope="module")
def edge(oracle):
    return Batch(oracle, [fill(k, n) for k, n in enumerate(EDGE_LENS)])


@pytest.fixture(scope="module")
def empties(oracle):
    return Batch(oracle, [b""] * 9, modes=[False])


@pytest.fixture(scope="module")
def long8(oracle):
    return Batch(oracle, [words(300 + k, 200000) for k in range(8)], modes=[False])


def to_dev(a):
    import torch
    return torch.from_numpy(a).cuda()


def guarded(total, shift):
    """A device buffer of 0xA5 and the `total` bytes of it that start `shift` bytes behind an aligned address."""
    import torch
    buf = torch.full((GUARD + 4 + total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    return buf, buf[GUARD + shift:GUARD + shift + total]


def check_guards(buf, total, shift):
    b = buf.cpu().numpy()
    assert (b[:GUARD + shift] == 0xA5).all(), "bytes in front of the result were written"
    assert (b[GUARD + shift + total:] == 0xA5).all(), "bytes behind the result were written"
    return b[GUARD + shift:GUARD + shift + total].tobytes()


# ---- 1. edge batch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("compat_go", MODES)
@pytest.mark.parametrize("wrap", WRAPS)
def test_edge_batch_equals_the_cpu_members(eng, edge, wrap, compat_go, device):
    want, want_off = edge.want(wrap, compat_go)
    out, off = eng.deflate_batch_framed(to_dev(edge.data) if device else edge.data, edge.off, wrap, compat_go=compat_go)
    assert isinstance(off, np.ndarray) and off.dtype == np.uint64
    assert np.array_equal(off, want_off), (off.tolist(), want_off.tolist())
    got = (out.cpu().numpy() if device else out)[:int(off[-1])].tobytes()
    if not device:
        assert isinstance(out, np.ndarray) and out.size == int(off[-1])
    for i, p in enumerate(edge.payloads):
        m = got[int(off[i]):int(off[i + 1])]
        assert m == edge.members[(wrap, compat_go)][i], "member %d (%d bytes of input)" % (i, len(p))
        assert cpu_read(wrap, m) == p, i
    assert got == want


# ---- 2. alignment -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("wrap", WRAPS)
def test_out_at_any_alignment_and_nothing_around_it_is_touched(eng, edge, empties, wrap, shift):
    for batch in (edge, empties):
        want, want_off = batch.want(wrap, False)
        buf, out = guarded(len(want), shift)
        _, off = eng.deflate_batch_framed(to_dev(batch.data), batch.off, wrap, out=out)
        assert np.array_equal(off, want_off)
        assert check_guards(buf, len(want), shift) == want
    # members of 11 and 23 bytes: their edges share dwords
    assert len(empties.members[(wrap, False)][0]) == {"zlib": 11, "gzip": 23}[wrap]


# ---- 3. out_cap ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("wrap", WRAPS)
def test_out_cap_is_exact(eng, edge, wrap, device):
    want, want_off = edge.want(wrap, False)
    data = to_dev(edge.data) if device else edge.data
    out, off = eng.deflate_batch_framed(data, edge.off, wrap, out_cap=len(want))
    assert np.array_equal(off, want_off)
    assert (out.cpu().numpy() if device else out)[:len(want)].tobytes() == want
    with pytest.raises(flate.FlateError) as ei:
        eng.deflate_batch_framed(data, edge.off, wrap, out_cap=len(want) - 1)
    assert ei.value.code == E_OUT_TOO_SMALL


# ---- 4. wrap = raw ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compat_go", MODES)
def test_wrap_raw_is_deflate_batch(eng, edge, compat_go):
    out, off = eng.deflate_batch_framed(edge.data, edge.off, "raw", compat_go=compat_go)
    ref, ref_off = eng.deflate_batch(edge.data, edge.off, compat_go=compat_go)
    assert np.array_equal(off, ref_off) and out.tobytes() == ref[:int(ref_off[-1])].tobytes()
    assert out.tobytes() == b"".join(edge.raw[compat_go])
    d = words(41, 5000)
    out, off = eng.deflate_batch_framed(edge.data, edge.off, "raw", compat_go=compat_go, zdicts=[d])
    ref, ref_off = eng.deflate_batch(edge.data, edge.off, compat_go=compat_go, zdicts=[d])
    assert np.array_equal(off, ref_off) and out.tobytes() == ref[:int(ref_off[-1])].tobytes()
    assert out.tobytes()[int(off[-2]):] == deflate_dict(edge.payloads[-1], d, 1 if compat_go else 0)


# ---- 5. the per-block entropy kernels -----------------------------------------------------------------------------
@pytest.mark.parametrize("wrap", WRAPS)
def test_streams_of_four_blocks_in_both_entropy_forms(eng, long8, wrap):
    want, want_off = long8.want(wrap, False)
    data = to_dev(long8.data)
    try:
        for per_block in (-1, 0):  # -1: one wavefront per block here (4 blocks per stream); 0: never
            eng.set_option("entropy_per_block", per_block)
            out, off = eng.deflate_batch_framed(data, long8.off, wrap)
            assert np.array_equal(off, want_off), per_block
            assert out.cpu().numpy()[:len(want)].tobytes() == want, per_block
    finally:
        eng.set_option("entropy_per_block", -1)


# ---- 6. dictionaries ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dict_case():
    dicts = [words(61, 40000), words(62, 900), words(63, 16), b""]
    dict_of, payloads = [], []
    for k in range(20):
        j = [0, 1, NO_DICT, 2, 3][k % 5]
        n = [0, 100, 3000, 70000][k % 4]
        d = dicts[j] if j != NO_DICT else b""
        payloads.append((d[-300:] + words(170 + k, n))[:n])  # (starts with the dictionary's end: matches into it)
        dict_of.append(j)
    return dicts, dict_of, payloads


def dict_member(oracle, p, d, compat_go):
    """The zlib member of payload p written with dictionary d (None: without one)."""
    compat = 1 if compat_go else 0
    if d is None:
        return oracle.frame(oracle.FRAME_ZLIB, oracle.deflate(p, compat=compat), p)
    return engine.zlib_dict_header(d) + deflate_dict(p, d, compat) + zlib.adler32(p).to_bytes(4, "big")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("compat_go", MODES)
def test_zlib_members_with_dictionaries(eng, oracle, dict_case, compat_go, device):
    dicts, dict_of, payloads = dict_case
    data, off = pack(payloads)
    out, ooff = eng.deflate_batch_framed(to_dev(data) if device else data, off, "zlib", compat_go=compat_go,
                                         zdicts=dicts, dict_of=dict_of)
    out = out.cpu().numpy() if device else out
    at = 0
    for i, (p, j) in enumerate(zip(payloads, dict_of)):
        d = None if j == NO_DICT else dicts[j]
        want = dict_member(oracle, p, d, compat_go)
        assert int(ooff[i]) == at, i
        got = out[at:at + len(want)].tobytes()
        assert got == want, "member %d (payload %d bytes, dictionary %s)" % (i, len(p), "none" if d is None else len(d))
        at += len(want)
        assert got[:2] == (b"\x78\x01" if d is None else b"\x78\x3f")
        o = zlib.decompressobj() if d is None else zlib.decompressobj(zdict=d)
        assert o.decompress(got) == p and o.eof
    assert int(ooff[-1]) == at
    if not device:
        assert out.size == at


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_five_streams_that_make_every_upload_of_the_call(eng, oracle, device):
    """The call with the most control-array uploads for the fewest streams: every match-finder list has one stream
    (single-window, multi-window, dictionary), a fourth names a dictionary its encoder never sees (under 128 bytes),
    the DICTIDs and the streams' checksums are staged, and every stream has a block, so the per-block entropy form
    uploads its block list as well.  Each upload takes a 256-byte-aligned slot of the staging: a budget that is too
    small shows here as FLATE_HIP_E_INTERNAL."""
    dicts = [words(61, 40000), words(62, 900)]
    shape = [(65535, NO_DICT), (3 * 65535 + 200, NO_DICT), (65535 + 300, 0), (100, 1), (20, NO_DICT)]
    dict_of = [j for _, j in shape]
    payloads = [((dicts[j][-300:] if j != NO_DICT else b"") + words(180 + k, n))[:n] for k, (n, j) in enumerate(shape)]
    data, off = pack(payloads)
    want = [dict_member(oracle, p, None if j == NO_DICT else dicts[j], False) for p, j in zip(payloads, dict_of)]
    want_off = np.zeros(len(want) + 1, np.uint64)
    np.cumsum(np.array([len(m) for m in want], dtype=np.uint64), out=want_off[1:])
    eng.set_option("entropy_per_block", 1)
    try:
        out, ooff = eng.deflate_batch_framed(to_dev(data) if device else data, off, "zlib", zdicts=dicts, dict_of=dict_of)
    finally:
        eng.set_option("entropy_per_block", -1)
    assert np.array_equal(ooff, want_off), (ooff.tolist(), want_off.tolist())
    out = out.cpu().numpy() if device else out
    for i, m in enumerate(want):
        assert out[int(ooff[i]):int(ooff[i + 1])].tobytes() == m, "member %d (%d bytes of input)" % (i, len(payloads[i]))


def test_dictionary_arguments(eng, oracle, dict_case):
    dicts, dict_of, payloads = dict_case
    data, off = pack(payloads)
    # dict_of = None with one dictionary: every stream uses it, the empty ones too
    out, ooff = eng.deflate_batch_framed(data, off, "zlib", compat_go=True, zdicts=dicts[0])
    want = b"".join(dict_member(oracle, p, dicts[0], True) for p in payloads)
    assert out.tobytes() == want and int(ooff[-1]) == len(want)
    # an empty dictionary has DICTID 1
    out, ooff = eng.deflate_batch_framed(data, off, "zlib", zdicts=[b""])
    assert out.tobytes()[:6] == b"\x78\x3f\x00\x00\x00\x01"
    assert out.tobytes() == b"".join(dict_member(oracle, p, b"", False) for p in payloads)
    # gzip has no dictionaries (the call: E_INVALID; the engine has always raised ValueError); a dict_of entry must
    # name one or be NO_DICT
    n = len(payloads)
    buf = np.zeros(1 << 20, np.uint8)
    out_off = np.zeros(n + 1, np.uint64)
    dk = engine._DictArgs(dicts, dict_of, n, False)
    assert eng._L.flate_hip_deflate_fast_batch_framed(eng._ctx, data.ctypes.data, off.ctypes.data, n, engine.WRAP_GZIP,
                                                      dk.ptr, dk.off_ptr, dk.n_dicts, dk.of_ptr, buf.ctypes.data,
                                                      buf.size, out_off.ctypes.data, 0) == E_INVALID
    for device in (False, True):
        d = to_dev(data) if device else data
        with pytest.raises(ValueError):
            eng.deflate_batch_framed(d, off, "gzip", zdicts=dicts, dict_of=dict_of)
        with pytest.raises(flate.FlateError) as ei:
            eng.deflate_batch_framed(d, off, "zlib", zdicts=dicts, dict_of=[len(dicts)] + dict_of[1:])
        assert ei.value.code == E_INVALID
    # an unknown wrap
    assert eng._L.flate_hip_deflate_fast_batch_framed(eng._ctx, data.ctypes.data, off.ctypes.data, len(payloads), 3, None,
                                                      None, 0, None, buf.ctypes.data, buf.size, out_off.ctypes.data,
                                                      0) == E_INVALID
    # no streams
    out, ooff = eng.deflate_batch_framed(data, off[:1], "gzip")
    assert ooff.tolist() == [0] and out.size == 0


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_no_dictionaries_but_a_dict_of(eng, edge, device):
    """What C, C++ and MoonBit callers may pass (the engine's _DictArgs always has a dict_off): n_dicts = 0, null
    dicts and dict_off, and a dict_of of FLATE_HIP_NO_DICT only -- accepted as by flate_hip_deflate_fast_batch_dict;
    the plain zlib members."""
    want, want_off = edge.want("zlib", False)
    n = len(edge.payloads)
    of = np.full(n, NO_DICT, np.uint32)
    data = to_dev(edge.data) if device else edge.data
    out = to_dev(np.zeros(len(want), np.uint8)) if device else np.zeros(len(want), np.uint8)
    out_off = np.zeros(n + 1, np.uint64)
    rc = eng._L.flate_hip_deflate_fast_batch_framed(
        eng._ctx, data.data_ptr() if device else data.ctypes.data, edge.off.ctypes.data, n, engine.WRAP_ZLIB, None, None,
        0, of.ctypes.data, out.data_ptr() if device else out.ctypes.data, len(want), out_off.ctypes.data,
        engine.DEVICE_PTRS if device else 0)
    assert rc == 0
    assert np.array_equal(out_off, want_off)
    assert (out.cpu().numpy() if device else out).tobytes() == want


# ---- 7. the spliced form ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def splice_case(oracle):
    payloads = [fill(k + 1, n) for k, n in enumerate(SPLICE_LENS)]
    data, off = pack(payloads)
    whole = b"".join(payloads)
    want = {}
    for go in MODES:
        one, bit_off = oracle.deflate_spliced(data, off, compat=1 if go else 0)
        for w in WRAPS:
            want[(w, go)] = (oracle.frame(kind_of(oracle, w), one, whole), bit_off)
    return payloads, data, off, whole, want


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("compat_go", MODES)
@pytest.mark.parametrize("wrap", WRAPS)
def test_spliced_member(eng, splice_case, wrap, compat_go, device):
    payloads, data, off, whole, want = splice_case
    member, bit_ref = want[(wrap, compat_go)]
    out, nbytes, bit_off = eng.deflate_spliced_framed(to_dev(data) if device else data, off, wrap, compat_go=compat_go,
                                                      index=True)
    host = out.cpu().numpy() if device else out
    assert nbytes == len(member) and host[:nbytes].tobytes() == member
    assert cpu_read(wrap, member) == whole
    _, _, bit_raw = eng.deflate_spliced(data, off, compat_go=compat_go)
    assert np.array_equal(bit_off, bit_raw) and np.array_equal(bit_off, bit_ref)
    # the index counts from the raw stream's first byte: the spliced inflater reads out + header length
    hl, tl = HLEN[wrap], TLEN[wrap]
    back, boff, blen, status, _ = eng.inflate_spliced(out[hl:], nbytes - hl - tl, bit_off, [len(p) for p in payloads])
    back = back.cpu().numpy() if device else back
    assert (status == 0).all()
    for i, p in enumerate(payloads):
        assert int(blen[i]) == len(p) and back[int(boff[i]):int(boff[i]) + len(p)].tobytes() == p, i
    if not device:  # host data without index=True: the member as bytes, as before
        assert eng.deflate_spliced_framed(data, off, wrap, compat_go=compat_go) == member


@pytest.mark.parametrize("wrap", WRAPS)
def test_spliced_member_edges(eng, oracle, splice_case, wrap):
    payloads, data, off, whole, want = splice_case
    member, _ = want[(wrap, False)]
    # no streams: header, the closing block, the trailer of nothing
    nothing = oracle.frame(kind_of(oracle, wrap), b"\x01\x00\x00\xff\xff", b"")
    assert eng.deflate_spliced_framed(data, off[:1], wrap) == nothing
    out, nbytes, _ = eng.deflate_spliced_framed(to_dev(data), off[:1], wrap)
    assert out.cpu().numpy()[:nbytes].tobytes() == nothing and cpu_read(wrap, nothing) == b""
    # out_cap: header + stream + trailer is enough, one byte less is not
    for device in (False, True):
        d = to_dev(data) if device else data
        out, nbytes, _ = eng.deflate_spliced_framed(d, off, wrap, out_cap=len(member), index=True)
        assert (out.cpu().numpy() if device else out)[:nbytes].tobytes() == member
        with pytest.raises(flate.FlateError) as ei:
            eng.deflate_spliced_framed(d, off, wrap, out_cap=len(member) - 1, index=True)
        assert ei.value.code == E_OUT_TOO_SMALL
    # out at an odd address, nothing around it touched
    for shift in (1, 3):
        buf, out = guarded(len(member), shift)
        _, nbytes, _ = eng.deflate_spliced_framed(to_dev(data), off, wrap, out=out)
        assert nbytes == len(member) and check_guards(buf, len(member), shift) == member


# ---- 8. nothing else moved ----------------------------------------------------------------------------------------
def test_the_raw_calls_after_a_framed_call_and_the_stage_times(eng, oracle, edge):
    eng.set_profiling(True)
    try:
        for wrap in WRAPS:
            eng.deflate_batch_framed(to_dev(edge.data), edge.off, wrap)
            t = eng.last_timing()
            assert t["checksum"] > 0 and t["lz77_match"] > 0 and t["huff_pack"] > 0, t
    finally:
        eng.set_profiling(False)
    out, off = eng.deflate_batch(edge.data, edge.off)
    assert out[:int(off[-1])].tobytes() == b"".join(edge.raw[False])
    one, nbytes, bit_off = eng.deflate_spliced(edge.data, edge.off)
    ref, ref_off = oracle.deflate_spliced(edge.data, edge.off)
    assert bytes(one[:nbytes]) == ref and np.array_equal(bit_off, ref_off)
    for kind, ref_sum in (("adler32", oracle.adler32), ("crc32", oracle.crc32)):
        sums = eng.checksum_batch(edge.data, edge.off, kind)
        assert [int(s) for s in sums] == [ref_sum(p) for p in edge.payloads], kind
        sums = eng.checksum_batch(to_dev(edge.data), edge.off, kind)
        assert [int(s) for s in sums] == [ref_sum(p) for p in edge.payloads], kind
