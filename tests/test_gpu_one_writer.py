"""flate_hip_one_writer_* on the GPU: one long raw, zlib or gzip stream written a part at a time.  For every input, piece
size and part list the concatenation of the calls' bytes and of their indexes must be flate_hip_deflate_fast_spliced_framed
of the whole input on the same engine AND the oracle-derived reference (tests/one_writer_ref.py), and every call's rc,
in_used, out_len and n_pieces the reference's.  The corpus is chosen on the CPU so that the reference alone shows every
carry 0..7 at a call boundary, a boundary directly behind a stored block, a final call without a piece whose closing
block starts at each of the 8 bit phases, and the empty stream; the tests assert that from the oracle's index."""
import ctypes as C
import gzip
import zlib

import numpy as np
import pytest

import one_writer_ref as R
from util import flate, make_streams

pytestmark = pytest.mark.gpu

DEVICE_PTRS, COMPAT_GO = 1, 2
GUARD = 0xA5
PIECES = (17, 300, 4096, 65535)
SIZE = {17: 20000, 300: 60000, 4096: 150000, 65535: 300000}  # bytes per input: at most about 300 KB
KINDS = ("text", "rand", "zero", "alt")


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


def plain_of(kind, P, n):
    """S-text, random bytes (stored blocks: the align8 branch), zeros, text and random alternating every P."""
    if kind == "text":
        return flate.synth("text", 1, n, first_stream=77).tobytes()
    if kind == "alt":
        text = flate.synth("text", 1, n, first_stream=78)
        rnd = np.random.default_rng(P).integers(0, 256, n, dtype=np.uint8)
        return np.where((np.arange(n) // P) % 2 == 0, text, rnd).astype(np.uint8).tobytes()
    data, _ = make_streams([(kind, n)], seed=100 + P)
    return data[:n].tobytes()


def part_lists(T, P):
    """name -> the new bytes of every call that is not final: fixed, random, growing, exactly k P, one byte short of
    P; at most a dozen calls each."""
    big = max(T // 7 + 1, 1)
    return {"fixed": R.fixed(T, big + 3)[:12], "random": R.random_sizes(T, big, seed=T + P)[:12],
            "growing": R.growing(T, 1, 4), "exactly k P": [P * max(T // (5 * P), 1)] * 12,
            "one byte short of P": [P - 1] * 12, "everything, then the end alone": [T]}


class Writer:
    """The C calls through ctypes, every output buffer prefilled: what lies in front of `out`, behind out[out_len] and --
    for a call that does not fit -- in all of it must stay what it was."""

    def __init__(self, eng, wrap, P, device=False, compat="moonbit"):
        self.eng, self.L, self.device, self.P = eng, eng._L, device, P
        self.h = C.c_void_p()
        flags = (DEVICE_PTRS if device else 0) | (COMPAT_GO if compat == "go" else 0)
        assert self.L.flate_hip_one_writer_open(eng._ctx, wrap, P, flags, C.byref(self.h)) == 0

    def write(self, part, final, cap=None, shift=0, index=True):
        part = bytes(part)
        n = len(part)
        room = R.bound(n, self.P) if cap is None else cap
        src = np.frombuffer(part + b"\0" * 16, np.uint8).copy()
        obuf = np.full(shift + room + 64, GUARD, np.uint8)
        if self.device:
            import torch
            d_in, d_out = torch.from_numpy(src).cuda(), torch.from_numpy(obuf).cuda()
            in_ptr, out_ptr = d_in.data_ptr(), d_out.data_ptr() + shift
            assert d_out.data_ptr() % 16 == 0
        else:
            in_ptr, out_ptr = src.ctypes.data, obuf.ctypes.data + shift
        used, ol, k = C.c_uint64(99), C.c_uint64(99), C.c_uint32(99)
        idx = np.full(n // self.P + 2, 12345, np.uint64)
        rc = self.L.flate_hip_one_writer_write(self.h, in_ptr if n else None, n, int(final), out_ptr, room, C.byref(used),
                                               C.byref(ol), idx.ctypes.data if index else None, C.byref(k))
        if self.device:
            import torch
            torch.cuda.synchronize()
            obuf = d_out.cpu().numpy()
        got = 0 if rc < 0 else int(ol.value)
        assert got <= room
        assert (obuf[:shift] == GUARD).all() and (obuf[shift + got:] == GUARD).all(), "bytes outside out[0, out_len)"
        n_idx = int(k.value) + (1 if rc == R.STREAM_END else 0) if rc >= 0 else 0
        assert (idx[n_idx:] == 12345).all()
        return int(used.value), obuf[shift:shift + got].tobytes(), (rc, int(ol.value), int(k.value), [int(b) for b in idx[:n_idx]])

    def reset(self):
        assert self.L.flate_hip_one_writer_reset(self.h) == 0

    def close(self):
        self.L.flate_hip_one_writer_free(self.h)
        self.h = C.c_void_p()


def whole_call(eng, plain, P, wrap, compat, device=False):
    """flate_hip_deflate_fast_spliced_framed of the whole input on the same engine -> (bytes, index)."""
    off = R.piece_offsets(len(plain), P)
    data = np.frombuffer(plain or b"\0", np.uint8)
    if device:
        import torch
        data = torch.from_numpy(data.copy()).cuda()
    out, n, bit_off = eng.deflate_spliced_framed(data, off, R.WRAP_NAME[wrap], compat_go=compat == "go", index=True)
    out = out.cpu().numpy() if device else out
    return bytes(out[:n]), [int(b) for b in bit_off]


def check_run(w, ref, sizes, what, **kw):
    """One stream through the writer; every call against the reference's, the concatenations against the whole."""
    want = ref.calls(sizes)
    got = R.feed(lambda buf, final: w.write(buf, final, **kw), ref.plain, sizes)
    assert len(got) == len(want), what
    for j, ((used, data, res), c) in enumerate(zip(got, want)):
        assert (res[0], used, res[1], res[2]) == (c.rc, c.in_used, c.out_len, c.n_pieces), (what, j, res, c[:4])
        assert res[3] == c.bit_off and data == c.data, (what, j)
    return b"".join(d for _, d, _ in got), [b for _, _, r in got for b in r[3]]


def is_stored(ref, i):
    """Piece i is one stored block: 3 bits, the padding to a byte, LEN, NLEN, its bytes (from the oracle's index)."""
    span = ref.bit_off[i + 1] - ref.bit_off[i]
    extra = span - 8 * int(ref.in_off[i + 1] - ref.in_off[i]) - 35
    return ref.bit_off[i + 1] % 8 == 0 and 0 <= extra <= 7


@pytest.fixture(scope="module")
def corpus(oracle):
    """{(kind, P): Whole} with wrap and compat mode rotating over the cases; computed once, shared, never changed."""
    out = {}
    for a, kind in enumerate(KINDS):
        for b, P in enumerate(PIECES):
            wrap = (R.GZIP, R.ZLIB, R.RAW)[(a + b) % 3]
            out[(kind, P)] = R.Whole(oracle, plain_of(kind, P, SIZE[P] + (a * 7 + b) % 5), P, wrap, "go" if (a + b) % 2 else "moonbit")
            out[(kind, P)].compat = "go" if (a + b) % 2 else "moonbit"
    return out


@pytest.fixture(scope="module")
def phases(oracle):
    """{phase: Whole}: streams of exactly m pieces of 17 bytes whose closing block starts at each of the 8 bit phases,
    found on the CPU from the oracle's index."""
    text = plain_of("alt", 17, 17 * 400)
    found = {}
    for m in range(1, 400):
        w = R.Whole(oracle, text[:17 * m], 17, (R.GZIP, R.ZLIB, R.RAW)[m % 3])
        w.compat = "moonbit"
        found.setdefault(w.bit_off[-1] % 8, w)
        if len(found) == 8:
            break
    assert sorted(found) == list(range(8))
    return found


def test_the_corpus_meets_the_coverage_conditions(corpus, phases):
    """From the oracle's index alone: every carry at a call boundary, a boundary behind a stored block, a final call
    without a piece at every phase of the closing block."""
    carries, behind_stored = set(), 0
    for (kind, P), ref in corpus.items():
        for sizes in part_lists(len(ref.plain), P).values():
            pieces = 0
            for c in ref.calls(sizes):
                pieces += c.n_pieces
                if c.n_pieces and not c.final:
                    carries.add(c.carry)
                    behind_stored += is_stored(ref, pieces - 1)
    assert carries == set(range(8)) and behind_stored >= 4, (carries, behind_stored)
    for ph, ref in phases.items():
        last = ref.calls([len(ref.plain)])[-1]
        assert last.final and last.in_len == 0 and last.n_pieces == 0 and last.start_bit == ph


@pytest.mark.parametrize("P", PIECES)
@pytest.mark.parametrize("kind", KINDS)
def test_any_cut_gives_the_whole_calls_bytes(eng, corpus, kind, P):
    ref = corpus[(kind, P)]
    device = (KINDS.index(kind) + PIECES.index(P) // 2) % 2 == 1
    whole = whole_call(eng, ref.plain, P, ref.wrap, ref.compat, device)
    assert whole == (ref.member, ref.bit_off)  # the whole call itself is the oracle's
    w = Writer(eng, ref.wrap, P, device, ref.compat)
    try:
        for k, (name, sizes) in enumerate(part_lists(len(ref.plain), P).items()):
            # (device callers: `out` at every misalignment in turn)
            got = check_run(w, ref, sizes, (kind, P, name), shift=(1, 2, 3, 5, 7, 9)[k] if device else 0)
            assert got == whole, (kind, P, name)
            w.reset()
    finally:
        w.close()


@pytest.mark.parametrize("device", (False, True))
def test_a_final_call_without_a_piece_at_every_phase(eng, phases, device):
    for ph, ref in phases.items():
        T = len(ref.plain)
        w = Writer(eng, ref.wrap, 17, device, ref.compat)
        try:
            for sizes in ([T], [17, T], [T - 17, 17, 0]):
                assert check_run(w, ref, sizes, (ph, sizes), shift=ph if device else 0) == whole_call(eng, ref.plain, 17, ref.wrap, ref.compat)
                w.reset()
        finally:
            w.close()


@pytest.mark.parametrize("device", (False, True))
@pytest.mark.parametrize("compat", ("moonbit", "go"))
@pytest.mark.parametrize("wrap", (R.RAW, R.ZLIB, R.GZIP))
def test_every_wrap_mode_and_side_and_the_empty_stream(eng, oracle, wrap, compat, device):
    plain = plain_of("alt", 300, 5000)
    for T in (0, 1, 299, 300, 301, 5000):
        ref = R.Whole(oracle, plain[:T], 300, wrap, compat)
        whole = whole_call(eng, ref.plain, 300, wrap, compat, device)
        assert whole == (ref.member, ref.bit_off)
        w = Writer(eng, wrap, 300, device, compat)
        try:
            for sizes in ([], [0, 0], [1, 298, 1, 1], [T // 2]):  # ([]: the final call is the only call)
                assert check_run(w, ref, sizes, (T, sizes), shift=3 if device else 0) == whole
                w.reset()
        finally:
            w.close()


@pytest.mark.parametrize("device", (False, True))
def test_too_little_room_changes_nothing(eng, corpus, device):
    """out_cap = needed - 1: FLATE_HIP_E_OUT_TOO_SMALL with *out_len = needed and `out` untouched (Writer.write holds the
    prefill); the same call at exactly needed delivers the reference's bytes."""
    for key in (("alt", 300), ("text", 4096), ("rand", 17)):
        ref = corpus[key]
        P = key[1]
        sizes = part_lists(len(ref.plain), P)["random"]
        w = Writer(eng, ref.wrap, P, device, ref.compat)
        try:
            want = ref.calls(sizes)
            it = iter(want)

            def write(buf, final):
                c = next(it)
                if c.out_len:
                    used, data, res = w.write(buf, final, cap=c.out_len - 1, shift=1 if device else 0)
                    assert (res[0], used, res[1], res[2], data) == (R.E_OUT_TOO_SMALL, 0, c.out_len, 0, b""), (key, res)
                return w.write(buf, final, cap=c.out_len, shift=1 if device else 0)  # exactly enough, to the byte

            got = R.feed(write, ref.plain, sizes)
            assert [(r[0], u, r[1], r[2]) for u, _, r in got] == [(c.rc, c.in_used, c.out_len, c.n_pieces) for c in want]
            assert b"".join(d for _, d, _ in got) == ref.member
            assert [b for _, _, r in got for b in r[3]] == ref.bit_off
        finally:
            w.close()


def test_the_end_is_sticky_until_reset_and_a_second_stream_is_a_fresh_one(eng, corpus):
    ref = corpus[("alt", 4096)]
    w = Writer(eng, ref.wrap, 4096, False, ref.compat)
    fresh = Writer(eng, ref.wrap, 4096, False, ref.compat)
    try:
        sizes = part_lists(len(ref.plain), 4096)["growing"]
        first = check_run(w, ref, sizes, "first")
        used, data, res = w.write(b"abc", False)
        assert (res[0], used, data) == (R.E_INVALID, 0, b"")  # behind the end every write is invalid ...
        assert w.write(b"", True)[2][0] == R.E_INVALID
        w.reset()                                             # ... until reset
        second = check_run(w, ref, part_lists(len(ref.plain), 4096)["fixed"], "second")
        assert first == second == check_run(fresh, ref, sizes, "fresh") == (ref.member, ref.bit_off)
        # a stream given up half way leaves nothing behind either
        w.reset()
        assert w.write(ref.plain[:3 * 4096 + 5], False)[0] == 3 * 4096
        w.reset()
        assert check_run(w, ref, sizes, "third") == first
    finally:
        w.close()
        fresh.close()


def test_a_writer_and_a_batch_call_interleaved_change_neither(eng, corpus, oracle):
    ref = corpus[("alt", 300)]
    data, off = make_streams([("text", 70000), ("rand", 3000), ("zero", 500), ("text", 200)], seed=3)
    alone, alone_off = eng.deflate_batch(data, off)
    w = Writer(eng, ref.wrap, 300, False, ref.compat)
    try:
        def write(buf, final):
            r = w.write(buf, final)
            out, out_off = eng.deflate_batch(data, off)  # an unrelated call on the same ctx, between two parts
            assert (out_off == alone_off).all() and bytes(out[:int(out_off[-1])]) == bytes(alone[:int(alone_off[-1])])
            return r
        got = R.feed(write, ref.plain, part_lists(len(ref.plain), 300)["random"])
        assert b"".join(d for _, d, _ in got) == ref.member
        assert [b for _, _, r in got for b in r[3]] == ref.bit_off
    finally:
        w.close()


@pytest.mark.parametrize("wrap", ("zlib", "gzip"))
def test_round_trips(eng, wrap):
    """engine.OneWriter: the standard library inflates the parts' concatenation to the input, inflate_spliced_framed
    reads it from the concatenated index, and OneReader reads it in parts."""
    P = 4096
    plain = plain_of("alt", P, 150003)
    for device in (False, True):
        wr = eng.open_one_writer(wrap, P, device=device)
        chunks, index, rest = [], [], b""
        for part, final in ((plain[:50000], False), (plain[50000:50001], False), (plain[50001:], True)):
            buf = np.frombuffer(rest + part, np.uint8)
            if device:
                import torch
                buf = torch.from_numpy(buf.copy()).cuda()
            used, out, res = wr.write(buf, final=final, index=True)  # (the default room: a part of random bytes is
            chunks.append(bytes(out.cpu().numpy() if device else out))    # repeated once with the reported size)
            index += [int(b) for b in res.bit_off]
            rest = (rest + part)[used:]
            assert res.rc == (1 if final else 0) and res.out_len == len(chunks[-1])
        wr.close()
        member = b"".join(chunks)
        assert (zlib.decompress(member) if wrap == "zlib" else gzip.decompress(member)) == plain
        n = len(index) - 1
        assert n == -(-len(plain) // P)
        sizes = [min(P, len(plain) - i * P) for i in range(n)]
        out, out_off, out_len, status, _, ms = eng.inflate_spliced_framed(np.frombuffer(member, np.uint8), len(member), wrap, index, sizes)
        assert ms == 0 and (status == 0).all() and bytes(out[:len(plain)]) == plain
    rd = eng.open_one_reader(wrap)
    back, buf, at = b"", b"", 0
    while True:
        new = member[at:at + 40000]
        at += len(new)
        buf += new
        used, out, res = rd.read(np.frombuffer(buf, np.uint8), final=at >= len(member))
        back += bytes(out)
        buf = buf[used:]
        if res.rc != 0:
            break
    rd.close()
    assert res.rc == 1 and back == plain
