"""ONE long stream read in PARTS on the GPU: flate_hip_one_reader_* (FlateEngine.open_one_reader).  Every expectation
comes from the CPU -- zlib for the bytes, tests/one_parts_ref.py (built on one_ref.Walk) for what each call must return
under the default unit rule -- or, for failing streams, from flate_hip_inflate_one on the whole stream, the call the
reader must equal whatever the cuts.  Every feeding loop runs under a hard cap on its calls (one_parts_ref.feed)."""
import random
import struct
import zlib

import numpy as np
import pytest

import gzip_ref
import one_parts_ref as R
import one_ref as ref
import one_window_corpus as corpus
from test_gpu_inflate_one import failing_streams
from util import STATUS_OF_ORACLE, flate

pytestmark = pytest.mark.gpu

KINDS = (ref.RAW, ref.ZLIB, ref.GZIP)
NAMES = {ref.RAW: "raw", ref.ZLIB: "zlib", ref.GZIP: "gzip"}
GUARD, ROOM = 0xA5, 1 << 21


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


def build(parts):
    """One raw stream from zlib compressors run one after the other: every piece but the last ends with Z_FULL_FLUSH (byte
    aligned, no history behind it), the last one finishes the stream.  parts: [(data, level, memLevel, strategy)]."""
    out = []
    for i, (data, level, mem, strategy) in enumerate(parts):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
        out.append(c.compress(data) + c.flush(zlib.Z_FINISH if i + 1 == len(parts) else zlib.Z_FULL_FLUSH))
    return b"".join(out)


@pytest.fixture(scope="module")
def streams():
    """{name: (raw, plain, Walk)}: computed once, shared, never changed.  A few hundred KiB of output each, the
    memLevel lowered so that a short stream has many dynamic blocks."""
    t = gzip_ref.text(420000, seed=41)
    d = zlib.Z_DEFAULT_STRATEGY
    mixed = [(t[:90000], 6, 3, d), (t[90000:150000], 6, 8, zlib.Z_FIXED), (gzip_ref.rand(150000, seed=6), 0, 8, d),
             (t[150000:260000], 6, 3, d)]
    made = {"level 6": (ref.deflate(t[:300000], 6, mem=1), t[:300000]),
            "level 1": (ref.deflate(t, 1, mem=2), t),
            "full flush": (ref.deflate(t[:250000], 6, mem=3, flush_every=30000), t[:250000]),
            "fixed blocks and a stored run": (build(mixed), b"".join(p[0] for p in mixed))}
    out = {}
    for name, (raw, plain) in made.items():
        w = ref.Walk(raw)
        assert w.status == 0 and w.n_units >= 8 and zlib.decompress(raw, -15) == plain, name
        out[name] = (raw, plain, w)
    return out


def reader(rd, device, guard=False):
    """`read` of one_parts_ref.feed over an engine reader: (Call, the bytes).  guard (device pointers): the output lies
    in a prefilled buffer between guard regions, and nothing outside out[0, out_len) may change."""
    import torch

    def read(buf, final, out_cap):
        cap = ROOM if out_cap is None else out_cap
        part = np.frombuffer(buf, np.uint8)
        out = None
        if device:
            part = torch.from_numpy(part.copy()).cuda()
            if guard:
                whole = torch.full((cap + 512,), GUARD, dtype=torch.uint8, device="cuda")
                out = whole[256:256 + max(cap, 1)]
        used, got, res = rd.read(part, final=final, out=out, out_cap=cap)
        if guard and device:
            torch.cuda.synchronize()
            img = whole.cpu().numpy()
            n = res.out_len if res.rc != R.OUT_TOO_SMALL else 0
            assert (img[:256] == GUARD).all() and (img[256 + n:] == GUARD).all(), "bytes outside out[0, out_len) changed"
        got = got.cpu().numpy() if device else got
        return R.Call(res.rc, used, res.out_len, res.n_units, res.err_off), bytes(got)
    return read


def whole(eng, f, kind, cap=ROOM):
    """flate_hip_inflate_one on the whole stream -> (status, err_off, out_len, the bytes, n_units)."""
    out, q = eng.inflate_one(np.frombuffer(bytes(f), np.uint8), NAMES[kind], out=np.zeros(cap, np.uint8))
    return q.status, q.err_off, q.out_len, bytes(out[:q.out_len]), q.n_units


def fixed(step):
    return iter(lambda: step, 0)


def check_against_model(eng, f, kind, w, plain, sizes_of, device, out_cap=None, guard=False, grow=1, what=""):
    """The same feeding loop over the reference and over the device: every call's five words and the bytes are equal."""
    m = R.Model(f, kind, walk=w, plain=plain)
    cap = w.n_units + len(f) + 8
    want_calls, want, _ = R.feed(R.model_reader(m), f, sizes_of(), out_cap, cap, grow)
    rd = eng.open_one_reader(NAMES[kind], device=device)
    try:
        # the cap on calls: the units plus the parts (the reference has just counted them) plus a small constant
        calls, got, rest = R.feed(reader(rd, device, guard), f, sizes_of(), out_cap, len(want_calls) + 4, grow)
    finally:
        rd.close()
    assert calls == want_calls, (what, kind, device, [(i, a, b) for i, (a, b) in enumerate(zip(calls, want_calls)) if a != b][:3])
    assert got == want, (what, kind, device)
    return calls, got, rest


# ---- 1. whole-call results whatever the cuts ----

@pytest.mark.parametrize("kind", KINDS)
def test_whole_call_results_whatever_the_cuts(eng, streams, kind):
    rnd = random.Random(7)
    stops = set()
    for name, (raw, plain, w) in streams.items():
        f = ref.wrap(raw, plain, kind)
        n_whole = whole(eng, f, kind)[4]
        assert n_whole == w.n_units, name
        # how the parts are cut -> (the new bytes per call, what a call that used nothing is followed by)
        cuts = {"4 KiB": (lambda: fixed(4096), 4096), "16 KiB": (lambda: fixed(16384), 16384),
                "64 KiB": (lambda: fixed(65536), 65536)}
        seeds = [rnd.randrange(1 << 30) for _ in range(2)]
        for s in seeds:
            cuts["random %d" % s] = (lambda s=s: (random.Random(s).randrange(1, 40000) for _ in iter(int, 1)), 5000)
        # three bytes short of the first unit: nothing is used, and the loop grows the part by one byte a call
        cuts["growing by one byte"] = (lambda: iter([ref.header_len(kind) + w.reach[0] - 3]), 1)
        for how, (sizes_of, grow) in cuts.items():
            for device in ((False, True) if how in ("16 KiB", "growing by one byte") else (how == "4 KiB",)):
                if how == "growing by one byte" and name != "level 6":
                    continue
                calls, got, rest = check_against_model(eng, f, kind, w, plain, sizes_of, device, guard=device, grow=grow,
                                                       what=(name, how))
                assert calls[-1].rc == R.STREAM_END and got == plain and not rest, (name, how)
                if how == "growing by one byte":
                    assert [c.in_used for c in calls[:4]] == [0, 0, 0, calls[3].in_used] and calls[3].n_units == 1
                assert sum(c.in_used for c in calls) == len(f) and sum(c.n_units for c in calls) == n_whole, (name, how)
                k = 0
                for c in calls[:-1]:
                    k += c.n_units
                    stops.add(w.unit_bit[k] % 8)
    assert stops >= set(range(8)), stops  # all eight carry bits occur where calls stop


@pytest.mark.parametrize("kind", KINDS)
def test_stored_headers_start_units_too(eng, streams, kind):
    """Option "one_stored_units" at 1, recorded at open: the handle keeps the rule after the ctx has gone back to 0."""
    raw, plain, w = streams["fixed blocks and a stored run"]
    f = ref.wrap(raw, plain, kind)
    eng.set_option("one_stored_units", 1)
    try:
        n_whole = whole(eng, f, kind)[4]
        readers = [(eng.open_one_reader(NAMES[kind], device=dev), dev) for dev in (False, True)]
    finally:
        eng.set_option("one_stored_units", 0)
    assert n_whole > w.n_units  # the stored run is cut into units
    for rd, dev in readers:
        for step in (16384, 65536):
            rd.reset()
            calls, got, rest = R.feed(reader(rd, dev), f, fixed(step), None, n_whole + len(f) // step + 8, grow=step)
            assert calls[-1].rc == R.STREAM_END and got == plain and not rest, (kind, dev, step)
            assert sum(c.in_used for c in calls) == len(f) and sum(c.n_units for c in calls) == n_whole, (kind, dev, step)
        rd.close()


# ---- 2. every carry bit ----

def test_every_carry_bit_around_known_unit_starts(eng, streams):
    raw, plain, w = streams["level 1"]
    ix = eng.inflate_one_index(np.frombuffer(raw, np.uint8), "raw")
    assert list(ix.unit_bit) == w.unit_bit
    picks = {}
    for k in range(2, w.n_units):
        picks.setdefault(int(ix.unit_bit[k]) % 8, k)
    assert set(picks) == set(range(8))
    stops = set()
    for b0, k in sorted(picks.items()):
        for cut in range(w.reach[k - 1] - 3, w.reach[k - 1] + 4):  # around the byte that completes unit k - 1
            calls, got, rest = check_against_model(eng, raw, ref.RAW, w, plain, lambda: iter([cut]), False, what=(b0, cut))
            assert got == plain and calls[-1].rc == R.STREAM_END
            stops.add(w.unit_bit[calls[0].n_units] % 8)
    assert stops == set(range(8))


# ---- 3. history across parts ----

def test_history_across_parts(eng):
    good = corpus.good_streams()
    for what, raw, plain, marks in good:
        w = ref.Walk(raw)
        assert w.status == 0
        edges = sorted({b // 8 for b in w.unit_bit[1:-1]} | {b // 8 + 1 for b in w.unit_bit[1:-1]})
        inside = sorted({(a + b) // 16 for a, b in zip(w.unit_bit, w.unit_bit[1:]) if b - a > 16})
        for cuts in (edges[:12], inside[:12], [w.reach[0]]):
            sizes = [b - a for a, b in zip([0] + cuts, cuts) if b > a]
            # (a part cut inside a unit delivers nothing of it: the loop then adds half a window)
            calls, got, rest = check_against_model(eng, raw, ref.RAW, w, plain, lambda: iter(sizes), len(cuts) == 1,
                                                   what=what, grow=16384)
            assert calls[-1].rc == R.STREAM_END and got == plain, what
    assert any(d == corpus.W and pos - d < w0 for what, raw, plain, marks in good for pos, _, d in marks
               for w0 in [ref.Walk(raw).out_off[1]]), "a match that reaches 32768 back"


def test_a_distance_in_front_of_the_stream_in_part_two(eng):
    """Less than 32 KiB produced, the failing copy in a later part: FLATE_HIP_E_CORRUPT at the whole call's offset."""
    twins = [t for t in corpus.failing_twins() if t[3] == "far"]
    assert twins
    seen_small = False
    for what, raw, front, _ in twins:
        st, eo, ol, out, _ = whole(eng, raw, ref.RAW)
        assert st == ref.CORRUPT and out == front, what
        w = ref.Walk(raw)  # (history-free: it reads through the copy)
        k = max(i for i in range(len(w.unit_bit)) if w.out_off[i] <= len(front) and i < w.n_units)
        if k == 0:
            continue
        seen_small = seen_small or len(front) < corpus.W
        for cut in (w.reach[k - 1], w.reach[k - 1] + 2):
            for device in (False, True):
                rd = eng.open_one_reader("raw", device=device)
                calls, got, _ = R.feed(reader(rd, device), raw, iter([cut]), None, w.n_units + 8, grow=64)
                assert len(calls) >= 2 and calls[0].rc == R.OK and calls[0].n_units == k, what
                assert (calls[-1].rc, calls[-1].err_off) == (st, eo) and got == out, (what, cut, calls[-1])
                assert reader(rd, device)(b"\0\0\0\0", False, 16)[0] == R.Call(st, 0, 0, 0, eo)  # sticky
                rd.close()
    assert seen_small


# ---- 4. error parity ----

@pytest.fixture(scope="module")
def failing(eng, oracle):
    what, raw, plain = ref.good_streams(None)[ref.MANY_UNITS]  # (the one file failing_streams cuts and flips)
    cases = failing_streams([None] * ref.MANY_UNITS + [(what, raw, plain, ref.Walk(raw))])
    out = [(what, raw) + whole(eng, raw, ref.RAW, ref.Walk(raw).out_len + 600) for what, raw in cases]
    for what, raw, st, eo, ol, got, _ in out:  # the yardstick itself against the oracle on the same bytes
        rc, want, _, eoff = oracle.inflate(raw, ol + 600, full=True)
        assert (st, eo, ol, got) == (STATUS_OF_ORACLE[rc], eoff, len(want), want), (what, st, eo, ol, rc, eoff, len(want))
    return out


@pytest.mark.parametrize("split,share", [(s, q) for s in (3, 2) for q in range(4)])
def test_error_parity_with_the_whole_call(eng, failing, split, share):
    """Every stream flate_hip_inflate_one is tested on, in parts of 1 / split of its length (a quarter of the corpus
    per case, so that each stays short)."""
    rd = eng.open_one_reader("raw")
    seen = set()
    for what, raw, st, eo, ol, out, _ in failing[share::4]:
        rd.reset()
        step = max(len(raw) // split, 1)
        # (where a part is too short for a unit the loop grows it, by a twelfth of the stream: a dozen calls at most)
        calls, got, rest = R.feed(reader(rd, False), raw, fixed(step), None, split + 12 + 16, grow=max(len(raw) // 12, 1))
        last = calls[-1]
        assert (0 if last.rc == R.STREAM_END else last.rc, last.err_off) == (st, eo), (what, last, st, eo)
        assert (len(got), got) == (ol, out), (what, len(got), ol)
        again = rd.read(np.frombuffer(raw[:4], np.uint8), final=True)[2]  # every later call: the same status
        assert (again.rc, again.out_len, again.err_off) == (last.rc, 0, last.err_off), what
        seen.add(st)
    rd.close()
    assert seen >= {0, ref.CORRUPT, ref.UNEXPECTED_EOF}


def test_error_offsets_inside_a_later_part_of_a_member(eng, streams):
    """A flipped bit deep inside a zlib and a gzip member, device and host pointers: the error comes out in a later part,
    where err_off is a part's offset plus the raw bytes in front of it, without the header -- the whole call's words."""
    raw, plain, w = streams["level 1"]
    k = 2 * w.n_units // 3
    for bit in (w.unit_bit[k] + 20, (w.unit_bit[k] + w.unit_bit[k + 1]) // 2):  # a unit's header, a unit's body
        bad = bytearray(raw)
        bad[bit >> 3] ^= 1 << (bit & 7)
        for kind in (ref.ZLIB, ref.GZIP):
            f = ref.wrap(bytes(bad), plain, kind)
            st, eo, ol, out, _ = whole(eng, f, kind)
            assert st == ref.CORRUPT and eo > 0  # (in the stream, or -- a flip that still decodes -- at the trailer)
            for device in (False, True):
                for step in (len(f) // 3, 16384):
                    rd = eng.open_one_reader(NAMES[kind], device=device)
                    calls, got, _ = R.feed(reader(rd, device), f, fixed(step), None, w.n_units + len(f) // step + 8, grow=4096)
                    rd.close()
                    last = calls[-1]
                    assert len(calls) >= 2 and calls[0].rc == R.OK and calls[0].in_used > 0 and last.rc == st, (kind, bit, last, st)
                    assert (last.err_off, len(got), got) == (eo, ol, out), (kind, bit, device, step, last, eo, ol)


# ---- 5. capacity ----

def test_capacity(eng, streams):
    raw, plain, w = streams["level 6"]
    f = ref.wrap(raw, plain, ref.GZIP)
    sizes = [b - a for a, b in zip(w.out_off, w.out_off[1:])]
    for device in (False, True):
        # smaller than a part's units: a prefix that fits, and the next call goes on
        calls, got, _ = check_against_model(eng, f, ref.GZIP, w, plain, lambda: fixed(65536), device, out_cap=max(sizes) + 100,
                                            guard=True, grow=4096, what="small capacity")
        assert got == plain and len(calls) > len(f) // 65536 + 3
    # smaller than the first unit: the size needed, the state unchanged, the bytes exact afterwards
    rd = eng.open_one_reader("gzip")
    read = reader(rd, False)
    c, got = read(f[:65536], False, sizes[0] - 1)
    assert c == R.Call(R.OUT_TOO_SMALL, 0, sizes[0], 0, -1) and got == b""
    c, got = read(f[:65536], False, sizes[0])
    assert (c.rc, c.out_len, c.n_units) == (R.OK, sizes[0], 1) and got == plain[:sizes[0]]
    calls, rest, _ = R.feed(read, f[c.in_used:], fixed(65536), None, w.n_units + 16, grow=4096)
    assert calls[-1].rc == R.STREAM_END and plain[:sizes[0]] + rest == plain
    rd.close()
    # "one_unit_max" lowered to a few KiB, recorded at open: a part of that size that completes no unit
    raw, plain, w = streams["fixed blocks and a stored run"]
    k = next(k for k in range(w.n_units) if w.reach[k] - w.unit_bit[k] // 8 > 8192)  # the first unit beyond the limit
    assert w.reach[k] - w.unit_bit[k] // 8 > 100000  # ... is the one with the fixed blocks and the stored run
    eng.set_option("one_unit_max", 8192)
    try:
        rd = eng.open_one_reader("raw")
    finally:
        eng.set_option("one_unit_max", 1 << 28)
    read = reader(rd, False)
    calls, got, rest = R.feed(read, raw, fixed(8192), None, w.n_units + len(raw) // 8192 + 8, grow=8192)
    assert calls[-1].rc == R.TOO_LARGE and sum(c.n_units for c in calls) == k and got == plain[:w.out_off[k]]
    assert read(rest, False, ROOM)[0].rc == R.TOO_LARGE  # sticky
    rd.close()


# ---- 6. container edges ----

def test_container_edges(eng, streams):
    raw, plain, w = streams["full flush"]
    hdr = gzip_ref.header(flg=4 | 8 | 16, extra=b"ab\x03\x00xyz", name=b"a name", comment=b"a comment")
    assert R.header_state(ref.GZIP, hdr + raw) == (R.GOOD, len(hdr))
    f = hdr + raw + struct.pack("<II", zlib.crc32(plain), len(plain))
    z = ref.wrap(raw, plain, ref.ZLIB)
    n = w.n_units
    cap = lambda sizes: n + len(sizes) + 12
    rd = eng.open_one_reader("gzip")
    read = reader(rd, False)

    def go(member, sizes, r=read, handle=rd):
        handle.reset()
        return R.feed(r, member, iter(sizes), None, cap(sizes) + 24, grow=1)

    # the header cut: nothing is used until it is whole and a unit behind it is
    for cut in (1, 3, 9, 10, 12, len(hdr) - 1, len(hdr)):
        rd.reset()
        assert read(f[:cut], False, None)[0] == R.Call(R.OK, 0, 0, 0, -1), cut
        c, first = read(f[:len(hdr) + w.reach[0]], False, None)
        assert (c.rc, c.n_units, first) == (R.OK, 1, plain[:w.out_off[1]]) and c.in_used == len(hdr) + w.unit_bit[1] // 8, cut
        calls, got, rest = R.feed(read, f[c.in_used:], iter([65536]), None, n + 8)
        assert calls[-1].rc == R.STREAM_END and first + got == plain and c.in_used + sum(x.in_used for x in calls) == len(f)
    # the trailer in a call of its own, and cut at each of its positions
    for j in range(9):
        calls, got, rest = go(f, [len(f) - 8 + j])
        assert got == plain and calls[-1].rc == R.STREAM_END and sum(c.in_used for c in calls) == len(f), j
        if j < 8:
            assert (calls[0].rc, calls[0].in_used, calls[0].out_len) == (R.OK, len(f) - 8, len(plain)), j
            assert calls[-1] == R.Call(R.STREAM_END, 8, 0, 0, -1), j
    rdz = eng.open_one_reader("zlib", device=True)
    for j in range(5):
        calls, got, rest = go(z, [len(z) - 4 + j], reader(rdz, True), rdz)
        assert got == plain and calls[-1].rc == R.STREAM_END and sum(c.in_used for c in calls) == len(z), j
    # a wrong CRC-32, ISIZE or Adler-32 fails at the last call, err_off = the member's length
    for member, at, r, h in ((f, -6, read, rd), (f, -2, read, rd), (z, -1, reader(rdz, True), rdz)):
        bad = bytearray(member)
        bad[at] ^= 4
        for sizes in ([len(member)], [len(member) - 5], [65536, 65536]):
            calls, got, rest = go(bytes(bad), sizes, r, h)
            assert (calls[-1].rc, calls[-1].err_off) == (R.CORRUPT, len(member)) and got == plain, (at, sizes)
            assert all(c.rc == R.OK for c in calls[:-1])
    rdz.close()
    # final_in with a truncated stream: the bytes in front are delivered, as the whole call delivers them
    cut = f[:len(f) * 2 // 3]
    st, eo, ol, out, _ = whole(eng, cut, ref.GZIP)
    assert st == ref.UNEXPECTED_EOF and 0 < ol < len(plain)
    for sizes in ([len(cut)], [len(cut) // 2]):
        calls, got, rest = go(cut, sizes)
        assert (calls[-1].rc, calls[-1].err_off) == (R.EOF, -1) and got == out, sizes
    # (reset and a second stream on the same handle: every `go` above); junk behind the trailer is left unused
    junk = f + b"junk behind the member"
    for sizes in ([len(junk)], [len(f) - 3], [65536]):
        calls, got, rest = go(junk, sizes)
        assert calls[-1].rc == R.STREAM_END and got == plain and sum(c.in_used for c in calls) == len(f), sizes
    # a bad header is bad on the first part, whatever follows
    calls, got, rest = go(b"\x1f\x8b\x09" + f[3:], [2, 2])
    assert [c.rc for c in calls] == [R.OK, R.CORRUPT] and calls[-1].err_off == 0
    rd.close()


# ---- 8. the unchanged path ----

def test_the_whole_calls_are_unchanged_after_a_reader_has_run(eng, streams):
    raw, plain, w = streams["level 6"]
    f = ref.wrap(raw, plain, ref.GZIP)
    rd = eng.open_one_reader("gzip")
    calls, got, _ = R.feed(reader(rd, False), f, fixed(50001), None, w.n_units + 16)  # (stops at odd carry bits)
    assert got == plain and any(w.unit_bit[sum(c.n_units for c in calls[:i + 1])] % 8 for i in range(len(calls) - 1))
    assert whole(eng, f, ref.GZIP) == (0, -1, len(plain), plain, w.n_units)
    out, q = eng.gzfile_read(np.frombuffer(f + f, np.uint8))
    assert (q.rc, q.out_len, q.n_members) == (0, 2 * len(plain), 2) and bytes(out[:q.out_len]) == plain + plain
    ix = eng.inflate_one_index(np.frombuffer(f, np.uint8), "gzip")
    assert list(ix.unit_bit) == w.unit_bit and list(ix.out_off) == w.out_off
    rd.close()
