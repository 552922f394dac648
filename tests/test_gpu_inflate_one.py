"""One long DEFLATE stream on the GPU: flate_hip_inflate_one_index.  Every expectation comes from the CPU: tests/one_ref.py
(the corpus, the bit-level block walker, zlib for the bytes); the walker's verdicts on the failing streams are first
held against the batch decoder's (flate_hip_inflate_batch on the same bytes as one stream), the yardstick of the
call's status and err_off."""
import ctypes as C
import struct

import numpy as np
import pytest

import deflate_corpus as dc
import one_ref as ref
from util import flate

pytestmark = pytest.mark.gpu

DEVICE_PTRS = 1
INVALID, OUT_TOO_SMALL = -1, -2
KINDS = (ref.RAW, ref.ZLIB, ref.GZIP)


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def good(oracle):
    """[(what, raw stream, plain, Walk)]: computed once, shared, never changed."""
    return [(w, r, p, ref.Walk(r)) for w, r, p in ref.good_streams(oracle)]


def on_device(b, shift=0, pad=64):
    """bytes -> (keep-alive tensor, device pointer of the first byte): the stream at byte `shift` of a larger tensor."""
    import torch
    t = torch.from_numpy(np.frombuffer(b"\xee" * shift + bytes(b) + b"\xee" * pad, np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + shift


def index(eng, f, kind, n_units, device=False, shift=0, cap=None, query=False):
    """One call -> (rc, n_units, out_bytes, n_candidates, status, err_off, unit_bit, out_off)."""
    n = len(f)
    keep, ptr = on_device(f, shift) if device else (np.frombuffer(b"\xee" * shift + bytes(f) + b"\xee", np.uint8).copy(), None)
    if not device:
        ptr = keep.ctypes.data + shift
    if cap is None:
        cap = n_units + 1
    ubit, ooff = np.full(cap + 2, 7, np.uint64), np.full(cap + 2, 7, np.uint64)
    nu, ob, nc, st, eo = C.c_uint32(99), C.c_uint64(99), C.c_uint32(99), C.c_int32(99), C.c_int64(99)
    rc = eng._L.flate_hip_inflate_one_index(eng._ctx, ptr if n else None, n, kind, 0 if query else cap,
                                            None if query else ubit.ctypes.data, None if query else ooff.ctypes.data,
                                            C.byref(nu), C.byref(ob), C.byref(nc), C.byref(st), C.byref(eo),
                                            DEVICE_PTRS if device else 0)
    assert (ubit[cap:] == 7).all() and (ooff[cap:] == 7).all(), "the arrays were written past index_cap"
    return rc, nu.value, ob.value, nc.value, st.value, eo.value, ubit, ooff


def check_index(eng, raw, plain, w, what, kind=ref.RAW, **kw):
    """The call equals the walk w: verdict, counts and -- of a failing stream too -- the index of the good units."""
    rc, nu, ob, nc, st, eo, ubit, ooff = index(eng, ref.wrap(raw, plain, kind), kind, w.n_units, **kw)
    assert (rc, st, nu, ob, eo) == (w.status, w.status, w.n_units, w.out_bytes, w.err_off), (what, kind, kw)
    assert nc >= nu and (nc >= 1 or not raw), (what, kind, kw, nc)  # (no input at all: nothing is probed)
    assert list(ubit[:nu + 1]) == w.unit_bit and list(ooff[:nu + 1]) == w.out_off, (what, kind, kw)
    return nc


# ---- the corpus ----

def test_every_stream_in_every_container(eng, good):
    for what, raw, plain, w in good:
        assert w.status == 0 and w.out_bytes == len(plain), what
        # every dynamic block the walker reaches starts a unit
        assert set(b[0] for b in w.blocks if b[1] == 2) <= set(w.unit_bit[:-1]), what
        counts = {check_index(eng, raw, plain, w, what, kind) for kind in KINDS}
        assert len(counts) == 1, (what, counts)  # the candidates are the raw stream's, whatever is around it


def test_device_pointers_and_shifted_buffers(eng, good):
    for k in (1, ref.MANY_UNITS, 6, 8):
        what, raw, plain, w = good[k]
        for shift in (0, 1, 3):
            check_index(eng, raw, plain, w, what, ref.GZIP, device=True, shift=shift)
    what, raw, plain, w = good[ref.MANY_UNITS]
    check_index(eng, raw, plain, w, what, ref.ZLIB, shift=3)
    check_index(eng, raw, plain, w, what, ref.RAW, device=True, shift=5)


def test_candidates_are_exactly_the_rule_hits_and_decoys_are_off_the_path(eng, good):
    for what, raw, plain in ref.decoy_streams():
        w = ref.Walk(raw)
        assert w.status == 0 and w.n_units == 1, what
        nc = check_index(eng, raw, plain, w, what)
        assert nc == len(ref.candidates(raw)) and nc > w.n_units, (what, nc)
    for k in (9, 10, 11):  # the small streams of the corpus
        what, raw, plain, w = good[k]
        assert check_index(eng, raw, plain, w, what, ref.GZIP) == len(ref.candidates(raw)), what


def test_query_capacity_and_the_python_wrapper(eng, good):
    what, raw, plain, w = good[ref.MANY_UNITS]
    f = ref.wrap(raw, plain, ref.GZIP)
    rc, nu, ob, nc, st, eo, _, _ = index(eng, f, ref.GZIP, w.n_units, query=True)
    assert (rc, nu, ob, st, eo) == (0, w.n_units, len(plain), 0, -1)
    rc, nu, ob, nc, st, eo, ubit, _ = index(eng, f, ref.GZIP, w.n_units, cap=w.n_units)  # one entry short
    assert (rc, nu, ob, st) == (OUT_TOO_SMALL, w.n_units, len(plain), 0) and (ubit == 7).all()
    ix = eng.inflate_one_index(np.frombuffer(f, np.uint8), "gzip")
    assert (ix.rc, ix.n_units, ix.out_bytes, ix.status, ix.err_off) == (0, w.n_units, len(plain), 0, -1)
    assert list(ix.unit_bit) == w.unit_bit and list(ix.out_off) == w.out_off
    q = eng.inflate_one_index(f, "gzip", query=True)
    assert q.unit_bit is None and q[:6] == ix[:6]
    import torch
    d = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()
    assert eng.inflate_one_index(d, "raw")[:6] == ix[:6]
    # refused before any HIP call
    src = np.frombuffer(f, np.uint8).copy()
    nu32, ob64, st32, one = C.c_uint32(0), C.c_uint64(0), C.c_int32(0), np.zeros(4, np.uint64)
    L = eng._L
    for wrap, a, b, flags in ((3, None, None, 0), (2, one.ctypes.data, None, 0), (2, None, None, 8), (2, None, None, 2)):
        assert L.flate_hip_inflate_one_index(eng._ctx, src.ctypes.data, len(f), wrap, 4 if a else 0, a, b, C.byref(nu32),
                                             C.byref(ob64), None, C.byref(st32), None, flags) == INVALID


# ---- failing streams ----

def failing_streams(good):
    """[(what, raw stream)]: unique streams that the serial decoder refuses somewhere, or that it must not."""
    seen, out = set(), []

    def add(what, raw):
        if bytes(raw) not in seen:
            seen.add(bytes(raw))
            out.append((what, bytes(raw)))

    for c in dc.CASES:
        add(c.name, c.data)
    for name, data, _, zdict in dc.variants():
        if not zdict:
            add(name, data)
    _, raw, _, w = good[ref.MANY_UNITS]
    mid = w.n_units // 2
    for what, u in (("first", 0), ("a middle", mid), ("the last", w.n_units - 1)):
        add("cut inside %s unit" % what, raw[:(w.unit_bit[u] + w.unit_bit[u + 1]) // 16])
    for what, bit in (("header", w.unit_bit[mid] + 20), ("body", (w.unit_bit[mid] + w.unit_bit[mid + 1]) // 2)):
        flipped = bytearray(raw)
        flipped[bit >> 3] ^= 1 << (bit & 7)
        add("one flipped bit in a middle unit's %s" % what, flipped)
    add("cut in front of the last byte", raw[:-1])
    legal, _, illegal = ref.history_pair()
    add("a distance to the stream's first byte", legal)
    add("a distance one byte in front of the stream", illegal)
    return out


def test_failing_streams_have_the_serial_decoders_verdict(eng, good):
    cases = failing_streams(good)
    walks = [ref.Walk(raw) for _, raw in cases]
    assert sum(1 for w in walks if w.status == ref.CORRUPT) > 50 and sum(1 for w in walks if w.status == ref.UNEXPECTED_EOF) > 50
    # the yardstick: the batch decoder on the same bytes, one stream each, with room for everything they produce
    off = np.zeros(len(cases) + 1, np.uint64)
    np.cumsum(np.array([len(r) for _, r in cases], dtype=np.uint64), out=off[1:])
    data = np.frombuffer(b"".join(r for _, r in cases) + b"\0" * 8, np.uint8).copy()
    _, _, olen, status, err = eng.inflate_batch(data, off, [w.out_len + 600 for w in walks], check=False)
    history = 0
    for (what, raw), w, s, e, n in zip(cases, walks, status, err, olen):
        if w.far and (int(s), int(e)) != (w.status, w.err_off):
            history += 1  # the one verdict that depends on history: the decoder's, not the index's
            assert int(s) == ref.CORRUPT, what
        else:
            assert (int(s), int(e), int(n)) == (w.status, w.err_off, w.out_len), (what, int(s), int(e), w.status, w.err_off)
    assert history >= 1
    for (what, raw), w in zip(cases, walks):
        check_index(eng, raw, b"", w, what)


def test_failing_streams_inside_containers(eng, good):
    _, raw, plain, w = good[ref.MANY_UNITS]
    cut = raw[:(w.unit_bit[5] + w.unit_bit[6]) // 16]
    wc = ref.Walk(cut)
    assert wc.status == ref.UNEXPECTED_EOF and wc.n_units == 5
    for kind in (ref.ZLIB, ref.GZIP):
        check_index(eng, cut, plain, wc, "cut inside unit 5", kind, device=True, shift=1)
    flipped = bytearray(raw)
    flipped[(w.unit_bit[7] + 20) >> 3] ^= 1 << ((w.unit_bit[7] + 20) & 7)
    wf = ref.Walk(bytes(flipped))
    assert wf.status != 0 and wf.n_units == 7  # the chain stops at a header the rule refuses: the tail probe's verdict
    for kind in KINDS:
        check_index(eng, bytes(flipped), plain, wf, "a flipped header bit", kind)
    # the framed batch decoder on the same framed bytes as one stream says the same of both
    for kind, name in ((ref.ZLIB, "zlib"), (ref.GZIP, "gzip")):
        for r, wx in ((cut, wc), (bytes(flipped), wf)):
            f = np.frombuffer(ref.wrap(r, plain, kind), np.uint8)
            _, _, olen, status = eng.inflate_batch_framed(f, np.array([0, f.size], np.uint64), name, out_sizes=[len(plain)])
            assert (int(status[0]), int(olen[0])) == (wx.status, wx.out_len), (name, int(status[0]), wx.status)
    # a wrong trailer is a decode's business, a bad header is this call's: FLATE_HIP_E_CORRUPT at offset 0, no units
    f = bytearray(ref.wrap(raw, plain, ref.GZIP))
    f[-5] ^= 0x10
    assert index(eng, bytes(f), ref.GZIP, w.n_units)[:6] == index(eng, ref.wrap(raw, plain, ref.GZIP), ref.GZIP, w.n_units)[:6]
    z = ref.wrap(raw, plain, ref.ZLIB)
    fdict = bytes([0x78, 0xbb]) + z[2:]
    assert (0x78 * 256 + 0xbb) % 31 == 0 and fdict[1] & 0x20
    bad = [fdict, b"\x1f\x8b\x09" + ref.wrap(raw, plain, ref.GZIP)[3:], ref.wrap(b"", b"", ref.GZIP)[:17], z[:5], b"\x78"]
    for f, kind in zip(bad, (ref.ZLIB, ref.GZIP, ref.GZIP, ref.ZLIB, ref.ZLIB)):
        rc, nu, ob, nc, st, eo, ubit, ooff = index(eng, f, kind, 0, device=len(f) > 4)
        assert (rc, nu, ob, nc, st, eo, ubit[0], ooff[0]) == (ref.CORRUPT, 0, 0, 0, ref.CORRUPT, 0, 0, 0), (f[:4], kind)
    # nothing at all
    for kind, want in ((ref.RAW, (ref.UNEXPECTED_EOF, -1)), (ref.ZLIB, (ref.CORRUPT, 0)), (ref.GZIP, (ref.CORRUPT, 0))):
        rc, nu, ob, nc, st, eo, _, _ = index(eng, b"", kind, 0)
        assert (rc, st, eo, nu, ob) == (want[0], want[0], want[1], 0, 0), kind
    # a container around no raw stream at all: the header is fine, the stream ends in front of its first block
    rc, nu, ob, nc, st, eo, _, _ = index(eng, ref.wrap(b"", b"", ref.GZIP), ref.GZIP, 0)
    assert (rc, st, eo, nu, nc) == (ref.UNEXPECTED_EOF, ref.UNEXPECTED_EOF, -1, 0, 1)


def test_a_unit_beyond_one_unit_max_is_too_large(eng, good):
    """The limit is on the reader's byte count: a unit is too large iff the reader, counting from the byte that holds
    the unit's first bit, takes more than "one_unit_max" bytes before the unit ends."""
    what, raw, plain, w = good[ref.MANY_UNITS]
    needs = [r - (u >> 3) for r, u in zip(w.reach, w.unit_bit)]
    assert len(needs) == w.n_units
    limit = sorted(needs)[len(needs) // 2]  # about half of the units need more bytes than this
    first = next(k for k, n in enumerate(needs) if n > limit)
    assert 0 < first and needs[first - 1] <= limit
    try:
        for lim, nu_want in ((limit, first), (needs[first] - 1, first), (max(needs), None)):
            eng.set_option("one_unit_max", lim)
            rc, nu, ob, nc, st, eo, ubit, _ = index(eng, raw, ref.RAW, w.n_units)
            if nu_want is None:  # every unit fits exactly
                assert (rc, nu, ob) == (0, w.n_units, len(plain)), lim
                continue
            nu_want = next(k for k, n in enumerate(needs) if n > lim)
            assert (rc, st, eo, ob, nu) == (ref.TOO_LARGE, ref.TOO_LARGE, -1, 0, nu_want), (lim, nu, nu_want)
            assert list(ubit[:nu + 1]) == w.unit_bit[:nu + 1]
    finally:
        eng.set_option("one_unit_max", 1 << 28)
    check_index(eng, raw, plain, w, what)
    for bad in (0, (1 << 28) + 1):
        with pytest.raises(flate.FlateError):
            eng.set_option("one_unit_max", bad)
