"""BGZF random access on the GPU: flate_hip_bgzf_read_ranges.  Every expectation comes from the CPU: the Python model
tests/bgzf_range_ref.py (positions, validity, touched set, out_off, statuses, the order of the verdict) on top of the
serial walk of tests/bgzf_ref.py, and gzip's own reader for the bytes."""
import ctypes as C
import gzip

import numpy as np
import pytest

import bgzf_range_ref as model
import bgzf_ref as ref
from util import flate

pytestmark = pytest.mark.gpu

DEVICE_PTRS = 1
GUARD = 0xA5
BYTES, VIRTUAL = model.POS_BYTES, model.POS_VIRTUAL


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def many():
    """ref.many_members(1025) with its walk and its bytes (computed once, shared, never changed)."""
    f, plain = ref.many_members(1025)
    return f, ref.Walk(f), plain


class Got:
    pass


def run(eng, f, kind, ranges, cap, device=False, shift=0, out_shift=0, null_out=False):
    """One flate_hip_bgzf_read_ranges call into a prefilled buffer; the guard bytes around the capacity and behind the
    host arrays must have stayed what they were."""
    import torch
    n, nr = len(f), len(ranges)
    begin = np.array([b for b, _ in ranges] + [0], np.uint64)
    end = np.array([e for _, e in ranges] + [0], np.uint64)
    obuf = np.full(out_shift + cap + 64, GUARD, np.uint8)
    if device:
        keep = torch.from_numpy(np.frombuffer(b"\0" * shift + bytes(f) + b"\0" * 64, np.uint8).copy()).cuda()
        ptr = keep.data_ptr() + shift
        d_out = torch.from_numpy(obuf).cuda()
        out_ptr = d_out.data_ptr() + out_shift
    else:
        keep = np.frombuffer(b"\0" * shift + bytes(f) + b"\0", np.uint8).copy()
        ptr, out_ptr = keep.ctypes.data + shift, obuf.ctypes.data + out_shift
    out_off = np.full(nr + 3, 7, np.uint64)
    status = np.full(nr + 2, 99, np.int32)
    nm, nd, bad, eo = C.c_uint32(99), C.c_uint32(99), C.c_uint32(99), C.c_int64(99)
    g = Got()
    g.rc = eng._L.flate_hip_bgzf_read_ranges(eng._ctx, ptr if n else None, n, kind, begin.ctypes.data, end.ctypes.data, nr,
                                             None if null_out else out_ptr, cap, out_off.ctypes.data, status.ctypes.data,
                                             C.byref(nm), C.byref(nd), C.byref(bad), C.byref(eo),
                                             DEVICE_PTRS if device else 0)
    if device:
        torch.cuda.synchronize()
        obuf = d_out.cpu().numpy()
    assert (out_off[nr + 1:] == 7).all() and (status[nr:] == 99).all(), "the host arrays were written past their end"
    g.out_off, g.status = [int(x) for x in out_off[:nr + 1]], [int(x) for x in status[:nr]]
    g.n_members, g.n_decoded, g.bad_member, g.err_off = nm.value, nd.value, bad.value, eo.value
    g.obuf, g.out_shift, g.cap = obuf, out_shift, cap
    g.body = obuf[out_shift:out_shift + cap]
    return g


def guards_ok(g, used):
    """Nothing in front of out, nothing behind the delivered bytes."""
    return (g.obuf[:g.out_shift] == GUARD).all() and (g.obuf[g.out_shift + used:] == GUARD).all()


def check(eng, f, kind, ranges, what, status=None, **kw):
    """One call against the model, with exactly the capacity that is needed."""
    R = model.read_ranges(f, kind, [b for b, _ in ranges], [e for _, e in ranges], status=status)
    g = run(eng, f, kind, ranges, R.out_off[-1], **kw)
    assert (g.rc, g.n_members, g.n_decoded, g.bad_member, g.err_off) == \
        (R.rc, R.n_members, R.n_decoded, R.bad_member, R.err_off), (what, kw, g.rc, g.n_decoded, g.bad_member, g.err_off)
    assert g.out_off == R.out_off, (what, kw)
    assert g.status == R.range_status, (what, kw)
    assert guards_ok(g, R.out_off[-1]), (what, kw, "guard bytes touched")
    got = g.body[:R.out_off[-1]].tobytes()
    if all(R.exact):
        assert got == R.data, (what, kw)
    else:
        for r in range(len(ranges)):
            if R.exact[r]:
                assert got[R.out_off[r]:R.out_off[r + 1]] == R.data[R.out_off[r]:R.out_off[r + 1]], (what, kw, r)
    return R, g


# ---- 1. exhaustive tiny file ----

def test_every_range_of_a_tiny_file_in_one_call(eng, oracle):
    data = ref.text(45)
    f, _ = ref.build_file(oracle, data, 7)
    w = ref.Walk(f)
    assert w.n_members == 8 and gzip.decompress(f) == data
    pairs = [(b, e) for b in range(48) for e in range(b, 48)]
    v = model.valid_virtual_offsets(w, f)
    vpairs = [(v[i], v[j]) for i in range(len(v)) for j in range(i, len(v))]
    for device in (False, True):
        R, _ = check(eng, f, BYTES, pairs, "tiny bytes", device=device, shift=5 if device else 0, out_shift=3)
        assert R.n_decoded == 7 and R.rc == 0
        R, _ = check(eng, f, VIRTUAL, vpairs, "tiny virtual", device=device, shift=11 if device else 0, out_shift=9)
        assert R.n_decoded == 7 and R.rc == 0 and R.out_off[-1] > 0


# ---- 2. member edges ----

def test_member_edges_in_bytes(eng, many):
    f, w, plain = many
    ranges = model.byte_edge_ranges(w)
    # ranges wholly inside runs of empty members deliver nothing, touch nothing; and the whole file as one range
    empty_runs = [k for k in range(w.n_members - 1) if w.out_off[k] == w.out_off[k + 1] == w.out_off[k + 2]]
    assert len(empty_runs) > 100
    for device in (False, True):
        check(eng, f, BYTES, ranges, "edges", device=device, shift=7 if device else 0, out_shift=1)
    R, g = check(eng, f, BYTES, [(0, w.out_bytes)], "the whole file", device=True, out_shift=13)
    assert R.data == plain and R.n_decoded == sum(1 for k in range(w.n_members) if w.out_off[k + 1] > w.out_off[k])
    inside = [(w.member_off[k] << 16, w.member_off[k + 1] << 16) for k in empty_runs[:300]]
    R, g = check(eng, f, VIRTUAL, inside, "inside runs of empty members", device=True)
    assert (g.rc, g.n_decoded, g.out_off[-1]) == (0, 0, 0)
    p = w.out_off[empty_runs[0]]
    R, g = check(eng, f, BYTES, [(p, p)] * 5, "empty byte ranges", device=True)
    assert (g.rc, g.n_decoded, g.out_off[-1]) == (0, 0, 0)


def test_member_edges_in_virtual_offsets(eng, many):
    f, w, plain = many
    ranges = model.virtual_edge_ranges(f, w)
    for device in (False, True):
        R, g = check(eng, f, VIRTUAL, ranges, "virtual edges", device=device, shift=3 if device else 0, out_shift=6)
        assert R.rc == -1 and -1 in R.range_status and 0 in R.range_status
        for r, st in enumerate(g.status):
            if st == -1:
                assert g.out_off[r] == g.out_off[r + 1]


def test_decoys_are_not_valid_virtual_offsets(eng):
    for k, (what, f) in enumerate(ref.decoy_files()):
        w = ref.Walk(f)
        decoys = model.decoy_offsets(f, w)
        assert decoys or "past in_len" in what, what
        ranges = model.virtual_edge_ranges(f, w) + [(0, len(f) << 16)]
        R, g = check(eng, f, VIRTUAL, ranges, what, device=bool(k & 1), shift=k + 1 if k & 1 else 0)
        for r, (b, e) in enumerate(ranges):
            if b >> 16 in decoys or e >> 16 in decoys:
                assert g.status[r] == -1, (what, b, e)
            elif b >> 16 in w.member_off and e >> 16 in w.member_off and not b & 0xffff and not e & 0xffff:
                assert g.status[r] == 0, (what, b, e)
        assert g.body[g.out_off[-2]:g.out_off[-1]].tobytes() == gzip.decompress(f)


# ---- 3. gather alignment ----

LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537]


def test_gather_at_every_alignment_of_source_and_destination(eng):
    rng = np.random.default_rng(12)
    payloads = [rng.integers(0, 256, ref.FULL_PAYLOAD, dtype=np.uint8).tobytes() for _ in range(4)]
    f = b"".join(ref.stored_member(p) for p in payloads) + ref.EOF
    U = b"".join(payloads)
    ranges, k = [], 0
    for m in range(16):
        for n in LENGTHS:
            b = 16 * ((k * 131) % 12000) + m
            ranges.append((b, b + n))
            k += 1
    assert all(e <= len(U) for _, e in ranges)
    want = b"".join(U[b:e] for b, e in ranges)
    for shift in range(16):
        g = run(eng, f, BYTES, ranges, len(want), device=True, shift=(3 * shift) % 16, out_shift=shift)
        assert g.rc == 0 and g.out_off[-1] == len(want), shift
        assert guards_ok(g, len(want)), (shift, "guard bytes touched")
        assert g.body.tobytes() == want, shift
    g = run(eng, f, BYTES, ranges, len(want), out_shift=5)  # host pointers: staged, copied back once
    assert g.rc == 0 and guards_ok(g, len(want)) and g.body.tobytes() == want


# ---- 4. once per call ----

def test_every_touched_member_is_decoded_once(eng, many):
    f, w, plain = many
    rng = np.random.default_rng(4)
    k = next(k for k in range(w.n_members) if w.out_off[k + 1] - w.out_off[k] == ref.FULL_PAYLOAD)
    lo, hi = w.out_off[k], w.out_off[k + 1]
    inside = [tuple(sorted(int(x) for x in rng.integers(lo, hi + 1, 2))) for _ in range(1000)]
    R, g = check(eng, f, BYTES, inside, "1000 ranges inside one member", device=True)
    assert g.n_decoded == 1 and g.rc == 0
    T = w.out_bytes
    mixed = [tuple(sorted(int(x) for x in rng.integers(0, T + 1, 2))) for _ in range(40)]
    mixed = [(b, min(e, b + 3000)) for b, e in mixed] * 3 + [(0, 100), (50, 150), (T - 10, T + 10)]
    rng.shuffle(mixed)
    R, g = check(eng, f, BYTES, [tuple(x) for x in mixed], "shuffled, overlapping, duplicated", device=True, out_shift=2)
    assert 1 < g.n_decoded < 200
    for n in (255, 256, 257, 65537):
        at = rng.integers(0, T, n)
        R, g = check(eng, f, BYTES, [(int(p), int(p) + 1) for p in at], "%d one-byte ranges" % n, device=n != 256)
        assert g.out_off[-1] == n and g.rc == 0


# ---- 5. only what is touched ----

def test_only_touched_members_are_verified(eng):
    for what, f, want_rc, want_bad in ref.failing_files():
        w = ref.Walk(f)
        status = {want_bad: want_rc}
        if "two failures" in what:
            status[2] = ref.CORRUPT
        good = [k for k in range(w.n_members) if k not in status and w.out_off[k + 1] > w.out_off[k]]
        avoid = [(w.out_off[k], w.out_off[k + 1]) for k in good] + [(w.out_off[k] + 5, w.out_off[k] + 900) for k in good]
        through = [(w.out_off[want_bad] + 1, w.out_off[want_bad] + 2), (0, w.out_bytes)]
        for device in (False, True):
            R, g = check(eng, f, BYTES, avoid, what, status=status, device=device, shift=3 if device else 0)
            assert g.rc == 0 and g.n_decoded == len(good) and all(s == 0 for s in g.status), what
            _, r = eng.bgzf_read(np.frombuffer(f, np.uint8))
            assert (r.rc, r.bad_member) == (want_rc, want_bad), what  # the whole file still fails
            R, g = check(eng, f, BYTES, avoid[:1] + through + avoid[1:], what, status=status, device=device)
            assert (g.rc, g.bad_member, g.err_off) == (want_rc, want_bad, w.member_off[want_bad]), what
            assert g.status[1] == want_rc and g.status[2] == want_rc and g.status[0] == 0, what
            vr = [(w.member_off[k] << 16 | 1, w.member_off[k + 1] << 16) for k in sorted(status)[-1:]] + \
                 [(w.member_off[good[0]] << 16, w.member_off[good[0]] << 16 | 7)]
            R, g = check(eng, f, VIRTUAL, vr, what, status=status, device=device)
            assert g.status == [status[sorted(status)[-1]], 0], what


# ---- 6. chains ----

def test_malformed_chains(eng):
    for k, (what, f, err_off, n_good) in enumerate(ref.malformed_files()):
        for device in (False, True):
            for kind in (BYTES, VIRTUAL):
                g = run(eng, f, kind, [(0, 0), (0, 1 << 16), (5, 9)], 8192, device=device, shift=(k + 1) % 16 if device else 0)
                assert (g.rc, g.err_off, g.bad_member, g.n_members, g.n_decoded) == (ref.CORRUPT, err_off, n_good, n_good, 0), what
                assert g.out_off == [0, 0, 0, 0] and g.status == [ref.CORRUPT] * 3, what
                assert (g.obuf == GUARD).all(), (what, "nothing may be written")
                R = model.read_ranges(f, kind, [0, 0, 5], [0, 1 << 16, 9], out_cap=8192)
                assert (R.rc, R.err_off, R.bad_member, R.out_off, R.range_status) == \
                    (g.rc, g.err_off, g.bad_member, g.out_off, g.status), what


# ---- 7. capacity ----

def test_capacity_and_the_size_query(eng, oracle):
    data = ref.write_inputs()[2 * 65280]
    f, _ = ref.build_file(oracle, data, 4096)
    w = ref.Walk(f)
    ranges = [(10, 5000), (0, 0), (4000, 70000), (len(data) - 3, len(data) + 3)]
    want = b"".join(data[b:e] for b, e in ranges)
    need = len(want)
    for device in (False, True):
        g = run(eng, f, BYTES, ranges, need - 1, device=device)
        assert (g.rc, g.out_off[-1], g.n_members) == (-2, need, w.n_members) and (g.obuf == GUARD).all(), device
        g = run(eng, f, BYTES, ranges, need, device=device)
        assert g.rc == 0 and g.body.tobytes() == want and guards_ok(g, need), device
        g = run(eng, f, BYTES, ranges, 0, device=device, null_out=True)  # the size query
        assert (g.rc, g.out_off[-1]) == (-2, need) and (g.obuf == GUARD).all(), device
        g = run(eng, f, BYTES, [(7, 7), (len(data), len(data) + 9)], 0, device=device, null_out=True)
        assert (g.rc, g.out_off, g.n_decoded) == (0, [0, 0, 0], 0), device  # a total of 0 is no query
        # no ranges: nothing is read, not even a malformed chain
        g = run(eng, f[:100], BYTES, [], 16, device=device)
        assert (g.rc, g.out_off, g.n_members) == (0, [0], 0) and (g.obuf == GUARD).all(), device
        # an empty file: every byte range is empty, virtual offset 0 is the only valid one
        g = run(eng, b"", BYTES, [(0, 0), (0, 9), (3, model.U64_MAX)], 16, device=device)
        assert (g.rc, g.out_off, g.status, g.n_members, g.n_decoded) == (0, [0] * 4, [0] * 3, 0, 0), device
        g = run(eng, b"", VIRTUAL, [(0, 0), (0, 1), (1 << 16, 1 << 16)], 16, device=device)
        assert (g.rc, g.out_off, g.status) == (-1, [0] * 4, [0, -1, -1]) and (g.obuf == GUARD).all(), device
        # the EOF marker alone: one member, no bytes
        g = run(eng, ref.EOF, BYTES, [(0, 5)], 16, device=device)
        assert (g.rc, g.out_off, g.n_members, g.n_decoded) == (0, [0, 0], 1, 0), device
        g = run(eng, ref.EOF, VIRTUAL, [(0, 28 << 16), (0, 1), (28 << 16, 28 << 16 | 1)], 16, device=device)
        assert (g.rc, g.out_off, g.status, g.n_decoded) == (-1, [0] * 4, [0, -1, -1], 0), device
    # refusals before any HIP call, through the real entry point
    lo, hi, off = np.array([5], np.uint64), np.array([4], np.uint64), np.zeros(2, np.uint64)
    src = np.frombuffer(f, np.uint8)
    L, out = eng._L.flate_hip_bgzf_read_ranges, np.zeros(64, np.uint8)
    args = lambda kind, b, e, flags: (eng._ctx, src.ctypes.data, len(f), kind, b.ctypes.data, e.ctypes.data, 1,
                                      out.ctypes.data, 64, off.ctypes.data, None, None, None, None, None, flags)
    assert L(*args(0, lo, hi, 0)) == -1 and L(*args(1, lo, hi, 0)) == -1   # begin > end
    assert L(*args(2, hi, lo, 0)) == -1 and L(*args(0, hi, lo, 8)) == -1   # pos_kind, flags
    assert L(*args(0, hi, lo, 0)) == 0 and out[0] == data[4]               # every optional pointer NULL


# ---- 8. a real-sized mix ----

def test_a_real_sized_mix(eng):
    import torch
    text = flate.synth("text", 128, 65536).tobytes()
    ours = eng.bgzf_write(np.frombuffer(text, np.uint8))
    rng = np.random.default_rng(21)
    cuts, p = [0], 0
    while p < len(text):
        p = min(len(text), p + int(rng.choice([1, 300, 9000, 40000, 65000])))
        cuts.append(p)
    foreign = b"".join(ref.zlib_member(text[a:b]) for a, b in zip(cuts, cuts[1:])) + ref.EOF
    T = len(text)
    lens = np.concatenate([(2.0 ** rng.uniform(0, 18, 1990)).astype(np.int64) - 1, [0, 0, T, T // 2, T // 3, 70000, 1 << 20, 3 << 20, 65536, 65537]])
    begins = [int(rng.integers(0, T - n + 1)) for n in lens]
    ranges = [(b, b + int(n)) for b, n in zip(begins, lens)]
    want = b"".join(text[b:e] for b, e in ranges)
    for f in (ours, foreign):
        assert gzip.decompress(f) == text
        w = ref.Walk(f)
        d_f = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).cuda()
        for device in (True, False):
            out, r = eng.bgzf_read_ranges(d_f if device else np.frombuffer(f, np.uint8), [b for b, _ in ranges],
                                          [e for _, e in ranges])
            assert (r.rc, r.n_members, r.bad_member, r.err_off) == (0, w.n_members, 0xffffffff, -1)
            assert int(r.out_off[-1]) == len(want) and not r.range_status.any()
            assert r.n_decoded == sum(1 for k in range(w.n_members) if w.out_off[k + 1] > w.out_off[k])
            got = out[:len(want)].cpu().numpy() if device else out[:len(want)]
            assert got.tobytes() == want, device


# ---- 9. the Python mirror ----

def test_engine_bgzf_read_ranges(eng, many):
    import torch
    f, w, plain = many
    begin, end = [0, 70000, 5, len(plain) - 1], [10, 140001, 5, len(plain) + 100]
    want = b"".join(plain[b:e] for b, e in zip(begin, end))
    R = model.read_ranges(f, BYTES, begin, end)
    src = np.frombuffer(f, np.uint8)
    for data in (src, f, torch.from_numpy(src.copy()).cuda()):
        out, r = eng.bgzf_read_ranges(data, begin, end)
        assert (r.rc, r.n_members, r.n_decoded, r.bad_member, r.err_off) == (0, w.n_members, R.n_decoded, 0xffffffff, -1)
        assert [int(x) for x in r.out_off] == R.out_off and list(r.range_status) == [0] * 4
        got = out[:len(want)]
        assert (got.cpu().numpy() if hasattr(got, "cpu") else got).tobytes() == want
    # a caller's buffer, too small and large enough; virtual offsets, one of them invalid
    out = np.full(len(want) + 8, GUARD, np.uint8)
    _, r = eng.bgzf_read_ranges(src, begin, end, out=out, out_cap=len(want) - 1)
    assert r.rc == -2 and int(r.out_off[-1]) == len(want) and (out == GUARD).all()
    _, r = eng.bgzf_read_ranges(src, begin, end, out=out)
    assert r.rc == 0 and out[:len(want)].tobytes() == want and (out[len(want):] == GUARD).all()
    k = next(k for k in range(w.n_members) if w.out_off[k + 1] - w.out_off[k] > 20)
    v = w.member_off[k] << 16
    out, r = eng.bgzf_read_ranges(src, [v | 3, v + (1 << 16)], [v | 9, v + (1 << 16) + 1], virtual=True)
    assert r.rc == -1 and list(r.range_status) == [0, -1] and [int(x) for x in r.out_off] == [0, 6, 6]
    assert out[:6].tobytes() == plain[w.out_off[k] + 3:w.out_off[k] + 9]
    with pytest.raises(flate.FlateError):
        eng.bgzf_read_ranges(src, [5], [4])
