"""The option "one_stored_units" on the GPU: stored block headers start units too, in the one-stream calls
(flate_hip_inflate_one_index / _one / _one_seek_index / _one_ranges) and in the gzip-file calls.  Every expectation comes
from the CPU: tests/stored_ref.py (the unit rule on top of one_ref's walker, the hand-built corpus), zlib for the bytes,
and -- for the one verdict that depends on history -- the batch decoder on the same bytes as one stream."""
import zlib

import numpy as np
import pytest

import gzfile_ref
import one_ref
import stored_ref as ref
from test_gpu_inflate_one import KINDS, check_index, index
from test_gpu_inflate_one_read import read
from util import flate

pytestmark = pytest.mark.gpu

SPAN = 65536
RULE_AT, GZ_RULE_AT = 12, 8  # the rule word of the two seek indexes
GUARD_BYTES = 64


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture()
def on(eng):
    """The engine with the option on for one test; off again behind it."""
    eng.set_option("one_stored_units", 1)
    yield eng
    eng.set_option("one_stored_units", 0)


@pytest.fixture(scope="module")
def corpus():
    """[(what, raw stream, plain, the walk with the option on, the walk with it off)]: computed once, never changed."""
    return [(w, r, p, ref.Walk(r), one_ref.Walk(r)) for w, r, p in one_ref.good_streams() + one_ref.decoy_streams()]


@pytest.fixture(scope="module")
def hand():
    return [(w, r, p, ref.Walk(r), n) for w, r, p, n in ref.hand_streams()]


def by_name(corpus, start):
    return next(c for c in corpus if c[0].startswith(start))


def guarded_read(eng, f, kind, cap, out_shift=0, **kw):
    """test_gpu_inflate_one_read.read with 64 guard bytes (and out_shift more) in FRONT of out as well as the 64 behind
    it: read() prefills the buffer, puts out at out_shift and asserts that everything in front of out and behind out +
    cap is untouched, and with device pointers the bytes behind *out_len too."""
    return read(eng, f, kind, cap, out_shift=GUARD_BYTES + out_shift, **kw)


def check_read(eng, raw, plain, w, what, kind=one_ref.RAW, **kw):
    rc, got, ol, st, eo, nu, nc, _ = guarded_read(eng, one_ref.wrap(raw, plain, kind), kind, len(plain), **kw)
    assert (rc, st, eo, ol, nu) == (0, 0, -1, len(plain), w.n_units), (what, kind, kw, rc, st, eo, ol, nu)
    assert got == plain, (what, kind, kw)
    return nc


# ---- the option ----

def test_the_option_is_accepted(eng):
    eng.set_option("one_stored_units", 1)
    eng.set_option("one_stored_units", 0)
    for bad in (2, -1):
        with pytest.raises(flate.FlateError) as e:
            eng.set_option("one_stored_units", bad)
        assert e.value.code == -1  # FLATE_HIP_E_INVALID


def test_a_run_of_stored_blocks_is_units_of_its_own_under_one_unit_max(eng, corpus):
    what, raw, plain, w, w_off = by_name(corpus, "level 0 only")
    assert len(plain) == 150000 and (w_off.n_units, w.n_units) == (1, 4)
    try:
        eng.set_option("one_unit_max", 70000)
        rc, nu, ob, nc, st, eo, _, _ = index(eng, raw, one_ref.RAW, 4)
        assert (rc, st, nu, ob) == (one_ref.TOO_LARGE, one_ref.TOO_LARGE, 0, 0)
        assert guarded_read(eng, raw, one_ref.RAW, len(plain))[0] == one_ref.TOO_LARGE
        eng.set_option("one_stored_units", 1)
        check_index(eng, raw, plain, w, what)
        check_read(eng, raw, plain, w, what, one_ref.GZIP, device=True, shift=1)
    finally:
        eng.set_option("one_unit_max", 1 << 28)
        eng.set_option("one_stored_units", 0)


# ---- whole streams ----

def test_every_stream_in_every_container_with_the_option_on_and_off_again(eng, corpus):
    eng.set_option("one_stored_units", 1)
    n_on = {}
    try:
        for what, raw, plain, w, _ in corpus:
            counts = {check_index(eng, raw, plain, w, what, kind) for kind in KINDS}
            assert len(counts) == 1, (what, counts)
            n_on[what] = counts.pop()
            if len(raw) <= 20000:
                assert n_on[what] == len(ref.candidates(raw)), what
            for kind in KINDS:
                check_read(eng, raw, plain, w, what, kind, device=kind == one_ref.ZLIB)
    finally:
        eng.set_option("one_stored_units", 0)
    units = {c[0]: c[3].n_units for c in corpus}
    assert units["Z_FULL_FLUSH every 10 000 bytes: empty stored blocks inside units"] == 60
    assert units["text, 70 000 random bytes, text: stored blocks mid-stream"] == 6
    assert units["level 0 only: one unit"] == 4 and units["Z_FIXED only: one unit"] == 1
    for what, raw, plain, _, w_off in corpus:  # the same context, the option back at 0: today's units
        n_off = check_index(eng, raw, plain, w_off, what, one_ref.GZIP)
        check_read(eng, raw, plain, w_off, what, one_ref.GZIP)
        # n_candidates of EVERY stream, the long ones too: a dynamic hit has BTYPE 2 and a stored hit BTYPE 0, so the
        # two sets meet at most in bit 0, which is a candidate whatever it holds
        assert n_on[what] == n_off + len(set(ref.hits(raw)) - {0}), (what, n_on[what], n_off)
    stored = {c[0]: len(ref.hits(c[1])) for c in corpus}
    assert stored["level 0 only: one unit"] == 28
    assert stored["Z_FULL_FLUSH every 10 000 bytes: empty stored blocks inside units"] == 188


# ---- the hand-built corpus ----

def test_hand_built_streams(on, hand):
    for what, raw, plain, w, units in hand:
        assert (w.status, w.n_units) == (0, units) and zlib.decompress(raw, -15) == plain, what
        nc = check_index(on, raw, plain, w, what)
        assert nc == len(ref.candidates(raw)), what
        check_index(on, raw, plain, w, what, one_ref.GZIP, device=True, shift=3)
        for kind, kw in ((one_ref.RAW, {}), (one_ref.ZLIB, dict(device=True, shift=1, out_shift=5))):
            check_read(on, raw, plain, w, what, kind, **kw)
    inner = by_name(hand, "a stream with stored and dynamic headers inside")
    assert len(ref.candidates(inner[1])) > inner[3].n_units + 6  # the inner stream's headers: probed, off the path


def test_failing_streams_have_the_serial_decoders_verdict(on):
    cases = ref.failing_streams()
    walks = [ref.Walk(raw) for _, raw, _ in cases]
    # the yardstick of status, err_off and the bytes in front: the batch decoder on the same bytes, one stream each
    off = np.zeros(len(cases) + 1, np.uint64)
    np.cumsum(np.array([len(r) for _, r, _ in cases], dtype=np.uint64), out=off[1:])
    data = np.frombuffer(b"".join(r for _, r, _ in cases) + b"\0" * 8, np.uint8).copy()
    out, out_off, olen, status, err = on.inflate_batch(data, off, [w.out_len + 600 for w in walks], check=False)
    for k, ((what, raw, want), w) in enumerate(zip(cases, walks)):
        s, e, n = int(status[k]), int(err[k]), int(olen[k])
        assert s == want and s != 0, (what, s)
        front = bytes(out[int(out_off[k]):int(out_off[k]) + n])
        if not w.far:  # the history-free walk says the same, and the index call says what the walk says
            assert (s, e, n) == (w.status, w.err_off, w.out_len), what
        check_index(on, raw, b"", w, what)
        for device in (False, True):
            rc, got, ol, st, eo, nu, nc, body = guarded_read(on, raw, one_ref.RAW, w.out_len + 600, device=device,
                                                             shift=int(device), out_shift=3 * int(device))
            assert (rc, st, eo, ol) == (s, s, e, n), (what, device, rc, st, eo, ol)
            assert got == front, (what, device)  # the bytes in front are delivered; behind out_len: read()'s guards
            if not w.far:
                assert nu == w.n_units, (what, nu)


# ---- the seek index of one stream ----

def slices(T, w):
    """(begin, end) of the ranges of the issue around the stream's first stored block of some size: inside it, across
    its boundary, one byte, nothing, everything."""
    k = next(i for i, b in enumerate(w.blocks) if b[1] == 0 and b[3] > 1000)
    a = sum(b[3] for b in w.blocks[:k])
    z = a + w.blocks[k][3]
    cross = (a - 300, a + 300) if a >= 300 else (z - 300, min(z + 300, T))  # a dynamic block in front, else the next block
    return [(a + 100, a + 900), cross, (a + 500, a + 501), (a + 7, a + 7), (0, T)]


def test_seek_index_of_one_stream_carries_its_rule(eng, corpus):
    import torch
    other = flate.FlateEngine(0)  # a context that never set the option
    try:
        for start in ("text, 70 000 random bytes, text", "level 0 only"):
            what, raw, plain, w, w_off = by_name(corpus, start)
            f = np.frombuffer(one_ref.wrap(raw, plain, one_ref.GZIP), np.uint8).copy()
            T = len(plain)
            eng.set_option("one_stored_units", 1)
            six = eng.inflate_one_seek_index(f, "gzip", SPAN)
            eng.set_option("one_stored_units", 0)
            off = eng.inflate_one_seek_index(f, "gzip", SPAN)
            never = other.inflate_one_seek_index(f, "gzip", SPAN)
            assert (six.rc, six.status, six.n_units, six.out_bytes) == (0, 0, w.n_units, T), what
            assert int(six.index[RULE_AT]) == 1 and int(off.index[RULE_AT]) == 0
            assert off.n_units == w_off.n_units and (off.index == never.index).all(), what
            assert (np.asarray(off.windows) == np.asarray(never.windows)).all(), what
            n = six.n_units
            ubit, ooff = six.index[16:16 + n + 1], six.index[16 + n + 1:16 + 2 * (n + 1)]
            assert list(ubit) == w.unit_bit and list(ooff) == w.out_off, what
            points = [int(u) for u in six.index[16 + 2 * (n + 1):]]
            assert six.n_points == len(points) > off.n_points
            # a point inside the stored stretch: a unit that starts with a stored block, not at the stream's start
            stored_starts = {b[0] for b in w.blocks if b[1] == 0}
            assert any(p and w.unit_bit[p] in stored_starts for p in points), what
            begin, end = zip(*slices(T, w))
            want = b"".join(plain[a:b] for a, b in zip(begin, end))
            for reader in (eng, other):  # the option is 0 on both: the rule is the index's
                out, r = reader.inflate_one_ranges(f, six, begin, end, wrap="gzip")
                assert r.rc == 0 and (r.range_status == 0).all(), (what, r.rc)
                assert out[:int(r.out_off[-1])].tobytes() == want, what
            eng.set_option("one_stored_units", 1)  # ... and an index built with the option off reads by its own rule too
            out, r = eng.inflate_one_ranges(f, off, begin, end, wrap="gzip")
            eng.set_option("one_stored_units", 0)
            assert r.rc == 0 and out[:int(r.out_off[-1])].tobytes() == want, what
            d = torch.from_numpy(f).cuda()
            dix = (six.index, torch.from_numpy(np.asarray(six.windows)).cuda())
            out, r = other.inflate_one_ranges(d, dix, begin[:3], end[:3], wrap="gzip")
            assert r.rc == 0 and out[:int(r.out_off[-1])].cpu().numpy().tobytes() == b"".join(
                plain[a:b] for a, b in zip(begin[:3], end[:3])), what
            bad = six.index.copy()
            bad[RULE_AT] = 2
            with pytest.raises(flate.FlateError) as e:
                eng.inflate_one_ranges(f, (bad, six.windows), begin, end, wrap="gzip")
            assert e.value.code == -1
    finally:
        eng.set_option("one_stored_units", 0)
        other.close()


# ---- a gzip file ----

@pytest.fixture(scope="module")
def gzfile():
    members = ref.gz_members()
    f = b"".join(m for m, _ in members)
    return np.frombuffer(f, np.uint8).copy(), b"".join(p for _, p in members), members, ref.gzfile_walk(f), gzfile_ref.Walk(f)


def check_gz_index(eng, f, w):
    ix = eng.gzfile_index(f)
    assert (ix.rc, ix.status, ix.n_units, ix.n_members, ix.out_bytes, ix.bad_member, ix.err_off, ix.stream_err_off) == (
        w.status,) + w.index_words()
    assert list(ix.unit_bit) == w.unit_bit and list(ix.out_off) == w.out_off
    assert list(ix.member_off) == w.member_off and list(ix.member_unit) == w.member_unit
    return ix


def test_gzip_file_with_stored_members(eng, gzfile):
    f, plain, members, w, w_off = gzfile
    assert w.status == 0 and w.n_members == 3 and w.n_units > w_off.n_units
    # the level-0 member: its first block is stored, and a unit starts there whatever the option says
    assert (members[1][0][10] >> 1) & 3 == 0 and w.unit_bit[w.member_unit[1]] == w_off.unit_bit[w_off.member_unit[1]]
    check_gz_index(eng, f, w_off)
    eng.set_option("one_stored_units", 1)
    try:
        check_gz_index(eng, f, w)
        out, r = eng.gzfile_read(f)
        assert (r.rc, r.status, r.out_len, r.n_members, r.n_units) == (0, 0, len(plain), 3, w.n_units)
        assert out[:r.out_len].tobytes() == plain
        six = eng.gzfile_seek_index(f, SPAN)
        assert (six.rc, six.status, six.n_units, six.n_members) == (0, 0, w.n_units, 3) and int(six.index[GZ_RULE_AT]) == 1
        # a trailer mismatch in the level-0 member is that member's, as with the option off
        broken = f.copy()
        at = w.member_off[2] - 6
        broken[at] ^= 0x10
        words = []
        for value in (1, 0):
            eng.set_option("one_stored_units", value)
            out, r = eng.gzfile_read(broken)
            words.append((r.rc, r.status, r.out_len, r.bad_member, r.err_off, r.stream_err_off, out[:r.out_len].tobytes()))
        assert words[0] == words[1] and words[0][:5] == (-4, -4, len(plain), 1, w.member_off[1])
    finally:
        eng.set_option("one_stored_units", 0)
    off = eng.gzfile_seek_index(f, SPAN)
    assert int(off.index[GZ_RULE_AT]) == 0 and off.n_units == w_off.n_units and six.n_points > off.n_points
    # ranges, on a context whose option is 0: inside the level-0 member, across the boundary between the level-0 member
    # and the random one (stored data on both sides), one byte, nothing, everything
    m1, m2 = w.out_off[w.member_unit[1]], w.out_off[w.member_unit[2]]
    T = len(plain)
    begin = [m1 + 20000, m2 - 5000, m2 + 33333, m1 + 9, 0, T - 70000 + 16000]
    end = [m1 + 20700, m2 + 5000, m2 + 33334, m1 + 9, T, T]
    want = b"".join(plain[a:b] for a, b in zip(begin, end))
    for ix in (six, off):
        out, r = eng.gzfile_ranges(f, ix, begin, end)
        assert r.rc == 0 and (r.range_status == 0).all() and out[:int(r.out_off[-1])].tobytes() == want
    bad = six.index.copy()
    bad[GZ_RULE_AT] = 2
    with pytest.raises(flate.FlateError) as e:
        eng.gzfile_ranges(f, (bad, six.windows), begin, end)
    assert e.value.code == -1
