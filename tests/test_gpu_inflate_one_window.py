"""flate_hip_inflate_one and flate_hip_inflate_one_index over tests/one_window_corpus.py: copies that reach the far end
of the 32 KiB window across unit boundaries, empty units, units of exactly one window, stored blocks inside units,
overlapping copies whose source lies in the unit in front, and a byte that passes through 70 units.  Nothing here is
the code under test's own: the bytes of a good stream are zlib's (test_one_window_corpus.py holds the corpus against
it), the units are the Python walker's (tests/one_ref.py), and status, err_off, out_len and the bytes in front of the
error of a failing twin are the serial batch decoder's (flate_hip_inflate_batch on the same bytes as one stream) and
the Writer's output model.  Every comparison is exact."""
import numpy as np
import pytest

import one_ref as ref
import one_window_corpus as corpus
from test_gpu_inflate_one import check_index
from test_gpu_inflate_one_lanes import BUILDS
from test_gpu_inflate_one_read import GUARD, check_good, read
from util import flate

pytestmark = pytest.mark.gpu

KINDS = (ref.RAW, ref.ZLIB, ref.GZIP)
ROUNDS = (1, 2, 3, 5, 64, 4096)


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def good():
    """[(what, raw stream, plain, Walk)]: computed once, shared, never changed."""
    return [(what, raw, plain, ref.Walk(raw)) for what, raw, plain, _ in corpus.good_streams()]


@pytest.fixture(scope="module")
def twins(eng):
    """[(what, raw, kind, cap, status, err_off, bytes)]: the serial decoder's verdict on every failing twin
    (flate_hip_inflate_batch, default options, room for everything it produces), its bytes held against the Writer's."""
    cases = corpus.failing_twins()
    walks = [ref.Walk(raw) for _, raw, _, _ in cases]
    off = np.zeros(len(cases) + 1, np.uint64)
    np.cumsum(np.array([len(c[1]) for c in cases], dtype=np.uint64), out=off[1:])
    data = np.frombuffer(b"".join(c[1] for c in cases) + b"\0" * 8, np.uint8).copy()
    caps = [w.out_len + 600 for w in walks]
    out, ooff, olen, status, err = eng.inflate_batch(data, off, caps, check=False)
    res = []
    for k, ((what, raw, front, kind), w) in enumerate(zip(cases, walks)):
        got = bytes(out[int(ooff[k]):int(ooff[k]) + int(olen[k])])
        if kind == "far":  # the one verdict that depends on history: corrupt at the copy, the bytes in front delivered
            assert (int(status[k]), got) == (ref.CORRUPT, front) and int(err[k]) > 0, (what, int(status[k]), int(olen[k]))
        else:
            assert (int(status[k]), int(err[k]), int(olen[k])) == (ref.UNEXPECTED_EOF, -1, w.out_len), what
            assert got == front[:w.out_len], what
        res.append((what, raw, kind, caps[k], int(status[k]), int(err[k]), got))
    return res


def check_twin(eng, twin, **kw):
    what, raw, kind, cap, status, err, want = twin
    rc, got, ol, st, eo, _, _, _ = read(eng, raw, ref.RAW, cap, **kw)
    assert (rc, st, eo, ol) == (status, status, err, len(want)), (what, kw, rc, st, eo, ol)
    assert got == want, (what, kw)


# ---- good streams ----

def test_every_stream_in_every_container_with_host_pointers(eng, good):
    for what, raw, plain, w in good:
        assert w.status == 0 and w.out_bytes == len(plain), what
        counts = {check_index(eng, raw, plain, w, what, kind) for kind in KINDS}
        assert len(counts) == 1, (what, counts)
        for kind in KINDS:
            check_good(eng, raw, plain, w, what, kind)


def test_device_pointers_at_shifted_addresses_into_a_guarded_buffer(eng, good):
    for what, raw, plain, w in good:
        check_index(eng, raw, plain, w, what, ref.GZIP, device=True, shift=1)
        check_good(eng, raw, plain, w, what, ref.GZIP, device=True, shift=1, out_shift=3)


@pytest.mark.parametrize("units", ROUNDS)
def test_rounds_carry_the_window(eng, good, units):
    """At "one_round_units" = 1 every window comes from the seed alone and the long pass-through takes 72 rounds; at
    2, 3 and 5 a window crosses rounds and scan steps both; at 64 the pass-through crosses one round (steps up to 32) and
    at 4096 its 72 units are one round, which takes the scan to step 64."""
    try:
        eng.set_option("one_round_units", units)
        for what, raw, plain, w in good:
            check_good(eng, raw, plain, w, what, ref.GZIP, device=True, shift=1)
    finally:
        eng.set_option("one_round_units", 4096)


@pytest.mark.parametrize("lanes,row", BUILDS)
def test_every_build_of_the_lane_decoder(eng, good, twins, lanes, row):
    try:
        eng.set_option("inflate_lanes", lanes)
        eng.set_option("inflate_row_dwords", row)
        for units in (3, 4096):
            eng.set_option("one_round_units", units)
            for what, raw, plain, w in good:
                check_good(eng, raw, plain, w, what, ref.GZIP, device=True, shift=1, out_shift=1)
            for twin in twins:
                check_twin(eng, twin, device=True, shift=3)
    finally:
        eng.set_option("one_round_units", 4096)
        eng.set_option("inflate_lanes", 0)
        eng.set_option("inflate_row_dwords", 8)


def test_a_stream_of_empty_units_writes_nothing(eng, good):
    what, raw, plain, w = next(g for g in good if g[0].startswith("three empty units"))
    assert plain == b"" and w.n_units == 3
    for kind in KINDS:
        f = ref.wrap(raw, plain, kind)
        for kw in ({}, {"device": True, "out_shift": 3}, {"query": True}, {"query": True, "device": True}):
            rc, got, ol, st, eo, nu, nc, body = read(eng, f, kind, 0, **kw)  # (read holds the guard bytes around out)
            assert (rc, ol, st, eo, nu) == (0, 0, 0, -1, 3) and got == b"", (kind, kw, rc, ol, st, eo, nu)
        rc, got, ol, st, eo, nu, nc, body = read(eng, f, kind, 32, device=True, shift=1)  # room that must stay untouched
        assert (rc, ol, st, eo, nu) == (0, 0, 0, -1, 3) and (body == GUARD).all(), kind


# ---- failing twins ----

def test_failing_twins_have_the_serial_decoders_verdict_and_bytes(eng, twins):
    assert {t[2] for t in twins} == {"far", "cut"}
    for k, twin in enumerate(twins):
        check_twin(eng, twin)
        check_twin(eng, twin, device=True, shift=1, out_shift=k % 4)
        what, raw = twin[:2]
        check_index(eng, raw, b"", ref.Walk(raw), what)  # history-free: the walker's verdict, a far copy included


def test_failing_twins_at_every_round_size(eng, twins):
    try:
        for units in ROUNDS:
            eng.set_option("one_round_units", units)
            for twin in twins:
                check_twin(eng, twin, device=True, shift=1)
    finally:
        eng.set_option("one_round_units", 4096)
