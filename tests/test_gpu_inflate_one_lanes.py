"""flate_hip_inflate_one's DECODE is the lane-per-stream dictionary decoder over spliced pieces with dictionaries; by
default a round of a few thousand units takes its 16-lane build.  Here the other builds -- 32 lanes, 64 lanes storing
straight to memory and through an output row of 8 and 16 dwords -- decode the file of 230 short units in one round and
in rounds of 7 (every round's last piece ends at the next unit's bit, not at BFINAL), and the streams that fail inside
that file or on a distance in front of the stream: zlib's bytes, the serial decoder's verdict, and nothing written
behind out_len."""
import numpy as np
import pytest

import one_ref as ref
from test_gpu_inflate_one_read import check_good, read
from util import flate

pytestmark = pytest.mark.gpu

BUILDS = [(32, 0), (64, 0), (64, 8), (64, 16)]


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def many(oracle):
    what, raw, plain = ref.good_streams(oracle)[ref.MANY_UNITS]
    return what, raw, plain, ref.Walk(raw)


@pytest.fixture(scope="module")
def failing(eng, many):
    """[(what, raw, cap, status, err_off, bytes)] of the serial decoder (flate_hip_inflate_batch, default options)."""
    _, raw, _, w = many
    mid = w.n_units // 2
    cases = [("cut inside %s unit" % name, raw[:(w.unit_bit[u] + w.unit_bit[u + 1]) // 16])
             for name, u in (("the first", 0), ("a middle", mid), ("the last", w.n_units - 1))]
    for name, bit in (("header", w.unit_bit[mid] + 20), ("body", (w.unit_bit[mid] + w.unit_bit[mid + 1]) // 2)):
        flipped = bytearray(raw)
        flipped[bit >> 3] ^= 1 << (bit & 7)
        cases.append(("one flipped bit in a middle unit's %s" % name, bytes(flipped)))
    legal, _, illegal = ref.history_pair()
    cases += [("a distance to the stream's first byte", legal), ("a distance one byte in front of the stream", illegal)]
    off = np.zeros(len(cases) + 1, np.uint64)
    np.cumsum(np.array([len(r) for _, r in cases], dtype=np.uint64), out=off[1:])
    data = np.frombuffer(b"".join(r for _, r in cases) + b"\0" * 8, np.uint8).copy()
    caps = [ref.Walk(r).out_len + 600 for _, r in cases]
    out, ooff, olen, status, err = eng.inflate_batch(data, off, caps, check=False)
    assert {int(s) for s in status} >= {0, ref.CORRUPT, ref.UNEXPECTED_EOF}
    return [(what, r, caps[k], int(status[k]), int(err[k]), bytes(out[int(ooff[k]):int(ooff[k]) + int(olen[k])]))
            for k, (what, r) in enumerate(cases)]


@pytest.mark.parametrize("lanes,row", BUILDS)
def test_every_build_of_the_lane_decoder_decodes_the_units(eng, many, failing, lanes, row):
    what, raw, plain, w = many
    assert w.n_units >= 100
    try:
        eng.set_option("inflate_lanes", lanes)
        eng.set_option("inflate_row_dwords", row)
        for units in (4096, 7):
            eng.set_option("one_round_units", units)
            check_good(eng, raw, plain, w, what, ref.GZIP, device=True, shift=1, out_shift=1)
            for name, r, cap, status, err, want in failing:
                rc, got, ol, st, eo, _, _, _ = read(eng, r, ref.RAW, cap, device=True, shift=3)
                assert (rc, st, eo, ol) == (status, status, err, len(want)), (name, units, rc, st, eo, ol)
                assert got == want, (name, units)
    finally:
        eng.set_option("one_round_units", 4096)
        eng.set_option("inflate_lanes", 0)
        eng.set_option("inflate_row_dwords", 8)


def test_wrapper_takes_the_size_from_isize_and_falls_back(eng, many):
    """FlateEngine.inflate_one(out=None) sizes a gzip member's output from its ISIZE: one call.  An ISIZE that is too
    small (or absurd) costs the query: the bytes still arrive, and the verdict is the trailer's."""
    import struct

    _, raw, plain, w = many
    f = ref.wrap(raw, plain, ref.GZIP)
    out, r = eng.inflate_one(np.frombuffer(f, np.uint8), "gzip")
    assert r[:5] == (0, len(plain), 0, -1, w.n_units) and out[:r.out_len].tobytes() == plain
    for isize in (5, 0, 0xffffffff):
        g = f[:-4] + struct.pack("<I", isize)
        out, r = eng.inflate_one(np.frombuffer(g, np.uint8), "gzip")
        assert r[:4] == (ref.CORRUPT, len(plain), ref.CORRUPT, len(g)), (isize, r)
        assert out[:r.out_len].tobytes() == plain, isize
