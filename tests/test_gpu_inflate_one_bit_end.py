"""InfParams::bit_end, the per-piece end the lane-per-stream decoder takes for flate_hip_inflate_one_ranges: NULL for
every caller that existed before it, so flate_hip_inflate_spliced and flate_hip_inflate_one deliver on the spliced
corpus what they delivered -- the input's own bytes (the encoder's input; zlib agrees) and status 0, with every lane
count -- and the same units, read through a seek index without points (every piece with its own end, the last one open),
are the same bytes.  The existing suite covers the first two; this file names them beside the new path."""
import zlib

import numpy as np
import pytest

import one_ref as ref
import seek_ref as sk
from util import flate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def spliced(eng):
    """(data, off, the spliced stream's bytes, bit_off): 96 streams of odd sizes as ONE DEFLATE stream."""
    sizes = [1 + (977 * k) % 5003 for k in range(96)]
    data = flate.synth("text", 1, sum(sizes))
    off = np.zeros(len(sizes) + 1, np.uint64)
    np.cumsum(np.array(sizes, np.uint64), out=off[1:])
    one, nbytes, bit_off = eng.deflate_spliced(data, off)
    stream = bytes(one[:nbytes])
    assert zlib.decompress(stream, -15) == data.tobytes()
    return data, off, stream, bit_off


def test_spliced_pieces_without_bit_end_decode_as_before(eng, spliced):
    data, off, stream, bit_off = spliced
    sizes = [int(b - a) for a, b in zip(off, off[1:])]
    try:
        eng.set_option("inflate_simt_min_streams", 0)  # the lane-per-stream decoder, whatever the batch's size
        eng.set_option("inflate_spec", 0)
        for lanes in (16, 32, 64):
            eng.set_option("inflate_lanes", lanes)
            back, ooff, olen, status, err = eng.inflate_spliced(np.frombuffer(stream, np.uint8), len(stream), bit_off, sizes)
            assert (status == 0).all() and [int(x) for x in olen] == sizes and (err == -1).all(), lanes
            assert bytes(back[:len(data)]) == data.tobytes(), lanes
    finally:
        eng.set_option("inflate_lanes", 0)
        eng.set_option("inflate_spec", 1)
        eng.set_option("inflate_simt_min_streams", 2049)


def test_inflate_one_rounds_without_bit_end_decode_as_before(eng, spliced):
    data, off, stream, bit_off = spliced
    w = ref.Walk(stream)
    assert w.status == 0 and w.n_units >= 96
    try:
        for units in (4096, 7):  # 7: the rounds' last pieces are closed by InfParams::closed
            eng.set_option("one_round_units", units)
            out, r = eng.inflate_one(np.frombuffer(stream, np.uint8), "raw")
            assert (r.rc, r.out_len, r.status, r.err_off, r.n_units) == (0, len(data), 0, -1, w.n_units), units
            assert out[:r.out_len].tobytes() == data.tobytes(), units
    finally:
        eng.set_option("one_round_units", 4096)


def test_the_same_units_with_bit_end_are_the_same_bytes(eng, spliced):
    data, off, stream, bit_off = spliced
    w = ref.Walk(stream)
    s = eng.inflate_one_seek_index(np.frombuffer(stream, np.uint8), "raw", flate.SEEK_SPAN_NONE)
    assert (s.rc, s.n_units, s.n_points) == (0, w.n_units, 1) and [int(x) for x in s.index] == \
        sk.index_words(w, data.tobytes(), len(stream), ref.RAW, sk.SPAN_NONE)
    mid = int(off[40]) + 3
    out, r = eng.inflate_one_ranges(np.frombuffer(stream, np.uint8), s, [0, mid], [len(data), mid + 9000], wrap="raw")
    assert (r.rc, list(r.range_status), r.bad_unit) == (0, [0, 0], sk.NO_UNIT)
    assert out[:len(data)].tobytes() == data.tobytes() and out[len(data):len(data) + 9000].tobytes() == data.tobytes()[mid:mid + 9000]
