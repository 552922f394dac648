"""The match finder's batch loop at the stream lengths where its per-batch bookkeeping changes state, through both
builds of the kernels (lz77_stream<.., HOOKS>, moonbit-flate_amd/csrc/lz77_kernels.hip).

The product build carries no test hook; the progress guard is each batch's own last step; the look-ahead load is issued
when the batch base enters a new 256-byte block of the window.  So the lengths sit around one and two dense batches
(128 .. 257), around the first look-ahead blocks and the end-of-window clamp of the look-ahead address (767 .. 1025), and
around the window (65535 .. 65537, 131070 = two windows); the inputs are the four that drive the parser differently:
text (about six matches per batch), zeros (one 258-byte match per batch), a ramp (long matches at a fixed distance) and
random bytes (dense batches that turn sparse).  Tokens and bytes are the oracle's, without tolerance, in every launch
shape of test_gpu_parity.test_batch_without_progress_is_an_error_not_a_hang -- one block per stream, persistent LDS-table
blocks beside guests, guests only, window units -- once with the hooks idle (the product build) and once with
debug_stall_batch above any batch count, which launches the HOOKS build and must change nothing.  A stall that does
happen -- on the first batch, which on random bytes is a batch that has turned sparse -- ends FLATE_HIP_E_INTERNAL: the
no-progress path is an error return, never a hang and never replayed records."""
import numpy as np
import pytest

from util import flate, make_streams, oracle_tokens_per_chunk

pytestmark = pytest.mark.gpu

LENGTHS = [128, 129, 191, 192, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025, 65535, 65536, 65537, 131070]
KINDS = ["text", "zero", "ramp", "rand"]
SPECS = [(k, n) for k in KINDS for n in LENGTHS]
NEVER = 0x7fffffff  # a dense batch no chunk reaches: the HOOKS build runs, the hook stays idle
PERSISTENT = (("guest_min_streams", 1), ("guest_blocks", 8), ("resident_blocks", 8))
# (name, options, dummy streams in front): the guests-only shape hands queue entry 0 of the single-window and of the
# multi-window queue -- the two dummies -- to the LDS-table blocks and everything else to the guests
SHAPES = [
    ("one_block_per_stream", (), 0),
    ("lds_blocks_and_guests", PERSISTENT + (("window_units", 0),), 0),
    ("guests_only", (("guest_min_streams", 1), ("guest_blocks", 16), ("resident_blocks", 4), ("window_units", 0),
                     ("profile_split_streams", 1)), 2),
    ("window_units", PERSISTENT + (("window_units", 1),), 0),
]


class Ref:
    pass


@pytest.fixture(scope="module")
def ref(oracle):
    """The streams (two dummies in front: 200 random bytes, and two windows of them) and the oracle's answer, once."""
    flate.build()
    r = Ref()
    r.specs = [("rand", 200), ("rand", 65535 + 200)] + SPECS
    r.data, r.off = make_streams(r.specs, seed=11)
    r.streams = [r.data[int(r.off[i]):int(r.off[i + 1])] for i in range(len(r.specs))]
    r.want = [oracle.deflate(s) for s in r.streams]
    r.tokens = [oracle_tokens_per_chunk(oracle, s) for s in r.streams]
    return r


def _batch(ref, dummies):
    first = 2 - dummies
    base = int(ref.off[first])
    return first, ref.data[base:int(ref.off[-1])], ref.off[first:] - np.uint64(base)


def _check(e, ref, dummies, what):
    first, data, off = _batch(ref, dummies)
    chunks = e.lz77_matches(data, off)
    out, out_off = e.deflate_batch(data, off)
    k = 0
    for i in range(first, len(ref.specs)):
        sb = ref.streams[i]
        for (start, cn), w in zip(flate.lz_chunks(sb.size), ref.tokens[i]):
            pos, tok = chunks[k]
            got = flate.tokens_from_matches(sb[start:start + cn], pos, tok)
            k += 1
            assert got.size == w.size and not (got != w).any(), (what, ref.specs[i], start, got.size, w.size)
        got = bytes(out[int(out_off[i - first]):int(out_off[i - first + 1])])
        assert got == ref.want[i], (what, ref.specs[i], len(got), len(ref.want[i]))
    assert k == len(chunks)


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_both_builds_give_the_oracles_tokens_and_bytes(ref, shape):
    name, opts, dummies = shape
    e = flate.FlateEngine(0)
    try:
        for k, v in opts:
            e.set_option(k, v)
        _check(e, ref, dummies, name + ", product build")
        if dummies:
            first, data, off = _batch(ref, dummies)
            e.lz77_matches(data, off)
            assert e.last_resident_share()[0] == dummies, e.last_resident_share()
        e.set_option("debug_stall_batch", NEVER)
        _check(e, ref, dummies, name + ", HOOKS build")
        e.set_option("debug_stall_batch", 0)
        _check(e, ref, dummies, name + ", product build again")
    finally:
        e.close()


@pytest.mark.parametrize("kind", ["text", "rand"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_a_stalled_first_batch_is_an_error(ref, shape, kind):
    # debug_stall_batch = 1: the first dense batch of every chunk forgets what it did.  On text it had found matches
    # (records and lengths must not be committed twice); on random bytes it had turned sparse.  Either way the guard
    # ends the chunk, the call comes back FLATE_HIP_E_INTERNAL naming the guard, and the engine works afterwards.
    name, opts, dummies = shape
    specs = [(kind, n) for n in (257, 1025, 65536, 131070)] * 3
    data, off = make_streams(specs, seed=12)
    e = flate.FlateEngine(0)
    try:
        for k, v in opts:
            e.set_option(k, v)
        e.set_option("debug_stall_batch", 1)
        with pytest.raises(flate.FlateError) as ei:
            e.deflate_batch(data, off)
        assert ei.value.code == -8 and "no progress" in str(ei.value), (name, kind)
        e.set_option("debug_stall_batch", 0)
        _check(e, ref, dummies, name + ", after the error")
    finally:
        e.close()
