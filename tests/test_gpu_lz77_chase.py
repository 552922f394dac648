"""The two-event chase of the dense batch (lz77_stream, moonbit-flate_amd/csrc/lz77_kernels.hip; the rule:
lz77_chase_rule.h) on the GPU: bytes equal to the oracle's, without tolerance, on the streams of
tests/lz77_chase_inputs.py -- runs of back-to-back short matches (pairs), repeats of 16 bytes or more and same-slot
lanes behind a short match (a general event as second hop), single events, matches that end the window;
tests/test_lz77_chase_inputs.py shows on the CPU that they reach those paths.  Through every build of the batch: one
block per stream, the smallest persistent launch (1300 streams: LDS-table blocks beside guests) with the default guest
blocks and with none, two-window streams with and without window units, FLATE_HIP_COMPAT_GO, the HOOKS build, and a
dictionary call."""
import numpy as np
import pytest

import lz77_chase_inputs as I
from deflate_dict_ref import deflate_dict
from util import flate

pytestmark = pytest.mark.gpu

N_SMALL = 1300  # guest_min_streams is 1280: the persistent launch starts there
PERSISTENT = (("guest_min_streams", 1), ("guest_blocks", 8), ("resident_blocks", 8))


class Ref:
    pass


@pytest.fixture(scope="module")
def small(oracle):
    flate.build()
    r = Ref()
    r.streams = I.small_streams(N_SMALL)
    r.data, r.off = I.batch(r.streams)
    r.want = [oracle.deflate(np.frombuffer(s, np.uint8)) for s in r.streams]
    return r


@pytest.fixture(scope="module")
def wide(oracle):
    flate.build()
    r = Ref()
    r.streams = I.two_window_streams(4) + I.small_streams(8, seed=3)
    r.data, r.off = I.batch(r.streams)
    r.want = [oracle.deflate(np.frombuffer(s, np.uint8)) for s in r.streams]
    return r


def _run(ref, opts=(), want=None, **kw):
    e = flate.FlateEngine(0)
    try:
        for k, v in opts:
            e.set_option(k, v)
        out, out_off = e.deflate_batch(ref.data[:int(ref.off[-1])], ref.off, **kw)
        share = e.last_resident_share()
    finally:
        e.close()
    out = np.asarray(out)
    want = want or ref.want
    bad = [i for i in range(len(ref.streams)) if bytes(out[int(out_off[i]):int(out_off[i + 1])]) != want[i]]
    assert not bad, (opts, kw, len(bad), [(i, len(ref.streams[i])) for i in bad[:10]])
    return share


def test_one_block_per_stream(small):
    _run(small, (("guest_blocks", 0),))


def test_smallest_persistent_launch_default_guest_blocks(small):
    res, queued = _run(small)
    assert queued == N_SMALL and 0 < res < N_SMALL, (res, queued)  # both kinds of block took streams


def test_persistent_launch_few_blocks(small):
    res, queued = _run(small, PERSISTENT)
    assert queued == N_SMALL and 0 < res < N_SMALL, (res, queued)


def test_hooks_build(small):
    _run(small, (("debug_stall_batch", 0x7fffffff),))  # a batch no chunk reaches: the HOOKS instantiations, hook idle


def test_compat_go(small, oracle):
    some = Ref()
    some.streams = small.streams[:190]
    some.data, some.off = I.batch(some.streams)
    want = [oracle.deflate(np.frombuffer(s, np.uint8), compat=oracle.COMPAT_GO) for s in some.streams]
    _run(some, (("guest_blocks", 0),), want=want, compat_go=True)
    _run(some, PERSISTENT, want=want, compat_go=True)


@pytest.mark.parametrize("units", [0, 1])
def test_two_window_streams(wide, units):
    _run(wide, PERSISTENT + (("window_units", units),))


def test_two_window_streams_one_block_per_stream(wide):
    _run(wide, (("guest_blocks", 0),))


def test_dictionary_call(small):
    # the dictionary is one of the streams: its words are the payloads' words, so the first batches match into it
    zdict = small.streams[18]  # 4096 bytes, the vocabulary of streams 16 .. 23
    some = Ref()
    some.streams = small.streams[16:24] + I.two_window_streams(1)
    some.data, some.off = I.batch(some.streams)
    want = [deflate_dict(s, zdict, 0) for s in some.streams]
    for opts in ((("guest_blocks", 0),), PERSISTENT):
        _run(some, opts, want=want, zdicts=[zdict], dict_of=[0] * len(some.streams))
