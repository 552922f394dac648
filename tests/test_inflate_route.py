"""Decoder routing (moonbit-flate_amd/csrc/inflate_route.h) on the CPU: which of the three decoders a decode call
runs, in which build, with how many lanes and rows, and in how many equal launches -- at the edges no GPU test can
afford to reach (2^28-byte streams, 2^31-bit pieces, the 45056-stream crossover).  tests/host_model/
inflate_route_model.cpp includes the header the driver includes; `expected` below restates the documented rules."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "inflate_route_model.cpp")
HDR = os.path.join(ROOT, "moonbit-flate_amd", "csrc", "inflate_route.h")
LIB = os.path.join(HERE, "host_model", "libinflate_route_model.so")

WAVE, SIMT, SPEC = 0, 1, 2
CUS = 256
NS = [1, 1024, 1025, 2048, 2049, 20479, 20480, 36863, 36864, 45055, 45056, 196608]
DEFAULTS = dict(lanes=0, row=8, simt_min=2049, spec=1, spec_shape=0, spec_max=45056)  # (flate_hip.h's option defaults)
KEYS = ["lanes", "row", "simt_min", "spec", "spec_shape", "spec_max"]


def ceil_div(a, b):
    return (a + b - 1) // b


def expected(o, cus, n, longest, spliced, size_only):
    """(decoder, shape, lanes, row, blocks per launch, launches)"""
    size_only = size_only and not spliced
    simt = (spliced or n >= o["simt_min"]) and not size_only and (spliced or longest < 2 ** 28)
    spec = (o["spec"] == 2 or (o["spec"] == 1 and (size_only or n < o["spec_max"]))) and \
        longest < (2 ** 31 if spliced else 2 ** 28)
    if spec:
        return (SPEC, o["spec_shape"] or (1 if n <= 4 * cus else 2), 0, 0, n, 1)
    if not simt:
        return (WAVE, 0, 0, 0, n, 1)
    lanes = o["lanes"] or (64 if n >= 144 * cus else 32 if n >= 80 * cus else 16)
    row = o["row"] if lanes == 64 and o["row"] in (8, 16) else 0
    sblocks = ceil_div(n, lanes)
    per = ceil_div(sblocks, ceil_div(sblocks, 8 * cus))
    return (SIMT, 0, lanes, row, per, ceil_div(sblocks, per))


@pytest.fixture(scope="module")
def model():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.dirname(HDR), SRC, "-o", LIB])
    L = C.CDLL(LIB)
    six = C.c_int64 * 6
    L.route_defaults.argtypes = [six]
    L.route_model.argtypes = [six, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.c_int, six]
    L.route_model_index.argtypes = [six, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32, C.c_int, C.c_int, six]
    L.route_defaults.restype = L.route_model.restype = L.route_model_index.restype = None

    def route(n, longest=65536, spliced=False, size_only=False, cus=CUS, **opts):
        o = dict(DEFAULTS, **opts)
        out = six()
        L.route_model(six(*[o[k] for k in KEYS]), cus, n, longest, int(spliced), int(size_only), out)
        got = tuple(out)
        assert got == expected(o, cus, n, longest, spliced, size_only), (n, longest, spliced, size_only, o)
        return got

    route.lib = L
    return route


def test_the_structs_defaults_are_the_documented_option_defaults(model):
    d = (C.c_int64 * 6)()
    model.lib.route_defaults(d)
    assert dict(zip(KEYS, d)) == DEFAULTS


@pytest.mark.parametrize("n", NS)
def test_default_options_at_every_batch_size_edge(model, n):
    dec, shape, lanes, row, per, launches = model(n)
    # below the crossover the sub-block decoder, in its small build up to one wavefront per SIMD; beyond, one lane per
    # stream in the 64-lane form with the 8-dword row
    if n < 45056:
        assert (dec, shape, lanes, row, per, launches) == (SPEC, 1 if n <= 1024 else 2, 0, 0, n, 1)
    else:
        assert (dec, lanes, row) == (SIMT, 64, 8) and per * launches >= ceil_div(n, 64)
    # a size-only pass: the sub-block decoder at any size; switched off, never the lane-per-stream decoder
    assert model(n, size_only=True)[0] == SPEC
    assert model(n, size_only=True, spec=0)[0] == WAVE
    # spliced: size-only does not hold, and without the sub-block decoder every batch size runs lane per stream
    assert model(n, spliced=True, size_only=True) == model(n, spliced=True)
    assert model(n, spliced=True, spec=0)[0] == SIMT


@pytest.mark.parametrize("n", NS)
def test_the_longest_entry_at_the_32_bit_limits_moves_the_whole_batch(model, n):
    for spec in (0, 1, 2):
        for size_only in (False, True):
            below = model(n, longest=2 ** 28 - 1, spec=spec, size_only=size_only)
            at = model(n, longest=2 ** 28, spec=spec, size_only=size_only)
            assert below == model(n, spec=spec, size_only=size_only)
            assert at[0] == WAVE  # 2^28 bytes: neither decoder with 32-bit bit positions
        # a spliced piece: 2^31 bits for the sub-block decoder; the lane-per-stream decoder takes any (checked) piece
        below = model(n, longest=2 ** 31 - 1, spliced=True, spec=spec)
        at = model(n, longest=2 ** 31, spliced=True, spec=spec)
        assert below == model(n, spliced=True, spec=spec)
        assert at[0] == SIMT and at == model(n, spliced=True, spec=0)


def test_one_long_stream_among_small_ones(model):
    n = 4096
    for big, dec in ((2 ** 28 - 1, SPEC), (2 ** 28, WAVE)):
        off = (C.c_uint64 * (n + 1))()
        for i in range(n):
            off[i + 1] = off[i] + (big if i == 7 else 100)
        out = (C.c_int64 * 6)()
        model.lib.route_model_index((C.c_int64 * 6)(*[DEFAULTS[k] for k in KEYS]), CUS, off, n, 0, 0, out)
        assert tuple(out) == expected(DEFAULTS, CUS, n, big, False, False) and out[0] == dec


@pytest.mark.parametrize("n", NS)
def test_forced_shapes_lanes_rows_and_thresholds(model, n):
    for spec, shape in itertools.product((0, 1, 2), (0, 1, 2)):
        got = model(n, spec=spec, spec_shape=shape)
        if got[0] == SPEC and shape:
            assert got[1] == shape
        assert (got[0] == SPEC) == (spec == 2 or (spec == 1 and n < 45056))
    for lanes, row, simt_min in itertools.product((0, 16, 32, 64), (0, 8, 16), (0, 1, 2049)):
        got = model(n, spec=0, lanes=lanes, row=row, simt_min=simt_min)
        assert (got[0] == SIMT) == (n >= simt_min)
        if got[0] == SIMT:
            assert got[2] == (lanes or (64 if n >= 36864 else 32 if n >= 20480 else 16))
            assert got[3] == (row if got[2] == 64 else 0)  # the row is ignored below 64 lanes
            sblocks = ceil_div(n, got[2])
            assert got[4] <= 8 * CUS and got[4] * (got[5] - 1) < sblocks <= got[4] * got[5]


def test_the_documented_split_of_196608_streams(model):
    assert model(196608, spec=0, lanes=64) == (SIMT, 0, 64, 8, 1536, 2)
    assert model(196608) == (SIMT, 0, 64, 8, 1536, 2)  # (and by default: beyond the crossover)
