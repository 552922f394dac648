"""The route of a round of flate_hip_inflate_one (inflate_route_units, moonbit-flate_amd/csrc/inflate_route.h) on the
CPU, as a stand-alone program under AddressSanitizer and UBSan: whatever the options say about the sub-block decoder,
a round of units -- spliced pieces with dictionaries -- runs on the lane-per-stream decoder, with the lanes, row and
equal launches of any spliced call, and the launches cover every unit."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "inflate_route_units_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "inflate_route.h")]
EXE = os.path.join(HERE, "host_model", "inflate_route_units_model")

SIMT = 1
CUS = 256
NS = [1, 7, 16, 17, 4096, 20479, 20480, 36863, 36864, 45056, 196608, 1 << 20]


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, SRC, "-o", EXE])
    return EXE


def ceil_div(a, b):
    return (a + b - 1) // b


@pytest.mark.parametrize("spec", [0, 1, 2])
@pytest.mark.parametrize("lanes", [0, 16, 32, 64])
def test_units_always_take_the_lane_per_stream_decoder(exe, spec, lanes):
    out = subprocess.run([exe, str(spec), str(lanes), str(CUS)] + [str(n) for n in NS], check=True, capture_output=True,
                         text=True).stdout.split("\n")
    rows = [tuple(int(x) for x in line.split()) for line in out if line]
    assert [r[0] for r in rows] == NS
    for n, decoder, shape, got_lanes, row, per, launches in rows:
        want_lanes = lanes or (64 if n >= 144 * CUS else 32 if n >= 80 * CUS else 16)
        sblocks = ceil_div(n, want_lanes)
        want_per = ceil_div(sblocks, ceil_div(sblocks, 8 * CUS))
        assert (decoder, shape, got_lanes) == (SIMT, 0, want_lanes), n
        assert row == (8 if want_lanes == 64 else 0), n  # (the option's default row)
        assert (per, launches) == (want_per, ceil_div(sblocks, want_per)), n
        assert per * launches * want_lanes >= n
