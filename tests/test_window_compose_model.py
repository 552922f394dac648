"""The COMPOSE operator of flate_hip_inflate_one on the CPU: moonbit-flate_amd/csrc/window_compose.h -- what the kernels
compile -- built with g++ into a stand-alone program under AddressSanitizer and UBSan.  Chains of 1, 2, 3, 64 and 65
random tail functions (units shorter and longer than 32 KiB, copies that reach into the window in front), of identities
and of all-literal functions are scanned as the kernels scan them and held against a brute-force resolution window by
window; the operator is associative."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "window_compose_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "window_compose.h")]
EXE = os.path.join(HERE, "host_model", "window_compose_model")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, SRC, "-o", EXE])
    return EXE


def test_scan_equals_brute_force(exe):
    out = subprocess.run([exe, "7"], check=True, capture_output=True, text=True).stdout.split()
    got = dict(zip(out[::2], out[1::2]))
    want = ["%s_%d" % (k, n) for k in ("random", "identity", "all_literal") for n in (1, 2, 3, 64, 65)] + ["associative"]
    assert got == {name: "ok" for name in want}
