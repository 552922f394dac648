"""The option "gzfile_serial_max" and flate_hip_gzfile_last_route without a GPU: the library exports the entry point,
_lib.py lists it with the header's argument count, the engine and the C++ mirror have the method, and the values the
option accepts and the arguments the call refuses are the checks of api_checks.h -- the functions the entry points run
in front of any HIP call, compiled here into the stand-alone program of tests/test_gzfile_serial_rule_model.py.  (With
a ctx, i.e. on a GPU, tests/test_gpu_gzfile_serial.py makes the same refusals through the library.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_gzfile_serial_rule_model import build
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "flate_hip_gzfile_last_route"
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    flate.build()
    from importlib import import_module
    return import_module("moonbit-flate_amd._lib").load()


def test_the_library_exports_what_the_header_declares(lib):
    L = __import__("importlib").import_module("moonbit-flate_amd._lib")
    hdr = open(os.path.join(ROOT, "include", "flate_hip.h")).read()
    assert hasattr(lib, NAME) and NAME in L.EXPORTS and NAME in L.SIGNATURES
    decl = re.search(r"\bint %s\(([^;]*)\);" % NAME, hdr)
    assert decl and len(decl.group(1).split(",")) == len(L.SIGNATURES[NAME][1]) == 4
    assert L.SIGNATURES[NAME][0] is C.c_int
    assert '"gzfile_serial_max"' in hdr and "gzfile_serial_rule.h" in hdr
    host = open(os.path.join(ROOT, "moonbit-flate_amd", "host", "flate_host.hpp")).read()
    assert "gzfile_last_route" in host and NAME + "(" in host
    assert callable(flate.FlateEngine.gzfile_last_route)


def test_null_pointers_are_refused(lib):
    a, b, w = C.c_uint32(7), C.c_uint32(7), C.c_uint64(7)
    assert lib.flate_hip_gzfile_last_route(None, C.byref(a), C.byref(b), C.byref(w)) == INVALID
    assert (a.value, b.value, w.value) == (7, 7, 7)
    assert lib.flate_hip_set_option(None, b"gzfile_serial_max", 1) == INVALID


def test_the_checks_of_the_option_and_of_the_call():
    out = subprocess.run([build(), "checks"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [ln.split() for ln in out.stdout.splitlines()]
    option = {int(r[1]): int(r[2]) for r in rows if r[0] == "option"}
    assert option == {0: 1, 1: 1, 19: 1, 1 << 20: 1, (1 << 28) - 1: 1, 1 << 28: 0, -1: 0, 1 << 40: 0}
    route = {r[1]: int(r[2]) for r in rows if r[0] == "route"}
    assert route == {"ok": 0, "no_ctx": INVALID, "no_serial_members": INVALID, "no_unit_members": INVALID,
                     "no_find_from": INVALID}
    assert ["limit", str((1 << 28) - 1)] in rows
