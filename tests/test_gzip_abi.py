"""CPU-side checks of the plain-gzip calls (flate_hip_gzip_index / flate_hip_gzip_read): the symbols are there and
listed, and each call refuses a missing ctx before it touches a device, whatever else it is given.  (The refusals that
need a ctx are api_checks.h's, driven on the CPU by tests/test_gzip_rule_model.py; GPU compute: tests/test_gpu_gzip.py.)"""
import ctypes as C
import importlib

import pytest

import gzip_ref as ref
from util import flate

CALLS = ["flate_hip_gzip_index", "flate_hip_gzip_read"]


@pytest.fixture(scope="module")
def lib():
    flate.build()
    return importlib.import_module("moonbit-flate_amd._lib").load()


def test_library_exports_the_gzip_calls(lib):
    for name in CALLS:
        assert hasattr(lib, name), name


def test_gzip_calls_are_listed_in_exports():
    exports = importlib.import_module("moonbit-flate_amd._lib").EXPORTS
    for name in CALLS:
        assert name in exports, name


def test_each_call_refuses_a_missing_ctx_before_it_touches_a_device(lib):
    f = ref.member(b"hello")
    buf = (C.c_uint8 * len(f))(*f)
    out = (C.c_uint8 * 256)()
    off, off2 = (C.c_uint64 * 4)(7, 7, 7, 7), (C.c_uint64 * 4)(7, 7, 7, 7)
    n64, n32, nc, bad, eo = C.c_uint64(9), C.c_uint32(9), C.c_uint32(9), C.c_uint32(9), C.c_int64(9)
    for flags in (0, 1, 2, 8, 0xffffffff):
        assert lib.flate_hip_gzip_index(None, buf, len(f), 4, off, off2, C.byref(n32), C.byref(n64), C.byref(nc),
                                        C.byref(eo), flags) == -1
        assert lib.flate_hip_gzip_index(None, buf, len(f), 0, None, None, C.byref(n32), C.byref(n64), None, None,
                                        flags) == -1
        assert lib.flate_hip_gzip_read(None, buf, len(f), out, 256, C.byref(n64), C.byref(n32), C.byref(bad),
                                       C.byref(eo), flags) == -1
    # ... and nothing was written
    assert list(off) == [7] * 4 and list(off2) == [7] * 4 and not any(out)
    assert (n64.value, n32.value, nc.value, bad.value, eo.value) == (9, 9, 9, 9, 9)


def test_the_option_is_refused_without_a_ctx(lib):
    assert lib.flate_hip_set_option(None, b"gzip_member_max", 4096) == -1
