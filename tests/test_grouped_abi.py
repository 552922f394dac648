"""The grouped call in the product library, as far as a machine without a GPU can see it: the symbol exists with its
argument count, is listed in EXPORTS and declared in the header, and a missing ctx is refused before anything is
written.  (What it computes: tests/test_gpu_grouped.py.)"""
import os
import re
from importlib import import_module

import numpy as np
import pytest

from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "flate_hip_deflate_fast_grouped_framed"


@pytest.fixture(scope="module")
def lib():
    flate.build()
    return import_module("moonbit-flate_amd._lib").load()


def test_the_symbol_is_exported_listed_and_declared_with_twelve_arguments(lib):
    _lib = import_module("moonbit-flate_amd._lib")
    assert hasattr(lib, NAME) and NAME in _lib.EXPORTS
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert len(argtypes) == 12
    hdr = open(os.path.join(ROOT, "include", "flate_hip.h")).read()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, "not declared"
    assert len(m.group(1).split(",")) == 12
    assert hasattr(flate.FlateEngine, "deflate_grouped_framed")


def test_the_route_query_exists_and_refuses_a_missing_ctx(lib):
    import ctypes as C
    _lib = import_module("moonbit-flate_amd._lib")
    name = "flate_hip_zip_write_last_route"
    assert hasattr(lib, name) and name in _lib.EXPORTS and len(_lib.SIGNATURES[name][1]) == 3
    a, b = C.c_uint32(7), C.c_uint32(7)
    assert lib.flate_hip_zip_write_last_route(None, C.byref(a), C.byref(b)) == -1
    assert (a.value, b.value) == (7, 7)
    assert hasattr(flate.FlateEngine, "zip_write_last_route")


def test_a_missing_ctx_is_refused_and_nothing_is_written(lib):
    data = np.arange(64, dtype=np.uint8)
    in_off = np.array([0, 32, 64], np.uint64)
    group_off = np.array([0, 2], np.uint32)
    out = np.full(4096, 0xA5, np.uint8)
    out_off = np.full(2, 7, np.uint64)
    bit_off = np.full(3, 7, np.uint64)
    rc = lib.flate_hip_deflate_fast_grouped_framed(None, data.ctypes.data, in_off.ctypes.data, 2, group_off.ctypes.data,
                                                   1, 1, out.ctypes.data, out.size, out_off.ctypes.data,
                                                   bit_off.ctypes.data, 0)
    assert rc == -1
    assert (out == 0xA5).all() and (out_off == 7).all() and (bit_off == 7).all()
