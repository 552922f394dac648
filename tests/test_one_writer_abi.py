"""flate_hip_one_writer_* without a GPU: the library exports the five calls, _lib.py lists them with the header's
argument counts and types, flate_hip_one_writer_bound is monotone and holds the reference's largest call, and a missing
ctx, handle or result pointer is refused before any device is touched.  (Every decision of the rule:
tests/test_one_writer_rule_model.py; with a ctx, on a GPU: tests/test_gpu_one_writer.py.)"""
import ctypes as C
import os
import re

import pytest

import one_writer_ref as R
from util import flate, make_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flate_hip_one_writer_bound", "flate_hip_one_writer_open", "flate_hip_one_writer_write",
         "flate_hip_one_writer_reset", "flate_hip_one_writer_free")
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    flate.build()
    from importlib import import_module
    return import_module("moonbit-flate_amd._lib").load()


def test_the_library_exports_what_the_header_declares(lib):
    L = __import__("importlib").import_module("moonbit-flate_amd._lib")
    hdr = open(os.path.join(ROOT, "include", "flate_hip.h")).read()
    res = {"int": C.c_int, "void": None, "size_t": C.c_size_t}
    for name in NAMES:
        assert hasattr(lib, name) and name in L.EXPORTS and name in L.SIGNATURES, name
        decl = re.search(r"\b(int|void|size_t) %s\(([^;]*)\);" % name, hdr)
        assert decl, name
        assert len(decl.group(2).split(",")) == len(L.SIGNATURES[name][1]), name
        assert L.SIGNATURES[name][0] is res[decl.group(1)], name
        fn = getattr(lib, name)
        assert fn.restype is L.SIGNATURES[name][0] and list(fn.argtypes) == L.SIGNATURES[name][1], name
    assert [len(L.SIGNATURES[n][1]) for n in NAMES] == [2, 5, 10, 1, 1]
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    assert L.SIGNATURES["flate_hip_one_writer_open"][1] == [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
    assert L.SIGNATURES["flate_hip_one_writer_write"][1] == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                                                             C.c_uint64, u64p, u64p, C.c_void_p, u32p]
    host = open(os.path.join(ROOT, "moonbit-flate_amd", "host", "flate_host.hpp")).read()
    assert "class OneWriter" in host and all(n + "(" in host for n in NAMES)
    assert callable(flate.FlateEngine.open_one_writer)


def test_the_bound_is_monotone_and_holds_every_call_of_the_reference(lib, oracle):
    for P in (0, 1, 17, 300, 4096, 65535):
        last = 0
        for n in list(range(0, 3000, 13)) + [65534, 65535, 65536, 1 << 20, (1 << 20) + 1, 1 << 32]:
            b = lib.flate_hip_one_writer_bound(n, P)
            assert b == R.bound(n, P) and b >= last, (n, P)
            last = b
    data, _ = make_streams([("rand", 700), ("text", 900), ("zero", 300), ("rand", 300)], seed=5)
    data = data.tobytes()
    for P in (1, 17, 300):
        for T in sorted({0, 1, P - 1, P, P + 1, 3 * P, 3 * P + 5}):
            for wrap in (R.RAW, R.ZLIB, R.GZIP):
                w = R.Whole(oracle, data[:T], P, wrap)
                for sizes in ([], [T], R.fixed(T, P), R.fixed(T, 1), [1, P], R.growing(T)):
                    for c in w.calls(sizes):
                        assert c.out_len <= lib.flate_hip_one_writer_bound(c.in_len, P), (P, T, wrap, c)


def test_null_arguments_are_refused_before_any_device_is_touched(lib):
    h = C.c_void_p()
    buf = (C.c_uint8 * 32)()
    idx = (C.c_uint64 * 8)()
    a, o, k = C.c_uint64(7), C.c_uint64(7), C.c_uint32(7)
    assert lib.flate_hip_one_writer_open(None, 2, 0, 0, C.byref(h)) == INVALID and not h
    assert lib.flate_hip_one_writer_write(None, buf, 32, 0, buf, 32, C.byref(a), C.byref(o), idx, C.byref(k)) == INVALID
    assert (a.value, o.value, k.value) == (7, 7, 7) and not any(idx)  # nothing was written
    assert lib.flate_hip_one_writer_reset(None) == INVALID
    lib.flate_hip_one_writer_free(None)  # (a null handle is nothing to free)
