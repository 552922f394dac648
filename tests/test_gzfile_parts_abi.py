"""flate_hip_gzfile_reader_* without a GPU: the library exports the four calls, _lib.py lists them with the header's
argument counts, and every FLATE_HIP_E_INVALID case is decided before any HIP call -- a missing ctx, reader or result
pointer, and (tests/test_gzfile_parts_rule_model.py: the checks themselves) every other refusal, which the entry points
take from api_checks.h in front of their first use of the ctx.  (With a ctx, on a GPU: tests/test_gpu_gzfile_parts.py;
what the Python class hands the calls: tests/test_engine_marshalling_gzfile_parts.py.)"""
import ctypes as C
import os
import re

import pytest

from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flate_hip_gzfile_reader_open", "flate_hip_gzfile_reader_read", "flate_hip_gzfile_reader_reset",
         "flate_hip_gzfile_reader_free")
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    flate.build()
    from importlib import import_module
    return import_module("moonbit-flate_amd._lib").load()


def test_the_library_exports_what_the_header_declares(lib):
    L = __import__("importlib").import_module("moonbit-flate_amd._lib")
    hdr = open(os.path.join(ROOT, "include", "flate_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in L.EXPORTS and name in L.SIGNATURES, name
        decl = re.search(r"\b(int|void) %s\(([^;]*)\);" % name, hdr)
        assert decl, name
        assert len(decl.group(2).split(",")) == len(L.SIGNATURES[name][1]), name
        assert L.SIGNATURES[name][0] is (C.c_int if decl.group(1) == "int" else None), name
    assert [len(L.SIGNATURES[n][1]) for n in NAMES] == [3, 13, 1, 1]
    host = open(os.path.join(ROOT, "moonbit-flate_amd", "host", "flate_host.hpp")).read()
    assert "class GzFileReader" in host and all(n + "(" in host for n in NAMES)
    assert callable(flate.FlateEngine.open_gzfile_reader)
    # the one reader's sentence now points here
    assert "several members read in parts (that is flate_hip_gzfile_reader_*" in hdr


def test_null_arguments_are_refused_before_anything_is_touched(lib):
    h = C.c_void_p()
    buf = (C.c_uint8 * 32)()
    a, o, e, s = C.c_uint64(7), C.c_uint64(7), C.c_int64(7), C.c_int64(7)
    m, u, b = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
    assert lib.flate_hip_gzfile_reader_open(None, 0, C.byref(h)) == INVALID and not h
    assert lib.flate_hip_gzfile_reader_read(None, buf, 32, 0, buf, 32, C.byref(a), C.byref(o), C.byref(m), C.byref(u),
                                            C.byref(b), C.byref(e), C.byref(s)) == INVALID
    assert (a.value, o.value, m.value, u.value, b.value, e.value, s.value) == (7,) * 7  # nothing was written
    assert lib.flate_hip_gzfile_reader_reset(None) == INVALID
    lib.flate_hip_gzfile_reader_free(None)  # (a null handle is nothing to free)


def test_the_entry_points_check_in_front_of_their_first_hip_call():
    """The source says so: in open and read the argument check is the first statement, and the ctx is not touched
    before it."""
    src = open(os.path.join(ROOT, "moonbit-flate_amd", "csrc", "flate_api_units.hip")).read()
    for name, check in (("flate_hip_gzfile_reader_open", "gzfile_reader_open_args"),
                        ("flate_hip_gzfile_reader_read", "gzfile_reader_read_args")):
        body = src[src.index("int %s(" % name):]
        body = body[body.index("{") + 1:]
        first = [ln.strip() for ln in body.split("\n") if ln.strip() and not ln.strip().startswith("//")][0]
        assert first.startswith("if (%s(" % check) and first.endswith("return FLATE_HIP_E_INVALID;"), (name, first)
