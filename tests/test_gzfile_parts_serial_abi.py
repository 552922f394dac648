"""flate_hip_gzfile_reader_set_serial_max / _last_route without a GPU: the library exports the two calls, _lib.py lists
them with the header's argument counts, the C++ and the Python reader carry them, and every FLATE_HIP_E_INVALID case
that needs no handle is decided before anything is touched -- a NULL reader, a NULL result pointer.  (The checks
themselves, the range of S and the fresh rule: tests/test_gzfile_parts_serial_rule_model.py; with a handle, on a GPU:
tests/test_gpu_gzfile_parts_serial.py.)"""
import ctypes as C
import os
import re

import pytest

from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flate_hip_gzfile_reader_set_serial_max", "flate_hip_gzfile_reader_last_route")
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
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(L.SIGNATURES[name][1]), name
        assert L.SIGNATURES[name][0] is C.c_int, name
    assert [len(L.SIGNATURES[n][1]) for n in NAMES] == [2, 4]
    host = open(os.path.join(ROOT, "moonbit-flate_amd", "host", "flate_host.hpp")).read()
    assert all(n + "(" in host for n in NAMES) and "bool set_serial_max(" in host and "Route last_route(" in host
    import inspect
    engine = __import__("importlib").import_module("moonbit-flate_amd.engine")
    assert callable(engine.GzFileReader.set_serial_max) and callable(engine.GzFileReader.last_route)
    assert inspect.signature(flate.FlateEngine.open_gzfile_reader).parameters["serial_max"].default == 0
    # the header no longer calls it a follow-up, and still says that the ctx option is not the reader's
    assert "routing short members whole is the follow-up" not in hdr
    assert 'The ctx option "gzfile_serial_max" is ignored by the reader' in hdr


def test_null_arguments_are_refused_before_anything_is_touched(lib):
    sm, os_, ff = C.c_uint32(7), C.c_uint32(7), C.c_uint64(7)
    assert lib.flate_hip_gzfile_reader_set_serial_max(None, 0) == INVALID
    assert lib.flate_hip_gzfile_reader_set_serial_max(None, 4096) == INVALID
    assert lib.flate_hip_gzfile_reader_last_route(None, C.byref(sm), C.byref(os_), C.byref(ff)) == INVALID
    assert (sm.value, os_.value, ff.value) == (7, 7, 7)  # nothing was written


def test_the_entry_points_check_first_and_make_no_hip_call():
    """The source says so: the argument check is the first statement of both, and neither body names a HIP call or
    the ctx."""
    src = open(os.path.join(ROOT, "moonbit-flate_amd", "csrc", "flate_api_units.hip")).read()
    for name, check in (("flate_hip_gzfile_reader_set_serial_max", "gzfile_reader_set_serial_max_args"),
                        ("flate_hip_gzfile_reader_last_route", "gzfile_reader_last_route_args")):
        body = src[src.index("int %s(" % name):]
        body = body[body.index("{") + 1:body.index("\n}\n")]
        first = [ln.strip() for ln in body.split("\n") if ln.strip() and not ln.strip().startswith("//")][0]
        assert first.startswith("if (%s(" % check) and first.endswith("return FLATE_HIP_E_INVALID;"), (name, first)
        assert "hip" not in body.replace("FLATE_HIP_", "").lower() and "ctx" not in body, name
