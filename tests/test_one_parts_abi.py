"""flate_hip_one_reader_* without a GPU: the library exports the four calls, _lib.py lists them with the header's
argument counts, a missing ctx, reader or result pointer is refused before anything is touched, and
FlateEngine.open_one_reader hands the calls what the header asks for -- recorded against a library that answers from a
script (tests/engine_trace_one_parts.py) and held against tests/golden/engine_calls_one_parts.json.  (Every refusal of
the argument checks: tests/test_one_parts_rule_model.py; with a ctx, on a GPU: tests/test_gpu_one_parts.py.)"""
import ctypes as C
import json
import os
import re

import pytest

import engine_trace
import engine_trace_one_parts as trace
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flate_hip_one_reader_open", "flate_hip_one_reader_read", "flate_hip_one_reader_reset", "flate_hip_one_reader_free")
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
    assert [len(L.SIGNATURES[n][1]) for n in NAMES] == [4, 10, 1, 1]
    host = open(os.path.join(ROOT, "moonbit-flate_amd", "host", "flate_host.hpp")).read()
    assert "class OneReader" in host and all(n + "(" in host for n in NAMES)
    assert callable(flate.FlateEngine.open_one_reader)


def test_null_arguments_are_refused_before_anything_is_touched(lib):
    h = C.c_void_p()
    buf = (C.c_uint8 * 32)()
    a, o, e, u = C.c_uint64(7), C.c_uint64(7), C.c_int64(7), C.c_uint32(7)
    assert lib.flate_hip_one_reader_open(None, 2, 0, C.byref(h)) == INVALID and not h
    assert lib.flate_hip_one_reader_read(None, buf, 32, 0, buf, 32, C.byref(a), C.byref(o), C.byref(e), C.byref(u)) == INVALID
    assert (a.value, o.value, e.value, u.value) == (7, 7, 7, 7)  # nothing was written
    assert lib.flate_hip_one_reader_reset(None) == INVALID
    lib.flate_hip_one_reader_free(None)  # (a null handle is nothing to free)


def test_the_python_reader_hands_the_calls_what_the_header_asks_for():
    want = json.load(open(trace.FIXTURE))
    assert list(want) == list(trace.SCENARIOS)
    got = {name: trace.run(name) for name in trace.SCENARIOS}
    for name in trace.SCENARIOS:
        assert got[name] == want[name], name
    names = {c: [a[0] for a in engine_trace.SIGNATURES["flate_hip_" + c]] for c in ("one_reader_open", "one_reader_read")}
    for dev, flags in (("host", 0), ("dev", flate.DEVICE_PTRS if hasattr(flate, "DEVICE_PTRS") else 1)):
        t = got["read/zlib/final/" + dev]["trace"]
        assert [c[0] for c in t] == ["one_reader_open", "one_reader_read", "one_reader_free"]
        opened = dict(zip(names["one_reader_open"], t[0][1]))
        assert (opened["wrap"], opened["flags"]) == (1, flags)  # the side is fixed at open
        read = dict(zip(names["one_reader_read"], t[1][1]))
        assert (read["in"], read["in_len"], read["final"]) == ("data", 200, 1)
        assert read["cap"] == 65536  # four times the part, 64 KiB at least
    # a first unit that does not fit: one more call with exactly the room it asked for
    t = got["read/second_sizing_call/host"]["trace"]
    assert [dict(zip(names["one_reader_read"], c[1]))["cap"] for c in t[1:3]] == [65536, 5000]
    # ... but not when the caller set the capacity; the statuses come back, anything else raises
    assert got["read/too_small_with_out_cap"]["ret"]["t"][2] == {"OnePartRead": [-2, 5000, -1, 0]}
    assert got["read/status-4"]["ret"]["t"][2] == {"OnePartRead": [-4, 25, 1234, 3]}
    assert got["read/raises"]["raises"] == "FlateError" and got["read/raises"]["code"] == -8
    assert got["read/raises"]["trace"][-1][0] == "one_reader_free"  # the handle is freed all the same
    assert got["read/wrong_side"]["raises"] == "FlateError" and len(got["read/wrong_side"]["trace"]) == 2
    # an empty part goes in as NULL with length 0; reset between two streams; the handle is freed once
    assert got["read/empty_part"]["trace"][1][1][1:3] == ["null", 0]
    assert [c[0] for c in got["reset_and_a_second_stream"]["trace"]] == [
        "one_reader_open", "one_reader_read", "one_reader_reset", "one_reader_read", "one_reader_free"]
