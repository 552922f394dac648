"""flate_hip_bgzf_reader_* / flate_hip_bgzf_writer_* without a GPU: the library exports the nine calls, _lib.py lists
them with the header's argument counts, and every FLATE_HIP_E_INVALID case is decided before any HIP call -- a missing
ctx, handle or result pointer here, and (tests/test_bgzf_parts_rule_model.py: the checks themselves) every other
refusal, which the entry points take from api_checks.h in front of their first use of the ctx.  The handles are host
words: open, reset and free touch no device, so they run here.  (On a GPU: tests/test_gpu_bgzf_parts.py; what the
Python classes hand the calls: tests/test_engine_marshalling_bgzf_parts.py.)"""
import ctypes as C
import os
import re

import pytest

from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flate_hip_bgzf_reader_open", "flate_hip_bgzf_reader_read", "flate_hip_bgzf_reader_reset",
         "flate_hip_bgzf_reader_free", "flate_hip_bgzf_writer_bound", "flate_hip_bgzf_writer_open",
         "flate_hip_bgzf_writer_write", "flate_hip_bgzf_writer_reset", "flate_hip_bgzf_writer_free")
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
        assert hasattr(lib, name) and name in L.EXPORTS and name in L.SIGNATURES and name in L.MAY_BE_MISSING, name
        decl = re.search(r"\b(int|void|size_t) %s\(([^;]*)\);" % name, hdr)
        assert decl, name
        assert len(decl.group(2).split(",")) == len(L.SIGNATURES[name][1]), name
        assert L.SIGNATURES[name][0] is {"int": C.c_int, "void": None, "size_t": C.c_size_t}[decl.group(1)], name
    assert [len(L.SIGNATURES[n][1]) for n in NAMES] == [3, 15, 1, 1, 2, 4, 10, 1, 1]
    host = open(os.path.join(ROOT, "moonbit-flate_amd", "host", "flate_host.hpp")).read()
    assert "class BgzfReader" in host and "class BgzfWriter" in host and all(n + "(" in host for n in NAMES)
    assert callable(flate.FlateEngine.open_bgzf_reader) and callable(flate.FlateEngine.open_bgzf_writer)
    # the contract's landmarks: the one difference from the whole call, the progress rule, what is out of scope
    for words in ("THE ONE DIFFERENCE from flate_hip_bgzf_read", "THE PROGRESS RULE: a part of at least 65536 bytes",
                  "Out of scope: ranges in parts", "a .gzi or .bai", "several members (BGZF in parts: flate_hip_bgzf_writer_*)"):
        assert words in hdr, words


def test_the_bound_is_the_whole_calls(lib):
    for n, bb in ((0, 0), (1, 0), (65280, 0), (65281, 0), (10 ** 9, 0), (5000, 4096), (3, 1)):
        assert lib.flate_hip_bgzf_writer_bound(n, bb) == lib.flate_hip_bgzf_bound(n, bb) >= 28
    assert lib.flate_hip_bgzf_writer_bound(100, 65536) == 0  # a block size that is refused


def test_null_arguments_are_refused_before_anything_is_touched(lib):
    h = C.c_void_p()
    buf = (C.c_uint8 * 32)()
    a, o, e = C.c_uint64(7), C.c_uint64(7), C.c_int64(7)
    m, b, k = C.c_uint32(7), C.c_uint32(7), C.c_int(7)
    assert lib.flate_hip_bgzf_reader_open(None, 0, C.byref(h)) == INVALID and not h
    assert lib.flate_hip_bgzf_reader_read(None, buf, 32, 0, buf, 32, C.byref(a), C.byref(o), 0, None, None, C.byref(m),
                                          C.byref(b), C.byref(e), C.byref(k)) == INVALID
    assert (a.value, o.value, m.value, b.value, e.value, k.value) == (7,) * 6  # nothing was written
    assert lib.flate_hip_bgzf_reader_reset(None) == INVALID
    lib.flate_hip_bgzf_reader_free(None)  # (a null handle is nothing to free)
    assert lib.flate_hip_bgzf_writer_open(None, 0, 0, C.byref(h)) == INVALID and not h
    assert lib.flate_hip_bgzf_writer_write(None, buf, 32, 0, buf, 32, C.byref(a), C.byref(o), None, C.byref(m)) == INVALID
    assert (a.value, o.value, m.value) == (7,) * 3
    assert lib.flate_hip_bgzf_writer_reset(None) == INVALID
    lib.flate_hip_bgzf_writer_free(None)


def test_the_entry_points_check_in_front_of_their_first_hip_call():
    """The source says so: in open, read and write the argument check is the first statement, and the ctx is not
    touched before it."""
    for file, pairs in (("flate_api_inflate.hip", (("flate_hip_bgzf_reader_open", "bgzf_reader_open_args"),
                                                    ("flate_hip_bgzf_reader_read", "bgzf_reader_read_args"))),
                        ("flate_api_deflate.hip", (("flate_hip_bgzf_writer_open", "bgzf_writer_open_args"),
                                                    ("flate_hip_bgzf_writer_write", "bgzf_writer_write_args")))):
        src = open(os.path.join(ROOT, "moonbit-flate_amd", "csrc", file)).read()
        for name, check in pairs:
            body = src[src.index("int %s(" % name):]
            body = body[body.index("{") + 1:]
            lines = [ln.strip() for ln in body.split("\n") if ln.strip() and not ln.strip().startswith("//")]
            first = lines[0] if lines[0].endswith(";") else lines[0] + " " + lines[1]
            assert first.startswith("if (%s(" % check) and first.endswith("return FLATE_HIP_E_INVALID;"), (name, first)
