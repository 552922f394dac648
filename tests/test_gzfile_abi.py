"""flate_hip_gzfile_index / flate_hip_gzfile_read without a GPU: the library exports them, _lib.py lists them with the
header's argument counts, the engine has the two methods, and every argument the calls refuse is refused by the checks
of api_checks.h -- the functions the entry points run in front of any HIP call, compiled here into the stand-alone
program of tests/test_gzfile_rule_model.py.  (With a ctx, i.e. on a GPU, tests/test_gpu_gzfile.py makes the same
refusals through the library.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

from test_gzfile_rule_model import build
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("flate_hip_gzfile_index", "flate_hip_gzfile_read")
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
        assert L.SIGNATURES[name][0] is C.c_int
    assert len(L.SIGNATURES[NAMES[0]][1]) == 18 and len(L.SIGNATURES[NAMES[1]][1]) == 14
    host = open(os.path.join(ROOT, "moonbit-flate_amd", "host", "flate_host.hpp")).read()
    assert "index_gzfile" in host and "decompress_gzfile" in host and all(n + "(" in host for n in NAMES)
    for method in ("gzfile_index", "gzfile_read"):
        assert callable(getattr(flate.FlateEngine, method))


def test_no_ctx_is_refused(lib):
    buf = (C.c_uint8 * 32)()
    w, u, st = C.c_uint64(0), C.c_uint32(0), C.c_int32(0)
    assert lib.flate_hip_gzfile_index(None, buf, 32, 0, None, None, 0, None, None, C.byref(u), C.byref(u), C.byref(w),
                                      None, C.byref(st), None, None, None, 0) == INVALID
    assert lib.flate_hip_gzfile_read(None, buf, 32, None, 0, C.byref(w), None, None, None, C.byref(st), None, None,
                                     None, 0) == INVALID


def test_every_refusal_of_the_argument_checks():
    out = subprocess.run([build(), "checks"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [ln.split() for ln in out.stdout.splitlines()]
    assert len(rows) == 26 and {r[0] for r in rows} == {"index", "read"}
    for call, what, rc in rows:
        assert int(rc) == (0 if what.startswith("ok") else INVALID), (call, what, rc)
    assert sum(1 for r in rows if not r[1].startswith("ok")) == 16
