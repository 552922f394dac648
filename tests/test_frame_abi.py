"""CPU-side checks of the framed encode calls (flate_hip_deflate_fast_batch_framed / _spliced_framed,
flate_hip_frame_overhead): the symbols are there, the overhead arithmetic is the oracle's, both calls refuse a
missing ctx before they touch a device.  (That the C++ host mirror compiles against them:
tests/test_host_cpp_framed.py; GPU compute: tests/test_gpu_deflate_framed.py.)"""
import ctypes as C
import importlib

import pytest

from util import flate


@pytest.fixture(scope="module")
def lib():
    flate.build()
    return importlib.import_module("moonbit-flate_amd._lib").load()


def test_library_exports_the_framed_calls(lib):
    listed = importlib.import_module("moonbit-flate_amd._lib").EXPORTS
    for name in ("flate_hip_frame_overhead", "flate_hip_deflate_fast_batch_framed",
                 "flate_hip_deflate_fast_spliced_framed"):
        assert hasattr(lib, name), name
        assert name in listed, name


def test_frame_overhead(lib, oracle):
    engine = importlib.import_module("moonbit-flate_amd.engine")
    raw, zl, gz = engine.WRAP_RAW, engine.WRAP_ZLIB, engine.WRAP_GZIP
    assert (raw, zl, gz) == (0, 1, 2)
    assert lib.flate_hip_frame_overhead(raw, 0) == 0 and lib.flate_hip_frame_overhead(raw, 1) == 0
    assert lib.flate_hip_frame_overhead(zl, 0) == 6
    assert lib.flate_hip_frame_overhead(zl, 1) == 10
    assert lib.flate_hip_frame_overhead(gz, 0) == 18
    assert lib.flate_hip_frame_overhead(3, 0) == 0 and lib.flate_hip_frame_overhead(0xFFFFFFFF, 1) == 0
    # the oracle's frames (no dictionaries there)
    L = oracle.lib()
    for kind, wrap in ((oracle.FRAME_RAW, raw), (oracle.FRAME_ZLIB, zl), (oracle.FRAME_GZIP, gz)):
        assert lib.flate_hip_frame_overhead(wrap, 0) == L.orc_frame_overhead(kind)
    assert engine.frame_overhead("zlib") == 6 and engine.frame_overhead("zlib", True) == 10
    assert engine.frame_overhead("gzip") == 18 and engine.frame_overhead("raw") == 0
    # a member of an empty stream: header, the closing block, the checksum of nothing
    assert len(oracle.frame(oracle.FRAME_ZLIB, oracle.deflate(b""), b"")) == 5 + 6
    assert len(oracle.frame(oracle.FRAME_GZIP, oracle.deflate(b""), b"")) == 5 + 18


def test_framed_calls_refuse_a_missing_ctx_before_they_touch_a_device(lib):
    off = (C.c_uint64 * 2)(0, 4)
    out_off = (C.c_uint64 * 2)()
    buf = (C.c_uint8 * 4)(1, 2, 3, 4)
    out = (C.c_uint8 * 64)()
    n = C.c_uint64(0)
    for wrap in (0, 1, 2, 3):
        assert lib.flate_hip_deflate_fast_batch_framed(None, buf, off, 1, wrap, None, None, 0, None, out, 64,
                                                       out_off, 0) == -1
        assert lib.flate_hip_deflate_fast_spliced_framed(None, buf, off, 1, wrap, out, 64, C.byref(n), None, 0) == -1
    # (an unknown wrap and gzip with dictionary arguments are refused in front of any HIP call as well; that needs
    # a ctx, i.e. a GPU: tests/test_gpu_deflate_framed.py)

