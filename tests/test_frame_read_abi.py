"""CPU-side checks of the framed read call (flate_hip_inflate_batch_framed): the symbol is there and listed, and
every wrap refuses a missing ctx before it touches a device.  (GPU compute: tests/test_gpu_inflate_framed.py; the
C++ host mirror: tests/test_host_cpp_framed_read.py; the clipped checksum arithmetic: tests/test_checksum_clip.py.)"""
import ctypes as C
import importlib

import pytest

from util import flate


@pytest.fixture(scope="module")
def lib():
    flate.build()
    return importlib.import_module("moonbit-flate_amd._lib").load()


def test_library_exports_the_framed_read_call(lib):
    assert hasattr(lib, "flate_hip_inflate_batch_framed")


def test_framed_read_call_is_listed_in_exports():
    assert "flate_hip_inflate_batch_framed" in importlib.import_module("moonbit-flate_amd._lib").EXPORTS


def test_framed_read_refuses_a_missing_ctx_before_it_touches_a_device(lib):
    member = bytes([0x78, 0x01, 0x01, 0x00, 0x00, 0xff, 0xff, 0, 0, 0, 1])
    buf = (C.c_uint8 * len(member))(*member)
    off = (C.c_uint64 * 2)(0, len(member))
    out = (C.c_uint8 * 64)()
    out_off = (C.c_uint64 * 2)(0, 64)
    out_len = (C.c_uint64 * 1)()
    status = (C.c_int32 * 1)()
    err_off = (C.c_int64 * 1)()
    used = (C.c_uint32 * 1)()
    for wrap in (0, 1, 2, 3):
        for flags in (0, 1, 8):
            assert lib.flate_hip_inflate_batch_framed(None, buf, off, 1, wrap, None, None, 0, out, out_off, out_len,
                                                      status, err_off, used, flags) == -1
    # (an unknown wrap, dictionary arguments with gzip / raw and a bad dictionary table are refused in front of any
    # HIP call as well; that needs a ctx, i.e. a GPU: tests/test_gpu_inflate_framed.py)
