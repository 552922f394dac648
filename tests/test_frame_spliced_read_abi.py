"""CPU-side checks of the spliced framed read call (flate_hip_inflate_spliced_framed): the symbol is there and listed
with its argument types, and every wrap and flag refuses a missing ctx before it touches a device.  The other
refusals the header promises "before any HIP call" -- an unknown wrap, an index that is not monotone or runs beyond
the member, a member shorter than header plus trailer, FLATE_HIP_SIZE_ONLY, NULL arguments -- need a ctx to tell them
from the missing one, i.e. a GPU: tests/test_gpu_inflate_spliced_framed.py::test_refused_arguments.  (The join
arithmetic: tests/test_checksum_join.py; the C++ host mirror: tests/test_host_cpp_spliced_framed_read.py.)"""
import ctypes as C
import importlib

import pytest

from util import flate


@pytest.fixture(scope="module")
def lib():
    flate.build()
    return importlib.import_module("moonbit-flate_amd._lib").load()


def test_library_exports_the_spliced_framed_read_call(lib):
    assert hasattr(lib, "flate_hip_inflate_spliced_framed")
    assert len(lib.flate_hip_inflate_spliced_framed.argtypes) == 14
    assert lib.flate_hip_inflate_spliced_framed.restype is C.c_int


def test_spliced_framed_read_call_is_listed_in_exports():
    assert "flate_hip_inflate_spliced_framed" in importlib.import_module("moonbit-flate_amd._lib").EXPORTS


def test_spliced_framed_read_refuses_a_missing_ctx_before_it_touches_a_device(lib):
    member = bytes([0x78, 0x01, 0x01, 0x00, 0x00, 0xff, 0xff, 0, 0, 0, 1])
    buf = (C.c_uint8 * len(member))(*member)
    bits = (C.c_uint64 * 2)(0, 0)
    out = (C.c_uint8 * 64)()
    out_off = (C.c_uint64 * 2)(0, 64)
    out_len = (C.c_uint64 * 1)()
    status = (C.c_int32 * 1)()
    err_off = (C.c_int64 * 1)()
    ms, me = C.c_int32(55), C.c_int64(55)
    for wrap in (0, 1, 2, 3):
        for flags in (0, 1, 8):
            for n in (0, 1):
                assert lib.flate_hip_inflate_spliced_framed(None, buf, len(member), wrap, bits, n, out, out_off,
                                                            out_len, status, err_off, C.byref(ms), C.byref(me),
                                                            flags) == -1
    assert (ms.value, me.value) == (55, 55)  # a refused call writes nothing
