"""CPU-side checks of the BGZF calls (flate_hip_bgzf_write / _index / _read, flate_hip_bgzf_bound): the symbols are
there and listed, each call refuses a missing ctx before it touches a device, the bound holds for the reference
files -- and the reference itself (tests/bgzf_ref.py) builds files that gzip reads back whole.  (GPU compute:
tests/test_gpu_bgzf.py; the member rule: tests/test_bgzf_index_model.py.)"""
import ctypes as C
import gzip
import importlib

import pytest

import bgzf_ref as ref
from util import flate

CALLS = ["flate_hip_bgzf_bound", "flate_hip_bgzf_write", "flate_hip_bgzf_index", "flate_hip_bgzf_read"]


@pytest.fixture(scope="module")
def lib():
    flate.build()
    return importlib.import_module("moonbit-flate_amd._lib").load()


@pytest.fixture(scope="module")
def inputs():
    return ref.write_inputs()


def test_library_exports_the_bgzf_calls(lib):
    for name in CALLS:
        assert hasattr(lib, name), name


def test_bgzf_calls_are_listed_in_exports():
    exports = importlib.import_module("moonbit-flate_amd._lib").EXPORTS
    for name in CALLS:
        assert name in exports, name


def test_each_call_refuses_a_missing_ctx_before_it_touches_a_device(lib):
    buf = (C.c_uint8 * 64)(*ref.EOF)
    out = (C.c_uint8 * 256)()
    off, off2 = (C.c_uint64 * 4)(), (C.c_uint64 * 4)()
    n64, n32, bad, eo, eof = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_int64(), C.c_int()
    for flags in (0, 1, 2, 3):
        assert lib.flate_hip_bgzf_write(None, buf, 28, 0, out, 256, C.byref(n64), off, flags) == -1
        assert lib.flate_hip_bgzf_index(None, buf, 28, 4, off, off2, C.byref(n32), C.byref(n64), C.byref(eof),
                                        C.byref(eo), flags) == -1
        assert lib.flate_hip_bgzf_read(None, buf, 28, out, 256, C.byref(n64), C.byref(n32), C.byref(bad), C.byref(eo),
                                       C.byref(eof), flags) == -1


@pytest.mark.parametrize("compat", [0, 1])
def test_bound_covers_the_reference_files(lib, oracle, inputs, compat):
    for n, data in inputs.items():
        for bb in (0, 4096, 65280) + ((1,) if n <= 300 else ()):
            f, _ = ref.build_file(oracle, data, bb, compat)
            assert lib.flate_hip_bgzf_bound(n, bb) >= len(f), (n, bb)
    assert lib.flate_hip_bgzf_bound(1000, 65536) == 0 and lib.flate_hip_bgzf_bound(0, 0) == 28


def test_reference_files_are_gzip_files(oracle, inputs):
    for n, data in inputs.items():
        for compat in (0, 1):
            f, off = ref.build_file(oracle, data, 0, compat)
            assert gzip.decompress(f) == data, n
            w = ref.Walk(f)
            assert (w.rc, w.member_off[:-1], w.eof_marker) == (0, [int(x) for x in off], 1), n
            assert w.out_bytes == n and f.endswith(ref.EOF)


def test_many_member_files_start_members_everywhere(oracle):
    f, plain = ref.many_members(1025)
    w = ref.Walk(f)
    assert w.n_members == 1025 and gzip.decompress(f) == plain
    assert {o % 64 for o in w.member_off[:-1]} == set(range(64))  # members start at every offset of a cache line
    sizes = {w.member_off[i + 1] - w.member_off[i] for i in range(1025)}
    assert 28 in sizes and ref.MEMBER_MAX in sizes
