"""The argument checks of the batch calls (moonbit-flate_amd/csrc/api_checks.h) and the containers' constants
(flate_kernels.h) on the CPU: the entry points refuse a missing ctx first, so through the library every other refusal
needs a device.  tests/host_model/api_checks_model.cpp includes the headers the entry points include."""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "api_checks_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(CSRC, "api_checks.h"), os.path.join(CSRC, "flate_kernels.h"), os.path.join(INC, "flate_hip.h")]
LIB = os.path.join(HERE, "host_model", "libapi_checks_model.so")

OK, INVALID, OUT_TOO_SMALL, CORRUPT, TOO_LARGE, UNEXPECTED_EOF = 0, -1, -2, -4, -6, -7  # include/flate_hip.h
SIZE_ONLY = 8
NO_DICT = 0xffffffff
RAW, ZLIB, GZIP = 0, 1, 2
ADLER32, CRC32 = 1, 2


def u64(*v):
    return (C.c_uint64 * len(v))(*v)


def u32(*v):
    return (C.c_uint32 * len(v))(*v)


@pytest.fixture(scope="module")
def m():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-I" + INC, SRC, "-o", LIB])
    L = C.CDLL(LIB)
    p = C.c_void_p
    L.m_ptrs_ok.argtypes = [p, p, C.c_uint32, p, p, p, p, p, C.c_uint32]
    L.m_ranges.argtypes = [p, C.c_uint32, p, C.c_uint32]
    L.m_deflate_batch_ptrs_ok.argtypes = L.m_deflate_spliced_ptrs_ok.argtypes = [p, p, C.c_uint32, p, p]
    L.m_dict_table_ok.argtypes = [p, p, C.c_uint32]
    L.m_dict_args_ok.argtypes = [p, p, C.c_uint32, p, C.c_uint32]
    L.m_spliced_index_check.argtypes = [p, C.c_uint32, p, C.c_uint64, C.c_uint64]
    L.m_is_stream_status.argtypes = [C.c_int]
    L.m_frame_constants.argtypes = [C.c_uint32, C.c_uint32 * 5]
    L.m_frame_constants.restype = None
    return L


def frame_constants(m, wrap):
    k = (C.c_uint32 * 5)()
    m.m_frame_constants(wrap, k)
    return tuple(k)


def test_container_constants_are_the_rfcs(m):
    # header without / with a dictionary, trailer, shortest member, checksum
    assert frame_constants(m, ZLIB) == (2, 6, 4, 6, ADLER32)  # RFC 1950
    assert frame_constants(m, GZIP) == (10, 10, 8, 18, CRC32)  # RFC 1952


def test_batch_pointers(m):
    buf, up = (C.c_uint8 * 8)(), u64(0, 5, 9)
    a, b, c = (C.c_uint64 * 2)(), (C.c_int32 * 2)(), (C.c_int64 * 2)()
    assert m.m_ptrs_ok(buf, up, 2, buf, up, a, b, c, 0) == 1
    for missing in range(7):  # any one of the seven pointers
        args = [buf, up, 2, buf, up, a, b, c, 0]
        args[missing if missing < 2 else missing + 1] = None
        assert m.m_ptrs_ok(*args) == 0, missing
    # size-only: nothing is stored, out and out_off may be null
    assert m.m_ptrs_ok(buf, up, 2, None, None, a, b, c, SIZE_ONLY) == 1
    assert m.m_ptrs_ok(None, up, 2, None, None, a, b, c, SIZE_ONLY) == 0
    # n = 0: no data pointers, but the arrays
    assert m.m_ptrs_ok(None, up, 0, None, up, a, b, c, 0) == 1
    assert m.m_ptrs_ok(None, None, 0, None, up, a, b, c, 0) == 0
    assert m.m_ptrs_ok(None, up, 0, None, None, a, b, c, 0) == 0


@pytest.mark.parametrize("n", [0, 2])
def test_encode_pointers(m, n):
    buf, up, one = (C.c_uint8 * 8)(), u64(0, 5, 9), (C.c_uint64 * 1)()
    # flate_hip_deflate_fast_batch(_dict, _framed): (in, in_off, n, out, out_off) -- the index arrays always, the data
    # pointers when there are streams
    assert m.m_deflate_batch_ptrs_ok(buf, up, n, buf, up) == 1
    for missing, needed in ((0, n > 0), (1, True), (3, n > 0), (4, True)):
        args = [buf, up, n, buf, up]
        args[missing] = None
        assert m.m_deflate_batch_ptrs_ok(*args) == (0 if needed else 1), missing
    assert m.m_deflate_batch_ptrs_ok(None, up, n, None, up) == (0 if n else 1)
    # flate_hip_deflate_fast_spliced(_framed): (in, in_off, n, out, out_len) -- no streams still write the closing
    # block, so out and out_len always; the bit index is optional and not part of the check
    assert m.m_deflate_spliced_ptrs_ok(buf, up, n, buf, one) == 1
    for missing, needed in ((0, n > 0), (1, True), (3, True), (4, True)):
        args = [buf, up, n, buf, one]
        args[missing] = None
        assert m.m_deflate_spliced_ptrs_ok(*args) == (0 if needed else 1), missing


def test_batch_ranges(m):
    up, down = u64(0, 5, 9), u64(0, 5, 4)
    assert m.m_ranges(up, 2, up, 0) == OK
    assert m.m_ranges(down, 2, up, 0) == INVALID
    assert m.m_ranges(up, 2, down, 0) == INVALID
    assert m.m_ranges(up, 2, None, SIZE_ONLY) == OK  # (out_off is not read)
    assert m.m_ranges(down, 2, None, SIZE_ONLY) == INVALID
    assert m.m_ranges(up, 0, up, 0) == OK
    big = 0x7ffe0000
    assert m.m_ranges(u64(7, 7 + big, 7 + big), 2, up, 0) == TOO_LARGE
    assert m.m_ranges(u64(7, 7 + big - 1, 7 + big - 1), 2, up, 0) == OK
    assert m.m_ranges(u64(7, 7, 7 + big), 2, up, 0) == TOO_LARGE  # (any stream of the batch)
    assert m.m_ranges(u64(0, big, 1), 2, up, 0) == INVALID  # a descending entry wins over a stream too large
    assert m.m_ranges(u64(0, big, big), 2, None, SIZE_ONLY) == TOO_LARGE


def test_dictionary_tables(m):
    d = (C.c_uint8 * 16)()
    up, down, empty = u64(4, 10, 10), u64(4, 10, 9), u64(4, 4, 4)
    for ok, of in ((m.m_dict_table_ok, None), (m.m_dict_args_ok, u32(0, NO_DICT, 1)), (m.m_dict_args_ok, None)):
        tail = () if ok is m.m_dict_table_ok else (of, 3)
        assert ok(d, up, 2, *tail) == 1
        assert ok(d, down, 2, *tail) == 0  # a descending entry
        assert ok(d, None, 2, *tail) == 0  # n_dicts > 0 without dict_off
        assert ok(None, up, 2, *tail) == 0  # non-empty dictionaries without dicts
        assert ok(None, empty, 2, *tail) == 1  # (empty ones need no bytes)
    assert m.m_dict_table_ok(None, None, 0) == 1  # the framed read without dictionaries
    assert m.m_dict_args_ok(d, up, 2, u32(0, 2, 1), 3) == 0  # dict_of out of range
    assert m.m_dict_args_ok(d, up, 2, u32(0, NO_DICT - 1, 1), 3) == 0
    assert m.m_dict_args_ok(d, up, 2, u32(NO_DICT, NO_DICT, NO_DICT), 3) == 1
    assert m.m_dict_args_ok(None, None, 0, u32(NO_DICT, NO_DICT, NO_DICT), 3) == 1  # no table: NO_DICT throughout
    assert m.m_dict_args_ok(None, None, 0, u32(NO_DICT, 0, NO_DICT), 3) == 0
    assert m.m_dict_args_ok(None, None, 0, None, 3) == 0  # "dictionary 0" of none


@pytest.mark.parametrize("wrap", [RAW, ZLIB, GZIP])
def test_spliced_index(m, wrap):
    frame = 0 if wrap == RAW else frame_constants(m, wrap)[3]
    assert frame == {RAW: 0, ZLIB: 6, GZIP: 18}[wrap]
    in_len = frame + 100
    slots = u64(0, 10, 20)
    check = m.m_spliced_index_check
    assert check(u64(0, 300, 800), 2, slots, in_len, frame) == OK  # (the index may end at the last bit)
    assert check(u64(0, 300, 801), 2, slots, in_len, frame) == INVALID  # one bit past 8 * (in_len - frame)
    assert check(u64(0, 801, 801), 2, slots, in_len, frame) == INVALID
    assert check(u64(0, 300, 299), 2, slots, in_len, frame) == INVALID  # a descending entry
    assert check(u64(0, 300, 800), 2, u64(0, 10, 9), in_len, frame) == INVALID
    if frame:
        assert check(u64(0, 0, 0), 2, slots, frame, frame) == OK  # the shortest member: an empty raw stream
        assert check(u64(0, 0, 0), 2, slots, frame - 1, frame) == INVALID  # in_len one below frame_min_len
        assert check(u64(0, 0, 1), 2, slots, frame, frame) == INVALID
    big = 2 ** 30
    assert check(u64(5, 5 + big, 5 + big), 2, slots, frame + 2 ** 28, frame) == TOO_LARGE  # a piece of 2^30 bits
    assert check(u64(5, 4 + big, 4 + big), 2, slots, frame + 2 ** 28, frame) == OK  # one bit less
    assert check(u64(5, 5 + big, 4 + big), 2, slots, frame + 2 ** 28, frame) == TOO_LARGE  # (entry by entry, in order)


def test_is_stream_status(m):
    for rc in range(-9, 2):
        assert m.m_is_stream_status(rc) == (1 if rc in (OK, OUT_TOO_SMALL, CORRUPT, UNEXPECTED_EOF) else 0), rc
