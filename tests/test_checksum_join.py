"""The join arithmetic of checksum_join_kernel (moonbit-flate_amd/csrc/checksum_clip.h: crc_concat_term,
adler_concat_term, adler_concat_finish), on the CPU: from the finished Adler-32 / CRC-32 of every piece of a spliced
stream and the bytes behind it, the sums of the CONCATENATION -- what the trailer of a zlib or gzip member around the
spliced stream carries (flate_hip_inflate_spliced_framed).  Every expectation is zlib's sum of the concatenated bytes.
tests/host_model/checksum_join_model.cpp includes the header the kernel includes."""
import ctypes as C
import itertools
import os
import subprocess
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "checksum_join_model.cpp")
HDR = os.path.join(ROOT, "moonbit-flate_amd", "csrc", "checksum_clip.h")
LIB = os.path.join(HERE, "host_model", "libchecksum_join_model.so")

LENGTHS = [0, 1, 3, 17, 65535, 65536, 65537, 70000, 131071]


@pytest.fixture(scope="module")
def model():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.dirname(HDR), SRC,
                               "-o", LIB])
    L = C.CDLL(LIB)
    L.join_concat.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32),
                              C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.join_concat.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(21)
    d = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    d[200000:340000] = 255  # (the largest per-piece sums)
    return d.tobytes()


def join(model, pieces, slots=None):
    """(adler32, crc32, bytes) of the concatenation of `pieces` by the model; slots (default: exact) clip them."""
    n = len(pieces)
    slots = [len(p) for p in pieces] if slots is None else slots
    counted = [p[:s] for p, s in zip(pieces, slots)]
    adlers = np.array([zlib.adler32(p) for p in counted], np.uint32)
    crcs = np.array([zlib.crc32(p) for p in counted], np.uint32)
    produced = np.array([len(p) for p in pieces], np.uint64)
    slot = np.array(slots, np.uint64)
    a, c, t = C.c_uint32(7), C.c_uint32(7), C.c_uint64(7)
    rc = model.join_concat(adlers.ctypes.data, crcs.ctypes.data, produced.ctypes.data, slot.ctypes.data, n,
                           C.byref(a), C.byref(c), C.byref(t))
    assert rc == 0, "the bytes behind a piece would wrap"
    whole = b"".join(counted)
    assert t.value == len(whole)
    return (a.value, c.value), (zlib.adler32(whole), zlib.crc32(whole))


def cut(data, lengths, at=0):
    out = []
    for n in lengths:
        out.append(data[at:at + n])
        at += n
    return out


def test_the_lengths_of_the_issue_in_their_order(model, data):
    got, want = join(model, cut(data, [0, 1, 17, 65536, 0, 70000, 3, 131071]))
    assert got == want


@pytest.mark.parametrize("first", LENGTHS)
def test_every_pair_and_triple_of_lengths(model, data, first):
    for rest in itertools.chain(itertools.product(LENGTHS, repeat=1), itertools.product(LENGTHS, repeat=2)):
        lengths = [first, *rest]
        got, want = join(model, cut(data, lengths, at=195000))
        assert got == want, lengths


def test_leading_trailing_and_consecutive_empties(model, data):
    for lengths in ([0, 0, 17], [17, 0, 0], [0, 65537, 0], [0, 0, 0, 3, 0, 0, 65535, 0, 0, 0], [3, 0, 0, 0, 0, 70000],
                    [0] * 40 + [131071] + [0] * 40 + [1] + [0] * 40):
        got, want = join(model, cut(data, lengths, at=100000))
        assert got == want, lengths


def test_a_single_piece_and_no_piece_at_all(model, data):
    for n in LENGTHS:
        got, want = join(model, cut(data, [n], at=199990))
        assert got == want, n
    assert join(model, [])[0] == (1, 0) == (zlib.adler32(b""), zlib.crc32(b""))
    assert join(model, [b""])[0] == (1, 0)
    assert join(model, [b"", b"", b""])[0] == (1, 0)


def test_many_pieces(model, data):
    """More pieces than one chunk of the kernel's walk, a third of them empty, and sums that wrap 65521 many times."""
    rng = np.random.default_rng(5)
    lengths = [0 if rng.integers(3) == 0 else int(rng.integers(1, 301)) for _ in range(3000)]
    got, want = join(model, cut(data, lengths, at=150000))
    assert got == want


def test_a_piece_counts_no_more_than_its_slot_holds(model, data):
    pieces = cut(data, [70000, 17, 65537, 3])
    got, want = join(model, pieces, slots=[70000, 5, 65536, 0])
    assert got == want
