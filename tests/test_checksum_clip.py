"""The piece-and-clip arithmetic of the checksum kernels (moonbit-flate_amd/csrc/checksum_clip.h), on the CPU: when
the 64 KiB pieces of a stream are planned over its output SLOT and the stream then produces fewer bytes
(flate_hip_inflate_batch_framed), the clipped pieces must tile exactly what was produced, no lane's run may count
bytes beyond it, and folding the per-piece sums the way checksum_fold_kernel does must give zlib's Adler-32 / CRC-32.
tests/host_model/checksum_clip_model.cpp includes the header the kernels include."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "checksum_clip_model.cpp")
HDR = os.path.join(ROOT, "moonbit-flate_amd", "csrc", "checksum_clip.h")
LIB = os.path.join(HERE, "host_model", "libchecksum_clip_model.so")

PIECE = 65536
SLOTS = [0, 1, 65535, 65536, 65537, 131072, 200000, 64 * PIECE + 1, 257 * PIECE]


def produced_values(slot):
    v = {0, 1, slot - 1, slot} | set(range(PIECE, slot, PIECE))  # ... and the 64 KiB edges below slot
    return sorted(x for x in v if 0 <= x <= slot)


@pytest.fixture(scope="module")
def model():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.dirname(HDR), SRC,
                               "-o", LIB])
    L = C.CDLL(LIB)
    L.clip_prepare.argtypes = [C.c_void_p, C.c_uint64]
    L.clip_prepare.restype = None
    L.clip_fold.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.clip_fold.restype = C.c_int
    return L


@pytest.fixture(scope="module")
def data(model):
    rng = np.random.default_rng(20)
    d = rng.integers(0, 256, max(SLOTS) + 16, dtype=np.uint8)
    d[3 * PIECE:5 * PIECE] = 255  # (the largest per-piece sums)
    model.clip_prepare(d.ctypes.data, max(SLOTS))
    return d


@pytest.fixture(scope="module")
def want(data):
    """{produced: (adler32, crc32)} of data[:produced], one running pass over the buffer"""
    out, a, c, at = {}, 1, 0, 0
    for p in sorted({p for s in SLOTS for p in produced_values(s)}):
        chunk = data[at:p].tobytes()
        a, c, at = zlib.adler32(chunk, a), zlib.crc32(chunk, c), p
        out[p] = (a, c)
    return out


@pytest.mark.parametrize("slot", SLOTS)
def test_clipped_pieces_tile_what_was_produced_and_fold_to_zlibs_sums(model, data, want, slot):
    for produced in produced_values(slot):
        a, c = C.c_uint32(0), C.c_uint32(0)
        rc = model.clip_fold(slot, produced, C.byref(a), C.byref(c))
        assert rc == 0, (slot, produced, {1: "the pieces do not tile [0, produced)", 2: "n - end wraps"}[rc])
        assert (a.value, c.value) == want[produced], (slot, produced)


def test_nothing_produced_is_the_sum_of_nothing(model, data):
    for slot in SLOTS:
        a, c = C.c_uint32(7), C.c_uint32(7)
        assert model.clip_fold(slot, 0, C.byref(a), C.byref(c)) == 0
        assert (a.value, c.value) == (1, 0) == (zlib.adler32(b""), zlib.crc32(b""))
