"""C++ host mirror (flate_host.hpp) of the packed windows' three calls: pack_seek_windows, unpack_seek_windows and
decompress_one_ranges_packed, driven by tests/host_cpp/seek_pack_driver.cpp on one file of the corpus in both modes and
compared here with tests/seek_pack_ref.py (the model), the oracle encoder's streams and zlib's bytes."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import one_ref as ref
import seek_pack_ref as sp
import seek_ref as sk
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "seek_pack_driver")
    src = os.path.join(HERE, "host_cpp", "seek_pack_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & sk.U64
    return h


def test_seek_pack_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_one_file_round_trips_through_the_cpp_mirror(oracle):
    exe = _compile()
    _, raw, plain = ref.good_streams()[ref.MANY_UNITS]
    w, cps = ref.Walk(raw), sp.copies(raw)
    T = len(plain)
    ranges = [(0, 10), (T - 5, T + 100), (100000, 100000), (150000, 190000), (7, 9)]
    cases = [(ref.GZIP, 40000, 1, ranges), (ref.RAW, 40000, 0, ranges[::-1])]
    blob = struct.pack("<I", len(cases))
    for kind, span, sparse, rg in cases:
        f = ref.wrap(raw, plain, kind)
        blob += struct.pack("<IQIQ", kind, span, sparse, len(f)) + f + struct.pack("<I", len(rg))
        blob += struct.pack("<%dQ" % len(rg), *[b for b, _ in rg]) + struct.pack("<%dQ" % len(rg), *[e for _, e in rg])
    case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
    case.write(blob)
    case.close()
    try:
        out = subprocess.run([exe, case.name], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(case.name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 3 * len(cases)
    for k, (kind, span, sparse, rg) in enumerate(cases):
        mode = sp.COMPRESS | (sp.SPARSE if sparse else 0)
        pts = sk.points(w.out_off, span)
        blks, kept = sp.blocks(plain, w.out_off, pts, mode, cps)
        off, packed = sp.pack(blks, lambda b: oracle.deflate(np.frombuffer(b, np.uint8)))
        index = sk.index_words(w, plain, len(raw), kind, span)
        head, words, data = [part.split() for part in lines[3 * k].split("|")]
        assert head == ["p", str(k), "0", str(kept), str(len(packed)), "-"], head
        assert [int(x) for x in words] == sp.pack_words(index, mode, off, kept), k
        assert bytes.fromhex(data[0]) == packed, k
        want_w = b"".join(blks)
        same = int(want_w == sk.windows(plain, w.out_off, pts))
        assert (not sparse) == bool(same)  # (the sparse windows differ from the build's, the others are the build's)
        assert lines[3 * k + 1].split() == ["u", str(k), "-", str(len(want_w)), str(same), str(fnv1a(want_w))], k
        m = sk.read(plain, w.out_off, pts, [b for b, _ in rg], [e for _, e in rg])
        head, o, status, data = [part.split() for part in lines[3 * k + 2].split("|")]
        assert head == ["r", str(k), "0", str(m[3]), str(sk.NO_UNIT), "-"], head
        assert [int(x) for x in o] == m[1] and [int(x) for x in status] == m[2], k
        assert bytes.fromhex(data[0] if data else "") == b"".join(m[5]), k
