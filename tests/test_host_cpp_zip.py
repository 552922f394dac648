"""C++ host mirror (flate_host.hpp) of the ZIP calls: compress_zip and decompress_zip, driven by
tests/host_cpp/zip_driver.cpp and compared here with tests/zip_ref.py (the archive around the raw call's streams, the
serial reader) and Python's zipfile."""
import io
import os
import struct
import subprocess
import tempfile
import zipfile
import zlib

import numpy as np
import pytest

import zip_ref as ref
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "zip_driver")
    src = os.path.join(HERE, "host_cpp", "zip_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_zip_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


def _run(exe, blob):
    case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
    case.write(blob)
    case.close()
    try:
        out = subprocess.run([exe, case.name], capture_output=True, text=True, timeout=180)
    finally:
        os.unlink(case.name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return [ln.split(" ") for ln in out.stdout.splitlines()]


@pytest.mark.gpu
def test_round_trip_and_read_through_the_cpp_mirror():
    exe = _compile()
    items = [(n.encode(), d) for n, d in ref.payloads()]
    foreign = dict(ref.zipfile_corpus(big=False))
    what, damaged, bad, status, _ = ref.entry_cases()[0]  # a wrong CRC in the directory
    truncated = ref.three()[:-5]
    blob = struct.pack("<I", 6)
    for flags in (0, 2):
        blob += struct.pack("<III", 0, flags, len(items)) + b"".join(
            struct.pack("<I", len(n)) + n + struct.pack("<Q", len(d)) + d for n, d in items)
    for f in (foreign["mixed"], foreign["unseekable sink"], damaged, truncated):
        blob += struct.pack("<IQ", 1, len(f)) + f
    rows = _run(exe, blob)
    assert len(rows) == 6
    eng = flate.FlateEngine(0)
    src = np.frombuffer(b"".join(d for _, d in items), np.uint8).copy()
    in_off = np.zeros(len(items) + 1, np.uint64)
    np.cumsum([len(d) for _, d in items], out=in_off[1:])
    for k, compat in enumerate((False, True)):
        raw, raw_off = eng.deflate_batch(src, in_off, compat_go=compat)
        raws = [raw[int(raw_off[i]):int(raw_off[i + 1])].tobytes() for i in range(len(items))]
        want, off = ref.write_archive(raws, [n for n, _ in items], [zlib.crc32(d) for _, d in items], [len(d) for _, d in items])
        assert rows[k][:2] == ["w", str(k)] and bytes.fromhex(rows[k][2]) == want, k
        assert [int(x) for x in rows[k][3].split(",")] == off and rows[k][4] == "1", k
        assert zipfile.ZipFile(io.BytesIO(want)).testzip() is None
    eng.close()
    for k, f in ((2, foreign["mixed"]), (3, foreign["unseekable sink"])):
        z = zipfile.ZipFile(io.BytesIO(f))
        assert rows[k][:6] == ["r", str(k), "0", str(len(z.infolist())), "-1", "-"], rows[k][:6]
        got = [e.split(":") for e in rows[k][6].split(",")]
        assert [(bytes.fromhex(n).decode(), int(s), bytes.fromhex(b)) for n, s, b in got] == \
               [(zi.filename, 0, z.read(zi)) for zi in z.infolist()]
    # one entry with a wrong CRC-32: the others are delivered, the error names its header
    ix = ref.Index(damaged)
    assert rows[4][:6] == ["r", "4", str(status), "3", "-1", "flate:_corrupt_input_before_offset_%d" % ix.entries[bad].header_off]
    got = [e.split(":") for e in rows[4][6].split(",")]
    z = zipfile.ZipFile(io.BytesIO(ref.three()))
    assert [(int(s), bytes.fromhex(b)) for _, s, b in got] == \
           [(status, b"") if i == bad else (0, z.read(zi)) for i, zi in enumerate(z.infolist())]
    # a malformed archive: where, nothing delivered
    bad_ix = ref.Index(truncated)
    assert rows[5][:6] == ["r", "5", str(ref.CORRUPT), str(bad_ix.n_entries), str(bad_ix.err_off),
                           "flate:_corrupt_input_before_offset_%d" % bad_ix.err_off] and rows[5][6] == ""
