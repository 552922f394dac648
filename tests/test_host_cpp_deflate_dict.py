"""C++ host mirror (flate_host.hpp) of batch deflate with preset dictionaries: a BatchWriter with a DictTable,
driven by tests/host_cpp/deflate_dict_driver.cpp, read back there by Reader::new_dict and compared here with the
reference helper (tests/deflate_dict_ref.py) and zlib."""
import os
import struct
import subprocess
import tempfile
import zlib

import pytest

from deflate_dict_ref import deflate_dict
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
NO_DICT = 0xFFFFFFFF


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "deflate_dict_driver")
    src = os.path.join(HERE, "host_cpp", "deflate_dict_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_deflate_dict_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
@pytest.mark.parametrize("compat_go", [False, True])
def test_batch_writer_with_dictionaries_through_the_cpp_mirror(compat_go):
    exe = _compile()
    words = lambda seed, n: flate.synth("text", 1, n, seed=seed).tobytes() if n else b""
    dicts = [words(61, 40000), words(62, 900), b"", words(63, 16)]
    streams = []  # (dictionary index or NO_DICT, payload)
    for k in range(11):
        j = [0, 1, 2, NO_DICT, 3][k % 5]
        n = [3000, 100, 70000, 0, 4096, 140000][k % 6]
        d = dicts[j] if j != NO_DICT else b""
        streams.append((j, (d[-300:] + words(70 + k, n))[:n]))
    blob = struct.pack("<II", 1 if compat_go else 0, len(dicts)) + b"".join(struct.pack("<I", len(d)) + d for d in dicts)
    blob += struct.pack("<I", len(streams)) + b"".join(struct.pack("<II", j, len(p)) + p for j, p in streams)
    case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
    case.write(blob)
    case.close()
    try:
        out = subprocess.run([exe, case.name], capture_output=True, text=True, timeout=180)
    finally:
        os.unlink(case.name)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split(" ") for ln in out.stdout.splitlines() if ln.startswith("s ")]
    assert len(rows) == len(streams)
    for i, ((j, p), row) in enumerate(zip(streams, rows)):
        d = dicts[j] if j != NO_DICT else b""
        got = bytes.fromhex(row[2]) if len(row) > 2 else b""
        assert got == deflate_dict(p, d, 1 if compat_go else 0), i
        assert row[1] == "1", "stream %d: Reader::new_dict did not return the payload" % i
        o = zlib.decompressobj(-15, zdict=d[-32768:]) if d else zlib.decompressobj(-15)
        assert o.decompress(got) == p and o.eof
