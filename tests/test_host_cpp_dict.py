"""C++ host mirror (flate_host.hpp) of batch inflate with preset dictionaries: decompress_batch / inflate_sizes
with dictionaries and dict_of, driven by tests/host_cpp/dict_driver.cpp, against the oracle."""
import os
import struct
import subprocess
import tempfile
import zlib

import pytest

from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "dict_driver")
    src = os.path.join(HERE, "host_cpp", "dict_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_dict_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_dictionary_batch_through_the_cpp_mirror(oracle):
    exe = _compile()
    words = lambda seed, n: flate.synth("text", 1, n, seed=seed).tobytes()
    dicts = [words(61, 40000), words(62, 900), b""]
    streams = []  # (dictionary index or 0xffffffff, capacity, compressed)
    for k in range(9):
        j = [0, 1, 2, 0xFFFFFFFF][k % 4]
        d = dicts[j] if j != 0xFFFFFFFF else b""
        s = d[-5000:] + words(70 + k, 3000) + d[:300]
        co = zlib.compressobj(1 + k % 9, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, d) if d else \
            zlib.compressobj(1 + k % 9, zlib.DEFLATED, -15)
        streams.append((j, len(s), co.compress(s) + co.flush()))
    streams.append((0xFFFFFFFF, 9000, streams[0][2]))       # its dictionary missing: corrupt
    streams.append((0, 9000, streams[0][2][:len(streams[0][2]) // 2]))  # truncated
    blob = struct.pack("<I", len(dicts)) + b"".join(struct.pack("<I", len(d)) + d for d in dicts)
    blob += struct.pack("<I", len(streams)) + b"".join(struct.pack("<III", j, c, len(b)) + b for j, c, b in streams)
    case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
    case.write(blob)
    case.close()
    try:
        out = subprocess.run([exe, case.name], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(case.name)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split(" ") for ln in out.stdout.splitlines() if ln.startswith("s ")]
    assert len(rows) == len(streams)
    for (j, cap, comp), row in zip(streams, rows):
        status, eoff, size = int(row[1]), int(row[2]), int(row[3])
        got = bytes.fromhex(row[4]) if len(row) > 4 else b""
        rc, want, used, weoff = oracle.inflate(comp, cap, full=True, zdict=dicts[j] if j != 0xFFFFFFFF else None)
        assert status == {0: 0, oracle.E_CORRUPT: -4, oracle.E_UNEXPECTED_EOF: -7}[rc]
        assert eoff == weoff
        if rc == 0:
            assert got == want and size == len(want)
    assert int(rows[-2][1]) == -4 and int(rows[-1][1]) == -7
