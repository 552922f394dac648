"""flate_host::OneWriter (host/flate_host.hpp): a small g++ driver writes one long gzip member through the mirror with
awkward write sizes and a small part size, on the GPU, and the whole call over the same pieces beside it; the two files
must be the same bytes, and zlib must read them back to the input."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from util import flate, make_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "one_writer_driver")
    src = os.path.join(HERE, "host_cpp", "one_writer_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    return exe


def test_the_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
@pytest.mark.parametrize("wrap,piece,part,size", [(2, 0, 200000, 700001), (1, 4096, 4096, 300000), (0, 300, 1000, 90007),
                                                  (2, 65535, 65535, 0)])
def test_awkward_writes_give_the_whole_calls_bytes(tmp_path, wrap, piece, part, size):
    exe = _compile()
    data, _ = make_streams([("text", size // 2), ("rand", size // 4), ("text", size - size // 2 - size // 4)], seed=17)
    plain = data[:size].tobytes()
    src, dst, whole = tmp_path / "plain.bin", tmp_path / "parts.out", tmp_path / "whole.out"
    src.write_bytes(plain)
    out = subprocess.run([exe, str(src), str(dst), str(whole), str(wrap), str(piece), str(part)], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(ln.split(" ", 1) for ln in out.stdout.splitlines())
    assert lines["close"] == "none" and lines["again"] == "none" and lines["late"] == "writer closed", lines
    assert lines["whole"] == "0"
    got = dst.read_bytes()
    assert got == whole.read_bytes()
    assert zlib.decompress(got, {0: -15, 1: 15, 2: 31}[wrap]) == plain
    P = piece or 65535
    assert int(lines["pieces"]) == -(-size // P) and int(lines["emitted"]) == len(got)
    # it went through the buffers, not around them: more than one call, and never much more staged than a part and a write
    if size:
        assert int(lines["calls"]) >= max(2, size // (part + 100000))
        assert int(lines["resident"]) <= 8 * (part + 100000) + 65536
