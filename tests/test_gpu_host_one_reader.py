"""flate_host::OneReader (host/flate_host.hpp): a small g++ driver reads one long gzip member through two 64 KiB
buffers, on the GPU; zlib says what it inflates to."""
import os
import subprocess
import zlib

import pytest

import gzip_ref
import one_ref as ref
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
PIECE = 65536


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "one_reader_driver")
    src = os.path.join(HERE, "host_cpp", "one_reader_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    return exe


def test_the_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_one_stream_round_trips_through_two_64_kib_buffers(tmp_path):
    exe = _compile()
    plain = gzip_ref.text(1500000, seed=52)
    raw = ref.deflate(plain, 6, mem=2)
    member = ref.wrap(raw, plain, ref.GZIP)
    assert len(member) > 3 * PIECE and zlib.decompress(member, 31) == plain  # several parts, and the truth
    src, dst = tmp_path / "member.gz", tmp_path / "plain.bin"
    src.write_bytes(member + b"NEXT")
    out = subprocess.run([exe, str(src), str(dst), str(PIECE), str(PIECE)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(ln.split(" ", 1) for ln in out.stdout.splitlines())
    assert lines["end"] == "EOF" and lines["close"] == "none", lines
    assert dst.read_bytes() == plain
    assert int(lines["calls"]) >= len(member) // PIECE  # it went through the buffers, not around them
    assert int(lines["resident"]) <= 4 * PIECE + 8192 and lines["unread"] == "4"  # ... and left what lies behind the member
