"""flate_host::GzFileReader::set_serial_max (host/flate_host.hpp): a small g++ driver reads a gzip file of many short
members through two 64 KiB buffers with S = 4096, on the GPU; zlib says what it inflates to, every member but the ones
a piece cuts at its start is delivered whole, and reset keeps the setting."""
import os
import subprocess

import pytest

import gzfile_ref as gf
import gzip_ref as gz
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
PIECE = 65536


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "gzfile_reader_serial_driver")
    src = os.path.join(HERE, "host_cpp", "gzfile_reader_serial_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    return exe


def test_the_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_short_members_are_delivered_whole_through_two_64_kib_buffers(tmp_path):
    exe = _compile()
    t = gz.text(600000, seed=61)
    members = [gz.member(t[a:a + 1500], 6) for a in range(0, len(t), 1500)]
    f = b"".join(members)
    assert len(f) > 3 * PIECE and b"".join(gf.members_of(f)) == t  # several parts, and the truth
    src, dst = tmp_path / "file.gz", tmp_path / "plain.bin"
    src.write_bytes(f)
    out = subprocess.run([exe, str(src), str(dst), str(PIECE), str(PIECE), "4096"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(ln.split(" ", 1) for ln in out.stdout.splitlines())
    n = len(members)
    assert lines["end"] == "EOF" and lines["close"] == "none" and lines["members"] == str(n), lines
    assert dst.read_bytes() == t
    # a piece of 64 KiB always holds its first member whole, and a member it cuts behind that waits for the next step
    assert lines["serial_members"] == str(n), lines
    assert int(lines["calls"]) >= len(f) // PIECE  # it went through the buffers, not around them
    assert (lines["late_set"], lines["too_large_set"]) == ("0", "0"), lines
    assert (lines["again_members"], lines["again_serial_members"], lines["again_same"]) == (str(n), str(n), "1"), lines
