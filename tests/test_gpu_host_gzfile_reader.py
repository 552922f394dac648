"""flate_host::GzFileReader (host/flate_host.hpp): a small g++ driver reads a gzip file of several members through two
64 KiB buffers, on the GPU; zlib says what it inflates to, and a wrong trailer ends it with the member's words."""
import os
import subprocess

import pytest

import gzfile_ref as gf
import gzip_ref as gz
import one_ref as ref
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
PIECE = 65536


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "gzfile_reader_driver")
    src = os.path.join(HERE, "host_cpp", "gzfile_reader_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    return exe


def test_the_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_a_file_of_members_round_trips_through_two_64_kib_buffers(tmp_path):
    exe = _compile()
    t = gz.text(1500000, seed=53)
    cuts = [0, 600000, 600500, 601000, 1300000, 1500000]
    members = [gf.wrap(ref.deflate(t[a:b], 6, mem=2), t[a:b]) for a, b in zip(cuts, cuts[1:])]
    f = b"".join(members)
    assert len(f) > 3 * PIECE and b"".join(gf.members_of(f)) == t  # several parts, and the truth
    src, dst = tmp_path / "file.gz", tmp_path / "plain.bin"
    src.write_bytes(f)
    out = subprocess.run([exe, str(src), str(dst), str(PIECE), str(PIECE)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(ln.split(" ", 1) for ln in out.stdout.splitlines())
    assert lines["end"] == "EOF" and lines["close"] == "none" and lines["members"] == "5", lines
    assert dst.read_bytes() == t
    assert int(lines["calls"]) >= len(f) // PIECE  # it went through the buffers, not around them
    assert int(lines["resident"]) <= 4 * PIECE + 8192
    # a wrong CRC-32 in the fourth member: its bytes are delivered, nothing behind them, and the words are the file's
    bad = bytearray(f)
    end = sum(len(m) for m in members[:4])
    bad[end - 8] ^= 1
    src.write_bytes(bytes(bad))
    out = subprocess.run([exe, str(src), str(dst), str(PIECE), str(PIECE)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(ln.split(" ", 1) for ln in out.stdout.splitlines())
    off = sum(len(m) for m in members[:3])
    assert lines["end"] != "EOF" and lines["close"] == "error" and lines["members"] == "3", lines
    assert (lines["bad_member"], lines["err_off"], lines["stream_err_off"]) == ("3", str(off), str(len(members[3]))), lines
    assert dst.read_bytes() == t[:1300000]
