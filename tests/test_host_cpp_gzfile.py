"""C++ host mirror (flate_host.hpp) of flate_hip_gzfile_index and flate_hip_gzfile_read: index_gzfile and
decompress_gzfile, driven by tests/host_cpp/gzfile_driver.cpp on three files of the corpus and compared here with
tests/gzfile_ref.py (the walk) and the files' plain bytes."""
import os
import struct
import subprocess
import tempfile

import pytest

import gzfile_ref as ref
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
MSGS = {0: "-", ref.CORRUPT: "flate:_corrupt_input_before_offset_%d", ref.UNEXPECTED_EOF: "unexpected_EOF"}


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "gzfile_driver")
    src = os.path.join(HERE, "host_cpp", "gzfile_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def _files():
    """[(file, what a read delivers)]: the 24-member file, a file cut inside its last member's stream, and bytes behind
    the last member."""
    pm = ref.phase_members()
    f, plain = b"".join(m for m, _ in pm), b"".join(p for _, p in pm)
    three = ref.three_members()
    g, gp = b"".join(m for m, _ in three), b"".join(p for _, p in three)
    cut = g[:len(g) - len(three[2][0]) // 2]
    return [(f, plain), (cut, gp[:ref.Walk(cut).out_len]), (g + b"\0" * 8, gp)]


def _run(args):
    files = _files()
    blob = struct.pack("<I", len(files)) + b"".join(struct.pack("<Q", len(f)) + f for f, _ in files)
    case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
    case.write(blob)
    case.close()
    try:
        out = subprocess.run([_compile(), case.name] + args, capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(case.name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return files, out.stdout.splitlines()


def test_gzfile_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_index_through_the_cpp_mirror():
    files, lines = _run([])
    assert len(lines) == len(files)
    walks = [ref.Walk(f) for f, _ in files]
    assert [w.status for w in walks] == [0, ref.UNEXPECTED_EOF, ref.CORRUPT]
    for k, (w, ln) in enumerate(zip(walks, lines)):
        head, *arrays = [part.split() for part in ln.split("|")]
        msg = MSGS[w.status] % w.err_off if "%" in MSGS[w.status] else MSGS[w.status]
        assert head == ["r", str(k)] + [str(x) for x in (w.status, w.n_units, w.n_members, w.out_bytes, w.bad_member,
                                                         w.err_off, w.stream_err_off)] + [msg], head
        assert [[int(x) for x in a] for a in arrays] == [w.unit_bit, w.out_off, w.member_off, w.member_unit], k


@pytest.mark.gpu
def test_read_through_the_cpp_mirror():
    files, lines = _run(["read"])
    assert len(lines) == len(files)
    for k, ((f, delivered), ln) in enumerate(zip(files, lines)):
        w = ref.Walk(f)
        parts = ln.split(" ")
        msg = MSGS[w.status] % w.err_off if "%" in MSGS[w.status] else MSGS[w.status]
        assert parts[:9] == ["d", str(k)] + [str(x) for x in (w.status, w.n_units, w.n_members, w.bad_member, w.err_off,
                                                              w.stream_err_off)] + [msg], parts[:9]
        assert bytes.fromhex(parts[9]) == delivered, k
