"""C++ host mirror (flate_host.hpp) of the option "gzfile_serial_max" and flate_hip_gzfile_last_route:
Engine::set_option, index_gzfile, decompress_gzfile and Engine::gzfile_last_route, driven by
tests/host_cpp/gzfile_serial_driver.cpp on the mixed file, the 24-member file and a file cut inside its last member, and
compared here with tests/gzfile_serial_ref.py (the model) and the files' plain bytes."""
import os
import struct
import subprocess
import tempfile

import pytest

import gzfile_ref as ref
import gzfile_serial_ref as sref
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
S = 4096


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "gzfile_serial_driver")
    src = os.path.join(HERE, "host_cpp", "gzfile_serial_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def _files():
    """[(file, what a read delivers)]"""
    f, plain, _ = sref.mixed_file()
    pm = ref.phase_members()
    g, gp = b"".join(m for m, _ in pm), b"".join(p for _, p in pm)
    three = ref.three_members()
    h, hp = b"".join(m for m, _ in three), b"".join(p for _, p in three)
    cut = h[:len(h) - len(three[2][0]) // 2]
    return [(f, plain), (g, gp), (cut, hp[:ref.Walk(cut).out_len])]


def test_gzfile_serial_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_index_read_and_route_through_the_cpp_mirror():
    files = _files()
    blob = struct.pack("<I", len(files)) + b"".join(struct.pack("<Q", len(f)) + f for f, _ in files)
    case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
    case.write(blob)
    case.close()
    try:
        out = subprocess.run([_compile(), case.name, str(S)], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(case.name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 2 * len(files)
    kinds = set()
    for k, (f, delivered) in enumerate(files):
        w = ref.Walk(f)
        m = sref.Model(f, S, w)
        head, ub, mu = [p.split() for p in lines[2 * k].split("|")]
        words = [str(x) for x in (w.status, m.n_units, w.n_members, m.serial_members, m.unit_members, m.find_from)]
        assert head == ["r", str(k)] + words, (k, head)
        assert [int(x) for x in ub] == m.unit_bit and [int(x) for x in mu] == m.member_unit, k
        parts = lines[2 * k + 1].split(" ")
        assert parts[:8] == ["d", str(k)] + words, (k, parts[:8])
        assert bytes.fromhex(parts[8]) == delivered, k
        kinds.add((m.serial_members > 0, m.unit_members > 0, w.status != 0))
    assert (True, True, False) in kinds and any(s and bad for s, _, bad in kinds)
