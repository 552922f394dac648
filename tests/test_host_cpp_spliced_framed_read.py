"""C++ host mirror (flate_host.hpp) of the spliced framed read call: decompress_spliced(eng, member, bit_off, sizes,
Wrap, out), driven by tests/host_cpp/spliced_framed_read_driver.cpp and compared here with the CPU fixtures of
tests/spliced_framed_ref.py (the oracle's spliced stream, index and frame)."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from framed_read_ref import gzmember
from spliced_framed_ref import fixture_members
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "spliced_framed_read_driver")
    src = os.path.join(HERE, "host_cpp", "spliced_framed_read_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_spliced_framed_read_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


def _run(exe, cases):
    """cases: (wrap, member, bit_off, sizes).  Returns ({i: (error text, bytes)}, {i: round trip verdict})."""
    blob = struct.pack("<I", len(cases))
    for wrap, member, bit_off, sizes in cases:
        blob += struct.pack("<II", 1 if wrap == "zlib" else 2, len(sizes))
        blob += np.asarray(bit_off, np.uint64).tobytes() + np.asarray(sizes, np.uint64).tobytes()
        blob += struct.pack("<I", len(member)) + member
    case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
    case.write(blob)
    case.close()
    try:
        out = subprocess.run([exe, case.name], capture_output=True, text=True, timeout=180)
    finally:
        os.unlink(case.name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows, again = {}, {}
    for ln in out.stdout.splitlines():
        f = ln.split(" ")
        if f[0] == "c":
            rows[int(f[1])] = (f[2], bytes.fromhex(f[3]) if len(f) > 3 else b"")
        elif f[0] == "r":
            again[int(f[1])] = f[2]
    return rows, again


@pytest.mark.gpu
def test_one_member_read_through_the_cpp_mirror(oracle):
    exe = _compile()
    ms = fixture_members(oracle)
    z, g = ms[("moonbit", "zlib")], ms[("go", "gzip")]
    flipped = bytearray(z.member)
    flipped[-1] ^= 1
    cut = g.member[:g.hl] + g.raw[:-1] + g.trailer
    off_boundary = g.bit_off.copy()
    off_boundary[7] += 1
    cases = [
        ("zlib", z.member, z.bit_off, z.sizes),
        ("gzip", g.member, g.bit_off, [s + 70000 for s in g.sizes]),
        ("gzip", gzmember(g.whole, flg=4 | 8 | 2, extra=b"\x09" * 33, raw=g.raw), g.bit_off, g.sizes),
        ("zlib", bytes(flipped), z.bit_off, z.sizes),
        ("gzip", b"\x1f\x8c" + g.member[2:], g.bit_off, g.sizes),
        ("gzip", cut, g.bit_off, g.sizes),
        ("gzip", g.member, off_boundary, g.sizes),
        ("zlib", bytes([0x78, 0x01, 0x01, 0x00, 0x00, 0xff, 0xff, 0, 0, 0, 1]), [0], []),
    ]
    rows, again = _run(exe, cases)
    assert len(rows) == len(cases)
    assert rows[0] == ("-", z.whole) and rows[1] == ("-", g.whole) and rows[2] == ("-", g.whole)
    assert rows[3] == ("flate:_corrupt_input_before_offset_%d" % len(z.member), z.whole)
    assert rows[4] == ("flate:_corrupt_input_before_offset_0", b"")
    assert rows[5][0] == "unexpected_EOF" and rows[5][1] == oracle.inflate(g.raw[:-1], len(g.whole), full=True)[1]
    assert rows[6][0] != "-" and rows[6][1][:sum(g.sizes[:6])] == g.whole[:sum(g.sizes[:6])]
    assert rows[7] == ("-", b"")
    assert again == {0: "ok", 1: "ok", 2: "ok", 7: "ok"}
