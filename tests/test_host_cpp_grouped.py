"""C++ host mirror (flate_host.hpp) of the grouped splice: compress_grouped, driven by tests/host_cpp/grouped_driver.cpp
and compared here with tests/grouped_ref.py; every member goes back through decompress_spliced with its index slice."""
import os
import struct
import subprocess
import tempfile

import pytest

import grouped_ref as ref
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
WRAPS = {"raw": 0, "zlib": 1, "gzip": 2}


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "grouped_driver")
    src = os.path.join(HERE, "host_cpp", "grouped_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_grouped_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
@pytest.mark.parametrize("wrap,go", [("zlib", False), ("gzip", True), ("raw", False)])
def test_members_and_indexes_through_the_cpp_mirror(oracle, wrap, go):
    data, off, lay = ref.empties()
    big, boff = ref.pieces([("text", 3000), ("rand", 300), ("zero", 128), ("text", 70000), ("rand", 17)], seed=21)
    cases = [ref.Expect(data, off, lay, go), ref.Expect(big, boff, ref.layout([2, 1, 2]), go)]
    for e in cases:
        blob = [struct.pack("<I", e.n_groups)]
        for g in range(e.n_groups):
            lo, hi = int(e.group_off[g]), int(e.group_off[g + 1])
            blob.append(struct.pack("<I", hi - lo))
            for i in range(lo, hi):
                p = e.data[int(e.in_off[i]):int(e.in_off[i + 1])].tobytes()
                blob.append(struct.pack("<Q", len(p)) + p)
        case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
        case.write(b"".join(blob))
        case.close()
        try:
            out = subprocess.run([_compile(), case.name, str(WRAPS[wrap]), "2" if go else "0"], capture_output=True,
                                 text=True, timeout=120)
        finally:
            os.unlink(case.name)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines = out.stdout.splitlines()
        assert len(lines) == e.n_groups
        for g, (ln, member) in enumerate(zip(lines, e.members(wrap))):
            head, idx, back = ln.split("|")
            assert head.split()[:2] == ["m", str(g)]
            assert bytes.fromhex(head.split()[2]) == member, g
            assert [int(x) for x in idx.split()] == ref.member_index(e.bit_off, e.group_off, g).tolist(), g
            assert bytes.fromhex(back) == e.inputs[g], g
