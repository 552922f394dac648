"""C++ host mirror (flate_host.hpp) of the plain-gzip calls: decompress_gzip, driven by tests/host_cpp/gzip_driver.cpp
on files of the corpus and compared here with tests/gzip_ref.py (the walk, zlib's own gzip reader)."""
import os
import struct
import subprocess
import tempfile

import pytest

import gzip_ref as ref
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "gzip_driver")
    src = os.path.join(HERE, "host_cpp", "gzip_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_gzip_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_read_through_the_cpp_mirror():
    exe = _compile()
    good = [ref.good_files()[k] for k in (2, 3, 9)] + [ref.decoy_files()[0][:3]]
    broken = [ref.malformed_files()[k] for k in (0, 6, 8)]
    failing = ref.failing_files()[0]
    files = [f for _, f, _ in good] + [b[1] for b in broken] + [failing[1], b""]
    blob = struct.pack("<I", len(files)) + b"".join(struct.pack("<Q", len(f)) + f for f in files)
    case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
    case.write(blob)
    case.close()
    try:
        out = subprocess.run([exe, case.name], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(case.name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [ln.split(" ") for ln in out.stdout.splitlines()]
    assert len(rows) == len(files)
    for k, (what, f, plain) in enumerate(good):
        w = ref.Walk(f)
        assert rows[k][:5] == ["r", str(k), "0", str(w.n_members), str(0xffffffff)] and rows[k][5] == "-1", (what, rows[k][:8])
        assert int(rows[k][6]) >= w.n_members and rows[k][7] == "-" and bytes.fromhex(rows[k][8]) == plain, what
    assert int(rows[3][6]) > ref.Walk(good[3][1]).n_members  # (the decoy file)
    msgs = {ref.CORRUPT: "flate:_corrupt_input_before_offset_%d", ref.UNEXPECTED_EOF: "unexpected_EOF"}
    for k, (what, f, _, rc, err_off, n) in enumerate(broken, start=len(good)):
        msg = msgs[rc] % err_off if "%" in msgs[rc] else msgs[rc]
        assert rows[k][:6] == ["r", str(k), str(rc), str(n), str(n), str(err_off)] and rows[k][7] == msg, (what, rows[k][:8])
        assert rows[k][8] == "", what
    # a member with a wrong CRC on a sound chain: it is named, the others are delivered
    k = len(good) + len(broken)
    what, f, rc, bad = failing
    w = ref.Walk(f)
    assert rows[k][:6] == ["r", str(k), str(rc), "3", str(bad), str(w.member_off[bad])], rows[k][:8]
    got = bytes.fromhex(rows[k][8])
    whole = ref.text(9000, seed=31)[:6500]
    assert len(got) == w.out_bytes and got[:w.out_off[bad]] == whole[:w.out_off[bad]] and \
        got[w.out_off[bad + 1]:] == whole[w.out_off[bad + 1]:]
    assert rows[k + 1][:8] == ["r", str(k + 1), "0", "0", str(0xffffffff), "-1", "0", "-"] and rows[k + 1][8] == ""
