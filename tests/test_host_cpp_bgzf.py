"""C++ host mirror (flate_host.hpp) of the BGZF calls: compress_bgzf and decompress_bgzf, driven by
tests/host_cpp/bgzf_driver.cpp on files of the corpus and compared here with tests/bgzf_ref.py (the reference file,
the serial walk) and gzip's own reader."""
import gzip
import os
import struct
import subprocess
import tempfile

import pytest

import bgzf_ref as ref
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "bgzf_driver")
    src = os.path.join(HERE, "host_cpp", "bgzf_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_bgzf_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


def _run(exe, cases):
    blob = struct.pack("<I", len(cases)) + b"".join(struct.pack("<IIIQ", k, bb, fl, len(d)) + d for k, bb, fl, d in cases)
    case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
    case.write(blob)
    case.close()
    try:
        out = subprocess.run([exe, case.name], capture_output=True, text=True, timeout=180)
    finally:
        os.unlink(case.name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return [ln.split(" ") for ln in out.stdout.splitlines()]


@pytest.mark.gpu
def test_round_trip_and_read_through_the_cpp_mirror(oracle):
    exe = _compile()
    inputs = ref.write_inputs()
    data = [inputs[0], inputs[65281], inputs[3 * 65280 + 5]]
    foreign = [f for _, f in ref.header_files()[:3]]
    (w1, bad1, e1, n1), (w2, bad2, rc2, m2) = ref.malformed_files()[1], ref.failing_files()[3]
    cases = [(0, 0, 0, data[0]), (0, 4096, 2, data[1]), (0, 0, 0, data[2])] + [(1, 0, 0, f) for f in foreign] + \
        [(1, 0, 0, bad1), (1, 0, 0, bad2)]
    rows = _run(exe, cases)
    assert len(rows) == len(cases)
    for k, (d, bb, compat) in enumerate(((data[0], 0, 0), (data[1], 4096, 1), (data[2], 0, 0))):
        want, off = ref.build_file(oracle, d, bb, compat)
        assert rows[k][:2] == ["w", str(k)] and bytes.fromhex(rows[k][2]) == want, k
        assert [int(x) for x in rows[k][3].split(",")] == [int(x) for x in off] and rows[k][4] == "1", k
    for k, f in enumerate(foreign, start=3):
        w = ref.Walk(f)
        assert rows[k][:8] == ["r", str(k), "0", str(w.n_members), str(0xffffffff), "-1", str(w.eof_marker), "-"], rows[k][:8]
        assert bytes.fromhex(rows[k][8]) == gzip.decompress(f)
    # a malformed chain: where no member could be read, nothing delivered
    assert rows[6][:8] == ["r", "6", "-4", str(n1), str(n1), str(e1), "0", "flate:_corrupt_input_before_offset_%d" % e1]
    assert rows[6][8] == ""
    # a member whose raw stream is cut short: the others are delivered
    w = ref.Walk(bad2)
    assert rows[7][:8] == ["r", "7", str(rc2), str(w.n_members), str(m2), str(w.member_off[m2]), "1", "unexpected_EOF"]
    got, whole = bytes.fromhex(rows[7][8]), ref.text(6000, seed=6)  # (what failing_files cuts its blocks from)
    assert len(got) == w.out_bytes and got[:w.out_off[m2]] == whole[:w.out_off[m2]] and \
        got[w.out_off[m2 + 1]:] == whole[w.out_off[m2 + 1]:]
