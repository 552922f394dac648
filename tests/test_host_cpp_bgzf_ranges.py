"""C++ host mirror (flate_host.hpp) of BGZF random access: decompress_bgzf_ranges, driven by
tests/host_cpp/bgzf_ranges_driver.cpp on files of the corpus and compared here with the Python model
(tests/bgzf_range_ref.py) and gzip's own reader."""
import gzip
import os
import struct
import subprocess
import tempfile

import pytest

import bgzf_range_ref as model
import bgzf_ref as ref
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "bgzf_ranges_driver")
    src = os.path.join(HERE, "host_cpp", "bgzf_ranges_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_bgzf_ranges_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


def _run(exe, cases):
    blob = struct.pack("<I", len(cases))
    for virt, f, ranges in cases:
        blob += struct.pack("<IQ", virt, len(f)) + f + struct.pack("<I", len(ranges))
        blob += struct.pack("<%dQ" % len(ranges), *[b for b, _ in ranges]) + struct.pack("<%dQ" % len(ranges), *[e for _, e in ranges])
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
def test_ranges_through_the_cpp_mirror():
    exe = _compile()
    f, plain = ref.many_members(65)
    w = ref.Walk(f)
    T = len(plain)
    byte_ranges = [(0, 10), (T - 5, T + 5), (100, 70000), (7, 7), (0, T)]
    k = next(k for k in range(w.n_members) if w.out_off[k + 1] - w.out_off[k] > 20)
    v = w.member_off[k] << 16
    virt_ranges = [(v | 2, v | 20), ((w.member_off[k] + 1) << 16, (w.member_off[k] + 1) << 16), (0, len(f) << 16)]
    (w1, bad1, e1, n1), (w2, bad2, rc2, m2) = ref.malformed_files()[1], ref.failing_files()[3]
    wb = ref.Walk(bad2)
    fail_ranges = [(0, 50), (wb.out_off[m2] + 1, wb.out_off[m2] + 9), (wb.out_off[m2 + 1], wb.out_off[m2 + 1] + 30)]
    cases = [(0, f, byte_ranges), (1, f, virt_ranges), (0, bad1, [(0, 9)]), (0, bad2, fail_ranges), (0, bad2, fail_ranges[::2]),
             (0, b"", [(0, 4)]), (0, f, [])]
    rows = _run(exe, cases)
    assert len(rows) == len(cases)
    status = {m2: rc2}
    messages = {0: "-", 1: None, 2: "flate:_corrupt_input_before_offset_%d" % e1, 3: "unexpected_EOF", 4: "-", 5: "-", 6: "-"}
    for i, (virt, ff, ranges) in enumerate(cases):
        R = model.read_ranges(ff, virt, [b for b, _ in ranges], [e for _, e in ranges], status=status if ff is bad2 else None)
        row = rows[i]
        assert [int(x) for x in row[:6]] == [i, R.rc, R.n_members, R.n_decoded, R.bad_member, R.err_off], (i, row[:6])
        assert [int(x) for x in row[6].split(",")] == R.out_off, i
        assert (row[7] == "-" and not ranges) or [int(x) for x in row[7].split(",")] == R.range_status, i
        if messages[i] is not None:
            assert row[8] == messages[i], (i, row[8])
        got = bytes.fromhex(row[9]) if len(row) > 9 else b""
        if R.rc == ref.CORRUPT and R.bad_member == R.n_members:
            assert got == b"", i  # a malformed chain: nothing delivered
            continue
        assert len(got) == R.out_off[-1], i
        for r in range(len(ranges)):
            if R.exact[r]:
                assert got[R.out_off[r]:R.out_off[r + 1]] == R.data[R.out_off[r]:R.out_off[r + 1]], (i, r)
    assert rows[1][1] == "-1" and rows[0][9] != ""
    assert bytes.fromhex(rows[0][9])[-T:] == gzip.decompress(f)
