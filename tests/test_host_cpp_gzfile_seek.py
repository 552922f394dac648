"""C++ host mirror (flate_host.hpp) of flate_hip_gzfile_seek_index and flate_hip_gzfile_ranges: seek_index_gzfile and
decompress_gzfile_ranges, driven by tests/host_cpp/gzfile_seek_driver.cpp on files of the corpus and compared here with
tests/gzfile_seek_ref.py (the model) and zlib's bytes."""
import os
import struct
import subprocess
import tempfile

import pytest

import gzfile_ref as gzf
import gzfile_seek_ref as R
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xffffffff


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "gzfile_seek_driver")
    src = os.path.join(HERE, "host_cpp", "gzfile_seek_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_gzfile_seek_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_build_and_read_through_the_cpp_mirror():
    exe = _compile()
    f, plain = R.seek_file()
    w = gzf.Walk(f)
    T = len(plain)
    e = w.out_off[w.member_unit[2]]  # the empty member
    ranges = [(0, 10), (T - 5, T + 100), (100000, 100000), (150000, 190000), (7, 9), (e - 9, e + 9), (2990, 3010)]
    tiny, tiny_plain = gzf.tiny_file()
    cut = f[:w.member_off[1] + (w.member_off[2] - w.member_off[1]) // 2]
    cases = [(4096, f, plain, ranges), (100000, f, plain, ranges[::-1]), (R.SPAN_NONE, tiny, tiny_plain, [(0, len(tiny_plain))]),
             (4096, cut, plain, [(0, 10)])]
    blob = struct.pack("<I", len(cases))
    for span, ff, p, rg in cases:
        blob += struct.pack("<QQ", span, len(ff)) + ff + struct.pack("<I", len(rg))
        blob += struct.pack("<%dQ" % len(rg), *[b for b, _ in rg]) + struct.pack("<%dQ" % len(rg), *[e for _, e in rg])
    case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
    case.write(blob)
    case.close()
    try:
        out = subprocess.run([exe, case.name], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(case.name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 2 * len(cases)
    for k, (span, ff, p, rg) in enumerate(cases[:3]):
        wk = gzf.Walk(ff)
        pts = R.points(wk, span)
        head, words = [part.split() for part in lines[2 * k].split("|")]
        assert head == ["s", str(k), "0", str(wk.n_units), str(wk.n_members), str(len(pts)), str(len(p)),
                        str(R.windows_bytes(wk, span)), str(NONE), "-1", "-1", "-"], head
        assert [int(x) for x in words] == R.index_words(wk, len(ff), span), k
        m = R.read(wk, p, pts, [b for b, _ in rg], [e for _, e in rg])
        head, off, status, data = [part.split() for part in lines[2 * k + 1].split("|")]
        assert head == ["r", str(k), "0", str(m[3]), str(NONE), "-"], head
        assert [int(x) for x in off] == m[1] and [int(x) for x in status] == m[2], k
        assert bytes.fromhex(data[0] if data else "") == b"".join(m[5]), k
    # a file that is cut short: the walk's verdict, no index, and a read that is refused
    wc = gzf.Walk(cut)
    head, words = [part.split() for part in lines[6].split("|")]
    assert head[:3] == ["s", "3", str(gzf.UNEXPECTED_EOF)] and words == []
    assert head[5:] == ["0", "0", "0", str(wc.bad_member), str(wc.err_off), str(wc.stream_err_off), "unexpected_EOF"], head
    head = lines[7].split("|")[0].split()
    assert head[:3] == ["r", "3", "-1"]
