"""C++ host mirror (flate_host.hpp) of flate_hip_inflate_one_seek_index and flate_hip_inflate_one_ranges:
seek_index_one and decompress_one_ranges, driven by tests/host_cpp/one_seek_driver.cpp on streams of the corpus and
compared here with tests/seek_ref.py (the model) and zlib's bytes."""
import os
import struct
import subprocess
import tempfile

import pytest

import one_ref as ref
import seek_ref as sk
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "one_seek_driver")
    src = os.path.join(HERE, "host_cpp", "one_seek_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_one_seek_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_build_and_read_through_the_cpp_mirror():
    exe = _compile()
    streams = ref.good_streams()
    _, raw, plain = streams[ref.MANY_UNITS]
    w = ref.Walk(raw)
    T = len(plain)
    cut = raw[:(w.unit_bit[9] + w.unit_bit[10]) // 16]
    ranges = [(0, 10), (T - 5, T + 100), (100000, 100000), (150000, 190000), (7, 9)]
    cases = [(ref.GZIP, 4096, raw, plain, ranges), (ref.RAW, 100000, raw, plain, ranges[::-1]),
             (ref.ZLIB, sk.SPAN_NONE, streams[6][1], streams[6][2], [(0, len(streams[6][2]))]),
             (ref.ZLIB, 4096, cut, plain, [(0, 10)])]
    blob = struct.pack("<I", len(cases))
    for kind, span, r, p, rg in cases:
        f = ref.wrap(r, p, kind)
        blob += struct.pack("<IQQ", kind, span, len(f)) + f + struct.pack("<I", len(rg))
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
    for k, (kind, span, r, p, rg) in enumerate(cases[:3]):
        wk = ref.Walk(r)
        pts = sk.points(wk.out_off, span)
        head, words = [part.split() for part in lines[2 * k].split("|")]
        assert head == ["s", str(k), "0", str(wk.n_units), str(len(pts)), str(len(p)), str((len(pts) - 1) * sk.WINDOW), "-"]
        assert [int(x) for x in words] == sk.index_words(wk, p, len(r), kind, span), k
        m = sk.read(p, wk.out_off, pts, [b for b, _ in rg], [e for _, e in rg])
        head, off, status, data = [part.split() for part in lines[2 * k + 1].split("|")]
        assert head == ["r", str(k), "0", str(m[3]), str(sk.NO_UNIT), "-"], head
        assert [int(x) for x in off] == m[1] and [int(x) for x in status] == m[2], k
        assert bytes.fromhex(data[0] if data else "") == b"".join(m[5]), k
    # a stream that is cut short: the serial verdict, no index, and a read that is refused
    head, words = [part.split() for part in lines[6].split("|")]
    assert head[:3] == ["s", "3", str(ref.UNEXPECTED_EOF)] and head[4:] == ["0", "0", "0", "unexpected_EOF"] and words == []
    head = lines[7].split("|")[0].split()
    assert head[:3] == ["r", "3", "-1"]
