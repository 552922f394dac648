"""C++ host mirror (flate_host.hpp) of flate_hip_inflate_one_index and flate_hip_inflate_one: index_one and
decompress_one, driven by tests/host_cpp/one_driver.cpp
on streams of the corpus and compared here with tests/one_ref.py (the bit-level block walker)."""
import os
import struct
import subprocess
import tempfile

import pytest

import one_ref as ref
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "one_driver")
    src = os.path.join(HERE, "host_cpp", "one_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_one_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_index_through_the_cpp_mirror():
    exe = _compile()
    streams = ref.good_streams()
    _, raw, plain = streams[ref.MANY_UNITS]
    w = ref.Walk(raw)
    cut = raw[:(w.unit_bit[9] + w.unit_bit[10]) // 16]
    flipped = bytearray(raw)
    flipped[(w.unit_bit[4] + 20) >> 3] ^= 1 << ((w.unit_bit[4] + 20) & 7)
    cases = [(ref.GZIP, raw, plain), (ref.RAW, streams[6][1], streams[6][2]), (ref.ZLIB, cut, plain),
             (ref.RAW, bytes(flipped), plain)]
    blob = struct.pack("<I", len(cases) + 1)
    blob += b"".join(struct.pack("<IQ", k, len(ref.wrap(r, p, k))) + ref.wrap(r, p, k) for k, r, p in cases)
    blob += struct.pack("<IQ", ref.GZIP, 5) + b"\x1f\x8b\x08\x00\x00"
    case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
    case.write(blob)
    case.close()
    try:
        out = subprocess.run([exe, case.name], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(case.name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [[part.split() for part in ln.split("|")] for ln in out.stdout.splitlines()]
    assert len(rows) == len(cases) + 1
    msgs = {0: "-", ref.CORRUPT: "flate:_corrupt_input_before_offset_%d", ref.UNEXPECTED_EOF: "unexpected_EOF"}
    for k, (kind, r, p) in enumerate(cases):
        w = ref.Walk(r)
        head, ubit, ooff = rows[k]
        msg = msgs[w.status] % w.err_off if "%" in msgs[w.status] else msgs[w.status]
        assert head[:6] == ["r", str(k), str(w.status), str(w.n_units), str(w.out_bytes), str(w.err_off)], head
        assert int(head[6]) >= max(w.n_units, 1) and head[7] == msg, head
        assert [int(x) for x in ubit] == w.unit_bit and [int(x) for x in ooff] == w.out_off, k
    assert [ref.Walk(r).status for _, r, _ in cases] == [0, 0, ref.UNEXPECTED_EOF, ref.CORRUPT]
    head, ubit, ooff = rows[-1]  # a header that is too short: corrupt at offset 0, no units
    assert head[2:] == [str(ref.CORRUPT), "0", "0", "0", "0", msgs[ref.CORRUPT] % 0] and ubit == ["0"] and ooff == ["0"]


@pytest.mark.gpu
def test_read_through_the_cpp_mirror():
    exe = _compile()
    streams = ref.good_streams()
    _, raw, plain = streams[ref.MANY_UNITS]
    small = streams[9]
    w = ref.Walk(raw)
    cut = raw[:(w.unit_bit[9] + w.unit_bit[10]) // 16]
    wrong = bytearray(ref.wrap(small[1], small[2], ref.GZIP))
    wrong[-6] ^= 1
    files = [(ref.GZIP, ref.wrap(raw, plain, ref.GZIP)), (ref.RAW, small[1]), (ref.ZLIB, ref.wrap(cut, plain, ref.ZLIB)),
             (ref.GZIP, bytes(wrong)), (ref.GZIP, b"\x1f\x8b\x08\x00\x00")]
    blob = struct.pack("<I", len(files)) + b"".join(struct.pack("<IQ", k, len(f)) + f for k, f in files)
    case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
    case.write(blob)
    case.close()
    try:
        out = subprocess.run([exe, case.name, "read"], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(case.name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = [ln.split(" ") for ln in out.stdout.splitlines()]
    assert len(rows) == len(files)
    assert rows[0][:5] == ["d", "0", "0", str(w.n_units), "-1"] and rows[0][6] == "-" and bytes.fromhex(rows[0][7]) == plain
    assert rows[1][:5] == ["d", "1", "0", "1", "-1"] and bytes.fromhex(rows[1][7]) == small[2]
    wc = ref.Walk(cut)
    assert rows[2][:5] == ["d", "2", str(ref.UNEXPECTED_EOF), str(wc.n_units), "-1"] and rows[2][6] == "unexpected_EOF"
    assert bytes.fromhex(rows[2][7]) == plain[:wc.out_len] and wc.out_len > wc.out_off[-1]
    assert rows[3][:5] == ["d", "3", str(ref.CORRUPT), "1", str(len(wrong))] and bytes.fromhex(rows[3][7]) == small[2]
    assert rows[3][6] == "flate:_corrupt_input_before_offset_%d" % len(wrong)
    assert rows[4][:5] == ["d", "4", str(ref.CORRUPT), "0", "0"] and rows[4][7] == ""
