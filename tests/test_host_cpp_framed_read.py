"""C++ host mirror (flate_host.hpp) of the framed read call: decompress_batch(..., Wrap::Zlib / Wrap::Gzip) and its
dictionary overload, driven by tests/host_cpp/framed_read_driver.cpp and compared here with the CPU expectations of
tests/framed_read_ref.py (header helpers, the oracle's inflate on the exact payload range, its checksums)."""
import os
import struct
import subprocess
import tempfile

import pytest

from framed_read_ref import NO_DICT, bad_members, dict_batch, expected, make_payloads
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "framed_read_driver")
    src = os.path.join(HERE, "host_cpp", "framed_read_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_framed_read_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


def _run(exe, wrap, dicts, members, caps):
    blob = struct.pack("<II", 1 if wrap == "zlib" else 2, len(dicts)) + \
        b"".join(struct.pack("<I", len(d)) + d for d in dicts)
    blob += struct.pack("<I", len(members)) + b"".join(struct.pack("<II", c, len(m)) + m for c, m in zip(caps, members))
    case = tempfile.NamedTemporaryFile(suffix=".bin", delete=False)
    case.write(blob)
    case.close()
    try:
        out = subprocess.run([exe, case.name], capture_output=True, text=True, timeout=180)
    finally:
        os.unlink(case.name)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = {}
    for ln in out.stdout.splitlines():
        f = ln.split(" ")
        if f[0] == "m":
            rows[int(f[1])] = (int(f[2]), int(f[3]), f[4], bytes.fromhex(f[5]) if len(f) > 5 else b"")
    return rows, out.stdout


def _compare(oracle, rows, wrap, members, slots, dicts):
    assert len(rows) == len(members)
    for i, m in enumerate(members):
        st, eo, want, j = expected(oracle, m, wrap, slots[i], dicts)
        status, used, msg, got = rows[i]
        text = {0: "-", -4: "flate:_corrupt_input_before_offset_%d" % eo, -7: "unexpected_EOF"}.get(st)
        assert (status, used, got) == (st, -1 if j == NO_DICT else j, want), (wrap, i, status, st, used, j)
        if text is not None:
            assert msg == text, (wrap, i, msg, text)
        else:
            assert msg != "-", (wrap, i)


@pytest.mark.gpu
@pytest.mark.parametrize("wrap", ["zlib", "gzip"])
def test_members_read_through_the_cpp_mirror(oracle, wrap):
    exe = _compile()
    cases = bad_members(oracle, wrap, make_payloads())
    members, slots = [m for _, m, _ in cases], [s for _, _, s in cases]
    rows, text = _run(exe, wrap, [], members, slots)
    if wrap == "gzip":  # (the mirror's contract: capacity 0 = the member's ISIZE, its last four bytes)
        slots = [int.from_bytes(m[-4:], "little") if s == 0 and len(m) >= 18 else s for m, s in zip(members, slots)]
    _compare(oracle, rows, wrap, members, slots, None)
    if wrap == "gzip":
        assert "refused" in text  # (gzip has no preset dictionaries)
        # capacity 0 = the member's ISIZE
        good = [(m, s) for what, m, s in cases if what == "good"][:4]
        rows, _ = _run(exe, wrap, [], [m for m, _ in good], [0] * len(good))
        _compare(oracle, rows, wrap, [m for m, _ in good], [s for _, s in good], None)


@pytest.mark.gpu
def test_zlib_members_with_dictionaries_through_the_cpp_mirror(oracle):
    exe = _compile()
    members, slots, dicts = dict_batch(oracle)
    rows, _ = _run(exe, "zlib", dicts, members, slots)
    _compare(oracle, rows, "zlib", members, slots, dicts)
    assert rows[5][0] == -4 and all(rows[i][0] == 0 for i in rows if i != 5)
