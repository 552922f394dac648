"""C++ host mirror (flate_host.hpp) of the framed encode calls: compress_batch(..., Wrap) with and without a
DictTable and compress_spliced(..., Wrap), driven by tests/host_cpp/framed_driver.cpp and compared here, byte for
byte, with the CPU recipes: the oracle's raw stream inside the oracle's frame, and for dictionary members
zlib_dict_header + tests/deflate_dict_ref.py + Adler-32."""
import gzip
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

from deflate_dict_ref import deflate_dict
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
NO_DICT = 0xFFFFFFFF
engine = __import__("importlib").import_module("moonbit-flate_amd.engine")


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "framed_driver")
    src = os.path.join(HERE, "host_cpp", "framed_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_framed_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


@pytest.mark.gpu
@pytest.mark.parametrize("compat_go", [False, True])
def test_members_and_spliced_members_through_the_cpp_mirror(oracle, compat_go):
    exe = _compile()
    compat = 1 if compat_go else 0
    words = lambda seed, n: flate.synth("text", 1, n, seed=seed).tobytes() if n else b""
    dicts = [words(61, 40000), words(62, 900), b"", words(63, 16)]
    streams = []  # (dictionary index or NO_DICT, payload)
    for k in range(12):
        j = [0, 1, 2, NO_DICT, 3][k % 5]
        n = [3000, 100, 70000, 0, 4096, 131070][k % 6]
        d = dicts[j] if j != NO_DICT else b""
        streams.append((j, (d[-300:] + words(70 + k, n))[:n]))
    blob = struct.pack("<II", compat, len(dicts)) + b"".join(struct.pack("<I", len(d)) + d for d in dicts)
    blob += struct.pack("<I", len(streams)) + b"".join(struct.pack("<II", j, len(p)) + p for j, p in streams)
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
        if f[0] in ("r", "z", "g", "d"):
            rows[(f[0], int(f[1]))] = bytes.fromhex(f[2]) if len(f) > 2 else b""
        elif f[0] in ("sz", "sg"):
            rows[f[0]] = bytes.fromhex(f[1])
    for i, (j, p) in enumerate(streams):
        raw = oracle.deflate(p, compat=compat)
        assert rows[("r", i)] == raw, i
        assert rows[("z", i)] == oracle.frame(oracle.FRAME_ZLIB, raw, p), i
        assert rows[("g", i)] == oracle.frame(oracle.FRAME_GZIP, raw, p), i
        assert zlib.decompress(rows[("z", i)]) == p and gzip.decompress(rows[("g", i)]) == p
        if j == NO_DICT:
            want = oracle.frame(oracle.FRAME_ZLIB, raw, p)
            o = zlib.decompressobj()
        else:
            want = engine.zlib_dict_header(dicts[j]) + deflate_dict(p, dicts[j], compat) + \
                zlib.adler32(p).to_bytes(4, "big")
            o = zlib.decompressobj(zdict=dicts[j])
        assert rows[("d", i)] == want, i
        assert o.decompress(rows[("d", i)]) == p and o.eof
    payloads = [p for _, p in streams]
    whole = b"".join(payloads)
    off = np.zeros(len(payloads) + 1, np.uint64)
    np.cumsum(np.array([len(p) for p in payloads], dtype=np.uint64), out=off[1:])
    one, _ = oracle.deflate_spliced(np.frombuffer(whole + b"\0", np.uint8), off, compat=compat)
    assert rows["sz"] == oracle.frame(oracle.FRAME_ZLIB, one, whole)
    assert rows["sg"] == oracle.frame(oracle.FRAME_GZIP, one, whole)
    assert zlib.decompress(rows["sz"]) == whole and gzip.decompress(rows["sg"]) == whole
    assert "bits %d" % (len(payloads) + 1) in out.stdout
