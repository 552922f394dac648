"""flate_host::BgzfReader and flate_host::BgzfWriter (host/flate_host.hpp): a small g++ driver reads BGZF files through
two small buffers and writes one part by part, on the GPU; tests/bgzf_parts_ref.py says what comes out."""
import gzip
import os
import subprocess

import pytest

import bgzf_parts_ref as R
import bgzf_ref as ref
from util import flate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _compile():
    flate.build()
    exe = os.path.join(HERE, "host_cpp", "bgzf_parts_driver")
    src = os.path.join(HERE, "host_cpp", "bgzf_parts_driver.cpp")
    libdir = os.path.join(ROOT, "moonbit-flate_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", src, "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "moonbit-flate_amd", "host"), "-L" + libdir,
                           "-lflate_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    return exe


def test_the_driver_compiles_without_gpu():
    assert os.path.exists(_compile())


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return dict(ln.split(" ", 1) for ln in out.stdout.splitlines())


FILES = [("many members", ref.many_members(65)[0]), ("a flipped CRC", dict((w, f) for w, f, _, _ in ref.failing_files())["a flipped CRC"]),
         ("garbage behind", dict((w, f) for w, f, _, _ in ref.malformed_files())["5 bytes of garbage after the last member"])]


@pytest.mark.gpu
@pytest.mark.parametrize("pieces", [(65536, 65536), (1 << 20, 3000)], ids=["64k", "small_out"])
@pytest.mark.parametrize("what,f", FILES, ids=[w for w, _ in FILES])
def test_reader_through_small_buffers(tmp_path, what, f, pieces):
    exe = _compile()
    m = R.ReaderModel(f)
    want = m.read(f, True)  # (every cut gives the same bytes and the same verdict: tests/test_bgzf_parts_ref.py)
    src, dst = tmp_path / "file.gz", tmp_path / "plain.bin"
    src.write_bytes(f)
    lines = _run(exe, "read", src, dst, *pieces)
    assert dst.read_bytes() == want.data
    if want.rc == R.STREAM_END:
        assert lines["end"] == "EOF" and lines["close"] == "none" and lines["marker"] == str(want.eof_marker)
        assert int(lines["members"]) == ref.Walk(f).n_members
    else:
        assert lines["end"] != "EOF" and lines["close"] == "error"
        assert (int(lines["bad_member"]), int(lines["err_off"])) == (want.bad_member, want.err_off)
        assert int(lines["members"]) == want.bad_member
    if pieces[0] == 65536 and len(f) > 3 * 65536:
        assert int(lines["calls"]) >= len(f) // 65536  # it went through the buffers, not around them


@pytest.mark.gpu
@pytest.mark.parametrize("part,chunk", [(65280, 1000), (2 * 65280, 70001)])
def test_writer_part_by_part(tmp_path, oracle, part, chunk):
    exe = _compile()
    data = ref.write_inputs()[3 * 65280 + 5]
    want, off = ref.build_file(oracle, data, 0, 0)
    src, dst = tmp_path / "plain.bin", tmp_path / "file.gz"
    src.write_bytes(data)
    lines = _run(exe, "write", src, dst, 0, part, chunk)
    got = dst.read_bytes()
    assert lines["close"] == "none" and got == want and gzip.decompress(got) == data
    assert (int(lines["blocks"]), int(lines["emitted"])) == (4, len(want))
    # (it went through the parts, not around them: a call whenever `part` bytes are staged, and the final one)
    assert int(lines["calls"]) >= len(data) // part + 1
