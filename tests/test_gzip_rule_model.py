"""The gzip member rule, the walk and the argument checks on the CPU: moonbit-flate_amd/csrc/gzip_rule.h -- what the
discovery kernels, frame_parse_kernel and the library's host code compile -- built with g++ into a stand-alone program
under AddressSanitizer and UBSan.  gzip_header_len runs at EVERY offset of every corpus file (each in an allocation of
exactly its size) and gzip_serial_walk on the candidate tables that tests/gzip_ref.py makes with zlib; both must equal
gzip_ref.  The same program drives the gzip checks of api_checks.h."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import gzip_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "gzip_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(CSRC, "gzip_rule.h"), os.path.join(CSRC, "api_checks.h"), os.path.join(INC, "flate_hip.h")]
EXE = os.path.join(HERE, "host_model", "gzip_rule_model")
INVALID = -1


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC, SRC, "-o", EXE])
    return EXE


def own_output_file(oracle):
    """Members as flate_hip_deflate_fast_batch_framed(FLATE_HIP_WRAP_GZIP) writes them, around the oracle's streams."""
    parts = [ref.text(n, seed=40 + n % 7) for n in (0, 1, 17, 5552, 70000)]
    f = b"".join(ref.own_member(oracle.deflate(np.frombuffer(p, np.uint8)), p) for p in parts)
    return "our own gzip members concatenated", f, b"".join(parts)


@pytest.fixture(scope="module")
def cases(oracle):
    """[(what, file, member_max)]: every file of the corpus."""
    out = [(w, f, ref.MEMBER_MAX) for w, f, _ in ref.good_files() + [own_output_file(oracle)]]
    out += [(w, f, ref.MEMBER_MAX) for w, f, _, _ in ref.decoy_files()]
    out += [(w, f, m) for w, f, m, _, _, _ in ref.malformed_files()]
    out += [(w, f, ref.MEMBER_MAX) for w, f, _, _ in ref.failing_files()]
    out += [("empty", b"", ref.MEMBER_MAX), ("every file under gzip_member_max 64", ref.good_files()[3][1], 64)]
    return out


def test_rule_and_walk_equal_the_python_reference_on_every_file(exe, cases, tmp_path):
    blob = [struct.pack("<I", len(cases))]
    walks = []
    for _, f, m in cases:
        w = ref.Walk(f, m)
        walks.append(w)
        blob.append(struct.pack("<QQ", m, len(f)) + f + struct.pack("<Q", len(w.table)))
        blob += [struct.pack("<QqQQ", *c) for c in w.table]
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(blob))
    lines = subprocess.run([exe, "walk", str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(cases)
    for (what, f, m), w, line in zip(cases, walks, lines):
        head, moff, ooff, rule = [part.split() for part in line.split("|")]
        assert [int(x) for x in head] == [w.rc, w.n_members, w.err_off], what
        assert [int(x) for x in moff] == w.member_off and [int(x) for x in ooff] == w.out_off, what
        want = {p: ref.header_len(f, p, ref.range_end(p, len(f), m)) for p in range(len(f))}
        assert {int(a): int(b) for a, b in (x.split(":") for x in rule)} == {p: h for p, h in want.items() if h}, what
        assert sorted(c[0] for c in w.table) == sorted(p for p, h in want.items() if h), what


def test_corpus_has_the_stated_verdicts(oracle):
    """The Python reference alone: the corpus is what the issue says it is, and zlib's own gzip reader agrees."""
    for what, f, plain in ref.good_files() + [own_output_file(oracle)]:
        w = ref.Walk(f)
        assert (w.rc, w.err_off, w.out_bytes) == (0, -1, len(plain)) and ref.plain_of(f) == plain, what
        assert w.member_off[-1] == len(f) and w.n_candidates >= w.n_members, what
    assert [ref.Walk(f).n_members for _, f, _ in ref.good_files()[:5]] == ref.MEMBER_COUNTS
    for what, f, plain, more in ref.decoy_files():
        w = ref.Walk(f)
        assert w.rc == 0 and ref.plain_of(f) == plain and w.out_bytes == len(plain), what
        assert (w.n_candidates > w.n_members) == more, what
    # the decoys are what they claim: one decodes cleanly and has a successor, one reaches the end of the file
    what, f, _, _ = ref.decoy_files()[0]
    w = ref.Walk(f)
    inner = [c for c in w.table if c[0] not in w.member_off and c[1] == 0]
    assert len(inner) == 2 and inner[0][0] + ref.header_len(f, inner[0][0], len(f)) + inner[0][2] + 8 == inner[1][0], what
    what, f, _, _ = ref.decoy_files()[1]
    w = ref.Walk(f)
    inner = [c for c in w.table if c[0] not in w.member_off and c[1] == 0]
    assert len(inner) == 1 and inner[0][0] + ref.header_len(f, inner[0][0], len(f)) + inner[0][2] + 8 == len(f), what
    for what, f, m, rc, err_off, n in ref.malformed_files():
        w = ref.Walk(f, m)
        assert (w.rc, w.err_off, w.n_members, w.out_bytes) == (rc, err_off, n, 0), what
        assert len(w.member_off) == n + 1 and w.member_off[-1] == err_off, what
        if m == ref.MEMBER_MAX:
            with pytest.raises(zlib.error):
                ref.plain_of(f)
    for what, f, rc, bad in ref.failing_files():
        w = ref.Walk(f)
        assert w.rc == 0 and w.n_members == 3, what  # (the chain is sound: the failure is a member's)
        with pytest.raises(zlib.error):
            ref.plain_of(f)
    assert ref.Walk(b"").n_members == 0 and ref.Walk(b"").rc == 0
    assert len(ref.malformed_files()[9][1]) == 17


def test_argument_checks(exe):
    out = subprocess.run([exe, "checks"], check=True, capture_output=True, text=True).stdout
    got = dict((k, int(v)) for k, v in (line.split() for line in out.splitlines()))
    assert got == {
        "index_ok": 0, "index_query_ok": 0, "index_one_array": INVALID, "index_other_array": INVALID,
        "index_no_count": INVALID, "index_no_bytes": INVALID, "index_no_in": INVALID, "index_empty_ok": 0,
        "index_flag_go": INVALID, "index_flag_size_only": INVALID,
        "read_ok": 0, "read_no_out_no_cap_ok": 0, "read_no_out": INVALID, "read_no_len": INVALID, "read_no_in": INVALID,
        "read_empty_ok": 0, "read_flag_size_only": INVALID,
        "member_max_0": 0, "member_max_1": 1, "member_max_4096": 1, "member_max_default": 1, "member_max_2_28": 0,
        "member_max_negative": 0,
        "dead_eof_unclipped": ref.UNEXPECTED_EOF, "dead_eof_clipped": ref.TOO_LARGE,
        "dead_eof_at_the_edge": ref.UNEXPECTED_EOF, "dead_corrupt_clipped": ref.CORRUPT, "dead_four_gib": ref.TOO_LARGE,
    }
