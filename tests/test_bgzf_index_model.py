"""The BGZF member rule and argument checks on the CPU: moonbit-flate_amd/csrc/bgzf_rule.h -- the one function the
discovery kernels and the library's host code compile -- built with g++ into a stand-alone program under
AddressSanitizer and UBSan, run over every file of the corpus (each in an allocation of exactly its size) and compared
with the serial walk of tests/bgzf_ref.py, at offset 0 and at EVERY offset.  The same program drives the BGZF checks
of api_checks.h."""
import os
import struct
import subprocess

import pytest

import bgzf_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "bgzf_index_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(CSRC, "bgzf_rule.h"), os.path.join(CSRC, "api_checks.h"), os.path.join(INC, "flate_hip.h")]
EXE = os.path.join(HERE, "host_model", "bgzf_index_model")
INVALID, TOO_LARGE = -1, -6


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC, SRC, "-o", EXE])
    return EXE


@pytest.fixture(scope="module")
def corpus():
    return ref.index_corpus()


def test_rule_and_walk_equal_the_python_walk_on_every_file(exe, corpus, tmp_path):
    blob = struct.pack("<I", len(corpus)) + b"".join(struct.pack("<Q", len(f)) + f for _, f in corpus)
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    lines = subprocess.run([exe, "walk", str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(corpus)
    for (what, f), line in zip(corpus, lines):
        head, offs, rule = [part.split() for part in line.split("|")]
        w = ref.Walk(f)
        assert [int(x) for x in head] == [w.rc, w.n_members, w.err_off, w.eof_marker, w.out_bytes], what
        assert [int(x) for x in offs] == (w.member_off if w.rc == 0 else []), what
        want = {p: ref.member_total(f, p) for p in range(len(f))}
        assert {int(a): int(b) for a, b in (x.split(":") for x in rule)} == {p: t for p, t in want.items() if t}, what


def test_corpus_has_the_stated_verdicts():
    for what, f, err_off, n in ref.malformed_files():
        w = ref.Walk(f)
        assert (w.rc, w.err_off, w.n_members, w.out_bytes) == (ref.CORRUPT, err_off, n, 0), what
    for what, f in ref.header_files() + ref.decoy_files():
        assert ref.Walk(f).rc == 0, what
    for what, f, _, _ in ref.failing_files():
        assert ref.Walk(f).rc == 0, what  # (the chain is fine: the failure is a member's)
    assert ref.Walk(ref.header_files()[4][1]).eof_marker == 0 and ref.header_files()[4][0] == "no EOF marker"
    assert ref.Walk(ref.EOF).eof_marker == 1 and ref.Walk(b"").n_members == 0


def test_argument_checks(exe):
    out = subprocess.run([exe, "checks"], check=True, capture_output=True, text=True).stdout
    got = dict((k, int(v)) for k, v in (line.split() for line in out.splitlines()))
    bound = lambda n: 2 * n + 400 + 26  # (bound_model of the program, inside 18 + 8 bytes)
    assert got == {
        "block_default": 65280, "block_1": 1, "block_65535": 65535, "block_65536": 0,
        "blocks_0": 0, "blocks_65280": 1, "blocks_65281": 2,
        "bound_0": 28, "bound_1": bound(1) + 28, "bound_tail": 2 * bound(4096) + bound(5) + 28, "bound_refused": 0,
        "write_ok": 0, "write_empty_ok": 0, "write_no_in": INVALID, "write_no_out": INVALID, "write_no_len": INVALID,
        "write_block_65536": INVALID, "write_flag_size_only": INVALID, "write_too_many_blocks": TOO_LARGE,
        "write_most_blocks": 0,
        "index_ok": 0, "index_query_ok": 0, "index_one_array": INVALID, "index_other_array": INVALID,
        "index_no_count": INVALID, "index_no_bytes": INVALID, "index_no_in": INVALID, "index_empty_ok": 0,
        "index_flag_go": INVALID,
        "read_ok": 0, "read_no_out_no_cap_ok": 0, "read_no_out": INVALID, "read_no_len": INVALID, "read_no_in": INVALID,
        "read_flag_size_only": INVALID,
        "first_cap_0": 4096, "first_cap_1m": 4096 + 1024,
        "rounds_0": 1, "rounds_2": 2, "rounds_3": 3, "rounds_4094": 12, "rounds_4095": 13,
    }
