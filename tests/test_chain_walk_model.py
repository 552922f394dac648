"""The discovery skeleton's host-compilable parts on the CPU: moonbit-flate_amd/csrc/chain_rule.h -- the link search
and the link rule the kernels of all four discoveries compile -- and carve.h, the helper every call's device arrays
are laid out with, built with g++ into a stand-alone program under AddressSanitizer and UBSan
(tests/host_model/chain_walk_model.cpp).  The search is held against a dictionary, the chain the rule yields against
bgzf_serial_walk and the Python walk on every file of the BGZF corpus, the layout against its own arithmetic."""
import os
import struct
import subprocess

import pytest

import bgzf_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "chain_walk_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("chain_rule.h", "carve.h", "bgzf_rule.h")]
EXE = os.path.join(HERE, "host_model", "chain_walk_model")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, SRC, "-o", EXE])
    return EXE


def test_find_equals_a_dictionary_walk(exe):
    """n = 0, 1, 2 and 1000 strictly rising offsets; want below, between, equal to each, equal to the last, above the
    last; lo from 0 to n: the program compares every answer itself and fails on the first that differs."""
    out = subprocess.run([exe, "find"], check=True, capture_output=True, text=True).stdout.split()
    assert out[0] == "find_ok" and int(out[1]) > 3 * 1000 * 50 and out[2:] == ["tiles_ok", "1"]


def test_the_linked_chain_equals_the_serial_walk_on_every_file(exe, tmp_path):
    corpus = ref.index_corpus()
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<I", len(corpus)) + b"".join(struct.pack("<Q", len(f)) + f for _, f in corpus))
    lines = subprocess.run([exe, "walk", str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(corpus)
    for (what, f), line in zip(corpus, lines):
        head, offs = [part.split() for part in line.split("|")]
        w = ref.Walk(f)
        assert [int(x) for x in head] == [w.rc, w.n_members, w.err_off], what
        assert [int(x) for x in offs] == (w.member_off if w.rc == 0 else []), what


def test_carve_layout(exe):
    """Mixed types and counts, one of them 0: the size pass and the pointer pass agree, every array starts on a
    256-byte boundary in call order, none overlaps the next, and the total is the sum of the rounded sizes."""
    lines = [l.split() for l in subprocess.run([exe, "carve"], check=True, capture_output=True, text=True).stdout.splitlines()]
    arrays, total = lines[:-1], int(lines[-1][1])
    assert [a[0] for a in arrays] == ["head", "bytes", "none", "halves", "recs", "last"] and lines[-1][0] == "total"
    at = 0
    for name, size_off, ptr_off, nbytes, end in arrays:
        assert int(size_off) == int(ptr_off) == at and at % 256 == 0, name  # (the size pass runs over a null base)
        at += (int(nbytes) + 255) // 256 * 256
        assert int(end) == at, name
    assert total == at == 256 + 512 + 0 + 256 + 256 + 8192
