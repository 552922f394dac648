"""Which members of a gzip file are decoded WHOLE, on the CPU: moonbit-flate_amd/csrc/gzfile_serial_rule.h -- what the
kernels and the library's host code compile -- built with g++ into a stand-alone program under AddressSanitizer and
UBSan (every file in an allocation of exactly its size).  The range end, the whole test, the node record, the hop
behind it and the serial walk must equal tests/gzfile_serial_ref.py's model on every file of the gzfile corpus and on
the mixed file, at S = 1, 19, 20, 64, 1000, 70 000 and 2^28 - 1 and at every member's exact hl + used and one byte
less.  The candidates' size-only decodes are zlib's, handed to both sides."""
import os
import struct
import subprocess

import pytest

import gzfile_ref as ref
import gzfile_serial_ref as sref
from test_gzfile_rule_model import corpus

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "gzfile_serial_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(CSRC, "gzfile_serial_rule.h"), os.path.join(CSRC, "gzfile_rule.h"),
        os.path.join(CSRC, "gzip_rule.h"), os.path.join(CSRC, "api_checks.h"), os.path.join(INC, "flate_hip.h")]
EXE = os.path.join(HERE, "host_model", "gzfile_serial_rule_model")
KINDS = {"end": 0, "dead": 1, "next": 2}
SIZES = (1, 19, 20, 64, 1000, 70000, sref.S_MAX)


def build():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC, SRC, "-o", EXE])
    return EXE


@pytest.fixture(scope="module")
def exe():
    return build()


@pytest.fixture(scope="module")
def cases():
    """[(what, file, S, walk)]: computed once, shared, never changed."""
    files = corpus() + [("the mixed file", sref.mixed_file()[0])]
    out = []
    for what, f in files:
        w = ref.Walk(f)
        sizes = set(SIZES)
        for e in sref.Model(f, sref.S_MAX, w).ends:
            if e is not None:
                sizes |= {e, e - 1}
        out += [(what, f, S, w) for S in sorted(s for s in sizes if s >= 1)]
    return out


def run(exe, cases, tmp_path):
    """cases: [(file, S, [(off, used, z, status)])] -> [(find_from, n_whole, rows)] as the program prints them."""
    blob = [struct.pack("<I", len(cases))]
    for f, S, cand in cases:
        blob.append(struct.pack("<Q", len(f)) + f + struct.pack("<QQ", S, len(cand)))
        blob += [struct.pack("<QQQq", *c) for c in cand]
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(blob))
    out = subprocess.run([exe, "walk", str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    rows = []
    for ln in out.stdout.splitlines():
        head, body = ln.split("|")
        rows.append(tuple(int(x) for x in head.split()) + ([tuple(int(x) for x in r.split(":")) for r in body.split()],))
    assert len(rows) == len(cases)
    return rows


def test_the_rule_and_the_walk_on_every_file_at_every_size(exe, cases, tmp_path):
    tables = {}
    inputs, wants = [], []
    for what, f, S, w in cases:
        offs = tables.setdefault(what, sref.table(f))
        cand, rows = [], []
        for p in offs:
            hl, E, st, used, z = sref.candidate(f, p, S)
            cand.append((p, used, z, st))
            wh = sref.is_whole(p, hl, E, st, used)
            end_bit = 8 * (p + hl + used) if wh else 0
            kind, e, _ = ref.hop(f, end_bit) if wh else ("end", 0, 0)
            rows.append((p, E, p + hl if p + hl <= E else E, int(wh), end_bit, z if wh else 0, KINDS[kind], e))
        inputs.append((f, S, cand))
        wants.append(rows)
    got = run(exe, inputs, tmp_path)
    seen = set()
    for (what, f, S, w), rows, (find_from, n_whole, got_rows) in zip(cases, wants, got):
        assert got_rows == rows, (what, S)
        m = sref.Model(f, S, w)
        assert find_from == m.find_from, (what, S, find_from, m.find_from)
        n = len(f)
        # the whole members the walk passed: the leading run of whole members
        lead = 0
        while lead < w.n_members and m.whole[lead]:
            lead += 1
        assert n_whole == lead, (what, S, n_whole, lead)
        if w.n_members:
            if find_from == n and all(m.whole):
                seen.add("all whole")
            if not any(m.whole) and find_from == 0:
                seen.add("all units")
            if 0 < find_from < n:
                seen.add("find_from inside")
            if any(m.whole[k] and not all(m.whole[:k]) for k in range(w.n_members)):
                seen.add("whole behind long")
        # the collapsed index is the walk's, thinned out
        assert set(m.unit_bit[:-1]) <= set(w.unit_bit[:-1]) and m.n_units <= w.n_units, (what, S)
        assert m.member_unit[-1] == m.n_units and len(m.member_unit) == len(w.member_unit), (what, S)
        assert m.serial_members + m.unit_members == w.n_members, (what, S)
    assert seen == {"all whole", "all units", "find_from inside", "whole behind long"}, seen


def test_a_member_is_whole_exactly_from_its_own_length_on():
    f, _, longs = sref.mixed_file()
    w = ref.Walk(f)
    assert w.status == 0 and w.n_members == 8
    for k in longs:
        assert w.member_unit[k + 1] - w.member_unit[k] >= 3, "a long member of fewer than 3 units"
    ends = sref.Model(f, sref.S_MAX, w).ends
    for k, e in enumerate(ends):
        assert sref.Model(f, e, w).whole[k] and not sref.Model(f, e - 1, w).whole[k], k
    m = sref.Model(f, 4096, w)
    assert m.whole == [k not in longs for k in range(8)] and m.find_from == w.member_off[3]
    assert (m.serial_members, m.unit_members) == (6, 2)
    assert m.n_units == w.n_units and m.unit_bit[:-1] == w.unit_bit[:-1]  # (every short member here is one unit already)
    assert m.unit_bit[-1] == 8 * (len(f) - 8)  # (the last member is whole: the byte-rounded end)
    big = sref.Model(f, sref.S_MAX, w)
    assert all(big.whole) and big.find_from == len(f) and big.n_units == 8
    assert big.unit_bit[-1] == 8 * (len(f) - 8) and big.unit_bit[-1] >= w.unit_bit[-1] > big.unit_bit[-1] - 8
