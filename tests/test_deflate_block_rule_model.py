"""The dynamic-header rule and the argument checks of flate_hip_inflate_one_index on the CPU:
moonbit-flate_amd/csrc/deflate_block_rule.h -- what the discovery kernels compile -- built with g++ into a stand-alone
program under AddressSanitizer and UBSan.  deflate_dyn_header_ok runs at EVERY bit offset of the corpus streams of 20 KB
or less and of every hand-built edge case of deflate_corpus.py (each stream in an allocation of exactly its size), and
at the walker's block starts of the longer streams; it must equal the restatement in tests/one_ref.py, and every
dynamic block the walker reaches must be a hit.  The same program drives the new checks of api_checks.h."""
import os
import struct
import subprocess

import pytest

import deflate_corpus as dc
import one_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "deflate_block_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(CSRC, "deflate_block_rule.h"), os.path.join(CSRC, "api_checks.h"), os.path.join(INC, "flate_hip.h")]
EXE = os.path.join(HERE, "host_model", "deflate_block_rule_model")
INVALID = -1
SMALL = 20000


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC, SRC, "-o", EXE])
    return EXE


@pytest.fixture(scope="module")
def streams(oracle):
    """[(what, raw stream)]: computed once."""
    out = [(w, r) for w, r, _ in ref.good_streams(oracle) + ref.decoy_streams()[::5]]
    legal, _, illegal = ref.history_pair()
    out += [("a distance to the first byte", legal), ("a distance in front of the stream", illegal)]
    out += [("edge case " + c.name, c.data) for c in dc.CASES]
    return out


def run(exe, tmp_path, cases):
    """cases: [(stream, bit offsets or None for all)] -> per case the offsets at which the C++ rule holds."""
    blob = [struct.pack("<I", len(cases))]
    for raw, bits in cases:
        bits = bits or []
        blob.append(struct.pack("<Q", len(raw)) + raw + struct.pack("<Q", len(bits)) + struct.pack("<%dQ" % len(bits), *bits))
    path = tmp_path / "cases.bin"
    path.write_bytes(b"".join(blob))
    lines = subprocess.run([exe, "rule", str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert len(lines) == len(cases) + 1
    return [[int(x) for x in line.split()] for line in lines[:-1]]


def test_rule_equals_the_python_reference(exe, streams, tmp_path):
    cases, want, names = [], [], []
    for what, raw in streams:
        w = ref.Walk(raw)
        dyn = [b[0] for b in w.blocks if b[1] == 2]
        if len(raw) <= SMALL:
            hits = [b for b in ref.candidates(raw) if b or ref.rule(raw, 0)]  # (candidates() always holds bit 0)
            cases.append((raw, None))
        else:
            probe = sorted({b[0] for b in w.blocks} | {b[0] + 1 for b in w.blocks} | {w.end_bit, 8 * len(raw) - 1})
            hits = [b for b in probe if ref.rule(raw, b)]
            cases.append((raw, probe))
        assert set(dyn) <= set(hits), what  # every true header is a candidate, or the chain has holes
        want.append(hits)
        names.append(what)
    got = run(exe, tmp_path, cases)
    for what, g, h in zip(names, got, want):
        assert g == h, what
    # the corpus holds what it is there for: decoys that are hits but no block of the outer stream, and refused headers
    what, raw = streams[[w for w, _ in streams].index("a stream inside a stored block, phase 0")]
    assert len(want[names.index(what)]) > len([b for b in ref.Walk(raw).blocks if b[1] == 2])
    refused = [c.name for c in dc.CASES if len(c.data) > 2 and (c.data[0] >> 1) & 3 == 2 and not ref.rule(c.data, 0)]
    assert len(refused) >= 10, refused


def test_corpus_is_what_the_issue_states(oracle):
    good = ref.good_streams(oracle)
    for what, raw, plain in good:
        w = ref.Walk(raw)
        assert (w.status, w.out_bytes, w.far) == (0, len(plain), False) and len(plain) <= 300000, what
        assert w.unit_bit[0] == 0 and w.unit_bit[1:-1] == [b[0] for b in w.blocks if b[1] == 2 and b[0]], what
    many = ref.Walk(good[ref.MANY_UNITS][1])
    sizes = [b - a for a, b in zip(many.out_off, many.out_off[1:])]
    assert many.n_units >= 100 and max(sizes) < 32768
    assert [ref.Walk(r).n_units for w, r, _ in good if "one unit" in w] == [1, 1]
    types = lambda k: {b[1] for b in ref.Walk(good[k][1]).blocks}
    assert types(5) >= {0, 2} and types(6) >= {0, 2} and types(7) == {1} and types(8) == {0}
    legal, plain, illegal = ref.history_pair()
    a, b = ref.Walk(legal), ref.Walk(illegal)
    assert (a.status, a.far, a.n_units, a.out_bytes) == (0, False, 2, len(plain))
    assert (b.status, b.far, b.n_units) == (0, True, 2)


def test_argument_checks(exe):
    out = subprocess.run([exe, "checks"], check=True, capture_output=True, text=True).stdout
    got = dict((k, int(v)) for k, v in (line.split() for line in out.splitlines()))
    assert got == {
        "index_ok": 0, "index_raw_ok": 0, "index_zlib_ok": 0, "index_wrap_3": INVALID, "index_query_ok": 0,
        "index_one_array": INVALID, "index_other_array": INVALID, "index_no_count": INVALID, "index_no_bytes": INVALID,
        "index_no_status": INVALID, "index_no_in": INVALID, "index_empty_ok": 0, "index_flag_go": INVALID,
        "index_flag_size_only": INVALID,
        "one_ok": 0, "one_query_ok": 0, "one_no_out": INVALID, "one_no_len": INVALID, "one_no_status": INVALID,
        "one_no_in": INVALID, "one_empty_ok": 0, "one_wrap_3": INVALID, "one_flag_go": INVALID,
        "one_flag_size_only": INVALID,
        "round_units_0": 0, "round_units_7": 1, "round_units_65536": 1, "round_units_65537": 0,
        "unit_max_0": 0, "unit_max_1": 1, "unit_max_default": 1, "unit_max_above": 0, "unit_max_negative": 0,
    }
